"""numpy complex128 restatement of the weight of a connected leafless configuration with two independent loops (reference
src/MessagePassing/loopcorrection.jl:79-89), FACTORED the way the device contracts it, sharing no code with the package (it imports tests/loop_ref.py only).

  decompose        internal degrees -> shape ("cycle", "theta", "dumbbell", "eight"), branch vertices (internal degree >= 3) and chains: maximal paths
                   [p_0 (branch), p_1 .. p_n (internal degree 2), p_{n+1} (branch)], n >= 0.  Canonical: vertices by position in the graph, a chain is walked
                   from the lower branch vertex, towards its neighbours in ascending order.  theta: three chains u -> w; dumbbell: closed chain on u, closed
                   chain on w, bridge u -> w (in this order); eight: two closed chains.  cycle: the ring from the lowest vertex towards its lower ring neighbour.
  factors          the factor matrices: per branch vertex its double-layer tensor B[x_0, x_1, ..] over its slots (x = ket + chi * bra; slot order: the chains'
                   ends in chain order, a closed chain's first leg before its last), per inner vertex A_k T_k (the ring matrices of loop_ref.cycle_matrices for
                   the open chain), per chain the antiprojector A_0 of its first edge as a matrix.
  weight           the weight from these factors through matmul / dot (BLAS), never a general einsum over the configuration
  bound            8 u S k_max prod ||F_i||_F over the S factor matrices F_i; k_max = the longest contraction of the restatement = the largest dimension of any
                   factor seen as a matrix (a branch tensor as (all slots but the last) x (last slot)); the plain norms, except where a factor cancels to 0 (see bound)."""
import numpy as np

import loop_ref as lr

EPS = 2.0 ** -53


def decompose(graph, edges):
    pos = graph.pos
    es = sorted({tuple(sorted(e, key=pos.__getitem__)) for e in edges}, key=lambda e: (pos[e[0]], pos[e[1]]))
    nb = {}
    for (a, b) in es:
        nb.setdefault(a, []).append(b); nb.setdefault(b, []).append(a)
    verts = sorted(nb, key=pos.__getitem__)
    for v in verts:
        nb[v].sort(key=pos.__getitem__)
    assert len(es) == len(edges) and min(len(x) for x in nb.values()) >= 2 and len(lr.components(es)) == 1
    loops = len(es) - len(verts) + 1
    if loops == 1:
        ring, prev, cur = [verts[0]], verts[0], nb[verts[0]][0]
        while cur != verts[0]:
            ring.append(cur)
            prev, cur = cur, [w for w in nb[cur] if w != prev][0]
        return dict(shape="cycle", ring=ring, branch=[], chains=[])
    if loops != 2:
        return dict(shape=None, loops=loops)
    branch = [v for v in verts if len(nb[v]) >= 3]
    used, chains = set(), []
    for b in branch:
        for w in nb[b]:
            if frozenset((b, w)) in used:
                continue
            path = [b, w]; used.add(frozenset((b, w)))
            while len(nb[path[-1]]) == 2:
                nx = [x for x in nb[path[-1]] if x != path[-2]][0]
                used.add(frozenset((path[-1], nx))); path.append(nx)
            chains.append(path)
    if len(branch) == 1:
        shape = "eight"
    elif all(p[0] != p[-1] for p in chains):
        shape = "theta"
    else:
        shape = "dumbbell"
        chains.sort(key=lambda p: 2 if p[0] != p[-1] else (0 if p[0] == branch[0] else 1))
    return dict(shape=shape, branch=branch, chains=chains)


def slots(dec):
    """per branch vertex the neighbours its slots lead to, in slot order"""
    b, ch = dec["branch"], dec["chains"]
    if dec["shape"] == "eight":
        return {b[0]: [ch[0][1], ch[0][-2], ch[1][1], ch[1][-2]]}
    if dec["shape"] == "theta":
        return {b[0]: [p[1] for p in ch], b[1]: [p[-2] for p in ch]}
    return {b[0]: [ch[0][1], ch[0][-2], ch[2][1]], b[1]: [ch[1][1], ch[1][-2], ch[2][-2]]}


def _vec(m):
    return np.asarray(m, dtype=np.complex128).T.reshape(-1)          # ket + chi * bra


def branch_tensor(tensors, messages, graph, v, to):
    """B[x_0, x_1, ..] of v over the legs towards `to`, x = ket + chi * bra, every other leg closed by its incoming message: a Gram phi psi^H (matmul)"""
    t = np.asarray(tensors[v], dtype=np.complex128)
    nbs = graph.nbrs[v]
    phi = t
    for j, w in enumerate(nbs):
        if w not in to:
            phi = np.moveaxis(np.tensordot(phi, np.asarray(messages[(w, v)], dtype=np.complex128), axes=([1 + j], [0])), -1, 1 + j)
    kept = [1 + nbs.index(w) for w in to]
    rest = [a for a in range(t.ndim) if a not in kept]
    dims = [t.shape[a] for a in kept]
    n = int(np.prod(dims))
    pm = np.transpose(phi, kept + rest).reshape(n, -1)
    sm = np.transpose(t, kept + rest).reshape(n, -1)
    G = (pm @ sm.conj().T).reshape(dims + dims)                         # (kets .., bras ..)
    z = len(dims)
    order = [ax for q in range(z) for ax in (z + q, q)]                 # (bra_0, ket_0, bra_1, ket_1, ..): C order makes x = ket + chi * bra
    return np.ascontiguousarray(np.transpose(G, order)).reshape([d * d for d in dims])


def chain_matrices(tensors, messages, graph, path):
    """[(A_k T_k, slack)] of the inner vertices p_1 .. p_n, T_k[(b,b'),(a,a')] with a the bond from p_{k-1} and b the bond to p_{k+1}; slack: see bound"""
    out = []
    for k in range(1, len(path) - 1):
        v, p, n = path[k], path[k - 1], path[k + 1]
        T = branch_tensor(tensors, messages, graph, v, [n, p])          # [x_b, x_a]
        f, b = _vec(messages[(v, n)]), _vec(messages[(n, v)])
        out.append((T - np.outer(f, b @ T), EPS * np.linalg.norm(f) * np.linalg.norm(b @ T)))
    return out


def end_antiprojector(messages, u, v):
    """(A_0, slack) of the edge (u, v), a matrix from u's side (columns) to v's side (rows): I - vec(m_{u->v}) vec(m_{v->u})^T"""
    f, b = _vec(messages[(u, v)]), _vec(messages[(v, u)])
    return np.eye(len(f)) - np.outer(f, b), EPS * np.linalg.norm(f) * np.linalg.norm(b)


def factors(tensors, messages, graph, dec):
    sl = slots(dec)
    mats = [chain_matrices(tensors, messages, graph, p) for p in dec["chains"]]
    a0 = [end_antiprojector(messages, p[0], p[1]) for p in dec["chains"]]
    return dict(B={v: branch_tensor(tensors, messages, graph, v, sl[v]) for v in dec["branch"]},
                mats=[[M for M, _ in ms] for ms in mats], A0=[A for A, _ in a0],
                slack=[0.0] * len(dec["branch"]) + [x for ms in mats for _, x in ms] + [x for _, x in a0])


def _chain_operator(mats, a0):
    P = a0
    for M in mats:
        P = M @ P
    return P                                                            # chi_far^2 x chi_near^2


def weight(fac, dec):
    ops = [_chain_operator(m, a) for m, a in zip(fac["mats"], fac["A0"])]
    b = dec["branch"]
    if dec["shape"] == "theta":
        B = fac["B"][b[0]]
        B = (ops[0] @ B.reshape(B.shape[0], -1)).reshape((ops[0].shape[0],) + B.shape[1:])
        B = np.matmul(ops[1], B)                                        # batched over the first leg
        B = np.matmul(B, ops[2].T)
        return complex(np.dot(B.reshape(-1), fac["B"][b[1]].reshape(-1)))
    if dec["shape"] == "dumbbell":
        g = []
        for q in range(2):
            B = fac["B"][b[q]]
            g.append(ops[q].T.reshape(-1) @ B.reshape(B.shape[0] * B.shape[1], B.shape[2]))     # sum B[x1, x2, y] L[x2, x1]
        return complex(g[1] @ (ops[2] @ g[0]))
    B = fac["B"][b[0]]
    r = ops[0].T.reshape(-1) @ B.reshape(B.shape[0] * B.shape[1], B.shape[2] * B.shape[3])
    return complex(r @ ops[1].T.reshape(-1))


def bound(fac, u, slack=False):
    """-> (8 u S k_max prod ||F_i||_F, S, k_max).  slack: for a configuration with a factor that CANCELS only -- the antiprojector of a bond of dimension 1 on a
    rescaled cache is 1 - m m = 0 up to rounding, and a norm that came out as exactly 0 would claim the weight is exactly 0.  X - f (b^T X) computed in f64 is
    only known to 2^-53 ||f|| ||b^T X|| (fac["slack"]); with slack that much is added to the factor's norm.  Everywhere else the plain norms are used."""
    fs = [B.reshape(-1, B.shape[-1]) for B in fac["B"].values()] + [M for ms in fac["mats"] for M in ms] + list(fac["A0"])
    S, kmax = len(fs), max(max(F.shape) for F in fs)
    return 8 * u * S * kmax * float(np.prod([np.linalg.norm(F) + (x if slack else 0.0) for F, x in zip(fs, fac["slack"])])), S, kmax
