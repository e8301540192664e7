"""numpy complex128 restatement of the reference's loop corrections (src/MessagePassing/loopcorrection.jl), sharing no code with the package:
what tests/test_loop_ref_cpu.py pins against exact contraction and what tests/test_gpu_loops.py compares the device against.

Conventions (those of the package and of the oracle): a graph is (vertices, edges); the tensor of v has axes (site, leg to each neighbour in
ascending vertex position); a message (src, dst) is chi x chi with axes (ket, bra).

  weight           loopcorrection.jl:79-89   contraction of one configuration: the vertices' double-layer tensors, the cache's messages on
                                             every leg that leaves the configuration, an antiprojector on every edge of it (:53-58)
  configurations   loopcorrection.jl:9       leafless_edge_induced_subgraphs(graph, max) -- by brute force over all edge subsets (small graphs only)
  loopcorrected    loopcorrection.jl:3-14    Z_bp (1 + sum of the weights), on rescaled tensors and messages (:8)
  bp / rescale     beliefpropagationcache.jl:51-72,82-140 -- a plain Jacobi-free Gauss-Seidel BP to a tolerance, and the rescaling that makes
                                             every vertex and edge scalar 1
The enumeration INCLUDES disconnected configurations (their weight is the product of the components' weights: the contraction factorises)."""
import itertools

import numpy as np


class RefGraph:
    def __init__(self, vertices, edges):
        self.vertices = list(vertices)
        self.pos = {v: i for i, v in enumerate(self.vertices)}
        self.edges = [tuple(e) for e in edges]
        self.nbrs = {v: [] for v in self.vertices}
        for (a, b) in self.edges:
            self.nbrs[a].append(b); self.nbrs[b].append(a)
        for v in self.vertices:
            self.nbrs[v].sort(key=self.pos.__getitem__)

    def axis(self, v, w):
        return 1 + self.nbrs[v].index(w)


def _double_layer(t, ms):
    """E[s-summed][(k_1, b_1), ..., (k_z, b_z)] -> array of shape (chi_1, chi_1, ..., chi_z, chi_z) with the legs listed in `ms` (axis -> message
    or None) closed by their message: sum_{s} psi[s, k..] conj(psi[s, b..]) prod m[k_j, b_j]"""
    z = t.ndim - 1
    ket = [0] + [1 + 2 * j for j in range(z)]
    bra = [0] + [2 + 2 * j for j in range(z)]
    args = [t.astype(np.complex128), ket, np.conj(t.astype(np.complex128)), bra]
    keep = []
    for j in range(z):
        if ms[j] is not None:
            args += [np.asarray(ms[j], dtype=np.complex128), [1 + 2 * j, 2 + 2 * j]]
        else:
            keep += [1 + 2 * j, 2 + 2 * j]
    return np.einsum(*args, keep, optimize=("greedy", 2 ** 27))


def antiprojector(m_uv, m_vu):
    """edge (u, v), loopcorrection.jl:53-58: delta - message(e) * message(reverse(e)); axes (k_u, b_u, k_v, b_v).  The side of u pairs with the
    message that ARRIVES at u, m_{v -> u}, the side of v with m_{u -> v}; no conjugate."""
    chi = m_uv.shape[0]
    eye = np.eye(chi)
    return np.einsum("ac,bd->abcd", eye, eye) - np.einsum("ab,cd->abcd", np.asarray(m_vu, dtype=np.complex128), np.asarray(m_uv, dtype=np.complex128))


def weight(tensors, messages, graph, edges):
    """loopcorrection.jl:79-89 for any configuration `edges` (connected or not): scalar(contract([incoming messages; bp factors; antiprojectors]))"""
    inside = {frozenset(e) for e in edges}
    verts = [v for v in graph.vertices if any(v in e for e in inside)]
    lab = {}

    def ix(*k):
        return lab.setdefault(k, len(lab))
    args = []
    for v in verts:
        nb = graph.nbrs[v]
        ms = [None if frozenset((v, w)) in inside else messages[(w, v)] for w in nb]
        idx = [i for w in nb if frozenset((v, w)) in inside for i in (ix("k", v, w), ix("b", v, w))]
        args += [_double_layer(tensors[v], ms), idx]
    for (u, v) in edges:
        args += [antiprojector(messages[(u, v)], messages[(v, u)]), [ix("k", u, v), ix("b", u, v), ix("k", v, u), ix("b", v, u)]]
    return complex(np.einsum(*args, [], optimize=("greedy", 2 ** 27)))


def cycle_matrices(tensors, messages, graph, ring):
    """[A_k T_k] of the simple cycle `ring` (vertex list), T_k[(b,b'),(a,a')] with a the bond from ring[k-1] and b the bond to ring[k+1]: the
    matrices whose product's trace is the weight -- their Frobenius norms enter the device test's error bound"""
    L = len(ring)
    out = []
    for k, v in enumerate(ring):
        p, n = ring[k - 1], ring[(k + 1) % L]
        nb = graph.nbrs[v]
        ms = [None if w in (p, n) else messages[(w, v)] for w in nb]
        E = _double_layer(tensors[v], ms)                      # axes (k_first, b_first, k_second, b_second) in neighbour order
        if graph.pos[p] < graph.pos[n]:
            ka, ba, kb, bb = 0, 1, 2, 3
        else:
            kb, bb, ka, ba = 0, 1, 2, 3
        ca, cb = E.shape[ka], E.shape[kb]
        T = np.transpose(E, (bb, kb, ba, ka)).reshape(cb * cb, ca * ca)      # row b + cb b', column a + ca a'
        f = np.asarray(messages[(v, n)], dtype=np.complex128).T.reshape(-1)  # vec: ket + chi bra
        b = np.asarray(messages[(n, v)], dtype=np.complex128).T.reshape(-1)
        out.append(T - np.outer(f, b @ T))
    return out


def cycle_weight(mats):
    P = mats[0]
    for M in mats[1:]:
        P = M @ P
    return complex(np.trace(P))


def ring_order(edges):
    """the vertices of a connected edge set in ring order when it is a simple cycle (every vertex of degree 2), else None"""
    nb = {}
    for (a, b) in edges:
        nb.setdefault(a, []).append(b); nb.setdefault(b, []).append(a)
    if any(len(x) != 2 for x in nb.values()):
        return None
    ring, prev, cur = [edges[0][0]], None, edges[0][0]
    while True:
        nxt = [w for w in nb[cur] if w != prev][0] if prev is not None else nb[cur][0]
        if nxt == ring[0]:
            return ring
        ring.append(nxt); prev, cur = cur, nxt


def configurations(graph, max_edges, connected_only=False):
    """every non-empty edge subset of at most max_edges edges whose edge-induced subgraph has no vertex of degree 1 (brute force)"""
    out = []
    for r in range(1, min(max_edges, len(graph.edges)) + 1):
        for sub in itertools.combinations(graph.edges, r):
            deg = {}
            for (a, b) in sub:
                deg[a] = deg.get(a, 0) + 1; deg[b] = deg.get(b, 0) + 1
            if min(deg.values()) < 2:
                continue
            if connected_only and len(components(sub)) != 1:
                continue
            out.append(sub)
    return out


def components(edges):
    comps = []
    for e in edges:
        hit = [c for c in comps if any(v in c[0] for v in e)]
        merged = (set(e), [e])
        for c in hit:
            merged[0].update(c[0]); merged[1].extend(c[1]); comps.remove(c)
        comps.append(merged)
    return [tuple(c[1]) for c in comps]


def bp(tensors, graph, tolerance=1e-13, maxiter=2000):
    """messages of a BP fixed point: sequential sweeps over all directed edges, m <- m / sum(m), until no message moves by more than `tolerance`"""
    messages = {}
    for (a, b) in graph.edges:
        chi = tensors[a].shape[graph.axis(a, b)]
        messages[(a, b)] = np.eye(chi, dtype=np.complex128) / chi
        messages[(b, a)] = np.eye(chi, dtype=np.complex128) / chi
    order = [e for (a, b) in graph.edges for e in ((a, b), (b, a))]
    for _ in range(maxiter):
        worst = 0.0
        for (src, dst) in order:
            ms = [None if w == dst else messages[(w, src)] for w in graph.nbrs[src]]
            m = _double_layer(tensors[src], ms)
            m = m / np.sum(m)
            worst = max(worst, float(np.max(np.abs(m - messages[(src, dst)]))))
            messages[(src, dst)] = m
        if worst <= tolerance:
            return messages
    raise RuntimeError(f"loop_ref.bp: not converged to {tolerance} in {maxiter} sweeps (last change {worst})")


def rescale(tensors, messages, graph):
    """-> (tensors', messages', Z_bp) with every edge scalar sum_ij m_e[i,j] m_rev[i,j] and every vertex scalar equal to 1
    (beliefpropagationcache.jl:82-140), Z_bp = prod vertex scalars / prod edge scalars of the input (abstract...:289-304)"""
    ms = dict(messages)
    z = 1.0 + 0.0j
    for (a, b) in graph.edges:
        n = np.sum(ms[(a, b)] * ms[(b, a)])
        z /= n
        ms[(a, b)] = ms[(a, b)] / np.sqrt(n); ms[(b, a)] = ms[(b, a)] / np.sqrt(n)
    ts = {}
    for v in graph.vertices:
        def vs(mm):
            return complex(_double_layer(tensors[v], [mm[(w, v)] for w in graph.nbrs[v]]))
        z *= vs(messages)
        ts[v] = np.asarray(tensors[v], dtype=np.complex128) / np.sqrt(vs(ms))
    return ts, ms, z


def loopcorrected(tensors, graph, max_edges, connected_only=False, messages=None):
    """loopcorrection.jl:3-14 -> (Z_bp (1 + sum W), Z_bp, [(configuration, W)])"""
    messages = bp(tensors, graph) if messages is None else messages
    ts, ms, zbp = rescale(tensors, messages, graph)
    ws = [(c, weight(ts, ms, graph, c)) for c in configurations(graph, max_edges, connected_only)]
    return zbp * (1 + sum(w for _, w in ws)), zbp, ws
