"""numpy restatement of the reference's boundary-MPS contraction (src/MessagePassing/boundarympscache.jl, src/expect.jl:84-156, src/norm_sqr.jl:86-91) for states on
open rectangular grids: what tests/test_bmps_ref_cpu.py pins against the dense simulator and tests/test_gpu_bmps.py compares the device against.

A state is (graph, tensors): vertices are 2-tuples, tensors[v] has axes (site, one leg per neighbour in graph.neighbors(v) order).  Everything is complex128 (or
clongdouble for the contractions: `dtype`; numpy.linalg.qr itself always runs in complex128).

Index letters of the einsum strings: U[x, i, j, y] the incoming MPS tensor (links x, y; ket / bra leg i, j), A[s, i, o, h, r] the site tensor (in, out, left, right),
conj(A)[s, j, p, g, q], V[b, o, p, c] the MPS on the other side (the daggered guess while fitting), L[x, h, g, b] / R[y, r, q, c] the environments."""
import numpy as np


def default_tolerance(dtype):
    """default_tolerance (src/MessagePassing/beliefpropagationcache.jl:104-108)"""
    return 1e-5 if np.dtype(dtype) in (np.dtype(np.complex64), np.dtype(np.float32)) else 1e-8


def partition(graph, partition_by="row"):
    """BoundaryMPSCache(...) (:145-175): groups of the first ("row") or last ("col") coordinate, sorted inside by the other; is_correct_format (:69-81) and
    pseudo_planar_edges (:560-576) as refusals.  Returns the grid rows[p][l] of vertices."""
    key = (lambda v: v[0]) if partition_by == "row" else (lambda v: v[1])
    order = (lambda v: v[1]) if partition_by == "row" else (lambda v: v[0])
    keys = sorted({key(v) for v in graph.vertices})
    rows = [sorted([v for v in graph.vertices if key(v) == k], key=order) for k in keys]
    part = {v: p for p, r in enumerate(rows) for v in r}
    for r in rows:
        for a, b in zip(r, r[1:]):
            if b not in graph.neighbors(a):
                raise ValueError("the graph would need pseudo-edges")
    for (a, b) in graph.edges:
        dp = abs(part[a] - part[b])
        if dp == 0:
            ra = rows[part[a]]
            if abs(ra.index(a) - ra.index(b)) != 1:
                raise ValueError("There's a partition that does not form a line: can't run boundary MPS")
        elif dp != 1:
            raise ValueError("Upon partitioning, graph does not form a line: can't run boundary MPS")
    if len(rows) < 2 or len({len(r) for r in rows}) != 1 or len(rows[0]) < 2:
        raise ValueError("not a rectangular grid")
    for p in range(len(rows) - 1):
        for a, b in zip(rows[p], rows[p + 1]):
            if b not in graph.neighbors(a):
                raise ValueError("not a rectangular grid")
    return rows


def link_dims(chis, R):
    """virtual_index_dimension (:119-143): link l between cross edges l - 1 and l; links 0 and L are 1"""
    L = len(chis)
    out = [1] * (L + 1)
    for l in range(1, L):
        below = float(np.prod([float(c) for c in chis[:l]]))
        above = float(np.prod([float(c) for c in chis[l:]]))
        out[l] = int(min(above * above, below * below, float(R)))
    return out


def qr_shapes(chis, R):
    """(m, n) of every QR the fitting driver issues for one message: the initial walk from the far end, then the steps of a sweep there and back"""
    L, link = len(chis), link_dims(chis, R)
    towards_lower = [(chis[i] ** 2 * link[i + 1], link[i]) for i in range(L - 1, 0, -1)]
    towards_higher = [(link[i] * chis[i] ** 2, link[i + 1]) for i in range(L - 1)]
    return towards_lower + towards_higher


def qr_numpy(M):
    return np.linalg.qr(M.astype(np.complex128), mode="reduced")


def qr_random_completion(seed, rtol=1e-10):
    """numpy.linalg.qr whose completion of the null space -- the columns of Q that a rank-deficient matrix leaves free -- is replaced by a seeded random one"""
    rng = np.random.default_rng(seed)

    def qr(M):
        Q0, Y0 = qr_numpy(M)
        d = np.abs(np.diag(Y0))
        scale = max(d.max(), np.finfo(float).tiny)
        if np.all(d > rtol * scale):
            return Q0, Y0
        # a column that adds nothing to the span of the ones before it leaves its column of Q free: Gram-Schmidt (two passes), a random direction there
        M = M.astype(np.complex128)
        m, n = M.shape
        Q, Y = np.zeros((m, n), dtype=np.complex128), np.zeros((n, n), dtype=np.complex128)
        for c in range(n):
            x = M[:, c].copy()
            for _ in range(2):
                for k in range(c):
                    h = np.vdot(Q[:, k], x)
                    Y[k, c] += h; x = x - Q[:, k] * h
            nx = np.linalg.norm(x)
            if nx > rtol * scale:
                Q[:, c], Y[c, c] = x / nx, nx
                continue
            x = rng.standard_normal(m) + 1j * rng.standard_normal(m)
            for _ in range(2):
                for k in range(c):
                    x = x - Q[:, k] * np.vdot(Q[:, k], x)
            Q[:, c] = x / np.linalg.norm(x)
        return Q, Y
    return qr


def _site(graph, tensors, rows, p, l, pin, pout, dtype):
    """A[s, in, out, left, right] of the vertex at (p, l); a missing leg has dimension 1"""
    v = rows[p][l]
    t = np.asarray(tensors[v]).astype(dtype)
    nb = list(graph.neighbors(v))
    want = [rows[pin][l] if 0 <= pin < len(rows) else None, rows[pout][l] if 0 <= pout < len(rows) else None,
            rows[p][l - 1] if l > 0 else None, rows[p][l + 1] if l + 1 < len(rows[p]) else None]
    axes, shape = [0], [t.shape[0]]
    for w in want:
        if w is not None and w in nb:
            axes.append(1 + nb.index(w)); shape.append(t.shape[1 + nb.index(w)])
        else:
            shape.append(1)
    assert len(axes) == t.ndim, "a vertex with an unexpected neighbour"
    return np.transpose(t, axes).reshape(shape)


def _three_left(U, Lenv, A, Ab):
    return np.einsum("xijy,xhgb,siohr,sjpgq->yborpq", U, Lenv, A, Ab.conj(), optimize=True)


def _left_step(U, Lenv, A, Ab, V):
    return np.einsum("yborpq,bopc->yrqc", _three_left(U, Lenv, A, Ab), V, optimize=True)


def _right_step(U, Renv, A, Ab, V):
    T = np.einsum("xijy,yrqc,siohr,sjpgq->xcohpg", U, Renv, A, Ab.conj(), optimize=True)
    return np.einsum("xcohpg,bopc->xhgb", T, V, optimize=True)


def _gauge_step(Bt, frm, to, qr, log):
    """gauge_step! (:270-285): factorize(m1, left_inds; ortho = "left") is a QR without truncation"""
    b = Bt[frm]
    if to > frm:
        M = b.reshape(-1, b.shape[3])
        log.append(M.shape)
        Q, Y = qr(M)
        Bt[frm] = Q.reshape(b.shape).astype(b.dtype)
        Bt[to] = np.einsum("nb,bopc->nopc", Y, Bt[to])
    else:
        M = b.reshape(b.shape[0], -1).T
        log.append(M.shape)
        Q, Y = qr(M)
        Bt[frm] = Q.T.reshape(b.shape).astype(b.dtype)
        Bt[to] = np.einsum("bopc,nc->bopn", Bt[to], Y)


def fit_message(A, U, chis, R, niters=50, tolerance=None, normalize=True, qr=qr_numpy, dtype=np.complex128, qr_log=None):
    """update_message!(alg "fitting", :330-369) for one interpartition message.  A[l]: site tensors [s, in, out, left, right] of the source partition, U[l]: the MPS
    entering it from the other side, chis[l]: the bond dimensions of the cross edges.  Returns (message tensors M_l[link, a, a', link'], sweeps, last epsilon)."""
    L, link = len(A), link_dims(chis, R)
    log = [] if qr_log is None else qr_log
    # the guess (:180-202), daggered onto the reverse edges (:204-218): delta(a, a') times all-ones links
    Bt = [np.einsum("b,op,c->bopc", np.ones(link[l]), np.eye(chis[l]), np.ones(link[l + 1])).astype(dtype) for l in range(L)]
    for i in range(L - 1, 0, -1):
        _gauge_step(Bt, i, i - 1, qr, log)
    one = np.ones((1, 1, 1, 1), dtype=dtype)
    Lenv, Renv = [None] * L, [None] * L
    Lenv[0], Renv[L - 1] = one, one
    for l in range(L - 1, 0, -1):
        Renv[l - 1] = _right_step(U[l], Renv[l], A[l], A[l], Bt[l])
    seq = list(range(L)) + list(range(L - 2, 0, -1))
    prev, prev_cf, sweeps, eps = None, 0.0, 0, float("nan")
    for it in range(1, niters + 1):
        if it == niters:
            seq = seq + [0]
        cf = 0.0
        for l in seq:
            if prev is not None:
                _gauge_step(Bt, prev, l, qr, log)
                if l > prev:
                    Lenv[l] = _left_step(U[prev], Lenv[prev], A[prev], A[prev], Bt[prev])
                else:
                    Renv[l] = _right_step(U[prev], Renv[prev], A[prev], A[prev], Bt[prev])
            m = np.einsum("yborpq,yrqc->bopc", _three_left(U[l], Lenv[l], A[l], A[l]), Renv[l], optimize=True)
            n = float(np.sqrt(np.sum(np.abs(m) ** 2)))
            cf += n
            if normalize and n != 0:
                m = m / n
            Bt[l] = m.conj()
            prev = l
        cf /= len(seq)
        eps, sweeps = abs(cf - prev_cf), it
        if tolerance is not None and eps < tolerance:
            break
        prev_cf = cf
    return [b.conj() for b in Bt], sweeps, eps


class BoundaryMPS:
    """all interpartition messages of a state, fitted once each (the quotient graph is a line: maxiter = 1, :30)"""

    def __init__(self, graph, tensors, R, partition_by="row", niters=50, tolerance="default", normalize=True, qr=qr_numpy, dtype=np.complex128):
        self.rows = partition(graph, partition_by)
        self.graph, self.tensors, self.R, self.dtype = graph, tensors, R, dtype
        P, L = len(self.rows), len(self.rows[0])
        self.P, self.L = P, L
        tol = default_tolerance(next(iter(tensors.values())).dtype) if isinstance(tolerance, str) else tolerance
        one = np.ones((1, 1, 1, 1), dtype=dtype)
        self.qr_log, self.sweeps, self.eps = [], {}, {}
        self.down, self.up = [None] * (P - 1), [None] * (P - 1)      # down[p]: p -> p + 1, up[p]: p + 1 -> p
        kw = dict(niters=niters, tolerance=tol, normalize=normalize, qr=qr, dtype=dtype, qr_log=self.qr_log)
        for p in range(P - 1):
            A = [_site(graph, tensors, self.rows, p, l, p - 1, p + 1, dtype) for l in range(L)]
            U = self.down[p - 1] if p > 0 else [one] * L
            self.down[p], self.sweeps[(p, p + 1)], self.eps[(p, p + 1)] = fit_message(A, U, [a.shape[2] for a in A], R, **kw)
        for p in range(P - 2, -1, -1):
            A = [_site(graph, tensors, self.rows, p + 1, l, p + 2, p, dtype) for l in range(L)]
            U = self.up[p + 1] if p + 1 < P - 1 else [one] * L
            self.up[p], self.sweeps[(p + 1, p)], self.eps[(p + 1, p)] = fit_message(A, U, [a.shape[2] for a in A], R, **kw)

    def _row(self, p):
        one = np.ones((1, 1, 1, 1), dtype=self.dtype)
        A = [_site(self.graph, self.tensors, self.rows, p, l, p - 1, p + 1, self.dtype) for l in range(self.L)]
        U = self.down[p - 1] if p > 0 else [one] * self.L
        V = self.up[p] if p < self.P - 1 else [one] * self.L
        return A, U, V, one

    def expect_parts(self, verts, ops):
        """path_contract (:616-667): (numer, denom) of operators ops[k] (d x d, op[s', s]) on verts[k], all in one partition"""
        where = {v: (p, l) for p, r in enumerate(self.rows) for l, v in enumerate(r)}
        ps = {where[v][0] for v in verts}
        if len(ps) != 1:
            raise ValueError("Observable support must be within a single partition (row/ column) of the graph for now.")
        p = ps.pop()
        A, U, V, one = self._row(p)
        pos = {where[v][1]: np.asarray(o, dtype=self.dtype) for v, o in zip(verts, ops)}
        lmin, lmax = min(pos), max(pos)
        Lenv = one
        for l in range(lmin):
            Lenv = _left_step(U[l], Lenv, A[l], A[l], V[l])
        Renv = [None] * self.L
        Renv[self.L - 1] = one
        for l in range(self.L - 1, lmin, -1):
            Renv[l - 1] = _right_step(U[l], Renv[l], A[l], A[l], V[l])
        X = Lenv
        for l in range(lmin, lmax + 1):
            K = np.einsum("ts,siohr->tiohr", pos[l], A[l]) if l in pos else A[l]
            X = _left_step(U[l], X, K, A[l], V[l])
        numer = np.einsum("yrqc,yrqc->", X, Renv[lmax])
        denom = np.einsum("yrqc,yrqc->", _left_step(U[lmin], Lenv, A[lmin], A[lmin], V[lmin]), Renv[lmin])
        return complex(numer), complex(denom)

    def expect(self, verts, ops):
        n, d = self.expect_parts(verts, ops)
        return n / d

    def log_norm_sqr(self):
        """partitionfunction with vertex_scalar / edge_scalar (:504-519): sum_p log(vertex scalar) - sum_(p, p + 1) log(edge scalar)"""
        lz = 0j
        for p in range(self.P):
            A, U, V, one = self._row(p)
            R = one
            for l in range(self.L - 1, 0, -1):
                R = _right_step(U[l], R, A[l], A[l], V[l])
            lz += np.log(complex(np.einsum("yrqc,yrqc->", _left_step(U[0], one, A[0], A[0], V[0]), R)))
        for p in range(self.P - 1):
            E = np.ones((1, 1), dtype=self.dtype)
            for l in range(self.L):
                E = np.einsum("ef,eopy,fopc->yc", E, self.down[p][l], self.up[p][l], optimize=True)
            lz -= np.log(complex(E[0, 0]))
        return complex(lz)
