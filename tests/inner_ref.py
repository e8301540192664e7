"""numpy complex128 restatement of inner(psi, phi; alg = "bp") -- belief propagation on BilinearForm(ket, bra) -- for the tests of tnqs_inner_bp.  Reference lines
(paths relative to the reference repository): src/inner.jl:65-69 (the call), src/Forms/bilinearform.jl:16-25 (bra = dag(prime(phi)): the conjugate is on the SECOND
argument), src/MessagePassing/abstractbeliefpropagationcache.jl:162-190 (updated_message), :223-259 (update), :289-304 (freenergy),
src/MessagePassing/beliefpropagationcache.jl:17-21 (message_diff), :47-49 (edge_scalar).  Built on the oracle's _absorb, _gram, message_diff and
forest_cover_edge_sequence (oracle/tnqs_oracle.py); tensors have axes (s, legs in ascending neighbour position), a message m[a, b] has a on the ket's leg and b on
the bra's and starts as the rectangular delta (delta(virtualinds(form, e)))."""
import numpy as np

import tnqs_oracle as o


def crandn(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)


def delta(r, c):
    m = np.zeros((r, c), dtype=np.complex128)
    k = min(r, c)
    m[np.arange(k), np.arange(k)] = 1
    return m


class FormCache:
    """the form network of (ket, bra) on the oracle graph g with its messages (absent: the delta)"""

    def __init__(self, g, ket, bra, messages=None):
        self.g, self.ket, self.bra = g, ket, bra
        self.messages = dict(messages or {})

    def copy(self):
        return FormCache(self.g, self.ket, self.bra, self.messages)

    def message(self, e):
        m = self.messages.get(e)
        if m is None:
            u, v = e
            ax = self.g.leg(u, v)
            m = delta(self.ket[u].shape[ax], self.bra[u].shape[ax])
        return m


def raw_message(fc, e):
    """sum_{s, rest} (ket_u x_{k != v} m_{k -> u})[s, a, rest'] conj(bra_u[s, b, rest']): every message absorbed on the ket's side (abstract...:162-181)"""
    u, v = e
    g = fc.g
    t = fc.ket[u].astype(np.complex128)
    for k in g.nbrs[u]:
        if k != v:
            t = o._absorb(t, g.leg(u, k), fc.message((k, u)).astype(np.complex128))
    return o._gram(t, fc.bra[u].astype(np.complex128), g.leg(u, v))


def updated_message(fc, e, normalize=True):
    """the raw message divided by its element sum when that is not exactly zero (abstract...:182-187)"""
    m = raw_message(fc, e)
    if normalize:
        s = m.sum()
        if s != 0:
            m = m / s
    return m


def sweep(fc, seq, normalize=True, store=np.complex128):
    """one Gauss-Seidel sweep over seq IN PLACE; returns message_diff averaged over the sequence (abstract...:223-259, beliefpropagationcache.jl:17-21).
    store: the type messages are kept in (the device keeps them in the state's type)"""
    diff = 0.0
    for e in seq:
        prev = fc.message(e)
        new = updated_message(fc, e, normalize).astype(store)
        fc.messages[e] = new
        diff += o.message_diff(new.astype(np.complex128), prev.astype(np.complex128))
    return diff / max(1, len(seq))


def run(g, ket, bra, nsweeps, seq=None, tolerance=None, normalize=True, store=np.complex128, info=None):
    """FormCache after nsweeps sweeps (fewer when a tolerance is met)"""
    fc = FormCache(g, ket, bra)
    seq = o.forest_cover_edge_sequence(g) if seq is None else seq
    niter, avg, conv = 0, None, False
    for i in range(1, nsweeps + 1):
        avg = sweep(fc, seq, normalize, store)
        niter = i
        if tolerance is not None and avg <= tolerance:
            conv = True
            break
    if info is not None:
        info.update(niter=niter, diff=avg, converged=conv)
    return fc


def vertex_terms(fc, v):
    """the terms t = X[n, a] conj(Y[n, b]) m[a, b] whose sum is vertex_scalar(v): X the ket tensor with the messages of every leg but the first absorbed,
    Y the bra tensor, m the message coming back through the first leg (for a vertex without neighbours: ket[s] conj(bra[s]))"""
    g = fc.g
    if not g.nbrs[v]:
        return (fc.ket[v].astype(np.complex128) * fc.bra[v].astype(np.complex128).conj()).ravel()
    w = g.nbrs[v][0]
    t = fc.ket[v].astype(np.complex128)
    for k in g.nbrs[v]:
        if k != w:
            t = o._absorb(t, g.leg(v, k), fc.message((k, v)).astype(np.complex128))
    ax = g.leg(v, w)
    X = np.moveaxis(t, ax, -1).reshape(-1, t.shape[ax])
    y = fc.bra[v].astype(np.complex128)
    Y = np.moveaxis(y, ax, -1).reshape(-1, y.shape[ax])
    m = fc.message((w, v)).astype(np.complex128)
    return (X[:, :, None] * Y.conj()[:, None, :] * m[None, :, :]).ravel()


def vertex_scalar(fc, v):
    """sum_ab raw_{v -> w}[a, b] m_{w -> v}[a, b] for the first neighbour w (any one gives the same contraction)"""
    g = fc.g
    if not g.nbrs[v]:
        return complex(np.sum(fc.ket[v].astype(np.complex128) * fc.bra[v].astype(np.complex128).conj()))
    w = g.nbrs[v][0]
    return complex(np.sum(raw_message(fc, (v, w)) * fc.message((w, v)).astype(np.complex128)))


def edge_scalar(fc, e):
    return complex(np.sum(fc.message(e).astype(np.complex128) * fc.message((e[1], e[0])).astype(np.complex128)))


def log_inner(fc):
    """freenergy of the form cache (abstract...:289-304): sum_v log(vertex scalar) - sum_e log(edge scalar), complex logs"""
    num = np.array([vertex_scalar(fc, v) for v in fc.g.vertices], dtype=complex)
    den = np.array([edge_scalar(fc, e) for e in fc.g.edges], dtype=complex)
    return complex(np.sum(np.log(num)) - np.sum(np.log(den)))


def cancellation(fc):
    """max over the vertices of sum|t| / |sum t| over the terms of the vertex scalar"""
    worst = 0.0
    for v in fc.g.vertices:
        t = vertex_terms(fc, v)
        worst = max(worst, float(np.abs(t).sum() / abs(t.sum())))
    return worst


def dense_state(g, tensors):
    """the state as one array with the site axes in vertex order (small graphs only)"""
    eid = {e: i for i, e in enumerate(g.edges)}
    nv = len(g.vertices)
    args = []
    for i, v in enumerate(g.vertices):
        idx = [i] + [nv + eid[(v, w) if (v, w) in eid else (w, v)] for w in g.nbrs[v]]
        args += [np.asarray(tensors[v], dtype=np.complex128), idx]
    return np.einsum(*args, list(range(nv)), optimize="greedy")


def dense_inner(g, ket, bra):
    """sum psi conj(phi), exactly"""
    return complex(np.sum(dense_state(g, ket) * dense_state(g, bra).conj()))


def log_close(a, b):
    """|a - b| with the imaginary parts compared modulo 2 pi"""
    d = complex(a) - complex(b)
    im = (d.imag + np.pi) % (2 * np.pi) - np.pi
    return abs(complex(d.real, im))


# ---- inputs shared by the CPU and the GPU tests -----------------------------------------------------------------------------------------------------------------
def random_dims(g, rng, lo, hi):
    return {e: int(rng.integers(lo, hi + 1)) for e in g.edges}


def tensors_of(g, dims, rng, d=2, bias=0.0):
    """site tensors with bond dimensions dims[e]: bias + complex normal entries"""
    out = {}
    for v in g.vertices:
        shp = (d,) + tuple(dims[(v, w) if (v, w) in dims else (w, v)] for w in g.nbrs[v])
        out[v] = bias + crandn(rng, shp)
    return out


def padded_related(g, ket, rng, amount=0.2):
    """phi = psi zero-padded by one on every bond plus amount x noise"""
    out = {}
    for v in g.vertices:
        t = ket[v]
        shp = (t.shape[0],) + tuple(n + 1 for n in t.shape[1:])
        p = np.zeros(shp, dtype=np.complex128)
        p[tuple(slice(0, n) for n in t.shape)] = t
        out[v] = p + amount * crandn(rng, shp)
    return out


def cube_graph():
    return o.named_grid((2, 2, 2))


LOOPY_CASES = {"grid3x4": lambda: o.named_grid((3, 4)), "hex2x2": lambda: o.named_hexagonal_lattice_graph(2, 2), "cube2x2x2": cube_graph}
# the largest cancellation(fc) over LOOPY_CASES after 3 and after 8 sweeps (tests/test_inner_ref_cpu.py recomputes it and holds it at or below 2: the end-to-end
# bound of tests/test_gpu_inner.py assumes that no vertex scalar cancels)
LOOPY_CANCELLATION = 1.2204


def loopy_case(name, seed=0):
    """(g, ket, bra) of a loopy end-to-end case: ket with bond dimensions 2..3 and entries 1 + 0.5 x complex normal (a positive part that keeps the vertex scalars
    from cancelling), bra = ket zero-padded by one on every bond plus 0.2 x noise"""
    g = LOOPY_CASES[name]()
    rng = np.random.default_rng([seed, sorted(LOOPY_CASES).index(name)])
    ket = {v: 1.0 + 0.5 * (t - 0.0) for v, t in tensors_of(g, random_dims(g, rng, 2, 3), rng).items()}
    bra = padded_related(g, ket, rng)
    return g, ket, bra


def tree_case(name, seed=0):
    """(g, ket, bra) on a tree with independent bond dimensions 1..4 per state and edge"""
    g = o.comb_tree((3, 3)) if name == "comb33" else o.named_grid((5,))
    rng = np.random.default_rng([seed, 7 if name == "comb33" else 9])
    ket = tensors_of(g, random_dims(g, rng, 1, 4), rng)
    bra = tensors_of(g, random_dims(g, rng, 1, 4), rng)
    return g, ket, bra
