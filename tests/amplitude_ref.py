"""numpy complex128 restatement of the amplitude <x|psi> of a bitstring by belief propagation -- the reference's single-layer path -- for the tests of
tnqs_amplitudes_bp.  Reference lines (paths relative to the reference repository): src/contract.jl:7-9 (contract(tn; alg = "bp")), src/sampling.jl:258-285
(certify_sample: every site projected on x_v, the single-layer network contracted), src/TensorNetworks/tensornetwork.jl:62-64 (default_message: delta of ONE index, a
vector of ones), :66-68 (bp_factors: the one tensor of the vertex), src/MessagePassing/abstractbeliefpropagationcache.jl:162-190 (updated_message), :223-259 (update),
:289-304 (freenergy / partitionfunction), src/MessagePassing/beliefpropagationcache.jl:17-21 (message_diff), :47-49 (edge_scalar).
The network of a string x has one tensor per vertex, A_v = T_v[x_v, ...] (axes: the legs in ascending neighbour position); a message is a vector on the leg and starts
as ALL ONES -- not e_0, which is what inner_ref's rectangular delta gives against a chi = 1 bra."""
import numpy as np

import tnqs_oracle as o
from inner_ref import crandn, dense_state, log_close, random_dims, tensors_of      # noqa: F401  (input builders, shared with the tests of inner)


class AmpCache:
    """the network of one string on the oracle graph g with its messages (absent: ones)"""

    def __init__(self, g, tensors, x, messages=None):
        self.g, self.x = g, dict(x)
        self.A = {v: np.asarray(tensors[v])[x[v]].astype(np.complex128) for v in g.vertices}
        self.messages = dict(messages or {})

    def message(self, e):
        m = self.messages.get(e)
        if m is None:
            u, v = e
            m = np.ones(self.A[u].shape[self.g.leg(u, v) - 1], dtype=np.complex128)      # tensornetwork.jl:62-64
        return m


def _ax(g, u, v):
    """axis of the leg u - v in A_u (the oracle counts the site axis, which A_u has lost)"""
    return g.leg(u, v) - 1


def raw_message(ac, e):
    """m[j] = sum A_u[..., j, ...] prod_{k != v} m_{k -> u}[i_k] (abstract...:162-181)"""
    u, v = e
    g = ac.g
    keep = _ax(g, u, v)
    t = ac.A[u]
    for k in reversed(g.nbrs[u]):                        # from the last leg to the first: the axes in front keep their positions
        if k != v:
            t = np.tensordot(t, ac.message((k, u)).astype(np.complex128), axes=([_ax(g, u, k)], [0]))
    assert t.ndim == 1 and t.shape[0] == ac.A[u].shape[keep]
    return t


def updated_message(ac, e, normalize=True):
    """the raw message divided by its element sum when that is not exactly zero (abstract...:182-187)"""
    m = raw_message(ac, e)
    if normalize:
        s = m.sum()
        if s != 0:
            m = m / s
    return m


def sweep(ac, seq, normalize=True, store=np.complex128):
    """one Gauss-Seidel sweep over seq IN PLACE; returns message_diff averaged over the sequence (abstract...:223-259, beliefpropagationcache.jl:17-21).
    store: the type messages are kept in (the device keeps them in the state's type)"""
    diff = 0.0
    for e in seq:
        prev = ac.message(e)
        new = updated_message(ac, e, normalize).astype(store)
        ac.messages[e] = new
        diff += o.message_diff(new.astype(np.complex128), prev.astype(np.complex128))
    return diff / max(1, len(seq))


def run(g, tensors, x, nsweeps, seq=None, tolerance=None, normalize=True, store=np.complex128, info=None):
    """AmpCache of ONE string after nsweeps sweeps -- fewer when its own average diff meets the tolerance: strings do not know of each other"""
    ac = AmpCache(g, tensors, x)
    seq = o.forest_cover_edge_sequence(g) if seq is None else seq
    niter, avg, conv = 0, 0.0, False
    for i in range(1, nsweeps + 1):
        if not seq:
            break
        avg = sweep(ac, seq, normalize, store)
        niter = i
        if tolerance is not None and avg <= tolerance:
            conv = True
            break
    if info is not None:
        info.update(niter=niter, diff=avg, converged=conv)
    return ac


def vertex_terms(ac, v):
    """the terms whose sum is vertex_scalar(v): A_v with the messages of every leg but the first absorbed, times the message coming back through the first leg"""
    g = ac.g
    if not g.nbrs[v]:
        return np.array([ac.A[v]], dtype=np.complex128).ravel()
    t = ac.A[v]
    for k in g.nbrs[v]:
        shp = [1] * t.ndim
        shp[_ax(g, v, k)] = -1
        t = t * ac.message((k, v)).astype(np.complex128).reshape(shp)
    return t.ravel()


def vertex_scalar(ac, v):
    """sum_j raw_{v -> w}[j] m_{w -> v}[j] for the first neighbour w; a vertex without neighbours: the entry T_v[x_v]"""
    g = ac.g
    if not g.nbrs[v]:
        return complex(ac.A[v])
    w = g.nbrs[v][0]
    return complex(np.sum(raw_message(ac, (v, w)) * ac.message((w, v)).astype(np.complex128)))


def edge_scalar(ac, e):
    return complex(np.sum(ac.message(e).astype(np.complex128) * ac.message((e[1], e[0])).astype(np.complex128)))


def log_amplitude(ac):
    """sum_v log(vertex scalar) - sum_e log(edge scalar), complex logs (abstract...:289-304); -inf when a scalar is exactly zero"""
    num = np.array([vertex_scalar(ac, v) for v in ac.g.vertices], dtype=complex)
    den = np.array([edge_scalar(ac, e) for e in ac.g.edges], dtype=complex)
    if np.any(num == 0) or np.any(den == 0):
        return complex(-np.inf, 0.0)
    return complex(np.sum(np.log(num)) - np.sum(np.log(den)))


def cancellation(ac):
    """max over the vertices of sum|t| / |sum t| over the terms of the vertex scalar"""
    worst = 0.0
    for v in ac.g.vertices:
        t = vertex_terms(ac, v)
        worst = max(worst, float(np.abs(t).sum() / abs(t.sum())))
    return worst


def log_amplitudes(g, tensors, configs, nsweeps, seq=None, tolerance=None, normalize=True, store=np.complex128, info=None):
    """the batch, string by string; configs: (B, nv) integers in vertex order.  info receives the per-string lists niter, diff, converged"""
    out, infos = [], []
    for row in np.asarray(configs).reshape(-1, len(g.vertices)):
        i = {}
        out.append(log_amplitude(run(g, tensors, dict(zip(g.vertices, (int(t) for t in row))), nsweeps, seq, tolerance, normalize, store, i)))
        infos.append(i)
    if info is not None:
        info.update(niter=[i["niter"] for i in infos], diff=[i["diff"] for i in infos], converged=[i["converged"] for i in infos])
    return np.array(out, dtype=complex)


# ---- inputs shared by the CPU and the GPU tests -----------------------------------------------------------------------------------------------------------------
def biased_state(g, dims, rng, d=2):
    """entries 1 + 0.5 x complex normal, as inner_ref.loopy_case: a positive part that keeps the vertex scalars from cancelling"""
    return {v: 1.0 + 0.5 * t for v, t in tensors_of(g, dims, rng, d=d).items()}


def loopy_state(name, seed=0):
    """(g, tensors) of a loopy end-to-end case of inner_ref: biased, bond dimensions 2..3"""
    import inner_ref
    g = inner_ref.LOOPY_CASES[name]()
    rng = np.random.default_rng([seed, 40 + sorted(inner_ref.LOOPY_CASES).index(name)])
    return g, biased_state(g, random_dims(g, rng, 2, 3), rng)


def grid33_state(chi, seed=0):
    """3 x 3 grid, biased, every bond chi (an int) or mixed dimensions (a list the edges cycle through)"""
    g = o.named_grid((3, 3))
    rng = np.random.default_rng([seed, 33])
    dims = {e: (chi if isinstance(chi, int) else chi[i % len(chi)]) for i, e in enumerate(g.edges)}
    return g, biased_state(g, dims, rng)


MIXED_DIMS = [1, 5, 3, 2, 7]


def freezing_state(g, chi, rng):
    """T_v[0] a product of one vector per leg (rank one: BP on the all-zeros string converges at once), T_v[1] generic and biased"""
    out = {}
    for v in g.vertices:
        z = len(g.nbrs[v])
        t = np.zeros((2,) + (chi,) * z, dtype=np.complex128)
        p = np.ones((), dtype=np.complex128)
        for _ in range(z):
            p = np.multiply.outer(p, 1.0 + 0.5 * crandn(rng, (chi,)))
        t[0] = p
        t[1] = 1.0 + 0.5 * crandn(rng, (chi,) * z)
        out[v] = t
    return out


def evolved_case():
    """(g, product state, drawn strings) of the evolved-state test: the biased chi = 1 product state on the 3 x 3 grid that one TFIM layer (evolved_layer) is applied to
    with maxdim = 3, and the eight strings drawn for it"""
    import inner_ref
    g = o.named_grid((3, 3))
    t0 = inner_ref.tensors_of(g, {e: 1 for e in g.edges}, np.random.default_rng(23), bias=1.0)
    return g, t0, random_strings(np.random.default_rng(29), g, 8)


def evolved_layer(colour_groups, vertices):
    """Rzz on every bond, colour by colour, then Rx on every vertex (unitary one-site gates after the last two-site gate: the device leaves them deferred)"""
    layer = []
    for grp in colour_groups:
        layer += [("Rzz", [a, b], 0.25) for (a, b) in grp]
    return layer + [("Rx", [v], 0.5) for v in vertices]


EVOLVED_SWEEPS = 4


def strings_that_do_not_cancel(g, tensors, drawn, seq, cap=2.0):
    """the drawn strings whose vertex scalars keep a cancellation factor <= cap after EVOLVED_SWEEPS sweeps: the end-to-end bound assumes it"""
    return np.array([x for x in drawn if cancellation(run(g, tensors, dict(zip(g.vertices, x)), EVOLVED_SWEEPS, seq=seq)) <= cap], dtype=np.int32).reshape(-1, len(g.vertices))


def sampling_case(nsamples=6):
    """(g, tensors, uniforms) of the sampling tie: the 8-vertex comb tree of tests/test_gpu_sampling.py's kind, biased chi = 3 tensors, fixed uniforms whose CPU replay
    (tests/sampling_ref.py) meets no conditional probability below SAMPLING_PMIN (tests/test_amplitude_ref_cpu.py)"""
    g = o.comb_tree((4, 2))
    rng = np.random.default_rng([2, 81])
    t = biased_state(g, {e: 3 for e in g.edges}, rng)
    return g, t, rng.random((nsamples, len(g.vertices)))


SAMPLING_PMIN = 0.05


def random_strings(rng, g, n):
    """n random bit strings, the all-zeros string in front"""
    x = rng.integers(0, 2, size=(n, len(g.vertices)))
    x[0] = 0
    return x.astype(np.int32)


# ---- bounds of the kernel-level GPU tests (tests/test_gpu_amplitudes.py), evaluated on the host --------------------------------------------------------------------
def unit_roundoff(dtype):
    """u of the accumulation: 2^-24 (ComplexF32: f32 matrix cores and fused multiply-adds) / 2^-53"""
    return 2.0 ** -24 if np.dtype(dtype) == np.complex64 else 2.0 ** -53


def dot_bound(dtype, K, mag, extra=0):
    """per entry 8 u (K + extra partials) sum|x||y|: any summation order of K products, the factor 8 for the four real products of a complex one and the rounding of
    the result (the form tests/test_gpu_inner.py uses for its Gram)"""
    return 8 * unit_roundoff(dtype) * (K + extra) * mag


def log_bound(g, dtype, factor=1.0):
    """the project's tolerance on log z (tests/test_gpu_inner.py): complex64 1e-6 (nv + ne), complex128 200 eps (nv + ne)"""
    n = len(g.vertices) + len(g.edges)
    return factor * (1e-6 if np.dtype(dtype) == np.complex64 else 200 * np.finfo(np.float64).eps) * n
