"""GPU tests of sample(psi, nsamples; alg = "bp") (reference src/sampling.jl:3-46): tnqs_sample_bp, tnqs_site_probabilities, tnqs_project_site.

Tolerances of the replay against the numpy oracle (test 1).  Measured on the MI355X, largest |p_device - p_oracle| over the steps that are compared
(margin 1e-3), see MEASURED below; each tolerance is about five times its figure, the margin ten times the tolerance and never above 1e-3."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":                      # child process of test_fused_call_equals_host_loop_without_speculation
    for _p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle"), HERE):
        if _p not in sys.path:
            sys.path.insert(0, _p)

import tnqs_amd as tn
import tnqs_oracle as o
import statevector as sv
import sampling_ref as sr
from helpers import to_oracle_graph, to_oracle_state

pytestmark = pytest.mark.gpu
L = tn.core.L

# largest |p_device - p_oracle| over the steps this test compares (i.e. at the margins below), per element type, measured on the MI355X; the figures per case are
# in profiles/r7_sample_bench.txt.  tolerance = five times the figure, margin = ten times the tolerance (capped at 1e-3)
MEASURED = {np.dtype(np.complex64): 2.24e-7, np.dtype(np.complex128): 7.2e-16}
MEASURED.update({np.dtype(np.float32): MEASURED[np.dtype(np.complex64)], np.dtype(np.float64): MEASURED[np.dtype(np.complex128)]})
TOL_PROB = {k: 5 * v for k, v in MEASURED.items()}
MARGIN = {k: min(10 * v, 1e-3) for k, v in TOL_PROB.items()}


# ---- raw entry points ------------------------------------------------------------------------------------------------------------------------------------
def sample_bp_raw(bpc, nsamples, kw, uniforms=None, seed=0):
    bo, keep = tn.core._bp_opts(bpc.graph, kw)
    nv = bpc.graph.nv()
    cfg = np.full((nsamples, nv), -1, dtype=np.int32); prob = np.full((nsamples, nv), -1.0)
    u = None if uniforms is None else np.ascontiguousarray(uniforms, dtype=np.float64)
    st = L.ApplyStats()
    L.check(L.lib.tnqs_sample_bp(bpc._h, nsamples, C.byref(bo), C.c_uint64(seed), None if u is None else u.ctypes.data_as(C.POINTER(C.c_double)),
                                 cfg.ctypes.data_as(C.POINTER(C.c_int32)), prob.ctypes.data_as(C.POINTER(C.c_double)), C.byref(st)))
    return cfg, prob, st


def host_loop(bpc, uniforms, kw):
    """the loop of tnqs_sample_bp over the public primitives: tnqs_copy, tnqs_site_probabilities, a host draw, tnqs_project_site, tnqs_bp_update"""
    g = bpc.graph; vs = list(g.vertices)
    bo, keep = tn.core._bp_opts(g, kw)
    cfg = np.zeros(uniforms.shape, dtype=np.int32); prob = np.zeros(uniforms.shape)
    for j, us in enumerate(uniforms):
        c = bpc.copy()
        for i, v in enumerate(vs):
            p = tn.site_probabilities(c, v)
            x = sr.draw(p, us[i])
            cfg[j, i], prob[j, i] = x, p[x]
            L.check(L.lib.tnqs_project_site(c._h, i, x))
            if i + 1 < len(vs):
                L.check(L.lib.tnqs_bp_update(c._h, C.byref(bo), None, None))
    return cfg, prob


def device_cache_like(oc, psi_tn):
    """device cache holding the tensors of psi_tn and the oracle cache's messages"""
    bpc = tn.BeliefPropagationCache(psi_tn)
    for e, m in oc.messages.items():
        bpc.setmessage(e, m)
    return bpc


# ---- 1. replay against the oracle ------------------------------------------------------------------------------------------------------------------------
def make_case(name, dtype):
    if name == "grid4x4":
        g, chi, ns = tn.named_grid((4, 4)), 4, 16
    elif name in ("grid3x3", "grid3x3_d3"):
        g, chi, ns = tn.named_grid((3, 3)), 3, 32
    elif name in ("comb33", "comb33_default"):
        g, chi, ns = tn.named_comb_tree((3, 3)), 4, 32
    elif name == "hh11":
        g, chi, ns = tn.heavy_hexagonal_lattice(1, 1), 4, 16
    else:
        raise KeyError(name)
    og = to_oracle_graph(g)
    psi = o.random_state(dtype, og, chi, seed=11)
    if name == "grid3x3_d3":                                   # unequal site dimensions: d = 3 at two vertices
        rng = np.random.default_rng(3)
        for v in (og.vertices[1], og.vertices[4]):
            shp = (3,) + psi.tensors[v].shape[1:]
            psi.tensors[v] = ((rng.standard_normal(shp) + 1j * rng.standard_normal(shp)) / np.sqrt(2)).astype(dtype)
    oc = o.update(o.BeliefPropagationCache(psi), maxiter=30)
    u = np.random.default_rng(7).random((ns, len(og.vertices)))
    kw = {} if name == "comb33_default" else dict(maxiter=4, tolerance=None, edge_sequence=list(oc.edge_sequence))
    return g, psi, oc, u, kw


def replay_case(name, dtype):
    """-> (largest |p_device - p_oracle| over the compared steps, samples left out, samples, configuration mismatches over the compared steps)"""
    g, psi, oc, u, kw = make_case(name, dtype)
    bpc = device_cache_like(oc, tn.TensorNetworkState(g, dict(psi.tensors)))
    assert bpc.dtype == np.dtype(dtype)
    ocfg, oprob, margin = sr.sample_ref(oc, u, **kw)
    dcfg, dprob, _ = sample_bp_raw(bpc, len(u), None if not kw else kw, uniforms=u)
    assert bpc.dtype == np.dtype(dtype)                        # a real handle stays real
    worst, left, bad = 0.0, 0, 0
    for j in range(len(u)):
        close = np.nonzero(margin[j] < MARGIN[np.dtype(dtype)])[0]
        k = int(close[0]) if len(close) else u.shape[1]
        left += k < u.shape[1]
        if k:
            worst = max(worst, float(np.max(np.abs(dprob[j, :k] - oprob[j, :k]))))
            bad += int(np.sum(dcfg[j, :k] != ocfg[j, :k]))
    return worst, left, len(u), bad


REPLAY = [(n, d) for n in ("grid4x4", "grid3x3", "comb33", "hh11") for d in (np.complex64, np.complex128)] + \
         [("comb33_default", np.complex128), ("grid3x3", np.float64), ("grid3x3_d3", np.complex128), ("grid3x3_d3", np.complex64)]


@pytest.mark.parametrize("name,dtype", REPLAY)
def test_replay_against_oracle(name, dtype):
    """same state, messages, uniforms, edge sequence and sweep count on both sides: configurations exactly, step probabilities to TOL_PROB; a sample leaves the
    comparison at the first step whose uniform lies within MARGIN of a cdf boundary of the oracle (at most 10 % of the samples may)"""
    worst, left, n, bad = replay_case(name, dtype)
    print(f"replay {name} {np.dtype(dtype).name}: max |dp| = {worst:.3e}, left out {left}/{n}, config mismatches {bad}")
    assert left <= 0.1 * n, (left, n)
    assert bad == 0
    assert worst <= TOL_PROB[np.dtype(dtype)], worst


# ---- 2. fused call = host loop ---------------------------------------------------------------------------------------------------------------------------
def fused_vs_loop():
    g = tn.named_grid((4, 4))
    psi = tn.random_tensornetworkstate(np.complex64, g, bond_dimension=4, seed=21)
    bpc = tn.symmetrize_and_normalize(tn.update(tn.BeliefPropagationCache(psi), maxiter=40, tolerance=1e-7))
    before = {e: bpc.message(e) for (a, b) in g.edges for e in ((a, b), (b, a))}
    t_before = bpc.tensor(g.vertices[5])
    u = np.random.default_rng(17).random((6, g.nv()))
    kw = bpc.default_bp_update_kwargs()                        # tolerance on
    assert kw["tolerance"] is not None
    fcfg, fprob, st = sample_bp_raw(bpc, len(u), kw, uniforms=u)
    hcfg, hprob = host_loop(bpc, u, kw)
    assert np.array_equal(fcfg, hcfg)
    assert np.array_equal(fprob, hprob), float(np.max(np.abs(fprob - hprob)))       # to the last bit
    assert st.n_bp_updates == len(u) * (g.nv() - 1) and st.n_bp_sweeps >= st.n_bp_updates
    for e, m in before.items():
        assert np.array_equal(bpc.message(e), m), e
    assert np.array_equal(bpc.tensor(g.vertices[5]), t_before)
    assert all(bpc._site_dim(v) == 2 for v in g.vertices)
    assert fcfg.min() >= 0 and fcfg.max() <= 1 and len({tuple(r) for r in fcfg}) > 1
    return True


def test_fused_call_equals_host_loop():
    assert fused_vs_loop()


def test_fused_call_equals_host_loop_without_speculation():
    env = dict(os.environ, TNQS_NO_SPECULATION="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "fused-vs-loop"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fused-vs-loop OK" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


# ---- 3. exact on a tree ----------------------------------------------------------------------------------------------------------------------------------
def test_sampling_is_exact_on_a_tree():
    g = tn.named_comb_tree((4, 2))
    assert g.nv() == 8 and g.is_tree()
    psi = tn.random_tensornetworkstate(np.complex128, g, bond_dimension=4, seed=31)
    amp = sv.tns_to_statevector(to_oracle_state(psi))
    exact = np.abs(amp) ** 2 / np.sum(np.abs(amp) ** 2)
    N = 2000
    # gauge_state=False: the comparison is with the state handed in.  The symmetric gauge adds its regularisation (10 eps) to the message eigenvalues before the
    # roots and so returns a slightly different state: with it the same run measured max |q - exact| = 1.2e-10 (relative 1.3e-8), without it 1.2e-16.  The
    # gauged run is checked below through its marginals.
    bits, logq = tn.sample_with_probabilities(psi, N, seed=5, gauge_state=False)
    assert len(bits) == N and set(bits[0]) == set(g.vertices)
    x = np.array([[b[v] for v in g.vertices] for b in bits])
    q = np.exp(logq)
    ex = exact[tuple(x.T)]
    print(f"tree: max |q - exact| = {np.max(np.abs(q - ex)):.3e}")
    assert np.max(np.abs(q - ex)) <= TOL_PROB[np.dtype(np.complex128)]
    for i in range(g.nv()):
        p1 = float(np.sum(np.moveaxis(exact, i, 0)[1]))
        assert abs(x[:, i].mean() - p1) <= 5 * np.sqrt(p1 * (1 - p1) / N), (i, x[:, i].mean(), p1)
    bits2, logq2 = tn.sample_with_probabilities(psi, 64, seed=5, gauge_state=False)
    assert bits2 == bits[:64] and np.array_equal(logq2, logq[:64])               # counter-based: (seed, sample, step) alone
    bits3, _ = tn.sample_with_probabilities(psi, 64, seed=6, gauge_state=False)
    assert bits3 != bits2
    assert tn.sample(psi, 3, seed=5, gauge_state=False) == bits[:3]
    # the default call (updated, gauged): q against the exact probability at a bound from the gauge itself.  The leaf bonds of this tree are rank-deficient
    # (chi = 4 against a 2-dimensional leaf), so the regularisation 10 eps added to a zero message eigenvalue enters the roots as sqrt(10 eps) = 4.7e-8; a
    # probability is an amplitude squared (factor 2) and the tree has 7 bonds: 7 x 2 x 4.7e-8 = 6.6e-7 relative (measured: 1.3e-8)
    gb, glogq = tn.sample_with_probabilities(psi, 400, seed=9)
    gx = np.array([[b[v] for v in g.vertices] for b in gb])
    grel = float(np.max(np.abs(np.exp(glogq) / exact[tuple(gx.T)] - 1)))
    print(f"tree, gauged: max |q / exact - 1| = {grel:.3e}")
    assert grel <= 6.6e-7


# ---- 4. the kernels on the engine's fast shapes ----------------------------------------------------------------------------------------------------------
def colour_seq(g):
    seq = []
    for grp in tn.edge_color(g):
        seq += [(a, b) for (a, b) in grp] + [(b, a) for (a, b) in grp]
    return seq


@pytest.mark.parametrize("shape", ["grid4x4_chi32", "deg3_chi16"])
def test_bp_update_on_projected_sites_matches_oracle(shape):
    """half of the vertices projected, then two sweeps over an explicit sequence: every message against the oracle at the bound test_gpu_parity.py uses
    for ComplexF32 BP updates at these shapes (5e-5); the 1 x 1 rdm of a projected vertex is its vertex scalar"""
    if shape == "grid4x4_chi32":
        g, chi = tn.named_grid((4, 4)), 32
    else:
        g, chi = tn.named_grid((4, 2), periodic=True), 16
        assert all(g.degree(v) == 3 for v in g.vertices)
    psi = tn.random_tensornetworkstate(np.complex64, g, bond_dimension=chi, seed=11)
    for v in g.vertices:
        psi.tensors[v] = (psi.tensors[v] / np.linalg.norm(psi.tensors[v])).astype(np.complex64)
    bpc = tn.BeliefPropagationCache(psi)
    chosen = [v for v in g.vertices if (v[0] + v[1]) % 2 == 0]
    assert len(chosen) == g.nv() // 2
    ops = to_oracle_state(psi)
    for k, v in enumerate(chosen):
        L.check(L.lib.tnqs_project_site(bpc._h, g.index[v], k % 2))
        ops.tensors[v] = ops.tensors[v][k % 2:k % 2 + 1]
    for v in g.vertices:
        assert bpc._site_dim(v) == (1 if v in chosen else 2)
        assert np.array_equal(bpc.tensor(v), ops.tensors[v])
    kw = dict(maxiter=2, tolerance=None, edge_sequence=colour_seq(g))
    out = tn.update(bpc, **kw)
    oc = o.update(o.BeliefPropagationCache(ops), **kw)
    worst = 0.0
    for (a, b) in g.edges:
        for e in ((a, b), (b, a)):
            m, mo = out.message(e), oc.message(e)
            worst = max(worst, np.max(np.abs(m - mo)) / np.max(np.abs(mo)))
    print(f"{shape}: worst message error {worst:.3e}")
    assert worst <= 5e-5
    vsc = tn.vertex_scalars(out)
    for v in chosen[:3]:
        rho = np.zeros((1, 1), dtype=np.complex128)
        L.check(L.lib.tnqs_rdm_1site(out._h, g.index[v], rho.ctypes.data_as(C.POINTER(C.c_double))))
        # (one launch per vertex against one batched launch: f64 sums of the same <= 2^20 terms in another order, sqrt(n) eps ~ 2e-13)
        assert abs(rho[0, 0] - vsc[g.index[v]]) <= 1e-12 * abs(vsc[g.index[v]])
        assert abs(rho[0, 0] - o.vertex_scalar(oc, v)) <= 5e-5 * abs(o.vertex_scalar(oc, v))
        assert np.array_equal(tn.site_probabilities(out, v), [1.0])


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("d", [2, 3, 4])
def test_site_probabilities_match_rdm_and_numpy(dtype, d):
    g = tn.named_grid((3, 2))
    tol = TOL_PROB[np.dtype(dtype)]
    for scale in (1e-4, 1.0, 1e4):
        rng = np.random.default_rng(100 + d)
        tensors = {}
        for v in g.vertices:
            shp = (d,) + (5,) * g.degree(v)
            tensors[v] = (scale * (rng.standard_normal(shp) + 1j * rng.standard_normal(shp))).astype(dtype)
        psi = tn.TensorNetworkState(g, tensors)
        bpc = tn.update(tn.BeliefPropagationCache(psi), maxiter=3, tolerance=None)
        oc = o.BeliefPropagationCache(o.TensorNetworkState(to_oracle_graph(g), {v: tensors[v].astype(np.complex128) for v in g.vertices}))
        for e in [(a, b) for (a, b) in g.edges] + [(b, a) for (a, b) in g.edges]:
            oc.messages[e] = bpc.message(e).astype(np.complex128)
        for v in g.vertices:
            p = tn.site_probabilities(bpc, v)
            assert p.shape == (d,) and abs(p.sum() - 1) < 1e-14
            rho = tn.rdm(bpc, v)
            assert np.max(np.abs(p - np.real(np.diag(rho)))) <= tol, (scale, v)
            assert np.max(np.abs(p - sr.site_probabilities(oc, v))) <= tol, (scale, v, p, sr.site_probabilities(oc, v))


# ---- 5. state bookkeeping --------------------------------------------------------------------------------------------------------------------------------
def test_projection_honours_a_deferred_gate_and_leaves_the_original_alone():
    g = tn.named_grid((3, 3))
    psi = tn.random_tensornetworkstate(np.complex64, g, bond_dimension=3, seed=41)
    bpc = tn.update(tn.BeliefPropagationCache(psi), maxiter=5, tolerance=None)
    v = g.vertices[4]
    info = {}
    rot, _ = tn.apply_gates([("X", [v])], bpc, apply_kwargs=dict(normalize_tensors=False), update_cache=False, info=info)
    assert info["n_deferred_1site"] == 1                       # the gate is pending, not applied
    pr = rot.project(v, 0)
    assert pr._site_dim(v) == 1 and rot._site_dim(v) == 2 and bpc._site_dim(v) == 2
    assert np.array_equal(pr.tensor(v), psi.tensors[v][1:2])   # X swaps the two configurations: the slice of the ROTATED tensor
    assert np.array_equal(rot.tensor(v), psi.tensors[v][::-1])
    assert np.array_equal(bpc.tensor(v), psi.tensors[v])
    for w in g.neighbors(v):
        assert pr.bond_dim(v, w) == 3 and np.array_equal(pr.message((w, v)), bpc.message((w, v)))
    # a pending scale factor (normalize_tensors after a two-site gate) is kept beside the slice
    a, b = g.vertices[0], g.vertices[1]
    gated, _ = tn.apply_gates([("Rzz", [a, b], 0.3)], bpc, apply_kwargs=dict(maxdim=3, normalize_tensors=True))
    sliced = gated.project(a, 1).tensor(a)                     # (taken first: reading gated's tensor applies its pending factor)
    assert np.allclose(sliced, gated.tensor(a)[1:2], rtol=1e-6, atol=0)


def test_error_codes_and_the_handle_stays_usable():
    g = tn.named_grid((2, 2))
    psi = tn.random_tensornetworkstate(np.complex128, g, bond_dimension=2, seed=51)
    bpc = tn.update(tn.BeliefPropagationCache(psi))
    h = bpc._h
    assert L.lib.tnqs_project_site(h, 0, 2) == L.ERR_INVALID and L.lib.tnqs_project_site(h, 0, -1) == L.ERR_INVALID
    assert L.lib.tnqs_project_site(h, 9, 0) == L.ERR_INVALID
    d = C.c_int()
    assert L.lib.tnqs_site_dim(h, 0, C.byref(d)) == L.OK and d.value == 2
    assert L.lib.tnqs_site_dim(h, -1, C.byref(d)) == L.ERR_INVALID
    p0 = tn.site_probabilities(bpc, g.vertices[0])             # still usable
    pr = bpc.project(g.vertices[0], 1)
    with pytest.raises(tn.TnqsError, match="projected"):
        tn.apply_gates([("X", [g.vertices[0]])], pr)
    with pytest.raises(tn.TnqsError, match="site dimension mismatch"):
        pr._set_tensor(g.vertices[0], psi.tensors[g.vertices[0]])
    pr._set_tensor(g.vertices[0], psi.tensors[g.vertices[0]][0:1])              # d = 1: the current site dimension
    assert np.array_equal(pr.tensor(g.vertices[0]), psi.tensors[g.vertices[0]][0:1])
    # tr rho = 0: a zero tensor
    zero = bpc.copy(); zero._set_tensor(g.vertices[1], np.zeros_like(psi.tensors[g.vertices[1]]))
    out = np.zeros(2)
    assert L.lib.tnqs_site_probabilities(zero._h, 1, out.ctypes.data_as(C.POINTER(C.c_double))) == L.ERR_NUMERIC
    with pytest.raises(tn.TnqsDomainError):
        sample_bp_raw(zero, 2, dict(maxiter=2, tolerance=None), uniforms=np.full((2, 4), 0.5))
    assert np.array_equal(tn.site_probabilities(zero, g.vertices[0]).shape, (2,))
    # a diagonal entry far below zero: a message that is not positive
    neg = bpc.copy()
    w = g.neighbors(g.vertices[0])[0]
    neg.setmessage((w, g.vertices[0]), np.diag([1.0, -3.0]).astype(np.complex128))
    assert L.lib.tnqs_site_probabilities(neg._h, 0, out.ctypes.data_as(C.POINTER(C.c_double))) == L.ERR_NUMERIC
    # uniforms outside [0, 1) are refused by the library too
    cfg = np.zeros((1, 4), dtype=np.int32); bad = np.full((1, 4), 1.0)
    assert L.lib.tnqs_sample_bp(h, 1, None, C.c_uint64(0), bad.ctypes.data_as(C.POINTER(C.c_double)), cfg.ctypes.data_as(C.POINTER(C.c_int32)), None, None) == L.ERR_INVALID
    assert np.array_equal(tn.site_probabilities(bpc, g.vertices[0]), p0)


def test_sharded_handles_are_refused():
    import torch
    g = tn.named_grid((2, 2))
    psi = tn.random_tensornetworkstate(np.complex64, g, bond_dimension=2, seed=61)
    bpc = tn.BeliefPropagationCache(psi)
    buf = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    cb = L.ALLGATHER_FN(lambda ctx, base, nbytes, nranks: -1)
    owner, op = L.i32([0, 0, 1, 1])
    L.check(L.lib.tnqs_set_sharding(bpc._h, 0, 2, op, cb, None, C.c_void_p(buf.data_ptr()), buf.numel()))
    assert L.lib.tnqs_project_site(bpc._h, 0, 0) == L.ERR_UNSUPPORTED
    cfg = np.zeros((1, 4), dtype=np.int32)
    assert L.lib.tnqs_sample_bp(bpc._h, 1, None, C.c_uint64(0), None, cfg.ctypes.data_as(C.POINTER(C.c_int32)), None, None) == L.ERR_UNSUPPORTED


if __name__ == "__main__":
    if sys.argv[1:] == ["fused-vs-loop"]:
        assert fused_vs_loop()
        print("fused-vs-loop OK")
