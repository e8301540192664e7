"""GPU tests of the two-site reduced density matrices of bonds (rdm_edges / expect_edges / rdm(bpc, [u, v]); tnqs_rdm_edges): the bond-contraction kernel
of csrc/kernels_rdm.hip through its debug entry point against extended-precision numpy, the two-operand matrix-core Gram in the shape the feature uses,
tnqs_rdm_edges against tests/rdm_edges_ref.py on IDENTICAL inputs (tensors and messages read back from a copy of the cache after the call), exactness on a
tree, the cross-check with the region contraction of expect(), batching, and the contract of the C entry point.

Bounds (derived, none of them measured on the kernels):
  edge_rdm kernel   |dev - ref| <= 8 2^-53 (chunks_u + chunks_v + chi^2) fac^2 sum_{a,a'} |E_u| |E_v| per entry: every chunk sum and the bond sum run in f64,
                    whatever the partial type
  two-operand Gram  1e-6 of the largest entry (f32 accumulation, the bound the project's kernel tests hold for 64-term products)
  tnqs_rdm_edges    on NORMALISED entries: complex64 the project's 1e-5; complex128 max(200 eps, 10 x the CPU baseline of tests/test_rdm_edges_ref_cpu.py)
  tree exactness    200 eps for float64 / complex128 (tests/test_oracle_pins.py test_bp_exact_on_trees), 1e-5 for float32 / complex64"""
import ctypes as C
import functools

import numpy as np
import pytest

import tnqs_amd as tn
import tnqs_oracle as o
import statevector as sv
import rdm_edges_ref as er
from tnqs_amd import core
from test_rdm_edges_ref_cpu import REGION_BASELINE

pytestmark = pytest.mark.gpu
lib = C.CDLL(tn.LIB_PATH)
ERR_INVALID = -1
EPS64 = float(np.finfo(np.float64).eps)
TOL = {np.dtype(np.complex64): 1e-5, np.dtype(np.complex128): max(200 * EPS64, 10 * REGION_BASELINE),
       np.dtype(np.float32): 1e-5, np.dtype(np.float64): 200 * EPS64}


def _ints(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.int32))


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _rand(rng, n, dt):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(dt)


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------------------
#        (d_u, d_v, chi, chunks_u, chunks_v)
ITEMS = [(2, 2, 1, 1, 1), (2, 2, 3, 1, 5), (1, 2, 3, 2, 1), (2, 3, 5, 3, 2), (2, 2, 32, 7, 4), (2, 2, 64, 2, 2)]
SCALES = [(0.75, 1.5), (0.0, 0.0), (0.0, 1.25), (1.75, 0.5), (0.875, 1.125), (1.5, 0.625)]      # 0: a null pointer (no factor pending)
GUARD = 40


def _env4(partial, d, chi):
    """the chunks of one end summed in extended precision, as E[s, a, s', a']; partial: [chunk][(s + d a) + d chi (s' + d a')]"""
    e = np.sum(partial.astype(np.clongdouble), axis=0)
    return e.reshape(chi, d, chi, d).transpose(3, 2, 1, 0)       # C order of the flat index: (a', s', a, s)


@pytest.mark.parametrize("ptype", [0, 1])
def test_edge_rdm_kernel_against_extended_precision(ptype):
    pdt = np.complex64 if ptype == 0 else np.complex128
    rng = np.random.default_rng(11 + ptype)
    pu = [_rand(rng, cu * (du * chi) ** 2, pdt).reshape(cu, -1) for (du, dv, chi, cu, cv) in ITEMS]
    pv = [_rand(rng, cv * (dv * chi) ** 2, pdt).reshape(cv, -1) for (du, dv, chi, cu, cv) in ITEMS]
    tot = GUARD + sum((du * dv) ** 2 + GUARD for (du, dv, chi, cu, cv) in ITEMS)
    out = np.full(tot, np.nan + 1j * np.nan, dtype=np.complex128)
    col = lambda k: _p(_ints([it[k] for it in ITEMS]))
    su = np.array([s[0] for s in SCALES]); svv = np.array([s[1] for s in SCALES])
    rc = lib.tnqs_dbg_edge_rdm(ptype, len(ITEMS), col(0), col(1), col(2), col(3), col(4), _p(np.concatenate([x.ravel() for x in pu])),
                               _p(np.concatenate([x.ravel() for x in pv])), _p(su), _p(svv), _p(out), GUARD)
    assert rc == 0, lib.tnqs_last_error()
    off = GUARD
    for (du, dv, chi, cu, cv), xu, xv, (fu, fv) in zip(ITEMS, pu, pv, SCALES):
        dd = du * dv
        got = out[off:off + dd * dd].reshape(dd, dd, order="F")
        eu, ev = _env4(xu, du, chi), _env4(xv, dv, chi)
        fac2 = np.longdouble((fu or 1.0) ** 2 * (fv or 1.0) ** 2)
        ref = (np.einsum("saSb,taTb->stST", eu, ev) * fac2).reshape(dd, dd)
        mag = (np.einsum("saSb,taTb->stST", np.abs(eu), np.abs(ev)) * fac2).reshape(dd, dd)
        bound = 8 * 2.0 ** -53 * (cu + cv + chi * chi) * mag.astype(np.float64)
        err = np.abs(got - ref.astype(np.complex128))
        print(f"MEASURED edge_rdm {pdt.__name__} {(du, dv, chi, cu, cv)}: max |dev - ref| / bound = {np.max(err / bound):.3e} (max bound {np.max(bound):.3e})")
        assert np.all(np.isfinite(got)) and np.all(err <= bound)
        assert np.all(np.isnan(out[off - GUARD:off].real))                   # the guard band in front of the item
        off += dd * dd + GUARD
    assert np.all(np.isnan(out[off - GUARD:].real)) and off == tot           # and the one behind the last


def test_edge_rdm_kernel_refuses_a_bond_beyond_its_lds():
    z = np.zeros(1, dtype=np.complex64); one = np.ones(1); out = np.zeros(16, dtype=np.complex128)
    rc = lib.tnqs_dbg_edge_rdm(0, 1, _p(_ints([2])), _p(_ints([2])), _p(_ints([4096])), _p(_ints([1])), _p(_ints([1])), _p(z), _p(z), _p(one), _p(one), _p(out), 0)
    assert rc == -2                                                          # TNQS_ERR_UNSUPPORTED before anything is allocated


# ---- 2. the two-operand Gram in the shape this feature uses ----------------------------------------------------------------------------------
def _gram_ref(x, y, D, PA, K, PB):
    KK = D * K
    tx = x.reshape(PB, K, PA, D).transpose(1, 3, 2, 0).reshape(KK, -1).astype(np.complex128)
    ty = y.reshape(PB, K, PA, D).transpose(1, 3, 2, 0).reshape(KK, -1).astype(np.complex128)
    return (tx @ ty.conj().T).T.reshape(-1)                                  # out[i + KK j], i = s + D k


def test_two_operand_gram_of_a_kept_site_index_and_leg():
    """E_u is a Gram with Y != X that keeps the site index (D = 2) and one leg: 32-dimensional (KK = 64, launch_mfma_gram64 through tnqs_dbg_gram_mfma, alone and
    with other kept legs in the same launch) and 16-dimensional (KK = 32: the engine sends it to launch_mfma_gram32, reached through tnqs_dbg_gram)"""
    rng = np.random.default_rng(3)
    for items in ([(2, 32, 32, 32)], [(2, 32, 32, 32), (2, 3, 20, 7), (2, 1, 32, 33)]):
        xs = [_rand(rng, int(np.prod(s)), np.complex64) for s in items]; ys = [_rand(rng, int(np.prod(s)), np.complex64) for s in items]
        refs = [_gram_ref(x, y, *s) for x, y, s in zip(xs, ys, items)]
        out = np.zeros(sum(r.size for r in refs), dtype=np.complex64)
        rc = lib.tnqs_dbg_gram_mfma(len(items), _p(_ints(items).ravel()), _p(np.concatenate(xs)), _p(np.concatenate(ys)), _p(out), 0, None)
        assert rc == 0, lib.tnqs_last_error()
        for s, got, ref in zip(items, np.split(out, np.cumsum([r.size for r in refs])[:-1]), refs):
            err = np.max(np.abs(got - ref)) / np.max(np.abs(ref))
            print(f"MEASURED two-operand gram64 {s} in a launch of {len(items)}: {err:.3e}")
            assert err < 1e-6
    D, PA, K, PB = 2, 16, 16, 16
    x, y = _rand(rng, D * PA * K * PB, np.complex64), _rand(rng, D * PA * K * PB, np.complex64)
    out = np.zeros((D * K) ** 2, dtype=np.complex64)
    assert lib.tnqs_dbg_gram(0, D, PA, K, PB, _p(x), _p(y), _p(out), 0, 1) == 0, lib.tnqs_last_error()
    ref = _gram_ref(x, y, D, PA, K, PB)
    err = np.max(np.abs(out - ref)) / np.max(np.abs(ref))
    print(f"MEASURED two-operand gram32 {(D, PA, K, PB)}: {err:.3e}")
    assert err < 1e-6


# ---- 3. tnqs_rdm_edges on identical inputs ---------------------------------------------------------------------------------------------------
def _read_back(bpc):
    """tensors, messages and neighbour lists of what the cache holds, from a COPY (reading a tensor materialises what is pending on it)"""
    cp = bpc.copy(); g = cp.graph
    ts = {v: cp.tensor(v).astype(np.complex128) for v in g.vertices}
    ms = {e: cp.message(e).astype(np.complex128) for (a, b) in g.edges for e in ((a, b), (b, a))}
    return ts, ms, {v: list(g.neighbors(v)) for v in g.vertices}


@functools.lru_cache(maxsize=None)
def _grid_cache(dt, chi, projected):
    g = tn.named_grid((3, 3))
    psi = tn.random_tensornetworkstate(dt, g, chi, seed=7 + chi)
    bpc = tn.update(tn.BeliefPropagationCache(psi), maxiter=40, tolerance=1e-6 if dt == np.complex64 else 1e-12)
    return bpc.project((2, 1), 1) if projected else bpc


def _worst_normalised(mats, req, ref_of):
    worst = 0.0
    for e, m in zip(req, mats):
        r = ref_of(e)
        assert m.shape == r.shape
        worst = max(worst, float(np.max(np.abs(m / np.trace(m) - r / np.trace(r)))))
    return worst


@pytest.mark.parametrize("dt,chi", [(np.complex64, 3), (np.complex128, 3), (np.complex64, 16), (np.complex64, 32)])
@pytest.mark.parametrize("projected", [False, True])
def test_rdm_edges_against_the_reference_on_identical_inputs(dt, chi, projected):
    bpc = _grid_cache(dt, chi, projected)
    req, mats = core._rdm_edges_raw(bpc, None)
    assert req == list(bpc.graph.edges)
    ts, ms, nb = _read_back(bpc)
    worst = _worst_normalised(mats, req, lambda e: er.rdm_edge(ts, ms, nb, *e))
    if projected:
        assert sorted(m.shape[0] for m in mats) == [2] * 3 + [4] * 9        # (2, 1) has three bonds
    print(f"MEASURED rdm_edges {np.dtype(dt).name} 3x3 chi {chi}{' one vertex projected' if projected else ''}: max normalised deviation {worst:.3e} (bound {TOL[np.dtype(dt)]:.1e})")
    assert worst <= TOL[np.dtype(dt)]
    # the public form: normalised, keyed by the edge
    pub = tn.rdm_edges(bpc)
    assert list(pub) == req and all(abs(np.trace(m) - 1) < 1e-12 for m in pub.values())


# ---- 4. exact on a tree ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64, np.complex64, np.complex128])
def test_rdm_of_a_bond_is_exact_on_the_comb_tree(dt):
    g = tn.named_comb_tree((3, 3))
    psi = tn.random_tensornetworkstate(dt, g, 3, seed=5)
    bpc = tn.update(tn.BeliefPropagationCache(psi))
    og = o.Graph(list(g.vertices), list(g.edges))
    vec = sv.tns_to_statevector(o.TensorNetworkState(og, {v: psi.tensors[v].astype(np.complex128) for v in g.vertices}))
    worst = 0.0
    for (u, v) in g.edges:
        m = np.moveaxis(vec, [og.pos[u], og.pos[v]], [0, 1]).reshape(4, -1)
        exact = m @ m.conj().T
        exact = exact / np.trace(exact)
        for pair in ([u, v], [v, u]):
            got = tn.rdm(bpc, pair)
            want = exact if pair[0] == u else exact.reshape(2, 2, 2, 2).transpose(1, 0, 3, 2).reshape(4, 4)
            worst = max(worst, float(np.max(np.abs(got - want))))
    print(f"MEASURED rdm(bpc, [u, v]) {np.dtype(dt).name} comb tree: max |bp - exact| = {worst:.3e} (bound {TOL[np.dtype(dt)]:.1e})")
    assert worst <= TOL[np.dtype(dt)]
    assert tn.rdm(bpc, (1, 1)).shape == (2, 2)                               # a vertex (here a tuple) keeps its path


# ---- 5. cross-check with the region contraction of expect() ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_expect_edges_equals_the_loop_of_expect_calls(dt):
    bpc = _grid_cache(dt, 3, False)
    got = tn.expect_edges(bpc, "ZZ")
    want = np.array([tn.expect(bpc, ("ZZ", [u, v])) for (u, v) in bpc.graph.edges])
    worst = float(np.max(np.abs(got - want)))
    print(f"MEASURED expect_edges ZZ {np.dtype(dt).name} 3x3 chi 3: max |batched - expect()| = {worst:.3e} (bound {TOL[np.dtype(dt)]:.1e})")
    assert got.shape == (12,) and worst <= TOL[np.dtype(dt)]
    z, x = tn.gate_matrix("Z"), tn.gate_matrix("X")
    some = list(bpc.graph.edges)[:3]
    a = tn.expect_edges(bpc, (z, x), some); b = tn.expect_edges(bpc, np.kron(z, x), some); c = tn.expect_edges(bpc, "ZX", some)
    assert np.max(np.abs(a - b)) < 1e-12 and np.max(np.abs(a - c)) < 1e-12
    assert np.max(np.abs(a - np.array([tn.expect(bpc, ("ZX", [u, v])) for (u, v) in some]))) <= TOL[np.dtype(dt)]


# ---- 6. batching -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_batches_under_a_workspace_bound(dt):
    bpc = _grid_cache(dt, 3, False)
    g = bpc.graph
    one_chain = 2 * 2 * 3 ** 4 * np.dtype(dt).itemsize                       # the two temporaries of the centre vertex's chain
    out = np.zeros(12 * 16, dtype=np.complex128); nb = C.c_int(0)
    rc = lib.tnqs_dbg_rdm_edges_ws(bpc._h, 0, None, None, _p(out), C.c_int64(int(one_chain)), C.byref(nb))
    assert rc == 0, lib.tnqs_last_error()
    assert 1 < nb.value <= 24
    ts, ms, nbrs = _read_back(bpc)
    mats = [out[16 * i:16 * (i + 1)].reshape(4, 4, order="F") for i in range(12)]
    worst = _worst_normalised(mats, list(g.edges), lambda e: er.rdm_edge(ts, ms, nbrs, *e))
    print(f"MEASURED rdm_edges {np.dtype(dt).name} in {nb.value} batches: max normalised deviation {worst:.3e} (bound {TOL[np.dtype(dt)]:.1e})")
    assert worst <= TOL[np.dtype(dt)]
    nb1 = C.c_int(0)
    assert lib.tnqs_dbg_rdm_edges_ws(bpc._h, 0, None, None, _p(out), C.c_int64(1 << 30), C.byref(nb1)) == 0 and nb1.value == 1


# ---- 7. the contract of the entry point ------------------------------------------------------------------------------------------------------
def test_orientation_repeats_empty_calls_and_errors():
    bpc = _grid_cache(np.complex64, 3, True)                                 # (2, 1) has site dimension 1
    g = bpc.graph
    u, v, w = (1, 1), (2, 1), (3, 1)
    req, mats = core._rdm_edges_raw(bpc, [(u, v), (v, u), (u, v), (v, w), (w, v)])
    assert [m.shape for m in mats] == [(2, 2)] * 5
    assert np.array_equal(mats[2], mats[0])                                  # a repeat is answered again
    assert np.array_equal(mats[1], mats[0].reshape(2, 1, 2, 1).transpose(1, 0, 3, 2).reshape(2, 2))
    assert np.array_equal(mats[4], mats[3].reshape(1, 2, 1, 2).transpose(1, 0, 3, 2).reshape(2, 2))
    full = _grid_cache(np.complex64, 3, False)
    r2, m2 = core._rdm_edges_raw(full, [((1, 1), (1, 2)), ((1, 2), (1, 1))])
    assert np.array_equal(m2[1], m2[0].reshape(2, 2, 2, 2).transpose(1, 0, 3, 2).reshape(4, 4)) and not np.array_equal(m2[1], m2[0])
    # an empty call
    z = _ints([0]); out = np.zeros(16, dtype=np.complex128)
    assert lib.tnqs_rdm_edges(full._h, 0, _p(z), _p(z), _p(out)) == 0 and not out.any()
    assert tn.rdm_edges(full, []) == {} and tn.expect_edges(full, "ZZ", []).shape == (0,)
    # not an edge, a bad vertex
    a, b = _ints([g.index[(1, 1)]]), _ints([g.index[(3, 3)]])
    assert lib.tnqs_rdm_edges(full._h, 1, _p(a), _p(b), _p(out)) == ERR_INVALID
    assert lib.tnqs_rdm_edges(full._h, 1, _p(a), _p(_ints([99])), _p(out)) == ERR_INVALID
    assert lib.tnqs_rdm_edges(full._h, 1, _p(a), _p(a), _p(out)) == ERR_INVALID
    assert lib.tnqs_rdm_edges(full._h, -1, _p(a), _p(b), _p(out)) == ERR_INVALID
    with pytest.raises(tn.TnqsArgumentError, match="only single vertices and bonds"):
        tn.rdm(full, [(1, 1), (3, 3)])


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_the_handle_is_left_as_it_was(dt):
    bpc = _grid_cache(dt, 3, False).copy()
    g = bpc.graph
    before_t = {v: bpc.tensor(v) for v in g.vertices}
    before_m = {e: bpc.message(e) for (a, b) in g.edges for e in ((a, b), (b, a))}
    tn.rdm_edges(bpc); tn.expect_edges(bpc, "XX")
    assert all(np.array_equal(bpc.tensor(v), before_t[v]) for v in g.vertices)
    assert all(np.array_equal(bpc.message(e), m) for e, m in before_m.items())


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_deferred_gates_and_pending_scales_are_part_of_the_answer(dt):
    """after a layer that ends in one-site gates (deferred) on normalised tensors (a pending scale factor), the UN-normalised matrices are those of the tensors
    the cache hands out afterwards"""
    g = tn.named_grid((3, 3))
    groups = tn.edge_color(g, 4)
    layer = [("Rx", [v], 0.3) for v in g.vertices]
    for grp in groups:
        layer += [("Rzz", [a, b], 0.25) for (a, b) in grp]
    layer += [("Rx", [v], 0.5) for v in g.vertices]
    bpkw = dict(maxiter=50, tolerance=1e-7 if dt == np.complex64 else 1e-12)
    psi0 = tn.tensornetworkstate(dt, lambda v: "↑", g)
    bpc = tn.update(tn.BeliefPropagationCache(psi0), **bpkw)
    for _ in range(2):
        bpc, _errs = tn.apply_gates(layer, bpc, apply_kwargs=dict(maxdim=3, cutoff=1e-10, normalize_tensors=True), bp_update_kwargs=bpkw)
    f = C.c_double(1.0); pending = []
    for v in g.vertices:
        assert lib.tnqs_dbg_pending_scale(bpc._h, g.index[v], C.byref(f)) == 0
        pending.append(f.value)
    assert any(x != 1.0 for x in pending), pending
    req, mats = core._rdm_edges_raw(bpc, None)
    ts, ms, nb = _read_back(bpc)
    worst = 0.0
    for e, m in zip(req, mats):
        r = er.rdm_edge(ts, ms, nb, *e)
        worst = max(worst, float(np.max(np.abs(m - r)) / np.max(np.abs(r))))
    print(f"MEASURED rdm_edges {np.dtype(dt).name} after a layer, un-normalised: max |dev - ref| / max |ref| = {worst:.3e} (bound {TOL[np.dtype(dt)]:.1e}; pending scales {min(pending):.3g} .. {max(pending):.3g})")
    assert worst <= TOL[np.dtype(dt)]
