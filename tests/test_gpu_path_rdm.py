"""GPU tests of the two-site reduced density matrices of the ends of paths (rdm_paths / rdm_pairs / expect_pairs / correlation_function; tnqs_rdm_paths): the apply
kernel of csrc/kernels_rdm.hip (the source's environment through a transfer matrix) through its debug entry point against extended-precision numpy, the bond
contraction with one partial type per end, tnqs_rdm_paths against tests/path_rdm_ref.py on IDENTICAL inputs (tensors and messages read back from a copy of the cache),
exactness on a tree, the cross-checks with expect() and rdm_edges, batching, pending scales, and the contract of the C entry point.

Bounds (derived, none of them measured on the kernels):
  path_apply kernel  per entry of the SUM of the output chunks: |dev - ref| <= 8 2^-53 (chunks_in + chi_a^2) fac^2 sum_{a,a'} |L| |T|: the chunk sums and the column sum
                     run in f64 whatever the types, and a float T widens exactly
  mixed edge_rdm     the bound of tests/test_gpu_rdm_edges.py: 8 2^-53 (chunks_u + chunks_v + chi^2) fac^2 sum |E_u| |E_v|
  tnqs_rdm_paths     on NORMALISED entries: complex64 the project's 1e-5; complex128 max(200 eps, 10 x the CPU baseline of tests/test_path_rdm_ref_cpu.py)
  tree exactness     200 eps for float64 / complex128, 1e-5 for float32 / complex64"""
import ctypes as C
import functools

import numpy as np
import pytest

import tnqs_amd as tn
import tnqs_oracle as o
import statevector as sv
import path_rdm_ref as pr
from tnqs_amd import core
from test_path_rdm_ref_cpu import PATH_BASELINE, GRID_PATHS, TREE_PATHS
from test_gpu_rdm_edges import ITEMS as EDGE_ITEMS, SCALES as EDGE_SCALES, _env4, _read_back

pytestmark = pytest.mark.gpu
lib = C.CDLL(tn.LIB_PATH)
ERR_INVALID, ERR_UNSUPPORTED = -1, -2
EPS64 = float(np.finfo(np.float64).eps)
TOL = {np.dtype(np.complex64): 1e-5, np.dtype(np.complex128): max(200 * EPS64, 10 * PATH_BASELINE),
       np.dtype(np.float32): 1e-5, np.dtype(np.float64): 200 * EPS64}
GUARD = 40


def _ints(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.int32))


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _rand(rng, n, dt):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(dt)


# ---- 1. the apply kernel ---------------------------------------------------------------------------------------------------------------------
#              (d, chi_a, chi_b, chunks_in, ksplit)   ksplit 0: as plan_path_apply chooses
APPLY_ITEMS = [(2, 1, 1, 1, 1), (2, 3, 5, 2, 1), (1, 2, 3, 1, 2), (3, 4, 2, 1, 3), (2, 16, 16, 3, 0), (2, 32, 32, 2, 5), (4, 2, 2, 1, 1)]
APPLY_SCALES = [0.75, 0.0, 1.5, 0.0, 1.25, 0.875, 0.0]      # 0: a null pointer (no factor pending)


@pytest.mark.parametrize("ptype", [0, 1])
@pytest.mark.parametrize("dtype", [0, 1])
def test_path_apply_kernel_against_extended_precision(ptype, dtype):
    pdt = np.complex64 if ptype == 0 else np.complex128
    tdt = np.complex64 if dtype == 0 else np.complex128
    rng = np.random.default_rng(23 + 2 * ptype + dtype)
    n = len(APPLY_ITEMS)
    col = lambda k: _ints([it[k] for it in APPLY_ITEMS])
    ks, nrb = _ints([0] * n), _ints([0] * n)
    assert lib.tnqs_dbg_path_apply_plan(n, _p(col(1)), _p(col(2)), _p(col(4)), _p(ks), _p(nrb)) == 0, lib.tnqs_last_error()
    assert all(k == it[4] for k, it in zip(ks, APPLY_ITEMS) if it[4]) and 1 <= ks[4] <= 16 and list(nrb) == [1, 1, 1, 1, 1, 4, 1]
    Ls = [_rand(rng, c * (d * ca) ** 2, pdt).reshape(c, -1) for (d, ca, cb, c, _k) in APPLY_ITEMS]
    Ts = [_rand(rng, (ca * cb) ** 2, tdt) for (d, ca, cb, c, _k) in APPLY_ITEMS]
    tot = GUARD + sum(int(k) * (d * cb) ** 2 + GUARD for k, (d, ca, cb, c, _k) in zip(ks, APPLY_ITEMS))
    out = np.full(tot, np.nan + 1j * np.nan, dtype=np.complex128)
    rc = lib.tnqs_dbg_path_apply(ptype, dtype, n, _p(col(0)), _p(col(1)), _p(col(2)), _p(col(3)), _p(col(4)), _p(np.concatenate([x.ravel() for x in Ls])),
                                 _p(np.concatenate(Ts)), _p(np.array(APPLY_SCALES)), _p(out), GUARD)
    assert rc == 0, lib.tnqs_last_error()
    off = GUARD
    for (d, ca, cb, c, _k), k, xl, xt, f in zip(APPLY_ITEMS, ks, Ls, Ts, APPLY_SCALES):
        nn = (d * cb) ** 2
        chunks = out[off:off + int(k) * nn].reshape(int(k), nn)
        assert np.all(np.isfinite(chunks))                                    # every element of every chunk was written
        got = np.sum(chunks.astype(np.clongdouble), axis=0).reshape(cb, d, cb, d).transpose(3, 2, 1, 0)       # [s, b, s', b']
        l4 = _env4(xl, d, ca)                                                 # [s, a, s', a'], chunks summed in extended precision
        t4 = xt.astype(np.clongdouble).reshape(ca, ca, cb, cb).transpose(3, 2, 1, 0)                          # [b, b', a, a']
        fac2 = np.longdouble((f or 1.0) ** 2)
        ref = np.einsum("saSc,bdac->sbSd", l4, t4) * fac2
        mag = (np.einsum("saSc,bdac->sbSd", np.abs(l4), np.abs(t4)) * fac2).astype(np.float64)
        bound = 8 * 2.0 ** -53 * (c + ca * ca) * mag
        err = np.abs((got - ref).astype(np.complex128))
        print(f"MEASURED path_apply P={pdt.__name__} T={tdt.__name__} {(d, ca, cb, c, int(k))}: max |dev - ref| / bound = {np.max(err / bound):.3e} (max bound {np.max(bound):.3e})")
        assert np.all(err <= bound)
        assert np.all(np.isnan(out[off - GUARD:off].real))                    # the guard band in front of the item
        off += int(k) * nn + GUARD
    assert np.all(np.isnan(out[off - GUARD:].real)) and off == tot            # and the one behind the last


def test_path_apply_kernel_refuses_more_than_16_rows():
    z = np.zeros(25, dtype=np.complex64); out = np.full(25 + 2, np.nan + 0j, dtype=np.complex128); one = _ints([1])
    rc = lib.tnqs_dbg_path_apply(0, 0, 1, _p(_ints([5])), _p(one), _p(one), _p(one), _p(one), _p(z), _p(z), _p(np.ones(1)), _p(out), 1)
    assert rc == ERR_UNSUPPORTED and np.all(np.isnan(out.real))               # before anything is allocated: nothing is written


# ---- 2. the bond contraction with one partial type per end ----------------------------------------------------------------------------------
@pytest.mark.parametrize("ptypes", [(1, 0), (0, 1)])
def test_edge_rdm_kernel_with_one_partial_type_per_end(ptypes):
    pu_t, pv_t = (np.complex64 if t == 0 else np.complex128 for t in ptypes)
    rng = np.random.default_rng(31 + ptypes[0])
    pu = [_rand(rng, cu * (du * chi) ** 2, pu_t).reshape(cu, -1) for (du, dv, chi, cu, cv) in EDGE_ITEMS]
    pv = [_rand(rng, cv * (dv * chi) ** 2, pv_t).reshape(cv, -1) for (du, dv, chi, cu, cv) in EDGE_ITEMS]
    tot = GUARD + sum((du * dv) ** 2 + GUARD for (du, dv, chi, cu, cv) in EDGE_ITEMS)
    out = np.full(tot, np.nan + 1j * np.nan, dtype=np.complex128)
    col = lambda k: _p(_ints([it[k] for it in EDGE_ITEMS]))
    su = np.array([s[0] for s in EDGE_SCALES]); svv = np.array([s[1] for s in EDGE_SCALES])
    rc = lib.tnqs_dbg_edge_rdm_mixed(ptypes[0], ptypes[1], len(EDGE_ITEMS), col(0), col(1), col(2), col(3), col(4), _p(np.concatenate([x.ravel() for x in pu])),
                                     _p(np.concatenate([x.ravel() for x in pv])), _p(su), _p(svv), _p(out), GUARD)
    assert rc == 0, lib.tnqs_last_error()
    off = GUARD
    for (du, dv, chi, cu, cv), xu, xv, (fu, fv) in zip(EDGE_ITEMS, pu, pv, EDGE_SCALES):
        dd = du * dv
        got = out[off:off + dd * dd].reshape(dd, dd, order="F")
        eu, ev = _env4(xu, du, chi), _env4(xv, dv, chi)
        fac2 = np.longdouble((fu or 1.0) ** 2 * (fv or 1.0) ** 2)
        ref = (np.einsum("saSb,taTb->stST", eu, ev) * fac2).reshape(dd, dd)
        mag = (np.einsum("saSb,taTb->stST", np.abs(eu), np.abs(ev)) * fac2).reshape(dd, dd)
        bound = 8 * 2.0 ** -53 * (cu + cv + chi * chi) * mag.astype(np.float64)
        err = np.abs(got - ref.astype(np.complex128))
        print(f"MEASURED edge_rdm ({pu_t.__name__}, {pv_t.__name__}) {(du, dv, chi, cu, cv)}: max |dev - ref| / bound = {np.max(err / bound):.3e}")
        assert np.all(np.isfinite(got)) and np.all(err <= bound)
        assert np.all(np.isnan(out[off - GUARD:off].real))
        off += dd * dd + GUARD
    assert np.all(np.isnan(out[off - GUARD:].real)) and off == tot


# ---- 3. tnqs_rdm_paths on identical inputs ---------------------------------------------------------------------------------------------------
def _call(bpc, paths, ws=None):
    """tnqs_rdm_paths (ws: tnqs_dbg_rdm_paths_ws with that bound) -> (rc, [[matrix of (p_0, p_k)]], batches)"""
    g = bpc.graph
    dims = [[bpc._site_dim(p[0]) * bpc._site_dim(w) for w in p[1:]] for p in paths]
    out = np.zeros(max(1, sum(dd * dd for ds in dims for dd in ds)), dtype=np.complex128)
    lens = _ints([len(p) for p in paths]); verts = _ints([g.index[v] for p in paths for v in p]); nb = C.c_int(0)
    if ws is None:
        rc = lib.tnqs_rdm_paths(bpc._h, len(paths), _p(lens), _p(verts), _p(out))
    else:
        rc = lib.tnqs_dbg_rdm_paths_ws(bpc._h, len(paths), _p(lens), _p(verts), _p(out), C.c_int64(int(ws)), C.byref(nb))
    mats, off = [], 0
    for ds in dims:
        mats.append([])
        for dd in ds:
            mats[-1].append(out[off:off + dd * dd].reshape(dd, dd, order="F").copy()); off += dd * dd
    return rc, mats, nb.value


@functools.lru_cache(maxsize=None)
def _grid_case(dt, chi, projected):
    """(cache, reference matrices of GRID_PATHS from the tensors and messages the cache hands out): computed once, shared, left unchanged"""
    g = tn.named_grid((3, 4))
    psi = tn.random_tensornetworkstate(dt, g, chi, seed=7 + chi)
    bpc = tn.update(tn.BeliefPropagationCache(psi), maxiter=40, tolerance=1e-6 if dt == np.complex64 else 1e-12)
    if projected:
        bpc = bpc.project((1, 2), 1).project((2, 2), 0)      # (1, 2): inner vertex of paths 0 and 4, far end of path 3; (2, 2): source of path 2, inner vertex of paths 3 and 4
    ts, ms, nb = _read_back(bpc)
    return bpc, [pr.path_rdms(ts, ms, nb, p) for p in GRID_PATHS]


def _worst_normalised(mats, refs):
    worst = 0.0
    for pm, prf in zip(mats, refs):
        assert len(pm) == len(prf)
        for m, r in zip(pm, prf):
            assert m.shape == r.shape
            worst = max(worst, float(np.max(np.abs(m / np.trace(m) - r / np.trace(r)))))
    return worst


@pytest.mark.parametrize("dt,chi", [(np.complex64, 3), (np.complex128, 3), (np.complex64, 16), (np.complex64, 32)])
@pytest.mark.parametrize("projected", [False, True])
def test_rdm_paths_against_the_reference_on_identical_inputs(dt, chi, projected):
    bpc, refs = _grid_case(dt, chi, projected)
    rc, mats, _ = _call(bpc, GRID_PATHS)
    assert rc == 0, lib.tnqs_last_error()
    worst = _worst_normalised(mats, refs)
    print(f"MEASURED rdm_paths {np.dtype(dt).name} 3x4 chi {chi}{' two vertices projected' if projected else ''}: max normalised deviation {worst:.3e} (bound {TOL[np.dtype(dt)]:.1e})")
    assert worst <= TOL[np.dtype(dt)]
    if projected:
        assert [m.shape[0] for m in mats[2]] == [2, 2] and [m.shape[0] for m in mats[3]] == [4, 4, 2, 2] and [m.shape[0] for m in mats[0]] == [2, 4, 4]
    # the public form: one dict per path, normalised, keyed by (p_0, p_k)
    pub = tn.rdm_paths(bpc, GRID_PATHS)
    assert [list(dct) for dct in pub] == [[(p[0], w) for w in p[1:]] for p in GRID_PATHS]
    assert all(abs(np.trace(m) - 1) < 1e-12 for dct in pub for m in dct.values())


# ---- 4. exact on a tree ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tree_case(dt):
    g = tn.named_comb_tree((3, 3))
    psi = tn.random_tensornetworkstate(dt, g, 3, seed=5)
    bpc = tn.update(tn.BeliefPropagationCache(psi))
    og = o.Graph(list(g.vertices), list(g.edges))
    vec = sv.tns_to_statevector(o.TensorNetworkState(og, {v: psi.tensors[v].astype(np.complex128) for v in g.vertices}))

    def exact(u, w):
        m = np.moveaxis(vec, [og.pos[u], og.pos[w]], [0, 1]).reshape(4, -1)
        r = m @ m.conj().T
        return r / np.trace(r)
    return bpc, exact


@pytest.mark.parametrize("dt", [np.float32, np.float64, np.complex64, np.complex128])
def test_rdm_of_the_ends_of_a_path_is_exact_on_the_comb_tree(dt):
    bpc, exact = _tree_case(dt)
    worst = 0.0
    for p, dct in zip(TREE_PATHS, tn.rdm_paths(bpc, TREE_PATHS)):
        assert len(dct) == len(p) - 1
        for (u, w), got in dct.items():
            worst = max(worst, float(np.max(np.abs(got - exact(u, w)))))
    print(f"MEASURED rdm_paths {np.dtype(dt).name} comb tree: max |bp - exact| = {worst:.3e} (bound {TOL[np.dtype(dt)]:.1e})")
    assert worst <= TOL[np.dtype(dt)]


# ---- 5. cross-checks with expect() and rdm_edges ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_expect_pairs_equals_the_loop_of_expect_calls(dt):
    """along one row of the grid and on the tree the path between two vertices is unique, so the one call and the loop of region contractions compute the same quantity"""
    bpc, _ = _grid_case(dt, 3, False)
    row = [(2, j) for j in range(1, 5)]
    pairs = [(row[i], row[j]) for i in range(4) for j in range(i + 1, 4)] + [(row[3], row[0]), (row[2], row[1])]
    got = tn.expect_pairs(bpc, "ZZ", pairs)
    want = np.array([tn.expect(bpc, ("ZZ", [u, w])) for (u, w) in pairs])
    worst = float(np.max(np.abs(got - want)))
    tbpc, _ = _tree_case(dt)
    tpairs = [((1, 3), (3, 3)), ((1, 3), (2, 1)), ((2, 3), (1, 1)), ((3, 3), (1, 3)), ((2, 2), (2, 3))]
    tgot = tn.expect_pairs(tbpc, (tn.gate_matrix("X"), tn.gate_matrix("Z")), tpairs)
    twant = np.array([tn.expect(tbpc, ("XZ", [u, w])) for (u, w) in tpairs])
    tworst = float(np.max(np.abs(tgot - twant)))
    print(f"MEASURED expect_pairs {np.dtype(dt).name}: max |one call - expect()| = {worst:.3e} (grid row, ZZ), {tworst:.3e} (comb tree, XZ) (bound {TOL[np.dtype(dt)]:.1e})")
    assert got.shape == (8,) and worst <= TOL[np.dtype(dt)] and tworst <= TOL[np.dtype(dt)]
    # the dict form: (w, u) after (u, w) is the index swap, an adjacent pair is allowed
    r = tn.rdm_pairs(bpc, [(row[0], row[2]), (row[2], row[0]), (row[0], row[1])])
    assert np.array_equal(r[(row[2], row[0])], r[(row[0], row[2])].reshape(2, 2, 2, 2).transpose(1, 0, 3, 2).reshape(4, 4))
    assert tn.rdm_pairs(bpc, []) == {} and tn.expect_pairs(bpc, "ZZ", []).shape == (0,) and tn.rdm_paths(bpc, []) == []


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_connected_correlation_function_and_first_step(dt):
    """connected: <O_0 O_k> - <O_0> <O_k> with the one-site values from the partial traces of the same matrix, against the three expect() calls.  On the TREE the
    marginals of the two-site matrix ARE the one-site matrices (BP is exact there), so the bound is the type's; on the loopy grid they agree only up to the BP
    residual, so there the plain correlation function is compared, and the connected one at complex128 with a bound derived from BP's convergence measure"""
    tol = TOL[np.dtype(dt)]
    tbpc, _ = _tree_case(dt)
    path = TREE_PATHS[0]
    got = tn.correlation_function(tbpc, "ZZ", path, connected=True)
    z0 = tn.expect(tbpc, ("Z", [path[0]]))
    want = np.array([tn.expect(tbpc, ("ZZ", [path[0], w])) - z0 * tn.expect(tbpc, ("Z", [w])) for w in path[1:]])
    worst = float(np.max(np.abs(got - want)))
    bpc, _ = _grid_case(dt, 3, False)
    row = GRID_PATHS[0]
    plain = tn.correlation_function(bpc, (tn.gate_matrix("X"), tn.gate_matrix("Z")), row)
    pwant = np.array([tn.expect(bpc, ("XZ", [row[0], w])) for w in row[1:]])
    pworst = float(np.max(np.abs(plain - pwant)))
    print(f"MEASURED correlation_function {np.dtype(dt).name}: connected ZZ on the tree {worst:.3e}, XZ on a grid row {pworst:.3e} (bound {tol:.1e})")
    assert got.shape == (6,) and worst <= tol and pworst <= tol
    if dt == np.complex128:
        # BP's convergence measure is 1 - fidelity^2 of successive messages (beliefpropagationcache.jl:17-21): a relative message change delta shows as delta^2, and
        # float64 cannot resolve it below eps.  So after sweeping on to a measure below 1e-12 the messages are within sqrt(max(measure, eps)) of their last update, and
        # the marginals of the two-site matrix differ from the one-site matrices by that times the amplification of the fixed-point map, bounded here by 100.
        # (measured on the device before this bound was derived: 8.9e-9 at a measure of 3.7e-14, i.e. 0.05 sqrt(measure))
        info = {}
        conv = tn.update(bpc, info=info, maxiter=500, tolerance=1e-12)
        assert info["diff"] <= 1e-12, info
        cbound = 100 * float(np.sqrt(max(info["diff"], EPS64)))
        cg = tn.correlation_function(conv, "ZZ", row, connected=True)
        z0 = tn.expect(conv, ("Z", [row[0]]))
        cw = np.array([tn.expect(conv, ("ZZ", [row[0], w])) - z0 * tn.expect(conv, ("Z", [w])) for w in row[1:]])
        print(f"MEASURED correlation_function complex128 connected ZZ on a grid row after {info['niter']} more sweeps (measure {info['diff']:.1e}): "
              f"{float(np.max(np.abs(cg - cw))):.3e} (bound {cbound:.1e})")
        assert np.max(np.abs(cg - cw)) <= cbound
    # k = 1 is the bond's matrix of rdm_edges
    rc, mats, _ = _call(bpc, GRID_PATHS)
    assert rc == 0
    req, em = core._rdm_edges_raw(bpc, [(p[0], p[1]) for p in GRID_PATHS])
    first = max(float(np.max(np.abs(pm[0] - e)) / np.max(np.abs(e))) for pm, e in zip(mats, em))
    print(f"MEASURED rdm_paths k = 1 against rdm_edges {np.dtype(dt).name}: {first:.3e} (bound {tol:.1e})")
    assert first <= tol


# ---- 6. batching -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_batches_under_a_workspace_bound(dt):
    bpc, refs = _grid_case(dt, 3, False)
    rc, one, nb1 = _call(bpc, GRID_PATHS, ws=1 << 30)
    assert rc == 0 and nb1 == 1, lib.tnqs_last_error()
    # the chain temporaries of a three-vertex path's three ends alone exceed this bound: every path needs more than the bound and runs alone
    rc, many, nb = _call(bpc, GRID_PATHS, ws=3 * 2 * 2 * 3 ** 2 * np.dtype(dt).itemsize)
    assert rc == 0 and nb == len(GRID_PATHS), lib.tnqs_last_error()
    w1, wn = _worst_normalised(one, refs), _worst_normalised(many, refs)
    print(f"MEASURED rdm_paths {np.dtype(dt).name} in 1 / {nb} batches: max normalised deviation {w1:.3e} / {wn:.3e} (bound {TOL[np.dtype(dt)]:.1e})")
    assert w1 <= TOL[np.dtype(dt)] and wn <= TOL[np.dtype(dt)]
    assert lib.tnqs_dbg_rdm_paths_ws(bpc._h, 0, None, None, None, C.c_int64(0), None) == ERR_INVALID


# ---- 7. pending scales -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_deferred_gates_and_pending_scales_are_part_of_the_answer(dt):
    """after two layers that end in one-site gates (deferred) on normalised tensors (pending scale factors on inner and end vertices), the UN-normalised matrices are
    those of the tensors the cache hands out afterwards"""
    g = tn.named_grid((3, 4))
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
    f = C.c_double(1.0); pending = {}
    for v in g.vertices:
        assert lib.tnqs_dbg_pending_scale(bpc._h, g.index[v], C.byref(f)) == 0
        pending[v] = f.value
    inner = {v for p in GRID_PATHS for v in p[1:-1]}; ends = {v for p in GRID_PATHS for v in (p[0], p[-1])}
    assert any(pending[v] != 1.0 for v in inner) and any(pending[v] != 1.0 for v in ends), pending
    rc, mats, _ = _call(bpc, GRID_PATHS)
    assert rc == 0, lib.tnqs_last_error()
    ts, ms, nb = _read_back(bpc)
    worst = 0.0
    for p, pm in zip(GRID_PATHS, mats):
        for m, r in zip(pm, pr.path_rdms(ts, ms, nb, p)):
            worst = max(worst, float(np.max(np.abs(m - r)) / np.max(np.abs(r))))
    print(f"MEASURED rdm_paths {np.dtype(dt).name} after two layers, un-normalised: max |dev - ref| / max |ref| = {worst:.3e} (bound {TOL[np.dtype(dt)]:.1e}; "
          f"pending scales {min(pending.values()):.3g} .. {max(pending.values()):.3g})")
    assert worst <= TOL[np.dtype(dt)]


# ---- 8. the contract of the entry point ------------------------------------------------------------------------------------------------------
def test_argument_errors_and_the_empty_call():
    bpc, _ = _grid_case(np.complex64, 3, False)
    ix = bpc.graph.index
    out = np.zeros(64, dtype=np.complex128)

    def rc_of(lens, verts, o=out):
        return lib.tnqs_rdm_paths(bpc._h, len(lens), _p(_ints(lens)), _p(_ints(verts)), _p(o) if o is not None else None)
    good = [ix[(1, 1)], ix[(1, 2)], ix[(1, 3)]]
    assert rc_of([3], good) == 0
    assert rc_of([3], [ix[(1, 1)], ix[(1, 2)], 99]) == ERR_INVALID                                   # a vertex out of range
    assert rc_of([2], [-1, ix[(1, 2)]]) == ERR_INVALID
    assert rc_of([3], [ix[(1, 1)], ix[(1, 2)], ix[(2, 3)]]) == ERR_INVALID                           # consecutive vertices that are not adjacent
    assert rc_of([3], [ix[(1, 1)], ix[(1, 2)], ix[(1, 1)]]) == ERR_INVALID                           # a repeated vertex
    assert rc_of([4], [ix[(1, 1)], ix[(1, 2)], ix[(2, 2)], ix[(2, 1)]]) == ERR_INVALID               # a chord
    assert rc_of([3, 1], good + [ix[(2, 2)]]) == ERR_INVALID                                         # a length below 2
    assert rc_of([3], good, None) == ERR_INVALID                                                     # a null output with npaths > 0
    assert lib.tnqs_rdm_paths(bpc._h, -1, None, None, _p(out)) == ERR_INVALID
    before = out.copy()
    assert lib.tnqs_rdm_paths(bpc._h, 0, None, None, None) == 0 and np.array_equal(out, before)      # npaths = 0 is a no-op
    with pytest.raises(tn.TnqsArgumentError, match="chord"):
        tn.rdm_paths(bpc, [[(1, 1), (1, 2), (2, 2), (2, 1)]])
    with pytest.raises(tn.TnqsArgumentError, match="only single vertices and bonds"):
        tn.rdm(bpc, [(1, 1), (1, 3)])


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_the_handle_is_left_as_it_was(dt):
    bpc = _grid_case(dt, 3, False)[0].copy()
    g = bpc.graph
    before_t = {v: bpc.tensor(v) for v in g.vertices}
    before_m = {e: bpc.message(e) for (a, b) in g.edges for e in ((a, b), (b, a))}
    tn.rdm_paths(bpc, GRID_PATHS); tn.expect_pairs(bpc, "XX", [((1, 1), (3, 4))]); tn.correlation_function(bpc, "ZZ", GRID_PATHS[4], connected=True)
    assert all(np.array_equal(bpc.tensor(v), before_t[v]) for v in g.vertices)
    assert all(np.array_equal(bpc.message(e), m) for e, m in before_m.items())
