"""GPU tests of the bond entanglement spectra and Renyi entropies (bond_spectra / bond_entropies / renyi_entropy; tnqs_bond_spectra): the four stages of
csrc/engine_spectra.cpp through their debug entry point against tests/bond_spectra_ref.py (complex128 numpy on the SAME stored values), tnqs_bond_spectra against the
same reference on the messages read back from the handle, known answers (GHZ, a padded product state, exact Schmidt spectra on a tree), the identity with the symmetric
gauge, the entropy functions on top and the contract of the C entry point.

Bounds (none of them measured on the kernels):
  an entry of a normalised spectrum, device against the reference on identical inputs, both element types (the device computes in f64 from the stored values):
      max(200 eps64 chi, 10 x SPECTRUM_BASELINE), SPECTRUM_BASELINE = the distance of the reference's own two routes on the kernel inputs
      (tests/test_bond_spectra_ref_cpu.py: 1e-15, so the bound is 200 eps64 chi = 4.4e-14 chi)
  sum of a spectrum: 1 to 4 chi eps64
  exact Schmidt spectrum on the comb tree: 200 eps64 chi for complex128, the project's 1e-5 for complex64 (the state itself is stored in f32)
  gauge identity: 1e-5 for complex64, 1e-10 for complex128 (the gauge's own SVD in the state's type is the limiting step)
  GHZ: ln 2 to 1e-9 (the reference's own test, test/test_constructors.jl:69-74)"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import tnqs_amd as tn
import tnqs_oracle as o
import statevector as sv
import bond_spectra_ref as br
from tnqs_amd import core
from tnqs_amd import _lib as L
from test_bond_spectra_ref_cpu import SPECTRUM_BASELINE, schmidt_spectrum

pytestmark = pytest.mark.gpu
lib = C.CDLL(tn.LIB_PATH)
ERR_INVALID, ERR_UNSUPPORTED, ERR_NUMERIC = -1, -2, -4
EPS64 = br.EPS64
GUARD = 24
DTYPES = [np.complex64, np.complex128]


def bound(chi):
    return max(200 * EPS64 * chi, 10 * SPECTRUM_BASELINE)


def _ints(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.int32))


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


# ---- 1. the kernels ------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _kernel_case(dt):
    """the kernel inputs of one element type and their reference spectra, computed once"""
    items = br.kernel_inputs(dt)
    refs = [br.bond_spectrum(br.effective(m1, p1), br.effective(m2, p2), br.cutoff_of(dt)) for (n, kind, m1, m2, p1, p2) in items]
    for r in refs:
        r.setflags(write=False)
    return items, refs


def _run_dbg(dt, items):
    """one tnqs_dbg_bond_spectrum launch over items [(chi, m1, m2, present1, present2)]: (spectra, flags); the guard words are checked here"""
    chis = [it[0] for it in items]
    tot = GUARD + sum(n + GUARD for n in chis)
    out = np.full(tot, np.nan, dtype=np.float64)
    flags = np.full(len(items), -1, dtype=np.int32)
    m1 = np.concatenate([it[1].ravel(order="F") for it in items]); m2 = np.concatenate([it[2].ravel(order="F") for it in items])
    present = _ints([[int(it[3]), int(it[4])] for it in items]).ravel()
    rc = lib.tnqs_dbg_bond_spectrum(0 if dt == np.complex64 else 1, len(items), _p(_ints(chis)), _p(m1), _p(m2), _p(present), _p(out), _p(flags), GUARD)
    assert rc == 0, lib.tnqs_last_error()
    spectra, off = [], GUARD
    for n in chis:
        assert np.all(np.isnan(out[off - GUARD:off]))                          # the guard band in front of the item
        spectra.append(out[off:off + n].copy())
        off += n + GUARD
    assert np.all(np.isnan(out[off - GUARD:])) and off == tot                  # and the one behind the last
    return spectra, flags


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("launch", ["all sizes: the chi = 72 items take the global-memory Jacobi, the others the LDS-resident one", "chi <= 64: the LDS-resident Jacobi alone"])
def test_bond_spectrum_kernels_against_the_reference(dt, launch):
    items, refs = _kernel_case(dt)
    keep = [i for i, it in enumerate(items) if launch.startswith("all") or it[0] <= 64]
    assert {items[i][0] for i in keep} == ({1, 2, 3, 5, 16, 17, 32, 64, 72} if launch.startswith("all") else {1, 2, 3, 5, 16, 17, 32, 64})
    spectra, flags = _run_dbg(dt, [(items[i][0],) + items[i][2:] for i in keep])
    assert not flags.any()
    worst = {}
    for i, lam in zip(keep, spectra):
        n, kind = items[i][0], items[i][1]
        assert np.all(np.isfinite(lam)) and np.all(np.diff(lam) <= 0)          # descending
        assert abs(lam.sum() - 1) <= 4 * n * EPS64
        err = float(np.max(np.abs(lam - refs[i])))
        worst[kind] = max(worst.get(kind, 0.0), err / (200 * EPS64 * n))
        assert err <= bound(n), (n, kind, err, bound(n))
    print(f"MEASURED bond spectrum kernels {np.dtype(dt).name}, {launch.split(':')[0]}: max |dev - ref| / (200 eps chi) per kind = "
          + ", ".join(f"{k} {v:.3e}" for k, v in sorted(worst.items())) + f" (bound {bound(72):.1e})")


@pytest.mark.parametrize("dt", DTYPES)
def test_a_negative_message_eigenvalue_flags_its_item_only(dt):
    items, refs = _kernel_case(dt)
    good = [i for i, it in enumerate(items) if it[1] == "full" and it[0] in (3, 5, 17)]
    m1, m2 = br.negative_item(dt)
    launch = [(items[good[0]][0],) + items[good[0]][2:], (5, m1, m2, True, True)] + [(items[i][0],) + items[i][2:] for i in good[1:]]
    spectra, flags = _run_dbg(dt, launch)
    assert flags.tolist() == [0, 1, 0, 0]
    for lam, i in zip([spectra[0]] + spectra[2:], good):
        assert np.max(np.abs(lam - refs[i])) <= bound(items[i][0])


def test_a_bond_beyond_256_is_refused():
    z = np.zeros(1, dtype=np.complex64); out = np.full(300, np.nan); flags = np.zeros(1, dtype=np.int32)
    rc = lib.tnqs_dbg_bond_spectrum(0, 1, _p(_ints([257])), _p(z), _p(z), _p(_ints([0, 0])), _p(out), _p(flags), 0)
    assert rc == ERR_UNSUPPORTED and np.all(np.isnan(out))


# ---- 2. tnqs_bond_spectra on identical inputs ----------------------------------------------------------------------------------------------------------------
GRAPHS = {"grid3x3": (lambda: tn.named_grid((3, 3)), 3), "heavyhex11": (lambda: tn.heavy_hexagonal_lattice(1, 1), 4), "cubic2x2x3": (lambda: tn.named_grid((2, 2, 3)), 2)}


@functools.lru_cache(maxsize=None)
def _cache(name, dt):
    make, chi = GRAPHS[name]
    g = make()
    psi = tn.random_tensornetworkstate(dt, g, chi, seed=7 + chi)
    return tn.update(tn.BeliefPropagationCache(psi), maxiter=40, tolerance=1e-6 if dt == np.complex64 else 1e-12)


def _ref_spectrum(bpc, e):
    return br.bond_spectrum(bpc.message(e), bpc.message((e[1], e[0])), br.cutoff_of(bpc.dtype))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", list(GRAPHS))
def test_bond_spectra_against_the_reference_on_identical_inputs(name, dt):
    bpc = _cache(name, dt).copy()
    g = bpc.graph; chi = GRAPHS[name][1]
    before_t = {v: bpc.tensor(v) for v in g.vertices}
    before_m = {e: bpc.message(e) for (a, b) in g.edges for e in ((a, b), (b, a))}
    spec = tn.bond_spectra(bpc)
    assert list(spec) == list(g.edges)
    flipped = tn.bond_spectra(bpc, [(b, a) for (a, b) in g.edges])
    worst = worst_flip = 0.0
    for e in g.edges:
        lam = spec[e]
        assert lam.dtype == np.float64 and lam.shape == (chi,) and np.all(np.diff(lam) <= 0) and abs(lam.sum() - 1) <= 4 * chi * EPS64
        worst = max(worst, float(np.max(np.abs(lam - _ref_spectrum(bpc, e)))))
        worst = max(worst, float(np.max(np.abs(flipped[(e[1], e[0])] - _ref_spectrum(bpc, (e[1], e[0]))))))
        worst_flip = max(worst_flip, float(np.max(np.abs(lam - flipped[(e[1], e[0])]))))
    print(f"MEASURED bond_spectra {np.dtype(dt).name} {name} chi {chi}: max |dev - ref| = {worst:.3e}, max |(u, v) - (v, u)| = {worst_flip:.3e} (bound {bound(chi):.1e})")
    assert worst <= bound(chi) and worst_flip <= bound(chi)
    # the handle is left as it was, bit for bit
    assert all(np.array_equal(bpc.tensor(v), before_t[v]) for v in g.vertices)
    assert all(np.array_equal(bpc.message(e), m) for e, m in before_m.items())


# ---- 3. known answers ----------------------------------------------------------------------------------------------------------------------------------------
def test_ghz_bonds_carry_ln2():
    g = tn.named_grid((3, 3))
    tensors = {}
    for v in g.vertices:
        t = np.zeros((2,) + (2,) * g.degree(v), dtype=np.complex128)
        t[(0,) * t.ndim] = 1
        t[(1,) * t.ndim] = 1
        tensors[v] = t
    bpc = tn.update(tn.BeliefPropagationCache(tn.TensorNetworkState(g, tensors)), maxiter=300, tolerance=1e-14)
    for alpha in (1, 2):
        s = tn.bond_entropies(bpc, alpha)
        assert s.shape == (12,) and np.max(np.abs(s - math.log(2))) < 1e-9
    e = g.edges[0]
    assert abs(tn.von_neumann_entanglement_entropy(bpc, tuple(e)) - math.log(2)) < 1e-9
    assert abs(tn.second_renyi_entanglement_entropy(bpc, tuple(e)) - math.log(2)) < 1e-9


@pytest.mark.parametrize("dt", DTYPES)
def test_a_padded_product_state_has_spectrum_one_zero_zero(dt):
    g = tn.named_grid((3, 3))
    tensors = {}
    for v in g.vertices:
        t = np.zeros((2,) + (3,) * g.degree(v), dtype=dt)
        t[(slice(None),) + (0,) * g.degree(v)] = np.array([0.6, 0.8j], dtype=dt)
        tensors[v] = t
    bpc = tn.update(tn.BeliefPropagationCache(tn.TensorNetworkState(g, tensors)), maxiter=10, tolerance=1e-6)
    for lam in tn.bond_spectra(bpc).values():
        assert np.max(np.abs(lam - np.array([1.0, 0.0, 0.0]))) <= 200 * EPS64 * 3
    for alpha in (0.5, 1, 2):
        assert np.max(np.abs(tn.bond_entropies(bpc, alpha))) <= 1e-12


@pytest.mark.parametrize("dt", DTYPES)
def test_exact_schmidt_spectrum_on_the_comb_tree(dt):
    g = tn.named_comb_tree((3, 3))
    psi = tn.random_tensornetworkstate(dt, g, 3, seed=5)
    bpc = tn.update(tn.BeliefPropagationCache(psi))
    og = o.Graph(list(g.vertices), list(g.edges))
    vec = sv.tns_to_statevector(o.TensorNetworkState(og, {v: psi.tensors[v].astype(np.complex128) for v in g.vertices}))
    spec = tn.bond_spectra(bpc)
    worst = max(float(np.max(np.abs(spec[(a, b)] - schmidt_spectrum(vec, og, a, b, 3)))) for (a, b) in g.edges)
    tol = 200 * EPS64 * 3 if dt == np.complex128 else 1e-5
    print(f"MEASURED bond_spectra {np.dtype(dt).name} comb tree chi 3: max |bp - Schmidt| = {worst:.3e} (bound {tol:.1e})")
    assert worst <= tol


# ---- 4. the gauge identity -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_spectrum_is_the_squared_gauge_singular_values(dt):
    bpc = _cache("grid3x3", dt)
    spec = tn.bond_spectra(bpc)
    gauged = tn.symmetric_gauge(bpc)
    worst = 0.0
    for e in bpc.graph.edges:
        s = np.sort(np.real(np.diag(gauged.message(e))).astype(np.float64))[::-1]
        worst = max(worst, float(np.max(np.abs(spec[e] - s * s / np.sum(s * s)))))
    tol = 1e-5 if dt == np.complex64 else 1e-10
    print(f"MEASURED bond_spectra {np.dtype(dt).name} 3x3 chi 3: max |spectrum - S^2 / sum S^2 of the gauge| = {worst:.3e} (bound {tol:.1e})")
    assert worst <= tol


# ---- 5. the entropy functions --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_entropy_functions(dt):
    bpc = _cache("grid3x3", dt)
    g = bpc.graph
    thr = br.cutoff_of(dt)
    spec = tn.bond_spectra(bpc)
    for alpha in (0.5, 1, 2):
        s = tn.bond_entropies(bpc, alpha)
        want = np.array([br.renyi(spec[e], alpha, thr) for e in g.edges])
        assert s.shape == (12,) and np.max(np.abs(s - want)) <= 1e-12
        e = g.edges[5]
        assert abs(tn.renyi_entropy(bpc, tuple(e), alpha) - s[5]) <= 1e-12
        assert abs(tn.renyi_entropy(bpc, tuple(e), alpha=alpha, alg="bp") - s[5]) <= 1e-12
    some = [g.edges[3], g.edges[0], g.edges[3]]
    assert np.array_equal(tn.bond_entropies(bpc, 2, some), tn.bond_entropies(bpc, 2)[[3, 0, 3]])
    u, v, w = (1, 1), (1, 2), (3, 3)
    assert abs(tn.renyi_entropy(bpc, [u], 1) - br.renyi(np.linalg.eigvalsh(tn.rdm(bpc, u), UPLO="U"), 1, thr)) <= 1e-12
    assert abs(tn.renyi_entropy(bpc, [u, v], 2) - br.renyi(np.linalg.eigvalsh(tn.rdm_edges(bpc, [(u, v)])[(u, v)], UPLO="U"), 2, thr)) <= 1e-12
    assert abs(tn.renyi_entropy(bpc, [u, w], 1) - br.renyi(np.linalg.eigvalsh(tn.rdm_pairs(bpc, [(u, w)])[(u, w)], UPLO="U"), 1, thr)) <= 1e-12
    assert tn.von_neumann_entanglement_entropy(bpc, (u, v)) == tn.renyi_entropy(bpc, (u, v), 1)
    assert tn.second_renyi_entanglement_entropy(bpc, [u]) == tn.renyi_entropy(bpc, [u], 2)


@pytest.mark.parametrize("dt", DTYPES)
def test_entropy_of_a_tensor_network_state_builds_and_updates_a_cache(dt):
    g = tn.named_grid((3, 3))
    psi = tn.random_tensornetworkstate(dt, g, 3, seed=10)
    kw = dict(maxiter=40, tolerance=1e-6 if dt == np.complex64 else 1e-12)
    bpc = tn.update(tn.BeliefPropagationCache(psi), **kw)
    e = ((2, 2), (2, 3))
    tol = 1e-5 if dt == np.complex64 else 1e-10                                # two handles, two updates
    assert abs(tn.renyi_entropy(psi, e, 1, cache_update_kwargs=kw) - tn.renyi_entropy(bpc, e, 1)) <= tol
    assert abs(tn.von_neumann_entanglement_entropy(psi, e, cache_update_kwargs=kw) - tn.renyi_entropy(bpc, e, 1)) <= tol
    default = tn.update(tn.BeliefPropagationCache(psi), **tn.BeliefPropagationCache(psi).default_bp_update_kwargs())
    assert abs(tn.renyi_entropy(psi, e, 2) - tn.renyi_entropy(default, e, 2)) <= tol


# ---- 6. the contract of the entry point ---------------------------------------------------------------------------------------------------------
def test_orientation_repeats_empty_calls_and_errors():
    bpc = _cache("grid3x3", np.complex64)
    g = bpc.graph
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    # the C entry with null lists = the explicit list of all edges as (src, dst)
    a = np.zeros(36); b = np.zeros(36)
    eu, up = L.i32([g.index[x] for (x, y) in g.edges]); ev, vp = L.i32([g.index[y] for (x, y) in g.edges])
    assert L.lib.tnqs_bond_spectra(bpc._h, -7, None, None, dp(a)) == 0 and L.lib.tnqs_bond_spectra(bpc._h, 12, up, vp, dp(b)) == 0
    assert np.array_equal(a, b) and abs(a.sum() - 12) < 1e-12
    # a repeat is answered again; the other orientation is its own computation
    u, v = g.edges[4]
    req, spec = core._bond_spectra_raw(bpc, [(u, v), (v, u), (u, v)])
    assert req == [(u, v), (v, u), (u, v)] and np.array_equal(spec[0], spec[2]) and np.array_equal(spec[0], a[12:15])
    assert np.max(np.abs(spec[0] - spec[1])) <= bound(3)
    assert np.array_equal(tn.bond_entropies(bpc, 1, [(u, v), (u, v)]), np.repeat(tn.bond_entropies(bpc, 1, [(u, v)]), 2))
    # an empty call
    z, zp = L.i32([0]); out = np.zeros(4)
    assert L.lib.tnqs_bond_spectra(bpc._h, 0, zp, zp, dp(out)) == 0 and not out.any()
    assert L.lib.tnqs_bond_spectra(bpc._h, 0, zp, zp, None) == 0
    assert tn.bond_spectra(bpc, []) == {} and tn.bond_entropies(bpc, 1, []).shape == (0,)
    # not an edge, a bad vertex, a null output with work to do, a negative count
    i11, p11 = L.i32([g.index[(1, 1)]]); i33, p33 = L.i32([g.index[(3, 3)]]); i99, p99 = L.i32([99])
    assert L.lib.tnqs_bond_spectra(bpc._h, 1, p11, p33, dp(out)) == ERR_INVALID
    assert L.lib.tnqs_bond_spectra(bpc._h, 1, p11, p99, dp(out)) == ERR_INVALID
    assert L.lib.tnqs_bond_spectra(bpc._h, 1, p11, p11, dp(out)) == ERR_INVALID
    assert L.lib.tnqs_bond_spectra(bpc._h, -1, p11, p33, dp(out)) == ERR_INVALID
    assert L.lib.tnqs_bond_spectra(bpc._h, 0, None, None, None) == ERR_INVALID
    assert not out.any()
    with pytest.raises(tn.TnqsArgumentError, match="not an edge"):
        tn.bond_spectra(bpc, [((1, 1), (3, 3))])
    with pytest.raises(tn.TnqsArgumentError, match="not an edge"):
        tn.renyi_entropy(bpc, ((1, 1), (9, 9)), 1)
    with pytest.raises(tn.TnqsArgumentError, match="single vertices and pairs"):
        tn.renyi_entropy(bpc, [(1, 1), (1, 2), (1, 3)], 1)
    with pytest.raises(tn.TnqsError, match="algorithm choice not supported"):
        tn.renyi_entropy(bpc, (u, v), 1, alg="exact")
    # the handle is still usable
    assert np.array_equal(tn.bond_spectra(bpc, [(u, v)])[(u, v)], spec[0])


def test_a_negative_message_eigenvalue_is_a_domain_error():
    bpc = _cache("grid3x3", np.complex128).copy()
    u, v = bpc.graph.edges[0]
    bpc.setmessage((v, u), np.diag([1.0, 0.5, -1e-3]).astype(np.complex128))
    with pytest.raises(tn.TnqsDomainError, match="negative beyond the cutoff"):
        tn.bond_spectra(bpc, [(u, v)])
    # the other orientation takes the root of the other message, and every other bond is untouched
    assert tn.bond_spectra(bpc, [(v, u)])[(v, u)].shape == (3,)
    bpc.setmessage((v, u), np.zeros((3, 3), dtype=np.complex128))
    with pytest.raises(tn.TnqsDomainError, match="trace"):
        tn.bond_spectra(bpc, [(u, v)])


def test_sharded_handles_are_refused():
    """a two-rank handle on one GPU (the set-up of tests/test_gpu_sampling.py test_sharded_handles_are_refused; the exchange buffer comes from the HIP runtime the
    library itself is linked against, and the callback is never reached)"""
    g = tn.named_grid((2, 2))
    bpc = tn.BeliefPropagationCache(tn.random_tensornetworkstate(np.complex64, g, bond_dimension=2, seed=61))
    buf = C.c_void_p()
    lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]; lib.hipFree.argtypes = [C.c_void_p]
    assert lib.hipMalloc(C.byref(buf), 1 << 16) == 0 and buf.value
    try:
        cb = L.ALLGATHER_FN(lambda ctx, base, nbytes, nranks: -1)
        owner, op = L.i32([0, 0, 1, 1])
        L.check(L.lib.tnqs_set_sharding(bpc._h, 0, 2, op, cb, None, buf, 1 << 16))
        out = np.zeros(8)
        assert L.lib.tnqs_bond_spectra(bpc._h, 0, None, None, out.ctypes.data_as(C.POINTER(C.c_double))) == ERR_UNSUPPORTED and not out.any()
        del bpc
    finally:
        lib.hipFree(buf)
