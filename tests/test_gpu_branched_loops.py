"""GPU tests of the loop corrections' two-loop configurations on the device (tnqs_config_weights, configuration_weights, branched = "device"):
loop_branch_gram_kernel through its debug entry point against numpy complex128 and against loop_cgemm_kernel to the bit, the configuration weights against tests/branched_loop_ref.py (and the general
contraction tests/loop_ref.py) on IDENTICAL inputs -- tensors and messages read back from the handle --, and norm_sqr end to end against exact contraction.

Bounds (derived, none measured on the kernels; u = 2^-24 for complex64, 2^-53 for complex128):
  loop_branch_gram  per entry |dev - ref| <= 8 u K sum_kk |A||B|
  weights           |dev - ref| <= 8 u S k_max prod ||F_i||_F over the S factor matrices of the restatement (branched_loop_ref.bound); a simple cycle: the ring
                    bound of tests/test_gpu_loops.py
  end to end        complex64: the project's 1e-5; complex128: max(10 x the CPU baseline, summed weight bounds / |1 + sum W|)
"""
import ctypes as C
import functools

import numpy as np
import pytest

import tnqs_amd as tn
import tnqs_oracle as o
import statevector as sv
import loop_ref as lr
import branched_loop_ref as br
from test_loop_ref_cpu import FULL_ORDER_BASELINE, BRIDGED, fixtures
from test_branched_loop_ref_cpu import cases, tensors_of, BONDS

pytestmark = pytest.mark.gpu
lib = C.CDLL(tn.LIB_PATH)
lib.tnqs_last_error.restype = C.c_char_p
L = tn.core.L
ERR_INVALID, ERR_UNSUPPORTED = -1, -2                    # include/tnqs.h
U = {np.complex64: 2.0 ** -24, np.complex128: 2.0 ** -53}
DT = {np.complex64: 0, np.complex128: 1}
KCHUNK = {np.complex64: 16, np.complex128: 8}            # LoopKT of csrc/kernels_loop.hip: the k-chunk of loop_tile_body
BP_KW = dict(maxiter=300, tolerance=None)
GUARD = 96
DTS = [np.complex64, np.complex128]


def _ints(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.int32))


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _rand(rng, shape, dt):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dt)


# ---- kernel level ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_loop_branch_gram_against_float64(dt):
    """rows below a 64-tile (6, 18), one past a tile edge (80 = 64 + 16; 64 itself) and k = 1, 2, chunk - 1, chunk + 1, 2 chunk + 3 in ONE launch; every order of
    the three pairs occurs"""
    kc = KCHUNK[dt]
    legs = [(2, 3, 1), (3, 3, 2), (4, 4, 5), (8, 8, 1)]
    ks = [1, 2, kc - 1, kc + 1, 2 * kc + 3]
    orders = [(0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2)]
    items = [(x, k, orders[(i + 2 * j) % 6]) for i, x in enumerate(legs) for j, k in enumerate(ks)]
    rng = np.random.default_rng(23)
    As = [_rand(rng, (k, x[2], x[1], x[0]), dt) for (x, k, _) in items]      # column-major (x0 x1 x2) x k, leg 0 fastest
    Bs = [_rand(rng, (k, x[2], x[1], x[0]), dt) for (x, k, _) in items]
    A = np.concatenate([a.reshape(-1) for a in As]); B = np.concatenate([b.reshape(-1) for b in Bs])
    tot = GUARD + sum(int(np.prod(x)) ** 2 + GUARD for (x, _, _) in items)
    Cbuf = np.full(tot, np.nan + 1j * np.nan, dtype=dt)
    rc = lib.tnqs_dbg_loop_branch_gram(DT[dt], len(items), _p(_ints([x for (x, _, _) in items])), _p(_ints([od for (_, _, od) in items])),
                                       _p(_ints([k for (_, k, _) in items])), _p(A), _p(B), _p(Cbuf), GUARD)
    assert rc == 0, lib.tnqs_last_error()
    off, worst = GUARD, 0.0
    for (x, k, od), a, b in zip(items, As, Bs):
        n = int(np.prod(x)) ** 2
        a64, b64 = a.astype(np.complex128), b.astype(np.complex128)
        # G[l2, l1, l0, l2', l1', l0'] -> memory order (pair od[0] fastest, ket before bra): C-order axes (bra od[2], ket od[2], .., bra od[0], ket od[0])
        G = np.einsum("kcba,kfed->cbafed", a64, b64.conj())
        Gabs = np.einsum("kcba,kfed->cbafed", np.abs(a64), np.abs(b64))
        ket = {0: 2, 1: 1, 2: 0}; bra = {0: 5, 1: 4, 2: 3}
        axes = [ax for p in (od[2], od[1], od[0]) for ax in (bra[p], ket[p])]
        ref, lim = np.transpose(G, axes).reshape(-1), 8 * U[dt] * k * np.transpose(Gabs, axes).reshape(-1)
        got = Cbuf[off:off + n]
        ratio = float(np.max(np.abs(got - ref) / lim))
        worst = max(worst, ratio)
        print(f"MEASURED loop_branch_gram {dt.__name__} legs {x} k {k} order {od}: max |dev - ref| / bound = {ratio:.3e}")
        assert np.all(np.isfinite(got)) and np.all(np.abs(got - ref) <= lim)
        assert np.all(np.isnan(Cbuf[off - GUARD:off].real))
        off += n + GUARD
    assert np.all(np.isnan(Cbuf[off - GUARD:].real)) and off == tot
    print(f"MEASURED loop_branch_gram {dt.__name__}: largest error / bound {worst:.3e}")


@pytest.mark.parametrize("dt", DTS)
def test_loop_cgemm_and_loop_branch_gram_agree_to_the_bit(dt):
    """the two kernels share one tile code (loop_tile_body) and differ in the output map only: the same A, B through tnqs_dbg_loop_cgemm (opB = 1, m = n = x0 x1 x2)
    and through tnqs_dbg_loop_branch_gram give the same BYTES once the GEMM's output is permuted as the Gram's map stores it.  Rows below a tile (6) and one past a
    tile edge (80), k = 1, chunk + 1, 2 chunk + 3, the identity order and a cyclic one, one launch of each kernel"""
    kc = KCHUNK[dt]
    items = [(x, k, od) for x in [(2, 3, 1), (4, 4, 5)] for k in [1, kc + 1, 2 * kc + 3] for od in [(0, 1, 2), (2, 0, 1)]]
    rng = np.random.default_rng(29)
    As = [_rand(rng, (k, x[2], x[1], x[0]), dt) for (x, k, _) in items]      # column-major (x0 x1 x2) x k, leg 0 fastest
    Bs = [_rand(rng, (k, x[2], x[1], x[0]), dt) for (x, k, _) in items]
    A = np.concatenate([a.reshape(-1) for a in As]); B = np.concatenate([b.reshape(-1) for b in Bs])
    rows = [int(np.prod(x)) for (x, _, _) in items]
    tot = GUARD + sum(r * r + GUARD for r in rows)
    Cgemm, Cgram = (np.full(tot, np.nan + 1j * np.nan, dtype=dt) for _ in range(2))
    rc = lib.tnqs_dbg_loop_cgemm(DT[dt], 1, len(items), _p(_ints(rows)), _p(_ints(rows)), _p(_ints([k for (_, k, _) in items])), _p(A), _p(B), _p(Cgemm), GUARD)
    assert rc == 0, lib.tnqs_last_error()
    rc = lib.tnqs_dbg_loop_branch_gram(DT[dt], len(items), _p(_ints([x for (x, _, _) in items])), _p(_ints([od for (_, _, od) in items])),
                                       _p(_ints([k for (_, k, _) in items])), _p(A), _p(B), _p(Cgram), GUARD)
    assert rc == 0, lib.tnqs_last_error()
    off = GUARD
    for (x, k, od), r in zip(items, rows):
        # the GEMM's C[i + m j]: C-order axes (l2', l1', l0', l2, l1, l0); as G of the test above (l2, l1, l0, l2', l1', l0'), then the same axes as there
        G = np.transpose(Cgemm[off:off + r * r].reshape(x[2], x[1], x[0], x[2], x[1], x[0]), (3, 4, 5, 0, 1, 2))
        ket = {0: 2, 1: 1, 2: 0}; bra = {0: 5, 1: 4, 2: 3}
        axes = [ax for p in (od[2], od[1], od[0]) for ax in (bra[p], ket[p])]
        want, got = np.ascontiguousarray(np.transpose(G, axes)).reshape(-1), Cgram[off:off + r * r]
        assert np.all(np.isfinite(got)) and np.all(np.isfinite(want))
        assert got.tobytes() == want.tobytes(), (x, k, od, int(np.sum(got.view(np.uint8) != want.view(np.uint8))))
        for Cbuf in (Cgemm, Cgram):
            assert np.all(np.isnan(Cbuf[off - GUARD:off].real))
        off += r * r + GUARD
    assert off == tot and np.all(np.isnan(Cgemm[off - GUARD:].real)) and np.all(np.isnan(Cgram[off - GUARD:].real))


# ---- weights on identical inputs ----------------------------------------------------------------------------------------------------------------
def _read_back(bpc):
    g = bpc.graph
    ts = {v: bpc.tensor(v).astype(np.complex128) for v in g.vertices}
    ms = {e: bpc.message(e).astype(np.complex128) for (a, b) in g.edges for e in ((a, b), (b, a))}
    return ts, ms, lr.RefGraph(g.vertices, g.edges)


def _reference(ts, ms, rg, cfg, dt, general=True, slack=False):
    """(weight, bound) of one configuration from the factored restatement; general: also checked against the general contraction"""
    dec = br.decompose(rg, cfg)
    if dec["shape"] == "cycle":
        mats = lr.cycle_matrices(ts, ms, rg, dec["ring"])
        return lr.cycle_weight(mats), 8 * U[dt] * len(mats) * max(max(m.shape) for m in mats) * np.prod([np.linalg.norm(m) for m in mats])
    fac = br.factors(ts, ms, rg, dec)
    ref = br.weight(fac, dec)
    if general:
        full = lr.weight(ts, ms, rg, cfg)
        assert abs(ref - full) <= 1e-11 * abs(full), (cfg, ref, full)
    return ref, br.bound(fac, U[dt], slack)[0]


def _check_configs(bpc, configs, dt, tag, general=True, slack=False):
    """configuration_weights on `bpc` as it stands against the restatement from what the cache holds; returns (weights, references, bounds)"""
    got = tn.configuration_weights(bpc, configs)         # first: reading a tensor back materialises what is pending on it
    ts, ms, rg = _read_back(bpc)
    refs, bounds, worst = [], [], 0.0
    for cfg, w in zip(configs, got):
        ref, bound = _reference(ts, ms, rg, cfg, dt, general, slack)
        worst = max(worst, abs(w - ref) / bound if bound > 0 else (0.0 if w == ref else np.inf))
        refs.append(ref); bounds.append(bound)
    print(f"MEASURED config_weights {tag}: {len(configs)} configurations, largest |dev - ref| / bound = {worst:.3e}; first: dev {got[0]:.6e} ref {refs[0]:.6e} bound {bounds[0]:.3e}")
    for cfg, w, ref, bound in zip(configs, got, refs, bounds):
        assert abs(w - ref) <= bound, (tag, cfg, w, ref, bound)
    return got, refs, bounds


def _rescaled(psi):
    return tn.rescale(tn.update(tn.BeliefPropagationCache(psi), **BP_KW))


def _state(name, chi, dt, seed):
    g, cfg, shape, lens, bonds = cases()[name]
    ts, _ = tensors_of(g, chi, bonds, seed, dtype=dt)
    return tn.TensorNetworkState(g, ts), cfg


SHAPES = [("theta_2x3", 2), ("theta_2x3", 3), ("theta_135", 2), ("theta_244", 2), ("hexagons", 2), ("eight", 2), ("eight", 3), ("eight_pendant", 2),
          ("dumbbell_2x4", 2), ("dumbbell_bridged", 2), ("dumbbell_bridged", 3), ("dumbbell_2x5", 2)]


@pytest.mark.parametrize("name,chi", SHAPES)
@pytest.mark.parametrize("dt", DTS)
def test_configuration_weight_of_every_shape(dt, name, chi):
    psi, cfg = _state(name, chi, dt, seed=31 + chi)
    _check_configs(_rescaled(psi), [cfg], dt, f"{name} chi{chi} {dt.__name__}")


@pytest.mark.parametrize("name", BONDS)
@pytest.mark.parametrize("dt", DTS)
def test_unequal_bonds_with_a_weight_that_does_not_vanish(dt, name):
    """bonds 2, 3, 4 (5 at the figure-eight's centre) that differ along every chain and between the chains, bonds of dimension 1 only on legs that LEAVE the
    configuration: rectangular chain products and L^T, a branch tensor whose legs change size from round to round, B_w in the final leg order, four different
    slot dimensions.  Against the factored restatement within the plain bound, the restatement against the general contraction loop_ref.weight"""
    psi, cfg = _state(name, 2, dt, seed=51)
    got, refs, _ = _check_configs(_rescaled(psi), [cfg], dt, f"{name} {dt.__name__}")
    assert abs(refs[0]) > 1e-6                                   # (complex128 is the sharp one: its bound is some 1e-9 of |W|)


@pytest.mark.parametrize("dt", DTS)
def test_theta_with_unequal_bonds(dt):
    """bonds 1 (the shared edge), 1 (an edge inside a chain), 3, 3 and 2 on the 2 x 3 grid.  The antiprojector of a bond of dimension 1 is 1 - m m, which a rescaled
    cache makes 0 up to rounding, so this weight is 0 up to rounding on both sides and the bound is tiny: the product of the factors' norms, two of which are of
    the order of 2^-53 (branched_loop_ref.bound with slack = True, this test only: the restatement's own rounding in a factor that cancels to 0).  Unequal bonds
    with a weight that does not vanish: the test above."""
    psi, cfg = _state("theta_unequal", 2, dt, seed=33)
    _check_configs(_rescaled(psi), [cfg], dt, f"theta_unequal {dt.__name__}", general=False, slack=True)      # (both contractions are 0 up to rounding: nothing to compare them by)


@functools.lru_cache(maxsize=None)
def _grid_cache(dt, chi):
    return _rescaled(tn.random_tensornetworkstate(dt, tn.named_grid((3, 3)), chi, seed=40 + chi))


def _connected_configs(g, max_edges):
    rg = lr.RefGraph(g.vertices, g.edges)
    return [list(c) for c in lr.configurations(rg, max_edges, connected_only=True)], rg


@pytest.mark.parametrize("dt", DTS)
def test_a_cycle_through_the_new_entry_is_loop_weights_to_the_bit(dt):
    r = _grid_cache(dt, 4)
    configs, rg = _connected_configs(r.graph, 8)
    cycles = [c for c in configs if br.decompose(rg, c)["shape"] == "cycle"]
    assert sorted(len(c) for c in cycles) == [4] * 4 + [6] * 4 + [8] * 5      # 8: the outer ring and the boundaries of the four L-shaped plaquette triples
    rings = [br.decompose(rg, c)["ring"] for c in cycles]       # from the lowest vertex towards its lower ring neighbour
    a, b = tn.configuration_weights(r, cycles), tn.loop_weights(r, rings)
    assert np.array_equal(a.view(np.float64), b.view(np.float64)) and np.all(a != 0)


@pytest.mark.parametrize("dt", DTS)
def test_all_configurations_of_the_3x3_grid_up_to_9_edges_in_one_call(dt):
    r = _grid_cache(dt, 2)
    configs, rg = _connected_configs(r.graph, 9)
    shapes = [br.decompose(rg, c)["shape"] for c in configs]
    assert set(shapes) == {"cycle", "theta", "eight"}           # nine edges of a square lattice never close a third loop
    print(f"3x3 up to 9 edges: {len(configs)} configurations, {shapes.count('theta')} thetas, {shapes.count('eight')} figure-eights")
    _check_configs(r, configs, dt, f"3x3 <= 9 edges {dt.__name__}")


@pytest.mark.parametrize("dt", DTS)
def test_edge_order_and_orientation_do_not_change_a_bit(dt):
    r = _grid_cache(dt, 2)
    g33 = cases()
    configs = [g33["theta_244"][1], g33["eight"][1]] + [[tuple(e) for e in r.graph.edges if e[0][0] <= 2 and e[1][0] <= 2]]      # + the theta of the upper 2 x 3 block
    base = tn.configuration_weights(r, configs)
    rng = np.random.default_rng(8)
    for _ in range(3):
        mixed = [[c[i] if rng.integers(2) else c[i][::-1] for i in rng.permutation(len(c))] for c in configs]
        again = tn.configuration_weights(r, mixed)
        assert np.array_equal(base.view(np.float64), again.view(np.float64))
    assert np.all(base != 0)


@pytest.mark.parametrize("dt", DTS)
def test_weights_with_a_pending_site_scale_and_pending_one_site_gates(dt):
    """as tests/test_gpu_loops.py sets it up: one normalising gate layer leaves a pending scale and pending one-site gates; the cache is NOT rescaled"""
    g = tn.named_grid((3, 3))
    bpc = tn.update(tn.BeliefPropagationCache(tn.random_tensornetworkstate(dt, g, 3, seed=77)), **BP_KW)
    layer = [("Rx", [v], 0.3) for v in g.vertices] + [("Rzz", [a, b], 0.2) for grp in tn.edge_color(g) for (a, b) in grp] + [("Rx", [v], 0.1) for v in g.vertices]
    bpc, _ = tn.apply_gates(layer, bpc, apply_kwargs=dict(maxdim=3, cutoff=None, normalize_tensors=True), bp_update_kwargs=BP_KW)
    cs = cases()
    configs = [cs["theta_244"][1], cs["eight"][1], [tuple(e) for e in g.edges if e[0][0] <= 2 and e[1][0] <= 2]]
    fac = C.c_double(0.0)
    verts = {v for c in configs for e in c for v in e}
    for v in verts:
        assert lib.tnqs_dbg_pending_scale(bpc._h, g.index[v], C.byref(fac)) == 0
        assert abs(fac.value - 1.0) > 1e-3, (v, fac.value)
    _check_configs(bpc, configs, dt, f"pending scale {dt.__name__}")


# ---- chi = 16: the case the host route refuses ----------------------------------------------------------------------------------------------------
def test_chi_16_theta_of_the_2x3_grid():
    dt = np.complex64
    g = tn.named_grid((2, 3))
    big = tn.update(tn.BeliefPropagationCache(tn.random_tensornetworkstate(dt, g, 16, seed=6)), maxiter=30, tolerance=None)
    with pytest.raises(tn.TnqsError, match=r"2\^24"):
        tn.loopcorrected_partitionfunction(big, 7)               # the default route, as before
    r = tn.rescale(big)
    configs, rg = _connected_configs(g, 7)
    assert sorted(len(c) for c in configs) == [4, 4, 6, 7]
    got, refs, bounds = _check_configs(r, configs, dt, "2x3 chi16 complex64", general=False)
    z = tn.loopcorrected_partitionfunction(big, 7, branched="device")
    want = tn.partitionfunction(big) * (1 + np.sum(got))
    print(f"MEASURED chi16 Z = {z:.8e}, Z_bp (1 + sum W) = {want:.8e}")
    assert abs(z - want) <= 1e-12 * abs(z)
    assert z == tn.norm_sqr(big, "loopcorrections", 7, branched="device")


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------------
def _summed_bound(tensors, g, ne, dt):
    """(sum W, summed bound, Z_bp) from the restatement at the fixed point: components with three or more loops are contracted on the host in complex128 (no device bound)"""
    rg = lr.RefGraph(g.vertices, g.edges)
    c128 = {v: t.astype(np.complex128) for v, t in tensors.items()}
    ts, ms, zbp = lr.rescale(c128, lr.bp(c128, rg), rg)
    cache = {}
    wsum, bsum = 0.0, 0.0
    for c in lr.configurations(rg, ne):
        parts = []
        for comp in lr.components(c):
            key = frozenset(frozenset(e) for e in comp)
            if key not in cache:
                loops = len(comp) - len({v for e in comp for v in e}) + 1
                cache[key] = _reference(ts, ms, rg, list(comp), dt, general=False) if loops <= 2 else (lr.weight(ts, ms, rg, comp), 0.0)
            parts.append(cache[key])
        wsum += np.prod([w for w, _ in parts])
        bsum += sum(b * np.prod([abs(w) for j, (w, _) in enumerate(parts) if j != i]) for i, (_, b) in enumerate(parts))
    return wsum, bsum, zbp


@pytest.mark.parametrize("name", ["grid2x3_chi2", "bridged_triangles_chi2"])
@pytest.mark.parametrize("dt", DTS)
def test_full_order_norm_sqr_on_the_device_route_is_the_exact_norm(dt, name):
    og, chi, seed = fixtures()[name]
    tensors = {v: t.astype(dt) for v, t in o.random_state(np.complex128, og, chi, seed=seed).tensors.items()}
    exact = float(np.sum(np.abs(sv.tns_to_statevector(o.TensorNetworkState(og, tensors))) ** 2))
    g = tn.NamedGraph(og.vertices, og.edges)
    psi = tn.TensorNetworkState(g, tensors)
    z = tn.norm_sqr(psi, alg="loopcorrections", max_configuration_size=g.ne(), cache_update_kwargs=BP_KW, branched="device")
    dev = abs(z - exact) / exact
    if dt is np.complex64:
        bound = 1e-5
    else:
        wsum, bsum, _ = _summed_bound(tensors, g, g.ne(), dt)
        bound = max(10 * FULL_ORDER_BASELINE[name], bsum / abs(1 + wsum))
    print(f"MEASURED norm_sqr branched=device {name} {dt.__name__}: |Z - exact| / exact = {dev:.3e} (bound {bound:.3e})")
    assert dev <= bound
    assert abs(tn.norm_sqr(psi, alg="bp", cache_update_kwargs=BP_KW) - exact) / exact > 1e-4
    assert abs(tn.norm(psi, alg="loopcorrections", max_configuration_size=g.ne(), cache_update_kwargs=BP_KW, branched="device") - np.sqrt(z)) <= 1e-12 * abs(np.sqrt(z))


@pytest.mark.parametrize("dt", DTS)
def test_order_10_on_the_3x3_grid_mixes_device_and_host_components(dt):
    """up to 10 edges: cycles, thetas and figure-eights on the device, the components with three loops (the grid without a corner) on the host, in one sum.
    NOT the full order (12) and hence not the exact norm: the host route refuses a configuration on all nine vertices with three or more loops (57 indices,
    it takes 52), with either value of `branched`.  The sum is compared with the restatement's sum of the same order at the fixed point.
    complex128 bound: max(1e-12 -- what tests/test_loop_ref_cpu.py asserts of such a sum --, summed device bounds / |1 + sum W|); complex64: the project's 1e-5"""
    g = tn.named_grid((3, 3))
    psi = tn.random_tensornetworkstate(dt, g, 2, seed=12)
    loops = [len(c) - len({v for e in c for v in e}) + 1 for c in _connected_configs(g, 10)[0]]
    assert max(loops) == 3 and 2 in loops
    z = tn.norm_sqr(psi, alg="loopcorrections", max_configuration_size=10, cache_update_kwargs=BP_KW, branched="device")
    wsum, bsum, zbp = _summed_bound(dict(psi.tensors), g, 10, dt)
    want = zbp * (1 + wsum)
    dev = abs(z - want) / abs(want)
    bound = 1e-5 if dt is np.complex64 else max(1e-12, bsum / abs(1 + wsum))
    print(f"MEASURED norm_sqr branched=device 3x3 chi2 order 10 {dt.__name__}: |Z - restatement| / |Z| = {dev:.3e} (bound {bound:.3e})")
    assert dev <= bound
    # the two routes agree where both run: up to 9 edges (the default route contracts the ten-edge thetas on all nine vertices on the host: 57 indices, refused)
    z9 = tn.norm_sqr(psi, alg="loopcorrections", max_configuration_size=9, cache_update_kwargs=BP_KW, branched="device")
    zh = tn.norm_sqr(psi, alg="loopcorrections", max_configuration_size=9, cache_update_kwargs=BP_KW)
    print(f"MEASURED 3x3 chi2 order 9 {dt.__name__}: |device route - host route| / |Z| = {abs(z9 - zh) / abs(zh):.3e}")
    assert abs(z9 - zh) <= 2 * bound * abs(zh) and abs(z9 - z) > 0
    with pytest.raises(tn.TnqsError, match="52"):
        tn.norm_sqr(psi, alg="loopcorrections", max_configuration_size=12, cache_update_kwargs=BP_KW, branched="device")


@pytest.mark.parametrize("dt", DTS)
def test_full_order_on_k4_mixes_device_and_host_components_and_is_the_exact_norm(dt):
    """K4 at chi = 2, all 6 edges: four triangles, three squares and six thetas on the device, K4 itself (three loops, 28 indices) on the host, in one sum against
    exact contraction.  complex128 bound: max(1e-12 -- what tests/test_loop_ref_cpu.py asserts of a full-order sum --, summed device bounds / |1 + sum W|)"""
    edges = [(a, b) for a in range(4) for b in range(a + 1, 4)]
    g = tn.NamedGraph(range(4), edges)
    psi = tn.random_tensornetworkstate(dt, g, 2, seed=14)
    exact = float(np.sum(np.abs(sv.tns_to_statevector(o.TensorNetworkState(o.Graph(list(range(4)), edges), dict(psi.tensors)))) ** 2))
    shapes = [br.decompose(lr.RefGraph(g.vertices, g.edges), c)["shape"] for c in _connected_configs(g, 6)[0]]
    assert sorted(map(str, shapes)) == ["None"] + ["cycle"] * 7 + ["theta"] * 6
    z = tn.norm_sqr(psi, alg="loopcorrections", max_configuration_size=6, cache_update_kwargs=BP_KW, branched="device")
    dev = abs(z - exact) / exact
    if dt is np.complex64:
        bound = 1e-5
    else:
        wsum, bsum, _ = _summed_bound(dict(psi.tensors), g, 6, dt)
        bound = max(1e-12, bsum / abs(1 + wsum))
    print(f"MEASURED norm_sqr branched=device K4 chi2 full order {dt.__name__}: |Z - exact| / exact = {dev:.3e} (bound {bound:.3e})")
    assert dev <= bound
    assert abs(tn.norm_sqr(psi, alg="bp", cache_update_kwargs=BP_KW) - exact) / exact > 1e-4


# ---- errors -----------------------------------------------------------------------------------------------------------------------------------
def _call(bpc, configs, out=None):
    g = bpc.graph
    n = _ints([len(c) for c in configs])
    eu = _ints([g.index[a] for c in configs for (a, b) in c]); ev = _ints([g.index[b] for c in configs for (a, b) in c])
    out = np.zeros(len(configs), dtype=np.complex128) if out is None else out
    return lib.tnqs_config_weights(bpc._h, len(configs), _p(n), _p(eu), _p(ev), _p(out))


def test_empty_call_invalid_and_unsupported_configurations():
    bpc = _grid_cache(np.complex64, 2)
    g = bpc.graph
    assert lib.tnqs_config_weights(bpc._h, 0, None, None, None, None) == 0
    assert len(tn.configuration_weights(bpc, [])) == 0
    sq = [((1, 1), (2, 1)), ((2, 1), (2, 2)), ((1, 2), (2, 2)), ((1, 1), (1, 2))]
    bad = {"an edge that is not in the graph": sq[:3] + [((1, 1), (2, 2))],
           "a repeated edge": sq + [((2, 1), (1, 1))],
           "a disconnected set": sq + [((3, 2), (3, 3))],
           "a vertex of internal degree 1": sq + [((2, 2), (3, 2))]}
    for what, cfg in bad.items():
        assert _call(bpc, [cfg]) == ERR_INVALID, (what, lib.tnqs_last_error())
        with pytest.raises(tn.TnqsError):
            tn.configuration_weights(bpc, [cfg])
    out = np.zeros(1, dtype=np.complex128)
    n, e = _ints([4]), _ints([0, 1, 2, 3])
    for args in ((None, _p(e), _p(e), _p(out)), (_p(n), None, _p(e), _p(out)), (_p(n), _p(e), None, _p(out)), (_p(n), _p(e), _p(e), None)):
        assert lib.tnqs_config_weights(bpc._h, 1, *args) == ERR_INVALID
    assert lib.tnqs_config_weights(bpc._h, 1, _p(n), _p(_ints([0, 1, 2, 99])), _p(e), _p(out)) == ERR_INVALID       # a vertex that does not exist
    with pytest.raises(tn.TnqsArgumentError):
        tn.configuration_weights(bpc, [[("nowhere", (1, 1))]])
    # three independent loops: refused by the call, summed on the host by the partition function
    three = [tuple(e) for e in g.edges if not (e[0] == (3, 3) or e[1] == (3, 3))]
    assert len(three) - len({v for e in three for v in e}) + 1 == 3
    assert _call(bpc, [three]) == ERR_UNSUPPORTED and b"independent loops" in lib.tnqs_last_error()
    with pytest.raises(tn.TnqsError, match="independent loops"):
        tn.configuration_weights(bpc, [three])
    assert tuple(three) in {tuple(c) for c in tn.leafless_edge_induced_subgraphs(g, 10)}
    zd, z9 = tn.loopcorrected_partitionfunction(bpc, 10, branched="device"), tn.loopcorrected_partitionfunction(bpc, 9, branched="device")
    assert np.isfinite(zd) and zd != z9                           # (its value: test_order_10_on_the_3x3_grid_mixes_device_and_host_components)
    for fn in (lambda: tn.loopcorrected_partitionfunction(bpc, 7, branched="gpu"), lambda: tn.norm_sqr(bpc, "loopcorrections", 7, branched=True),
               lambda: tn.norm(bpc, "loopcorrections", max_configuration_size=7, branched="")):
        with pytest.raises(tn.TnqsArgumentError, match="branched"):
            fn()


def test_a_sharded_handle_is_refused():
    """a two-rank handle on one GPU as tests/test_gpu_amplitudes.py sets it up.  (The third TNQS_ERR_UNSUPPORTED case, a vertex of degree > 7, cannot be reached
    from a test: tnqs_set_site_tensor refuses such a tensor, so no handle holds one; the check in decompose() is a second line of defence.)"""
    g = tn.named_grid((2, 3))
    bpc = tn.BeliefPropagationCache(tn.random_tensornetworkstate(np.complex64, g, 2, seed=61))
    theta = [tuple(e) for e in g.edges]
    buf = C.c_void_p()
    lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]; lib.hipFree.argtypes = [C.c_void_p]
    assert lib.hipMalloc(C.byref(buf), 1 << 16) == 0 and buf.value
    try:
        cb = L.ALLGATHER_FN(lambda ctx, base, nbytes, nranks: -1)
        owner, op = L.i32([0, 0, 0, 1, 1, 1])
        L.check(L.lib.tnqs_set_sharding(bpc._h, 0, 2, op, cb, None, buf, 1 << 16))
        out = np.full(1, np.nan + 0j)
        assert _call(bpc, [theta], out) == ERR_UNSUPPORTED and np.isnan(out[0].real) and b"sharded" in lib.tnqs_last_error()
        with pytest.raises(tn.TnqsError, match="sharded"):
            tn.configuration_weights(bpc, [theta])
        del bpc
    finally:
        lib.hipFree(buf)
