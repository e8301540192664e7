"""GPU tests of the loop corrections (norm_sqr, alg = "loopcorrections"): the three kernels of csrc/kernels_loop.hip through their debug entry points
against numpy float64, tnqs_loop_weights against tests/loop_ref.py on IDENTICAL inputs (tensors and messages read back from the rescaled cache), and
norm_sqr end to end against exact contraction.

Bounds (derived, none of them measured on the kernels; u = 2^-24 for complex64, 2^-53 for complex128):
  loop_cgemm        max |dev - ref| <= 8 u k ||A||_F ||B||_F per item
  loop_antiproject  |dev - ref| <= 8 u (n + 2) (max|T| + max|f| max_c sum_i |b_i| |T_ic|): a sum of n products and one more product and sum per entry
  loop_trace        |dev - ref| <= 8 2^-53 p q sum |X_ij| |Y_ji| whatever the element type: the accumulation is in f64
  cycle weight      |dev - ref| <= 8 u L n_max prod_k ||A_k T_k||_F, the norms from the reference's matrices
  end to end        complex128: max(10 x the CPU baseline of tests/test_loop_ref_cpu.py, the summed weight bound / |1 + sum W|); complex64: the project's 1e-5"""
import ctypes as C
import functools

import numpy as np
import pytest

import tnqs_amd as tn
import tnqs_oracle as o
import statevector as sv
import loop_ref as lr
from test_loop_ref_cpu import FULL_ORDER_BASELINE, BRIDGED, fixtures

pytestmark = pytest.mark.gpu
lib = C.CDLL(tn.LIB_PATH)
ERR_INVALID = -1
U = {np.complex64: 2.0 ** -24, np.complex128: 2.0 ** -53}
DT = {np.complex64: 0, np.complex128: 1}
BP_KW = dict(maxiter=300, tolerance=None)      # no convergence test: 300 sweeps put these small states at the fixed point to rounding


def _ints(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.int32))


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _rand(rng, n, dt):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(dt)


# ---- kernel level ---------------------------------------------------------------------------------------------------------------------------
LAUNCHES = {"small": [(9, 9, 2), (25, 9, 50), (33, 65, 31)],                 # below a tile; rectangular and odd; one past a tile edge in each direction
            "tiles": [(64, 64, 64), (256, 256, 512), (9, 9, 2)]}             # exactly one tile; several tiles; and a small one in the same launch
GUARD = 96


@pytest.mark.parametrize("launch", sorted(LAUNCHES))
@pytest.mark.parametrize("opB", [0, 1])
@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_loop_cgemm_against_float64(dt, opB, launch):
    shapes = LAUNCHES[launch]
    rng = np.random.default_rng(17 + 2 * opB + len(launch))
    As = [_rand(rng, m * k, dt).reshape(k, m).T for (m, n, k) in shapes]                                         # column-major m x k
    Bs = [(_rand(rng, n * k, dt).reshape(k, n).T if opB else _rand(rng, n * k, dt).reshape(n, k).T) for (m, n, k) in shapes]      # n x k (H) or k x n (N)
    A = np.concatenate([a.T.reshape(-1) for a in As]); B = np.concatenate([b.T.reshape(-1) for b in Bs])
    tot = GUARD + sum(m * n + GUARD for (m, n, k) in shapes)
    Cbuf = np.full(tot, np.nan + 1j * np.nan, dtype=dt)
    rc = lib.tnqs_dbg_loop_cgemm(DT[dt], opB, len(shapes), _p(_ints([s[0] for s in shapes])), _p(_ints([s[1] for s in shapes])), _p(_ints([s[2] for s in shapes])),
                                 _p(A), _p(B), _p(Cbuf), GUARD)
    assert rc == 0, lib.tnqs_last_error()
    off = GUARD
    for (m, n, k), a, b in zip(shapes, As, Bs):
        got = Cbuf[off:off + m * n].reshape(n, m).T
        a64, b64 = a.astype(np.complex128), b.astype(np.complex128)
        ref = a64 @ (b64.conj().T if opB else b64)
        err, bound = np.max(np.abs(got - ref)), 8 * U[dt] * k * np.linalg.norm(a64) * np.linalg.norm(b64)
        print(f"MEASURED loop_cgemm {dt.__name__} op{'H' if opB else 'N'} {(m, n, k)}: {err:.3e} (bound {bound:.3e})")
        assert np.all(np.isfinite(got)) and err <= bound
        assert np.all(np.isnan(Cbuf[off - GUARD:off].real))                  # the guard band in front of the item
        off += m * n + GUARD
    assert np.all(np.isnan(Cbuf[off - GUARD:].real)) and off == tot          # and the one behind the last


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_loop_antiproject_against_float64(dt):
    shapes = [(9, 9), (256, 256), (9, 4)]                                     # n = 9 and n = 256 (square, as in a ring of equal bonds) and a rectangular one
    rng = np.random.default_rng(5)
    Ts = [_rand(rng, r * c, dt).reshape(c, r).T for (r, c) in shapes]
    fs = [_rand(rng, r, dt) for (r, c) in shapes]; bs = [_rand(rng, r, dt) for (r, c) in shapes]
    T = np.concatenate([t.T.reshape(-1) for t in Ts]); f = np.concatenate(fs); b = np.concatenate(bs)
    rc = lib.tnqs_dbg_loop_antiproject(DT[dt], len(shapes), _p(_ints([s[0] for s in shapes])), _p(_ints([s[1] for s in shapes])), _p(T), _p(f), _p(b))
    assert rc == 0, lib.tnqs_last_error()
    off = 0
    for (r, c), t, fv, bv in zip(shapes, Ts, fs, bs):
        got = T[off:off + r * c].reshape(c, r).T; off += r * c
        t64, f64, b64 = t.astype(np.complex128), fv.astype(np.complex128), bv.astype(np.complex128)
        ref = t64 - np.outer(f64, b64 @ t64)
        bound = 8 * U[dt] * (r + 2) * (np.max(np.abs(t64)) + np.max(np.abs(f64)) * np.max(np.abs(b64) @ np.abs(t64)))
        err = np.max(np.abs(got - ref))
        print(f"MEASURED loop_antiproject {dt.__name__} {(r, c)}: {err:.3e} (bound {bound:.3e})")
        assert err <= bound


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_loop_trace_accumulates_in_float64(dt):
    shapes = [(9, 9), (256, 256), (25, 9)]
    rng = np.random.default_rng(6)
    Xs = [_rand(rng, p * q, dt).reshape(q, p).T for (p, q) in shapes]; Ys = [_rand(rng, p * q, dt).reshape(p, q).T for (p, q) in shapes]
    X = np.concatenate([x.T.reshape(-1) for x in Xs]); Y = np.concatenate([y.T.reshape(-1) for y in Ys])
    out = np.zeros(len(shapes), dtype=np.complex128)
    rc = lib.tnqs_dbg_loop_trace(DT[dt], len(shapes), _p(_ints([s[0] for s in shapes])), _p(_ints([s[1] for s in shapes])), _p(X), _p(Y), _p(out))
    assert rc == 0, lib.tnqs_last_error()
    for (p, q), x, y, got in zip(shapes, Xs, Ys, out):
        x64, y64 = x.astype(np.complex128), y.astype(np.complex128)
        ref = np.sum(x64 * y64.T)
        bound = 8 * 2.0 ** -53 * p * q * np.sum(np.abs(x64) * np.abs(y64.T))
        print(f"MEASURED loop_trace {dt.__name__} {(p, q)}: {abs(got - ref):.3e} (bound {bound:.3e})")
        assert abs(got - ref) <= bound


# ---- weights on identical inputs ----------------------------------------------------------------------------------------------------------------
def _ring_graph(L):
    return tn.NamedGraph(range(L), [(k, (k + 1) % L) for k in range(L)])


def _read_back(bpc):
    g = bpc.graph
    ts = {v: bpc.tensor(v).astype(np.complex128) for v in g.vertices}
    ms = {e: bpc.message(e).astype(np.complex128) for (a, b) in g.edges for e in ((a, b), (b, a))}
    return ts, ms, lr.RefGraph(g.vertices, g.edges)


def _check_weights(bpc, rings, dt, tag):
    """tnqs_loop_weights on `bpc` as it stands against the reference's ring matrices from what the cache holds; returns (weights, bounds)"""
    got = tn.loop_weights(bpc, rings)                    # first: reading a tensor back materialises what is pending on it
    ts, ms, rg = _read_back(bpc)
    bounds = []
    for ring, w in zip(rings, got):
        mats = lr.cycle_matrices(ts, ms, rg, ring)
        ref = lr.cycle_weight(mats)
        assert abs(ref - lr.weight(ts, ms, rg, [(ring[k], ring[(k + 1) % len(ring)]) for k in range(len(ring))])) <= 1e-12 * max(1.0, abs(ref))
        bound = 8 * U[dt] * len(ring) * max(max(m.shape) for m in mats) * np.prod([np.linalg.norm(m) for m in mats])
        print(f"MEASURED loop_weights {tag} ring {ring}: |dev - ref| = {abs(w - ref):.3e} (bound {bound:.3e}, |W| = {abs(ref):.3e})")
        assert abs(w - ref) <= bound, (tag, ring, w, ref)
        bounds.append(bound)
    return got, bounds


def _rescaled(psi):
    return tn.rescale(tn.update(tn.BeliefPropagationCache(psi), **BP_KW))


@pytest.mark.parametrize("chi", [2, 3, 5])
@pytest.mark.parametrize("L", [3, 4, 6])
@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_ring_weights(dt, L, chi):
    psi = tn.random_tensornetworkstate(dt, _ring_graph(L), chi, seed=100 * L + chi)
    r = _rescaled(psi)
    b, bb = _check_weights(r, [list(range(L))], dt, f"ring{L} chi{chi} {dt.__name__}")
    if L == 4:                                                   # the other orientation and another start: the same number, each within its bound of it
        a, ba = _check_weights(r, [[2, 1, 0, 3]], dt, "ring4 reversed")
        assert abs(a[0] - b[0]) <= ba[0] + bb[0]


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_ring_with_unequal_bonds_has_rectangular_transfer_matrices(dt):
    g = _ring_graph(4)
    bond = {frozenset((0, 1)): 2, frozenset((1, 2)): 3, frozenset((2, 3)): 2, frozenset((3, 0)): 3}
    rng = np.random.default_rng(9)
    tensors = {}
    for v in g.vertices:
        shp = (2,) + tuple(bond[frozenset((v, w))] for w in g.neighbors(v))
        tensors[v] = (rng.standard_normal(shp) + 1j * rng.standard_normal(shp)).astype(dt)
    _check_weights(_rescaled(tn.TensorNetworkState(g, tensors)), [[0, 1, 2, 3]], dt, f"ring4 bonds 2,3,2,3 {dt.__name__}")


PLAQUETTES = [[(1, 1), (2, 1), (2, 2), (1, 2)], [(2, 1), (3, 1), (3, 2), (2, 2)], [(1, 2), (2, 2), (2, 3), (1, 3)], [(2, 2), (3, 2), (3, 3), (2, 3)]]


@functools.lru_cache(maxsize=None)
def _grid_cache(dt, chi):
    return _rescaled(tn.random_tensornetworkstate(dt, tn.named_grid((3, 3)), chi, seed=40 + chi))


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_all_plaquettes_of_a_grid_in_one_call(dt):
    """vertices of degree 2, 3 and 4 in one launch: the contraction length of the build runs from 2 to 2 * 16"""
    _check_weights(_grid_cache(dt, 4), PLAQUETTES, dt, f"3x3 chi4 {dt.__name__}")


@pytest.mark.parametrize("chi", [8, 16])
def test_one_plaquette_at_larger_bonds(chi):
    """n = chi^2 = 64 (exactly one tile) and 256 (several tiles), complex64"""
    _check_weights(_grid_cache(np.complex64, chi), [PLAQUETTES[3]], np.complex64, f"3x3 chi{chi} complex64")


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_weights_with_a_pending_site_scale_and_pending_one_site_gates(dt):
    """one normalising gate layer leaves the site tensors with a pending scale (and pending one-site gates); tnqs_loop_weights folds both in.
    The cache is NOT rescaled here (rescaling would materialise the scale): the function computes Tr prod (A_k T_k) of whatever it is given."""
    g = tn.named_grid((3, 3))
    bpc = tn.update(tn.BeliefPropagationCache(tn.random_tensornetworkstate(dt, g, 3, seed=77)), **BP_KW)
    layer = [("Rx", [v], 0.3) for v in g.vertices] + [("Rzz", [a, b], 0.2) for grp in tn.edge_color(g) for (a, b) in grp] + [("Rx", [v], 0.1) for v in g.vertices]
    bpc, _ = tn.apply_gates(layer, bpc, apply_kwargs=dict(maxdim=3, cutoff=None, normalize_tensors=True), bp_update_kwargs=BP_KW)
    rings = PLAQUETTES[:2]
    fac = C.c_double(0.0)
    for v in {v for ring in rings for v in ring}:                # the scale really is pending on every vertex the call touches, and is no trivial factor
        assert lib.tnqs_dbg_pending_scale(bpc._h, g.index[v], C.byref(fac)) == 0
        assert abs(fac.value - 1.0) > 1e-3, (v, fac.value)
    _check_weights(bpc, rings, dt, f"pending scale {dt.__name__}")
    for v in {v for ring in rings for v in ring}:                # the call leaves it pending (the handle is not changed); the read-back of _check_weights may not
        assert lib.tnqs_dbg_pending_scale(bpc._h, g.index[v], C.byref(fac)) == 0


def test_empty_call_and_invalid_cycles():
    bpc = _grid_cache(np.complex64, 4)
    g = bpc.graph
    assert lib.tnqs_loop_weights(bpc._h, 0, None, None, None) == 0
    assert len(tn.loop_weights(bpc, [])) == 0
    out = np.zeros(2, dtype=np.complex128)
    ix = g.index
    for bad in ([(1, 1), (2, 1), (3, 1)],                         # a path: the closing pair are no neighbours
                [(1, 1), (2, 2), (1, 2)],                         # consecutive vertices that are no neighbours
                [(1, 1), (2, 1)],                                 # fewer than 3 vertices
                [(1, 1), (2, 1), (1, 1), (1, 2)]):                # a repeated vertex
        rc = lib.tnqs_loop_weights(bpc._h, 1, _p(_ints([len(bad)])), _p(_ints([ix[v] for v in bad])), _p(out))
        assert rc == ERR_INVALID, (bad, rc)
    assert lib.tnqs_loop_weights(bpc._h, 1, _p(_ints([3])), _p(_ints([0, 1, 99])), _p(out)) == ERR_INVALID
    with pytest.raises(tn.TnqsError):
        tn.loop_weights(bpc, [[(1, 1), (2, 1), (3, 1)]])


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FULL_ORDER_BASELINE))
@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_full_order_norm_sqr_is_the_exact_norm(dt, name):
    og, chi, seed = fixtures()[name]
    tensors = {v: t.astype(dt) for v, t in o.random_state(np.complex128, og, chi, seed=seed).tensors.items()}
    exact = float(np.sum(np.abs(sv.tns_to_statevector(o.TensorNetworkState(og, tensors))) ** 2))
    g = tn.NamedGraph(og.vertices, og.edges)
    psi = tn.TensorNetworkState(g, tensors)
    ne = g.ne()
    z = tn.norm_sqr(psi, alg="loopcorrections", max_configuration_size=ne, cache_update_kwargs=BP_KW)
    dev = abs(z - exact) / exact
    if dt is np.complex64:
        bound = 1e-5
    else:      # the summed bound of the device-weighed cycles, relative to 1 + sum W, from the reference's matrices
        rg = lr.RefGraph(g.vertices, g.edges)
        c128 = {v: t.astype(np.complex128) for v, t in tensors.items()}
        ts, ms, _ = lr.rescale(c128, lr.bp(c128, rg), rg)
        wsum, bsum = 0.0, 0.0
        for c in lr.configurations(rg, ne):
            parts = []                                           # (weight, bound) per component; a host-contracted component (complex128) has no device bound
            for comp in lr.components(c):
                ring = lr.ring_order(comp)
                if ring is None:
                    parts.append((lr.weight(ts, ms, rg, comp), 0.0))
                else:
                    mats = lr.cycle_matrices(ts, ms, rg, ring)
                    parts.append((lr.cycle_weight(mats), 8 * U[dt] * len(ring) * max(max(m.shape) for m in mats) * np.prod([np.linalg.norm(m) for m in mats])))
            wsum += np.prod([w for w, _ in parts])
            bsum += sum(b * np.prod([abs(w) for j, (w, _) in enumerate(parts) if j != i]) for i, (_, b) in enumerate(parts))
        bound = max(10 * FULL_ORDER_BASELINE[name], bsum / abs(1 + wsum))
    print(f"MEASURED norm_sqr loopcorrections {name} {dt.__name__}: |Z - exact| / exact = {dev:.3e} (bound {bound:.3e})")
    assert dev <= bound
    zbp = tn.norm_sqr(psi, alg="bp", cache_update_kwargs=BP_KW)
    assert abs(zbp - exact) / exact > 1e-4                       # BP alone is off: the corrections closed the gap


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_norm_sqr_bp_norm_and_trees(dt):
    g = tn.named_grid((3, 3))
    psi = tn.random_tensornetworkstate(dt, g, 2, seed=3)
    b0 = tn.BeliefPropagationCache(psi)
    bpc = tn.update(b0, **b0.default_bp_update_kwargs())        # what norm_sqr does with a TensorNetworkState (src/norm_sqr.jl:68-72)
    assert tn.norm_sqr(psi, alg="bp") == tn.partitionfunction(bpc)
    assert tn.norm_sqr(bpc, alg="bp") == tn.partitionfunction(bpc)
    z = tn.norm_sqr(bpc, alg="loopcorrections", max_configuration_size=4)
    assert tn.norm(bpc, alg="loopcorrections", max_configuration_size=4) == complex(np.sqrt(z))
    assert tn.norm(psi, alg="bp") == complex(np.sqrt(tn.partitionfunction(bpc)))
    # first order on the 3 x 3 grid: the four plaquette weights, and the same with connected_only (nothing disconnected fits 4 edges)
    r = tn.rescale(bpc)
    w = tn.loop_weights(r, PLAQUETTES)
    assert abs(z - tn.partitionfunction(bpc) * (1 + np.sum(w))) <= 1e-12 * abs(z)
    assert tn.loopcorrected_partitionfunction(bpc, 4, connected_only=True) == z
    tree = tn.named_comb_tree((3, 3))
    tb = tn.update(tn.BeliefPropagationCache(tn.random_tensornetworkstate(dt, tree, 2, seed=4)), maxiter=1)
    assert tn.norm_sqr(tb, alg="loopcorrections", max_configuration_size=9) == tn.partitionfunction(tb)      # no configurations: Z_bp unchanged


def test_errors():
    g = tn.named_grid((2, 3))
    psi = tn.random_tensornetworkstate(np.complex64, g, 2, seed=5)
    with pytest.raises(tn.TnqsError):
        tn.norm_sqr(psi, alg="exact")
    with pytest.raises(tn.TnqsArgumentError):
        tn.norm_sqr(psi, alg="loopcorrections")
    # the theta (two squares sharing an edge, 7 edges) of a 2 x 3 grid at chi = 16 is contracted on the host, and its double-layer intermediates reach
    # 16^6 = 2^24 elements: refused before anything is read back or allocated
    big = tn.update(tn.BeliefPropagationCache(tn.random_tensornetworkstate(np.complex64, g, 16, seed=6)), maxiter=2)
    with pytest.raises(tn.TnqsError, match=r"2\^24"):
        tn.loopcorrected_partitionfunction(big, 7)
    assert abs(tn.loopcorrected_partitionfunction(big, 6)) > 0            # the squares and the hexagon alone run on the device
