"""GPU tests of inner(psi, phi; alg = "bp"): the rectangular Gram and the bilinear message epilogue (csrc/kernels_inner.hip) through their debug entry points
against extended-precision numpy, and tnqs_inner_bp / tn.inner end to end against the numpy restatement of tests/inner_ref.py run on identical inputs (tensors read
back from the handles, the same sequence, a fixed number of sweeps, no tolerance); log z is compared with its imaginary part modulo 2 pi.

Tolerances (none of them measured on the kernels):
  Gram      per entry 8 u (N + nchunks) sum|x||y|, u = 2^-24 (f32 accumulation) / 2^-53, N the contracted length: the worst case of any summation order of the N
            products and the nchunks partials, the factor 8 for the four real products of a complex one and the rounding of the result
  epilogue  the bound tests/test_gpu_small_site.py holds msg_finalize_kernel to, with rows cols in place of chi^2: nchunks eps sum|partials| per element
            (eps = 2^-23 / 2^-52), carried through the division for normalised messages; message_diff 1e-12 against the f64 formula on the kernel's own new_msg
  log z     complex64: 1e-6 (nv + ne) -- each of the nv vertex scalars is one f32 contraction held to the 1e-6 the f32 kernel tests hold, the ne edge scalars are f64
            sums, log z is stationary in the messages and no vertex scalar cancels (tests/test_inner_ref_cpu.py holds the cancellation factor at or below 2);
            complex128: 200 eps (nv + ne); symmetries: twice that"""
import ctypes as C

import numpy as np
import pytest

import tnqs_amd as tn
import tnqs_oracle as o
import inner_ref as ref

pytestmark = pytest.mark.gpu
lib = C.CDLL(tn.LIB_PATH)
ERR_INVALID, ERR_UNSUPPORTED = -1, -2                    # include/tnqs.h
ROUTE_INNER_MFMA = 9                                     # include/tnqs_debug.h
EPS64 = np.finfo(np.float64).eps
DT = {0: np.complex64, 1: np.complex128}


def _ints(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.int32))


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _measured(what, err, bound):
    print(f"MEASURED {what}: {err:.3e} (bound {bound:.3e})")


def _guarded(dt, sizes, guard):
    """guard, item 0, guard, item 1, ..., guard, filled with a sentinel; returns the array and the items' offsets"""
    sent = dt(-7.5 + 3.25j)
    offs, n = [], guard
    for s in sizes:
        offs.append(n); n += s + guard
    return np.full(n, sent, dtype=dt), offs, sent


def _guards_intact(buf, offs, sizes, guard, sent):
    keep = np.ones(buf.size, dtype=bool)
    for off, s in zip(offs, sizes):
        keep[off:off + s] = False
    return bool(np.all(buf[keep] == sent))


# ---- 1. rectangular Gram --------------------------------------------------------------------------------------------------------------------------------------------
GRAM_SHAPES = [(2, 1, 1, 1), (2, 2, 3, 3), (2, 3, 2, 5), (6, 5, 8, 7), (2, 16, 16, 16), (2, 17, 31, 9), (4, 32, 32, 32), (2, 33, 64, 8), (2, 64, 64, 16), (2, 64, 33, 8)]
GUARD = 5


def inner_gram(dtype, shapes, xs, ys, max_chunks):
    """one tnqs_dbg_inner_gram call; xs[i]: array (PB, Ka, PA) (= column-major [PA][Ka][PB]); returns (rc, outs (Kb, Ka), nchunks, route, guards intact)"""
    dt = DT[dtype]
    X = np.concatenate([x.ravel() for x in xs]).astype(dt)
    Y = None if ys is None else np.concatenate([y.ravel() for y in ys]).astype(dt)
    sizes = [s[1] * s[2] for s in shapes]
    out, offs, sent = _guarded(dt, sizes, GUARD)
    nch = np.zeros(len(shapes), dtype=np.int32); route = C.c_int(0)
    rc = lib.tnqs_dbg_inner_gram(dtype, len(shapes), _p(_ints(np.array(shapes).ravel())), _p(X), _p(Y), _p(out), max_chunks, _p(nch), GUARD, C.byref(route))
    outs = [out[off:off + s].reshape(sh[2], sh[1]).copy() for off, s, sh in zip(offs, sizes, shapes)]
    return rc, outs, nch, route.value, _guards_intact(out, offs, sizes, GUARD, sent), out, sent


def _gram_check(dtype, shapes, xs, ys, outs, nch, what):
    u = 2.0 ** -24 if dtype == 0 else 2.0 ** -53
    worst = 0.0
    for sh, x, y, got, nc in zip(shapes, xs, ys, outs, nch):
        xl, yl = x.astype(DT[dtype]).astype(np.clongdouble), y.astype(DT[dtype]).astype(np.clongdouble)
        want = np.einsum("qap,qbp->ba", xl, yl.conj())
        mag = np.einsum("qap,qbp->ba", np.abs(xl), np.abs(yl))
        bound = 8 * u * (sh[0] * sh[3] + int(nc)) * mag
        err = np.abs(got.astype(np.clongdouble) - want)
        ratio = float(np.max(err / bound))
        assert ratio <= 1.0, (what, sh, ratio)
        worst = max(worst, ratio)
    _measured(f"inner_gram {what}: largest error / bound", worst, 1.0)


@pytest.mark.parametrize("max_chunks", [0, 4])
@pytest.mark.parametrize("dtype", [0, 1])
def test_rectangular_gram_mixed_shapes_in_one_launch(dtype, max_chunks):
    rng = np.random.default_rng([11, dtype])
    xs = [ref.crandn(rng, (s[3], s[1], s[0])) for s in GRAM_SHAPES]
    ys = [ref.crandn(rng, (s[3], s[2], s[0])) for s in GRAM_SHAPES]
    rc, outs, nch, route, intact, _, _ = inner_gram(dtype, GRAM_SHAPES, xs, ys, max_chunks)
    assert rc == 0 and route == ROUTE_INNER_MFMA and intact
    if max_chunks:
        assert nch[GRAM_SHAPES.index((4, 32, 32, 32))] >= 3          # 128 contracted indices: 4 blocks of 32 (f32) / 8 of 16 (f64)
    _gram_check(dtype, GRAM_SHAPES, xs, ys, outs, nch, f"dtype {dtype} max_chunks {max_chunks}")


@pytest.mark.parametrize("dtype", [0, 1])
def test_rectangular_gram_with_y_equal_x(dtype):
    shapes = [s for s in GRAM_SHAPES if s[1] == s[2]]
    rng = np.random.default_rng([12, dtype])
    xs = [ref.crandn(rng, (s[3], s[1], s[0])) for s in shapes]
    rc, outs, nch, route, intact, _, _ = inner_gram(dtype, shapes, xs, None, 0)
    assert rc == 0 and route == ROUTE_INNER_MFMA and intact
    _gram_check(dtype, shapes, xs, xs, outs, nch, f"dtype {dtype} Y == X")
    for got in outs:                                     # a Gram of X with itself is Hermitian whatever the rounding of the products
        assert np.allclose(got, got.conj().T, rtol=0, atol=1e-4 * np.max(np.abs(got)))


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("shape", [(2, 65, 3, 2), (2, 3, 65, 2)])
def test_rectangular_gram_refuses_a_dimension_beyond_64(dtype, shape):
    rng = np.random.default_rng(13)
    xs, ys = [ref.crandn(rng, (shape[3], shape[1], shape[0]))], [ref.crandn(rng, (shape[3], shape[2], shape[0]))]
    rc, _, _, _, _, out, sent = inner_gram(dtype, [shape], xs, ys, 0)
    assert rc == ERR_UNSUPPORTED and np.all(out == sent)


# ---- 2. epilogue ----------------------------------------------------------------------------------------------------------------------------------------------------
FIN_SHAPES = [(1, 1), (2, 3), (3, 2), (16, 16), (17, 31), (64, 33)]
FIN_NCHUNKS = [1, 5]


def inner_finalize(dtype, shapes, nchunks, partials, olds, normalize):
    """one tnqs_dbg_inner_finalize call; partials[i]: (nchunks, cols, rows) (= [chunk][a + rows b]); returns [(new (cols, rows), diff, sum)], guards intact"""
    dt = DT[dtype]
    n = len(shapes)
    P = np.concatenate([p.ravel() for p in partials]).astype(dt)
    has_old = _ints([0 if (olds is None or q is None) else 1 for q in (olds or [None] * n)])
    old = None if olds is None else np.concatenate([(np.zeros((c, r)) if q is None else q).ravel() for q, (r, c) in zip(olds, shapes)]).astype(dt)
    sizes = [r * c for r, c in shapes]
    new, offs, sent = _guarded(dt, sizes, GUARD)
    diff = np.zeros(n); ssum = np.zeros(2 * n)
    rc = lib.tnqs_dbg_inner_finalize(dtype, n, _p(_ints([s[0] for s in shapes])), _p(_ints([s[1] for s in shapes])), _p(_ints(nchunks)), _p(P), _p(old), _p(has_old),
                                     _p(_ints(normalize)), _p(new), _p(diff), _p(ssum), GUARD)
    assert rc == 0
    res = [(new[off:off + s].reshape(c, r).copy(), diff[i], complex(ssum[2 * i], ssum[2 * i + 1])) for i, (off, s, (r, c)) in enumerate(zip(offs, sizes, shapes))]
    return res, _guards_intact(new, offs, sizes, GUARD, sent)


def _fin_partials(rng, r, c, nch, dt):
    """partials whose element sum does not cancel: a common positive part plus noise"""
    base = 1.0 + 0.3 * ref.crandn(rng, (c, r))
    return np.stack([(base / nch + 0.1 / np.sqrt(nch) * ref.crandn(rng, (c, r))).astype(dt) for _ in range(nch)])


def _diff_ref(new, old, r, c):
    return o.message_diff(new.astype(np.complex128), ref.delta(r, c).T if old is None else old.astype(np.complex128))       # (arrays are (cols, rows))


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("dtype", [0, 1])
def test_epilogue_every_shape_and_chunk_count_in_one_launch(dtype, normalize):
    dt = DT[dtype]
    eps = 2.0 ** -23 if dtype == 0 else 2.0 ** -52
    rng = np.random.default_rng([21, dtype])
    shapes = [s for s in FIN_SHAPES for _ in FIN_NCHUNKS]
    nchunks = [n for _ in FIN_SHAPES for n in FIN_NCHUNKS]
    partials = [_fin_partials(rng, r, c, n, dt) for (r, c), n in zip(shapes, nchunks)]
    olds = [None if i % 3 == 0 else ref.crandn(rng, (c, r)).astype(dt) for i, (r, c) in enumerate(shapes)]
    res, intact = inner_finalize(dtype, shapes, nchunks, partials, olds, [normalize] * len(shapes))
    assert intact
    worst = worst_d = 0.0
    for (r, c), nch, p, old, (new, diff, ssum) in zip(shapes, nchunks, partials, olds, res):
        p = p.astype(np.complex128)
        m = p.sum(axis=0)
        B = nch * eps * np.abs(p).sum(axis=0)            # summation bound of any order, per element
        s = m.sum()
        assert abs(ssum - s) <= B.sum()
        if normalize:
            # got = fl(m~ / s~), |m~ - m| <= B, |s~ - s| <= sum(B): |got - m / s| <= B / |s~| + |m| sum(B) / (|s| |s~|) + 4 eps |m / s|, |s~| >= |s| - sum(B)
            assert abs(s) / np.abs(m).sum() >= 0.1
            sl = abs(s) - B.sum()
            tol = B / sl + np.abs(m) * B.sum() / (abs(s) * sl) + 4 * eps * np.abs(m / s)
            m = m / s
        else:
            tol = B + eps * np.abs(m)
        ratio = float(np.max(np.abs(new - m) / tol))
        assert ratio <= 1.0, (r, c, nch, ratio)
        worst = max(worst, ratio)
        dd = abs(diff - _diff_ref(new, old, r, c))
        assert dd < 1e-12, (r, c, nch, diff)
        worst_d = max(worst_d, dd)
    _measured(f"inner_finalize dtype {dtype} normalize {normalize} new_msg: largest error / bound", worst, 1.0)
    _measured(f"inner_finalize dtype {dtype} normalize {normalize} message_diff", worst_d, 1e-12)


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("r,c,nch", [(2, 3, 1), (17, 31, 5), (64, 33, 5)])
def test_epilogue_leaves_an_exactly_zero_sum_unnormalised(dtype, r, c, nch):
    """small-integer partials whose elements come in (p, -p) pairs: every sum is exact, the element sum is exactly zero, the output is the plain reduction bit for bit"""
    rng = np.random.default_rng(r + c + nch)
    half = (r * c) // 2
    v = rng.integers(-8, 9, size=(nch, half)) + 1j * rng.integers(-8, 9, size=(nch, half))
    flat = np.zeros((nch, r * c), dtype=np.complex128)
    flat[:, 0:2 * half:2] = v; flat[:, 1:2 * half:2] = -v
    partials = flat.reshape(nch, c, r).astype(DT[dtype])
    m = flat.sum(axis=0).reshape(c, r)
    assert m.sum() == 0 and np.max(np.abs(m)) > 0
    ((new, diff, ssum),), intact = inner_finalize(dtype, [(r, c)], [nch], [partials], None, [1])
    assert intact and ssum == 0 and np.array_equal(new.astype(np.complex128), m)
    assert abs(diff - _diff_ref(m, None, r, c)) < 1e-12
    _measured(f"inner_finalize dtype {dtype} zero sum {r} x {c} nchunks {nch}", float(np.max(np.abs(new - m))), 0.0)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------------------------------
def tn_graph(og):
    return tn.NamedGraph(list(og.vertices), list(og.edges))


def cache_of(og, tensors, dt):
    g = tn_graph(og)
    return tn.BeliefPropagationCache(tn.TensorNetworkState(g, {v: np.ascontiguousarray(tensors[v]).astype(dt) for v in og.vertices}))


def read_back(bpc, og):
    return {v: bpc.tensor(v).astype(np.complex128) for v in og.vertices}


def bound_of(og, dt, factor=1.0):
    n = len(og.vertices) + len(og.edges)
    return factor * (1e-6 if np.dtype(dt) == np.complex64 else 200 * EPS64) * n


def _compare(what, og, K, B, nsweeps, dt, seq=None, factor=1.0):
    seq = o.forest_cover_edge_sequence(og) if seq is None else seq
    got = tn.log_inner(K, B, cache_update_kwargs=dict(maxiter=nsweeps, edge_sequence=seq))
    want = ref.log_inner(ref.run(og, read_back(K, og), read_back(B, og), nsweeps, seq=seq))
    err, bound = ref.log_close(got, want), bound_of(og, dt, factor)
    _measured(f"log z {what} {np.dtype(dt).name} after {nsweeps} sweeps", err, bound)
    assert err <= bound, (got, want)
    return got


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
@pytest.mark.parametrize("name", ["comb33", "path5"])
def test_trees_one_sweep_is_the_dense_overlap(name, dt):
    og, ket, bra = ref.tree_case(name)
    K, B = cache_of(og, ket, dt), cache_of(og, bra, dt)
    info = {}
    got = tn.log_inner(K, B, info=info)                  # the defaults: one sweep of the tree order, no tolerance
    want = np.log(ref.dense_inner(og, read_back(K, og), read_back(B, og)))
    err, bound = ref.log_close(got, want), bound_of(og, dt)
    _measured(f"log z tree {name} {np.dtype(dt).name} against the dense overlap", err, bound)
    assert info["niter"] == 1 and not info["converged"]
    assert err <= bound
    z = tn.inner(K, B)
    assert abs(z - np.exp(want)) <= 2 * bound * abs(np.exp(want))


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
@pytest.mark.parametrize("name", sorted(ref.LOOPY_CASES))
def test_loopy_graphs_with_related_states(name, dt):
    og, ket, bra = ref.loopy_case(name)
    K, B = cache_of(og, ket, dt), cache_of(og, bra, dt)
    for nsweeps in (3, 8):
        _compare(name, og, K, B, nsweeps, dt)


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_library_default_sequence_and_workspace_bound(dt):
    """the library's own default order (levels of several messages; most vertex scalars need the pass after the last sweep), replayed on the reference; the same
    call with a workspace bound of one byte runs every message alone and agrees"""
    og, ket, bra = ref.loopy_case("grid3x4")
    K, B = cache_of(og, ket, dt), cache_of(og, bra, dt)
    cap = 4 * len(og.edges)
    src, dst, n = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32), C.c_int(0)
    assert lib.tnqs_dbg_default_sequence(K._h, _p(src), _p(dst), cap, C.byref(n)) == 0
    seq = [(og.vertices[a], og.vertices[b]) for a, b in zip(src[:n.value], dst[:n.value])]
    want = ref.log_inner(ref.run(og, read_back(K, og), read_back(B, og), 3, seq=seq))
    got = tn.log_inner(K, B, cache_update_kwargs=dict(maxiter=3))
    err, bound = ref.log_close(got, want), bound_of(og, dt)
    _measured(f"log z default sequence {np.dtype(dt).name}", err, bound)
    assert err <= bound
    opts = tn.core.L.BpOpts(); opts.maxiter = 3; opts.tolerance = -1.0; opts.normalize = 1; opts.n_sequence = 0
    out = np.zeros(2); nb = C.c_int(0); nb0 = C.c_int(0)
    assert lib.tnqs_dbg_inner_bp_ws(K._h, B._h, C.byref(opts), _p(out), None, None, C.c_int64(1), C.byref(nb)) == 0
    err = ref.log_close(complex(out[0], out[1]), want)
    _measured(f"log z default sequence, one message per batch ({nb.value} batches) {np.dtype(dt).name}", err, bound)
    assert err <= bound
    assert lib.tnqs_dbg_inner_bp_ws(K._h, B._h, C.byref(opts), _p(out), None, None, C.c_int64(1 << 30), C.byref(nb0)) == 0
    assert nb.value > nb0.value


def _grid33_chi(rng, chi_ket, chi_bra):
    """3 x 3 grid, ket entries 1 + 0.5 x noise at chi_ket, bra = the ket cut to chi_bra on every bond plus 0.2 x noise"""
    og = o.named_grid((3, 3))
    ket = {v: 1.0 + 0.5 * t for v, t in ref.tensors_of(og, {e: chi_ket for e in og.edges}, rng).items()}
    bra = {v: ket[v][(slice(None),) + (slice(0, chi_bra),) * (ket[v].ndim - 1)] + 0.2 * ref.crandn(rng, (2,) + (chi_bra,) * (ket[v].ndim - 1)) for v in og.vertices}
    return og, ket, bra


def test_chi_32_against_chi_16_on_the_matrix_cores():
    og, ket, bra = _grid33_chi(np.random.default_rng(32), 32, 16)
    K, B = cache_of(og, ket, np.complex64), cache_of(og, bra, np.complex64)
    _compare("3 x 3 grid chi 32 / 16", og, K, B, 2, np.complex64)


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_inner_of_a_state_with_itself_is_norm_sqr(dt):
    og, ket, _ = ref.loopy_case("grid3x4")
    K = cache_of(og, ket, dt)
    seq = o.forest_cover_edge_sequence(og)
    for nsweeps in (3, 8):
        got = tn.log_inner(K, K, cache_update_kwargs=dict(maxiter=nsweeps, edge_sequence=seq))
        want = np.log(complex(tn.norm_sqr(tn.update(K, maxiter=nsweeps, edge_sequence=seq), alg="bp")))
        err, bound = ref.log_close(got, want), bound_of(og, dt)
        _measured(f"log inner(psi, psi) against log norm_sqr {np.dtype(dt).name} after {nsweeps} sweeps", err, bound)
        assert err <= bound
    _compare("inner(psi, psi)", og, K, K, 3, dt)


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_conjugate_symmetry_and_linearity(dt):
    og, ket, bra = _grid33_chi(np.random.default_rng(6), 4, 3)
    K, B = cache_of(og, ket, dt), cache_of(og, bra, dt)
    kw = dict(maxiter=8, edge_sequence=o.forest_cover_edge_sequence(og))
    a = tn.log_inner(K, B, cache_update_kwargs=kw)
    bound = bound_of(og, dt, 2.0)
    err = ref.log_close(tn.log_inner(B, K, cache_update_kwargs=kw), np.conj(a))
    _measured(f"inner(phi, psi) against conj(inner(psi, phi)) {np.dtype(dt).name}", err, bound)
    assert err <= bound
    c = 0.7 - 1.3j
    v0 = og.vertices[4]
    scaled = dict(read_back(K, og)); scaled[v0] = c * scaled[v0]
    err = ref.log_close(tn.log_inner(cache_of(og, scaled, dt), B, cache_update_kwargs=kw), a + np.log(c))
    _measured(f"inner(c psi, phi) against c inner(psi, phi) {np.dtype(dt).name}", err, bound)
    assert err <= bound


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_pending_gates_and_scales_are_honoured(dt):
    """a handle that one apply_gates layer with normalising gates left with pending scale factors and deferred one-site gates, not read back before the call,
    against its copy after network() round-tripped it through the host"""
    og, ket, _ = ref.loopy_case("grid3x4")
    g = tn_graph(og)
    K0 = cache_of(og, ket, dt)
    groups = tn.edge_color(g, 4)
    layer = []
    for grp in groups:
        layer += [("Rzz", [a, b], 0.25) for (a, b) in grp]
    layer += [("Rx", [v], 0.5) for v in g.vertices]      # unitary one-site gates after the last two-site gate: they stay deferred
    bpkw = dict(maxiter=20, tolerance=1e-6 if dt == np.complex64 else 1e-10)
    K1, _ = tn.apply_gates(layer, tn.update(K0, **bpkw), apply_kwargs=dict(maxdim=3, cutoff=1e-12, normalize_tensors=True), bp_update_kwargs=bpkw)
    f = C.c_double(1.0); pending = 0
    for i in range(len(og.vertices)):
        assert lib.tnqs_dbg_pending_scale(K1._h, i, C.byref(f)) == 0
        pending += f.value != 1.0
    assert pending > 0
    kw = dict(maxiter=4, edge_sequence=o.forest_cover_edge_sequence(og))
    got = tn.log_inner(K1, K0, cache_update_kwargs=kw)
    K2 = tn.BeliefPropagationCache(K1.copy().network())
    want = tn.log_inner(K2, K0, cache_update_kwargs=kw)
    err, bound = ref.log_close(got, want), bound_of(og, dt)
    _measured(f"pending handle against its round-tripped copy {np.dtype(dt).name}", err, bound)
    assert err <= bound
    _compare("round-tripped copy", og, K2, K0, 4, dt)


@pytest.mark.parametrize("dt,tol", [(np.complex64, 1e-6), (np.complex128, 1e-12)])
def test_convergence_reporting(dt, tol):
    og, ket, bra = ref.loopy_case("hex2x2")
    K, B = cache_of(og, ket, dt), cache_of(og, bra, dt)
    seq = o.forest_cover_edge_sequence(og)
    info, rinfo = {}, {}
    got = tn.log_inner(K, B, cache_update_kwargs=dict(maxiter=40, tolerance=tol, edge_sequence=seq), info=info)
    fc = ref.run(og, read_back(K, og), read_back(B, og), 40, seq=seq, tolerance=tol, info=rinfo)
    print(f"MEASURED convergence {np.dtype(dt).name}: niter {info['niter']} (reference {rinfo['niter']}), diff {info['diff']:.3e} (reference {rinfo['diff']:.3e})")
    assert info["converged"] and rinfo["converged"] and info["diff"] <= tol
    assert abs(info["niter"] - rinfo["niter"]) <= 1
    assert ref.log_close(got, ref.log_inner(fc)) <= bound_of(og, dt)


def test_contract():
    og, ket, bra = ref.loopy_case("grid3x4")
    K, B = cache_of(og, ket, np.complex64), cache_of(og, bra, np.complex64)
    # neither cache's messages change across the call
    K, B = tn.update(K, maxiter=2), tn.update(B, maxiter=2)
    edges = [e for (a, b) in tn_graph(og).edges for e in ((a, b), (b, a))]
    before = [(K.message(e).tobytes(), B.message(e).tobytes()) for e in edges]
    a = tn.log_inner(K, B, cache_update_kwargs=dict(maxiter=3))
    assert before == [(K.message(e).tobytes(), B.message(e).tobytes()) for e in edges]
    # ket is bra; a TensorNetworkState argument is uploaded to a temporary handle
    assert np.isfinite(tn.log_inner(K, K, cache_update_kwargs=dict(maxiter=3)).real)
    b = tn.log_inner(K.network(), B, cache_update_kwargs=dict(maxiter=3))
    assert ref.log_close(a, b) <= bound_of(og, np.complex64)
    # a projected vertex on both sides
    v0 = og.vertices[5]
    Kp, Bp = K.project(v0, 1), B.project(v0, 1)
    seq = o.forest_cover_edge_sequence(og)
    _compare("projected vertex", og, Kp, Bp, 3, np.complex64, seq=seq)
    with pytest.raises(tn.TnqsArgumentError):
        tn.log_inner(Kp, B)                              # site dimensions 1 and 2 at v0
    out = np.zeros(2)
    assert lib.tnqs_inner_bp(Kp._h, B._h, None, _p(out), None, None) == ERR_INVALID
    # mismatched graph, element type, algorithm, null pointers
    og2 = o.named_grid((4, 3))
    ket2 = ref.tensors_of(og2, {e: 2 for e in og2.edges}, np.random.default_rng(1))
    K2 = cache_of(og2, ket2, np.complex64)
    with pytest.raises(tn.TnqsArgumentError):
        tn.inner(K, K2)
    assert lib.tnqs_inner_bp(K._h, K2._h, None, _p(out), None, None) == ERR_INVALID
    K128 = cache_of(og, ket, np.complex128)
    with pytest.raises(tn.TnqsArgumentError):
        tn.inner(K, K128)
    assert lib.tnqs_inner_bp(K._h, K128._h, None, _p(out), None, None) == ERR_INVALID
    with pytest.raises(tn.TnqsError, match='"bp"'):
        tn.inner(K, B, alg="exact")
    assert lib.tnqs_inner_bp(K._h, B._h, None, None, None, None) == ERR_INVALID
    assert lib.tnqs_inner_bp(K._h, None, None, _p(out), None, None) == ERR_INVALID
    assert lib.tnqs_inner_bp(None, B._h, None, _p(out), None, None) == ERR_INVALID
    # NULL options: 25 sweeps, no tolerance
    niter = C.c_int(0); diff = C.c_double(-1.0)
    assert lib.tnqs_inner_bp(K._h, B._h, None, _p(out), C.byref(niter), C.byref(diff)) == 0
    assert niter.value == 25 and 0 <= diff.value < 1e-9
    want = ref.log_inner(ref.run(og, read_back(K, og), read_back(B, og), 12))
    assert ref.log_close(complex(out[0], out[1]), want) <= bound_of(og, np.complex64)


def test_an_exactly_zero_overlap_gives_minus_infinity():
    """orthogonal site vectors at one vertex of a product state: the vertex scalar is exactly zero"""
    og = o.named_grid((2, 2))
    ket = {v: np.array([1.0, 0.0]).reshape((2,) + (1,) * len(og.nbrs[v])) for v in og.vertices}
    bra = dict(ket); v0 = og.vertices[0]; bra[v0] = np.array([0.0, 1.0]).reshape(ket[v0].shape)
    got = tn.log_inner(cache_of(og, ket, np.complex128), cache_of(og, bra, np.complex128))
    assert got.real == -np.inf and got.imag == 0 and tn.inner(cache_of(og, ket, np.complex128), cache_of(og, bra, np.complex128)) == 0
