"""GPU tests of tnqs_amplitudes_bp / tn.log_amplitudes: the kernels of csrc/kernels_amp.hip through their debug entry points against extended-precision numpy, and the
call end to end against the numpy restatement of tests/amplitude_ref.py run on identical inputs (tensors read back from the handle, the same sequence, a fixed number of
sweeps); log a is compared with its imaginary part modulo 2 pi.

Tolerances (none of them measured on the kernels):
  leg GEMM, absorb   per entry 8 u K sum|x||y|, u = 2^-24 (f32 accumulation) / 2^-53, K the contracted length: the worst case of any summation order of the K products,
                     the factor 8 for the four real products of a complex one and the rounding of the result (the form tests/test_gpu_inner.py uses for its Gram; a
                     chain of one accumulator, so no extra partials)
  epilogue           f64 sums of at most 64 numbers of the element type: per element 64 eps64 sum|raw| carried through the division, plus the rounding of the result
                     to the element type (eps = 2^-23 / 2^-52); message_diff 1e-12 against the f64 formula on the kernel's own new_msg
  log a              the project's tolerance on log z (tests/test_gpu_inner.py): complex64 1e-6 (nv + ne), complex128 200 eps (nv + ne) -- each vertex scalar is one f32
                     contraction held to the kernel bounds above, log a is stationary in the messages and no vertex scalar cancels (tests/test_amplitude_ref_cpu.py
                     holds the cancellation factor of these inputs at or below 2)"""
import ctypes as C

import numpy as np
import pytest

import tnqs_amd as tn
import tnqs_oracle as o
import inner_ref
import amplitude_ref as ref

pytestmark = pytest.mark.gpu
lib = C.CDLL(tn.LIB_PATH)
L = tn.core.L
ERR_INVALID, ERR_UNSUPPORTED = -1, -2                    # include/tnqs.h
EPS64 = np.finfo(np.float64).eps
DT = {0: np.complex64, 1: np.complex128}
GUARD = 5


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


# ---- 1. the leg GEMM ------------------------------------------------------------------------------------------------------------------------------------------------
KS = [1, 3, 16, 32, 64]
ROWS = [(1, 1), (15, 1), (1, 15), (17, 1), (1, 17), (32, 32), (1024, 1), (1, 1024), (3, 5)]      # (PA, PB): PA = 1 the first bond leg, PB = 1 the last
GROUPS = [(0, 1), (1, 15), (16, 17), (67, 0), (15, 16), (17, 67)]                                # strings per present site value


def gemm_jobs():
    """(d, PA, K, PB, x, has_m): every K with every row shape; the group sizes, d = 3 with only x in {0, 2}, and the unset message go round"""
    jobs = []
    for i, K in enumerate(KS):
        for j, (PA, PB) in enumerate(ROWS):
            n0, n1 = GROUPS[(i + j) % len(GROUPS)]
            d = 3 if (i + j) % 4 == 3 else 2
            x = np.array([0] * n0 + [d - 1] * n1, dtype=np.int32)
            np.random.default_rng(i * 100 + j).shuffle(x)
            jobs.append((d, PA, K, PB, x, int((i + 2 * j) % 5 != 2)))
    return jobs


def leg_gemm(dtype, jobs, Ts, Ms):
    dt = DT[dtype]
    shape = _ints([[d, PA, K, PB, len(x)] for d, PA, K, PB, x, _ in jobs]).ravel()
    T = np.concatenate([t.ravel() for t in Ts]).astype(dt)
    M = np.concatenate([m.ravel() for m in Ms]).astype(dt)
    x = _ints(np.concatenate([j[4] for j in jobs]))
    sizes = [PA * PB * len(xx) for _, PA, _, PB, xx, _ in jobs]
    R, offs, sent = _guarded(dt, sizes, GUARD)
    rc = lib.tnqs_dbg_amp_leg_gemm(dtype, len(jobs), _p(shape), _p(T), _p(x), _p(M), _p(_ints([j[5] for j in jobs])), _p(R), GUARD)
    outs = [R[off:off + s].reshape(len(j[4]), j[3], j[1]).copy() for off, s, j in zip(offs, sizes, jobs)]
    return rc, outs, _guards_intact(R, offs, sizes, GUARD, sent), R, sent


@pytest.mark.parametrize("dtype", [0, 1])
def test_leg_gemm_mixed_items_in_one_launch(dtype):
    dt = DT[dtype]
    rng = np.random.default_rng([41, dtype])
    jobs = gemm_jobs()
    assert {len(j[4]) - int(np.count_nonzero(j[4])) for j in jobs} | {int(np.count_nonzero(j[4])) for j in jobs} >= {0, 1, 15, 16, 17, 67}
    Ts = [ref.crandn(rng, (PB, K, PA, d)).astype(dt) for d, PA, K, PB, _, _ in jobs]      # column-major [d][PA][K][PB]
    Ms = [ref.crandn(rng, (len(x), K)).astype(dt) for _, _, K, _, x, _ in jobs]           # [K][string]
    rc, outs, intact, _, _ = leg_gemm(dtype, jobs, Ts, Ms)
    assert rc == 0 and intact
    worst = 0.0
    for (d, PA, K, PB, x, has_m), t, m, got in zip(jobs, Ts, Ms, outs):
        tl = t.astype(np.clongdouble)[:, :, :, x]                                          # (PB, K, PA, string)
        ml = m.astype(np.clongdouble) if has_m else np.ones(m.shape, dtype=np.clongdouble)
        want = np.einsum("bkap,pk->pba", tl, ml)
        mag = np.einsum("bkap,pk->pba", np.abs(tl), np.abs(ml))
        ratio = float(np.max(np.abs(got.astype(np.clongdouble) - want) / ref.dot_bound(dt, K, mag)))
        assert ratio <= 1.0, (d, PA, K, PB, len(x), has_m, ratio)
        worst = max(worst, ratio)
    _measured(f"amp_leg_gemm dtype {dtype}: largest error / bound", worst, 1.0)


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("K", [0, 65])
def test_leg_gemm_refuses_a_bond_dimension_it_does_not_take(dtype, K):
    dt = DT[dtype]
    rng = np.random.default_rng(42)
    T = ref.crandn(rng, (2, max(K, 1), 3, 2)).astype(dt); M = ref.crandn(rng, (3, max(K, 1))).astype(dt)      # d = 2, PA = 3, PB = 2, three strings
    R, _, sent = _guarded(dt, [18], GUARD)
    rc = lib.tnqs_dbg_amp_leg_gemm(dtype, 1, _p(_ints([2, 3, K, 2, 3])), _p(T), _p(_ints([0, 1, 1])), _p(M), _p(_ints([1])), _p(R), GUARD)
    assert rc == ERR_UNSUPPORTED and np.all(R == sent)


# ---- 2. the remaining legs ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1])
def test_absorb_mixed_items_in_one_launch(dtype):
    dt = DT[dtype]
    rng = np.random.default_rng([43, dtype])
    items = [(PA, K, PB, ns, int((i + j + q) % 4 != 1)) for i, K in enumerate(KS) for j, ns in enumerate([1, 5, 67]) for q, (PA, PB) in enumerate([(1, 6), (5, 4), (7, 1)])]
    ins = [ref.crandn(rng, (ns, PB, K, PA)).astype(dt) for PA, K, PB, ns, _ in items]
    ms = [ref.crandn(rng, (ns, K)).astype(dt) for _, K, _, ns, _ in items]
    sizes = [PA * PB * ns for PA, _, PB, ns, _ in items]
    out, offs, sent = _guarded(dt, sizes, GUARD)
    rc = lib.tnqs_dbg_amp_absorb(dtype, len(items), _p(_ints([it[:4] for it in items]).ravel()), _p(np.concatenate([a.ravel() for a in ins])),
                                 _p(np.concatenate([a.ravel() for a in ms])), _p(_ints([it[4] for it in items])), _p(out), GUARD)
    assert rc == 0 and _guards_intact(out, offs, sizes, GUARD, sent)
    worst = 0.0
    for (PA, K, PB, ns, has_m), a, m, off, s in zip(items, ins, ms, offs, sizes):
        got = out[off:off + s].reshape(ns, PB, PA)
        al = a.astype(np.clongdouble); ml = m.astype(np.clongdouble) if has_m else np.ones(m.shape, dtype=np.clongdouble)
        want = np.einsum("pbka,pk->pba", al, ml)
        mag = np.einsum("pbka,pk->pba", np.abs(al), np.abs(ml))
        ratio = float(np.max(np.abs(got.astype(np.clongdouble) - want) / ref.dot_bound(dt, K, mag)))
        assert ratio <= 1.0, (PA, K, PB, ns, has_m, ratio)
        worst = max(worst, ratio)
    _measured(f"amp_absorb dtype {dtype}: largest error / bound", worst, 1.0)
    R, _, sent = _guarded(dt, [4], GUARD)
    assert lib.tnqs_dbg_amp_absorb(dtype, 1, _p(_ints([2, 65, 2, 1])), _p(np.zeros(260, dtype=dt)), _p(np.zeros(65, dtype=dt)), _p(_ints([1])), _p(R), GUARD) == ERR_UNSUPPORTED
    assert np.all(R == sent)


# ---- 3. the epilogue ------------------------------------------------------------------------------------------------------------------------------------------------
def finalize(dtype, chis, nstrs, raws, olds, normalize, done, diff0=-3.0, sum0=-5.0):
    """one tnqs_dbg_amp_finalize call; raws[i], olds[i]: (nstr, chi) (olds[i] None: unset); returns [(new (nstr, chi), diff (nstr), sum (nstr) complex)], guards intact"""
    dt = DT[dtype]
    n = len(chis)
    R = np.concatenate([r.ravel() for r in raws]).astype(dt)
    O = np.concatenate([(np.zeros((ns, c)) if q is None else q).ravel() for q, c, ns in zip(olds, chis, nstrs)]).astype(dt)
    sizes = [c * ns for c, ns in zip(chis, nstrs)]
    new, offs, sent = _guarded(dt, sizes, GUARD)
    tot = int(np.sum(nstrs))
    diff = np.full(tot, diff0); ssum = np.full(2 * tot, sum0)
    dn = None if done is None else _ints(np.concatenate(done))
    rc = lib.tnqs_dbg_amp_finalize(dtype, n, _p(_ints(chis)), _p(_ints(nstrs)), _p(R), _p(O), _p(_ints([0 if q is None else 1 for q in olds])), _p(_ints(normalize)), _p(dn),
                                   _p(new), _p(diff), _p(ssum), GUARD)
    assert rc == 0
    res, at = [], 0
    for off, s, c, ns in zip(offs, sizes, chis, nstrs):
        res.append((new[off:off + s].reshape(ns, c).copy(), diff[at:at + ns].copy(), ssum[2 * at:2 * at + 2 * ns:2] + 1j * ssum[2 * at + 1:2 * at + 2 * ns:2]))
        at += ns
    return res, _guards_intact(new, offs, sizes, GUARD, sent), sent


FIN_CHIS = [1, 2, 3, 16, 17, 33, 64]


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("dtype", [0, 1])
def test_epilogue_every_shape_in_one_launch(dtype, normalize):
    dt = DT[dtype]
    eps = 2.0 ** -23 if dtype == 0 else 2.0 ** -52
    rng = np.random.default_rng([44, dtype])
    chis = [c for c in FIN_CHIS for _ in (0, 1)]
    nstrs = [ns for _ in FIN_CHIS for ns in (1, 7)]
    raws = [(1.0 + 0.3 * ref.crandn(rng, (ns, c))).astype(dt) for c, ns in zip(chis, nstrs)]       # a positive part: the element sum does not cancel
    olds = [None if i % 3 == 0 else ref.crandn(rng, (ns, c)).astype(dt) for i, (c, ns) in enumerate(zip(chis, nstrs))]
    res, intact, _ = finalize(dtype, chis, nstrs, raws, olds, [normalize] * len(chis), None)
    assert intact
    worst = worst_d = 0.0
    for c, ns, raw, old, (new, diff, ssum) in zip(chis, nstrs, raws, olds, res):
        r = raw.astype(np.complex128)
        for p in range(ns):
            m = r[p]; s = m.sum()
            B = 64 * EPS64 * np.abs(m).sum()                # the f64 sum of at most 64 numbers, any order
            assert abs(ssum[p] - s) <= B
            if normalize:
                assert abs(s) / np.abs(m).sum() >= 0.1
                tol = np.abs(m) * B / (abs(s) * (abs(s) - B)) + 4 * EPS64 * np.abs(m / s) + eps * np.abs(m / s)
                m = m / s
            else:
                tol = np.zeros(c)                        # the raw message goes through f64 and back: bit for bit
            err = np.abs(new[p] - m)
            assert np.all(err <= tol), (c, ns, p)
            if normalize:
                worst = max(worst, float(np.max(err / tol)))
            oldp = np.ones(c) if old is None else old[p].astype(np.complex128)
            dd = abs(diff[p] - o.message_diff(new[p].astype(np.complex128), oldp))
            assert dd < 1e-12, (c, ns, p, diff[p])
            worst_d = max(worst_d, dd)
    _measured(f"amp_finalize dtype {dtype} normalize {normalize} new_msg: largest error / bound", worst, 1.0)
    _measured(f"amp_finalize dtype {dtype} normalize {normalize} message_diff", worst_d, 1e-12)


@pytest.mark.parametrize("dtype", [0, 1])
def test_epilogue_zero_sum_done_flags_and_refusal(dtype):
    dt = DT[dtype]
    rng = np.random.default_rng([45, dtype])
    # an exactly zero element sum (small integers in (p, -p) pairs) is left undivided, bit for bit
    v = rng.integers(-8, 9, size=(3, 8)) + 1j * rng.integers(-8, 9, size=(3, 8))
    raw0 = np.zeros((3, 17), dtype=np.complex128); raw0[:, 0:16:2] = v; raw0[:, 1:16:2] = -v
    # done flags: strings 1 and 3 of five are finished -- their old message stays bit for bit, their diff and sum slots are not written
    raw1 = (1.0 + 0.3 * ref.crandn(rng, (5, 33))).astype(dt); old1 = ref.crandn(rng, (5, 33)).astype(dt)
    done = [np.zeros(3, dtype=np.int32), np.array([0, 1, 0, 1, 0], dtype=np.int32)]
    res, intact, _ = finalize(dtype, [17, 33], [3, 5], [raw0, raw1], [None, old1], [1, 1], done)
    assert intact
    new0, diff0, sum0 = res[0]
    assert np.all(sum0 == 0) and np.array_equal(new0.astype(np.complex128), raw0)
    for p in range(3):
        assert abs(diff0[p] - o.message_diff(raw0[p], np.ones(17))) < 1e-12
    new1, diff1, sum1 = res[1]
    for p in range(5):
        if done[1][p]:
            assert new1[p].tobytes() == old1[p].tobytes() and diff1[p] == -3.0 and sum1[p] == complex(-5.0, -5.0)
        else:
            assert abs(sum1[p] - raw1[p].astype(np.complex128).sum()) < 1e-12 * 33 and np.max(np.abs(new1[p] - raw1[p] / raw1[p].astype(np.complex128).sum())) < 1e-5
            assert abs(diff1[p] - o.message_diff(new1[p].astype(np.complex128), old1[p].astype(np.complex128))) < 1e-12
    new, _, sent = _guarded(dt, [65], GUARD)
    z = np.zeros(65, dtype=dt)
    assert lib.tnqs_dbg_amp_finalize(dtype, 1, _p(_ints([65])), _p(_ints([1])), _p(z), _p(z), _p(_ints([0])), _p(_ints([1])), None, _p(new), _p(np.zeros(1)), _p(np.zeros(2)),
                                     GUARD) == ERR_UNSUPPORTED
    assert np.all(new == sent)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------------------------------
def tn_graph(og):
    return tn.NamedGraph(list(og.vertices), list(og.edges))


def cache_of(og, tensors, dt):
    return tn.BeliefPropagationCache(tn.TensorNetworkState(tn_graph(og), {v: np.ascontiguousarray(tensors[v]).astype(dt) for v in og.vertices}))


def read_back(bpc, og):
    return {v: bpc.tensor(v).astype(np.complex128) for v in og.vertices}


def cdt(dt):
    return np.complex64 if np.dtype(dt) in (np.dtype(np.float32), np.dtype(np.complex64)) else np.complex128


def _compare(what, og, K, xs, nsweeps, dt, seq=None, factor=1.0, tensors=None):
    seq = o.forest_cover_edge_sequence(og) if seq is None else seq
    got = tn.log_amplitudes(K, xs, cache_update_kwargs=dict(maxiter=nsweeps, edge_sequence=seq))
    want = ref.log_amplitudes(og, read_back(K, og) if tensors is None else tensors, xs, nsweeps, seq=seq, store=cdt(dt))
    err = max(ref.log_close(a, b) for a, b in zip(got, want))
    bound = ref.log_bound(og, cdt(dt), factor)
    _measured(f"log a {what} {np.dtype(dt).name} after {nsweeps} sweeps, {len(xs)} strings", err, bound)
    assert err <= bound, (got, want)
    return got


@pytest.mark.parametrize("dt", [np.float32, np.float64, np.complex64, np.complex128])
@pytest.mark.parametrize("name", ["comb33", "path5"])
def test_trees_the_defaults_give_the_dense_amplitude(name, dt):
    og, ket, _ = inner_ref.tree_case(name)
    if np.dtype(dt).kind == "f":
        ket = {v: t.real for v, t in ket.items()}
    K = cache_of(og, ket, dt)
    xs = ref.random_strings(np.random.default_rng(3), og, 6)
    info = {}
    got = tn.log_amplitudes(K, xs, info=info)            # the defaults: one sweep of the tree order, no tolerance
    psi = ref.dense_state(og, read_back(K, og))
    bound = ref.log_bound(og, cdt(dt))
    err = max(ref.log_close(a, np.log(psi[tuple(x)] + 0j)) for a, x in zip(got, xs))
    _measured(f"log a tree {name} {np.dtype(dt).name} against the dense amplitude", err, bound)
    assert got.dtype == np.complex128 and list(info["niter"]) == [1] * 6 and not any(info["converged"]) and not any(info["flags"])
    assert err <= bound
    a = tn.amplitudes(K, xs)
    assert np.max(np.abs(a / psi[tuple(xs.T)] - 1)) <= 2 * bound
    # one dict, exactly what `sample` returns, gives a scalar
    one = tn.log_amplitudes(K, dict(zip(og.vertices, (int(t) for t in xs[1]))))
    assert isinstance(one, complex) and ref.log_close(one, got[1]) <= bound
    # agreement with inner(psi, |x>) on the device: within the sum of the two bounds
    basis = {v: np.eye(2)[xv].reshape((2,) + (1,) * len(og.nbrs[v])) for v, xv in zip(og.vertices, xs[2])}
    li = tn.log_inner(K, cache_of(og, basis, dt))
    assert ref.log_close(li, got[2]) <= 2 * bound


def test_all_strings_of_a_tree_in_one_call_sum_to_the_dense_norm():
    og, ket, _ = inner_ref.tree_case("comb33")
    K = cache_of(og, ket, np.complex128)
    nv = len(og.vertices)
    xs = np.array([[(n >> i) & 1 for i in range(nv)] for n in range(2 ** nv)], dtype=np.int32)
    a = tn.amplitudes(K, xs)
    psi = ref.dense_state(og, read_back(K, og))
    rel = abs(np.sum(np.abs(a) ** 2) / np.sum(np.abs(psi) ** 2) - 1)
    _measured("sum |a(x)|^2 over all 512 strings of comb33 against the dense norm", rel, 2 * ref.log_bound(og, np.complex128))
    assert rel <= 2 * ref.log_bound(og, np.complex128)
    assert np.max(np.abs(a / psi[tuple(xs.T)] - 1)) <= 2 * ref.log_bound(og, np.complex128)


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
@pytest.mark.parametrize("name", sorted(inner_ref.LOOPY_CASES))
def test_loopy_graphs_small_bond_dimensions(name, dt):
    og, t = ref.loopy_state(name)
    K = cache_of(og, t, dt)
    xs = ref.random_strings(np.random.default_rng(5), og, 6)      # the all-zeros string and five random ones
    for nsweeps in (3, 8):
        _compare(name, og, K, xs, nsweeps, dt)


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
@pytest.mark.parametrize("chi", [16, 32])
def test_loopy_grid_on_full_and_ragged_matrix_core_tiles(chi, dt):
    og, t = ref.grid33_state(chi)
    K = cache_of(og, t, dt)
    xs = ref.random_strings(np.random.default_rng(chi), og, 67)
    _compare(f"3 x 3 grid chi {chi}", og, K, xs, 3, dt)


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_mixed_bond_dimensions_including_one_and_five(dt):
    og, t = ref.grid33_state(ref.MIXED_DIMS)
    K = cache_of(og, t, dt)
    _compare("3 x 3 grid mixed bond dimensions", og, K, ref.random_strings(np.random.default_rng(7), og, 67), 3, dt)


def _raw_call(K, xs, opts, fn=None, budget=None):
    xs = _ints(xs); nb = len(xs)
    out = np.zeros(2 * nb); niter = np.zeros(nb, dtype=np.int32); diff = np.zeros(nb); flags = np.zeros(nb, dtype=np.int32); nbat = C.c_int(0)
    if budget is None:
        rc = lib.tnqs_amplitudes_bp(K._h, nb, _p(xs), C.byref(opts) if opts is not None else None, _p(out), _p(niter), _p(diff), _p(flags))
    else:
        rc = lib.tnqs_dbg_amplitudes_bp_ws(K._h, nb, _p(xs), C.byref(opts) if opts is not None else None, _p(out), _p(niter), _p(diff), _p(flags), C.c_int64(budget), C.byref(nbat))
    return rc, out[0::2] + 1j * out[1::2], niter, diff, flags, nbat.value


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_library_default_sequence_and_workspace_bound(dt):
    """the library's own default order (levels of several messages; most vertex scalars need the pass after the last sweep), replayed on the reference; the same call
    with a workspace bound of one byte runs every message and every string alone and agrees"""
    og, t = ref.loopy_state("grid3x4")
    K = cache_of(og, t, dt)
    xs = ref.random_strings(np.random.default_rng(5), og, 6)
    cap = 4 * len(og.edges)
    src, dst, n = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32), C.c_int(0)
    assert lib.tnqs_dbg_default_sequence(K._h, _p(src), _p(dst), cap, C.byref(n)) == 0
    seq = [(og.vertices[a], og.vertices[b]) for a, b in zip(src[:n.value], dst[:n.value])]
    want = ref.log_amplitudes(og, read_back(K, og), xs, 3, seq=seq, store=dt)
    bound = ref.log_bound(og, dt)
    got = tn.log_amplitudes(K, xs, cache_update_kwargs=dict(maxiter=3))
    err = max(ref.log_close(a, b) for a, b in zip(got, want))
    _measured(f"log a default sequence {np.dtype(dt).name}", err, bound)
    assert err <= bound
    opts = L.BpOpts(); opts.maxiter = 3; opts.tolerance = -1.0; opts.normalize = 1; opts.n_sequence = 0
    rc, one, niter, _, flags, nb1 = _raw_call(K, xs, opts, budget=1)
    assert rc == 0 and list(niter) == [3] * 6 and not any(flags)
    err = max(ref.log_close(a, b) for a, b in zip(one, want))
    _measured(f"log a default sequence, one message and one string per batch ({nb1} batches) {np.dtype(dt).name}", err, bound)
    assert err <= bound
    rc, _, _, _, _, nb0 = _raw_call(K, xs, opts, budget=1 << 30)
    assert rc == 0 and nb1 > nb0 > 0


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_batch_composition_does_not_change_a_string(dt):
    og, t = ref.grid33_state(5)
    K = cache_of(og, t, dt)
    xs = ref.random_strings(np.random.default_rng(9), og, 67)
    kw = dict(maxiter=4, edge_sequence=o.forest_cover_edge_sequence(og))
    batch = tn.log_amplitudes(K, xs, cache_update_kwargs=kw)
    bound = ref.log_bound(og, dt)
    for j in (0, 16, 66):
        alone = tn.log_amplitudes(K, xs[j], cache_update_kwargs=kw)
        same = tn.log_amplitudes(K, np.tile(xs[j], (67, 1)), cache_update_kwargs=kw)
        err = max(ref.log_close(alone, batch[j]), max(ref.log_close(s, batch[j]) for s in same))
        _measured(f"string {j} alone / in a batch of 67 / 67 times {np.dtype(dt).name}", err, bound)
        assert err <= bound


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_strings_freeze_on_their_own_under_a_tolerance(dt):
    """the freezing case of tests/test_amplitude_ref_cpu.py: per-string sweep counts equal the reference's, a string's result in the batch is its result alone"""
    og = o.named_grid((3, 3))
    rng = np.random.default_rng(17)
    t = ref.freezing_state(og, 3, rng)
    xs = ref.random_strings(rng, og, 5)
    xs[1] = 1
    K = cache_of(og, t, dt)
    tol = {np.complex64: 1e-6, np.complex128: 1e-9}[dt]
    seq = o.forest_cover_edge_sequence(og)
    kw = dict(maxiter=40, tolerance=tol, edge_sequence=seq)
    info, rinfo = {}, {}
    got = tn.log_amplitudes(K, xs, cache_update_kwargs=kw, info=info)
    want = ref.log_amplitudes(og, read_back(K, og), xs, 40, seq=seq, tolerance=tol, store=dt, info=rinfo)
    print(f"MEASURED freezing {np.dtype(dt).name}: niter {list(info['niter'])} (reference {rinfo['niter']}), diff {list(info['diff'])}")
    assert list(info["niter"]) == rinfo["niter"] and all(info["converged"]) and info["niter"][0] == 2 < info["niter"][1]
    bound = ref.log_bound(og, dt)
    assert max(ref.log_close(a, b) for a, b in zip(got, want)) <= bound
    for j in range(len(xs)):
        i1 = {}
        alone = tn.log_amplitudes(K, xs[j:j + 1], cache_update_kwargs=kw, info=i1)
        assert alone[0] == got[j] and i1["niter"][0] == info["niter"][j] and i1["diff"][0] == info["diff"][j]      # frozen: bit for bit what the string gives alone


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_evolved_state_with_pending_scales_and_deferred_gates(dt):
    """one TFIM layer with maxdim 3 on the biased chi = 1 product state: non-uniform bond dimensions, pending scale factors (normalising gates) and deferred one-site
    gates, not read back before the call; against the reference on the tensors of a round-tripped copy.  The handle's messages and <Z> are unchanged by the call."""
    og, t0, drawn = ref.evolved_case()
    g = tn_graph(og)
    K0 = cache_of(og, t0, dt)
    layer = ref.evolved_layer(tn.edge_color(g, 4), g.vertices)
    bpkw = dict(maxiter=20, tolerance=1e-6 if dt == np.complex64 else 1e-10)
    K1, _ = tn.apply_gates(layer, tn.update(K0, **bpkw), apply_kwargs=dict(maxdim=3, cutoff=1e-12, normalize_tensors=True), bp_update_kwargs=bpkw)
    f = C.c_double(1.0); pending = 0
    for i in range(len(og.vertices)):
        assert lib.tnqs_dbg_pending_scale(K1._h, i, C.byref(f)) == 0
        pending += f.value != 1.0
    assert pending > 0
    tensors = read_back(tn.BeliefPropagationCache(K1.copy().network()), og)
    seq = o.forest_cover_edge_sequence(og)
    xs = ref.strings_that_do_not_cancel(og, tensors, drawn, seq)
    assert 4 * len(xs) >= 3 * len(drawn)                 # (tests/test_amplitude_ref_cpu.py holds the same share on the oracle's evolution of this state)
    edges = [e for (a, b) in g.edges for e in ((a, b), (b, a))]
    before = [K1.message(e).tobytes() for e in edges]
    z_before = [tn.expect(K1, ("Z", [v])) for v in g.vertices]
    _compare("evolved state", og, K1, xs, ref.EVOLVED_SWEEPS, dt, seq=seq, tensors=tensors)
    assert before == [K1.message(e).tobytes() for e in edges]
    z_after = [tn.expect(K1, ("Z", [v])) for v in g.vertices]
    assert np.max(np.abs(np.array(z_before) - np.array(z_after))) <= (1e-5 if dt == np.complex64 else 1e-12)


def test_sampling_tie_log_q_is_log_p_on_a_tree():
    og, t, uniforms = ref.sampling_case()
    K = tn.update(cache_of(og, t, np.complex128), maxiter=1)
    bits, logq = tn.sample_with_probabilities(K, len(uniforms), gauge_state=False, uniforms=uniforms, bp_update_kwargs=dict(maxiter=1))
    logp = tn.log_probabilities(K, bits)
    bound = 2 * ref.log_bound(og, np.complex128) + len(og.vertices) * 3.6e-15 / ref.SAMPLING_PMIN
    err = float(np.max(np.abs(logp - logq)))
    _measured("sampling tie: log p against log q", err, bound)
    assert err <= bound


def test_errors_and_corners():
    og, t = ref.loopy_state("grid3x4")
    K = cache_of(og, t, np.complex64)
    nv = len(og.vertices)
    xs = ref.random_strings(np.random.default_rng(5), og, 3)
    bad = xs.copy(); bad[1, 4] = 2
    with pytest.raises(tn.TnqsArgumentError):
        tn.log_amplitudes(K, bad)
    with pytest.raises(tn.TnqsArgumentError):
        tn.log_amplitudes(K, xs[:, :-1])
    d = dict(zip(og.vertices, (int(v) for v in xs[0]))); del d[og.vertices[3]]
    with pytest.raises(tn.TnqsArgumentError):
        tn.log_amplitudes(K, [d])
    with pytest.raises(tn.TnqsError, match='"bp"'):
        tn.log_amplitudes(K, xs, alg="exact")
    with pytest.raises(tn.TnqsError, match='"bp"'):
        tn.amplitudes(K, xs, alg="boundarymps")
    out = np.zeros(6)
    assert lib.tnqs_amplitudes_bp(K._h, 3, _p(_ints(bad)), None, _p(out), None, None, None) == ERR_INVALID
    assert lib.tnqs_amplitudes_bp(K._h, 3, None, None, _p(out), None, None, None) == ERR_INVALID
    assert lib.tnqs_amplitudes_bp(K._h, 3, _p(_ints(xs)), None, None, None, None, None) == ERR_INVALID
    assert lib.tnqs_amplitudes_bp(None, 3, _p(_ints(xs)), None, _p(out), None, None, None) == ERR_INVALID
    opts = L.BpOpts(); opts.maxiter = 3; opts.tolerance = -1.0; opts.normalize = 1; opts.n_sequence = 2
    assert lib.tnqs_amplitudes_bp(K._h, 3, _p(_ints(xs)), C.byref(opts), _p(out), None, None, None) == ERR_INVALID
    assert not np.any(out)
    # nstrings = 0
    assert lib.tnqs_amplitudes_bp(K._h, 0, None, None, None, None, None, None) == 0
    empty = tn.log_amplitudes(K, np.zeros((0, nv), dtype=np.int32))
    assert empty.shape == (0,) and empty.dtype == np.complex128
    # NULL options: 25 sweeps, no tolerance; the optional outputs may be NULL
    rc, la, niter, diff, flags, _ = _raw_call(K, xs, None)
    assert rc == 0 and list(niter) == [25] * 3 and np.all(diff < 1e-9) and not any(flags)
    assert lib.tnqs_amplitudes_bp(K._h, 3, _p(_ints(xs)), None, _p(out), None, None, None) == 0
    assert np.array_equal(out[0::2] + 1j * out[1::2], la)
    # a TensorNetworkState is uploaded to a temporary handle
    la2 = tn.log_amplitudes(K.network(), xs, cache_update_kwargs=dict(maxiter=25))
    assert max(ref.log_close(a, b) for a, b in zip(la, la2)) <= ref.log_bound(og, np.complex64)


def test_a_bond_dimension_beyond_64_and_a_sharded_handle_are_refused():
    """a two-rank handle on one GPU as tests/test_gpu_bond_spectra.py sets it up: the exchange buffer comes from the HIP runtime the library itself is linked against,
    and the callback is never reached"""
    g = tn.named_grid((2, 2))
    out = np.zeros(2); cfg = np.zeros((1, 4), dtype=np.int32)
    big = tn.BeliefPropagationCache(tn.random_tensornetworkstate(np.complex64, g, bond_dimension=65, seed=3))
    assert lib.tnqs_amplitudes_bp(big._h, 1, _p(cfg), None, _p(out), None, None, None) == ERR_UNSUPPORTED and not out.any()
    bpc = tn.BeliefPropagationCache(tn.random_tensornetworkstate(np.complex64, g, bond_dimension=2, seed=61))
    buf = C.c_void_p()
    lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]; lib.hipFree.argtypes = [C.c_void_p]
    assert lib.hipMalloc(C.byref(buf), 1 << 16) == 0 and buf.value
    try:
        cb = L.ALLGATHER_FN(lambda ctx, base, nbytes, nranks: -1)
        owner, op = L.i32([0, 0, 1, 1])
        L.check(L.lib.tnqs_set_sharding(bpc._h, 0, 2, op, cb, None, buf, 1 << 16))
        assert lib.tnqs_amplitudes_bp(bpc._h, 1, _p(cfg), None, _p(out), None, None, None) == ERR_UNSUPPORTED and not out.any()
        bad = cfg.copy(); bad[0, 0] = 5
        assert lib.tnqs_amplitudes_bp(bpc._h, 1, _p(bad), None, _p(out), None, None, None) == ERR_INVALID      # the arguments are checked first
        del bpc
    finally:
        lib.hipFree(buf)


def test_an_exactly_zero_slice_gives_minus_infinity_for_its_strings_only():
    og, t = ref.loopy_state("hex2x2")
    v0 = og.vertices[2]
    t = dict(t); t[v0] = t[v0].copy(); t[v0][1] = 0
    K = cache_of(og, t, np.complex128)
    xs = ref.random_strings(np.random.default_rng(8), og, 6)
    xs[1, 2] = 1; xs[0, 2] = 0
    info = {}
    la = tn.log_amplitudes(K, xs, cache_update_kwargs=dict(maxiter=3, edge_sequence=o.forest_cover_edge_sequence(og)), info=info)
    tb = read_back(K, og)
    want = [None if x[2] == 1 else ref.log_amplitudes(og, tb, x, 3, seq=o.forest_cover_edge_sequence(og))[0] for x in xs]
    a = tn.amplitudes(K, xs, cache_update_kwargs=dict(maxiter=3, edge_sequence=o.forest_cover_edge_sequence(og)))
    for j, x in enumerate(xs):
        if x[2] == 1:
            assert la[j].real == -np.inf and la[j].imag == 0 and info["flags"][j] == 1 and a[j] == 0
        else:
            assert info["flags"][j] == 0 and ref.log_close(la[j], want[j]) <= ref.log_bound(og, np.complex128)
    assert sum(int(x[2]) for x in xs) >= 1 and sum(1 - int(x[2]) for x in xs) >= 1


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_an_edgeless_graph(dt):
    og = o.Graph([(1,), (2,), (3,)], [])
    rng = np.random.default_rng(4)
    t = {v: 1.0 + 0.5 * ref.crandn(rng, (2,)) for v in og.vertices}
    K = cache_of(og, t, dt)
    xs = np.array([[0, 0, 0], [1, 0, 1], [1, 1, 1]], dtype=np.int32)
    info = {}
    la = tn.log_amplitudes(K, xs, info=info)
    tb = read_back(K, og)
    for a, x in zip(la, xs):
        want = sum(np.log(tb[v][xv]) for v, xv in zip(og.vertices, x))
        assert ref.log_close(a, want) <= ref.log_bound(og, dt)
    assert list(info["niter"]) == [0, 0, 0]
