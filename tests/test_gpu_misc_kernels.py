"""GPU tests of the small kernels that otherwise run inside larger calls only, through the entry points of csrc/debug_misc.cpp: permute_kernel, identity_kernel,
random_fill_kernel, sum_doubles_kernel, record_pack_kernel + header_gather_kernel (kernels_util.hip), copy_items_kernel (kernels_chi64.hip), loop_dot_kernel and its tail
(kernels_loop.hip), bmps_norm_kernel (kernels_bmps.hip), amp_sweep_end_kernel and amp_scalar_kernel (kernels_amp.hip).

Data movement is compared bit for bit; every output lies between guard bands of a sentinel that must come back untouched.  Reductions are held to the derived bounds
of tests/misc_kernels_ref.py (depth 2^-53 sum|terms|), none of them measured on the kernels; the one measured constant is C_LIBM, the device libm's error, whose
measurement test_libm_constant repeats and prints.  Every test prints MEASURED error / bound."""
import ctypes as C

import numpy as np
import pytest

import tnqs_amd as tn
import misc_kernels_ref as ref

pytestmark = pytest.mark.gpu
lib = C.CDLL(tn.LIB_PATH)
L = tn.core.L
ERR_INVALID, ERR_UNSUPPORTED = -1, -2                    # include/tnqs.h
DT = {0: np.complex64, 1: np.complex128}
GUARD = 7
SENTINEL = 777.0 - 555.0j
U53 = ref.U53
LD = np.longdouble
lib.tnqs_dbg_random_fill.argtypes = [C.c_int, C.c_int64, C.c_uint64, C.c_double, C.c_int, C.c_void_p, C.c_int]
lib.tnqs_dbg_permute.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int]
lib.tnqs_dbg_amp_sweep_end.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _i32(v):
    return np.ascontiguousarray(v, dtype=np.int32)


def _i64(v):
    return np.ascontiguousarray(v, dtype=np.int64)


def _ok(rc):
    assert rc == 0, L.lib.tnqs_last_error()


class Banded:
    """guard, item 0, guard, item 1, ..., guard in one array of `dtype`, everything filled with `fill`"""

    def __init__(self, lens, dtype, guard=GUARD, fill=SENTINEL):
        self.lens, self.guard, self.fill = list(lens), guard, np.asarray(fill).astype(dtype)
        self.arr = np.full(guard + sum(n + guard for n in self.lens), self.fill, dtype=dtype)
        self.start = []
        off = guard
        for n in self.lens:
            self.start.append(off)
            off += n + guard

    def item(self, i):
        return self.arr[self.start[i]:self.start[i] + self.lens[i]]

    def guards_intact(self):
        mask = np.ones(self.arr.size, dtype=bool)
        for s, n in zip(self.start, self.lens):
            mask[s:s + n] = False
        g = self.arr[mask]
        return bool(np.all(g.view(np.uint8) == np.full(g.size, self.fill, dtype=self.arr.dtype).view(np.uint8)))


# ---- permute_kernel<T> -----------------------------------------------------------------------------------------------------------------------------------------------
def _permute(dtype, dims, strides, x):
    n = int(np.prod(dims, dtype=np.int64))
    out = Banded([n], DT[dtype])
    _ok(lib.tnqs_dbg_permute(dtype, len(dims), _p(_i32(dims)), _p(_i64(strides)), x.size, _p(x), _p(out.arr), GUARD))
    assert out.guards_intact()
    return out.item(0)


@pytest.mark.parametrize("dtype", [0, 1])
def test_permute_every_rank_and_order(dtype):
    """ranks 1 to 8 with prime dimensions, five leg orders each, dimension-1 legs between others: out equals the numpy transpose bit for bit"""
    count = 0
    shapes = [(r, s) for r, s in ref.PERM_SHAPES.items()] + [(len(s), s) for s in ref.PERM_ONES]
    for rank, shape in shapes:
        x = ref.ramp(int(np.prod(shape)), DT[dtype])
        for perm in ref.perms_of(rank):
            dims, st = ref.permute_args(shape, perm)
            got = _permute(dtype, dims, st, x)
            want = np.transpose(x.reshape(shape, order="F"), perm).ravel(order="F")
            assert np.array_equal(got, want), (shape, perm)
            assert np.array_equal(got, ref.permute_ref(x, dims, st))
            count += 1
    print(f"MEASURED permute dtype={dtype}: {count} permutations bit-exact")


@pytest.mark.parametrize("dtype", [0, 1])
def test_permute_grid_stride_loop(dtype):
    """2,042,040 elements: more than 4096 x 256, every workgroup loops"""
    shape = ref.PERM_LARGE
    x = ref.ramp(int(np.prod(shape)), DT[dtype])
    perm = [3, 7, 0, 5, 1, 6, 2, 4]
    assert x.size == 2042040 > 4096 * 256
    dims, st = ref.permute_args(shape, perm)
    got = _permute(dtype, dims, st, x)
    assert np.array_equal(got, np.transpose(x.reshape(shape, order="F"), perm).ravel(order="F"))
    print(f"MEASURED permute large dtype={dtype}: {got.size} elements bit-exact")


@pytest.mark.parametrize("dtype", [0, 1])
def test_permute_as_the_configuration_engine_fills_it(dtype):
    """the 2-D transpose of a closed chain (nn x nf out of nf x nn) and the 4-index shuffle M[a, b, a', b'] = Lt[a', a, b', b] of engine_configs.cpp"""
    cn, cf = 3, 5
    nn, nf = cn * cn, cf * cf
    x = ref.ramp(nn * nf, DT[dtype])
    got = _permute(dtype, [nn, nf], [nf, 1], x)
    assert np.array_equal(got, x.reshape((nf, nn), order="F").T.ravel(order="F"))
    ca, cb = 3, 5
    x = ref.ramp(ca * ca * cb * cb, DT[dtype])
    got = _permute(dtype, [ca, cb, ca, cb], [ca, ca * ca * cb, 1, ca * ca], x)
    want = np.transpose(x.reshape((ca, ca, cb, cb), order="F"), (1, 3, 0, 2)).ravel(order="F")
    assert np.array_equal(got, want)
    print(f"MEASURED permute engine forms dtype={dtype}: bit-exact")


def test_permute_refuses_a_source_index_outside_the_input():
    x = ref.ramp(30, np.complex64)
    out = Banded([30], np.complex64)
    before = out.arr.copy()
    for dims, st, n_in in (([2, 3, 5], [1, 2, 7], 30), ([2, 3, 5], [1, 2, 6], 29), ([2, 3], [1, -1], 30), ([2] * 9, [1] * 9, 30), ([0, 3], [1, 2], 30)):
        rc = lib.tnqs_dbg_permute(0, len(dims), _p(_i32(dims)), _p(_i64(st)), n_in, _p(x), _p(out.arr), GUARD)
        assert rc == ERR_INVALID, (dims, st)
        assert np.array_equal(out.arr, before)


# ---- identity_kernel<T> -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 17, 256])
def test_identity(dtype, n):
    out = Banded([n * n], DT[dtype])
    _ok(lib.tnqs_dbg_identity(dtype, n, _p(out.arr), GUARD))
    assert out.guards_intact()
    assert np.array_equal(out.item(0).reshape(n, n), np.eye(n, dtype=DT[dtype]))
    assert not np.signbit(out.item(0).real).any() and not np.signbit(out.item(0).imag).any()


# ---- copy_items_kernel ------------------------------------------------------------------------------------------------------------------------------------------------
COPY_N16 = [0, 1, 255, 256, 4096, 4097, 16 * 256 * 3 + 5, 10147, 1]      # (10147 words + one 8-byte element = a 165 x 123 ComplexF32 matrix)
COPY_TAIL = [0, 0, 1, 0, 0, 1, 0, 1, 1]


@pytest.mark.parametrize("with_tail", [False, True])
def test_copy_items_mixed_lengths_in_one_launch(with_tail):
    """whole 16-byte words and, for an odd number of 8-byte elements, the last element on its own; the guard right behind every item proves that nothing past it is
    written (the engine's theta slot is followed by other gates' data)"""
    rng = np.random.default_rng(4)
    tail = COPY_TAIL if with_tail else [0] * len(COPY_N16)
    nbytes = [16 * n + 8 * t for n, t in zip(COPY_N16, tail)]
    src = rng.integers(0, 255, sum(nbytes), dtype=np.uint8)               # (255 never occurs: a byte of the device's gap filling cannot pass for data)
    dst = Banded(nbytes, np.uint8, guard=64, fill=0xA5)
    _ok(lib.tnqs_dbg_copy_items(len(nbytes), _p(_i64(COPY_N16)), _p(_i32(tail)) if with_tail else None, _p(src), _p(dst.arr), 64))
    assert dst.guards_intact()
    off = 0
    for i, nb in enumerate(nbytes):
        assert np.array_equal(dst.item(i), src[off:off + nb]), i
        off += nb
    print(f"MEASURED copy_items tail={with_tail}: {len(nbytes)} items, {sum(nbytes)} bytes bit-exact")


# ---- record_pack_kernel + header_gather_kernel --------------------------------------------------------------------------------------------------------------------------
def test_record_pack_and_header_gather():
    rng = np.random.default_rng(8)
    cap_max = 256
    x2_off = 32 + cap_max * 8                                              # as the engine forms it
    cases = [(1, 0), (33, 1), (256, 5000), (33, 0), (1, 5000), (256, 1)]   # (nS, x2_words)
    info = rng.integers(1, 1000, (len(cases), 4)).astype(np.int32)
    terr = rng.random(len(cases))
    S = [rng.random(ns) for ns, _ in cases]
    X2 = [rng.integers(0, 2 ** 63, nw, dtype=np.uint64) for _, nw in cases]
    nbytes = [x2_off + 8 * nw + 24 for _, nw in cases]                      # 24 spare bytes behind the payload: they stay as they were
    dst = Banded(nbytes, np.uint8, guard=64, fill=0xA5)
    headers = np.full(4 * len(cases), np.nan)
    _ok(lib.tnqs_dbg_record_pack(len(cases), _p(info), _p(terr), _p(np.concatenate(S)), _p(_i32([c[0] for c in cases])), _p(np.concatenate(X2)),
                                 _p(_i64([c[1] for c in cases])), _p(_i64([x2_off] * len(cases))), _p(_i64(nbytes)), _p(dst.arr), _p(headers), 64))
    assert dst.guards_intact()
    for i in range(len(cases)):
        want = ref.record_ref(info[i], terr[i], S[i], X2[i], x2_off, nbytes[i], 0xA5)
        assert np.array_equal(dst.item(i), want), i
        assert headers[4 * i:4 * i + 4].tolist() == [float(info[i, 2]), float(info[i, 3]), terr[i], 0.0]
    bad = _i64([x2_off] * len(cases)); bad[2] = 32 + 8 * 255               # S would run into X2
    assert lib.tnqs_dbg_record_pack(len(cases), _p(info), _p(terr), _p(np.concatenate(S)), _p(_i32([c[0] for c in cases])), _p(np.concatenate(X2)),
                                    _p(_i64([c[1] for c in cases])), _p(bad), _p(_i64(nbytes)), _p(dst.arr), _p(headers), 64) == ERR_INVALID
    print(f"MEASURED record_pack: {len(cases)} records bit-exact")


# ---- amp_sweep_end_kernel -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nstr", [1, 255, 256, 257])
@pytest.mark.parametrize("nseq", [1, 13])
def test_amp_sweep_end(nstr, nseq):
    """the kernel adds in the order t = 0 .. nseq - 1 and divides once: a sequential f64 loop reproduces fdiff bit for bit, so the decision avg <= tol is exact"""
    rng = np.random.default_rng([nstr, nseq])
    diffs = rng.random((nseq, nstr)) * np.exp(4 * rng.standard_normal((nseq, nstr)))
    diffs[:, 0] = 0.25                                                     # the average is exactly 0.25: sits on the tolerance below
    for tol in (0.25, -1.0, float(np.median(diffs.mean(axis=0)))):
        done0 = (rng.random(nstr) < 0.3).astype(np.int32)
        done0[0] = 0
        niter0 = rng.integers(1, 5, nstr).astype(np.int32)
        fdiff0 = rng.random(nstr)
        done, niter, fdiff = done0.copy(), niter0.copy(), fdiff0.copy()
        _ok(lib.tnqs_dbg_amp_sweep_end(nseq, nstr, 7, tol, _p(diffs), _p(done), _p(niter), _p(fdiff)))
        wd, wn, wf = ref.sweep_end_ref(diffs, 7, tol, done0, niter0, fdiff0)
        assert np.array_equal(done, wd) and np.array_equal(niter, wn) and np.array_equal(fdiff.view(np.uint64), wf.view(np.uint64))
        was = done0 == 1
        assert np.array_equal(niter[was], niter0[was]) and np.array_equal(fdiff[was], fdiff0[was]) and np.all(done[was] == 1)      # a finished string: nothing changes
        if tol < 0:
            assert np.array_equal(done, done0)                            # nobody finishes
        if tol == 0.25:
            assert done[0] == 1 and fdiff[0] == 0.25                      # an average exactly equal to the tolerance finishes


# ---- sum_doubles_kernel -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 5000])
def test_sum_doubles(n):
    x = ref.sum_inputs(n)
    out = np.full(1, np.nan)
    _ok(lib.tnqs_dbg_sum_doubles(n, _p(x) if n else None, _p(out)))
    want = ref.sum_ref(x)
    bound = ref.sum_depth(n) * U53 * float(np.sum(np.abs(x)))
    err = abs(float(LD(out[0]) - LD(want)))
    print(f"MEASURED sum_doubles n={n}: error {err:.3e}, bound {bound:.3e}, ratio {err / bound if bound else 0.0:.3f}")
    assert err <= bound
    if n <= 1:
        assert out[0] == (x[0] if n else 0.0)


# ---- loop_dot_kernel<T> + tail ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1])
def test_loop_dot_mixed_lengths_in_one_launch(dtype):
    """one launch over lengths on both sides of a workgroup's 4096 elements, a length at which the 1024-workgroup cap binds and every workgroup loops, and a zero vector"""
    lens = ref.DOT_LENGTHS + [3000]
    xs, ys = zip(*[ref.dot_inputs(n, DT[dtype]) for n in lens])
    xs = list(xs)
    xs[-1] = np.zeros(3000, dtype=DT[dtype])                               # a zero vector
    out = np.full(2 * len(lens), np.nan)
    nwg = np.zeros(len(lens), dtype=np.int32)
    _ok(lib.tnqs_dbg_loop_dot(dtype, len(lens), _p(_i64(lens)), _p(np.concatenate(xs)), _p(np.concatenate(ys)), _p(out), _p(nwg)))
    assert nwg.tolist() == [ref.loop_dot_nwg(n) for n in lens] and nwg[5] == 1024
    worst = 0.0
    for i, n in enumerate(lens):
        re, im, mre, mim = ref.dot_ref(xs[i], ys[i])
        d = ref.loop_dot_depth(n)
        for got, want, mag in ((out[2 * i], re, mre), (out[2 * i + 1], im, mim)):
            err, bound = abs(float(LD(got) - want)), d * U53 * mag
            assert err <= bound, (n, err, bound)
            worst = max(worst, err / bound if bound else 0.0)
    assert out[-2] == 0 and out[-1] == 0
    print(f"MEASURED loop_dot dtype={dtype}: worst error / bound = {worst:.3f} over lengths {lens}")
    assert worst <= 0.5


@pytest.mark.parametrize("dtype", [0, 1])
def test_loop_dot_is_bilinear(dtype):
    """no conjugate: X = Y = i ones gives -n exactly"""
    lens = [1, 300, 5000]
    x = np.concatenate([np.full(n, 1j, dtype=DT[dtype]) for n in lens])
    out = np.full(2 * len(lens), np.nan)
    _ok(lib.tnqs_dbg_loop_dot(dtype, len(lens), _p(_i64(lens)), _p(x), _p(x.copy()), _p(out), None))
    assert out.tolist() == [v for n in lens for v in (-float(n), 0.0)]


# ---- bmps_norm_kernel<T> ------------------------------------------------------------------------------------------------------------------------------------------------
def _norm_items(dtype):
    """(n, src, normalize, conj, has_dst, has_norm) per item: every length with all four (normalize, conj) pairs, then the null-pointer forms, a zero vector, and for
    ComplexF32 entries scaled by 1e-18 and 1e18"""
    items = []
    for n in ref.NORM_LENGTHS:
        v = ref.norm_inputs(n, DT[dtype])
        items += [(n, v, nz, cj, 1, 1) for nz in (0, 1) for cj in (0, 1)]
    v = ref.norm_inputs(1025, DT[dtype], seed=1)
    items += [(1025, v, 1, 1, 1, 1), (1025, v, 1, 1, 0, 1), (1025, v, 1, 1, 1, 0), (1025, v, 1, 1, 0, 0)]
    items.append((1025, np.zeros(1025, dtype=DT[dtype]), 1, 1, 1, 1))
    if dtype == 0:
        for sc in (1e-18, 1e18):
            v = ref.norm_inputs(1023, DT[dtype], scale=sc, seed=2)
            items += [(1023, v, 1, 0, 1, 1), (1023, v, 0, 1, 1, 1)]
    return items


def _run_norm(dtype, items):
    dst = Banded([it[0] for it in items], DT[dtype])
    norms = np.full(len(items), -7.0)
    _ok(lib.tnqs_dbg_bmps_norm(dtype, len(items), _p(_i64([it[0] for it in items])), _p(np.concatenate([it[1] for it in items])), _p(_i32([it[2] for it in items])),
                               _p(_i32([it[3] for it in items])), _p(_i32([it[4] for it in items])), _p(_i32([it[5] for it in items])), _p(dst.arr), _p(norms), GUARD))
    assert dst.guards_intact()
    return dst, norms


def _check_norm(dtype, items, dst, norms):
    uT = ref.u_of(DT[dtype])
    worst_n, worst_d = 0.0, 0.0
    dev_norm = {}
    for i, (n, v, nz, cj, hd, hn) in enumerate(items):
        if hn:
            dev_norm[v.tobytes()] = norms[i]
    for i, (n, v, nz, cj, hd, hn) in enumerate(items):
        want = ref.norm_ref(v)
        if hn:
            # s = sum of squares within depth u s; sqrt halves the relative error and adds C_LIBM u of its own
            bound = (0.5 * ref.norm_depth(n) + ref.C_LIBM) * U53 * float(want)
            err = abs(float(LD(norms[i]) - want))
            assert err <= bound, (i, n, err, bound)
            worst_n = max(worst_n, err / bound if bound else 0.0)
        else:
            assert norms[i] == -7.0
        got = dst.item(i)
        if not hd:
            assert np.all(got == DT[dtype](SENTINEL))                      # a null dst: the item's place is untouched
            continue
        nrm = dev_norm[v.tobytes()]                                        # the same input gives the same sum: the factor the kernel formed
        f = (1.0 / nrm) if (nz and nrm != 0) else 1.0
        vr, vi = v.real.astype(LD) * LD(f), (-v.imag if cj else v.imag).astype(LD) * LD(f)
        for g, w in ((got.real, vr), (got.imag, vi)):
            bound = (uT + 4 * U53) * np.abs(w).astype(np.float64)
            err = np.abs((g.astype(LD) - w).astype(np.float64))
            assert np.all(err <= bound), (i, n)
            worst_d = max(worst_d, float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny))))
    return worst_n, worst_d


@pytest.mark.parametrize("dtype", [0, 1])
def test_bmps_norm_one_launch(dtype):
    items = _norm_items(dtype)
    dst, norms = _run_norm(dtype, items)
    wn, wd = _check_norm(dtype, items, dst, norms)
    # conj flips the sign of the imaginary part bit for bit and nothing else
    for k in range(len(ref.NORM_LENGTHS)):
        for nz in (0, 1):
            a, b = dst.item(4 * k + 2 * nz), dst.item(4 * k + 2 * nz + 1)
            assert np.array_equal(a.real, b.real) and np.array_equal(a.imag, -b.imag)
    zero = [i for i, it in enumerate(items) if not it[1].any()][0]
    assert norms[zero] == 0 and not dst.item(zero).any()                   # a zero vector: factor 1, output zero
    print(f"MEASURED bmps_norm dtype={dtype}: norm error / bound = {wn:.3f}, element error / bound = {wd:.3f} over {len(items)} items")
    assert wn <= 0.5


@pytest.mark.parametrize("dtype", [0, 1])
def test_bmps_norm_one_item_per_launch(dtype):
    """as the engine launches it: one item at a time; the results are those of the batched launch bit for bit"""
    items = [it for it in _norm_items(dtype) if it[0] in (1, 1025, 70000) and it[2] == 1 and it[3] == 1][:4]
    dst_all, norms_all = _run_norm(dtype, items)
    for i, it in enumerate(items):
        dst, norms = _run_norm(dtype, [it])
        _check_norm(dtype, [it], dst, norms)
        if it[5]:
            assert norms[0] == norms_all[i]
        if it[4]:
            assert np.array_equal(dst.item(0), dst_all.item(i))


# ---- random_fill_kernel<T> ----------------------------------------------------------------------------------------------------------------------------------------------
def _fill(dtype, n, seed, scale, real_only=0):
    out = Banded([n], DT[dtype])
    _ok(lib.tnqs_dbg_random_fill(dtype, n, seed, scale, real_only, _p(out.arr), GUARD))
    assert out.guards_intact()
    return out.item(0)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _fill_error(got, index, seed, scale, dtype):
    """worst of (|got - ref| - u_T |ref|) / (2^-53 scale max(1, rad)) over both parts: the libm error of the element in units of 2^-53"""
    re, im, rad = ref.random_fill_ref(index, seed, scale)
    uT = ref.u_of(DT[dtype])
    unit = U53 * scale * np.maximum(1.0, rad.astype(np.float64))
    worst = 0.0
    for g, w in ((got.real, re), (got.imag, im)):
        err = np.abs((g.astype(LD) - w).astype(np.float64)) - uT * np.abs(w.astype(np.float64))
        worst = max(worst, float(np.max(err / unit)))
    return worst


@pytest.mark.parametrize("dtype", [0, 1])
def test_random_fill_values_prefix_and_real_only(dtype):
    seed, scale = 12345, 0.75
    a, b = _fill(dtype, 1000, seed, scale), _fill(dtype, 100000, seed, scale)
    assert _same_bits(a, b[:1000])        # element e does not depend on the launch shape
    worst = _fill_error(b, np.arange(100000), seed, scale, dtype)
    print(f"MEASURED random_fill dtype={dtype}: worst libm error {worst:.3f} x 2^-53 scale max(1, rad), C_LIBM = {ref.C_LIBM}")
    assert worst <= ref.C_LIBM
    r = _fill(dtype, 1000, seed, scale, real_only=1)
    assert not r.imag.any() and not np.signbit(r.imag).any() and _same_bits(r.real, a.real)
    other = _fill(dtype, 1000, seed + 1, scale)
    assert np.all(other.real != a.real) and np.all(other.imag != a.imag)    # another seed: every element differs
    assert _fill(dtype, 0, seed, scale).size == 0


def test_random_fill_past_the_launch_cap():
    """65536 x 256 + 1000 ComplexF32 elements: the grid-stride loop runs; the first 100,000 are the small fill's bit for bit and the last 1000 match the restatement"""
    seed, scale, n = 12345, 0.75, 65536 * 256 + 1000
    big = _fill(0, n, seed, scale)
    small = _fill(0, 100000, seed, scale)
    assert _same_bits(big[:100000], small)
    worst = _fill_error(big[-1000:], np.arange(n - 1000, n), seed, scale, 0)
    print(f"MEASURED random_fill large: worst libm error of the last 1000 elements {worst:.3f} x 2^-53")
    assert worst <= ref.C_LIBM


@pytest.mark.parametrize("dtype", [0, 1])
def test_random_fill_statistics(dtype):
    scale = 0.5
    v = _fill(dtype, ref.FILL_STATS_N, ref.FILL_STATS_SEED, scale)
    st = ref.fill_stats(v.real, v.imag, scale)
    print(f"MEASURED random_fill statistics dtype={dtype} (each <= 5): " + ", ".join(f"{s:.3f}" for s in st))
    assert max(st) <= 5.0


# ---- amp_scalar_kernel<T> -----------------------------------------------------------------------------------------------------------------------------------------------
def _scalar(dtype, items, nv, ne, cfg, guard=GUARD):
    dt = DT[dtype]
    nstr, ld = cfg.shape
    ones = lambda chi: np.ones((chi, nstr), dtype=dt)      # noqa: E731  (what stands in an absent array's place; the kernel gets a null pointer)
    # [chi][nstrings] with the entry index fastest: element (j, n) at j + chi n
    m = np.concatenate([(ones(it.chi) if it.m is None else np.asarray(it.m, dtype=dt)).ravel(order="F") for it in items])
    mr = np.concatenate([(ones(it.chi) if it.mr is None else np.asarray(it.mr, dtype=dt)).ravel(order="F") for it in items])
    present = _i32([[it.m is not None, it.mr is not None] for it in items])
    raw = np.concatenate([np.zeros(nstr, dtype=np.complex128) if it.rawsum is None else np.asarray(it.rawsum, dtype=np.complex128) for it in items])
    scale = np.asarray([1.0 if it.scale is None else it.scale for it in items], dtype=np.float64)
    sites = [np.zeros(0, dtype=dt) if it.site is None else np.asarray(it.site, dtype=dt) for it in items]
    site = np.concatenate(sites) if sum(s.size for s in sites) else np.zeros(1, dtype=dt)
    out = Banded([2 * nstr], np.float64, guard=guard, fill=-4321.0)
    flags = Banded([nstr], np.int32, guard=guard, fill=-77)
    rc = lib.tnqs_dbg_amp_scalar(dtype, nv, ne, _p(_i32([it.chi for it in items])), _p(m), _p(mr), _p(present), _p(raw), _p(_i32([it.rawsum is not None for it in items])),
                                 _p(_i32([it.normalize for it in items])), _p(scale), _p(_i32([it.scale is not None for it in items])), _p(site), _p(_i32([s.size for s in sites])),
                                 _p(_i32([it.site is not None for it in items])), _p(np.ascontiguousarray(cfg)), ld, nstr, _p(out.arr), _p(flags.arr), guard)
    return rc, out, flags


def _wrap(d):
    return d - 2 * np.pi * np.round(d / (2 * np.pi))


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("nstr", ref.SCALAR_STRINGS)
def test_amp_scalar(dtype, nstr):
    items, nv, ne, cfg = ref.scalar_case(nstr, DT[dtype])
    rc, out, flags = _scalar(dtype, items, nv, ne, cfg)
    _ok(rc)
    assert out.guards_intact() and flags.guards_intact()
    re, im, wflags, phase_mag = ref.scalar_ref(items, nv, cfg)
    got = out.item(0).reshape(nstr, 2)
    assert flags.item(0).tolist() == wflags.tolist()
    bound = ref.scalar_bound(items, cfg)
    worst_re, worst_im = 0.0, 0.0
    for n in range(nstr):
        if wflags[n] & 2:
            assert np.isnan(got[n, 0]) and np.isnan(got[n, 1])
        elif wflags[n] & 1:
            assert got[n, 0] == -np.inf and got[n, 1] == 0 and not np.signbit(got[n, 1])
        else:
            assert -np.pi < got[n, 1] <= np.pi
            e_re = abs(float(LD(got[n, 0]) - re[n]))
            # every phase is off by at most its item's relative error; the running sum of the phases rounds once per item, and the wrap once more
            b_im = bound[n] + (len(items) + 2) * U53 * phase_mag[n]
            e_im = abs(float(_wrap(LD(got[n, 1]) - im[n])))
            assert e_re <= bound[n], (n, e_re, bound[n])
            assert e_im <= b_im, (n, e_im, b_im)
            worst_re, worst_im = max(worst_re, e_re / bound[n]), max(worst_im, e_im / b_im)
    print(f"MEASURED amp_scalar dtype={dtype} nstr={nstr}: real part error / bound = {worst_re:.3f}, phase error / bound = {worst_im:.3f}, flags = {wflags.tolist()}")
    assert worst_re <= 0.5 and worst_im <= 0.5


@pytest.mark.parametrize("dtype", [0, 1])
def test_amp_scalar_on_the_branch_cut(dtype):
    """one exactly negative real item: as a vertex item its phase is pi, as an edge item -pi, which wraps to pi -- the interval is (-pi, pi], closed at the top"""
    nstr = 5
    neg = lambda: ref.ScalarItem(1, np.full((1, nstr), -2.0, dtype=DT[dtype]), np.full((1, nstr), 1.5, dtype=DT[dtype]))      # noqa: E731
    cfg = np.full((nstr, 2), -1, dtype=np.int32)
    for nv, ne in ((1, 0), (0, 1)):
        rc, out, flags = _scalar(dtype, [neg()], nv, ne, cfg)
        _ok(rc)
        got = out.item(0).reshape(nstr, 2)
        assert not flags.item(0).any() and np.all(got[:, 1] == np.pi), (nv, ne, got[:, 1])
        want_re = np.log(3.0) if nv else -np.log(3.0)
        assert np.all(np.abs(got[:, 0] - want_re) <= (1 + ref.C_LIBM) * U53)


def test_amp_scalar_refuses_chi_outside_1_64():
    items, nv, ne, cfg = ref.one_term_case(4, np.complex64)
    for chi in (0, 65):
        items[0].chi = chi
        items[0].m = np.ones((max(chi, 1), 4), dtype=np.complex64)
        rc, out, flags = _scalar(0, items, nv, ne, cfg)
        assert rc == ERR_UNSUPPORTED
        assert np.all(out.arr == -4321.0) and np.all(flags.arr == -77)


@pytest.mark.parametrize("dtype", [0, 1])
def test_libm_constant(dtype):
    """the measurement behind C_LIBM (tests/misc_kernels_ref.py): one-term items, where the sum adds nothing, against the extended-precision restatement, in units of
    2^-53; C_LIBM is at least four times the worst value seen"""
    nstr = 4096
    items, nv, ne, cfg = ref.one_term_case(nstr, DT[dtype])
    rc, out, flags = _scalar(dtype, items, nv, ne, cfg)
    _ok(rc)
    re, im, wflags, _ = ref.scalar_ref(items, nv, cfg)
    got = out.item(0).reshape(nstr, 2)
    assert not flags.item(0).any()
    e_re = float(np.max(np.abs((got[:, 0].astype(LD) - re).astype(np.float64)))) / U53
    e_im = float(np.max(np.abs(_wrap((got[:, 1].astype(LD) - im).astype(np.float64))))) / U53
    print(f"MEASURED libm one-term dtype={dtype}: log|z| error {e_re:.3f} x 2^-53, phase error {e_im:.3f} x 2^-53, C_LIBM = {ref.C_LIBM}")
    assert 4 * max(e_re, e_im / np.pi) <= ref.C_LIBM      # (a phase of up to pi carries pi times the unit)
