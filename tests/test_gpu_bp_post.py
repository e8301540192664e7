"""Kernel-level GPU tests of the kernels that post-process a BP cache and prepare a gate's environments -- msg_rescale_kernel, edge_scalar_kernel, symg_build_kernel,
symg_finish_kernel (kernels_bp.hip), env_prepare_kernel, env_finish_kernel (kernels_chol.hip), diag_kernel, cscale_kernel (kernels_util.hip), both dtypes -- through
the tnqs_dbg_* entry points of include/tnqs_debug.h, against the high-precision reference of tests/bp_post_ref.py (pinned to the oracle in
tests/test_bp_post_ref_cpu.py).  Sizes 1 .. 128 cover no trip, exactly one trip (n = 16) and several trips with a ragged tail of the kernels' 256-stride element
loop, and the benchmark's 32 and 64; n = 256 is the limit the engine accepts.  Every output array carries guard bands that are checked after every call.

Bounds are derived, none is measured on the kernels: every kernel accumulates in f64 and rounds once to T, so per output element (real and imaginary part each)
    |out - ref| <= 8 (k + 4) 2^-53 (sum of |terms|) + [T = float] 2^-23 |ref|              (bp_post_ref.bound)
with k = n (roots, env_finish, symg_finish), 2 n (Ce: a chain of n over roots that are chains of n), n^2 (edge_scalar: 2 n^2 real terms; msg_rescale: the three
reductions' bounds carried through 1 / sqrt, bp_post_ref.msg_rescale), 2 (env_prepare, cscale).  Exact properties use ==.  The worst measured ratio error / bound is
printed per test (MEASURED lines; DESIGN.md 5 records them)."""
import ctypes as C

import numpy as np
import pytest

import tnqs_amd as tn
import bp_post_ref as ref

pytestmark = pytest.mark.gpu
lib = C.CDLL(tn.LIB_PATH)
ERR_UNSUPPORTED = -2                                     # include/tnqs.h
SIZES = (1, 2, 3, 15, 16, 17, 31, 32, 33, 64, 128)
MIXED = (32, 3, 17, 1, 64, 16, 33)                       # one launch of items of different n, not monotonic
DTYPES = (0, 1)
GUARD = 5
SENT = -7.5 + 3.25j
ND = [(n, dt) for dt in DTYPES for n in SIZES]
ND_IDS = [f"n{n}-{'c64' if dt == 0 else 'c128'}" for n, dt in ND]
DT_IDS = ["c64", "c128"]


def _ints(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.int32))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _cat(ms, dt):
    """the items' matrices one after the other, column-major; None = a slot the kernel must not read (filled with NaN)"""
    return np.ascontiguousarray(np.concatenate([ref.flat(m) if not isinstance(m, int) else np.full(m, np.nan) for m in ms]).astype(dt))


def _measured(what, ratio):
    print(f"MEASURED {what}: error / bound = {ratio:.3f}")


class Guarded:
    """an output array as the entry points take it: guard sentinels, item 0, guard sentinels, item 1, ..., guard sentinels"""

    def __init__(self, lens, dt, guard=GUARD):
        self.lens, self.guard = list(lens), guard
        self.fill = np.asarray(SENT).astype(dt) if np.issubdtype(dt, np.complexfloating) else np.asarray(SENT.real).astype(dt)
        self.start = np.cumsum([guard] + [l + guard for l in self.lens])[:-1]
        self.a = np.full(guard + sum(l + guard for l in self.lens), self.fill, dtype=dt)
        self.mask = np.ones(self.a.size, dtype=bool)
        for s, l in zip(self.start, self.lens):
            self.mask[s:s + l] = False

    def item(self, i):
        return self.a[self.start[i]:self.start[i] + self.lens[i]]

    def mats(self, ns):
        return [ref.unflat(self.item(i), n) for i, n in enumerate(ns)]

    def check(self, written=True):
        assert np.all(self.a[self.mask] == self.fill), "a guard element was overwritten"
        if written:
            assert not np.any(self.a[~self.mask] == self.fill), "an element of an item was not written"
        else:
            assert np.all(self.a == self.fill)


def _worst(pairs):
    """pairs of (error array, bound array): asserts every element is inside its bound, returns the worst ratio"""
    w = 0.0
    for e, b in pairs:
        e, b = np.asarray(e, dtype=np.float64), np.asarray(b, dtype=np.float64)
        assert np.all(np.isfinite(e))
        bad = e > b
        assert not bad.any(), f"{int(bad.sum())} elements outside the bound, worst error {e[bad].max():.3e} against {b[bad][np.argmax(e[bad])]:.3e}"
        nz = b > 0
        if nz.any():
            w = max(w, float(np.max(e[nz] / b[nz])))
    return w


# ---- the entry points ---------------------------------------------------------------------------------------------------------------------------------------------
def msg_rescale(ns, mes, mers, dtype, rc_want=0):
    dt = ref.CT[dtype]
    pres = _ints([x is not None for pair in zip(mes, mers) for x in pair])
    a = _cat([m if m is not None else n * n for m, n in zip(mes, ns)], dt); b = _cat([m if m is not None else n * n for m, n in zip(mers, ns)], dt)
    oa, ob = Guarded([n * n for n in ns], dt), Guarded([n * n for n in ns], dt)
    rc = lib.tnqs_dbg_msg_rescale(dtype, len(ns), _p(_ints(ns)), _p(a), _p(b), _p(pres), _p(oa.a), _p(ob.a), GUARD)
    assert rc == rc_want, (rc, lib.tnqs_last_error())
    oa.check(rc == 0); ob.check(rc == 0)
    return oa.mats(ns), ob.mats(ns)


def edge_scalar(ns, mes, mers, dtype, rc_want=0):
    dt = ref.CT[dtype]
    pres = _ints([x is not None for pair in zip(mes, mers) for x in pair])
    a = _cat([m if m is not None else n * n for m, n in zip(mes, ns)], dt); b = _cat([m if m is not None else n * n for m, n in zip(mers, ns)], dt)
    out = np.full(2 * len(ns), -5.0)
    rc = lib.tnqs_dbg_edge_scalar(dtype, len(ns), _p(_ints(ns)), _p(a), _p(b), _p(pres), _p(out))
    assert rc == rc_want, (rc, lib.tnqs_last_error())
    if rc:
        assert np.all(out == -5.0)
    return out[0::2] + 1j * out[1::2]


def env_prepare(ns, ms, dtype, rc_want=0):
    pres = _ints([m is not None for m in ms])
    a = _cat([m if m is not None else n * n for m, n in zip(ms, ns)], ref.CT[dtype])
    H, V = Guarded([n * n for n in ns], np.complex128), Guarded([n * n for n in ns], np.complex128)
    rc = lib.tnqs_dbg_env_prepare(dtype, len(ns), _p(_ints(ns)), _p(a), _p(pres), _p(H.a), _p(V.a), GUARD)
    assert rc == rc_want, (rc, lib.tnqs_last_error())
    H.check(rc == 0); V.check(rc == 0)
    return H.mats(ns), V.mats(ns)


def env_finish(ns, As, Vs, cutoffs, dtype, rc_want=0):
    dt = ref.CT[dtype]
    ms, pr = Guarded([n * n for n in ns], dt), Guarded([n * n for n in ns], dt)
    flags = _ints([-9] * (2 * len(ns)))
    cut = np.ascontiguousarray(np.asarray(cutoffs, dtype=np.float64))
    rc = lib.tnqs_dbg_env_finish(dtype, len(ns), _p(_ints(ns)), _p(_cat(As, np.complex128)), _p(_cat(Vs, np.complex128)), _p(cut), _p(ms.a), _p(pr.a), _p(flags), GUARD)
    assert rc == rc_want, (rc, lib.tnqs_last_error())
    ms.check(rc == 0); pr.check(rc == 0)
    if rc:
        assert np.all(flags == -9)
    return ms.mats(ns), pr.mats(ns), [(int(flags[2 * i]), int(flags[2 * i + 1])) for i in range(len(ns))]


def symg_build(ns, AXs, VXs, AYs, VYs, reg, dtype, rc_want=0):
    dt = ref.CT[dtype]
    g = {k: Guarded([n * n for n in ns], np.complex128) for k in ("rx", "ry", "irx", "iry")}
    g["Ce"] = Guarded([n * n for n in ns], dt); g["Ce0"] = Guarded([n * n for n in ns], dt)
    flag = _ints([-9])
    rc = lib.tnqs_dbg_symg_build(dtype, len(ns), _p(_ints(ns)), _p(_cat(AXs, np.complex128)), _p(_cat(VXs, np.complex128)), _p(_cat(AYs, np.complex128)),
                                 _p(_cat(VYs, np.complex128)), C.c_double(reg), _p(g["rx"].a), _p(g["ry"].a), _p(g["irx"].a), _p(g["iry"].a), _p(g["Ce"].a), _p(g["Ce0"].a),
                                 _p(flag), GUARD)
    assert rc == rc_want, (rc, lib.tnqs_last_error())
    for v in g.values():
        v.check(rc == 0)
    if rc:
        assert flag[0] == -9
    return {k: v.mats(ns) for k, v in g.items()}, int(flag[0])


def symg_finish(ns, USs, Vs, irxs, irys, dtype, rc_want=0):
    dt = ref.CT[dtype]
    Xs, Xd, S = Guarded([n * n for n in ns], dt), Guarded([n * n for n in ns], dt), Guarded(ns, np.float64)
    rc = lib.tnqs_dbg_symg_finish(dtype, len(ns), _p(_ints(ns)), _p(_cat(USs, dt)), _p(_cat(Vs, dt)), _p(_cat(irxs, np.complex128)), _p(_cat(irys, np.complex128)),
                                  _p(Xs.a), _p(Xd.a), _p(S.a), GUARD)
    assert rc == rc_want, (rc, lib.tnqs_last_error())
    Xs.check(rc == 0); Xd.check(rc == 0); S.check(rc == 0)
    return [S.item(i).copy() for i in range(len(ns))], Xs.mats(ns), Xd.mats(ns)


def diag(ns, Ss, dtype, rc_want=0):
    out = Guarded([n * n for n in ns], ref.CT[dtype])
    s = np.ascontiguousarray(np.concatenate(Ss).astype(np.float64))
    rc = lib.tnqs_dbg_diag(dtype, len(ns), _p(_ints(ns)), _p(s), _p(out.a), GUARD)
    assert rc == rc_want, (rc, lib.tnqs_last_error())
    out.check(rc == 0)
    return out.mats(ns)


def cscale(srcs, res, ims, dtype):
    lens = [len(s) for s in srcs]
    out = Guarded(lens, ref.CT[dtype])
    rc = lib.tnqs_dbg_cscale(dtype, len(lens), _p(_ints(lens)), _p(np.ascontiguousarray(np.concatenate(srcs).astype(ref.CT[dtype]))),
                             _p(np.ascontiguousarray(np.asarray(res, dtype=np.float64))), _p(np.ascontiguousarray(np.asarray(ims, dtype=np.float64))), _p(out.a), GUARD)
    assert rc == 0, (rc, lib.tnqs_last_error())
    out.check()
    return [out.item(i).copy() for i in range(len(lens))]


# ---- msg_rescale ------------------------------------------------------------------------------------------------------------------------------------------------------
def _check_rescale(what, ns, mes, mers, dtype):
    oa, ob = msg_rescale(ns, mes, mers, dtype)
    pairs = []
    for n, me, mer, a, b in zip(ns, mes, mers, oa, ob):
        ra, rb, aa, ab, nn = ref.msg_rescale(me, mer, n, dtype)
        pairs += [(ref.err(a, ra), ref.bound(n * n, aa, ra, dtype)), (ref.err(b, rb), ref.bound(n * n, ab, rb, dtype))]
        # what the rescaling is for: the edge scalar of the outputs is 1 (twice the relative bound of the factors, over the sum of |terms|)
        es, are, aim = ref.edge_scalar(a, b, n, 1)
        rel = 2 * float(np.max(ref.bound(n * n, aa, ra, dtype) / np.maximum(np.abs(ra).astype(np.float64), 1e-300)))
        assert abs(complex(es) - 1) <= rel * (are + aim), (n, complex(es))
    _measured(what, _worst(pairs))
    return oa, ob


@pytest.mark.parametrize("n,dtype", ND, ids=ND_IDS)
def test_msg_rescale_general_messages(n, dtype):
    rng = ref.rng_for(10, n, dtype)
    _check_rescale(f"msg_rescale n {n} dtype {dtype}", [n], [ref.message(n, rng)], [ref.message(n, rng)], dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_msg_rescale_mixed_launch_null_messages_and_scales(dtype):
    """one launch of seven edges of different n: both messages null, one null, scales 1e-18 .. 1e6 (the result does not depend on the scale)"""
    rng = ref.rng_for(11, dtype)
    scales = (1e-18, 1e6, 1.0, 1e-9, 1e3, 1e-18, 1e6)
    null = ((0, 0), (1, 0), (0, 1), (1, 1), (0, 0), (0, 1), (0, 0))
    mes = [None if z[0] else ref.message(n, rng, scale=s) for n, s, z in zip(MIXED, scales, null)]
    mers = [None if z[1] else ref.message(n, rng, scale=1 / s if s > 1 else s) for n, s, z in zip(MIXED, scales, null)]
    oa, ob = _check_rescale(f"msg_rescale mixed dtype {dtype}", list(MIXED), mes, mers, dtype)
    i = null.index((1, 1))                                # both null: identity / sqrt(n) on both sides
    assert np.array_equal(oa[i], ob[i]) and np.array_equal(oa[i], np.diag(np.diag(oa[i]))) and abs(oa[i][0, 0] - 1 / np.sqrt(MIXED[i])) < 1e-6


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_msg_rescale_real_negative_scalar_puts_the_sign_into_me(dtype):
    ns, mes, mers = [3, 17, 32], [], []
    for n in ns:
        rng = ref.rng_for(12, n)
        me, mer = rng.standard_normal((n, n)), rng.standard_normal((n, n))
        mes.append(me); mers.append(mer if np.sum(me * mer) < 0 else -mer)
    oa, ob = _check_rescale(f"msg_rescale real negative dtype {dtype}", ns, mes, mers, dtype)
    for me, mer, a, b in zip(mes, mers, oa, ob):
        assert np.all(a.imag == 0) and np.all(b.imag == 0)                                     # the exactly real branch: no phase at all
        assert np.all(np.sign(a.real) == -np.sign(me)) and np.all(np.sign(b.real) == np.sign(mer))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_msg_rescale_tiny_imaginary_part_takes_the_principal_branch(dtype):
    """the same negative real scalar with ONE element given an imaginary part (the only imaginary term of the scalar, so it is not zero in any arithmetic): no sign flip,
    1 / sqrt(n) on the principal branch is -+ i / sqrt|n|"""
    ns, mes, mers = [3, 17], [], []
    for n in ns:
        rng = ref.rng_for(12, n)
        me, mer = rng.standard_normal((n, n)).astype(complex), rng.standard_normal((n, n))
        mer = mer if np.sum(me.real * mer) < 0 else -mer
        me[1 % n, 0] += 1j * abs(me[1 % n, 0]) * (1e-5 if dtype == 0 else 1e-13) * np.sign(mer[1 % n, 0])        # Im(n) > 0, arg(n) just below +pi
        mes.append(me); mers.append(mer)
    oa, ob = _check_rescale(f"msg_rescale tiny imaginary dtype {dtype}", ns, mes, mers, dtype)
    for n, me, mer, a, b in zip(ns, mes, mers, oa, ob):
        nn = ref.msg_rescale(me, mer, n, dtype)[4]
        assert nn.imag > 0 and nn.real < 0
        big = np.abs(mer) > 0.1                          # 1 / sqrt(n) = -i / sqrt|n| (1 + O(1e-5)): real inputs come out imaginary, sign(Im) = -sign(input)
        assert np.all(np.sign(b.imag[big]) == -np.sign(mer[big])) and np.all(np.abs(b.real[big]) < 1e-4 * np.abs(b.imag[big]))
        big = np.abs(me.real) > 0.1
        assert np.all(np.sign(a.imag[big]) == -np.sign(me.real[big]))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_msg_rescale_zero_message_gives_zeros(dtype):
    """a zero message has no norm to divide by: the reference yields NaN (0 / 0); the kernel writes finite zeros to BOTH outputs"""
    rng = ref.rng_for(13)
    ns = [17, 3]
    oa, ob = msg_rescale(ns, [np.zeros((17, 17)), ref.message(3, rng)], [ref.message(17, rng), np.zeros((3, 3))], dtype)
    for a, b in zip(oa, ob):
        assert np.all(a == 0) and np.all(b == 0)
    assert np.all(np.isnan(ref.msg_rescale(np.zeros((3, 3)), ref.message(3, rng), 3, dtype)[0]))


# ---- edge_scalar ------------------------------------------------------------------------------------------------------------------------------------------------------
def _check_edge_scalar(what, ns, mes, mers, dtype):
    got = edge_scalar(ns, mes, mers, dtype)
    pairs = []
    for n, me, mer, v in zip(ns, mes, mers, got):
        r, are, aim = ref.edge_scalar(me, mer, n, dtype)
        d = np.clongdouble(v) - r
        pairs += [(abs(float(d.real)), ref.bound(2 * n * n, are, 0, 1)), (abs(float(d.imag)), ref.bound(2 * n * n, aim, 0, 1))]
    _measured(what, _worst(pairs))
    return got


@pytest.mark.parametrize("n,dtype", ND, ids=ND_IDS)
def test_edge_scalar_general_messages(n, dtype):
    rng = ref.rng_for(20, n, dtype)
    _check_edge_scalar(f"edge_scalar n {n} dtype {dtype}", [n], [ref.message(n, rng)], [ref.message(n, rng)], dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_edge_scalar_mixed_launch_null_messages_and_cancellation(dtype):
    rng = ref.rng_for(21, dtype)
    null = ((0, 0), (1, 0), (0, 1), (1, 1), (0, 0), (0, 1), (0, 0))
    ns = list(MIXED)
    mes = [None if z[0] else ref.message(n, rng) for n, z in zip(ns, null)]
    mers = [None if z[1] else ref.message(n, rng) for n, z in zip(ns, null)]
    for n in (16, 64, 32):                               # me = [u u], mer = [w -w]: the terms cancel in pairs, the sum is rounding only -- held to the summation bound
        u = ref.message(n, rng)[:, :n // 2].astype(ref.CT[dtype]); w = ref.message(n, rng)[:, :n // 2].astype(ref.CT[dtype])
        ns.append(n); mes.append(np.hstack([u, u])); mers.append(np.hstack([w, -w]))
    got = _check_edge_scalar(f"edge_scalar mixed dtype {dtype}", ns, mes, mers, dtype)
    assert got[null.index((1, 1))] == MIXED[null.index((1, 1))]                                 # trace of the identity, exactly
    assert abs(got[1] - np.trace(mers[1].astype(ref.CT[dtype]))) < 1e-5                       # me null: the trace of mer
    for k in (-1, -2, -3):
        assert abs(got[k]) < 1e-6 * ref.edge_scalar(mes[k], mers[k], ns[k], dtype)[1]          # (and far below the sum of |terms|: it did cancel)


# ---- env_prepare ------------------------------------------------------------------------------------------------------------------------------------------------------
def _check_env_prepare(what, ns, ms, dtype):
    Hs, Vs = env_prepare(ns, ms, dtype)
    pairs = []
    for n, m, H, V in zip(ns, ms, Hs, Vs):
        assert np.array_equal(H, H.conj().T), "H is not exactly Hermitian"
        assert np.array_equal(V, np.eye(n)), "V is not exactly the identity"
        rH, _, aH = ref.env_prepare(m, n, dtype)
        if m is None:
            assert np.array_equal(H, np.eye(n))
        pairs.append((ref.err(H, rH), ref.bound(2, aH, rH, 1)))                                 # (H is complex128 for both dtypes: no rounding to T)
    _measured(what, _worst(pairs))


@pytest.mark.parametrize("n,dtype", ND + [(256, 0), (256, 1)], ids=ND_IDS + ["n256-c64", "n256-c128"])
def test_env_prepare_general_messages(n, dtype):
    _check_env_prepare(f"env_prepare n {n} dtype {dtype}", [n], [ref.message(n, ref.rng_for(30, n, dtype))], dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_env_prepare_mixed_launch_with_null_messages(dtype):
    rng = ref.rng_for(31, dtype)
    _check_env_prepare(f"env_prepare mixed dtype {dtype}", list(MIXED), [None if i in (1, 4) else ref.message(n, rng) for i, n in enumerate(MIXED)], dtype)


# ---- env_finish -------------------------------------------------------------------------------------------------------------------------------------------------------
CUT = {0: float(np.float32(1e-3)), 1: 1e-3}              # (a cutoff real(T) represents: the reference compares in T, the kernel in double, which then agree)


def _check_env_finish(what, ns, As, Vs, cuts, dtype):
    ms, pr, flags = env_finish(ns, As, Vs, cuts, dtype)
    pairs, refs = [], []
    for n, A, V, c, m, p, f in zip(ns, As, Vs, cuts, ms, pr, flags):
        rm, rp, am, ap, rf, lam, kept = ref.env_finish(A, V, c, dtype)
        assert f == rf, (n, f, rf)
        bm, bp = ref.bound(n, am, rm, dtype), ref.bound(n, ap, rp, dtype)
        pairs += [(ref.err(m, rm), bm), (ref.err(p, rp), bp)]
        # proj is the orthogonal projector on the kept space and msqrt lives there: (P + E)^2 - (P + E) = P E + E P - E + E^2, |E| <= the bound, |P| <= 1, plus
        # what the reference's own P misses (the eigenvectors are orthonormal to f64 rounding only)
        P, M = p.astype(np.complex128), m.astype(np.complex128)
        rP, rM = np.asarray(rp).astype(np.complex128), np.asarray(rm).astype(np.complex128)
        tol_p = (2 * n + 2) * 2 * np.max(bp) + np.max(np.abs(rP @ rP - rP))
        tol_m = (n + 1) * 2 * (np.max(bm) + np.max(np.abs(rM)) * np.max(bp)) + np.max(np.abs(rM @ rP - rM))
        assert np.max(np.abs(P @ P - P)) <= tol_p and np.max(np.abs(M @ P - M)) <= tol_m
        assert np.array_equal(np.round(np.einsum("ij,ik,kj->j", V.conj(), P, V).real).astype(int), kept.astype(int))        # which columns were kept
        refs.append((rf, kept))
    _measured(what, _worst(pairs))
    return refs


@pytest.mark.parametrize("n,dtype", ND + [(256, 0), (256, 1)], ids=ND_IDS + ["n256-c64", "n256-c128"])
def test_env_finish_full_rank_spectrum_keeps_every_column(n, dtype):
    A, V, w = ref.eig_factors(ref.psd(n, ref.rng_for(40, n, dtype)))
    cut = min(CUT[dtype], float(np.float32(w.min() / 4)))
    (rf, kept), = _check_env_finish(f"env_finish n {n} dtype {dtype}", [n], [A], [V], [cut], dtype)
    assert rf == (1, 0) and kept.all()


def _edge_spectrum(n, dtype):
    """0 | just below the cutoff | just above | below in f64 but ON the cutoff once cast to f32 | above | negative beyond the cutoff | the rest in (0.2, 1)"""
    c = CUT[dtype]
    lam = np.linspace(0.2, 1.0, n)
    lam[:6] = [0.0, c * (1 - 2.0 ** -20), c * (1 + 2.0 ** -20), c * (1 - 2.0 ** -30), c * (1 + 2.0 ** -30), -0.3]
    kept = np.ones(n, dtype=bool); kept[[0, 1, 5]] = False; kept[3] = dtype == 0
    return lam, kept


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_env_finish_cutoff_after_the_cast_zero_and_negative_eigenvalues(dtype):
    """one launch: the edge spectrum at n = 17, 33, 7, the same without the negative eigenvalue (no error flag), and a full-rank item in between (flags (1, 0))"""
    ns, As, Vs, cuts, want = [], [], [], [], []
    for k, n in enumerate((17, 33, 7, 17)):
        rng = ref.rng_for(41, n, dtype, k)
        lam, kept = _edge_spectrum(n, dtype)
        if k == 3:
            lam[5] = 0.3; kept[5] = True
        perm = rng.permutation(n); lam, kept = lam[perm], kept[perm]
        A, V = ref.factors_with_spectrum(n, lam, rng)
        ns.append(n); As.append(A); Vs.append(V); cuts.append(CUT[dtype]); want.append(((0, 0 if k == 3 else 1), kept))
        if k == 1:
            A, V, _ = ref.eig_factors(ref.psd(16, rng))
            ns.append(16); As.append(A); Vs.append(V); cuts.append(1e-6); want.append(((1, 0), np.ones(16, dtype=bool)))
    got = _check_env_finish(f"env_finish edges dtype {dtype}", ns, As, Vs, cuts, dtype)
    for (rf, kept), (wf, wk) in zip(got, want):
        assert rf == wf and np.array_equal(kept, wk)     # (the reference's decisions are the ones written down above; the kernel's equal the reference's)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_env_finish_mixed_launch_with_a_cutoff_per_item(dtype):
    """one launch of seven items of different n, each with a cutoff of its own: full-rank spectra cut at another depth each (half, none, five, one column dropped) and
    the edge spectrum at n = 17 and 33 -- an item that read another item's cutoff, or wrote its two flags to another item's slot, shows in the flags and the projector"""
    rng = ref.rng_for(42, dtype)
    ns, As, Vs, cuts, want = list(MIXED), [], [], [], []
    for n, drop in zip(ns, (16, 0, None, 0, 5, 1, None)):                                        # columns the cutoff drops; None: the edge spectrum
        if drop is None:
            lam, kept = _edge_spectrum(n, dtype)
            perm = rng.permutation(n); lam, kept = lam[perm], kept[perm]
            A, V = ref.factors_with_spectrum(n, lam, rng)
            cut, flags = CUT[dtype], (0, 1)
        else:
            A, V, w = ref.eig_factors(ref.psd(n, rng))                                          # (w ascending: the cutoff drops the first `drop` columns)
            cut = float(np.float32(w[0] / 4 if drop == 0 else np.sqrt(w[drop - 1] * w[drop])))
            assert drop == 0 or float(np.float32(w[drop - 1])) < cut < float(np.float32(w[drop]))
            kept, flags = np.arange(n) >= drop, (int(drop == 0), 0)
        As.append(A); Vs.append(V); cuts.append(cut); want.append((flags, kept))
    assert len(set(cuts)) >= 6
    got = _check_env_finish(f"env_finish mixed dtype {dtype}", ns, As, Vs, cuts, dtype)
    for (rf, kept), (wf, wk) in zip(got, want):
        assert rf == wf and np.array_equal(kept, wk)


# ---- symg_build -------------------------------------------------------------------------------------------------------------------------------------------------------
def _check_symg_build(what, ns, fx, fy, reg, dtype, want_flag=0):
    out, flag = symg_build(ns, [f[0] for f in fx], [f[1] for f in fx], [f[0] for f in fy], [f[1] for f in fy], reg, dtype)
    pairs, refs = [], []
    want = 0
    for i, n in enumerate(ns):
        r, ab = ref.symg_build(fx[i][0], fx[i][1], fy[i][0], fy[i][1], reg, dtype)
        want |= r["flag"]
        for k in ("rx", "ry", "irx", "iry"):
            assert np.all(np.isfinite(out[k][i]))
            pairs.append((ref.err(out[k][i], r[k]), ref.bound(n, ab[k], r[k], 1)))              # (complex128 outputs for both dtypes)
        pairs.append((ref.err(out["Ce"][i], r["Ce"]), ref.bound(2 * n, ab["Ce"], r["Ce"], dtype)))
        assert np.array_equal(out["Ce"][i], out["Ce0"][i]), "Ce and Ce0 differ"
        refs.append(r)
    assert flag == want == want_flag
    _measured(what, _worst(pairs))
    return out, refs


@pytest.mark.parametrize("reg0", (False, True), ids=("reg-default", "reg-0"))
@pytest.mark.parametrize("n,dtype", ND, ids=ND_IDS)
def test_symg_build_from_eigen_factors(n, dtype, reg0):
    rng = ref.rng_for(50, n, dtype)
    fx, fy = ref.eig_factors(ref.psd(n, rng))[:2], ref.eig_factors(ref.psd(n, rng))[:2]
    _check_symg_build(f"symg_build n {n} dtype {dtype} reg0 {reg0}", [n], [fx], [fy], 0.0 if reg0 else ref.DEFAULT_REG[dtype], dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_symg_build_at_the_largest_bond_dimension(dtype):
    rng = ref.rng_for(51, dtype)
    fx, fy = ref.eig_factors(ref.psd(256, rng))[:2], ref.eig_factors(ref.psd(256, rng))[:2]
    _check_symg_build(f"symg_build n 256 dtype {dtype}", [256], [fx], [fy], ref.DEFAULT_REG[dtype], dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_symg_build_mixed_launch(dtype):
    rng = ref.rng_for(52, dtype)
    fx = [ref.eig_factors(ref.psd(n, rng))[:2] for n in MIXED]; fy = [ref.eig_factors(ref.psd(n, rng))[:2] for n in MIXED]
    _check_symg_build(f"symg_build mixed dtype {dtype}", list(MIXED), fx, fy, ref.DEFAULT_REG[dtype], dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_symg_build_regularisation_flag_and_zero_eigenvalue(dtype):
    reg = ref.DEFAULT_REG[dtype]
    for n in (3, 17):
        rng = ref.rng_for(53, n, dtype)
        good = ref.factors_with_spectrum(n, np.linspace(0.2, 1.0, n), rng)
        lam = np.linspace(0.2, 1.0, n); lam[1] = -reg / 2                                      # reg lifts it over zero: no flag, a finite inverse root
        _check_symg_build(f"symg_build -reg/2 n {n} dtype {dtype}", [n], [ref.factors_with_spectrum(n, lam, rng)], [good], reg, dtype, want_flag=0)
        _check_symg_build(f"symg_build -reg/2 y n {n} dtype {dtype}", [n, n], [good, good], [ref.factors_with_spectrum(n, lam, rng), good], reg, dtype, want_flag=0)
        lam[1] = -2 * reg                                                                       # still negative: the flag, in either message
        _check_symg_build(f"symg_build -2reg x n {n} dtype {dtype}", [n], [ref.factors_with_spectrum(n, lam, rng)], [good], reg, dtype, want_flag=1)
        _check_symg_build(f"symg_build -2reg y n {n} dtype {dtype}", [n, n], [good, good], [good, ref.factors_with_spectrum(n, lam, rng)], reg, dtype, want_flag=1)
        lam[1] = 0.0                                                                            # reg = 0 and a zero eigenvalue: inverse root 0, not inf
        A, V = ref.factors_with_spectrum(n, lam, rng)
        out, _ = _check_symg_build(f"symg_build zero eigenvalue n {n} dtype {dtype}", [n], [(A, V)], [good], 0.0, dtype, want_flag=0)
        v = V[:, 1]
        assert abs(v.conj() @ out["irx"][0].conj() @ v) < 1e-12 and abs(v.conj() @ out["rx"][0].conj() @ v) < 1e-12


# ---- symg_finish ------------------------------------------------------------------------------------------------------------------------------------------------------
def _svd_factors(n, dtype, rng, sigma=None):
    """U Sigma and V of a random n x n matrix (numpy's SVD in f64; sigma: replaces the singular values), columns shuffled, and two inverse roots"""
    u, s, vh = np.linalg.svd(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    s = s / s[0] if sigma is None else np.asarray(sigma, dtype=np.float64)
    order = rng.permutation(n)
    if n > 1 and np.array_equal(s[order], np.sort(s)[::-1]):
        order = np.roll(order, 1)                        # (never hand the columns over sorted)
    fx, fy = ref.eig_factors(ref.psd(n, rng)), ref.eig_factors(ref.psd(n, rng))
    irx = ((fx[1] / np.sqrt(fx[2])) @ fx[1].conj().T).conj(); iry = ((fy[1] / np.sqrt(fy[2])) @ fy[1].conj().T).conj()
    return (u * s)[:, order].astype(ref.CT[dtype]), vh.conj().T[:, order].astype(ref.CT[dtype]), irx, iry


def _check_symg_finish(what, ns, fs, dtype):
    Ss, Xss, Xds = symg_finish(ns, [f[0] for f in fs], [f[1] for f in fs], [f[2] for f in fs], [f[3] for f in fs], dtype)
    pairs, perms = [], []
    for n, f, S, Xs, Xd in zip(ns, fs, Ss, Xss, Xds):
        rS, rXs, rXd, aXs, aXd, perm = ref.symg_finish(*f, dtype)
        assert np.all(np.diff(S) <= 0) and np.array_equal(S, S.astype(ref.RT[dtype]).astype(np.float64))       # descending, and (double)(T)sigma
        pairs += [(np.abs(S - rS).astype(np.float64), ref.bound(n, rS.astype(np.float64), rS, dtype)), (ref.err(Xs, rXs), ref.bound(n, aXs, rXs, dtype)),
                  (ref.err(Xd, rXd), ref.bound(n, aXd, rXd, dtype))]
        perms.append(perm)
    _measured(what, _worst(pairs))
    return Ss, Xss, Xds, perms


@pytest.mark.parametrize("n,dtype", ND + [(256, 0), (256, 1)], ids=ND_IDS + ["n256-c64", "n256-c128"])
def test_symg_finish_sorts_shuffled_triplets(n, dtype):
    f = _svd_factors(n, dtype, ref.rng_for(60, n, dtype))
    _, _, _, (perm,) = _check_symg_finish(f"symg_finish n {n} dtype {dtype}", [n], [f], dtype)
    assert n < 2 or not np.array_equal(perm, np.arange(n))                                      # the kernel did have to sort


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_symg_finish_mixed_launch_ties_zero_and_nan_columns(dtype):
    ns, fs = list(MIXED), []
    for k, n in enumerate(MIXED):
        rng = ref.rng_for(61, n, dtype)
        US, V, irx, iry = _svd_factors(n, dtype, rng)
        if n >= 16:
            lo, hi = 2, n - 3
            US[:, hi] = -US[:, lo]                       # |column| exactly equal: two equal singular values, the lower column index has to come first
            US[:, 5] = 0                                 # a zero singular value: zero columns of Xs and Xd
            US[1, 7] = np.nan                            # a column that is not a number: S entry 0, zero columns, nobody else disturbed
            if dtype == 1:
                US[:, 9] = 1e150 * (1 + 1j)              # norm^2 = 2e300 n, finite but not < 1e300: the other half of the guard (out of complex64's range)
        fs.append((US, V, irx, iry))
    dead = {5, 7, 9} if dtype == 1 else {5, 7}
    Ss, Xss, Xds, perms = _check_symg_finish(f"symg_finish edges dtype {dtype}", ns, fs, dtype)
    for n, S, Xs, Xd, perm in zip(ns, Ss, Xss, Xds, perms):
        if n < 16:
            continue
        pos = {int(c): int(r) for r, c in enumerate(perm)}
        assert pos[n - 3] == pos[2] + 1 and S[pos[2]] == S[pos[n - 3]] > 0                     # the tie, in stable order
        k = len(dead)
        assert list(perm[-k:]) == sorted(dead) and np.all(S[-k:] == 0) and np.all(S[:-k] > 0) # (the dead columns tie at 0: stable order among them too)
        assert np.all(Xs[:, -k:] == 0) and np.all(Xd[:, -k:] == 0) and np.all(np.isfinite(Xs)) and np.all(np.isfinite(Xd))


# ---- diag, cscale -----------------------------------------------------------------------------------------------------------------------------------------------------
def _check_diag(ns, dtype):
    Ss = [ref.rng_for(70, n, k).random(n) * 10.0 ** ref.rng_for(71, n, k).integers(-12, 3, n) for k, n in enumerate(ns)]
    for n, S, m in zip(ns, Ss, diag(ns, Ss, dtype)):
        assert np.array_equal(m, ref.diag(S, dtype)) and np.count_nonzero(m) == n and m.dtype == ref.CT[dtype]


@pytest.mark.parametrize("n,dtype", ND, ids=ND_IDS)
def test_diag_is_exact(n, dtype):
    _check_diag([n], dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_diag_is_exact_in_a_mixed_launch(dtype):
    _check_diag([17, 33] + list(MIXED), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_cscale_to_one_rounding(dtype):
    lens = [257, 1, 64 * 256 + 3, 255, 2 * 33 * 33, 256]                                        # (the third: more than one trip of the 64 x 256 grid stride)
    rng = ref.rng_for(72, dtype)
    srcs = [rng.standard_normal(l) + 1j * rng.standard_normal(l) for l in lens]
    res, ims = rng.standard_normal(len(lens)), rng.standard_normal(len(lens))
    pairs = []
    for s, re, im, got in zip(srcs, res, ims, cscale(srcs, res, ims, dtype)):
        v, a = ref.cscale(s, re, im, dtype)
        pairs.append((ref.err(got, v), ref.bound(2, a, np.maximum(np.abs(v.real), np.abs(v.imag)), dtype)))
    _measured(f"cscale dtype {dtype}", _worst(pairs))


# ---- refusal ------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_bond_dimension_above_256_is_refused_and_nothing_is_written(dtype):
    ns = [3, 257]
    z = [np.eye(n, dtype=complex) for n in ns]
    msg_rescale(ns, z, z, dtype, ERR_UNSUPPORTED)
    edge_scalar(ns, z, z, dtype, ERR_UNSUPPORTED)
    env_prepare(ns, z, dtype, ERR_UNSUPPORTED)
    env_finish(ns, z, z, [1e-6, 1e-6], dtype, ERR_UNSUPPORTED)
    symg_build(ns, z, z, z, z, 0.0, dtype, ERR_UNSUPPORTED)
    symg_finish(ns, z, z, z, z, dtype, ERR_UNSUPPORTED)
    diag(ns, [np.ones(n) for n in ns], dtype, ERR_UNSUPPORTED)


# ---- the engine's wiring at the benchmark's bond dimensions ---------------------------------------------------------------------------------------------------------
# The kernel tests above do not show that symmetric_gauge_t and rescale_messages_t hand the kernels the right buffers once n^2 > 256: a ring of four sites
# 2 x chi x chi against the oracle.  ComplexF64 is held to 1e-9 (the parity tests' level, widened for chi and the conditioning: the oracle's messages have condition
# numbers 65 (chi 17) and 114 (chi 32) here).  ComplexF32 is held to 4 x the deviation of the ORACLE's own complex64 run from its complex128 run on the same state
# and schedule (seed 5, maxiter 8, computed on the CPU: the reference's f32 noise; 4 allows another, equally valid summation order):
#                      edge scalars (relative)   rescaled messages (max norm)   S / sum(S)
ORACLE_F32_NOISE = {17: (1.13e-7,                7.64e-8,                       4.45e-6),
                    32: (1.60e-7,                6.87e-8,                       4.63e-6)}


@pytest.mark.parametrize("chi", (17, 32))
@pytest.mark.parametrize("dtype", (np.complex64, np.complex128), ids=DT_IDS)
def test_engine_rescale_and_gauge_match_the_oracle_on_a_ring(dtype, chi):
    import tnqs_oracle as o
    import statevector as sv
    from helpers import to_oracle_state
    tol_es, tol_msg, tol_S = [4 * x for x in ORACLE_F32_NOISE[chi]] if dtype == np.complex64 else (1e-9, 1e-9, 1e-9)
    g = tn.named_grid((2, 2))
    psi = tn.random_tensornetworkstate(dtype, g, bond_dimension=chi, seed=5)
    kw = dict(maxiter=8, tolerance=None, edge_sequence=tn.forest_cover_edge_sequence(g))
    bpc = tn.update(tn.BeliefPropagationCache(psi), **kw)
    oc = o.update(o.BeliefPropagationCache(to_oracle_state(psi)), **kw)
    assert max(np.linalg.cond(oc.message(e).astype(np.complex128)) for e in oc.g.directed_edges()) < 1e4
    es = tn.edge_scalars(bpc)
    worst = [0.0, 0.0, 0.0]
    for i, e in enumerate(g.edges):
        r = o.edge_scalar(oc, e)
        worst[0] = max(worst[0], abs(es[i] - r) / abs(r))
    rm, orm = tn.rescale_messages(bpc), o.rescale(oc)
    for (a, b) in g.edges:
        for d in ((a, b), (b, a)):
            worst[1] = max(worst[1], np.max(np.abs(rm.message(d) - orm.message(d))) / max(1.0, np.max(np.abs(orm.message(d)))))
    scal = np.abs(tn.edge_scalars(rm) - 1)
    sg, osg = tn.symmetric_gauge(bpc), o.symmetric_gauge(oc)
    for (a, b) in g.edges:
        m, mr = sg.message((a, b)), sg.message((b, a))
        assert np.max(np.abs(m - np.diag(np.diag(m)))) == 0 and np.array_equal(m, mr)          # exactly diagonal, equal in both directions
        S, So = np.diag(m).real, np.diag(osg.message((a, b))).real
        assert np.all(np.diff(S) <= 0)
        worst[2] = max(worst[2], np.max(np.abs(S / S.sum() - So / So.sum())))
    v0 = sv.tns_to_statevector(to_oracle_state(psi)); v1 = sv.tns_to_statevector(to_oracle_state(sg.network()))
    fid = abs(sv.fidelity(v0, v1) - 1)
    print(f"MEASURED engine chi {chi} {np.dtype(dtype).name}: edge scalars {worst[0]:.3e} (tol {tol_es:.3e}), rescaled messages {worst[1]:.3e} (tol {tol_msg:.3e}), "
          f"|edge scalar - 1| {scal.max():.3e}, spectra {worst[2]:.3e} (tol {tol_S:.3e}), |fidelity - 1| {fid:.3e}")
    assert worst[0] <= tol_es and worst[1] <= tol_msg and worst[2] <= tol_S
    assert scal.max() <= tol_es and fid <= tol_S
