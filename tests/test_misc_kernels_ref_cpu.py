"""CPU checks of tests/misc_kernels_ref.py, the restatements tests/test_gpu_misc_kernels.py holds the small kernels to, and of the inputs that test uses: the conditions
its bounds assume are asserted here on the same inputs, without a GPU."""
import ctypes as C

import numpy as np
import pytest

import tnqs_amd as tn
import inner_ref
import amplitude_ref as amp
import misc_kernels_ref as ref


def test_permute_restatement_is_numpy_transpose():
    for rank, shape in ref.PERM_SHAPES.items():
        x = ref.ramp(int(np.prod(shape)), np.complex128)
        for perm in ref.perms_of(rank):
            dims, st = ref.permute_args(shape, perm)
            want = np.transpose(x.reshape(shape, order="F"), perm).ravel(order="F")
            assert np.array_equal(ref.permute_ref(x, dims, st), want), (rank, perm)
    perms = [tuple(p) for p in ref.perms_of(5)]
    assert len(set(perms)) == 5                       # the two random ones are neither each other nor one of the three named ones


def test_ramp_is_exact_in_both_types():
    n = int(np.prod(ref.PERM_LARGE))
    a, b = ref.ramp(n, np.complex64), ref.ramp(n, np.complex128)
    assert np.array_equal(a.astype(np.complex128), b) and len(np.unique(a)) == n


def test_dot_and_norm_restatements_agree_with_numpy():
    for n in (1, 255, 4097):
        x, y = ref.dot_inputs(n, np.complex128)
        re, im, mre, mim = ref.dot_ref(x, y)
        want = np.vdot(x.conj(), y)
        assert abs(complex(re, im) - want) <= 4 * n * np.finfo(np.float64).eps * max(mre, mim)
        v = ref.norm_inputs(n, np.complex128)
        assert abs(float(ref.norm_ref(v)) - np.linalg.norm(v)) <= 4 * n * np.finfo(np.float64).eps * np.linalg.norm(v)
    assert ref.sum_ref([1e100, 1.0, -1e100]) == 1.0


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_dot_inputs_do_not_cancel(dtype):
    for n in ref.DOT_LENGTHS:
        x, y = ref.dot_inputs(n, dtype)
        k = ref.cancellation(x, y)
        print(f"MEASURED dot inputs n={n} {np.dtype(dtype).name}: sum|x||y| / |sum x y| = {k:.3f}")
        assert k <= ref.DOT_CAP


def test_loop_dot_plan_host_only():
    lib = C.CDLL(tn.LIB_PATH)
    ns = np.asarray([0, 1, 4096, 4097, 300001, 4096 * 1024, 4096 * 1024 + 1, 4096 * 1024 + 4097, 1 << 40], dtype=np.int64)
    nwg = np.full(len(ns), -1, dtype=np.int32)
    rc = lib.tnqs_dbg_loop_dot(0, len(ns), ns.ctypes.data_as(C.c_void_p), None, None, None, nwg.ctypes.data_as(C.c_void_p))
    assert rc == 0
    assert nwg.tolist() == [ref.loop_dot_nwg(int(n)) for n in ns] == [1, 1, 1, 2, 74, 1024, 1024, 1024, 1024]


def test_scalar_restatement_is_the_amplitude_on_a_tree():
    g, ket, _ = inner_ref.tree_case("comb33")
    rng = np.random.default_rng(11)
    for x in amp.random_strings(rng, g, 4):
        for normalize in (True, False):
            ac = amp.run(g, ket, dict(zip(g.vertices, x)), 1, normalize=normalize)
            items, nv, cfg = ref.items_of_cache(ac, normalize)
            re, im, flags, _ = ref.scalar_ref(items, nv, cfg)
            want = amp.log_amplitude(ac)
            assert flags[0] == 0
            assert amp.log_close(complex(float(re[0]), float(im[0])), want) < 1e-12


def test_scalar_restatement_flags_and_wrap():
    one = np.ones((1, 1))
    it = lambda z: ref.ScalarItem(1, one * z, None)      # noqa: E731
    cfg = np.zeros((1, 4), dtype=np.int32)
    re, im, fl, _ = ref.scalar_ref([it(-1.0), it(-1.0), it(-1.0)], 3, cfg)      # 3 pi -> pi, not -pi
    near_pi = lambda v: abs(abs(float(v)) - np.pi) < 1e-15      # noqa: E731  (an odd multiple of pi sits on the cut: either end of (-pi, pi] up to rounding)
    assert fl[0] == 0 and re[0] == 0 and near_pi(im[0])
    re, im, fl, _ = ref.scalar_ref([it(1.0), it(-1.0)], 1, cfg)                 # -pi -> pi
    assert near_pi(im[0])
    re, im, fl, _ = ref.scalar_ref([it(np.exp(3j)), it(np.exp(3j)), it(np.exp(-3j))], 2, cfg)      # 3 + 3 + 3 = 9 -> 9 - 2 pi
    assert abs(float(im[0]) - (9 - 2 * np.pi)) < 1e-15
    re, im, fl, _ = ref.scalar_ref([it(0.0), it(2.0)], 2, cfg)
    assert fl[0] == 1 and re[0] == -np.inf and im[0] == 0
    re, im, fl, _ = ref.scalar_ref([it(0.0), it(np.inf)], 2, cfg)
    assert fl[0] == 3 and np.isnan(re[0]) and np.isnan(im[0])


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("nstr", ref.SCALAR_STRINGS)
def test_scalar_inputs_keep_kappa_under_the_cap_and_cross_two_pi(nstr, dtype):
    items, nv, ne, cfg = ref.scalar_case(nstr, dtype)
    assert cfg.shape[1] > nv and {it.chi for it in items} >= {1, 2, 63, 64}
    vals, kap = ref.item_values(items, cfg)
    re, im, flags, phase_mag = ref.scalar_ref(items, nv, cfg)
    want = np.zeros(nstr, dtype=np.int32)
    for s, f in ((ref.ZERO_STRING, 1), (ref.INF_STRING, 2), (ref.BOTH_STRING, 3)):
        if nstr > s:
            want[s] = f
    assert flags.tolist() == want.tolist()
    ok = np.isfinite(vals.real) & np.isfinite(vals.imag) & (vals != 0)
    worst = float(np.max(kap[ok]))
    print(f"MEASURED amp_scalar inputs nstr={nstr} {np.dtype(dtype).name}: worst kappa = {worst:.3f}, sum of |phases| = {phase_mag.max():.1f} rad")
    assert worst <= ref.KAPPA_CAP
    clean = flags == 0
    assert np.all(phase_mag[clean] > 5 * 2 * np.pi)                                   # the running sum passes 2 pi several times
    assert np.all((im[clean] > -np.pi) & (im[clean] <= np.pi))
    negreal = [i for i, it in enumerate(items) if it.site is None and it.m is not None and np.all(vals[i].imag == 0) and np.all(vals[i].real < 0)]
    assert len(negreal) >= 2 and min(negreal) < nv <= max(negreal)                    # exactly negative real: one vertex item, one edge item


def test_random_fill_restatement_statistics():
    """the seed of the GPU test's statistics holds all three bounds on the restatement itself; splitmix64 is the published generator (first outputs from seed 0)"""
    assert [int(v) for v in ref.splitmix64(np.arange(3, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    re, im, rad = ref.random_fill_ref(np.arange(ref.FILL_STATS_N), ref.FILL_STATS_SEED, 0.5)
    st = ref.fill_stats(re, im, 0.5)
    print("MEASURED random_fill restatement statistics (each <= 5): " + ", ".join(f"{s:.3f}" for s in st))
    assert max(st) <= 5.0
    assert np.all(np.isfinite(rad.astype(np.float64))) and float(rad.max()) <= np.sqrt(2 * 32 * np.log(2.0)) + 1e-9      # u1 >= 2^-32
    re2, im2, _ = ref.random_fill_ref(np.arange(1000), ref.FILL_STATS_SEED, 0.5, real_only=True)
    assert np.array_equal(re2, re[:1000]) and not im2.any()


def test_sweep_end_restatement():
    diffs = np.array([[0.5, 0.25, 1.0], [0.5, 0.75, 3.0]])
    done, niter, fdiff = ref.sweep_end_ref(diffs, 4, 0.5, np.array([0, 0, 1], dtype=np.int32), np.array([1, 1, 2], dtype=np.int32), np.array([9.0, 9.0, 7.0]))
    assert done.tolist() == [1, 1, 1] and niter.tolist() == [4, 4, 2] and fdiff.tolist() == [0.5, 0.5, 7.0]
    done, _, _ = ref.sweep_end_ref(diffs, 4, -1.0, np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int32), np.zeros(3))
    assert not done.any()


def test_record_restatement_layout():
    rec = ref.record_ref([9, 9, 5, 1], 0.125, [3.0, 2.0], [7, 8], 64, 96, 0xAB)
    assert rec[:32].view(np.float64).tolist() == [5.0, 1.0, 0.125, 0.0] and rec[32:48].view(np.float64).tolist() == [3.0, 2.0]
    assert np.all(rec[48:64] == 0xAB) and rec[64:80].view(np.uint64).tolist() == [7, 8] and np.all(rec[80:] == 0xAB)
