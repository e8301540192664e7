"""Kernel-level GPU tests of the SVD stage of a two-site gate as the engine launches it -- csrc/gate_svd.cpp launch_theta_svd_stage, the function
TwoSiteBatch::svd_and_finish calls: the gates' JacobiItems, svd_batch (theta_svd_pre_kernel, jacobi_lds_kernel, jacobi_kernel, the tall route) and the recovery of V
(recover_v_mfma_kernel / recover_v_kernel<T, 8>) -- through tnqs_dbg_theta_svd_stage (include/tnqs_debug.h), against the complex128 reference and the checks of
tests/theta_svd_ref.py (checked themselves in tests/test_theta_svd_ref_cpu.py).

What the single-item kernel tests cannot see and these launches can: an item offered to several launches at once, each kernel deciding ON THE DEVICE whether it is its
own (three spellings of theta_pre_takes: an item taken twice, or by nobody, fails its numbers or the who-ran check); dimensions read on the device inside launches
sized from upper bounds (ranks below the bounds, a small item in a launch instantiated for a large one, the leading dimension r d inside a slot sized for the bound);
V recovered with nu < n; rows 257..512 (jacobi_kernel<T, 8>, the tall route and both recovery kernels on 260 rows); recover_v_kernel<float, 8>.  All d = 2, the smallest
shapes that reach each branch (the item tables: theta_svd_ref.dyn_f32_items / dyn_f64_items / static_items).

Tolerances are those of the single-item test of the kernel that route_out names, or derived (theta_svd_ref's docstring); none is measured here.  Every test prints the
error / bound ratios it found (MEASURED lines)."""
import ctypes as C

import numpy as np
import pytest

import tnqs_amd as tn
import theta_svd_ref as ref

pytestmark = pytest.mark.gpu
lib = C.CDLL(tn.LIB_PATH)
lib.tnqs_last_error.restype = C.c_char_p


def run(what, items, dtype, dyn, recover_form=0, seed=0):
    L = ref.Launch(items, dtype, dyn, seed=seed)
    rc = L.call(lib, recover_form=recover_form)
    assert rc == 0, lib.tnqs_last_error()
    print(f"routes {what}: " + ", ".join(f"{it.name}={ref.ROUTE_NAME.get(int(r), int(r))}({int(s)} sweeps)" for it, r, s in zip(L.items, L.routes, L.sweeps)))
    res = ref.check_launch(L)
    by_route = {}
    for it, r in zip(L.items, L.routes):
        for line, ratio in res[it.name].items():
            print(f"MEASURED svd_stage {what} item {it.name} [{ref.ROUTE_NAME[int(r)]}] {line}: error / bound = {ratio:.2g}")
            by_route[int(r)] = max(by_route.get(int(r), 0.0), ratio)
    for r, w in sorted(by_route.items()):
        print(f"MEASURED svd_stage {what} route {ref.ROUTE_NAME[r]}: worst error / bound = {w:.2g}")
    return L, res


def signature(L, name):
    i = [it.name for it in L.items].index(name)
    return ref.has_pre_signature(*L.outputs(i), L.items[i].cap)


@pytest.mark.parametrize("recover_form", [0, 1], ids=["recover-engine", "recover-generic"])
def test_dyn_launch_c64(recover_form):
    """the run-ahead regime, ComplexF32: eleven gates offered to theta_svd_pre_kernel, jacobi_lds_kernel<float, 16> (item G's 140 rows pick the instantiation for all) and the
    recovery at once.  A: the low-rank factor, V through Q; B: K <= TNQS_PRE_MIN_COLS, plain Jacobi on 16 x 12 and V recovered with nu = 12 < n = 16; C: the low-rank route
    withdrawn on the device (info[7] = 0 with Q set), theta itself, 20 x 20 inside a slot for 24 x 24; D: the same with 12 columns, declined; E: the pre = 1 offer taken by a
    wide theta stored 80 x 20; F: declined, 60 x 8 with leading dimension 60 inside a slot for 80 x 20; G: beyond the preconditioned kernel's rows; H: rank 3; I*: zero
    thetas on the three routes.  Who ran shows in the capped items: A, C, E carry the preconditioned kernel's unformed columns, B, D, F do not (check_item asserts the
    latter).  recover-generic: the same launch with recover_v_kernel<float, 8>, whose spelling of the predicate the engine runs without the matrix cores"""
    L, res = run(f"dyn c64 recover_form {recover_form}", ref.dyn_f32_items(), 0, 1, recover_form, seed=11)
    for name in ("A", "C", "E"):
        assert signature(L, name) is True, name
    for name in ("B", "D", "F"):
        assert signature(L, name) is False, name
    for it, sw in zip(L.items, L.sweeps):           # every item was factorised by somebody: its sweep count arrived in info[4]
        if it.kind != "zero":
            assert 0 < sw < 60, (it.name, sw)


def test_dyn_launch_c128():
    """the run-ahead regime, ComplexF64 (no preconditioned kernel in double): jacobi_lds_kernel<double, 16> and recover_v_kernel<double, 8> with nu < n (B), ranks below
    the bounds (D, F), a wide theta's leading dimension inside a larger slot (F)"""
    L, res = run("dyn c128", ref.dyn_f64_items(), 1, 1, seed=12)
    for name in ("B", "D", "F"):
        assert signature(L, name) is False, name


@pytest.mark.parametrize("dtype,recover_form", [(0, 0), (1, 0), (0, 1)], ids=["c64", "c128", "c64-recover-generic"])
def test_static_launch(dtype, recover_form):
    """the static regime (host dims, the chi = 128 shapes of two_trips at d = 2): 24 x 24; the 24 x 10 factor of a 24 x 24 theta (nu < n); 260 x 12 -- ComplexF32: the tall
    route, whose polishing launch is jacobi_kernel<float, 8> (it runs on the zero item, whose Cholesky pivots are all refused), then the recovery over 260 rows
    (recover_v_mfma_kernel, or recover_v_kernel<float, 8> with recover_form = 1); ComplexF64: jacobi_kernel<double, 8> and rows >= 256 of recover_v_kernel<double, 8>"""
    run(f"static c{64 << dtype} recover_form {recover_form}", ref.static_items(dtype), dtype, 0, recover_form, seed=13 + dtype)


@pytest.mark.parametrize("dtype", [0, 1], ids=["c64", "c128"])
def test_refusals_write_nothing(dtype):
    """dyn = 1 with a bound that fails the one_trip rule (260 rows); d^2 chi beyond 512: TNQS_ERR_UNSUPPORTED, and no array is touched"""
    for items, dyn in (([ref.Item("24x24", 12, 12), ref.Item("260x12", 130, 6)], 1), ([ref.Item("516", 4, 4, n1=258, n2=4)], 0), ([ref.Item("516", 4, 4, n1=258, n2=4)], 1)):
        L = ref.Launch(items, dtype, dyn)
        assert L.call(lib) == ref.ERR_UNSUPPORTED, lib.tnqs_last_error()
        assert np.array_equal(L.theta, L.theta_in) and np.array_equal(L.theta0, L.theta0_in) and np.array_equal(L.thetaV, L.thetaV_in)
        assert np.all(L.sweeps == -1) and np.all(L.routes == 0)
