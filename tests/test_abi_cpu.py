"""CPU-side checks of the drop-in boundary: the C-ABI library loads, exports every symbol include/tnqs.h declares,
and refuses to run without a GPU (no CPU fallback)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "tnqs.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set(re.findall(r"\b(tnqs_[a-z0-9_]+)\s*\(", src))
    names.discard("tnqs_allgatherv_fn")
    return names


def test_library_exports_every_declared_symbol():
    import ctypes
    import tnqs_amd as tn
    lib = ctypes.CDLL(tn.LIB_PATH)
    decl = declared_symbols()
    assert len(decl) >= 20
    for name in sorted(decl):
        assert hasattr(lib, name), f"{name} declared in include/tnqs.h but not exported"
    assert set(tn.EXPORTS) == decl
    assert lib.tnqs_version() >= 100


def test_library_exports_every_declared_debug_symbol():
    """the kernel-level entry points of include/tnqs_debug.h (the GPU tests reach the kernels through them; tests/kernel_coverage.py says which test reaches which
    kernel, and tests/test_kernel_coverage_cpu.py keeps that table complete): each declaration has its export"""
    import ctypes
    import tnqs_amd as tn
    lib = ctypes.CDLL(tn.LIB_PATH)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tnqs_debug.h")).read(), flags=re.S)
    decl = set(re.findall(r"\b(tnqs_dbg_[a-z0-9_]+)\s*\(", src))
    assert {"tnqs_dbg_rowgemm", "tnqs_dbg_gram_mfma", "tnqs_dbg_pair16", "tnqs_dbg_pair_gram2x16", "tnqs_dbg_svd_tall", "tnqs_dbg_fiber_gemm",
            "tnqs_dbg_small_site", "tnqs_dbg_msg_finalize", "tnqs_dbg_msg_rescale", "tnqs_dbg_edge_scalar", "tnqs_dbg_env_prepare", "tnqs_dbg_env_finish",
            "tnqs_dbg_symg_build", "tnqs_dbg_symg_finish", "tnqs_dbg_diag", "tnqs_dbg_cscale", "tnqs_dbg_fiber_plan",
            "tnqs_dbg_operator_sum", "tnqs_dbg_gate_theta", "tnqs_dbg_gate_finish", "tnqs_dbg_qr2", "tnqs_dbg_small_svd",
            "tnqs_dbg_site_prob", "tnqs_dbg_site_draw", "tnqs_dbg_site_project", "tnqs_dbg_site1", "tnqs_dbg_norm_factor", "tnqs_dbg_scale",
            "tnqs_dbg_inner_scalar", "tnqs_dbg_theta_svd_stage", "tnqs_dbg_fiber_pass_c128", "tnqs_dbg_gram_c128", "tnqs_dbg_gram_route",
            "tnqs_dbg_permute", "tnqs_dbg_random_fill", "tnqs_dbg_identity", "tnqs_dbg_sum_doubles", "tnqs_dbg_record_pack", "tnqs_dbg_copy_items",
            "tnqs_dbg_loop_dot", "tnqs_dbg_bmps_norm", "tnqs_dbg_amp_sweep_end", "tnqs_dbg_amp_scalar"} <= decl
    for name in sorted(decl):
        assert hasattr(lib, name), f"{name} declared in include/tnqs_debug.h but not exported"


def declared_debug_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tnqs_debug.h")).read(), flags=re.S)
    return set(re.findall(r"\b(tnqs_dbg_[a-z0-9_]+)\s*\(", src))


def test_library_exports_nothing_but_the_declared_symbols():
    """the other direction: every tnqs_* function the library defines is declared in include/tnqs.h or include/tnqs_debug.h, so a leftover or misspelt definition of
    an entry point (each is defined in one place, checked against its header by the compiler) does not go unnoticed"""
    import subprocess
    import tnqs_amd as tn
    out = subprocess.run(["nm", "-D", "--defined-only", tn.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (tnqs_\w+)$", out, flags=re.M))
    decl = declared_symbols() | declared_debug_symbols()
    assert len(exported) >= 100
    assert exported == decl, (sorted(exported - decl), sorted(decl - exported))


def test_one_error_string_for_every_translation_unit():
    """the entry points of include/tnqs.h and include/tnqs_debug.h are defined in different source files and share ONE thread-local error string: tnqs_last_error()
    returns the message of the call that failed last on this thread, whichever file defines it"""
    import ctypes
    import tnqs_amd as tn
    lib = ctypes.CDLL(tn.LIB_PATH)
    lib.tnqs_last_error.restype = ctypes.c_char_p
    INVALID, HIP = -1, -3      # TNQS_ERR_INVALID, TNQS_ERR_HIP (include/tnqs.h)
    shape = (ctypes.c_int * 6)(2, 4, 4, 4, 2, 4)
    nlaunches = ctypes.c_int(-7)
    rc = lib.tnqs_dbg_fiber_plan(3, 0, 1, 1, 1, shape, None, 0, ctypes.byref(nlaunches), None)      # use = 3: a host-only debug entry with a bad argument
    assert rc == INVALID and nlaunches.value == -7
    assert lib.tnqs_last_error() == b"tnqs_dbg_fiber_plan: bad arguments"
    dtype = ctypes.c_int(-7)
    rc = lib.tnqs_scalartype(None, ctypes.byref(dtype))      # an entry of include/tnqs.h replaces the message
    assert rc == INVALID and dtype.value == -7
    assert lib.tnqs_last_error() == b"null handle"
    count = ctypes.c_int(0)
    assert lib.tnqs_device_count(ctypes.byref(count)) == 0
    assert lib.tnqs_last_error() == b"null handle"      # a call that succeeds leaves it alone
    if count.value == 0:      # a device entry without a device: the refusal comes from the debug layer's own check
        chi = (ctypes.c_int * 1)(2)
        S = (ctypes.c_double * 2)(1.0, 2.0)
        out = (ctypes.c_float * 8)()
        rc = lib.tnqs_dbg_diag(0, 1, chi, S, out, 0)
        assert rc == HIP
        assert b"no HIP device available" in lib.tnqs_last_error()
        assert not any(out)


def test_no_cpu_fallback():
    import torch
    import tnqs_amd as tn
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    g = tn.named_grid((2, 2))
    psi = tn.tensornetworkstate(np.complex64, lambda v: "↑", g)
    with pytest.raises(tn.TnqsError, match="no HIP device"):
        tn.BeliefPropagationCache(psi)


def test_product_package_does_not_import_oracle():
    pkg = os.path.join(ROOT, "tensornetworkquantumsimulator.jl_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".hpp", ".h")):
                txt = open(os.path.join(dp, f), errors="replace").read()
                assert "tnqs_oracle" not in txt and "import statevector" not in txt and "oracle/" not in txt, f


def test_c_driver_compiles_against_the_abi_and_fails_loudly_without_a_gpu(tmp_path):
    """examples/c_driver.c (plain C, gcc) links against libtnqs_hip.so through include/tnqs.h alone; without a GPU the library
    refuses to run (no CPU fallback) and the driver reports the library's error string"""
    import subprocess
    import torch
    exe = str(tmp_path / "c_driver")
    pkg = os.path.join(ROOT, "tensornetworkquantumsimulator.jl_amd")
    r = subprocess.run(["gcc", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_driver.c"), "-o", exe,
                        "-L" + pkg, "-ltnqs_hip", "-lm", "-Wl,-rpath," + pkg], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if torch.cuda.is_available():
        pytest.skip("GPU present: the run itself is covered by tests/test_gpu_parity.py")
    p = subprocess.run([exe, "3", "2"], capture_output=True, text=True)
    assert p.returncode == 1 and "no HIP device" in p.stderr
