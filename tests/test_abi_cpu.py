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
    """the kernel-level entry points of include/tnqs_debug.h (tests/test_gpu_kernels.py reaches every kernel through them): each declaration has its export"""
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
            "tnqs_dbg_inner_scalar", "tnqs_dbg_theta_svd_stage"} <= decl
    for name in sorted(decl):
        assert hasattr(lib, name), f"{name} declared in include/tnqs_debug.h but not exported"


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
