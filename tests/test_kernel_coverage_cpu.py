"""The kernel-to-test table of tests/kernel_coverage.py has to stay full: every __global__ function of the package's csrc/*.hip has a row, every row names an entry
point that a header declares and a test file that exists and calls it."""
import glob
import os
import re

import kernel_coverage as cov

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tensornetworkquantumsimulator.jl_amd", "csrc")


def _without_comments(src):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


def global_kernels():
    """name -> source file of every __global__ function (templates once), attributes between __global__ and void allowed"""
    out = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        src = _without_comments(open(path).read())
        names = re.findall(r"__global__[^;{}]*?\bvoid\s+(\w+)\s*\(", src)
        assert len(names) == src.count("__global__"), path          # nothing the pattern does not understand
        for n in names:
            assert n not in out, n
            out[n] = os.path.basename(path)
    return out


def declared(header):
    src = _without_comments(open(os.path.join(ROOT, "include", header)).read())
    return set(re.findall(r"\b(tnqs_[a-z0-9_]+)\s*\(", src))


def test_every_kernel_has_a_row_and_every_row_a_kernel():
    kernels = global_kernels()
    assert len(kernels) >= 90
    missing, stale = sorted(set(kernels) - set(cov.COVERAGE)), sorted(set(cov.COVERAGE) - set(kernels))
    assert not missing, f"kernels without a row in tests/kernel_coverage.py: {[(k, kernels[k]) for k in missing]}"
    assert not stale, f"rows of tests/kernel_coverage.py without a kernel: {stale}"


def test_every_row_names_a_declared_entry_point_and_a_test_that_calls_it():
    names = declared("tnqs_debug.h") | declared("tnqs.h")
    texts = {}
    for kernel, (entry, test_file) in cov.COVERAGE.items():
        path = os.path.join(ROOT, test_file)
        assert os.path.isfile(path), (kernel, test_file)
        assert os.path.basename(test_file).startswith("test_gpu_"), (kernel, test_file)
        if entry == cov.END_TO_END:
            continue
        assert entry in names, f"{kernel}: {entry} is declared in neither header"
        if path not in texts:
            texts[path] = open(path).read()
        assert re.search(r"\b" + re.escape(entry) + r"\b", texts[path]), f"{kernel}: {test_file} does not mention {entry}"


def test_end_to_end_rows_are_listed_as_open():
    """a row marked end to end is a gap: DESIGN.md has to say so"""
    open_rows = sorted(k for k, (entry, _) in cov.COVERAGE.items() if entry == cov.END_TO_END)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for k in open_rows:
        assert k in design, f"{k} is covered end to end only and DESIGN.md does not list it as open"
