"""The chi = 32 plane kernels as the engine launches them (tnqs_dbg_pair32, tnqs_dbg_pair_gram32: ONE launch over items of different geometry, planned by the engine's
plan_* functions and launched by its launch_* functions) against the float64 references of tests/plane32_ref.py:
  pair product          x3_pair_kernel                 (mfma_pair_kernel under TNQS_NO_BF16X3=1)
  both messages         x3_pair_gram2_kernel<false>    (mfma_pair_gram2_kernel)
  one message           x3_pair_gram2_kernel<true>     (mfma_pair_gram_kernel)
Every test asserts the route the entry point reports before it looks at a number.  Outputs go up NaN-filled between NaN guard bands; the Gram partials are NaN-filled and
guarded on the device: an element or a partial nobody wrote, and a write outside an item, all show.  The f32 kernels run in a child process (test_f32_plane_kernel_leg).

Bounds (plane32_ref.py; none tuned to a kernel -- complex64 numpy on the same inputs stays under half of each, tests/test_plane32_ref_cpu.py), relative to the largest
entry of the item's reference: pair product 1e-6, Gram 2e-6, Gram of a product the device rounded to f32 3e-6.  The inputs are seeded and the kernels sum in a fixed
order, so the measured values (MEASURED below, the largest over all cases of this file on the MI355X) repeat."""
import os
import subprocess
import sys

import numpy as np
import pytest

import plane32_ref as R

pytestmark = pytest.mark.gpu
NO_X3 = os.environ.get("TNQS_NO_BF16X3") == "1"          # the library reads the switch once per process
ROUTE = R.ROUTE_F32 if NO_X3 else R.ROUTE_X3
ERR_HIP = -3                                              # TNQS_ERR_HIP (include/tnqs.h)
KERNEL = {("pair", R.ROUTE_X3): "x3_pair_kernel", ("pair", R.ROUTE_F32): "mfma_pair_kernel",
          ("gram2", R.ROUTE_X3): "x3_pair_gram2_kernel<false>", ("gram2", R.ROUTE_F32): "mfma_pair_gram2_kernel",
          ("gram1", R.ROUTE_X3): "x3_pair_gram2_kernel<true>", ("gram1", R.ROUTE_F32): "mfma_pair_gram_kernel"}
# the largest value each kernel printed over all cases of this file on the MI355X, next to its bound (complex64 numpy on the same inputs: 3.0e-7, 6.7e-7, 8.4e-7)
MEASURED = {"x3_pair_kernel": (3.9e-7, R.PAIR_BOUND), "mfma_pair_kernel": (4.2e-7, R.PAIR_BOUND),
            "x3_pair_gram2_kernel<false>": (1.19e-6, R.GRAM_BOUND), "mfma_pair_gram2_kernel": (1.02e-6, R.GRAM_BOUND),      # (both at the 128-slice items)
            "x3_pair_gram2_kernel<true>": (7.7e-7, R.GRAM_BOUND), "mfma_pair_gram_kernel": (9.7e-7, R.GRAM_BOUND),
            "level: x3_pair_gram2_kernel<false>": (7.0e-7, R.LEVEL_GRAM_BOUND), "level: mfma_pair_gram2_kernel": (8.7e-7, R.LEVEL_GRAM_BOUND)}


def device_ok(res):
    """a HIP error leaves the process's device context unusable: nothing that follows in this session would mean anything, so the session ends there"""
    if res["rc"] == ERR_HIP:
        pytest.exit(f"HIP error in a kernel-level entry point: {res['err']}", returncode=3)
    assert res["rc"] == 0, res["err"]
    assert res["route"] == ROUTE, res["route"]


def measured(kind, case, err):
    print(f"MEASURED {KERNEL[(kind, ROUTE)]} route {ROUTE} {case}: {err:.3e}")


def check_plan(kind, res, items, spw):
    """the launch was laid out by the rule (so that the forced spw really is what ran)"""
    want = R.expected_plan(kind, res["route"], [R.slices(it) for it in items], spw)
    assert (res["spw"], res["begin"], res["nwg"], res["total"]) == want


def check_pair(res, items, refs, bound, case):
    assert R.bands_intact(res["out"], res["out_slices"], res["out_before"]), "a write outside an item of out"
    errs = [R.rel_err(o, r) for o, r in zip(res["outs"], refs)]
    for it, e in zip(items, errs):
        measured("pair", f"{case} {it}", e)
    assert all(e < bound for e in errs), errs            # (a NaN -- an element nobody wrote -- fails the comparison)
    return errs


def check_grams(kind, res, items, gy, gx, bound, case):
    assert R.bands_intact(res["out_y"], res["out_slices"], res["out_y_before"]), "a write outside an item of out_y"
    if kind == "gram1":
        assert np.array_equal(res["out_x"].view(np.uint8), res["out_x_before"].view(np.uint8)), "the one-message form wrote out_x"
    else:
        assert R.bands_intact(res["out_x"], res["out_slices"], res["out_x_before"]), "a write outside an item of out_x"
    errs = []
    for i, it in enumerate(items):
        es = [R.rel_err(res["oy"][i], gy[i])] + ([R.rel_err(res["ox"][i], gx[i])] if kind == "gram2" else [])
        e = float("nan") if any(np.isnan(es)) else max(es)
        measured(kind, f"{case} {it}", e)
        errs.append(e)
    assert all(e < bound for e in errs), errs            # (a NaN -- a partial nobody wrote -- fails the comparison)
    return errs


@pytest.mark.parametrize("name", sorted(R.LISTS))
@pytest.mark.parametrize("spw", [0, 1, 5, 16])
def test_pair32_multi_item_launch(name, spw):
    """all items of a list in ONE launch_mfma_pair (find_item over slice_begin): the engine's spw (1 at these sizes), 5 (ragged last ranges, odd range lengths: the
    double-buffer parity and the two staging sets), 16 (one full group for a 128-slice item, padded groups with nothing to do for the rest)"""
    d = R.launch_data(name)
    res = R.run_pair32(d["items"], d["X"], d["M"], spw=spw)
    device_ok(res)
    check_plan("pair", res, d["items"], spw)
    check_pair(res, d["items"], d["prod"], R.PAIR_BOUND, f"{name} spw {spw}")


@pytest.mark.parametrize("name", sorted(R.LISTS))
@pytest.mark.parametrize("spw", [0, 2, 5, 16])
def test_pair_gram32_both_messages(name, spw):
    """form 0: both messages of every item from ONE launch_mfma_pair_gram2, each item's nwg partials per message summed by launch_reduce; a padded group's workgroups
    (s_begin >= s_end) must write zero partials"""
    d = R.launch_data(name)
    res = R.run_pair_gram32(d["items"], 0, d["X"], d["Y"], d["M"], spw=spw)
    device_ok(res)
    check_plan("gram2", res, d["items"], spw)
    check_grams("gram2", res, d["items"], d["gy"], d["gx"], R.GRAM_BOUND, f"{name} spw {spw}")


@pytest.mark.parametrize("name", sorted(R.LISTS))
@pytest.mark.parametrize("spw", [0, 4, 5, 16])
def test_pair_gram32_single_message(name, spw):
    """form 1: one message per item (My = partial_x = null) on the route launch_plane_grams takes; 4 and 5 are values the f32 rule really produces; out_x comes back
    as it went up"""
    d = R.launch_data(name)
    res = R.run_pair_gram32(d["items"], 1, d["X"], d["Y"], d["M"], spw=spw)
    device_ok(res)
    check_plan("gram1", res, d["items"], spw)
    check_grams("gram1", res, d["items"], d["gy"], d["gx"], R.GRAM_BOUND, f"{name} spw {spw}")


def test_plane32_items_of_different_scale_in_one_launch():
    """MIXED with the items scaled by 1, 1e-12, 1e6, 1e-3, 0 (X all zero, Y not), 1e3, 1e-6, 1e-9 in ONE launch of each kernel: the error is per item, relative to that
    item's own largest reference entry (no scaling anywhere: bf16 has the exponent range of f32), and the all-zero item's product and Grams are exactly zero -- a
    neighbour's data leaking in would show.  (1e-36 is outside the documented domain and stays in test_bf16x3_plane_kernels_are_f32_accurate)"""
    d = R.launch_data("MIXED", True)
    zi = R.SCALES.index(0.0)
    tag = [f"scale {s:g}" for s in R.SCALES]
    res = R.run_pair32(d["items"], d["X"], d["M"])
    device_ok(res)
    check_pair(res, list(zip(tag, d["items"])), d["prod"], R.PAIR_BOUND, "scaled")
    assert not np.any(res["outs"][zi])
    for kind, form in (("gram2", 0), ("gram1", 1)):
        res = R.run_pair_gram32(d["items"], form, d["X"], d["Y"], d["M"])
        device_ok(res)
        check_grams(kind, res, list(zip(tag, d["items"])), d["gy"], d["gx"], R.GRAM_BOUND, "scaled")
        assert not np.any(res["oy"][zi]) and (form == 1 or not np.any(res["ox"][zi]))


def test_plane32_level_as_the_engine_runs_it():
    """one BP level as route_pair32 builds it, four items in each launch: T = psi x_pa Ma x_pb Mb (tnqs_dbg_pair32), then both results through the plane (r, jo) from
    (X = T as the device returned it, Y = psi) (form 0), against float64 from psi and the four matrices directly -- the only test where one kernel's output is the other's
    input: it pins lx / ly, Mx / My and partial_y / partial_x between the two kernels against the mathematics.  The two [2][32]^4 items are degree-4 sites (disjoint
    planes: the BP messages through jo and r); a [2][32]^3 site has no two disjoint planes, there r is one of the product's legs (plane32_ref.LEVEL)"""
    d = R.level_data()
    prod_items = [(c, pa, pb) for c, (pa, pb), _ in d["items"]]; gram_items = [(c, r, jo) for c, _, (r, jo) in d["items"]]
    res = R.run_pair32(prod_items, d["psi"], [m[:2048] for m in d["M"]])
    device_ok(res)
    assert R.bands_intact(res["out"], res["out_slices"], res["out_before"])
    T = [np.array(o) for o in res["outs"]]
    assert all(np.all(np.isfinite(t)) for t in T)
    res = R.run_pair_gram32(gram_items, 0, T, d["psi"], [m[2048:] for m in d["M"]])
    device_ok(res)
    check_grams("gram2", res, d["items"], d["msg_jo"], d["msg_r"], R.LEVEL_GRAM_BOUND, "level")


def test_plane32_refuses_what_it_does_not_cover():
    """a 16-dimensional leg in the plane, lx == ly, a lower plane leg above 8 elements without a companion leg, a degree-6 site that needs a fourth slice counter: each
    TNQS_ERR_UNSUPPORTED with the outputs untouched, also as the second item of a launch whose first item is covered"""
    d = R.launch_data("MIXED")
    rng = np.random.default_rng(0)
    for bad in R.REFUSED:
        for items, X, Y, M in (([bad], [], [], []), ([R.MIXED[0], bad], [d["X"][0]], [d["Y"][0]], [d["M"][0]])):
            x = R.rnd(rng, 2 * int(np.prod(bad[0]))); m = R.rnd(rng, 2048)
            res = R.run_pair32(items, X + [x], M + [m])
            assert res["rc"] == R.ERR_UNSUPPORTED, (bad, res["rc"], res["err"])
            assert np.array_equal(res["out"].view(np.uint8), res["out_before"].view(np.uint8))
            for form in (0, 1):
                res = R.run_pair_gram32(items, form, X + [x], Y + [x], M + [m])
                assert res["rc"] == R.ERR_UNSUPPORTED, (bad, form, res["rc"], res["err"])
                assert np.array_equal(res["out_y"].view(np.uint8), res["out_y_before"].view(np.uint8))
                assert np.array_equal(res["out_x"].view(np.uint8), res["out_x_before"].view(np.uint8))


def test_f32_plane_kernel_leg():
    """mfma_pair_kernel, mfma_pair_gram2_kernel and mfma_pair_gram_kernel only run under TNQS_NO_BF16X3=1 (the fallback, and the A/B leg of the benchmark), which the
    library reads once per process: this file runs again in ONE fresh child process with the switch set; every test there asserts ROUTE_F32 and holds the same bounds"""
    if NO_X3:
        pytest.skip("this is the child")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-s", "-m", "gpu", os.path.abspath(__file__), "-p", "no:cacheprovider"],
                       env=dict(os.environ, TNQS_NO_BF16X3="1", PYTHONPATH=os.pathsep.join(sys.path)), capture_output=True, text=True, timeout=900)
    lines = [l[l.index("MEASURED"):] for l in r.stdout.splitlines() if "MEASURED" in l]
    print("\n".join(lines))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "27 passed, 1 skipped" in r.stdout and " failed" not in r.stdout, r.stdout[-1000:]
    assert lines and all(f" route {R.ROUTE_F32} " in l for l in lines)
    assert {l.split()[1] for l in lines} == {"mfma_pair_kernel", "mfma_pair_gram2_kernel", "mfma_pair_gram_kernel"}
