"""The two ComplexF64 matrix-core kernels of csrc/kernels_f64.hip -- mfma_fiber_gemm_f64_kernel<NBLK, KS, GEN> and mfma_gram_f64in_kernel -- launched as the engine launches
them (tnqs_dbg_fiber_pass_c128, tnqs_dbg_gram_c128: several items of different sizes in ONE launch, planned by plan_fiber_pass / gram_route + plan_gram) against the float64
references of tests/fiber_c128_ref.py, within the derived bounds stated there (checked on the CPU by tests/test_fiber_c128_ref_cpu.py).  Every test asserts the route -- and
the instantiation -- the entry reports BEFORE it looks at a number: a launch that falls back to the vector kernel fails its test instead of passing on another kernel.
The outputs go up filled with NaN between guard bands, the norm partials with a marker, so an element nobody wrote, a write outside an item and a norm slot written for an
item that wants none all show."""
import numpy as np
import pytest

import fiber_c128_ref as R

pytestmark = pytest.mark.gpu
ERR_HIP = -3      # TNQS_ERR_HIP (include/tnqs.h)


def device_ok(res):
    """a HIP error leaves the process's device context unusable: nothing that follows in this session would mean anything, so the session ends there"""
    if res["rc"] == ERR_HIP:
        pytest.exit(f"HIP error in a kernel-level entry point: {res['err']}", returncode=3)


@pytest.mark.parametrize("name", sorted(R.FIBER_CASES))
def test_fiber_pass(name):
    """one launch per (Kmax class, Nmax class, form) = all 18 instantiations, each with the 40-tile item, a ragged item, the smallest item and PA = 48 / PB = 1; forced tiles
    per workgroup (20: the prefetch loop past its first swap); scales 1e-100, 1e100 and an exact zero; the launches that fall back to fiber_gemm_kernel<double, 8>"""
    c = R.FIBER_CASES[name]
    res = R.run_fiber_pass(name)
    device_ok(res)
    assert res["rc"] == 0, res["err"]
    assert res["route"] == c["route"] and res["inst"] == c["inst"], (res["route"], res["inst"])
    assert R.bands_intact(res["out"], res["out_slices"], res["out_before"])
    assert R.bands_intact(res["partials"], [res["partials_slice"]], res["partials_before"])
    _, _, refs = R.fiber_data(name)
    part = res["partials"][res["partials_slice"]]
    assert part.size == sum(res["nwg"])
    for i, (it, out, (ref, A)) in enumerate(zip(c["items"], res["outs"], refs)):
        B = R.fiber_bound(it, A)
        assert not np.any(np.isnan(out.view(np.float64))), (it, "unwritten output elements")
        err = np.abs(out - ref)
        print(name, it, "max |out - ref| / bound =", float(np.max(err / np.where(B > 0, B, 1.0))))
        assert R.inside(out, ref, B), it
        slots = part[res["begin"][i]:res["begin"][i] + res["nwg"][i]]
        if c["scale"] == 0.0:
            assert np.all(out == 0), it
        if c["want"][i]:
            n_ref = float(np.sum(np.abs(ref) ** 2)); nb = R.norm_bound(it, ref, A, res["nwg"][i])
            print(name, it, "|norm - ref| / bound =", abs(float(np.sum(slots)) - n_ref) / nb if nb > 0 else 0.0)
            assert abs(float(np.sum(slots)) - n_ref) <= nb, it
            if c["scale"] == 0.0:
                assert np.all(slots == 0), it
        else:
            assert np.all(slots == R.PART_FILL), (it, "norm partials of an item that wants no norm")


@pytest.mark.parametrize("name", sorted(R.GRAM_CASES))
def test_gram(name):
    """launches with every item X == Y (upper block triangle + mirror: 1, 3, 6, 10 blocks), with none (all 16 blocks) and mixed, nb = 1 .. 4 in each; the engine's chunking,
    one chunk and three chunks per item (chunks of 1 tile, of 2 and of 5 or more: each branch of the double buffer); scales; the launches that fall back to
    gram_kernel<double, double, 4>"""
    c = R.GRAM_CASES[name]
    res = R.run_gram(name)
    device_ok(res)
    assert res["rc"] == 0, res["err"]
    assert res["route"] == c["route"], res["route"]
    assert R.bands_intact(res["out"], res["out_slices"], res["out_before"])
    _, _, refs = R.gram_data(name)
    for it, s, out, (ref, A), nch in zip(c["items"], c["same"], res["outs"], refs, res["nchunks"]):
        B = R.gram_bound(it, A, nch)
        assert not np.any(np.isnan(out.view(np.float64))), (it, "unwritten output elements")
        err = np.abs(out - ref)
        print(name, it, "chunks", nch, "max |out - ref| / bound =", float(np.max(err / np.where(B > 0, B, 1.0))))
        assert R.inside(out, ref, B), it
        if s:
            KK = it[0] * it[2]
            G, Bm = out.reshape(KK, KK), B.reshape(KK, KK)
            assert np.all(np.abs(G - G.conj().T) <= Bm + Bm.T), (it, "out is not Hermitian within the bound")
        if c["scale"] == 0.0:
            assert np.all(out == 0), it
