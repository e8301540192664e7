"""The references and the planner restatement of tests/plane32_ref.py, without a GPU: the references against an independent einsum of the full contraction, the
engine's plan functions (read through the host-only mode of tnqs_dbg_pair32 / tnqs_dbg_pair_gram32) against the restated rules on every item list, forced spw and
form, the invariants the kernels rely on, the known values of the 20 x 20 and 7 x 7 lattices, and the room the bounds leave: plain complex64 numpy on the same inputs
stays under half of each."""
import os
import subprocess
import sys

import numpy as np
import pytest

import plane32_ref as R

NO_X3 = os.environ.get("TNQS_NO_BF16X3") == "1"          # the library reads the switch once per process: the f32 rules are read in a child (test_planner_under_the_f32_switch)
BULK_ITEM = ((32, 32, 32, 32), 2, 1)
# the lists of the GPU tests, the two lattices' bulk levels, and launches whose slice totals give the f32 one-message rule 5, 6 and 7 slices per workgroup
PLAN_LISTS = {"MIXED": R.MIXED, "BULK": R.BULK, "LEVEL": [(c, r, jo) for c, _, (r, jo) in R.LEVEL], "L7": [BULK_ITEM] * 25, "L20": [BULK_ITEM] * 324,
              "f32spw5": [BULK_ITEM] * 80 + R.MIXED, "f32spw6": [BULK_ITEM] * 100, "f32spw7": [BULK_ITEM] * 112 + R.BULK, "odd": R.MIXED[:3] * 37}
FORCED = {"pair": (0, 1, 5, 16), "gram2": (0, 2, 5, 16), "gram1": (0, 4, 5, 16)}


def host_plan(kind, items, spw):
    res = R.run_pair32(items, spw=spw) if kind == "pair" else R.run_pair_gram32(items, 0 if kind == "gram2" else 1, spw=spw)
    assert res["rc"] == 0, res["err"]
    return res


def test_references_against_an_independent_einsum():
    """absorb / pair_product / pair_gram (tensordot + moveaxis) against one einsum over the whole contraction, on a leg-0 item with lx > ly and on a contiguous one"""
    rng = np.random.default_rng(5)
    for (chi, lx, ly), sub in [(((32, 2, 32), 2, 0), "sabc"), (((4, 32, 32), 1, 2), "sabc")]:
        t = R.tensor(R.rnd(rng, 2 * int(np.prod(chi))), chi); y = R.tensor(R.rnd(rng, t.size), chi)
        Mx, My = R.matrix(R.rnd(rng, 1024)), R.matrix(R.rnd(rng, 1024))
        L = {0: "a", 1: "b", 2: "c"}; x_, y_ = L[lx], L[ly]
        out = sub.replace(x_, "X").replace(y_, "Y")
        ref = np.einsum(f"{sub},{x_}X,{y_}Y->{out}", t, Mx, My)
        assert np.allclose(R.pair_product(t, Mx, My, lx, ly), ref, rtol=0, atol=1e-11 * np.max(np.abs(ref)))
        # Gram keeping ly with lx absorbed: G[Y, Z] = sum t[.. x .. Y ..] Mx[x, X] conj(y[.. X .. Z ..])
        ysub = sub.replace(x_, "X").replace(y_, "Z"); tsub = sub.replace(y_, "Y")
        ref = np.einsum(f"{tsub},{x_}X,{ysub}->YZ", t, Mx, y.conj())
        assert np.allclose(R.pair_gram(t, y, Mx, lx, ly), ref, rtol=0, atol=1e-11 * np.max(np.abs(ref)))
        # device layouts: tensor() reads the column-major array, the site index fastest
        flat = R.rnd(rng, 2 * int(np.prod(chi)))
        assert R.tensor(flat, chi)[1, 3, 1, 2] == flat[1 + 2 * (3 + chi[0] * (1 + chi[1] * 2))]
        m = R.rnd(rng, 1024)
        assert R.matrix(m)[3, 5] == m[3 + 32 * 5]


def test_geometry_restatement():
    """slices = elements / (16 x 1024) on every covered item; the refused shapes are not covered"""
    for items in list(R.LISTS.values()) + [PLAN_LISTS["LEVEL"]]:
        for it in items:
            assert R.slices(it) * 16 * 1024 == 2 * int(np.prod(it[0])), it
    assert [R.slices(it) for it in R.MIXED] == [1, 1, 4, 4, 16, 32, 16, 128]
    assert [R.slices(it) for it in R.BULK] == [128, 128, 4, 4]
    assert R.geometry(*R.MIXED[4]) == (4, 4, 1) and R.geometry(*R.MIXED[5]) == (1, 32, 1) and R.geometry(*R.MIXED[6]) == (4, 1, 4) and R.geometry(*R.MIXED[3]) == (2, 2, 1)
    for it in R.REFUSED:
        assert R.geometry(*it) is None, it


@pytest.mark.parametrize("kind", ["pair", "gram2", "gram1"])
@pytest.mark.parametrize("name", sorted(PLAN_LISTS))
def test_planner_against_the_restatement(kind, name):
    """the engine's plan function = the restated rule, for the engine's own spw and each forced one; and what the kernels rely on: wg_begin a multiple of the group (16;
    32 on the f32 both-messages kernel), the workgroups add up, and the groups' slice ranges cover every slice"""
    items = PLAN_LISTS[name]; sl = [R.slices(it) for it in items]
    for spw in FORCED[kind]:
        res = host_plan(kind, items, spw)
        assert res["route"] == (R.ROUTE_F32 if NO_X3 else R.ROUTE_X3)
        want_spw, begin, nwg, total = R.expected_plan(kind, res["route"], sl, spw)
        assert (res["spw"], res["begin"], res["nwg"], res["total"]) == (want_spw, begin, nwg, total), (name, kind, spw)
        assert spw <= 0 or res["spw"] == spw
        assert sum(res["nwg"]) == res["total"] and res["begin"][0] == 0
        assert all(b1 == b0 + n for b0, b1, n in zip(res["begin"], res["begin"][1:], res["nwg"]))
        if kind == "gram1" and res["route"] == R.ROUTE_F32:                  # one workgroup per slice range
            assert all(n * res["spw"] >= s > (n - 1) * res["spw"] for n, s in zip(res["nwg"], sl))
            continue
        group = 32 if (kind == "gram2" and res["route"] == R.ROUTE_F32) else 16
        assert all(b % group == 0 and n % group == 0 and n > 0 for b, n in zip(res["begin"], res["nwg"]))
        assert all(8 * (n // group) * res["spw"] >= s for n, s in zip(res["nwg"], sl))      # 8 slice ranges per group: no slice is left out


@pytest.mark.skipif(NO_X3, reason="values of the bf16 route")
def test_known_values_of_the_lattices():
    """the bulk of a 20 x 20 lattice (324 sites) and of a 7 x 7 one (25)"""
    for n, spw, per_item in [(324, 16, 16), (25, 4, 64)]:
        res = host_plan("pair", [BULK_ITEM] * n, 0)
        assert res["spw"] == spw and res["nwg"] == [per_item] * n and res["total"] == per_item * n
    assert host_plan("gram2", [BULK_ITEM] * 324, 0)["spw"] == 16
    assert host_plan("gram1", [BULK_ITEM] * 4, 0)["spw"] == 1


def test_f32_rule_values():
    """the f32 one-message rule really gives 4, 5, 6, 7 and 16 slices per workgroup on launches the lists above hold"""
    got = [R.plan_pair_gram([R.slices(it) for it in PLAN_LISTS[k]])[0] for k in ("MIXED", "f32spw5", "f32spw6", "f32spw7", "L20")]
    assert got == [4, 5, 6, 7, 16]


def test_planner_under_the_f32_switch():
    """plan_pair_gram and the 32-workgroup groups of plan_pair_gram2 only apply under TNQS_NO_BF16X3=1, which the library reads once per process: the planner tests run
    again in one child process with the switch set"""
    if NO_X3:
        pytest.skip("this is the child")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "not gpu", os.path.abspath(__file__), "-k", "planner_against", "-p", "no:cacheprovider"],
                       env=dict(os.environ, TNQS_NO_BF16X3="1", PYTHONPATH=os.pathsep.join(sys.path)), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert f"{3 * len(PLAN_LISTS)} passed" in r.stdout and " failed" not in r.stdout


def test_refusals_on_the_host():
    """an uncovered shape is refused before anything else happens, in the host-only mode too"""
    for it in R.REFUSED:
        assert R.run_pair32([R.MIXED[0], it])["rc"] == R.ERR_UNSUPPORTED, it
        for form in (0, 1):
            assert R.run_pair_gram32([R.MIXED[0], it], form)["rc"] == R.ERR_UNSUPPORTED, it


def _c64(a):
    return [np.asarray(x, dtype=np.complex64) for x in a]


@pytest.mark.parametrize("name", sorted(R.LISTS))
def test_bounds_leave_room_for_plain_f32(name):
    """complex64 numpy on the inputs of the GPU tests against the float64 references: under half of each bound on every item, so a kernel over a bound is not f32
    rounding (a lost bf16 piece of an operand is 4e-3, a lost slice far more)"""
    d = R.launch_data(name)
    got = R.references(d["items"], d["X"], d["Y"], d["M"], dt=np.complex64)
    for i, it in enumerate(d["items"]):
        ep = R.rel_err(got["prod"][i], d["prod"][i]); eg = max(R.rel_err(got["gy"][i], d["gy"][i]), R.rel_err(got["gx"][i], d["gx"][i]))
        print(f"MEASURED complex64 numpy {it}: pair product {ep:.2e}, Gram {eg:.2e}")
        assert got["prod"][i].dtype == np.complex64 and got["gy"][i].dtype == np.complex64
        assert ep < 0.5 * R.PAIR_BOUND and eg < 0.5 * R.GRAM_BOUND, (it, ep, eg)


def test_level_bound_leaves_room_for_plain_f32():
    """the level: T rounded to complex64 and the Grams in complex64 stay under half of 3e-6"""
    d = R.level_data()
    got = R.level_reference(d["items"], d["psi"], d["M"], dt=np.complex64)
    for i, it in enumerate(d["items"]):
        e = max(R.rel_err(got["msg_jo"][i], d["msg_jo"][i]), R.rel_err(got["msg_r"][i], d["msg_r"][i]))
        print(f"MEASURED complex64 numpy level {it}: {e:.2e}")
        assert e < 0.5 * R.LEVEL_GRAM_BOUND, (it, e)


def test_scaled_launch_has_one_zero_item():
    d = R.launch_data("MIXED", True)
    zero = [i for i, x in enumerate(d["X"]) if not np.any(x)]
    assert zero == [R.SCALES.index(0.0)] and all(np.any(y) for y in d["Y"])
    i = zero[0]
    assert not np.any(d["prod"][i]) and not np.any(d["gy"][i]) and not np.any(d["gx"][i])
