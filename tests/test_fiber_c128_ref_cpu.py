"""The references, bounds and case lists of tests/fiber_c128_ref.py, checked on the CPU: the float64 references follow the layout formulas of include/tnqs_debug.h, the
derived bounds are neither vacuous nor too tight at the shapes the GPU test runs (numpy's own complex128 result against an np.clongdouble evaluation stays inside them; a
result with an operand rounded to complex64, with one element moved by 1e-12 absprod, with X transposed or with two items' outputs swapped is outside), the case lists cover
what they claim, and -- through the HOST ONLY modes of tnqs_dbg_fiber_pass_c128 / tnqs_dbg_gram_c128 -- every case selects the route and the instantiation it is named for."""
import numpy as np
import pytest

import fiber_c128_ref as R

LD = np.clongdouble
# one representative launch per item list (the tpw / scale / chunk variants share their items)
FIBER_LISTS = sorted(n for n, c in R.FIBER_CASES.items() if c["scale"] == 1.0 and c["tpw"] == 0 and c["mfma"] == 1)
GRAM_LISTS = ["same_chunks3", "none_chunks3", "mixed_chunks3", "fallback_kk3", "fallback_kk66"]


def test_references_follow_the_layout_formulas():
    """element by element from the index formulas, on items with D = 3 and with every dimension different"""
    rng = np.random.default_rng(1)
    for item in [(3, 5, 4, 6, 3, 2), (2, 3, 7, 2, 1, 5), (1, 2, 3, 5, 2, 4)]:
        D, PA, K, PB, Do, No = item
        nin, nx, nout = R.fiber_sizes(item)
        x, X = R.rnd(rng, nin), R.rnd(rng, nx)
        ref = np.zeros(nout, dtype=complex); ab = np.zeros(nout)
        for b in range(PB):
            for a in range(PA):
                for n in range(No):
                    for sp in range(Do):
                        for k in range(K):
                            for s in range(D):
                                xi, Xi = x[s + D * (a + PA * (k + K * b))], X[(s + D * k) + D * K * (sp + Do * n)]
                                o = sp + Do * (a + PA * (n + No * b))
                                ref[o] += xi * Xi; ab[o] += abs(xi) * abs(Xi)
        r, A = R.fiber_ref(item, x, X)
        assert np.allclose(r, ref, rtol=1e-13, atol=0) and np.allclose(A, ab, rtol=1e-13, atol=0)
    for item in [(3, 2, 5, 3), (2, 3, 2, 4), (1, 4, 3, 2)]:
        D, PA, K, PB = item
        KK = D * K
        x, y = R.rnd(rng, R.gram_sizes(item)[0]), R.rnd(rng, R.gram_sizes(item)[0])
        ref = np.zeros(KK * KK, dtype=complex); ab = np.zeros(KK * KK)
        for b in range(PB):
            for a in range(PA):
                for k in range(K):
                    for s in range(D):
                        for k2 in range(K):
                            for s2 in range(D):
                                xi, yi = x[s + D * (a + PA * (k + K * b))], y[s2 + D * (a + PA * (k2 + K * b))]
                                o = (s + D * k) + KK * (s2 + D * k2)
                                ref[o] += xi * np.conj(yi); ab[o] += abs(xi) * abs(yi)
        r, A = R.gram_ref(item, x, y)
        assert np.allclose(r, ref, rtol=1e-13, atol=0) and np.allclose(A, ab, rtol=1e-13, atol=0)


def to_c64(a):
    return a.astype(np.complex64).astype(np.complex128)


def moved(ref, absprod, where):
    out = ref.copy(); out[where] += 1e-12 * absprod[where]
    return out


@pytest.mark.parametrize("name", FIBER_LISTS)
def test_product_bounds_hold_and_bite(name):
    c = R.FIBER_CASES[name]
    ins, Xs, refs = R.fiber_data(name)
    flat_ref, flat_bound = np.concatenate([r for r, _ in refs]), np.concatenate([R.fiber_bound(it, A) for it, (_, A) in zip(c["items"], refs)])
    for it, x, X, (ref, A) in zip(c["items"], ins, Xs, refs):
        D, PA, K, PB, Do, No = it
        B = R.fiber_bound(it, A)
        exact, A_ld = R.fiber_ref(it, x, X, dt=LD)
        assert np.all(np.abs(ref - exact) <= 0.5 * B.astype(np.longdouble)), it         # the reference's own rounding takes at most its half of the bound
        assert np.all(np.abs(A - A_ld) <= 1e-13 * A_ld)
        assert R.inside(ref, ref, B)
        assert not R.inside(R.fiber_ref(it, to_c64(x), X)[0], ref, B), it
        assert not R.inside(R.fiber_ref(it, x, to_c64(X))[0], ref, B), it
        for where in (0, ref.size // 2, ref.size - 1):
            assert not R.inside(moved(ref, A, where), ref, B), it
        if D * K > 1 and Do * No > 1:                                                    # (a vector is its own transpose in memory)
            Xt = np.ascontiguousarray(X.reshape(Do * No, D * K).T).reshape(-1)           # X read with its two indices exchanged
            assert not R.inside(R.fiber_ref(it, x, Xt)[0], ref, B), it
        # the norm of the item: float64 sum of |ref|^2 against the long double one, and what a complex64 operand does to it
        nwg = R.fiber_tiles(it)
        n_exact = np.sum(np.abs(exact) ** 2)
        assert abs(np.sum(np.abs(ref) ** 2) - n_exact) <= R.norm_bound(it, ref, A, nwg)
        assert abs(np.sum(np.abs(R.fiber_ref(it, to_c64(x), X)[0]) ** 2) - n_exact) > R.norm_bound(it, ref, A, nwg)
    # two items' outputs written into each other's place, as far as the sizes allow
    outs = [r for r, _ in refs]; outs[0], outs[1] = outs[1], outs[0]
    assert not R.inside(np.concatenate(outs), flat_ref, flat_bound)


@pytest.mark.parametrize("name", GRAM_LISTS)
def test_gram_bounds_hold_and_bite(name):
    c = R.GRAM_CASES[name]
    Xs, Ys, refs = R.gram_data(name)
    chunks = [1] * len(c["items"]) if c["route"] == R.GRAM_GENERIC else [n for n, _ in R.gram_chunks(c["items"], c["max_chunks"])]      # (the bound must hold with the fewest chunks)
    bounds = [R.gram_bound(it, A, n) for it, (_, A), n in zip(c["items"], refs, chunks)]
    for it, x, y, s, (ref, A), B in zip(c["items"], Xs, Ys, c["same"], refs, bounds):
        exact, _ = R.gram_ref(it, x, y, dt=LD)
        assert np.all(np.abs(ref - exact) <= 0.5 * B.astype(np.longdouble)), it
        assert B.max() < 1e-12 * A.max()
        assert not R.inside(R.gram_ref(it, to_c64(x), to_c64(x) if s else y)[0], ref, B), it
        for where in (0, ref.size // 2, ref.size - 1):
            assert not R.inside(moved(ref, A, where), ref, B), it
        KK = it[0] * it[2]
        if not s:
            assert not R.inside(ref.reshape(KK, KK).T.reshape(-1), ref, B), it           # the transpose: X and Y exchanged without the conjugate
        assert not R.inside(ref.conj(), ref, B), it                                     # out^H of the transpose: the mirror written without its conjugation
    outs = [r for r, _ in refs]; outs[0], outs[1] = outs[1], outs[0]
    assert not R.inside(np.concatenate(outs), np.concatenate([r for r, _ in refs]), np.concatenate(bounds))


def test_case_lists_cover_what_they_claim():
    F = R.FIBER_CASES
    # one launch per (Kmax class, Nmax class, form): 18 instantiations, each launch with the 40-tile item, the ragged one, the smallest and PA = 48 / PB = 1
    assert {F[n]["inst"] for n in F if F[n]["route"] != R.FIBER_GENERIC} == {(nb, ks, g) for nb in (1, 2, 4) for ks in (4, 8, 16) for g in (0, 1)}
    for Kc in R.CLASSES:
        for Nc in R.CLASSES:
            for form, D in (("plain", 1), ("general", 2)):
                c = F[f"{form}_k{Kc}_n{Nc}"]; items = c["items"]
                assert c["inst"] == (R.INST[Nc][0], R.INST[Kc][1], int(D == 2))
                assert max(i[0] * i[2] for i in items) == Kc and max(i[4] * i[5] for i in items) == Nc
                assert items[0][0] == D and items[0][0] * items[0][2] == Kc and items[0][4] * items[0][5] == Nc and R.fiber_tiles(items[0]) == 40
                assert any((i[0] * i[2]) % 4 and (i[4] * i[5]) % 16 and i[1] == 3 and i[3] == 11 and i[0] == D for i in items)
                assert any(i[0] * i[2] == 4 and i[4] * i[5] == 1 and i[1] == 1 and i[3] == 40 for i in items)
                assert any(i[1] == 48 and i[3] == 1 for i in items)
                if D == 1:
                    assert sum(i[2] == i[5] for i in items) <= 1 and all(w == 0 for w in c["want"])
                else:
                    assert any(i[0] == 2 and i[2] % 2 == 1 and i[1] == 3 for i in items) and 0 < sum(c["want"]) < len(items)
    assert (3, 5, 4, 6, 3, 2) in F["general_k16_n16"]["items"]
    for form in ("plain_k32_n32", "general_k64_n16"):
        assert all(f"{form}_tpw{t}" in F for t in (1, 5, 20))
    for n in ("fallback_plain_kk3", "fallback_plain_k65", "fallback_general_kk66", "fallback_plain_no_mfma", "fallback_general_no_mfma"):
        assert F[n]["route"] == R.FIBER_GENERIC
    assert any(i[0] * i[2] == 3 for i in F["fallback_plain_kk3"]["items"]) and any(i[2] == 65 for i in F["fallback_plain_k65"]["items"])
    assert max(i[0] * i[2] for i in F["fallback_general_kk66"]["items"]) == 66
    # Grams: the KK list, D and PA; every launch has nb = 1 .. 4; chunks of exactly 1 tile, exactly 2 and 5 or more occur
    G = R.GRAM_CASES
    every = R.GRAM_SAME + R.GRAM_NONE + R.GRAM_MIXED
    assert {4, 5, 15, 16, 17, 31, 32, 33, 48, 63, 64} <= {i[0] * i[2] for i in every} and (3, 3, 5, 11) in every
    assert {i[0] for i in every} == {1, 2, 3} and {i[1] for i in every} == {1, 3, 20, 32, 33}
    for items in (R.GRAM_SAME, R.GRAM_NONE, R.GRAM_MIXED):
        assert {(i[0] * i[2] + 15) // 16 for i in items} == {1, 2, 3, 4}
        assert any(R.gram_tiles(i) * 32 != i[1] * i[3] for i in items)                     # ragged tiles
    assert {(G["mixed_chunks0"]["same"][k], (i[0] * i[2] + 15) // 16) for k, i in enumerate(R.GRAM_MIXED)} >= {(1, 1), (1, 3), (0, 2), (0, 4)}
    tpcs = {tpc for mc in (0, 1, 3) for items in (R.GRAM_SAME, R.GRAM_NONE, R.GRAM_MIXED) for _, tpc in R.gram_chunks(items, mc)}
    assert 1 in tpcs and 2 in tpcs and any(t >= 5 for t in tpcs)
    assert any(i[0] * i[2] == 3 for i in G["fallback_kk3"]["items"]) and any(i[0] * i[2] == 66 for i in G["fallback_kk66"]["items"]) and G["fallback_no_mfma"]["mfma"] == 0


def expected_fiber_route(c):
    """the route rule of a ComplexF64 pass, stated from DESIGN.md ("Fiber GEMM routes"): chain -- every item 4 <= D K <= 64 and Do No <= 64; epilogue -- the maxima"""
    kk = [i[0] * i[2] for i in c["items"]]; nn = [i[4] * i[5] for i in c["items"]]
    if not c["mfma"]:
        return R.FIBER_GENERIC
    if c["use"] == R.CHAIN:
        return R.FIBER_F64_PLAIN if all(4 <= k <= 64 and n <= 64 for k, n in zip(kk, nn)) else R.FIBER_GENERIC
    return R.FIBER_F64_GENERAL if 4 <= max(kk) <= 64 and max(nn) <= 64 else R.FIBER_GENERIC


@pytest.mark.parametrize("name", sorted(R.FIBER_CASES))
def test_host_only_fiber_pass_selects_what_the_case_is_named_for(name):
    c = R.FIBER_CASES[name]
    res = R.run_fiber_pass(name, host_only=True)
    assert res["rc"] == 0, res["err"]
    assert expected_fiber_route(c) == c["route"]
    assert res["route"] == c["route"] and res["inst"] == c["inst"]
    begin, nwg = res["begin"], res["nwg"]
    assert begin == [sum(nwg[:i]) for i in range(len(nwg))] and min(nwg) >= 1
    if c["route"] != R.FIBER_GENERIC:
        tpw = c["tpw"] or (8 if c["use"] == R.CHAIN else 32)
        assert nwg == [-(-R.fiber_tiles(i) // tpw) for i in c["items"]]


@pytest.mark.parametrize("name", sorted(R.GRAM_CASES))
def test_host_only_gram_selects_what_the_case_is_named_for(name):
    c = R.GRAM_CASES[name]
    res = R.run_gram(name, host_only=True)
    assert res["rc"] == 0, res["err"]
    covered = c["mfma"] and all(4 <= i[0] * i[2] <= 64 for i in c["items"])
    assert res["route"] == c["route"] == (R.GRAM_F64IN if covered else R.GRAM_GENERIC)
    if covered:
        assert res["nchunks"] == [n for n, _ in R.gram_chunks(c["items"], c["max_chunks"])]
    else:
        assert min(res["nchunks"]) >= 1


def test_entries_refuse_what_the_engine_never_launches():
    """a chain stage has no site index and no norm: the plain kernel would ignore both, so the entry refuses them instead of computing something else"""
    import ctypes as C
    lib, IP, VP = R._entries()
    for shape, want in (((2, 4, 4, 4, 2, 4), 0), ((1, 4, 4, 4, 1, 4), 1)):
        s = (C.c_int * 6)(*shape); w = (C.c_int * 1)(want); route = C.c_int(-7)
        assert lib.tnqs_dbg_fiber_pass_c128(0, 1, 1, s, w, None, None, None, None, 0, 0, C.byref(route), None, None, None) == -1 and route.value == -7
