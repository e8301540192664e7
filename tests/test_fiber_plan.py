"""Which fiber GEMM kernel a pass launches and how its items are laid out (no GPU): the engine's planner (csrc/fiber_plan.cpp plan_fiber_pass) read through
the host-only entry point tnqs_dbg_fiber_plan (include/tnqs_debug.h) against a restatement of the rules written here from their description -- the route
conditions of DESIGN.md ("Fiber GEMM routes") and the tile / tiles-per-workgroup rules documented next to each kernel's plan function.  Only shapes go in."""
import ctypes as C

import numpy as np
import pytest

import tnqs_amd as tn

IP = C.POINTER(C.c_int)
GENERIC, MFMA, ROWGEMM, F64 = 0, 1, 2, 3
CHAIN, EPILOGUE, PLAIN = 0, 1, 2
C64, C128 = 0, 1


def fiber_plan(use, dtype, items, use_mfma=1, use_chi64=1):
    """items: (D, PA, K, PB, Do, No) each.  Returns (launches, per_item): launches = dicts in stream order, per_item = dicts in the caller's order."""
    lib = C.CDLL(tn.LIB_PATH)
    fn = lib.tnqs_dbg_fiber_plan
    fn.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, IP, IP, C.c_int, IP, IP]
    fn.restype = C.c_int
    n = len(items)
    shape = np.ascontiguousarray(np.array(items, dtype=np.intc).reshape(n, 6))
    la = np.full((8, 10), -1, dtype=np.intc); it = np.full((max(1, n), 7), -1, dtype=np.intc); nl = C.c_int(-1)
    rc = fn(use, dtype, use_mfma, use_chi64, n, shape.ctypes.data_as(IP), la.ctypes.data_as(IP), 8, C.byref(nl), it.ctypes.data_as(IP))
    assert rc == 0 and 0 <= nl.value <= 8, rc
    lk = ("route", "D", "K", "TR", "tpw", "KKmax", "NNmax", "wgs", "nitems", "general")
    ik = ("launch", "begin", "nwg", "TA", "TB", "nta", "ntb")
    return [dict(zip(lk, map(int, la[l]))) for l in range(nl.value)], [dict(zip(ik, map(int, it[i]))) for i in range(n)]


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------------------
def pick_TR(KK, esz):
    for tr in (64, 32, 16, 8, 4):
        if KK * tr * esz <= 64 * 1024:
            return tr
    raise ValueError("too large")


def tiles_generic(PA, PB, TR):
    TA = min(PA, TR); TB = min(max(1, TR // TA), PB)
    return TA, TB, -(-PA // TA), -(-PB // TB)


def tiles_f64(PA, PB):
    TA = 16 if PA >= 16 else 8 if PA >= 8 else 4 if PA >= 4 else 2 if PA >= 2 else 1; TB = 16 // TA
    return TA, TB, -(-PA // TA), -(-PB // TB)


def rowgemm_covers(D, PA, K, PB, Do, No):
    if PA >= 32:
        if PA % 32:
            return False
    elif 32 % PA or PB % (32 // PA):
        return False
    return D == Do and D in (1, 2) and 1 <= No <= K and K in (32, 64)


def tiles_rowgemm(PA, PB):
    return (32, 1, PA // 32, PB) if PA >= 32 else (32, 1, 1, PB // (32 // PA))


def expected(use, f32, items, use_mfma=True, use_chi64=True):
    esz = 8 if f32 else 16
    KKmax = max([1] + [D * K for (D, PA, K, PB, Do, No) in items]); NNmax = max([1] + [Do * No for (D, PA, K, PB, Do, No) in items])       # over ALL items of the pass
    rgD, cap = {CHAIN: (1, 64), EPILOGUE: (2, 32), PLAIN: (0, 0)}[use]
    takes = [bool(rgD) and f32 and use_mfma and it[0] == rgD and rowgemm_covers(*it) and (it[2] != 64 or use_chi64) for it in items]
    launches, per_item = [], [None] * len(items)

    def lay_out(idx, tiles, tpw, head):
        w = 0
        for i, t in zip(idx, tiles):
            nwg = -(-(t[2] * t[3]) // tpw)
            per_item[i] = dict(launch=len(launches), begin=w, nwg=nwg, TA=t[0], TB=t[1], nta=t[2], ntb=t[3]); w += nwg
        launches.append(dict(head, tpw=tpw, KKmax=KKmax, NNmax=NNmax, wgs=w, nitems=len(idx), general=int(use == EPILOGUE)))

    for K in (64, 32):
        idx = [i for i, it in enumerate(items) if takes[i] and it[2] == K]
        if not idx:
            continue
        tiles = [tiles_rowgemm(items[i][1], items[i][3]) for i in idx]
        tpw = int(max(4.0, min(float(cap), sum(t[2] * t[3] for t in tiles) / 2048.0))) & ~3
        lay_out(idx, tiles, tpw, dict(route=ROWGEMM, D=rgD, K=K, TR=32))
    idx = [i for i in range(len(items)) if not takes[i]]
    if not idx and not (use == EPILOGUE and items):        # (the epilogue plans its last launch even when nothing is left for it)
        return launches, per_item
    matrix = use != PLAIN and use_mfma
    if use == CHAIN:
        f64 = matrix and not f32 and all(4 <= D * K <= 64 and 1 <= Do * No <= 64 for (D, PA, K, PB, Do, No) in (items[i] for i in idx))
    else:
        f64 = matrix and not f32 and 4 <= KKmax <= 64 and NNmax <= 64
    if f64:
        tiles = [tiles_f64(items[i][1], items[i][3]) for i in idx]
        tpw = 32 if use == EPILOGUE else int(max(8.0, min(64.0, sum(t[2] * t[3] for t in tiles) / 4096.0))) & ~3
        lay_out(idx, tiles, tpw, dict(route=F64, D=0, K=0, TR=16))
    elif matrix and f32 and 8 <= KKmax <= 64 and NNmax <= 64:
        if use == EPILOGUE:
            tpw = 16
        else:
            tpw = int(max(1.0, min(32.0, sum(D * PA * PB / 32.0 for (D, PA, K, PB, Do, No) in items) / 4096.0)))      # tiles of ALL items of the pass
            if tpw >= 4:
                tpw &= ~3
        lay_out(idx, [tiles_generic(items[i][1], items[i][3], 32) for i in idx], tpw, dict(route=MFMA, D=0, K=0, TR=32))
    else:
        TR = pick_TR(KKmax, esz)
        lay_out(idx, [tiles_generic(items[i][1], items[i][3], TR) for i in idx], 1, dict(route=GENERIC, D=0, K=0, TR=TR))
    return launches, per_item


# ---- items of a site tensor [d][chi_0]..[chi_{z-1}] ---------------------------------------------------------------------------------------------------------
def chain_item(dims, leg):
    d, chi = dims[0], dims[1:]
    return (1, d * int(np.prod(chi[:leg], dtype=np.int64)), chi[leg], int(np.prod(chi[leg + 1:], dtype=np.int64)), 1, chi[leg])


def epi_item(dims, leg, chin):
    d, chi = dims[0], dims[1:]
    return (d, int(np.prod(chi[:leg], dtype=np.int64)), chi[leg], int(np.prod(chi[leg + 1:], dtype=np.int64)), d, chin)


def chain_pass(sites, leg=1):
    return [chain_item(s, leg) for s in sites]


CASES = {
    # chain passes
    "chain_rowgemm_k32": (CHAIN, C64, chain_pass([[2, 32, 32]] * 3), 1, 1),
    "chain_rowgemm_k64": (CHAIN, C64, chain_pass([[2, 64, 64]] * 3), 1, 1),
    "chain_mfma_11": (CHAIN, C64, chain_pass([[2, 16, 16]] * 3), 1, 1),
    "chain_k64_then_k32_then_rest": (CHAIN, C64, chain_pass([[2, 32, 32], [2, 16, 16], [2, 64, 64], [2, 32, 32]]), 1, 1),
    "chain_24_with_64_quirk": (CHAIN, C64, chain_pass([[2, 24, 24], [2, 64, 64]]), 1, 1),
    "chain_24_alone": (CHAIN, C64, chain_pass([[2, 24, 24]]), 1, 1),
    "chain_f64": (CHAIN, C128, chain_pass([[2, 8, 8]] * 3), 1, 1),
    "chain_f64_one_chi70": (CHAIN, C128, chain_pass([[2, 8, 8], [2, 70, 70], [2, 8, 8]]), 1, 1),
    "chain_f64_one_chi3": (CHAIN, C128, chain_pass([[2, 8, 8], [2, 3, 3]]), 1, 1),
    "chain_chi3_generic": (CHAIN, C64, chain_pass([[2, 3, 3, 3]] * 2), 1, 1),
    "chain_chi40_three_legs": (CHAIN, C64, chain_pass([[2, 40, 40, 40], [2, 40, 40]], leg=0), 1, 1),
    "chain_chi70_f32": (CHAIN, C64, chain_pass([[2, 70, 70]]), 1, 1),
    "chain_no_mfma": (CHAIN, C64, chain_pass([[2, 32, 32], [2, 16, 16], [2, 64, 64]]), 0, 1),
    "chain_no_mfma_f64": (CHAIN, C128, chain_pass([[2, 8, 8]]), 0, 1),
    "chain_no_chi64": (CHAIN, C64, chain_pass([[2, 64, 64], [2, 32, 32]]), 1, 0),
    "chain_rowgemm_pa_fails": (CHAIN, C64, [chain_item([3, 32, 32], 0), chain_item([2, 32, 32], 0)], 1, 1),
    # gate epilogues
    "epi_rowgemm": (EPILOGUE, C64, [epi_item([2, 32, 32, 32], 1, 32), epi_item([2, 32, 32, 32], 0, 32)], 1, 1),
    "epi_rowgemm_k64_k32": (EPILOGUE, C64, [epi_item([2, 32, 32], 1, 32), epi_item([2, 64, 64], 1, 64), epi_item([2, 64, 64], 0, 48)], 1, 1),
    "epi_chi_shrinks": (EPILOGUE, C64, [epi_item([2, 16, 16, 16], 1, 12), epi_item([2, 16, 16, 16], 2, 12)], 1, 1),
    "epi_chi_shrinks_rowgemm": (EPILOGUE, C64, [epi_item([2, 32, 32, 32], 1, 20), epi_item([2, 32, 32], 0, 20)], 1, 1),
    "epi_d2_pa3_not_covered": (EPILOGUE, C64, [epi_item([2, 3, 32, 4], 1, 32), epi_item([2, 32, 32], 1, 32)], 1, 1),
    "epi_d3": (EPILOGUE, C64, [epi_item([3, 8, 8], 0, 8), epi_item([3, 8, 8], 1, 8)], 1, 1),
    "epi_kk_below_8": (EPILOGUE, C64, [epi_item([2, 3, 3], 0, 3)], 1, 1),
    "epi_chi40_generic": (EPILOGUE, C64, [epi_item([2, 40, 40], 0, 40)], 1, 1),
    "epi_f64": (EPILOGUE, C128, [epi_item([2, 8, 8, 8], 1, 8), epi_item([2, 8, 8], 0, 6)], 1, 1),
    "epi_f64_kk_below_4": (EPILOGUE, C128, [epi_item([2, 1, 4], 0, 2)], 1, 1),
    "epi_f64_chi40": (EPILOGUE, C128, [epi_item([2, 40, 40], 0, 40)], 1, 1),
    "epi_no_mfma": (EPILOGUE, C64, [epi_item([2, 32, 32, 32], 1, 32), epi_item([2, 16, 16], 0, 16)], 0, 1),
    "epi_no_mfma_f64": (EPILOGUE, C128, [epi_item([2, 8, 8], 0, 8)], 0, 1),
    "epi_no_chi64": (EPILOGUE, C64, [epi_item([2, 64, 64], 1, 64), epi_item([2, 32, 32], 1, 32)], 1, 0),
    # generic whatever the shape: one-site operators (D = d, K = 1), the second factorisation pass on ComplexF64 sites the f64 kernel could take
    "plain_one_site": (PLAIN, C64, [(3, 27, 1, 1, 3, 1), (2, 1024, 1, 1, 2, 1)], 1, 1),
    "plain_second_pass_f64": (PLAIN, C128, [epi_item([2, 8, 8, 8], 1, 8), epi_item([2, 8, 8], 0, 8)], 1, 1),
    "plain_rowgemm_shape": (PLAIN, C64, [epi_item([2, 32, 32, 32], 1, 32)], 1, 1),
    # tiles per workgroup, from item counts: f32 matrix-core tiles each side of 4 x 4096 tiles (one tile per item) ...
    "tpw_mfma_under": (CHAIN, C64, chain_pass([[2, 16, 16]] * (4 * 4096 - 1), leg=0), 1, 1),
    "tpw_mfma_at": (CHAIN, C64, chain_pass([[2, 16, 16]] * (4 * 4096), leg=0), 1, 1),
    "tpw_mfma_over": (CHAIN, C64, chain_pass([[2, 16, 16]] * (4 * 4096 + 1), leg=0), 1, 1),
    "tpw_mfma_7": (CHAIN, C64, chain_pass([[2, 16, 16]] * (7 * 4096 + 5), leg=0), 1, 1),
    # ... and the register-direct kernel each side of 4 x 2048 tiles (two tiles per item; its floor of 4 holds on both) and of 8 x 2048, where tpw moves
    "tpw_rowgemm_under_4": (CHAIN, C64, chain_pass([[2, 32, 32]] * (4096 - 1)), 1, 1),
    "tpw_rowgemm_over_4": (CHAIN, C64, chain_pass([[2, 32, 32]] * (4096 + 1)), 1, 1),
    "tpw_rowgemm_under_8": (CHAIN, C64, chain_pass([[2, 32, 32]] * (8192 - 1)), 1, 1),
    "tpw_rowgemm_over_8": (CHAIN, C64, chain_pass([[2, 32, 32]] * (8192 + 1)), 1, 1),
    "tpw_rowgemm_epilogue_cap": (EPILOGUE, C64, [epi_item([2, 32, 32, 32], 2, 32)] * 2100, 1, 1),
    "empty": (CHAIN, C64, [], 1, 1),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_matches_the_rules(name):
    use, dtype, items, mf, c64 = CASES[name]
    la, it = fiber_plan(use, dtype, items, mf, c64)
    ela, eit = expected(use, dtype == C64, items, bool(mf), bool(c64))
    assert la == ela
    assert it == eit


def test_routes_of_the_named_cases():
    """the restatement itself, pinned on the cases whose outcome the design states in words"""
    route = lambda name: [(l["route"], l["K"], l["tpw"]) for l in expected(CASES[name][0], CASES[name][1] == C64, CASES[name][2], bool(CASES[name][3]), bool(CASES[name][4]))[0]]
    assert route("chain_rowgemm_k32") == [(ROWGEMM, 32, 4)] and route("chain_rowgemm_k64") == [(ROWGEMM, 64, 4)] and route("chain_mfma_11") == [(MFMA, 0, 1)]
    assert route("chain_k64_then_k32_then_rest") == [(ROWGEMM, 64, 4), (ROWGEMM, 32, 4), (MFMA, 0, 1)]
    quirk = expected(*[CASES["chain_24_with_64_quirk"][0], True, CASES["chain_24_with_64_quirk"][2]])[0]
    assert [l["route"] for l in quirk] == [ROWGEMM, MFMA] and quirk[1]["KKmax"] == 64            # <2, 2, 16> because of the 64 in the same pass
    assert expected(CHAIN, True, CASES["chain_24_alone"][2])[0][0]["KKmax"] == 24                 # <1, 1, 8> on its own
    assert route("chain_f64") == [(F64, 0, 8)] and [r[0] for r in route("chain_f64_one_chi70")] == [GENERIC] and [r[0] for r in route("chain_f64_one_chi3")] == [GENERIC]
    assert [r[0] for r in route("chain_chi3_generic")] == [GENERIC] and [r[0] for r in route("chain_no_mfma")] == [GENERIC]
    assert route("chain_no_chi64") == [(ROWGEMM, 32, 4), (MFMA, 0, 1)]
    assert route("epi_rowgemm") == [(ROWGEMM, 32, 4), (MFMA, 0, 16)]                              # nothing left: the last launch is planned empty
    assert route("epi_chi_shrinks") == [(MFMA, 0, 16)] and route("epi_f64") == [(F64, 0, 32)] and route("epi_d2_pa3_not_covered") == [(ROWGEMM, 32, 4), (MFMA, 0, 16)]
    assert [r[0] for r in route("plain_second_pass_f64")] == [GENERIC] and [r[0] for r in route("plain_rowgemm_shape")] == [GENERIC]
    assert [route(n)[0][2] for n in ("tpw_mfma_under", "tpw_mfma_at", "tpw_mfma_over", "tpw_mfma_7")] == [3, 4, 4, 4]
    assert [route(n)[0][2] for n in ("tpw_rowgemm_under_4", "tpw_rowgemm_over_4", "tpw_rowgemm_under_8", "tpw_rowgemm_over_8")] == [4, 4, 4, 8]
    assert route("tpw_rowgemm_epilogue_cap")[0][2] == 32
