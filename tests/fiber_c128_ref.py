"""Plain numpy float64 references of the two ComplexF64 matrix-core operations (csrc/kernels_f64.hip) for a LIST of items -- the fiber product and the Gram over the
fibers -- each with the element-wise magnitude `absprod` the error bounds are stated in, the bounds themselves, and the case lists the CPU test
(tests/test_fiber_c128_ref_cpu.py) and the GPU test (tests/test_gpu_fiber_c128.py) share.  The references and bounds need neither a GPU nor the library; the two
ctypes wrappers at the end (run_fiber_pass, run_gram) call tnqs_dbg_fiber_pass_c128 / tnqs_dbg_gram_c128, host_only = the plan alone.

Layouts (include/tnqs_debug.h): a fiber item (D, PA, K, PB, Do, No) has in[(s, k), (a, b)] at s + D (a + PA (k + K b)), X[(s, k), (s', n)] at kk + KK nn with kk = s + D k,
nn = s' + Do n, out[(s', n), (a, b)] at s' + Do (a + PA (n + No b)); a Gram item (D, PA, K, PB) has X, Y laid out like `in` and out[p + KK q].

Bounds, u = 2^-53, none tuned:
  product   |out - ref| <= 2 (2 KK + 8) u absprod          absprod = |X|^T |in|: the complex dot product of length KK = D K (4 real products and 3 sums per term, KK - 1
                                                           sums of terms: (2 KK + 8) u covers it to first order with room for the fused forms), doubled because the
                                                           reference is itself a float64 evaluation with the same bound
  Gram      |out - ref| <= 2 (2 F + 2 nchunks + 8) u absprod   absprod = |X| |Y|^T, F = PA PB fibers, plus the sum over the chunks' partials
  norm      |sum partials - sum |ref|^2| <= sum (2 |ref| E + E^2) + (m + nwg + 8) u sum |ref|^2      E = the product bound, m output elements added up in nwg partials
"""
import numpy as np

U = 2.0 ** -53
CHAIN, EPILOGUE = 0, 1
# TNQS_DBG_ROUTE_* (include/tnqs_debug.h)
FIBER_GENERIC, FIBER_F64_PLAIN, FIBER_F64_GENERAL, GRAM_GENERIC, GRAM_F64IN = 15, 16, 17, 18, 19


def rnd(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex128)


# ---- the fiber product ----------------------------------------------------------------------------------------------------------------------------------------
def fiber_sizes(item):
    D, PA, K, PB, Do, No = item
    return D * PA * K * PB, D * K * Do * No, Do * PA * No * PB      # in, X, out


def fiber_matrix(x, D, PA, K, PB):
    """the tensor as a matrix [kk = s + D k, f = a + PA b]"""
    return x.reshape(PB, K, PA, D).transpose(1, 3, 0, 2).reshape(K * D, PB * PA)


def fiber_ref(item, x, X, dt=np.complex128):
    """(ref, absprod) in the memory order of out; dt: the type the product is evaluated in (np.clongdouble: the evaluation the float64 one is judged against)"""
    D, PA, K, PB, Do, No = item
    rt = np.float64 if dt == np.complex128 else np.longdouble
    M = fiber_matrix(np.asarray(x), D, PA, K, PB); XT = np.asarray(X).reshape(Do * No, D * K)      # XT[nn, kk]
    O = XT.astype(dt) @ M.astype(dt)
    A = np.abs(XT).astype(rt) @ np.abs(M).astype(rt)
    back = lambda o: o.reshape(No, Do, PB, PA).transpose(2, 0, 3, 1).reshape(-1)                     # [nn = (n, s'), f = (b, a)] -> b, n, a, s'
    return back(O), back(A)


def fiber_bound(item, absprod):
    return 2 * (2 * item[0] * item[2] + 8) * U * absprod


def norm_bound(item, ref, absprod, nwg):
    E = fiber_bound(item, absprod); r = np.abs(ref)
    return float(np.sum(2 * r * E + E * E) + (ref.size + nwg + 8) * U * np.sum(r * r))


# ---- the Gram over the fibers ---------------------------------------------------------------------------------------------------------------------------------
def gram_sizes(item):
    D, PA, K, PB = item
    return D * PA * K * PB, (D * K) ** 2


def gram_ref(item, x, y, dt=np.complex128):
    """(ref, absprod) with element (p, q) at p + KK q"""
    D, PA, K, PB = item
    rt = np.float64 if dt == np.complex128 else np.longdouble
    Mx = fiber_matrix(np.asarray(x), D, PA, K, PB); My = fiber_matrix(np.asarray(y), D, PA, K, PB)
    G = Mx.astype(dt) @ My.astype(dt).conj().T
    A = np.abs(Mx).astype(rt) @ np.abs(My).astype(rt).T
    return G.T.reshape(-1), A.T.reshape(-1)


def gram_bound(item, absprod, nchunks):
    return 2 * (2 * item[1] * item[3] + 2 * nchunks + 8) * U * absprod


def inside(out, ref, bound):
    """every element within its bound (a NaN is outside)"""
    return bool(np.all(np.abs(np.asarray(out) - ref) <= bound))


# ---- the planner's layout, restated for the coverage claims of the case lists (csrc/kernels_f64.hip plan_fiber_gemm_f64, csrc/kernels.hip plan_gram) --------------
def fiber_tiles(item):
    D, PA, K, PB, Do, No = item
    TA = 16 if PA >= 16 else 8 if PA >= 8 else 4 if PA >= 4 else 2 if PA >= 2 else 1
    return -(-PA // TA) * -(-PB // (16 // TA))


def gram_tiles(item):
    D, PA, K, PB = item
    TA = min(PA, 32); TB = min(max(1, 32 // TA), PB)
    return -(-PA // TA) * -(-PB // TB)


def gram_chunks(items, max_chunks):
    """(chunks, tiles per chunk) of every item of one launch"""
    if max_chunks <= 0:
        max_chunks = max(1, 2048 // len(items))
    out = []
    for it in items:
        t = gram_tiles(it); tpc = -(-t // min(max_chunks, t))
        out.append((-(-t // tpc), tpc))
    return out


# ---- fiber-pass cases: one launch each ------------------------------------------------------------------------------------------------------------------------
CLASSES = (16, 32, 64)
INST = {16: (1, 4), 32: (2, 8), 64: (4, 16)}      # class of Nmax -> NBLK, class of Kmax -> KS


def plain_items(Kc, Nc):
    """class-defining item (40 tiles), ragged item (KK, NN no multiple of 4 / 16, tiles ragged in a and b), the smallest item the kernel takes, PA = 48 with PB = 1;
    No != K on every item except, where Kc == Nc, the class-defining one"""
    return [(1, 16, Kc, 40, 1, Nc), (1, 3, Kc - 3, 11, 1, Nc - 5), (1, 1, 4, 40, 1, 1), (1, 48, Kc // 2 + 1, 1, 1, Nc // 2 + 2)]


def general_items(Kc, Nc):
    """the same four with D = Do = 2.  KK = 2 K and NN = 2 No are even then, so the ragged item has K = Kc / 2 - 1 (odd; KK = Kc - 2) and No = (Nc - 5) // 2 (odd; NN =
    Nc - 6), still no multiple of 4 / 16, and the smallest item is K = 2, No = 1; the odd KK = Kc - 3, NN = Nc - 5 and KK = 4, NN = 1 themselves ride along as D = Do = 1
    items, which the general kernel takes as well"""
    return [(2, 16, Kc // 2, 40, 2, Nc // 2), (2, 3, Kc // 2 - 1, 11, 2, (Nc - 5) // 2), (1, 3, Kc - 3, 11, 1, Nc - 5), (1, 1, 4, 40, 1, 1), (2, 1, 2, 40, 2, 1),
            (2, 48, Kc // 4 + 1, 1, 2, Nc // 4 + 1)]


def _case(use, items, route, mfma=1, tpw=0, scale=1.0, want=None):
    if want is None:
        want = [0] * len(items) if use == CHAIN else [(i + 1) % 2 for i in range(len(items))]      # general launches: every other item wants its norm
    Kmax = max(it[0] * it[2] for it in items); Nmax = max(it[4] * it[5] for it in items)
    cls = lambda v: 16 if v <= 16 else 32 if v <= 32 else 64
    inst = (0, 0, 0) if route == FIBER_GENERIC else (INST[cls(Nmax)][0], INST[cls(Kmax)][1], int(route == FIBER_F64_GENERAL))
    return dict(use=use, items=items, want=want, mfma=mfma, tpw=tpw, scale=scale, route=route, inst=inst)


FIBER_CASES = {}
for _Kc in CLASSES:
    for _Nc in CLASSES:
        FIBER_CASES[f"plain_k{_Kc}_n{_Nc}"] = _case(CHAIN, plain_items(_Kc, _Nc), FIBER_F64_PLAIN)
        FIBER_CASES[f"general_k{_Kc}_n{_Nc}"] = _case(EPILOGUE, general_items(_Kc, _Nc) + ([(3, 5, 4, 6, 3, 2)] if (_Kc, _Nc) == (16, 16) else []), FIBER_F64_GENERAL)
for _tpw in (1, 5, 20):      # (0 is the class case itself); 20: the 40-tile item walks 5 tiles per wave, past the first swap of the two register sets
    FIBER_CASES[f"plain_k32_n32_tpw{_tpw}"] = _case(CHAIN, plain_items(32, 32), FIBER_F64_PLAIN, tpw=_tpw)
    FIBER_CASES[f"general_k64_n16_tpw{_tpw}"] = _case(EPILOGUE, general_items(64, 16), FIBER_F64_GENERAL, tpw=_tpw)
for _s, _tag in ((1e-100, "tiny"), (1e100, "huge"), (0.0, "zero")):
    FIBER_CASES[f"plain_k16_n16_{_tag}"] = _case(CHAIN, plain_items(16, 16), FIBER_F64_PLAIN, scale=_s)
    FIBER_CASES[f"general_k16_n16_{_tag}"] = _case(EPILOGUE, general_items(16, 16), FIBER_F64_GENERAL, scale=_s)
# launches the matrix-core kernel does not take: the generic vector kernel runs them and the entry says so
FIBER_CASES["fallback_plain_kk3"] = _case(CHAIN, plain_items(16, 16) + [(1, 5, 3, 7, 1, 3)], FIBER_GENERIC)
FIBER_CASES["fallback_plain_k65"] = _case(CHAIN, plain_items(16, 16) + [(1, 4, 65, 3, 1, 2)], FIBER_GENERIC)
FIBER_CASES["fallback_general_kk66"] = _case(EPILOGUE, general_items(16, 16) + [(2, 4, 33, 3, 2, 3)], FIBER_GENERIC)
FIBER_CASES["fallback_plain_no_mfma"] = _case(CHAIN, plain_items(16, 16), FIBER_GENERIC, mfma=0)
FIBER_CASES["fallback_general_no_mfma"] = _case(EPILOGUE, general_items(16, 16), FIBER_GENERIC, mfma=0)


def fiber_data(name):
    """the inputs of a case (per item: in, X), and its float64 reference (per item: ref, absprod) -- computed once per process"""
    if name not in _FIBER_DATA:
        c = FIBER_CASES[name]
        rng = np.random.default_rng(sum(map(ord, name)))
        ins = [c["scale"] * rnd(rng, fiber_sizes(it)[0]) for it in c["items"]]
        Xs = [rnd(rng, fiber_sizes(it)[1]) for it in c["items"]]
        refs = [fiber_ref(it, a, b) for it, a, b in zip(c["items"], ins, Xs)]
        for a in ins + Xs + [r for p in refs for r in p]:
            a.setflags(write=False)
        _FIBER_DATA[name] = (ins, Xs, refs)
    return _FIBER_DATA[name]


_FIBER_DATA = {}

# ---- Gram cases: one launch each; (D, PA, K, PB) with PA in {1, 3, 20, 32, 33} and PB leaving the last tile of 32 fibers ragged (PA = 32: 5 whole tiles) -------------
GRAM_SAME = [(1, 1, 4, 40), (3, 3, 5, 11), (1, 20, 17, 7), (2, 32, 16, 5), (1, 33, 33, 40), (1, 3, 63, 11), (2, 20, 32, 7)]        # KK 4, 15, 17, 32, 33, 63, 64
GRAM_NONE = [(1, 3, 5, 11), (2, 1, 8, 40), (1, 32, 31, 5), (3, 20, 16, 7), (1, 33, 64, 40), (1, 1, 33, 40)]                          # KK 5, 16, 31, 48, 64, 33
GRAM_MIXED = [(2, 3, 2, 11), (1, 33, 17, 40), (2, 32, 24, 5), (3, 1, 21, 40), (1, 20, 32, 7), (1, 3, 16, 11)]                        # KK 4, 17, 48, 63, 32, 16
MIXED_FLAGS = [1, 0, 1, 0, 1, 0]


def _gcase(items, same, route, mfma=1, max_chunks=0, scale=1.0):
    return dict(items=items, same=same, mfma=mfma, max_chunks=max_chunks, scale=scale, route=route)


GRAM_CASES = {}
for _mc in (0, 1, 3):
    GRAM_CASES[f"same_chunks{_mc}"] = _gcase(GRAM_SAME, [1] * len(GRAM_SAME), GRAM_F64IN, max_chunks=_mc)
    GRAM_CASES[f"none_chunks{_mc}"] = _gcase(GRAM_NONE, [0] * len(GRAM_NONE), GRAM_F64IN, max_chunks=_mc)
    GRAM_CASES[f"mixed_chunks{_mc}"] = _gcase(GRAM_MIXED, MIXED_FLAGS, GRAM_F64IN, max_chunks=_mc)
for _s, _tag in ((1e-100, "tiny"), (1e100, "huge"), (0.0, "zero")):
    GRAM_CASES[f"same_{_tag}"] = _gcase(GRAM_SAME, [1] * len(GRAM_SAME), GRAM_F64IN, max_chunks=3, scale=_s)
    GRAM_CASES[f"none_{_tag}"] = _gcase(GRAM_NONE, [0] * len(GRAM_NONE), GRAM_F64IN, max_chunks=3, scale=_s)
GRAM_CASES["fallback_kk3"] = _gcase(GRAM_SAME + [(1, 5, 3, 7)], [1] * (len(GRAM_SAME) + 1), GRAM_GENERIC, max_chunks=3)
GRAM_CASES["fallback_kk66"] = _gcase(GRAM_NONE + [(2, 4, 33, 3)], [0] * (len(GRAM_NONE) + 1), GRAM_GENERIC, max_chunks=3)
GRAM_CASES["fallback_no_mfma"] = _gcase(GRAM_MIXED, MIXED_FLAGS, GRAM_GENERIC, mfma=0, max_chunks=3)


def gram_data(name):
    """the inputs of a case (per item: X, Y; Y is X itself where the item is `same`) and its float64 reference (per item: ref, absprod)"""
    if name not in _GRAM_DATA:
        c = GRAM_CASES[name]
        rng = np.random.default_rng(sum(map(ord, name)))
        Xs = [c["scale"] * rnd(rng, gram_sizes(it)[0]) for it in c["items"]]
        Ys = [x if s else c["scale"] * rnd(rng, x.size) for x, s in zip(Xs, c["same"])]
        refs = [gram_ref(it, x, y) for it, x, y in zip(c["items"], Xs, Ys)]
        for a in Xs + Ys + [r for p in refs for r in p]:
            a.setflags(write=False)
        _GRAM_DATA[name] = (Xs, Ys, refs)
    return _GRAM_DATA[name]


_GRAM_DATA = {}


# ---- the two entry points (include/tnqs_debug.h) through ctypes; host_only: the plan alone, no device is touched ---------------------------------------------------
GUARD = 8                       # guard band, in elements of the array's own type
PART_FILL = -7.25               # what the norm partials go up filled with


def _entries():
    import ctypes as C
    import tnqs_amd as tn
    lib = C.CDLL(tn.LIB_PATH)
    IP, VP = C.POINTER(C.c_int), C.c_void_p
    lib.tnqs_dbg_fiber_pass_c128.argtypes = [C.c_int, C.c_int, C.c_int, IP, IP, VP, VP, VP, VP, C.c_int, C.c_int, IP, IP, IP, IP]
    lib.tnqs_dbg_gram_c128.argtypes = [C.c_int, C.c_int, IP, IP, VP, VP, VP, C.c_int, IP, C.c_int, IP]
    lib.tnqs_last_error.restype = C.c_char_p
    return lib, IP, VP


def _banded(chunks, fill, dtype):
    """guard, item 0, guard, ..., guard filled with `fill`; returns the array and the slices of the items"""
    n = GUARD + sum(c + GUARD for c in chunks)
    arr = np.full(n, fill, dtype=dtype); sl = []; o = GUARD
    for c in chunks:
        sl.append(slice(o, o + c)); o += c + GUARD
    return arr, sl


def bands_intact(arr, slices, before):
    """the bytes outside the items are what went up (NaN fillings compare as bytes)"""
    mask = np.ones(arr.size, dtype=bool)
    for s in slices:
        mask[s] = False
    return bool(np.array_equal(arr[mask].view(np.uint8), before[mask].view(np.uint8)))


def run_fiber_pass(name, host_only=False):
    """-> dict(rc, route, inst, begin, nwg) and, on the device, outs (per item), out / out_before / out_slices, partials / partials_before / partials_slice"""
    import ctypes as C
    lib, IP, VP = _entries()
    c = FIBER_CASES[name]; n = len(c["items"])
    shape = np.ascontiguousarray(np.array(c["items"], dtype=np.intc).reshape(n, 6)); want = np.array(c["want"], dtype=np.intc)
    route = C.c_int(-1); inst = np.full(3, -1, dtype=np.intc); begin = np.full(n, -1, dtype=np.intc); nwg = np.full(n, -1, dtype=np.intc)
    ip = lambda a: a.ctypes.data_as(IP)
    rc = lib.tnqs_dbg_fiber_pass_c128(c["use"], c["mfma"], n, ip(shape), ip(want), None, None, None, None, c["tpw"], GUARD, C.byref(route), ip(inst), ip(begin), ip(nwg))
    res = dict(rc=rc, err=lib.tnqs_last_error(), route=route.value, inst=tuple(map(int, inst)), begin=list(map(int, begin)), nwg=list(map(int, nwg)))
    if host_only or rc != 0:
        return res
    ins, Xs, _ = fiber_data(name)
    cin = np.concatenate(ins); cX = np.concatenate(Xs)
    out, osl = _banded([fiber_sizes(it)[2] for it in c["items"]], complex(np.nan, np.nan), np.complex128)
    part, psl = _banded([sum(res["nwg"])], PART_FILL, np.float64)
    out0, part0 = out.copy(), part.copy()
    vp = lambda a: a.ctypes.data_as(VP)
    route2 = C.c_int(-1); inst2 = np.full(3, -1, dtype=np.intc)
    rc = lib.tnqs_dbg_fiber_pass_c128(c["use"], c["mfma"], n, ip(shape), ip(want), vp(cin), vp(cX), vp(out), vp(part), c["tpw"], GUARD, C.byref(route2), ip(inst2), ip(begin), ip(nwg))
    res.update(rc=rc, err=lib.tnqs_last_error(), route=route2.value, inst=tuple(map(int, inst2)), out=out, out_before=out0, out_slices=osl, outs=[out[s] for s in osl],
               partials=part, partials_before=part0, partials_slice=psl[0])
    return res


def run_gram(name, host_only=False):
    """-> dict(rc, route, nchunks) and, on the device, outs (per item), out / out_before / out_slices"""
    import ctypes as C
    lib, IP, VP = _entries()
    c = GRAM_CASES[name]; n = len(c["items"])
    shape = np.ascontiguousarray(np.array(c["items"], dtype=np.intc).reshape(n, 4)); same = np.array(c["same"], dtype=np.intc)
    route = C.c_int(-1); nch = np.full(n, -1, dtype=np.intc)
    ip = lambda a: a.ctypes.data_as(IP)
    if host_only:
        rc = lib.tnqs_dbg_gram_c128(c["mfma"], n, ip(shape), ip(same), None, None, None, c["max_chunks"], ip(nch), GUARD, C.byref(route))
        return dict(rc=rc, err=lib.tnqs_last_error(), route=route.value, nchunks=list(map(int, nch)))
    Xs, Ys, _ = gram_data(name)
    cX = np.concatenate(Xs)
    cY = np.concatenate([np.full(x.size, complex(np.nan, np.nan)) if s else y for x, y, s in zip(Xs, Ys, c["same"])])      # the slot of a `same` item is not read
    out, osl = _banded([gram_sizes(it)[1] for it in c["items"]], complex(np.nan, np.nan), np.complex128)
    out0 = out.copy()
    vp = lambda a: a.ctypes.data_as(VP)
    rc = lib.tnqs_dbg_gram_c128(c["mfma"], n, ip(shape), ip(same), vp(cX), None if all(c["same"]) else vp(cY), vp(out), c["max_chunks"], ip(nch), GUARD, C.byref(route))
    return dict(rc=rc, err=lib.tnqs_last_error(), route=route.value, nchunks=list(map(int, nch)), out=out, out_before=out0, out_slices=osl, outs=[out[s] for s in osl])
