"""Plain numpy float64 references of the chi = 32 plane operations (csrc/kernels_x3.hip, csrc/kernels_mfma.hip: pair product, pair-Gram for both messages and for one)
for a LIST of items, the item lists the CPU test (tests/test_plane32_ref_cpu.py) and the GPU test (tests/test_gpu_plane32.py) share, and a restatement of the four
workgroup-layout rules (plan_pair, plan_x3_pair_gram1, plan_pair_gram2, plan_pair_gram) and of the slice geometry (pair_geometry) written from their descriptions.
The references and the restatement need neither a GPU nor the library; the two ctypes wrappers at the end (run_pair32, run_pair_gram32) call tnqs_dbg_pair32 /
tnqs_dbg_pair_gram32 (include/tnqs_debug.h), without data = the plan alone (host only).

An item is (chi, lx, ly): the site tensor [d = 2][chi_0]..[chi_{z-1}] (column-major, site index fastest) with the plane of the two 32-dimensional legs lx, ly.
Matrices are stored M[i + 32 j]; a Gram comes back as out[b + 32 b'].

Bounds (test_bf16x3_plane_kernels_are_f32_accurate), relative to the largest entry of the reference, on either route:
  pair product 1e-6, each Gram 2e-6, each Gram of a product the device itself rounded to f32 (the level test) 3e-6."""
import functools

import numpy as np

ROUTE_X3, ROUTE_F32 = 1, 2                      # TNQS_DBG_ROUTE_* (include/tnqs_debug.h)
ERR_UNSUPPORTED = -2                            # include/tnqs.h
PAIR_BOUND, GRAM_BOUND, LEVEL_GRAM_BOUND = 1e-6, 2e-6, 3e-6
D = 2

# the smallest shapes that reach every branch: contiguous companions and the leg-0 branch of the geometry, all three slice counters, one- and four-slice items next to
# 128-slice ones
MIXED = [((8, 32, 32), 1, 2),            # 1 slice: 15 of the 16 workgroups of its group have nothing to do
         ((32, 32, 8), 0, 1),            # leg-0 branch, 1 slice
         ((32, 32, 32), 0, 2),           # leg-0 branch, n0 = 4
         ((32, 16, 32, 2), 0, 2),        # leg-0 branch, companions on a 16-dimensional leg, n1 = 2
         ((32, 32, 4, 32), 1, 3),        # n0 = 4, n1 = 4
         ((32, 8, 32, 32), 3, 0),        # lx > ly, leg-0 branch, n1 = 32
         ((32, 32, 32, 4), 1, 2),        # n2 = 4 with t2
         ((32, 32, 32, 32), 2, 1)]       # the workload's own item, the only one of its size in the launch
# a level of the engine: planes {0, 3} / {1, 2} of bulk sites next to degree-3 sites
BULK = [((32, 32, 32, 32), 0, 3), ((32, 32, 32, 32), 1, 2), ((32, 32, 32), 1, 2), ((32, 32, 32), 0, 1)]
LISTS = {"MIXED": MIXED, "BULK": BULK}
# one BP level as route_pair32 builds it: (chi, (pa, pb) the pair product's legs, (r, jo) the pair-Gram's plane).  T = psi x_pa Ma x_pb Mb, then out_y = the Gram of
# (T x_r Mx, psi) keeping jo and out_x = the Gram of (T x_jo My, psi) keeping r.  On a degree-4 site the two planes are disjoint and these are the BP messages leaving
# through jo and through r.  A degree-3 site has no two disjoint planes: there r is one of the product's legs and is absorbed a second time (Mb, then Mx) -- no BP
# message, but the same chain of the two kernels, with a reference just as direct
LEVEL = [((32, 32, 32, 32), (0, 1), (2, 3)), ((32, 32, 32, 32), (1, 2), (3, 0)), ((32, 32, 32), (0, 1), (1, 2)), ((32, 32, 32), (1, 2), (2, 0))]
# what the entry points refuse: a 16-dimensional leg in the plane, lx == ly, a lower plane leg above 8 elements without a companion leg, a degree-6 site that needs a
# fourth slice counter
REFUSED = [((32, 16, 32), 0, 1), ((32, 32, 32), 1, 1), ((4, 32, 32), 1, 2), ((32, 8, 2, 2, 2, 32), 0, 5)]


def rnd(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def tensor(flat, chi, dt=np.complex128):
    """the column-major site tensor as a numpy array indexed [s, i_0, ..., i_{z-1}]"""
    shp = (D,) + tuple(chi)
    return np.asarray(flat).reshape(shp[::-1]).transpose(*range(len(shp) - 1, -1, -1)).astype(dt)


def matrix(flat, dt=np.complex128):
    """M[i, j] from M[i + 32 j]"""
    return np.asarray(flat).reshape(32, 32).T.astype(dt)


# ---- the references: evaluated in the type of their arguments (complex128: the reference; complex64: what plain f32 arithmetic gives) ------------------------------------
def absorb(t, M, leg):
    """t x_leg M: out[.., j on leg, ..] = sum_i t[.., i on leg, ..] M[i, j]"""
    return np.moveaxis(np.tensordot(t, M, axes=([1 + leg], [0])), -1, 1 + leg)


def pair_product(t, Mx, My, lx, ly):
    return absorb(absorb(t, Mx, lx), My, ly)


def gram_keeping(X, Y, kept):
    """G[b, b'] = sum over everything but leg `kept` of X[.., b, ..] conj(Y[.., b', ..])"""
    axes = [a for a in range(X.ndim) if a != 1 + kept]
    return np.tensordot(X, Y.conj(), axes=(axes, axes))


def pair_gram(X, Y, M, absorbed, kept):
    return gram_keeping(absorb(X, M, absorbed), Y, kept)


def rel_err(got, ref):
    """largest deviation relative to the largest entry of the reference (NaN where anything is not finite); an all-zero reference wants exact zeros"""
    got = np.asarray(got); top = float(np.max(np.abs(ref)))
    if not np.all(np.isfinite(got)):
        return float("nan")
    if top == 0.0:
        return 0.0 if not np.any(got) else float("inf")
    return float(np.max(np.abs(got - ref))) / top


# ---- the slice geometry and the four layout rules, restated ----------------------------------------------------------------------------------------------------------------
def geometry(chi, lx, ly, d=D):
    """the slice counters (n0, n1, n2) of a plane the kernels cover, None for one they do not.  A slice is 16 companion elements x the 32 x 32 plane.  Both plane legs above
    16 or more elements: the companions are 16 contiguous elements, the counters walk what is left below the lower leg, between the legs and above the upper one.  The lower
    leg directly above a 2-dimensional site index: the companions are the site index x 8 values of the first other leg whose dimension is a multiple of 8; the counters
    walk the rest of that leg and at most two more legs"""
    z = len(chi)
    if lx == ly or not (0 <= lx < z and 0 <= ly < z) or chi[lx] != 32 or chi[ly] != 32:
        return None
    pre = lambda j: d * int(np.prod(chi[:j], dtype=np.int64))
    p, q = min(lx, ly), max(lx, ly)
    if pre(p) % 16 == 0:
        return pre(p) // 16, pre(q) // (pre(p) * 32), int(np.prod(chi[q + 1:], dtype=np.int64))
    if pre(p) != 2:
        return None
    others = [i for i in range(z) if i not in (p, q)]
    comp = next((i for i in others if chi[i] % 8 == 0), None)
    rest = [chi[i] for i in others if i != comp]
    if comp is None or len(rest) > 2:
        return None
    return (chi[comp] // 8,) + tuple(rest + [1, 1])[:2]


def slices(item):
    return int(np.prod(geometry(*item)))


def _cdiv(a, b):
    return -(-a // b)


def _lay_out(counts):
    begin = list(np.cumsum([0] + counts[:-1])) if counts else []
    return [int(b) for b in begin], counts, int(sum(counts))


def plan_pair(sl, spw=0):
    """pair product and the bf16 one-message pair-Gram.  spw: 16, halved while 2 sum(slices) / spw < 1024, down to 1; an item gets 16 ceil(ceil(slices / spw) / 8)
    workgroups.  -> (spw, wg_begin, nwg, total)"""
    if spw <= 0:
        spw = 16
        while spw > 1 and 2 * sum(sl) / spw < 1024:
            spw //= 2
    return (spw,) + _lay_out([16 * _cdiv(_cdiv(s, spw), 8) for s in sl])


plan_x3_pair_gram1 = plan_pair


def plan_pair_gram2(sl, spw=0, per_group=16):
    """both messages.  spw: the largest power of two <= 16 with sum 16 groups >= 1024, else 1, groups = ceil(ceil(slices / spw) / 8); an item gets per_group groups
    workgroups, per_group = 16 on the bf16 route and 32 on the f32 route"""
    groups = lambda s, w: _cdiv(_cdiv(s, w), 8)
    if spw <= 0:
        spw = next((w for w in (16, 8, 4, 2) if sum(16 * groups(s, w) for s in sl) >= 1024), 1)
    return (spw,) + _lay_out([per_group * groups(s, spw) for s in sl])


def plan_pair_gram(sl, spw=0):
    """the f32 one-message pair-Gram.  spw = int(clamp(sum(slices) / 2048, 4, 16)); an item gets ceil(slices / spw) workgroups"""
    if spw <= 0:
        spw = int(max(4.0, min(16.0, sum(sl) / 2048.0)))
    return (spw,) + _lay_out([_cdiv(s, spw) for s in sl])


def expected_plan(kind, route, sl, spw=0):
    """kind: "pair", "gram2" (form 0), "gram1" (form 1) on the route the entry point reported"""
    if kind == "gram2":
        return plan_pair_gram2(sl, spw, 16 if route == ROUTE_X3 else 32)
    if kind == "gram1" and route == ROUTE_F32:
        return plan_pair_gram(sl, spw)
    return plan_pair(sl, spw)


# ---- inputs and references of a launch, computed once and read-only ---------------------------------------------------------------------------------------------------------
# the items of MIXED scaled differently in one launch, one of them all zero (X; its Y stays): error is per item, relative to that item's own largest reference entry
SCALES = (1.0, 1e-12, 1e6, 1e-3, 0.0, 1e3, 1e-6, 1e-9)


@functools.lru_cache(maxsize=None)
def launch_data(name, scaled=False):
    """-> dict(items, X, Y: flat complex64 per item, M: 2048 complex64 per item (Mx, My), prod, gy, gx: float64 references in device layout -- prod flat like X,
    gy / gx as out[b + 32 b'])"""
    items = LISTS[name]
    rng = np.random.default_rng(sum(map(ord, name)) + (1000 if scaled else 0))
    X = [rnd(rng, D * int(np.prod(c))) for c, _, _ in items]; Y = [rnd(rng, x.size) for x in X]; M = [rnd(rng, 2048) for _ in items]
    if scaled:
        for x, y, s in zip(X, Y, SCALES):
            x *= np.float32(s)
            if s != 0.0:
                y *= np.float32(s)
    out = dict(items=items, X=X, Y=Y, M=M)
    out.update(references(items, X, Y, M))
    for v in out.values():
        for a in v:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return out


def references(items, X, Y, M, dt=np.complex128):
    prod, gy, gx = [], [], []
    for (chi, lx, ly), x, y, m in zip(items, X, Y, M):
        tx, ty, Mx, My = tensor(x, chi, dt), tensor(y, chi, dt), matrix(m[:1024], dt), matrix(m[1024:], dt)
        prod.append(np.ravel(pair_product(tx, Mx, My, lx, ly), order="F"))
        gy.append(np.ravel(pair_gram(tx, ty, Mx, lx, ly), order="F"))         # keeps ly, lx absorbed with Mx
        gx.append(np.ravel(pair_gram(tx, ty, My, ly, lx), order="F"))         # keeps lx, ly absorbed with My
    return dict(prod=prod, gy=gy, gx=gx)


@functools.lru_cache(maxsize=None)
def level_data():
    """the items of LEVEL: psi and four matrices per item.  -> dict(items, psi, M (4 x 1024 complex64 per item: Ma, Mb, Mx, My), msg_jo, msg_r: the float64 results from
    psi and the four matrices directly, as out[b + 32 b'])"""
    rng = np.random.default_rng(4321)
    psi = [rnd(rng, D * int(np.prod(c))) for c, _, _ in LEVEL]; M = [rnd(rng, 4096) for _ in LEVEL]
    out = dict(items=LEVEL, psi=psi, M=M)
    out.update(level_reference(LEVEL, psi, M))
    for k in ("psi", "M", "msg_jo", "msg_r"):
        for a in out[k]:
            a.setflags(write=False)
    return out


def level_reference(items, psi, M, dt=np.complex128, round_T=None):
    """msg_jo: psi with (pa, Ma), (pb, Mb), (r, Mx) absorbed one after the other, then the Gram with psi keeping jo; msg_r: (pa, Ma), (pb, Mb), (jo, My), keeping r.
    round_T: the type the intermediate T is rounded to (what the device does: complex64)"""
    res = dict(msg_jo=[], msg_r=[])
    for (chi, (pa, pb), (r, jo)), p, m in zip(items, psi, M):
        t = tensor(p, chi, dt); Ma, Mb, Mx, My = (matrix(m[1024 * k:1024 * (k + 1)], dt) for k in range(4))
        T = absorb(absorb(t, Ma, pa), Mb, pb)
        if round_T is not None:
            T = T.astype(round_T).astype(dt)
        res["msg_jo"].append(np.ravel(gram_keeping(absorb(T, Mx, r), t, jo), order="F"))
        res["msg_r"].append(np.ravel(gram_keeping(absorb(T, My, jo), t, r), order="F"))
    return res


# ---- the two entry points through ctypes ------------------------------------------------------------------------------------------------------------------------------------
from fiber_c128_ref import GUARD, _banded, bands_intact      # noqa: E402  (guard band of 8 elements of the array's own type; the same layout and check)


def _entries():
    import ctypes as C
    import tnqs_amd as tn
    lib = C.CDLL(tn.LIB_PATH)
    IP, VP = C.POINTER(C.c_int), C.c_void_p
    lib.tnqs_dbg_pair32.argtypes = [C.c_int, C.c_int, IP, IP, IP, IP, VP, VP, VP, C.c_int, C.c_int, IP, IP, IP, IP, IP]
    lib.tnqs_dbg_pair_gram32.argtypes = [C.c_int, C.c_int, IP, IP, IP, IP, C.c_int, VP, VP, VP, VP, VP, C.c_int, C.c_int, IP, IP, IP, IP, IP]
    lib.tnqs_last_error.restype = C.c_char_p
    return lib, IP, VP


def banded(sizes):
    """guard, item 0, guard, ..., guard, all NaN complex64; returns the array and the items' slices"""
    return _banded(sizes, complex(np.nan, np.nan), np.complex64)


def _shape_args(items, IP):
    z = np.array([len(c) for c, _, _ in items], dtype=np.intc); chi = np.array([x for c, _, _ in items for x in c], dtype=np.intc)
    lx = np.array([it[1] for it in items], dtype=np.intc); ly = np.array([it[2] for it in items], dtype=np.intc)
    return [a.ctypes.data_as(IP) for a in (z, chi, lx, ly)], (z, chi, lx, ly)


def _plan_outputs(n, C, IP):
    route, spw, total = C.c_int(-1), C.c_int(-1), C.c_int(-1); begin = np.full(n, -1, dtype=np.intc); nwg = np.full(n, -1, dtype=np.intc)
    args = [C.byref(route), C.byref(spw), begin.ctypes.data_as(IP), nwg.ctypes.data_as(IP), C.byref(total)]
    return args, lambda: dict(route=route.value, spw=spw.value, begin=list(map(int, begin)), nwg=list(map(int, nwg)), total=total.value)


def run_pair32(items, X=None, M=None, spw=0):
    """-> dict(rc, err, route, spw, begin, nwg, total) and, with data, outs (per item), out / out_before / out_slices.  X is None: host only"""
    import ctypes as C
    lib, IP, VP = _entries()
    n = len(items); shape, keep = _shape_args(items, IP); plan, read = _plan_outputs(n, C, IP)
    if X is None:
        rc = lib.tnqs_dbg_pair32(D, n, *shape, None, None, None, spw, GUARD, *plan)
        return dict(rc=rc, err=lib.tnqs_last_error(), **read())
    cin = np.concatenate(X); cm = np.concatenate(M)
    out, osl = banded([x.size for x in X]); out0 = out.copy()
    rc = lib.tnqs_dbg_pair32(D, n, *shape, cin.ctypes.data_as(VP), cm.ctypes.data_as(VP), out.ctypes.data_as(VP), spw, GUARD, *plan)
    return dict(rc=rc, err=lib.tnqs_last_error(), out=out, out_before=out0, out_slices=osl, outs=[out[s] for s in osl], **read())


def run_pair_gram32(items, form, X=None, Y=None, M=None, spw=0):
    """-> dict(rc, err, route, spw, begin, nwg, total) and, with data, oy / ox (per item), out_y / out_x, their copies before the call and the slices.  X is None: host only"""
    import ctypes as C
    lib, IP, VP = _entries()
    n = len(items); shape, keep = _shape_args(items, IP); plan, read = _plan_outputs(n, C, IP)
    if X is None:
        rc = lib.tnqs_dbg_pair_gram32(D, n, *shape, form, None, None, None, None, None, spw, GUARD, *plan)
        return dict(rc=rc, err=lib.tnqs_last_error(), **read())
    cx, cy, cm = np.concatenate(X), np.concatenate(Y), np.concatenate(M)
    oy, sl = banded([1024] * n); ox, _ = banded([1024] * n); oy0, ox0 = oy.copy(), ox.copy()
    rc = lib.tnqs_dbg_pair_gram32(D, n, *shape, form, cx.ctypes.data_as(VP), cy.ctypes.data_as(VP), cm.ctypes.data_as(VP), oy.ctypes.data_as(VP), ox.ctypes.data_as(VP),
                                  spw, GUARD, *plan)
    return dict(rc=rc, err=lib.tnqs_last_error(), out_y=oy, out_x=ox, out_y_before=oy0, out_x_before=ox0, out_slices=sl, oy=[oy[s] for s in sl], ox=[ox[s] for s in sl],
                **read())
