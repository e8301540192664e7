"""Kernel-level GPU tests of the sampling kernels (kernels_sample.hip: site_prob_partial_kernel<T>, site_draw_kernel, site_project_kernel<T>), the ComplexF32 d = 2 one-site
gate with its normalisation (kernels_util.hip: site1_c64_kernel, norm_factor_kernel, scale_kernel<T>) and the form scalars (kernels_inner.hip: inner_scalar_kernel<T>), through
the tnqs_dbg_* entry points of include/tnqs_debug.h, against the references of tests/site_kernels_ref.py (pinned on the CPU in tests/test_site_kernels_ref_cpu.py).  Shapes are
the smallest at which the index arithmetic leaves its trivial case: site dimensions that do not divide 256 on more than one workgroup, tail lanes, grid-stride loops, items of
different lengths in one launch.  Every output array carries guard bands that are checked after every call.

Bounds are derived, none is measured on the kernels (site_kernels_ref states each next to the reference it belongs to):
    site_prob_partial   |partial - ref| <= (ceil(n / NT) + ceil(256 / d) + 4) 2^-53 sum|terms| per workgroup and site index, ref from the ownership map
    site1               |out - ref| <= 8 2^-24 sum_s |G[s', s]| |in[s]| + sum_s |G - fl32(G)|[s', s] |in[s]| per real component
    norm partials       |sum of partials - fsum(|out|^2)| <= k 2^-53 fsum, k = 4 ceil(npairs / (256 nbx)) + 12
    norm_factor         |factor - 1 / sqrt(sum)| <= 2 ulp on the site1 path (<= 64 partials); direct: relative ((ceil(npart / 256) + 9) / 2 + 3) 2^-53
    inner_scalar        8 (k + 4) 2^-53 sum|terms|, k = rows cols
site_draw, site_project and scale are compared bit for bit.  The worst measured ratio error / bound is printed per test (MEASURED lines; DESIGN.md 5 records them)."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import tnqs_amd as tn
import sampling_ref as sr
import site_kernels_ref as ref

pytestmark = pytest.mark.gpu
lib = C.CDLL(tn.LIB_PATH)
DTYPES = (0, 1)
DT_IDS = ["c64", "c128"]
GUARD = 5
SENT = -7.5 + 3.25j
ISENT = -77


def _ints(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.int32))


def _f64(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.float64))


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.real.dtype.itemsize])


def _measured(what, ratio):
    print(f"MEASURED {what}: error / bound = {ratio:.3f}")


def _worst(pairs):
    """pairs of (error array, bound array): asserts every element is inside its bound, returns the worst ratio"""
    w = 0.0
    for e, b in pairs:
        e, b = np.atleast_1d(np.asarray(e, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
        assert np.all(np.isfinite(e))
        bad = e > b
        assert not bad.any(), f"{int(bad.sum())} elements outside the bound, worst error {e[bad].max():.3e} against {b[bad][np.argmax(e[bad])]:.3e}"
        nz = b > 0
        if nz.any():
            w = max(w, float(np.max(e[nz] / b[nz])))
    return w


class Guarded:
    """an output array as the entry points take it: guard sentinels, item 0, guard sentinels, item 1, ..., guard sentinels"""

    def __init__(self, lens, dt, guard=GUARD):
        self.lens, self.guard = list(lens), guard
        dt = np.dtype(dt)
        self.fill = np.asarray(SENT if dt.kind == "c" else SENT.real if dt.kind == "f" else ISENT).astype(dt)
        self.start = np.cumsum([guard] + [l + guard for l in self.lens])[:-1]
        self.a = np.full(guard + sum(l + guard for l in self.lens), self.fill, dtype=dt)
        self.mask = np.ones(self.a.size, dtype=bool)
        for s, l in zip(self.start, self.lens):
            self.mask[s:s + l] = False

    def item(self, i):
        return self.a[self.start[i]:self.start[i] + self.lens[i]]

    def check(self, written=None):
        """the guard bands are as they went up; written True / False: every / no element of an item was written"""
        assert np.all(self.a[self.mask] == self.fill), "a guard element was overwritten"
        if written is True:
            assert not np.any(self.a[~self.mask] == self.fill), "an element of an item was not written"
        if written is False:
            assert np.all(self.a == self.fill)


# ---- site_prob_partial -------------------------------------------------------------------------------------------------------------------------------------------------------
def site_prob(t, p, d, dtype, nblocks=0):
    nb = C.c_int(-1)
    assert lib.tnqs_dbg_site_prob(dtype, t.size, d, None, None, nblocks, None, 0, C.byref(nb)) == 0
    assert nb.value == (nblocks if nblocks else ref.plan_site_prob(t.size, d))
    out = Guarded([16 * nb.value], np.float64)
    used = C.c_int(-1)
    rc = lib.tnqs_dbg_site_prob(dtype, t.size, d, _p(t), _p(p), nblocks, _p(out.a), GUARD, C.byref(used))
    assert rc == 0 and used.value == nb.value, (rc, lib.tnqs_last_error())
    out.check()
    part = out.item(0).reshape(nb.value, 16)
    assert np.all(part[:, d:] == out.fill), "a slot s >= d was written"
    assert not np.any(part[:, :d] == out.fill), "a slot s < d was not written"
    return part[:, :d].copy()


def _check_partials(t, p, d, dtype, nblocks):
    n = t.size
    part = site_prob(t, p, d, dtype, nblocks)
    nb = part.shape[0]
    want, ab = ref.partials(t, p, d, nb)
    err = np.abs(part.astype(ref.LD) - want[:, :d]).astype(np.float64)
    return err, ref.partial_bound(n, d, nb, ab[:, :d]), part, want[:, :d]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("d", ref.SITE_DIMS)
def test_site_prob_every_partial_is_the_ownership_maps(d, dtype):
    pairs = []
    for n, nblocks in ref.site_prob_cases(d):
        t, p = ref.site_inputs(n, d, dtype, 1)
        err, bound, part, want = _check_partials(t, p, d, dtype, nblocks)
        bad = err > bound
        assert not bad.any(), (n, d, nblocks, np.argwhere(bad)[:4].tolist(), part[bad][:4], want[bad][:4].astype(np.float64))
        pairs.append((err, bound))
    _measured(f"site_prob_partial d {d} dtype {dtype}", _worst(pairs))


def test_site_prob_forced_workgroups_agree_on_the_diagonal():
    """1, 2 and 5 workgroups on the same data: different partial arrays (each checked above), one diagonal"""
    for d in (3, 7):
        n = d * (1500 // d)
        t, p = ref.site_inputs(n, d, 0, 1)
        dg, dab = ref.diag(t, p, d)
        for nb in (1, 2, 5):
            tot = site_prob(t, p, d, 0, nb).astype(ref.LD).sum(axis=0)
            assert np.all(np.abs(tot - dg).astype(np.float64) <= ref.partial_bound(n, d, nb, dab))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_site_prob_1024_workgroup_cap(dtype):
    n, d = ref.BIG_CASE[dtype]
    t, p = ref.site_inputs(n, d, dtype, 1)
    err, bound, part, _ = _check_partials(t, p, d, dtype, 0)
    assert part.shape[0] == 1024
    _measured(f"site_prob_partial n {n} d {d} dtype {dtype}", _worst([(err, bound)]))


@pytest.mark.parametrize("scale", (1e-30, 1.0, 1e30))
def test_site_prob_c64_scale_sweep(scale):
    """products of 1e-60 and 1e+60 live only in the f64 accumulator: the bound is relative to the partial's own sum of |terms|, so nothing may underflow or overflow"""
    d, n = 3, 3 * (2048 // 3 + 1)
    rng = np.random.default_rng(77)
    sc = np.tile(np.array([1.0, 1e-3, 1.0]), n // d)
    t = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * scale).astype(np.complex64)
    p = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * sc * scale).astype(np.complex64)
    tiny = float(np.finfo(np.float32).tiny)
    for a in (t, p):                                             # normal floats only: this is about the accumulator, not about denormal inputs
        assert np.all(np.abs(a.real) >= tiny) and np.all(np.abs(a.imag) >= tiny) and np.all(np.isfinite(a))
    err, bound, part, want = _check_partials(t, p, d, 0, 0)
    assert part.shape[0] == 3 and np.all(part != 0) and np.all(np.isfinite(part))
    _measured(f"site_prob_partial scale {scale:g}", _worst([(err, bound)]))


# ---- site_draw ------------------------------------------------------------------------------------------------------------------------------------------------------------
def site_draw(items):
    """items: dicts with partial (nblocks x 16), d, neg_tol, u (float) or counter (seed, sample, step), draw -> (p [n, 16], x, px, status) with the sentinels where nothing was
    written; the guards are checked"""
    n = len(items)
    parts = _f64(np.concatenate([np.asarray(it["partial"], dtype=np.float64).reshape(-1) for it in items]))
    nbs = [np.asarray(it["partial"]).size // 16 for it in items]
    u = _f64([it.get("u", 0.987654321) for it in items])
    use = _ints(["counter" in it for it in items])
    ctr = np.ascontiguousarray(np.array([it.get("counter", (0, 0, 0)) for it in items], dtype=np.uint64).reshape(-1))
    P, X, PX = Guarded([16] * n, np.float64), Guarded([1] * n, np.int32), Guarded([1] * n, np.float64)
    st = _ints([ISENT] * n)
    rc = lib.tnqs_dbg_site_draw(n, _p(_ints(nbs)), _p(_ints([it["d"] for it in items])), _p(parts), _p(_f64([it.get("neg_tol", 1e-8) for it in items])), _p(u), _p(use), _p(ctr),
                                _p(_ints([it.get("draw", 1) for it in items])), _p(P.a), _p(X.a), _p(PX.a), _p(st), GUARD)
    assert rc == 0, (rc, lib.tnqs_last_error())
    P.check(); X.check(); PX.check()
    p = np.stack([P.item(i) for i in range(n)])
    for i, it in enumerate(items):
        assert np.all(p[i, it["d"]:] == P.fill), "p was written beyond d"
    return p, np.array([X.item(i)[0] for i in range(n)]), np.array([PX.item(i)[0] for i in range(n)]), st.copy()


def _partial_of(diag, nblocks, rng):
    """an nblocks x 16 partial array whose columns add up to about diag (the kernel's own in-order sum decides the exact value)"""
    diag = np.asarray(diag, dtype=np.float64)
    w = rng.random((nblocks, len(diag))) + 0.1
    part = np.zeros((nblocks, 16))
    part[:, :len(diag)] = w / w.sum(axis=0) * diag
    part[:, len(diag):] = np.nan                                 # slots the kernel must not read
    return part


def _boundary_uniforms(p):
    cdf = np.cumsum(p)                                           # sequential f64: the kernel's cdf bit for bit
    us = [0.0, float(np.nextafter(1.0, 0.0))]
    for c in cdf:
        us += [float(c), float(np.nextafter(c, -np.inf)), float(np.nextafter(c, np.inf))]
    return [u for u in us if u >= 0], cdf                      # (below a boundary at 0 there is no uniform)


def _draw_variants(d):
    rng = np.random.default_rng(100 + d)
    out = [(_partial_of(rng.random(d) + 0.05, 3, rng), 1e-8), (_partial_of(rng.random(d) * 10.0 ** rng.integers(-3, 3, d), 1, rng), 1e-8)]
    if d >= 2:
        dg = rng.random(d) + 0.05; dg[0] = 0.0                   # a leading zero-probability entry
        if d >= 3:
            dg[d // 2] = 0.0; dg[1] = -1e-12                     # an interior one, and a negative entry within neg_tol: counts as 0
        out.append((_partial_of(dg, 2, rng), 1e-8))
    return out


@pytest.mark.parametrize("d", (1, 2, 3, 16))
def test_site_draw_rule_on_every_cdf_boundary(d):
    """p bit for bit, then x = sampling_ref.draw(p, u) and px = p[x] for u = 0, the largest double below 1, every cdf boundary and its two neighbours: no case is left out"""
    items, want = [], []
    for part, tol in _draw_variants(d):
        status, p = ref.draw_expect(part, d, tol)
        assert status == 0
        us, cdf = _boundary_uniforms(p)
        for u in us:
            items.append(dict(partial=part, d=d, neg_tol=tol, u=u)); want.append((p, u, cdf))
    pg, x, px, st = site_draw(items)
    assert len(items) >= 3 * d * 2 + 2
    for i, (p, u, cdf) in enumerate(want):
        assert np.array_equal(_bits(pg[i, :d]), _bits(p)), (i, pg[i, :d], p)
        assert st[i] == 0
        assert x[i] == sr.draw(pg[i, :d], u), (i, u, cdf.tolist(), x[i])
        assert _bits(np.float64(px[i])) == _bits(pg[i, x[i]])
        if u < cdf[-1]:
            assert pg[i, x[i]] > 0, "a zero-probability entry was drawn"
        if u == cdf[0] and d > 1:
            assert x[i] >= 1                                     # u < cdf, not u <= cdf


def test_site_draw_fallback_on_a_trailing_zero_entry_is_pinned():
    """the known corner: the fallback is "the last entry if u >= cdf[d - 1]", also where that entry has probability zero"""
    rng = np.random.default_rng(5)
    for _ in range(200):
        dg = np.append(rng.random(3) + 0.1, 0.0)
        part = _partial_of(dg, 1, rng)
        _, p = ref.draw_expect(part, 4, 1e-8)
        if np.cumsum(p)[-1] < 1.0:
            break
    else:
        raise AssertionError("no probabilities whose f64 cdf ends below 1")
    u = float(np.nextafter(1.0, 0.0))
    assert u >= np.cumsum(p)[-1] and sr.draw(p, u) == 3
    pg, x, px, st = site_draw([dict(partial=part, d=4, u=u), dict(partial=part, d=4, u=float(np.nextafter(np.cumsum(p)[-1], 0.0)))])
    assert st.tolist() == [0, 0] and x[0] == 3 and px[0] == 0.0 and pg[0, 3] == 0.0
    assert x[1] == 2 and px[1] == pg[1, 2] > 0


def _row(vals, nan_rest=True):
    r = np.full((1, 16), np.nan if nan_rest else 0.0); r[0, :len(vals)] = vals
    return r


def test_site_draw_status_and_bad_input_outputs():
    tol = 2.0 ** -10
    below = float(np.nextafter(2.0 ** -10, 1.0))
    items = [dict(partial=_row([0.0, 0.0, 0.0]), d=3, u=0.5),                                  # tr = 0
             dict(partial=_row([0.25, -0.5]), d=2, u=0.5),                                     # tr < 0
             dict(partial=_row([np.inf, 1.0]), d=2, u=0.5),                                    # tr = +inf
             dict(partial=_row([1.0, np.nan, 1.0]), d=3, u=0.5),                               # tr = NaN
             dict(partial=_row([1.0 + tol, -below]), d=2, neg_tol=tol, u=0.75),                # an entry just below -neg_tol tr (tr = 1 exactly)
             dict(partial=_row([1.0 + tol, -tol]), d=2, neg_tol=tol, u=0.75),                  # exactly at -neg_tol tr: clean
             dict(partial=_row([0.5, 0.5]), d=2, u=0.75),                                      # a clean item behind bad ones: the status word is the item's own
             dict(partial=_row([0.0, 0.0]), d=2, u=0.5, draw=0),                               # bad, no draw: p and status only
             dict(partial=np.concatenate([_row([1e308, 1.0]), _row([1e308, 1.0])]), d=2, u=0.5)]      # the sum over workgroups overflows
    for it, want in zip(items, (1, 1, 1, 1, 2, 0, 0, 1, 1)):
        assert ref.draw_expect(it["partial"], it["d"], it.get("neg_tol", 1e-8))[0] == want
    assert 1.0 + tol + -below == 1.0 and -below < -tol * 1.0
    pg, x, px, st = site_draw(items)
    assert st.tolist() == [1, 1, 1, 1, 2, 0, 0, 1, 1]
    for i in (0, 1, 2, 3, 4, 8):
        assert np.all(pg[i, :items[i]["d"]] == 0) and x[i] == 0 and px[i] == 0
    assert np.all(pg[7, :2] == 0) and x[7] == ISENT and px[7] == SENT.real
    assert pg[5, :2].tolist() == [1.0 + tol, 0.0] and x[5] == 0 and px[5] == 1.0 + tol
    assert pg[6, :2].tolist() == [0.5, 0.5] and x[6] == 1 and px[6] == 0.5


def test_site_draw_without_draw_leaves_x_and_px():
    rng = np.random.default_rng(9)
    part = _partial_of(rng.random(3) + 0.1, 2, rng)
    _, p = ref.draw_expect(part, 3, 1e-8)
    pg, x, px, st = site_draw([dict(partial=part, d=3, u=0.3, draw=0), dict(partial=part, d=3, u=0.3, draw=1), dict(partial=part, d=3, counter=(1, 2, 3), draw=0)])
    for i in range(3):
        assert np.array_equal(_bits(pg[i, :3]), _bits(p)) and st[i] == 0
    assert x[0] == ISENT and px[0] == SENT.real and x[2] == ISENT and px[2] == SENT.real
    assert x[1] == sr.draw(p, 0.3) and px[1] == p[x[1]]


def test_site_draw_counter_based_uniform_to_all_53_bits():
    """u is the mirror's value u_m exactly: diag = [u_m, 1 - u_m] (tr = 1 and cdf[0] = u_m exactly) gives x = 1 because u < cdf[0] fails, and diag = [u_m + 2^-53,
    1 - u_m - 2^-53] gives x = 0; a uniform that differs from u_m by one unit of 2^-53 either way fails one of the two"""
    triples = ref.counter_triples()
    items = []
    for t in triples:
        um = ref.counter_uniform(*t)
        assert 0.0 < um < 1.0 - 2.0 ** -53
        for v in (um, um + 2.0 ** -53):
            assert v + (1.0 - v) == 1.0 and (1.0 - v) + v == 1.0
            items.append(dict(partial=_row([v, 1.0 - v]), d=2, counter=t, u=0.0 if v == um else 0.999))      # (the explicit uniform must not matter)
    pg, x, px, st = site_draw(items)
    assert np.all(st == 0)
    for i, it in enumerate(items):
        assert pg[i, 0] == it["partial"][0, 0] and pg[i, 1] == it["partial"][0, 1]
    got = x.reshape(-1, 2)
    wrong = [(triples[i], got[i].tolist()) for i in range(len(triples)) if got[i].tolist() != [1, 0]]
    assert not wrong, wrong[:5]
    assert np.all(px.reshape(-1, 2)[:, 0] == pg[0::2, 1]) and np.all(px.reshape(-1, 2)[:, 1] == pg[1::2, 0])


# ---- site_project -------------------------------------------------------------------------------------------------------------------------------------------------------------
def site_project(psi, nout, d, x, on_device, dtype):
    out = Guarded([nout], ref.CT[dtype])
    rc = lib.tnqs_dbg_site_project(dtype, nout, d, _p(psi), x, int(on_device), _p(out.a), GUARD)
    assert rc == 0, (rc, lib.tnqs_last_error())
    out.check(True)
    return out.item(0)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("d", (1, 2, 3, 16))
def test_site_project_every_x_both_ways(d, dtype):
    rng = np.random.default_rng([d, dtype])
    for nout in (1, 255, 257):
        psi = np.ascontiguousarray((rng.standard_normal(nout * d) + 1j * rng.standard_normal(nout * d)).astype(ref.CT[dtype]))
        for x in range(-1, d + 1):                               # -1 and d clamp to the ends
            want = psi[min(max(x, 0), d - 1)::d]
            for on_device in (0, 1):
                got = site_project(psi, nout, d, x, on_device, dtype)
                assert np.array_equal(_bits(got), _bits(want)), (nout, d, x, on_device)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_site_project_grid_stride(dtype):
    """more outputs than the 4096 x 256 threads of the launch: the grid-stride path"""
    nout, d, x = 4096 * 256 + 3, (2, 3)[dtype], (1, 2)[dtype]
    rng = np.random.default_rng(dtype)
    psi = np.ascontiguousarray((rng.standard_normal(nout * d) + 1j * rng.standard_normal(nout * d)).astype(ref.CT[dtype]))
    got = site_project(psi, nout, d, x, 1 - dtype, dtype)
    assert np.array_equal(_bits(got), _bits(psi[x::d]))


# ---- site1 + norm_factor + scale ----------------------------------------------------------------------------------------------------------------------------------------------
GATES = {"A": np.array([[0.8 + 0.3j, -0.35 + 0.55j], [0.2 - 0.65j, 1.1 + 0.05j]]),      # not symmetric, all eight coefficients of different magnitude, none a float
         "I": np.eye(2, dtype=complex), "X": np.array([[0, 1], [1, 0]], dtype=complex),
         "N": np.array([[2.5 - 1.25j, 0.125j], [-3 + 0.75j, 0.0625 + 4j]])}              # not unitary
NPAIRS = (1, 2, 255, 256 * 64 + 1, 300007, 3)                                             # the last item is an all-zero tensor


def site1(xs, gates, nbx, normalize):
    n = len(xs)
    lens = [2 * len(x) for x in xs]
    out, parts, fac = Guarded(lens, np.complex64), Guarded([n * nbx], np.float64), Guarded([1] * n, np.float64)
    rc = lib.tnqs_dbg_site1(n, _p(_ints([len(x) for x in xs])), _p(np.ascontiguousarray(np.concatenate([x.reshape(-1) for x in xs]).astype(np.complex64))),
                            _p(_f64(np.concatenate([ref.gate_abi(g) for g in gates]))), nbx, int(normalize), _p(out.a), _p(parts.a), _p(fac.a), GUARD)
    assert rc == 0, (rc, lib.tnqs_last_error())
    out.check(); parts.check(True if normalize else False); fac.check(True if normalize else False)
    return [out.item(i).reshape(-1, 2).copy() for i in range(n)], parts.item(0).reshape(n, nbx).copy(), np.array([fac.item(i)[0] for i in range(n)])


def scale(srcs, factors, dtype):
    lens = [s.size for s in srcs]
    out = Guarded(lens, ref.CT[dtype])
    rc = lib.tnqs_dbg_scale(dtype, len(lens), _p(_ints(lens)), _p(np.ascontiguousarray(np.concatenate([s.reshape(-1) for s in srcs]).astype(ref.CT[dtype]))), _p(_f64(factors)),
                            _p(out.a), GUARD)
    assert rc == 0, (rc, lib.tnqs_last_error())
    out.check(True)
    return [out.item(i).copy() for i in range(len(lens))]


def _scaled_on_host(x, f, dtype):
    """(T)(factor) times the input, computed in T"""
    ft = ref.RT[dtype](f)
    x = np.ascontiguousarray(np.asarray(x).astype(ref.CT[dtype]).reshape(-1))
    return (x.view(ref.RT[dtype]) * ft).view(ref.CT[dtype])


def _site1_inputs():
    rng = np.random.default_rng(31)
    xs = [(rng.standard_normal((k, 2)) + 1j * rng.standard_normal((k, 2))).astype(np.complex64) for k in NPAIRS]
    xs[-1][:] = 0
    return xs


SITE1_X = _site1_inputs()


@pytest.mark.parametrize("rot", range(4))
@pytest.mark.parametrize("nbx", (1, 64))
def test_site1_gate_norm_partials_and_factors(nbx, rot):
    """one launch over tensors of different lengths, item i under gate (i + rot) mod 4: every length meets every gate over the four rotations"""
    names = [list(GATES)[(i + rot) % 4] for i in range(len(NPAIRS))]
    outs, parts, fac = site1(SITE1_X, [GATES[k] for k in names], nbx, True)
    pairs, npairs_, fpairs = [], [], []
    for x, k, o, pr, f in zip(SITE1_X, names, outs, parts, fac):
        want, bound = ref.site1(GATES[k], x)
        o128 = o.astype(np.complex128)
        pairs += [(np.abs(o128.real - want.real), bound), (np.abs(o128.imag - want.imag), bound)]
        if k == "I":
            assert np.array_equal(o, x)
        if k == "X":
            assert np.array_equal(o, x[:, ::-1])
        s_dev, s_ref = math.fsum(pr), ref.norm2_fsum(o)
        assert np.all(pr >= 0)
        npairs_.append((abs(s_dev - s_ref), ref.norm_partial_k(len(x), nbx) * ref.U53 * s_ref))
        if s_dev > 0:
            f_ref = float(1 / np.sqrt(ref.LD(s_dev)))
            fpairs.append((abs(f - f_ref), 2 * ref.ulp(f_ref)))
        else:
            assert f == 1.0 and not np.any(o)                    # an all-zero tensor keeps the factor 1
    assert fac[-1] == 1.0
    _measured(f"site1 nbx {nbx} rot {rot}", _worst(pairs))
    _measured(f"site1 norm partials nbx {nbx} rot {rot}", _worst(npairs_))
    _measured(f"norm_factor after site1 nbx {nbx} rot {rot}", _worst(fpairs))


def test_site1_without_normalize_leaves_partials_and_factors():
    xs = SITE1_X[:4]
    gs = [GATES[k] for k in ("A", "N", "A", "N")]
    outs, _, _ = site1(xs, gs, 64, False)                        # (site1() asserts that neither array was written)
    ref_outs, _, _ = site1(xs, gs, 64, True)
    for a, b in zip(outs, ref_outs):
        assert np.array_equal(_bits(a), _bits(b))


def test_site1_normalize_chain_gives_unit_norm():
    """site1 -> norm_factor -> scale as a normalising one-site gate runs them.  float: the factor rounds to f32 (2^-24 relative on the norm) and so does every element (2^-24
    on the norm at most): 3 2^-24 with the factor's own error.  double: factor to 2 ulp = 4 2^-53, the device's norm^2 to k 2^-53 (k / 2 on the norm), element rounding 2^-53"""
    names = ("A", "N", "X", "A", "N")
    xs = SITE1_X[:5]
    outs, parts, fac = site1(xs, [GATES[k] for k in names], 64, True)
    f32 = scale(outs, fac, 0)
    f64 = scale([o.astype(np.complex128) for o in outs], fac, 1)
    pairs32, pairs64 = [], []
    for x, o, f, a, b in zip(xs, outs, fac, f32, f64):
        assert np.array_equal(_bits(a), _bits(_scaled_on_host(o, f, 0)))
        assert np.array_equal(_bits(b), _bits(_scaled_on_host(o, f, 1)))
        pairs32.append((abs(math.sqrt(ref.norm2_fsum(a)) - 1), 3 * ref.U24))
        pairs64.append((float(abs(np.sqrt(ref.norm2_ld(b)) - 1)), (ref.norm_partial_k(len(x), 64) / 2 + 6) * ref.U53))
    _measured("unit norm after scale<float>", _worst(pairs32))
    _measured("unit norm after scale<double>", _worst(pairs64))


def test_norm_factor_direct():
    """1 / sqrt of the sum of any number of partials: the kernel's sum carries ceil(npart / 256) + 9 roundings (a thread's chain, 6 levels of the wave sum, the waves in order),
    half of that relative on the factor, + 3 for the square root, the division and the second-order terms; a sum that is not positive gives 1"""
    rng = np.random.default_rng(17)
    nps = [1, 2, 64, 255, 256, 257, 1000, 0, 3, 3, 5]
    ps = [rng.random(k) * 10.0 ** rng.integers(-6, 6) for k in nps]
    ps[8] = np.zeros(3); ps[9] = np.array([1.0, -3.0, 1.0]); ps[10] = np.array([4.0, 0.0, 0.0, 0.0, 0.0])
    fac = Guarded([1] * len(nps), np.float64)
    rc = lib.tnqs_dbg_norm_factor(len(nps), _p(_ints(nps)), _p(_f64(np.concatenate(ps))), _p(fac.a), GUARD)
    assert rc == 0, (rc, lib.tnqs_last_error())
    fac.check(True)
    f = [fac.item(i)[0] for i in range(len(nps))]
    assert f[7] == 1.0 and f[8] == 1.0 and f[9] == 1.0 and f[10] == 0.5
    pairs = []
    for k, p, g in list(zip(nps, ps, f))[:7]:
        want = float(1 / np.sqrt(ref.LD(math.fsum(p))))
        pairs.append((abs(g - want) / want, ((-(-k // 256) + 9) / 2 + 3) * ref.U53))
    _measured("norm_factor", _worst(pairs))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_scale_is_the_product_in_T_bit_for_bit(dtype):
    rng = np.random.default_rng(23 + dtype)
    lens = (1, 3, 255, 256 * 64 + 5, 70001)
    factors = (0.5, 1.0 / 3.0, -2.75, 1.2345678901234567e-3, 1.0000001)
    srcs = [(rng.standard_normal(k) + 1j * rng.standard_normal(k)).astype(ref.CT[dtype]) for k in lens]
    for got, s, f in zip(scale(srcs, factors, dtype), srcs, factors):
        assert np.array_equal(_bits(got), _bits(_scaled_on_host(s, f, dtype)))


# ---- inner_scalar -------------------------------------------------------------------------------------------------------------------------------------------------------------
SHAPES = ((1, 1), (2, 3), (3, 2), (16, 16), (17, 31), (64, 33), (64, 64))
RAW = ("absent", "zero", "set, normalize 0", "set, normalize 1")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_inner_scalar_every_branch_mixed_shapes_in_one_launch(dtype):
    """every combination of m / mr present or absent (a null message is the rectangular delta e % rows == e / rows), rawsum absent / zero / set with normalize 0 / 1, each scale
    factor absent or present, on every shape, all items in ONE launch.  Slots the kernel gets a null pointer for hold NaN"""
    rng = np.random.default_rng(41 + dtype)
    ct = ref.CT[dtype]
    items = []
    for (rows, cols), hm, hr, raw, ha, hb in itertools.product(SHAPES, (1, 0), (1, 0), range(4), (0, 1), (0, 1)):
        k = rows * cols
        m = (rng.standard_normal(k) + 1j * rng.standard_normal(k)).astype(ct) if hm else None
        mr = (rng.standard_normal(k) + 1j * rng.standard_normal(k)).astype(ct) if hr else None
        rs = None if raw == 0 else 0j if raw == 1 else complex(rng.standard_normal(), rng.standard_normal())
        items.append(dict(rows=rows, cols=cols, m=m, mr=mr, rawsum=rs, normalize=int(raw in (1, 3)), sa=rng.random() + 0.5 if ha else None, sb=-(rng.random() + 0.5) if hb else None))
    n = len(items)
    assert n == 7 * 64
    nan = lambda k: np.full(k, np.nan + 1j * np.nan, dtype=ct)
    M = np.ascontiguousarray(np.concatenate([it["m"] if it["m"] is not None else nan(it["rows"] * it["cols"]) for it in items]))
    MR = np.ascontiguousarray(np.concatenate([it["mr"] if it["mr"] is not None else nan(it["rows"] * it["cols"]) for it in items]))
    pres = _ints([[it["m"] is not None, it["mr"] is not None] for it in items]).reshape(-1)
    rawsum = _f64([[np.nan, np.nan] if it["rawsum"] is None else [it["rawsum"].real, it["rawsum"].imag] for it in items]).reshape(-1)
    sa = _f64([np.nan if it["sa"] is None else it["sa"] for it in items]); sb = _f64([np.nan if it["sb"] is None else it["sb"] for it in items])
    hs = _ints([[it["sa"] is not None, it["sb"] is not None] for it in items]).reshape(-1)
    out = Guarded([1] * n, np.complex128)
    rc = lib.tnqs_dbg_inner_scalar(dtype, n, _p(_ints([it["rows"] for it in items])), _p(_ints([it["cols"] for it in items])), _p(M), _p(MR), _p(pres), _p(rawsum),
                                   _p(_ints([it["rawsum"] is not None for it in items])), _p(_ints([it["normalize"] for it in items])), _p(sa), _p(sb), _p(hs), _p(out.a), GUARD)
    assert rc == 0, (rc, lib.tnqs_last_error())
    out.check(True)
    pairs = []
    for i, it in enumerate(items):
        want, are, aim = ref.inner_scalar(it["m"], it["mr"], it["rows"], it["cols"], it["rawsum"], it["normalize"], it["sa"], it["sb"])
        got = complex(out.item(i)[0])
        e, b = (abs(got.real - want.real), abs(got.imag - want.imag)), (ref.inner_bound(it["rows"], it["cols"], are), ref.inner_bound(it["rows"], it["cols"], aim))
        assert e[0] <= b[0] and e[1] <= b[1], ({k: v for k, v in it.items() if k not in ("m", "mr")}, got, want)
        pairs.append((np.array(e), np.array(b)))
    _measured(f"inner_scalar dtype {dtype}", _worst(pairs))


def test_inner_scalar_refuses_what_the_engine_refuses():
    out = Guarded([1], np.complex128)
    z = np.zeros(65 * 2, dtype=np.complex64)
    one = _ints([1]); two = _ints([1, 1]); f = _f64([1.0, 1.0])
    rc = lib.tnqs_dbg_inner_scalar(0, 1, _p(_ints([65])), _p(_ints([2])), _p(z), _p(z), _p(two), _p(f), _p(one), _p(one), _p(f), _p(f), _p(two), _p(out.a), GUARD)
    assert rc == -2
    rc = lib.tnqs_dbg_inner_scalar(0, 1, _p(_ints([0])), _p(_ints([2])), _p(z), _p(z), _p(two), _p(f), _p(one), _p(one), _p(f), _p(f), _p(two), _p(out.a), GUARD)
    assert rc == -1
    out.check(False)
