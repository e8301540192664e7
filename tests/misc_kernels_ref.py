"""Plain numpy restatements (np.longdouble / math.fsum) of the small kernels tests/test_gpu_misc_kernels.py reaches through csrc/debug_misc.cpp, each written from
the kernel's one-line description, and the inputs both that test and tests/test_misc_kernels_ref_cpu.py build (the CPU test checks the conditions the bounds assume).

Bounds.  u = 2^-53.  A sum of f64 terms that a kernel forms thread by thread, then over a wave (6 butterfly steps), then over the waves of a workgroup (one thread adds
them in turn) is within depth u sum|terms| of the exact sum of the same terms, depth = the number of roundings a term can pass through (first order; the inputs here keep
depth u below 1e-13, so the second-order part is far below the factor two the tests keep in hand): terms per thread + 6 + waves per workgroup, + 2 where a term is one
of the two real products of a complex product (the product and the difference), and the same again (without the + 2) for a tail kernel that sums the workgroups'
partials.  The terms are formed from the stored, already rounded inputs.

C_LIBM is the device libm's error in units of 2^-53 for log, hypot, atan2, sincospi and sqrt.  The ROCm tree carries no OCML accuracy document, so it is measured: the
worst error of one-term amp_scalar items (chi = 1, |z| in [1/4, 4]) and of random_fill's elements against the extended-precision restatement, times 4 and not below 4.
Measured on an MI355X: see C_MEASURED below and DESIGN.md."""
import math

import numpy as np

U53 = 2.0 ** -53
C_MEASURED = {"one-term log|z|": 2.379, "one-term phase / pi": 1.240, "random_fill": 2.046}      # worst seen on an MI355X, units of 2^-53 (tests/test_gpu_misc_kernels.py prints them)
C_LIBM = 10.0                                                                                       # 4 x 2.379, rounded up
LD = np.longdouble
CLD = np.clongdouble


def u_of(dtype):
    return 2.0 ** -24 if np.dtype(dtype) == np.complex64 else U53


# ---- permutation, identity ------------------------------------------------------------------------------------------------------------------------------------------
def ramp(n, dtype):
    """element e = e + i (e + 0.5): every misplaced element shows (exact in both types below 2^23 elements)"""
    e = np.arange(n, dtype=np.float64)
    return (e + 1j * (e + 0.5)).astype(dtype)


def permute_ref(x, dims_out, stride_in):
    """out[idx_0 + dims_out[0] (idx_1 + ...)] = x[sum_k idx_k stride_in[k]]"""
    off = np.zeros(tuple(dims_out), dtype=np.int64)
    for k, (d, s) in enumerate(zip(dims_out, stride_in)):
        shp = [1] * len(dims_out)
        shp[k] = d
        off = off + (np.arange(d, dtype=np.int64) * s).reshape(shp)
    return x[off.ravel(order="F")]


def strides_of(shape):
    """column-major element strides"""
    out, acc = [], 1
    for d in shape:
        out.append(acc)
        acc *= d
    return out


def permute_args(shape_in, perm):
    """(dims_out, stride_in) of out = transpose(in, perm), both column-major: output leg k is input leg perm[k]"""
    st = strides_of(shape_in)
    return [shape_in[p] for p in perm], [st[p] for p in perm]


PERM_SHAPES = {1: (7,), 2: (3, 5), 3: (2, 3, 5), 4: (2, 3, 5, 7), 5: (2, 3, 5, 7, 11), 6: (2, 3, 5, 7, 11, 13), 7: (2, 3, 5, 2, 3, 5, 7), 8: (2, 3, 2, 3, 2, 5, 2, 3)}
PERM_ONES = [(3, 1, 5), (1, 3, 1, 1, 5, 1, 2), (1, 1, 1), (2, 1, 3, 1, 5, 1, 7, 1)]      # dimension-1 legs between others
PERM_LARGE = (2, 3, 5, 7, 11, 13, 17, 4)                                                  # 2,042,040 elements > 4096 x 256: the grid-stride loop runs (a last leg of 2 would stay below)


def perms_of(rank):
    """the identity, the full reversal, a cyclic shift and two seeded random permutations"""
    rng = np.random.default_rng(rank)
    ident = list(range(rank))
    out = [ident, ident[::-1], ident[1:] + ident[:1]]
    out += [list(rng.permutation(rank)) for _ in range(2)]
    return out


# ---- random fill ------------------------------------------------------------------------------------------------------------------------------------------------------
def splitmix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def random_fill_ref(index, seed, scale, real_only=False):
    """entry e <- splitmix64(seed + 0xD1B54A32D192ED03 e) -> u1 = (high 32 bits + 1) / 2^32, u2 = low 32 bits / 2^32 -> Box-Muller: sqrt(-2 ln u1) scale (cos, sin)(2 pi u2).
    Returns (re, im, rad) in np.longdouble, rad without the scale"""
    e = np.asarray(index, dtype=np.uint64)
    with np.errstate(over="ignore"):
        r = splitmix64(np.uint64(seed) + np.uint64(0xD1B54A32D192ED03) * e)
    u1 = ((r >> np.uint64(32)).astype(LD) + LD(1)) / LD(4294967296)
    u2 = (r & np.uint64(0xFFFFFFFF)).astype(LD) / LD(4294967296)
    rad = np.sqrt(LD(-2) * np.log(u1))
    two_pi = LD(8) * np.arctan(LD(1))
    re = rad * LD(scale) * np.cos(two_pi * u2)
    im = np.zeros_like(re) if real_only else rad * LD(scale) * np.sin(two_pi * u2)
    return re, im, rad


FILL_STATS_N = 1 << 20
FILL_STATS_SEED = 20240607


def fill_stats(re, im, scale):
    """(|mean re| / (scale / sqrt n), |mean im| / (scale / sqrt n), |var / scale^2 - 1| / sqrt(2 / n), |corr| / (1 / sqrt n)): each is held to 5"""
    re = np.asarray(re, dtype=np.float64)
    im = np.asarray(im, dtype=np.float64)
    n = re.size
    var = 0.5 * (np.mean(re * re) + np.mean(im * im))      # the variance per part about the true mean 0 (2 n samples, so sqrt(2 / (2 n)) would do; the bound keeps sqrt(2 / n))
    corr = np.mean(re * im) / np.sqrt(np.mean(re * re) * np.mean(im * im))
    rn = math.sqrt(n)
    return abs(np.mean(re)) * rn / scale, abs(np.mean(im)) * rn / scale, abs(var / scale ** 2 - 1) / math.sqrt(2.0 / n), abs(corr) * rn


# ---- sums, dots, norms ------------------------------------------------------------------------------------------------------------------------------------------------
def sum_ref(x):
    return math.fsum(float(t) for t in x)


def sum_depth(n):
    return -(-max(n, 1) // 256) + 6 + 4


def sum_inputs(n):
    rng = np.random.default_rng(1000 + n)
    return rng.standard_normal(n) * np.exp(3 * rng.standard_normal(n))      # mixed signs, magnitudes over several decades


def dot_ref(x, y):
    """sum_e x[e] y[e] (bilinear) in extended precision and the sum of the absolute values of the real products that make up either part"""
    xr, xi, yr, yi = (np.asarray(t, dtype=LD) for t in (x.real, x.imag, y.real, y.imag))
    re = np.sum(xr * yr) - np.sum(xi * yi)
    im = np.sum(xr * yi) + np.sum(xi * yr)
    mag_re = float(np.sum(np.abs(xr * yr)) + np.sum(np.abs(xi * yi)))
    mag_im = float(np.sum(np.abs(xr * yi)) + np.sum(np.abs(xi * yr)))
    return re, im, mag_re, mag_im


def loop_dot_nwg(n):
    return max(1, min(-(-n // 4096), 1024))


def loop_dot_depth(n):
    nwg = loop_dot_nwg(n)
    return (-(-max(n, 1) // (256 * nwg)) + 6 + 4 + 2) + (-(-nwg // 256) + 6 + 4)


DOT_LENGTHS = [1, 255, 4096, 4097, 300001, 4096 * 1024 + 4097]
DOT_CAP = 2.0


def dot_inputs(n, dtype, seed=0):
    """x = a e^{i t}, y = b e^{-i t + small}: the products stay near the positive real axis, so sum|x||y| / |sum x y| <= DOT_CAP and the bound means something
    relative to the result"""
    rng = np.random.default_rng([seed, n])
    t = rng.uniform(-np.pi, np.pi, n)
    x = (1 + 0.3 * rng.uniform(-1, 1, n)) * np.exp(1j * t)
    y = (1 + 0.3 * rng.uniform(-1, 1, n)) * np.exp(-1j * t + 0.4j * rng.uniform(-1, 1, n))
    return x.astype(dtype), y.astype(dtype)


def cancellation(x, y):
    """sum|x||y| / |sum x y|"""
    re, im, _, _ = dot_ref(x, y)
    return float(np.sum(np.abs(x).astype(LD) * np.abs(y).astype(LD)) / np.hypot(re, im))


def norm_ref(x):
    xr, xi = np.asarray(x.real, dtype=LD), np.asarray(x.imag, dtype=LD)
    return np.sqrt(np.sum(xr * xr) + np.sum(xi * xi))


def norm_depth(n):
    """a term is one square: the product, the sum of the pair, then the thread's, the wave's and the 16 waves' additions"""
    return 2 + -(-n // 1024) + 6 + 16


NORM_LENGTHS = [1, 1023, 1024, 1025, 70000]


def norm_inputs(n, dtype, scale=1.0, seed=0):
    rng = np.random.default_rng([seed, n, 17])
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * scale).astype(dtype)


# ---- record packing ---------------------------------------------------------------------------------------------------------------------------------------------------
def record_ref(info, terr, S, x2, x2_off, nbytes, fill):
    """the record of one gate: (info[2], info[3], terr, 0) as doubles | S | ... | X2 at byte x2_off; every other byte keeps `fill`"""
    rec = np.full(nbytes, fill, dtype=np.uint8)
    rec[:32] = np.array([info[2], info[3], terr, 0.0], dtype=np.float64).view(np.uint8)
    rec[32:32 + 8 * len(S)] = np.asarray(S, dtype=np.float64).view(np.uint8)
    rec[x2_off:x2_off + 8 * len(x2)] = np.asarray(x2, dtype=np.uint64).view(np.uint8)
    return rec


# ---- the end of an amplitude sweep ------------------------------------------------------------------------------------------------------------------------------------
def sweep_end_ref(diffs, iter_, tol, done, niter, fdiff):
    """per string that is not done: fdiff = (diffs added in the order t = 0 .. nseq - 1) / nseq in f64, niter = iter, done when tol >= 0 and fdiff <= tol"""
    nseq, nstr = diffs.shape
    done, niter, fdiff = done.copy(), niter.copy(), fdiff.copy()
    for n in range(nstr):
        if done[n]:
            continue
        s = np.float64(0)
        for t in range(nseq):
            s = s + diffs[t, n]
        avg = s / np.float64(nseq)
        niter[n] = iter_
        fdiff[n] = avg
        if tol >= 0 and avg <= tol:
            done[n] = 1
    return done, niter, fdiff


# ---- vertex and edge scalars and their log sum ------------------------------------------------------------------------------------------------------------------------
class ScalarItem:
    """one vertex or edge scalar for every string: sum_j m[j, n] mr[j, n] (an absent array: ones), times rawsum[n] when `normalize` and rawsum[n] != 0, times scale;
    site (a vector): an isolated vertex whose value is site[cfg[n, vertex]]"""

    def __init__(self, chi, m=None, mr=None, rawsum=None, normalize=False, scale=None, site=None):
        self.chi, self.m, self.mr, self.rawsum, self.normalize, self.scale, self.site = chi, m, mr, rawsum, normalize, scale, site


def item_values(items, cfg):
    """(values [item][string] in np.clongdouble, kappa [item][string] = sum|m||mr| / |sum m mr| (1 for an isolated vertex))"""
    nstr = cfg.shape[0]
    vals = np.zeros((len(items), nstr), dtype=CLD)
    kap = np.ones((len(items), nstr), dtype=np.float64)
    for i, it in enumerate(items):
        if it.site is not None:
            v = np.asarray(it.site).astype(CLD)[cfg[:, i]]
        else:
            m = np.ones((it.chi, nstr), dtype=CLD) if it.m is None else np.asarray(it.m).astype(CLD)
            mr = np.ones((it.chi, nstr), dtype=CLD) if it.mr is None else np.asarray(it.mr).astype(CLD)
            with np.errstate(invalid="ignore", over="ignore"):
                v = np.sum(m * mr, axis=0)
                a = np.sum(np.abs(m) * np.abs(mr), axis=0)
            with np.errstate(divide="ignore", invalid="ignore"):
                kap[i] = np.where(np.abs(v) > 0, a / np.abs(v), np.inf).astype(np.float64)
            if it.rawsum is not None and it.normalize:
                rs = np.asarray(it.rawsum).astype(CLD)
                v = np.where(rs != 0, v * rs, v)
        if it.scale is not None:
            v = v * LD(it.scale)
        vals[i] = v
    return vals, kap


def scalar_ref(items, nv, cfg):
    """per string: sum over the vertex items of log(value) minus the sum over the edge items, as (log|.|, phase wrapped into (-pi, pi]); flag 1 where an item is exactly
    zero -> (-inf, 0), flag 2 where one is not finite -> (nan, nan).  Returns (re, im) in np.longdouble, flags, and per string sum_i |phase_i|"""
    vals, _ = item_values(items, cfg)
    nstr = cfg.shape[0]
    pi = LD(4) * np.arctan(LD(1))
    re, im, flags, phase_mag = np.zeros(nstr, dtype=LD), np.zeros(nstr, dtype=LD), np.zeros(nstr, dtype=np.int32), np.zeros(nstr)
    for n in range(nstr):
        lr, li = LD(0), LD(0)
        for i in range(len(items)):
            v = vals[i, n]
            if not (np.isfinite(v.real) and np.isfinite(v.imag)):
                flags[n] |= 2
                continue
            if v == 0:
                flags[n] |= 1
                continue
            sgn = 1 if i < nv else -1
            ph = np.arctan2(v.imag, v.real)
            lr += sgn * np.log(np.hypot(v.real, v.imag))
            li += sgn * ph
            phase_mag[n] += abs(float(ph))
        if flags[n] & 2:
            re[n], im[n] = np.nan, np.nan
        elif flags[n] & 1:
            re[n], im[n] = -np.inf, 0
        else:
            li = li - 2 * pi * np.round(li / (2 * pi))
            if li <= -pi:
                li += 2 * pi
            if li > pi:
                li -= 2 * pi
            re[n], im[n] = lr, li
    return re, im, flags, phase_mag


def items_of_cache(ac, normalize=True):
    """the items tnqs_amplitudes_bp hands the kernel for ONE string, from an amplitude_ref.AmpCache: per vertex the normalised message towards its first neighbour, the
    message coming back and the raw element sum (an isolated vertex: the site vector); per edge both messages.  Returns (items, nv, cfg)"""
    import amplitude_ref as amp
    g = ac.g
    items = []
    for v in g.vertices:
        if not g.nbrs[v]:
            items.append(ScalarItem(1, site=np.array([ac.A[v]]).ravel()))
            continue
        w = g.nbrs[v][0]
        raw = amp.raw_message(ac, (v, w))
        s = raw.sum()
        m = raw / s if (normalize and s != 0) else raw
        items.append(ScalarItem(len(raw), m=m.reshape(-1, 1), mr=ac.message((w, v)).reshape(-1, 1), rawsum=np.array([s]), normalize=normalize))
    for e in g.edges:
        items.append(ScalarItem(len(ac.message(e)), m=ac.message(e).reshape(-1, 1), mr=ac.message((e[1], e[0])).reshape(-1, 1)))
    return items, len(g.vertices), np.zeros((1, len(g.vertices)), dtype=np.int32)


KAPPA_CAP = 4.0
SCALAR_STRINGS = [1, 3, 4, 5, 9]
SCALAR_PAD = 3                 # ld = nv + SCALAR_PAD
ZERO_STRING, INF_STRING, BOTH_STRING = 1, 3, 4      # the strings (where the launch has them) on which an item is exactly zero / infinite / both happen


def _phased(rng, chi, nstr, phase, dtype, other=True):
    """m, mr [chi][nstr] whose products all have a phase within 0.1 of `phase`: kappa stays near 1"""
    a = rng.uniform(0.5, 1.5, (chi, nstr)) / chi
    p = phase + rng.uniform(-0.1, 0.1, (chi, nstr))
    if not other:
        return (a * np.exp(1j * p)).astype(dtype), None
    q = rng.uniform(-1.0, 1.0, (chi, nstr))
    return (a * np.exp(1j * (p - q))).astype(dtype), (rng.uniform(0.5, 1.5, (chi, nstr)) * np.exp(1j * q)).astype(dtype)


def scalar_case(nstr, dtype):
    """(items, nv, ne, cfg [nstr][ld]) of the amp_scalar launch: vertex items with phases near +3, edge items near -3 (the running sum of the phases passes +-2 pi
    several times), every null-pointer form, rawsum forms, scale factors, isolated vertices with d = 2 and 3, exactly negative real items, and the flag strings"""
    rng = np.random.default_rng([nstr, 5])
    V, E = [], []
    m, mr = _phased(rng, 1, nstr, 3.0, dtype); V.append(ScalarItem(1, m, mr))
    m, _ = _phased(rng, 2, nstr, 3.0, dtype, other=False); V.append(ScalarItem(2, m, None))
    m, _ = _phased(rng, 63, nstr, 3.0, dtype, other=False); V.append(ScalarItem(63, None, m))
    m, mr = _phased(rng, 64, nstr, 2.0, dtype)
    V.append(ScalarItem(64, m, mr, rawsum=rng.uniform(0.5, 2, nstr) * np.exp(1j * rng.uniform(0.9, 1.1, nstr)), normalize=True))
    V.append(ScalarItem(64))                                                                                      # both null: the value is chi
    m, mr = _phased(rng, 2, nstr, 3.0, dtype)
    V.append(ScalarItem(2, m, mr, rawsum=np.full(nstr, 1e30 - 7e29j), normalize=False))                           # normalize off: the rawsum is not used
    m, mr = _phased(rng, 63, nstr, 3.0, dtype)
    rs = rng.uniform(0.5, 2, nstr) * np.exp(0.05j * rng.uniform(-1, 1, nstr)); rs[::2] = 0                         # an exactly zero rawsum: the item stays as it is
    V.append(ScalarItem(63, m, mr, rawsum=rs, normalize=True))
    V.append(ScalarItem(1, site=(np.array([1.5, 0.75]) * np.exp(3j)).astype(dtype)))                               # isolated vertices, d = 2 and 3
    V.append(ScalarItem(1, site=(np.array([0.5, 2.0, 1.25]) * np.exp(np.array([3j, 2.9j, -3.1j]))).astype(dtype)))
    V.append(ScalarItem(1, np.full((1, nstr), -2.0, dtype=dtype), np.full((1, nstr), 1.5, dtype=dtype)))            # exactly negative real: phase exactly pi
    m, mr = _phased(rng, 4, nstr, 3.0, dtype); V.append(ScalarItem(4, m, mr, scale=0.37))
    m, mr = _phased(rng, 5, nstr, 3.0, dtype)                                                                      # the flag item
    if nstr > ZERO_STRING:
        m[:, ZERO_STRING] = 0
    if nstr > INF_STRING:
        m[2, INF_STRING] = np.inf
    if nstr > BOTH_STRING:
        m[0, BOTH_STRING] = np.inf
    V.append(ScalarItem(5, m, mr))
    for chi in (1, 2, 63, 64):
        m, mr = _phased(rng, chi, nstr, -3.0, dtype); E.append(ScalarItem(chi, m, mr))
    E.append(ScalarItem(1, np.full((1, nstr), 0.5, dtype=dtype), np.full((1, nstr), -3.0, dtype=dtype)))            # exactly negative real
    m, mr = _phased(rng, 3, nstr, -3.0, dtype); E.append(ScalarItem(3, m, mr, scale=2.5))
    m, mr = _phased(rng, 7, nstr, -3.0, dtype)
    if nstr > BOTH_STRING:
        mr[:, BOTH_STRING] = 0                                                                                     # zero here, infinite in the vertex item: flag 3
    E.append(ScalarItem(7, m, mr))
    nv, ne = len(V), len(E)
    cfg = np.full((nstr, nv + SCALAR_PAD), -1, dtype=np.int32)                                                      # -1: never read
    for i, it in enumerate(V):
        if it.site is not None:
            cfg[:, i] = rng.integers(0, len(it.site), nstr)
    return V + E, nv, ne, cfg


def scalar_bound(items, cfg, C=None):
    """per string sum_items (chi + C) 2^-53 kappa_i over the items that raise no flag"""
    C = C_LIBM if C is None else C
    _, kap = item_values(items, cfg)
    chi = np.array([it.chi for it in items], dtype=np.float64).reshape(-1, 1)
    k = np.where(np.isfinite(kap), kap, 0.0)
    return np.sum((chi + C) * U53 * k, axis=0)


def one_term_case(nstr, dtype, seed=3):
    """chi = 1 items with |z| in [1/4, 4] and any phase, one vertex item per launch entry: what C_LIBM is measured on"""
    rng = np.random.default_rng(seed)
    z = (rng.uniform(0.25, 4, (1, nstr)) * np.exp(1j * rng.uniform(-np.pi, np.pi, (1, nstr)))).astype(dtype)
    return [ScalarItem(1, z, None)], 1, 0, np.full((nstr, 1), -1, dtype=np.int32)
