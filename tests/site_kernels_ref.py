"""Plain numpy / Python references of the sampling kernels (kernels_sample.hip: site_prob_partial, site_draw, site_project), the ComplexF32 d = 2 one-site gate with its
normalisation (kernels_util.hip: site1_c64, norm_factor, scale) and the form scalars (kernels_inner.hip: inner_scalar), for tests/test_gpu_site_kernels.py; pinned on the
CPU in tests/test_site_kernels_ref_cpu.py.  Each function restates the DOCUMENTED operation in extended precision (np.longdouble / math.fsum) and returns next to every
value the sum of the absolute values of the terms it adds up, which the tests' derived bounds need.  The draw rule is sampling_ref.draw: there is no second one here.
dtype: 0 = ComplexF32, 1 = ComplexF64 as in include/tnqs.h."""
import math

import numpy as np

CT = {0: np.complex64, 1: np.complex128}
RT = {0: np.float32, 1: np.float64}
LD = np.longdouble
U53 = 2.0 ** -53
U24 = 2.0 ** -24


# ---- site_prob_partial ----------------------------------------------------------------------------------------------------------------------------------------------------
def plan_site_prob(n, d):
    """the workgroups the engine launches for a site tensor of n elements (kernels_sample.hip plan_site_prob): 1024 elements per workgroup, at most 1024 workgroups"""
    return max(1, min(1024, (n + 1023) // 1024))


def owner(n, d, nblocks):
    """THE OWNERSHIP MAP.  Element e belongs to thread e mod NT (NT = the launch's thread count rounded down to a multiple of d) and to site index e mod d;
    -> (workgroup, site index) of every element"""
    NT = 256 * nblocks - (256 * nblocks) % d
    e = np.arange(n)
    return (e % NT) // 256, e % d


def diag_terms(tabs, psi):
    """the terms of diag[s] = sum_l Re(T[s, l] conj psi[s, l]), one per element, as longdouble (exact for float inputs: 24-bit x 24-bit products, two of them)"""
    a, b = np.asarray(tabs), np.asarray(psi)
    return a.real.astype(LD) * b.real.astype(LD) + a.imag.astype(LD) * b.imag.astype(LD)


def diag(tabs, psi, d):
    """diag[s] = sum_l Re(T[s, l] conj psi[s, l]) for flat arrays with the site index fastest -> (diag, sum of |terms|), d longdoubles each"""
    t = diag_terms(tabs, psi).reshape(-1, d)
    return t.sum(axis=0), np.abs(t).sum(axis=0)


def partials(tabs, psi, d, nblocks):
    """the nblocks x 16 partial array the kernel must leave, from the ownership map -> (partial, sum of |terms|), longdouble; slots s >= d are zero"""
    t = diag_terms(tabs, psi)
    blk, s = owner(t.size, d, nblocks)
    ref = np.zeros(nblocks * 16, dtype=LD); ab = np.zeros(nblocks * 16, dtype=LD)
    np.add.at(ref, blk * 16 + s, t); np.add.at(ab, blk * 16 + s, np.abs(t))
    return ref.reshape(nblocks, 16), ab.reshape(nblocks, 16)


def partial_bound(n, d, nblocks, absval):
    """|partial - ref| <= (ceil(n / NT) + ceil(256 / d) + 4) 2^-53 sum|terms|, a term being one element's Re(T conj psi): a thread's chain of ceil(n / NT) f64 additions, then
    the in-order sum of the ceil(256 / d) lanes of its site index.  For float inputs the two products of a term are exact doubles and their sum rounds once (part of the + 4, with
    the second-order terms).  For double inputs the products round as well, relative to each product and not to their sum: the + 4 holds them as long as the two products of a
    term do not cancel to less than a third of their magnitudes on a partial that has nothing else in it -- true of the fixed inputs of the test (worst ratio 0.47, at n = d = 16)"""
    NT = 256 * nblocks - (256 * nblocks) % d
    return (-(-n // NT) + -(-256 // d) + 4) * U53 * np.asarray(absval, dtype=np.float64)


def site_prob_cases(d):
    """(n, nblocks) of the GPU test for site dimension d; nblocks 0 = plan_site_prob.  One element per site index (also n < NT); one partly idle workgroup; one full workgroup whose
    threads loop; exactly 2 and 3 workgroups (n just above 1024 and 2048: the lanes of a site index start at another offset in every workgroup when d does not divide 256);
    1, 2 and 5 workgroups forced on the same data (5 workgroups of 1500 elements: n < NT again, with idle workgroups)"""
    return [(d, 0), (d * max(1, 150 // d), 0), (d * (1000 // d), 0), (d * (1024 // d + 1), 0), (d * (2048 // d + 1), 0),
            (d * (1500 // d), 1), (d * (1500 // d), 2), (d * (1500 // d), 5), (d * (5000 // d), 5)]


SITE_DIMS = (1, 2, 3, 5, 7, 16)
BIG_CASE = {0: (3 * (2 ** 20 // 3 + 1), 3), 1: (5 * (2 ** 20 // 5 + 1), 5)}        # dtype -> (n, d): n just above 2^20, the 1024-workgroup cap


def site_inputs(n, d, dtype, seed, scale=1.0):
    """T and psi of n = d k elements: entries of mixed sign, psi's magnitude per site index alternating by 10^6, so that mass moved between indices cannot hide"""
    rng = np.random.default_rng([seed, n, d, dtype])
    sc = np.tile(10.0 ** (-6.0 * (np.arange(d) % 2)), n // d)
    t = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * scale
    p = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * sc * scale
    return np.ascontiguousarray(t.astype(CT[dtype])), np.ascontiguousarray(p.astype(CT[dtype]))


# ---- site_draw ------------------------------------------------------------------------------------------------------------------------------------------------------------
M64 = (1 << 64) - 1


def mix64(x):
    """splitmix64's finaliser on 64-bit words (kernels_sample.hip sample_mix64)"""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def counter_uniform(seed, sample, step):
    """the counter-based uniform of site_draw_kernel: a function of (seed, sample, step) alone, 53 bits, in [0, 1)"""
    r = mix64((mix64((mix64(seed & M64) + 0xD1B54A32D192ED03 * (sample & M64)) & M64) + 0xC2B2AE3D27D4EB4F * (step & M64)) & M64)
    return (r >> 11) * 2.0 ** -53


def counter_triples():
    """about 200 (seed, sample, step): the ends of the range in every field, triples that differ in exactly one field, random 64-bit words"""
    ends = (0, 1, M64, M64 - 1, 1 << 63, 1 << 32)
    base = (0x0123456789ABCDEF, 7, 11)
    out = [(a, b, c) for a in (0, M64) for b in (0, M64) for c in (0, M64)]
    for k in range(3):
        for v in ends + tuple(range(2, 12)):
            t = list(base); t[k] = v; out.append(tuple(t))
    out = list(dict.fromkeys(out))                            # (the base triple itself turns up once per field)
    rng = np.random.default_rng(2024)
    w = rng.integers(0, 1 << 63, size=(200 - len(out), 3), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(200 - len(out), 3), dtype=np.uint64)
    out += [tuple(int(x) for x in row) for row in w]
    return out


def seq_sum(values):
    """the f64 sum in index order, starting from 0.0 -- what a sequential device loop computes (np.sum adds pairwise)"""
    s = 0.0
    for v in values:
        s = s + float(v)
    return s


def draw_expect(partial, d, neg_tol):
    """what site_draw_kernel must leave for a host-built nblocks x 16 partial array, bit for bit: (status, p).  diag and tr are sequential f64 sums, p = max(diag, 0) / tr;
    any bad status: p = 0"""
    partial = np.asarray(partial, dtype=np.float64).reshape(-1, 16)
    dg = [seq_sum(partial[:, j]) for j in range(d)]
    tr = seq_sum(dg)
    status = 0
    if not (tr > 0) or not (tr <= 1.79769313486231570e308):
        status = 1
    else:
        status = 2 if any(x < -neg_tol * tr for x in dg) else 0
    if status:
        return status, np.zeros(d)
    return 0, np.array([(0.0 if x < 0 else x) / tr for x in dg], dtype=np.float64)


# ---- site1 + norm_factor + scale ----------------------------------------------------------------------------------------------------------------------------------------------
def gate_abi(G):
    """a 2 x 2 gate G[s', s] as the C ABI takes it: column-major G[s' + 2 s], (re, im) doubles"""
    G = np.asarray(G, dtype=np.complex128)
    return np.ascontiguousarray(np.stack([G.ravel(order="F").real, G.ravel(order="F").imag], axis=1).ravel())


def site1(G, x):
    """out[i, s'] = sum_s G[s', s] x[i, s] in complex128 for x of shape (npairs, 2) -> (out, bound): per real component
        |device - out| <= 8 2^-24 sum_s |G[s', s]| |x[i, s]| + sum_s (|dRe G| + |dIm G|)[s', s] |x[i, s]|
    The kernel works with fl32(G): every coefficient moves by dG = G - fl32(G) (second term, computed exactly here).  A real component is a sum of four products
    g a with sum |g a| <= sum_s |G[s', s]| |x[i, s]| (Cauchy-Schwarz on (re, im)); products and the three additions round to nearest in f32 in any order, fused or not:
    at most 4 roundings on any term, gamma_4 = 4 u / (1 - 4 u) < 8 u with u = 2^-24"""
    G = np.asarray(G, dtype=np.complex128); x = np.asarray(x).astype(np.complex128)
    Gf = G.real.astype(np.float32).astype(np.float64) + 1j * G.imag.astype(np.float32).astype(np.float64)
    dG = np.abs(G.real - Gf.real) + np.abs(G.imag - Gf.imag)
    out = x @ G.T
    ax = np.abs(x)
    return out, 8 * U24 * (ax @ np.abs(G).T) + ax @ dG.T


def norm2_fsum(x):
    """sum of |x|^2 by math.fsum; exact for complex64 x (the squares of floats are exact doubles)"""
    x = np.asarray(x)
    r, i = x.real.astype(np.float64).ravel(), x.imag.astype(np.float64).ravel()
    return math.fsum(np.concatenate([r * r, i * i]))


def norm2_ld(x):
    """sum of |x|^2 as a longdouble (for complex128 x)"""
    x = np.asarray(x)
    return np.sum(x.real.astype(LD) ** 2) + np.sum(x.imag.astype(LD) ** 2)


def norm_partial_k(npairs, nbx):
    """the roundings on any term of a workgroup's norm partial: 4 additions per pair of a thread's chain of ceil(npairs / (256 nbx)) pairs, 6 levels of the wave sum,
    the 4 waves in order, + 2 for the second-order terms"""
    return 4 * -(-npairs // (256 * nbx)) + 12


def ulp(x):
    return float(np.spacing(np.float64(abs(x))))


# ---- inner_scalar -------------------------------------------------------------------------------------------------------------------------------------------------------------
def delta(rows, cols):
    """the rectangular identity a null message stands for, flat [a + rows b]: 1 where e % rows == e // rows"""
    e = np.arange(rows * cols)
    return (e % rows == e // rows).astype(np.float64)


def inner_scalar(m, mr, rows, cols, rawsum, normalize, scale_a, scale_b):
    """sum_e m[e] mr[e] over flat rows x cols messages (None = the rectangular identity) in extended precision; times rawsum when one is given, normalize is set and it is not
    exactly zero; times the scale factors given -> (value complex128, sum|terms| of the real part, of the imaginary part)"""
    x = (delta(rows, cols) if m is None else np.asarray(m)).astype(np.clongdouble)
    y = (delta(rows, cols) if mr is None else np.asarray(mr)).astype(np.clongdouble)
    re = np.sum(x.real * y.real) - np.sum(x.imag * y.imag); im = np.sum(x.real * y.imag) + np.sum(x.imag * y.real)
    are = np.sum(np.abs(x.real * y.real) + np.abs(x.imag * y.imag)); aim = np.sum(np.abs(x.real * y.imag) + np.abs(x.imag * y.real))
    if rawsum is not None and normalize and complex(rawsum) != 0:
        sr, si = LD(complex(rawsum).real), LD(complex(rawsum).imag)
        re, im, are, aim = re * sr - im * si, re * si + im * sr, are * abs(sr) + aim * abs(si), are * abs(si) + aim * abs(sr)
    f = LD(1)
    for s in (scale_a, scale_b):
        if s is not None:
            f = f * LD(s)
    return complex(float(re * f), float(im * f)), float(are * abs(f)), float(aim * abs(f))


def inner_bound(rows, cols, absval):
    """8 (k + 4) 2^-53 sum|terms| with k = rows cols, the convention of bp_post_ref.bound for an f64 result"""
    return 8.0 * (rows * cols + 4) * U53 * absval
