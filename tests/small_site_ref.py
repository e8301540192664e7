"""float64 reference of the BP message of one site and of the message epilogue, for the kernel-level tests of bp_small_site_kernel and msg_finalize_kernel
(tests/test_gpu_small_site.py), pinned against the oracle in tests/test_small_site_ref_cpu.py.  Also: a complex64 restatement of the same steps, used ONLY to size
the tolerance of those tests, and the shapes and inputs both test modules share.

Conventions: a site tensor is a numpy array with axes (s, l_0 .. l_{z-1}); the message entering through leg k is m_k[l_k, l_k'] (ket index first); the outgoing
message is out[b, b'] = sum psi[s, .. b ..] prod_k m_k[l_k, l_k'] conj(psi[s, .. b' ..]).  On the device all of them are column-major (flat / unflat below)."""
import functools
import itertools

import numpy as np

LETTERS = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"


def r32(x):
    """the float64 value of the complex64 rounding of x: what the kernel is given"""
    return np.asarray(x).astype(np.complex64).astype(np.complex128)


def message(psi, Ms, jo):
    """raw message through leg jo in complex128 on the f32-rounded inputs; Ms[k] None = not present (identity); Ms[jo] is ignored"""
    psi = r32(psi)
    z = psi.ndim - 1
    ket = list(LETTERS[:z + 1])                       # s, l_0 ..
    bra = list(ket)
    ops, subs = [psi], ["".join(ket)]
    for k in range(z):
        if k == jo:
            bra[k + 1] = LETTERS[26 + k]
        elif Ms[k] is not None:
            bra[k + 1] = LETTERS[26 + k]
            ops.append(r32(Ms[k])); subs.append(ket[k + 1] + bra[k + 1])
    ops.append(psi.conj()); subs.append("".join(bra))
    return np.einsum(",".join(subs) + "->" + ket[jo + 1] + bra[jo + 1], *ops, optimize="greedy")


def message_c64(psi, Ms, jo):
    """the same message in numpy complex64 arithmetic, in the kernel's steps: absorb leg by leg, then the Gram with conj(psi).  Sizes tolerances, nothing else"""
    psi = np.asarray(psi).astype(np.complex64)
    t = psi
    for k in range(psi.ndim - 1):
        if k != jo and Ms[k] is not None:
            t = np.moveaxis(np.tensordot(t, np.asarray(Ms[k]).astype(np.complex64), axes=([k + 1], [0])), -1, k + 1)
    other = [a for a in range(psi.ndim) if a != jo + 1]
    out = np.tensordot(t, psi.conj(), axes=(other, other))
    assert out.dtype == np.complex64
    return out


def message_bound(psi, Ms, jo):
    """a-priori bound on the f32 rounding error of any summation order, relative to max|message|: (n_terms + z) 2^-24 (|psi| x |M| .. x |psi|) / max|message|,
    n_terms = the terms one output element sums sequentially at most (the legs' dimensions and the rest index of the Gram)"""
    z = psi.ndim - 1
    ap = np.abs(r32(psi))
    am = [None if (m is None or k == jo) else np.abs(r32(m)) for k, m in enumerate(Ms)]
    n_terms = sum(psi.shape[k + 1] for k in range(z) if k != jo and am[k] is not None) + psi.size // psi.shape[jo + 1]
    absval = message(ap, am, jo).real
    return (n_terms + z) * 2.0 ** -24 * np.max(absval) / np.max(np.abs(message(psi, Ms, jo)))


def message_diff(a, b):
    """1 - |<a, b>|^2 / (|a|^2 |b|^2) in float64"""
    a = np.asarray(a, dtype=np.complex128).ravel(); b = np.asarray(b, dtype=np.complex128).ravel()
    dot = np.sum(a.conj() * b)
    return float(1.0 - (dot.real ** 2 + dot.imag ** 2) / (np.sum(np.abs(a) ** 2) * np.sum(np.abs(b) ** 2)))


def finalize(raw, old, normalize):
    """(m, diff): m = raw / sum(raw) unless normalize is off or the sum is exactly zero; diff = message_diff(m, old), old None = identity"""
    m = np.asarray(raw, dtype=np.complex128)
    if normalize:
        s = m.sum()
        if s != 0:
            m = m / s
    return m, message_diff(m, np.eye(m.shape[0]) if old is None else old)


def conditioning(raw):
    """|sum(m)| / sum|m|: how much of the normalising sum survives its cancellation"""
    return float(abs(np.sum(raw)) / np.sum(np.abs(raw)))


def rel_err(got, ref):
    return float(np.max(np.abs(np.asarray(got, dtype=np.complex128) - ref)) / np.max(np.abs(ref)))


def flat(a):
    return np.ascontiguousarray(np.asarray(a).ravel(order="F"))


def unflat(v, n):
    return np.asarray(v).reshape((n, n), order="F")


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------------------------
def crandn(rng, shape):
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)).astype(np.complex64)


def inputs(d, chis, tag=0, psd_like=False):
    """complex random site tensor and one distinct complex matrix per leg: non-Hermitian random ones, or (psd_like, for the epilogue cases, whose normalising
    sum must not cancel) A A^dagger / chi + 0.1 random"""
    rng = np.random.default_rng([d, len(chis), tag] + list(chis))
    psi = crandn(rng, (d,) + tuple(chis))
    Ms = []
    for c in chis:
        if psd_like:
            a = crandn(rng, (c, c)).astype(np.complex128)
            Ms.append((a @ a.conj().T / c + 0.1 * crandn(rng, (c, c))).astype(np.complex64))
        else:
            Ms.append(crandn(rng, (c, c)))
    return psi, Ms


def masked(Ms, present):
    return [m if p else None for m, p in zip(Ms, present)]


# the scalar form's shapes (d, leg dimensions): z = 1 .. 8, d = 1 .. 4, odd and mixed legs, a leg of dimension 1, exactly 64 and exactly 8192 elements, and as
# OUTGOING leg every dimension at which the final Gram's slice count changes its case: nsl = clamp(1024 / co^2, 1, 16) is 16 (clamped) for co <= 8, does not divide
# 1024 for co in {9, 10, 12, 13, 17, 18}, is 4 at 16, 2 at 22, 1 from 23 on, and no = 1024 exactly at 32
SCALAR_SHAPES = [
    (4, (32,)), (2, (32,)),
    (2, (8, 8)), (3, (22, 23)), (1, (31, 32)),
    (2, (9, 10, 12)), (2, (13, 17, 18)), (2, (32, 4, 32)), (1, (32, 32, 8)), (4, (1, 16, 3)), (2, (2, 4, 4)),
    (3, (5, 7, 3, 11)), (2, (2, 3, 8, 2)),
    (2, (4, 3, 2, 5, 3)),
    (1, (3, 2, 4, 2, 3, 2)),
    (2, (3,) * 7),
    (2, (2,) * 8),
]
SCALAR_CASES = [(d, chis, jo) for (d, chis) in SCALAR_SHAPES for jo in range(len(chis))]
NULL_SHAPES = [(3, (6, 5, 7)), (2, (4, 5, 3, 6))]
NULL_CASES = [(d, chis, present) for (d, chis) in NULL_SHAPES for present in itertools.product((0, 1), repeat=len(chis))]
# the matrix-core form: every leg 16-dimensional, 256 .. 8192 elements
MFMA_SHAPES = [(1, (16, 16)), (2, (16, 16)), (4, (16, 16)), (1, (16, 16, 16)), (2, (16, 16, 16))]
MFMA_CASES = [(d, chis, present) for (d, chis) in MFMA_SHAPES for present in itertools.product((0, 1), repeat=len(chis))]
# one launch of both forms, 64 .. 8192 elements, the largest items neither first nor last: (d, leg dimensions, outgoing leg, present)
MULTI_ITEMS = [(2, (2, 4, 4), 1, (1, 1, 1)), (2, (16, 16, 16), 2, (1, 1, 0)), (1, (16, 16), 0, (1, 1)), (3, (5, 7, 3, 11), 3, (1, 0, 1, 1)),
               (2, (32, 4, 32), 0, (1, 1, 1)), (2, (9, 10, 12), 1, (1, 1, 1)), (4, (16, 16), 1, (1, 1)), (2, (2,) * 8, 5, (1,) * 8)]
SCALES = [1e-18, 1e-9, 1.0, 1e6]
SCALE_SHAPES = [(2, (13, 17, 18)), (3, (5, 7, 3, 11)), (2, (16, 16, 16)), (1, (16, 16))]
# the epilogue cases (psd-like messages): matrix-core shapes (run in both forms) and scalar-only shapes
EPILOGUE_SHAPES = MFMA_SHAPES + [(2, (9, 10, 12)), (3, (5, 7, 3, 11)), (2, (31, 32)), (2, (8, 8)), (4, (1, 16, 3))]
EPILOGUE_TAG = 9      # (the seed: chosen so that every case's conditioning is at least 0.1, tests/test_small_site_ref_cpu.py)


def raw_cases():
    """every (psi, Ms with absent ones None, jo) the raw-message tests of tests/test_gpu_small_site.py compare with `message`"""
    for d, chis, jo in SCALAR_CASES:
        psi, Ms = inputs(d, chis)
        yield psi, Ms, jo
    for d, chis, present in NULL_CASES + MFMA_CASES:
        psi, Ms = inputs(d, chis)
        for jo in range(len(chis)):
            yield psi, masked(Ms, present), jo
    for d, chis, jo, present in MULTI_ITEMS:
        psi, Ms = inputs(d, chis, tag=1)
        yield psi, masked(Ms, present), jo


@functools.lru_cache(maxsize=None)
def restatement_worst():
    """the worst error of the complex64 restatement against `message` over raw_cases(): the measure of what f32 arithmetic gives on these inputs"""
    worst = 0.0
    for psi, Ms, jo in raw_cases():
        worst = max(worst, rel_err(message_c64(psi, Ms, jo), message(psi, Ms, jo)))
    print(f"small-site sweep: worst error of the complex64 numpy restatement {worst:.3e}, kernel bound {4 * worst:.3e}")
    return worst


def raw_bound():
    """bound of the kernels' raw message, max|got - ref| / max|ref|: four times the restatement's worst error (the kernel sums up to 256 terms sequentially per
    thread where numpy's BLAS blocks them)"""
    return 4.0 * restatement_worst()
