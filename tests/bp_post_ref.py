"""High-precision numpy restatements of the kernels that post-process a BP cache and prepare a gate's environments -- msg_rescale, edge_scalar (kernels_bp.hip),
env_prepare, env_finish (kernels_chol.hip), symg_build, symg_finish (kernels_bp.hip), diag, cscale (kernels_util.hip) -- for tests/test_gpu_bp_post.py, pinned to
the oracle in tests/test_bp_post_ref_cpu.py.  Each function restates the DOCUMENTED operation (kernels.hpp, the reference's rescale_messages!, pseudo_sqrt_inv_sqrt
and symmetric_gauge), evaluated in complex128 for the ComplexF32 kernels and in np.clongdouble for the ComplexF64 kernels, and returns next to every output the
sum of the absolute values of the terms the output element adds up (`abs`): the tests' bound

    |out - ref| <= 8 (k + 4) 2^-53 abs + [T = float] 2^-23 |ref|          (bound() below; k = the terms of the element's longest chain)

needs it.  Matrices are numpy arrays M[i, j]; the device holds them column-major (flat / unflat).  dtype: 0 = ComplexF32, 1 = ComplexF64 as in include/tnqs.h."""
import numpy as np

CT = {0: np.complex64, 1: np.complex128}                 # the kernels' T
RT = {0: np.float32, 1: np.float64}
WC = {0: np.complex128, 1: np.clongdouble}               # the precision the reference works in
WR = {0: np.float64, 1: np.longdouble}
DEFAULT_REG = {0: 10 * 2.0 ** -23, 1: 10 * 2.0 ** -52}   # symmetric_gauge's default regularisation, 10 eps(real(T))


def flat(m):
    return np.asarray(m).ravel(order="F")


def unflat(v, n):
    return np.asarray(v).reshape((n, n), order="F")


def bound(k, absval, ref, dtype):
    """the derived error bound per output element (real and imaginary part each): f64 accumulation of a chain of k terms, one rounding to T"""
    b = 8.0 * (k + 4) * 2.0 ** -53 * np.asarray(absval, dtype=np.float64)
    if dtype == 0:
        b = b + 2.0 ** -23 * np.abs(np.asarray(ref)).astype(np.float64)
    return b


def err(got, ref):
    """max(|re difference|, |im difference|) per element, in float64"""
    d = np.asarray(got).astype(np.clongdouble) - np.asarray(ref).astype(np.clongdouble)
    return np.maximum(np.abs(d.real), np.abs(d.imag)).astype(np.float64)


def _msg(m, n, dtype):
    return np.eye(n, dtype=WC[dtype]) if m is None else np.asarray(m).astype(CT[dtype]).astype(WC[dtype])


def edge_scalar(me, mer, n, dtype):
    """sum_ab me[a, b] mer[a, b] (beliefpropagationcache.jl:47-49), None = identity.  Returns (value, abs of the real part's terms, abs of the imaginary part's)"""
    x, y = _msg(me, n, dtype), _msg(mer, n, dtype)
    val = np.sum(x * y)
    are = np.sum(np.abs(x.real * y.real) + np.abs(x.imag * y.imag))
    aim = np.sum(np.abs(x.real * y.imag) + np.abs(x.imag * y.real))
    return val, float(are), float(aim)


def msg_rescale(me, mer, n, dtype):
    """rescale_messages! of one edge (beliefpropagationcache.jl:127-140): both messages to unit Frobenius norm, nn = sum(me .* mer); exactly real nn: its sign goes
    into me; both divided by sqrt(nn), principal branch.  A zero message gives NaN here (0 / 0) -- the kernel writes zeros, which its test asserts on its own.
    Returns (me', mer', abs_me, abs_mer, nn): abs = |ref| (1 + P / (2 |nn|)) with P = sum|me||mer| of the normalised messages, so that bound(n^2, abs, ..) is the
    three reductions' bounds (each 8 (n^2 + 4) 2^-53 relative to its sum of |terms|) carried through the two 1 / sqrt"""
    x, y = _msg(me, n, dtype), _msg(mer, n, dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        x = x / np.sqrt(np.sum(np.abs(x) ** 2)); y = y / np.sqrt(np.sum(np.abs(y) ** 2))
        nn = np.sum(x * y)
        if nn.imag == 0:
            sgn = np.sign(nn.real); x = x * sgn; nn = nn * sgn
        f = 1 / np.sqrt(nn)
        a, b = x * f, y * f
        amp = 1 + float(np.sum(np.abs(x) * np.abs(y))) / (2 * float(abs(nn)))
    return a, b, np.abs(a) * amp, np.abs(b) * amp, nn


def env_prepare(m, n, dtype):
    """H = (M + M^dagger) / 2 and V = identity, both complex128 on the device (safe_eigen's input, utils.jl:94-108); None = identity.  Returns (H, V, abs_H)"""
    if m is None:
        return np.eye(n, dtype=WC[dtype]), np.eye(n, dtype=WC[dtype]), np.eye(n)
    x = _msg(m, n, dtype)
    return (x + x.conj().T) / 2, np.eye(n, dtype=WC[dtype]), ((np.abs(x) + np.abs(x.T)) / 2).astype(np.float64)


def env_finish(A, V, cutoff, dtype):
    """pseudo_sqrt_inv_sqrt (utils.jl:18-27) from the complex128 eigen factors (A = H V, V): lambda_j = Re(v_j^dagger a_j); the eigenvalue is cast to real(T) BEFORE
    the test `iszero(x) || abs(x) < cutoff`; a negative eigenvalue that passes it is an error (flag) and its column is left out; msqrt = sum sqrt(lambda_j) v_j
    v_j^dagger, proj = msqrt minv = sum v_j v_j^dagger over the kept j.  Returns (msqrt, proj, abs_msqrt, abs_proj, (full, error), lambda, kept)"""
    A = np.asarray(A, dtype=np.complex128).astype(WC[dtype]); V = np.asarray(V, dtype=np.complex128).astype(WC[dtype])
    lam = np.sum(V.real * A.real + V.imag * A.imag, axis=0)
    lt = lam.astype(RT[dtype]).astype(np.float64)
    zero = (lt == 0) | (np.abs(lt) < cutoff)
    neg = ~zero & (lt < 0)
    kept = ~zero & ~neg
    sq = np.where(kept, np.sqrt(np.where(kept, lam, 1)), 0).astype(WR[dtype])
    Vk = V * kept
    aV, sq64 = np.abs(V).astype(np.float64), sq.astype(np.float64)                # (the sums of |terms| need no more than float64)
    return (Vk * sq) @ V.conj().T, Vk @ V.conj().T, (aV * kept * sq64) @ aV.T, (aV * kept) @ aV.T, \
        (int(not zero.any()), int(neg.any())), lam, kept


def symg_build(AX, VX, AY, VY, reg, dtype):
    """the first half of symmetric_gauge per edge (symmetric_gauge.jl:13-30) from the eigen factors of both messages: eigenvalues + reg (flag: one of them negative);
    r = conj((M + reg)^1/2), ir = conj((M + reg)^-1/2) -- ITensors.eigen diagonalises M^T -- with root and inverse root 0 where the regularised eigenvalue is not
    positive; Ce = rx ry^T.  Returns dict(rx, ry, irx, iry, Ce, flag) and dict of the same keys' abs"""
    out, ab = {}, {}
    flag = 0
    for tag, A, V in (("x", AX, VX), ("y", AY, VY)):
        A = np.asarray(A, dtype=np.complex128).astype(WC[dtype]); V = np.asarray(V, dtype=np.complex128).astype(WC[dtype])
        lam = np.sum(V.real * A.real + V.imag * A.imag, axis=0) + WR[dtype](reg)
        flag |= int(np.any(lam < 0))
        pos = lam > 0
        r = np.where(pos, np.sqrt(np.where(pos, lam, 1)), 0).astype(WR[dtype])
        ir = np.where(pos, 1 / np.where(pos, r, 1), 0).astype(WR[dtype])
        out["r" + tag] = ((V * r) @ V.conj().T).conj(); out["ir" + tag] = ((V * ir) @ V.conj().T).conj()
        aV = np.abs(V).astype(np.float64)                                         # (the sums of |terms| need no more than float64)
        ab["r" + tag] = (aV * r.astype(np.float64)) @ aV.T; ab["ir" + tag] = (aV * ir.astype(np.float64)) @ aV.T
    out["Ce"] = out["rx"] @ out["ry"].T
    ab["Ce"] = np.abs(out["rx"]).astype(np.float64) @ np.abs(out["ry"]).astype(np.float64).T
    out["flag"] = flag
    return out, ab


def symg_finish(US, V, irx, iry, dtype):
    """the second half (symmetric_gauge.jl:32-55) from the SVD factors U Sigma and V of Ce (type T, singular triplets as columns in ANY order) and the f64 inverse
    roots: sigma_u = |column u| (0 for a column whose norm^2 is NaN or not < 1e300, the kernel's guard), S = sigma sorted descending, stable; Xs = irx U S^1/2, Xd = iry conj(V) S^1/2 in that
    order, zero columns where sigma = 0.  Returns (S, Xs, Xd, abs_Xs, abs_Xd, perm)"""
    US = np.asarray(US).astype(CT[dtype]).astype(WC[dtype]); V = np.asarray(V).astype(CT[dtype]).astype(WC[dtype])
    irx = np.asarray(irx, dtype=np.complex128).astype(WC[dtype]); iry = np.asarray(iry, dtype=np.complex128).astype(WC[dtype])
    with np.errstate(invalid="ignore", over="ignore"):
        s2 = np.sum(US.real ** 2 + US.imag ** 2, axis=0)
        ok = np.isfinite(s2) & (s2 < 1e300)
    sig = np.sqrt(np.where(ok, s2, 0))
    perm = np.argsort(-sig.astype(np.float64), kind="stable")
    S = sig[perm]
    live = S > 0
    cols_u = np.where(live, US[:, perm], 0); cols_v = np.where(live, V[:, perm].conj(), 0)
    f = np.where(live, 1 / np.sqrt(np.where(live, S, 1)), 0); g = np.sqrt(S)
    a64 = lambda m: np.abs(m).astype(np.float64)                                   # (the sums of |terms| need no more than float64)
    return S, (irx @ cols_u) * f, (iry @ cols_v) * g, (a64(irx) @ a64(cols_u)) * f.astype(np.float64), (a64(iry) @ a64(cols_v)) * g.astype(np.float64), perm


def diag(S, dtype):
    return np.diag(np.asarray(S, dtype=np.float64).astype(RT[dtype])).astype(CT[dtype])


def cscale(src, re, im, dtype):
    """src (re + i im).  Returns (value, abs): abs = the larger of the two components' sums of |terms|"""
    x = np.asarray(src).astype(CT[dtype]).astype(WC[dtype])
    re, im = WR[dtype](re), WR[dtype](im)
    val = x * (re + 1j * im) if dtype == 0 else (x.real * re - x.imag * im) + 1j * (x.real * im + x.imag * re)
    return val, np.maximum(np.abs(x.real * re) + np.abs(x.imag * im), np.abs(x.real * im) + np.abs(x.imag * re)).astype(np.float64)


# ---- inputs the CPU pin and the GPU tests share --------------------------------------------------------------------------------------------------------------------
def rng_for(*key):
    return np.random.default_rng([97] + [int(k) for k in key])


def psd(n, rng, rank=None, scale=1.0):
    """B B^dagger / rank, B complex n x rank (rank = 2 n by default: condition number of a few tens)"""
    rank = 2 * n if rank is None else rank
    B = rng.standard_normal((n, rank)) + 1j * rng.standard_normal((n, rank))
    return (B @ B.conj().T) / (2 * rank) * scale


def message(n, rng, perturb=0.1, scale=1.0):
    """a general message: PSD plus a complex NON-Hermitian perturbation (transpositions and dropped conjugations show)"""
    m = psd(n, rng)
    m = m + perturb * np.max(np.abs(m)) / np.sqrt(n) * (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    return m * scale


def eig_factors(H):
    """(A = H V, V) of a Hermitian H by numpy's eigh in f64, as the device's Jacobi leaves them"""
    H = np.asarray(H, dtype=np.complex128)
    w, V = np.linalg.eigh((H + H.conj().T) / 2)
    return H @ V, V, w


def factors_with_spectrum(n, lam, rng):
    """eigen factors with a PRESCRIBED spectrum: V from eigh of a random Hermitian matrix, A = V diag(lam) (so a zero eigenvalue is exactly zero)"""
    _, V, _ = eig_factors(psd(n, rng))
    return V * np.asarray(lam, dtype=np.float64), V
