"""numpy restatement (complex128) of the bond entanglement spectrum of the reference (src/entanglement.jl:73-86 with pseudo_sqrt_inv_sqrt, src/utils.jl:18-26,
and renyi_entropy on a matrix, entanglement.jl:21-29), for a bond (u, v) with m1 = message u -> v and m2 = message v -> u in the layout tnqs_get_message returns:

  1. m2 = Q L Q^dagger (Hermitian, f64);  r = Q f(L) Q^dagger,  f(x) = 0 when |x| < cutoff else sqrt(x);  x <= -cutoff: DomainError;  cutoff = 10 eps(real type), absolute
  2. rho = r m1^T r;  lambda = eigenvalues of rho / tr rho
  3. entropy: drop |lambda| <= 10 eps(real type);  alpha = 1: -sum lambda log lambda, else log(sum lambda^alpha) / (1 - alpha)

bond_spectrum is the eigh route (steps 1-2 as written).  bond_spectrum_svd is a second, independent route to the same numbers: with r1 = m1^{1/2},
rho = (r2 r1^T)(r2 r1^T)^dagger, so lambda = sigma^2(r2 r1^T) / sum sigma^2 -- defined for a positive semi-definite m1 only.  kernel_inputs() builds the inputs the
kernel test uses; the CPU test measures the distance of the two routes on them, m1 taken through psd_part() for both (SPECTRUM_BASELINE)."""
import numpy as np

EPS64 = float(np.finfo(np.float64).eps)


class DomainError(ArithmeticError):
    pass


def cutoff_of(dtype) -> float:
    dt = np.dtype(dtype)
    real = np.float32 if dt in (np.dtype(np.float32), np.dtype(np.complex64)) else np.float64
    return 10.0 * float(np.finfo(real).eps)


def _herm(m):
    m = np.asarray(m, dtype=np.complex128)
    return (m + m.conj().T) / 2


def pseudo_sqrt(m, cutoff):
    """step 1: the root of a Hermitian message, eigenvalues with |x| < cutoff dropped"""
    w, q = np.linalg.eigh(_herm(m))
    if np.any(w <= -cutoff):
        raise DomainError(f"sqrt of a negative message eigenvalue ({w.min():.3e})")
    f = np.where(np.abs(w) < cutoff, 0.0, np.sqrt(np.clip(w, 0.0, None)))
    return (q * f) @ q.conj().T


def bond_spectrum(m1, m2, cutoff):
    """steps 1-2: eigenvalues of rho / tr rho, descending (signed, unfiltered)"""
    r = pseudo_sqrt(m2, cutoff)
    rho = _herm(r @ np.asarray(m1, dtype=np.complex128).T @ r)
    tr = float(np.trace(rho).real)
    if not (tr > 0 and np.isfinite(tr)):
        raise DomainError(f"trace of the bond density matrix is {tr!r}")
    return np.sort(np.linalg.eigvalsh(rho))[::-1] / tr


def bond_spectrum_svd(m1, m2, cutoff):
    """the same spectrum from the singular values of r2 r1^T (m1 Hermitian positive semi-definite up to rounding: its negative eigenvalues are clipped)"""
    r2 = pseudo_sqrt(m2, cutoff)
    w, q = np.linalg.eigh(_herm(m1))
    r1 = (q * np.sqrt(np.clip(w, 0.0, None))) @ q.conj().T
    s = np.linalg.svd(r2 @ r1.T, compute_uv=False)
    return np.sort(s * s)[::-1] / np.sum(s * s)


def psd_part(m):
    """the Hermitian positive semi-definite part of a message (negative eigenvalues set to zero), complex128: the domain on which BOTH routes are defined -- the SVD
    route needs r1 = m1^{1/2}.  A message that is positive semi-definite in exact arithmetic keeps eigenvalues of either sign at rounding level once it is stored
    (1e-7 of its norm for a rank-deficient complex64 message); comparing the routes on (psd_part(m1), m2) measures the routes, not that rounding"""
    w, q = np.linalg.eigh(_herm(m))
    return (q * np.clip(w, 0.0, None)) @ q.conj().T


def renyi(lam, alpha, threshold):
    """step 3 on a spectrum"""
    lam = np.asarray(lam, dtype=np.float64)
    lam = lam[np.abs(lam) > threshold]
    if alpha == 1:
        return float(-np.sum(lam * np.log(lam)))
    return float(np.log(np.sum(lam ** alpha)) / (1 - alpha))


def renyi_of_matrix(rho, alpha, normalize=True):
    """entanglement.jl:21-29"""
    rho = np.asarray(rho)
    thr = cutoff_of(rho.dtype)
    if normalize:
        rho = rho / np.trace(rho)
    return renyi(np.linalg.eigvalsh(_herm(rho)), alpha, thr)


# ---- the inputs of the kernel test (tests/test_gpu_bond_spectra.py) ------------------------------------------------------------------------------------------
KERNEL_CHIS = (1, 2, 3, 5, 16, 17, 32, 64, 72)        # odd, prime, not a multiple of 16, multiples of 16, and 72: the smallest even chi whose f64 Jacobi with V leaves the LDS
KINDS = ("full", "rank1", "rankhalf", "null1", "null2")
LOW_RANK_NORM = 1e-2                                  # ||m||_2 of the rank-deficient messages: their nonzero eigenvalues stay >= 100 x cutoff, the zero ones are far below it


def _unitary(rng, n):
    q, r = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    return q * (np.diag(r) / np.abs(np.diag(r)))


def _message(rng, n, k, lo):
    """m = B B^dagger / tr with B = Q[:, :k] diag(sqrt(w)), Q a random unitary and w spread between lo and 1 of the largest: a rank-k message with known eigenvalues w / sum w"""
    w = rng.permutation(np.linspace(lo, 1.0, k)) if k > 1 else np.ones(1)
    b = _unitary(rng, n)[:, :k] * np.sqrt(w)
    m = b @ b.conj().T
    return m / np.trace(m).real


def kernel_inputs(dtype, chis=KERNEL_CHIS, seed=2024):
    """[(chi, kind, m1, m2, present1, present2)] in the given dtype: for every chi a full-rank pair (eigenvalues of m2 between 0.05 and 1 of the largest; m1 a generic
    B B^dagger / tr), rank-1 and rank-chi/2 pairs scaled to ||m||_2 <= 1e-2 (chi >= 2 / chi >= 4), and one pair with either message null (= identity; the slot holds zeros)"""
    rng = np.random.default_rng(seed)
    items = []
    for n in chis:
        for kind in KINDS:
            if kind == "rank1":
                if n < 2:
                    continue
                m1, m2 = _message(rng, n, 1, 1.0) * LOW_RANK_NORM, _message(rng, n, 1, 1.0) * LOW_RANK_NORM
            elif kind == "rankhalf":
                if n < 4:
                    continue
                m1, m2 = _message(rng, n, n // 2, 0.5) * LOW_RANK_NORM, _message(rng, n, n // 2, 0.5) * LOW_RANK_NORM
            else:
                b = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
                m1 = b @ b.conj().T
                m1 = m1 / np.trace(m1).real
                m2 = _message(rng, n, n, 0.05)
            p1, p2 = kind != "null1", kind != "null2"
            if not p1:
                m1 = np.zeros((n, n))
            if not p2:
                m2 = np.zeros((n, n))
            items.append((n, kind, np.asfortranarray(m1.astype(dtype)), np.asfortranarray(m2.astype(dtype)), p1, p2))
    return items


def effective(m, present):
    """the message the kernels see: the stored one, or the identity for a null pointer"""
    return np.asarray(m, dtype=np.complex128) if present else np.eye(m.shape[0], dtype=np.complex128)


def negative_item(dtype, n=5, seed=5):
    """a pair whose m2 has one constructed eigenvalue of -1e-3 (the others between 0.2 and 1)"""
    rng = np.random.default_rng(seed)
    q = _unitary(rng, n)
    w = np.linspace(0.2, 1.0, n); w[1] = -1e-3
    m2 = (q * w) @ q.conj().T
    return np.asfortranarray(_message(rng, n, n, 0.05).astype(dtype)), np.asfortranarray(m2.astype(dtype))
