"""Plain numpy (complex128) restatement of the gate path's per-gate small algebra -- from the Gram factors of the two sites to theta, its low-rank form, the
truncation and the new site tensors -- for tests/test_gpu_gate_algebra.py, pinned to oracle.simple_update in tests/test_gate_algebra_ref_cpu.py.  Every function
restates a stage as csrc/kernels_theta.hip and csrc/kernels.hpp DOCUMENT it (the R-factor interface, theta, the operator-sum factors, the CholeskyQR2 composition,
the NDTensors truncation rule, X1 / X2), not the kernels' loops.

Conventions.  A site with physical dimension d and bond dimension chi towards the partner has n = d chi columns, index (s, b) = s + d b.  Its gauged tensor,
matricised as Psi[outer, (s, b)], factors as Psi = Q R with the R factor read through ONE interface whatever produced it (GateItem, kernels.hpp):
    R[a, (s, b)] = sqrt(l_a) conj(GV[(s, b), idx_a]),      R^+[:, a] = GW[:, idx_a] / sqrt(l_a),      a < r
  mode 0 (eigen):     G = Psi^dagger Psi = V L V^dagger, GA = G V, GV = GW = V; l_j = Re(v_j^dagger a_j); kept: l_j > tau l_max (tau < 0: all, l := max(l, 0) + |tau| l_max)
  mode 1 (Cholesky):  G = L L^dagger, GV = L, GW = (L^-1)^dagger, l = 1, all columns
  mode 2 (explicit):  GV = R^dagger, GW = R^+, l = 1, the first rk columns
theta[(a, s1'), (c, s2')] = sum g[(s1' s2'), (s1 s2)] sum_b R1[a, (s1, b)] R2[c, (s2, b)], rows a + r1 s1', columns c + r2 s2'; the gate matrix has the first vertex
most significant.  Matrices are numpy arrays M[i, j]; the device holds them column-major.  dtype: 0 = ComplexF32 state, 1 = ComplexF64 (include/tnqs.h).

Bounds (prod_bound): an output that is an f64-accumulated complex product of inner length L, rounded once to the output type with unit roundoff u_T, differs from
this complex128 reference by at most  2 (2 L + 16) 2^-53 (|A| |B|)_ij + u_T |ref_ij|  in its real and in its imaginary part (a complex term is two real products
per part, |ar br| + |ai bi| <= |a| |b|; the 16 covers the scale factors applied to operands or result; the leading 2 this reference's own rounding)."""
import numpy as np

CT = {0: np.complex64, 1: np.complex128}
RT = {0: np.float32, 1: np.float64}
UT = {0: 2.0 ** -24, 1: 2.0 ** -53}                      # unit roundoff of T
U64 = 2.0 ** -53


def flat(m):
    return np.asarray(m).ravel(order="F")


def unflat(v, rows, cols):
    return np.asarray(v).reshape((rows, cols), order="F")


def err(got, ref):
    """max(|re difference|, |im difference|) per element"""
    d = np.asarray(got).astype(np.complex128) - np.asarray(ref).astype(np.complex128)
    return np.maximum(np.abs(d.real), np.abs(d.imag))


def prod_bound(absprod, L, ref, u_out, longdouble_ref=False):
    return (1.0 if longdouble_ref else 2.0) * (2 * L + 16) * U64 * np.asarray(absprod, dtype=np.float64) + u_out * np.abs(np.asarray(ref)).astype(np.float64)


# ---- the R-factor interface -------------------------------------------------------------------------------------------------------------------------------------
def eigen_factors(Psi):
    """mode 0 factors of a matricised gauged tensor Psi[outer, (s, b)]: (GA, GV, GW) = (G V, V, V) from LAPACK's Hermitian eigen factorisation of G = Psi^dagger Psi"""
    Psi = np.asarray(Psi, dtype=np.complex128)
    G = Psi.conj().T @ Psi
    G = (G + G.conj().T) / 2
    _, V = np.linalg.eigh(G)
    return G @ V, V, V.copy()


def chol_factors(Psi):
    """mode 1 factors: GV = L (G = L L^dagger), GW = (L^-1)^dagger; GA is not read"""
    Psi = np.asarray(Psi, dtype=np.complex128)
    G = Psi.conj().T @ Psi
    L = np.linalg.cholesky((G + G.conj().T) / 2)
    return np.zeros_like(L), L, np.linalg.inv(L).conj().T


def explicit_factors(R):
    """mode 2 factors of an explicit R (rk x n): GV = R^dagger, GW = R^+ (n x n, the first rk columns valid)"""
    R = np.asarray(R, dtype=np.complex128)
    rk, n = R.shape
    GV = np.zeros((n, n), dtype=np.complex128); GW = np.zeros((n, n), dtype=np.complex128)
    GV[:, :rk] = R.conj().T
    GW[:, :rk] = np.linalg.pinv(R)
    return np.zeros((n, n), dtype=np.complex128), GV, GW


def rayleigh(GA, GV):
    """l_j = Re(v_j^dagger a_j) and the sum of |terms| of each (for its bound, inner length n)"""
    lam = np.sum(GV.conj() * GA, axis=0).real
    return lam, np.sum(np.abs(GV) * np.abs(GA), axis=0)


def kept(lam, tau):
    """the rank decision of the eigen route: (lam_kept, idx)"""
    lam = np.asarray(lam, dtype=np.float64)
    lmax = max(0.0, float(lam.max()))
    if tau < 0:
        return np.maximum(lam, 0.0) - tau * lmax, np.arange(len(lam))
    idx = np.nonzero((lam > tau * lmax) & (lam > 0))[0]
    return lam[idx], idx


def decision_margin(lam, tau):
    """how far (as a factor >= 1) the closest eigenvalue is from the threshold tau l_max -- the tests require 100"""
    lam = np.asarray(lam, dtype=np.float64)
    thr = abs(tau) * lam.max()
    if tau < 0 or thr <= 0:
        return np.inf
    r = np.abs(lam[lam != 0]) / thr
    return float(np.min(np.maximum(r, 1 / r))) if len(r) else np.inf


def site_R(mode, GA, GV, GW, tau=0.0, rk=None, lam=None, idx=None):
    """(lam, idx, R (r x n), R^+ (n x r)) of a site; lam / idx given: the device's (already checked) decision is used instead of this module's"""
    n = GV.shape[0]
    if lam is None:
        if mode == 0:
            lam, idx = kept(rayleigh(GA, GV)[0], tau)
        else:
            r = n if mode == 1 else int(rk)
            lam, idx = np.ones(r), np.arange(r)
    lam = np.asarray(lam, dtype=np.float64); idx = np.asarray(idx, dtype=np.int64)
    sq = np.sqrt(lam)
    R = sq[:, None] * GV[:, idx].conj().T
    Rp = GW[:, idx] / sq[None, :]
    return lam, idx, R, Rp


def ill_conditioned(mode, GV, lam):
    """info[6] of one site: smallest / largest squared singular value of the kept factor below 1e-4 (Cholesky: from the pivots; explicit factor: never)"""
    if mode == 2:
        return 0
    v = np.diag(GV).real ** 2 if mode == 1 else np.asarray(lam)
    return int(len(v) > 0 and v.max() > 0 and v.min() < 1e-4 * v.max())


# ---- theta and its operator-sum form ----------------------------------------------------------------------------------------------------------------------------
def _R3(R, d, chi):
    return R.reshape(R.shape[0], chi, d).transpose(0, 2, 1)            # [a, s, b] from column index s + d b


def gate4(gate, d1, d2):
    return np.asarray(gate, dtype=np.complex128).reshape(d1, d2, d1, d2)   # [s1', s2', s1, s2]


def theta(R1, R2, gate, d1, d2, chi):
    """theta (r1 d1 x r2 d2) and (|.| |.|): the same contraction of the absolute values, for prod_bound with L = d1 d2 chi"""
    g = gate4(gate, d1, d2)
    a, b = _R3(R1, d1, chi), _R3(R2, d2, chi)
    th = np.einsum("xyst,asb,ctb->xayc", g, a, b, optimize=True)
    ab = np.einsum("xyst,asb,ctb->xayc", np.abs(g), np.abs(a), np.abs(b), optimize=True)
    r1, r2 = R1.shape[0], R2.shape[0]
    return th.reshape(d1 * r1, d2 * r2), ab.reshape(d1 * r1, d2 * r2)


def operator_AB(R1, R2, fa, fb, d1, d2, chi):
    """A[(a, s1'), (k, b)] = sum_s1 a_k[s1', s1] R1[a, (s1, b)], B likewise with b_k and R2; columns b + chi k.  fa: kappa x d1 x d1 as [k][s' + d s].
    Returns (A, |a| |R1|, B, |b| |R2|): inner length d"""
    kappa = len(fa) // (d1 * d1)
    ak = np.asarray(fa).reshape(kappa, d1, d1).transpose(0, 2, 1)      # [k, s', s]
    bk = np.asarray(fb).reshape(kappa, d2, d2).transpose(0, 2, 1)
    a, b = _R3(R1, d1, chi), _R3(R2, d2, chi)

    def form(op, r):
        v = np.einsum("kxs,asb->xakb", op, r, optimize=True)           # rows a + r x, columns b + chi k
        return v.reshape(v.shape[0] * v.shape[1], -1)
    return form(ak, a), form(np.abs(ak), np.abs(a)), form(bk, b), form(np.abs(bk), np.abs(b))


def operator_sum_gate(fa, fb, d1, d2):
    """sum_k a_k (x) b_k as a gate matrix [(s1' s2'), (s1 s2)]"""
    kappa = len(fa) // (d1 * d1)
    ak = np.asarray(fa).reshape(kappa, d1, d1).transpose(0, 2, 1)
    bk = np.asarray(fb).reshape(kappa, d2, d2).transpose(0, 2, 1)
    return np.einsum("kxs,kyt->xyst", ak, bk).reshape(d1 * d2, d1 * d2)


def stored_theta(th, wide):
    """what the device keeps: theta, or (one-sided Jacobi needs rows >= columns) its adjoint"""
    return th.conj().T if wide else th


# ---- truncation (NDTensors truncate!, restated from oracle/tnqs_oracle.py truncate_spectrum) in the data's real precision -------------------------------------------
def truncate(sig_desc, maxdim, cutoff, rt):
    """sig_desc: singular values, descending (float64).  The rule runs on p = s^2 in the data's real precision rt, relative cutoff, mindim = 1.
    Returns (n_keep, truncerr, steps): steps = [(truncerr + p_n, cutoff scale)] of the last accepting and the rejecting test of the cutoff loop"""
    s = np.asarray(sig_desc, dtype=np.float64).astype(rt)
    p = s * s
    n = len(p)
    if p[0] <= 0 or n == 1:
        return 1, 0.0, []
    truncerr = rt(0)
    md = n if not maxdim or maxdim <= 0 else int(maxdim)
    while n > md:
        truncerr = rt(truncerr + p[n - 1]); n -= 1
    scale = rt(0)
    for v in p:
        scale = rt(scale + v)
    if scale == 0:
        scale = rt(1)
    c = rt(0 if cutoff is None or cutoff < 0 else cutoff)
    steps = []
    while n > 1:
        t = rt(truncerr + p[n - 1])
        steps.append((float(t), float(rt(c * scale))))
        if t <= rt(c * scale):
            truncerr = t; n -= 1
        else:
            break
    return n, float(rt(truncerr / scale)), steps[-2:]


def decisions_clear(steps, rel=1e-3):
    """|truncerr + p_n - cutoff scale| > rel cutoff scale at the accepting and the rejecting step"""
    return all(abs(t - cs) > rel * cs for t, cs in steps)


def new_factors(th, n_keep, Rp1, Rp2, d1, d2):
    """X1[(s, b), (s1', u)] = R1^+ U sqrt(S), X2[(s, b), (s2', u)] = R2^+ (sqrt(S) V^dagger)^T over the n_keep largest singular triplets of theta (LAPACK), columns s' + d u;
    returns (S, X1, X2, P) with P[(s, b), s1', (s, b)', s2'] = sum_u X1 X2, which is free of the SVD's phase freedom"""
    U, S, Vh = np.linalg.svd(th, full_matrices=False)
    U, S, Vh = U[:, :n_keep], S[:n_keep], Vh[:n_keep]
    r1, r2 = Rp1.shape[1], Rp2.shape[1]
    Lf = (U * np.sqrt(S)).reshape(d1, r1, n_keep)                     # rows a + r1 s1'
    Rf = (np.sqrt(S)[:, None] * Vh).reshape(n_keep, d2, r2)
    X1 = np.einsum("ia,xau->ixu", Rp1, Lf).transpose(0, 2, 1).reshape(Rp1.shape[0], -1)       # columns s1' + d1 u
    X2 = np.einsum("jc,uyc->jyu", Rp2, Rf).transpose(0, 2, 1).reshape(Rp2.shape[0], -1)
    return S, X1, X2, pair_product(X1, X2, d1, d2, n_keep)


def pair_product(X1, X2, d1, d2, nk):
    """P[i, s1', j, s2'] = sum_u X1[i, (s1', u)] X2[j, (s2', u)]"""
    a = np.asarray(X1, dtype=np.complex128).reshape(X1.shape[0], nk, d1)
    b = np.asarray(X2, dtype=np.complex128).reshape(X2.shape[0], nk, d2)
    return np.einsum("iux,juy->ixjy", a, b, optimize=True)


def truncated_theta_product(th, n_keep, Rp1, Rp2, d1, d2):
    """R1^+ theta_n R2^+T as P[i, s1', j, s2'] with theta_n the best rank-n_keep approximation, and the same product of absolute values (|R1^+| |U| S |V^dagger| |R2^+|^T)"""
    U, S, Vh = np.linalg.svd(th, full_matrices=False)
    tn = (U[:, :n_keep] * S[:n_keep]) @ Vh[:n_keep]
    ta = (np.abs(U[:, :n_keep]) * S[:n_keep]) @ np.abs(Vh[:n_keep])
    r1, r2 = Rp1.shape[1], Rp2.shape[1]

    def wrap(t, p1, p2):
        return np.einsum("ia,xayc,jc->ixjy", p1, t.reshape(d1, r1, d2, r2), p2, optimize=True)
    return wrap(tn, Rp1, Rp2), wrap(ta, np.abs(Rp1), np.abs(Rp2))


# ---- the second factorisation pass (CholeskyQR2 composition, kernels.hpp Qr2ComposeItem) ------------------------------------------------------------------------------
def qr2_compose(R1, Rp1, A2, V2, tau):
    """with the eigen pair (A2 = G2 V2, V2) of G2 = Q1^dagger Q1 (r1 x r1 block of an n x n matrix): R2 = L2^1/2 W2^dagger over l2 > tau l2_max, and
    GVout = (R2 R1)^dagger, GWout = R1^+ R2^+ (n x rk), rk"""
    lam2, _ = rayleigh(A2, V2)
    l2, sel = kept(lam2, tau)
    r1 = R1.shape[0]
    W2 = V2[:r1][:, sel]
    R2 = np.sqrt(l2)[:, None] * W2.conj().T
    R2p = W2 / np.sqrt(l2)[None, :]
    return (R2 @ R1).conj().T, Rp1 @ R2p, len(sel), lam2
