"""CPU pin of tests/bp_post_ref.py (the reference of tests/test_gpu_bp_post.py) to the oracle, at n = 3 and n = 17, both dtypes: edge_scalar and the message half of
rescale on complex NON-Hermitian and null messages; symmetric_gauge and pseudo_sqrt_inv_sqrt on complex Hermitian ones (the oracle's eigh reads the upper triangle of a
message, the device averages it with its adjoint -- env_prepare -- so the two agree on Hermitian input only, which is what both are handed in a BP cache).

One edge a - b with site dimension n and the identity as both site tensors: the gauged tensors of the oracle ARE its Xs and Xd.  Tolerances: the oracle works in the
messages' precision, so 2e-5 (ComplexF32: a few hundred f32 roundings on numbers <= 1, inverse roots of condition <= 100) and 1e-11 (ComplexF64); Xs, Xd and the
projector carry another factor 100 (2e-3 / 1e-9) for the inverse roots on top of an SVD or eigendecomposition in T.  The ComplexF32 pins are therefore coarse: they
catch a transposition or a dropped conjugate (an O(1) error), not a scaling factor that is off by 1e-3.  The ComplexF64 pins (1e-11, 1e-9) carry that weight -- the
restatement is the same code for both dtypes, only the working precision differs."""
import numpy as np
import pytest

import tnqs_oracle as o
import bp_post_ref as ref

TOL = {0: 2e-5, 1: 1e-11}
CASES = [(n, dt) for n in (3, 17) for dt in (0, 1)]


def _cache(n, dtype, me, mer):
    g = o.Graph(["a", "b"], [("a", "b")])
    eye = np.eye(n, dtype=ref.CT[dtype])
    c = o.BeliefPropagationCache(o.TensorNetworkState(g, {"a": eye.copy(), "b": eye.copy()}), edge_sequence=[])
    if me is not None:
        c.messages[("a", "b")] = np.asarray(me).astype(ref.CT[dtype])
    if mer is not None:
        c.messages[("b", "a")] = np.asarray(mer).astype(ref.CT[dtype])
    return c


def _close(a, b, tol):
    a, b = np.asarray(a).astype(np.complex128), np.asarray(b).astype(np.complex128)
    return np.max(np.abs(a - b)) <= tol * max(1.0, np.max(np.abs(b)))


@pytest.mark.parametrize("n,dtype", CASES)
@pytest.mark.parametrize("null", [(0, 0), (1, 0), (0, 1), (1, 1)], ids=lambda v: f"null{v[0]}{v[1]}")
def test_edge_scalar_and_message_rescale_match_the_oracle(n, dtype, null):
    rng = ref.rng_for(1, n, dtype)
    me = None if null[0] else ref.message(n, rng)
    mer = None if null[1] else ref.message(n, rng)
    c = _cache(n, dtype, me, mer)
    val, _, _ = ref.edge_scalar(me, mer, n, dtype)
    assert abs(complex(val) - o.edge_scalar(c, ("a", "b"))) <= TOL[dtype] * max(1.0, abs(complex(val)))
    a, b, _, _, nn = ref.msg_rescale(me, mer, n, dtype)
    r = o.rescale(c)
    assert _close(a, r.messages[("a", "b")], TOL[dtype]) and _close(b, r.messages[("b", "a")], TOL[dtype])
    assert abs(complex(np.sum(a * b)) - 1) < 1e-12                                 # what rescale_messages! is for
    if null == (1, 1):
        assert nn.imag == 0 and _close(a, np.eye(n) / np.sqrt(n), 1e-15)


def test_message_rescale_folds_the_sign_of_a_real_negative_scalar_into_me():
    n = 3
    rng = ref.rng_for(2)
    me, mer = rng.standard_normal((n, n)), rng.standard_normal((n, n))
    if np.sum(me * mer) > 0:
        mer = -mer
    for dtype in (0, 1):
        a, b, _, _, nn = ref.msg_rescale(me, mer, n, dtype)
        r = o.rescale(_cache(n, dtype, me, mer))
        assert nn.imag == 0 and nn.real > 0
        assert _close(a, r.messages[("a", "b")], TOL[dtype]) and _close(b, r.messages[("b", "a")], TOL[dtype])
        assert np.all(a.imag == 0) and np.all(b.imag == 0) and abs(complex(np.sum(a * b)) - 1) < 1e-12
        assert np.all(np.sign(a.real) == -np.sign(me)) and np.all(np.sign(b.real) == np.sign(mer))


@pytest.mark.parametrize("n,dtype", CASES)
def test_symmetric_gauge_matches_the_oracle_up_to_the_svd_phases(n, dtype):
    rng = ref.rng_for(3, n, dtype)
    X, Y = ref.psd(n, rng).astype(ref.CT[dtype]), ref.psd(n, rng).astype(ref.CT[dtype])
    og = o.symmetric_gauge(_cache(n, dtype, X, Y))
    oXs, oXd, oS = og.tns.tensors["a"], og.tns.tensors["b"], np.diag(og.messages[("a", "b")]).real
    H1, _, _ = ref.env_prepare(X, n, dtype); H2, _, _ = ref.env_prepare(Y, n, dtype)
    AX, VX, _ = ref.eig_factors(H1); AY, VY, _ = ref.eig_factors(H2)
    out, _ = ref.symg_build(AX, VX, AY, VY, ref.DEFAULT_REG[dtype], dtype)
    assert out["flag"] == 0
    ce = out["Ce"].astype(ref.CT[dtype])
    u, s, vh = np.linalg.svd(ce.astype(np.complex128))
    order = rng.permutation(n)                                                    # the device's Jacobi leaves the triplets unsorted
    S, Xs, Xd, _, _, perm = ref.symg_finish((u * s)[:, order], vh.conj().T[:, order], out["irx"], out["iry"], dtype)
    tol = TOL[dtype] * 100                                                        # inverse roots of condition ~ 30 on top of an SVD in T
    assert np.array_equal(order[perm], np.arange(n)) and np.all(np.diff(S.astype(np.float64)) <= 0)
    assert _close(S, oS, TOL[dtype])
    ph = np.sum(np.asarray(Xs).astype(np.complex128).conj() * oXs, axis=0); ph = ph / np.abs(ph)
    assert _close(np.asarray(Xs).astype(np.complex128) * ph, oXs, tol) and _close(np.asarray(Xd).astype(np.complex128) * ph.conj(), oXd, tol)
    # Ce itself: Xs Xd^T = irx Ce iry^T is free of the phases
    lhs = (out["irx"] @ out["Ce"] @ out["iry"].T).astype(np.complex128)
    assert _close(lhs, oXs.astype(np.complex128) @ oXd.astype(np.complex128).T, tol)
    assert np.array_equal(ref.diag(S, dtype), np.diag(S.astype(ref.RT[dtype])).astype(ref.CT[dtype]))


@pytest.mark.parametrize("n,dtype", CASES)
def test_env_finish_matches_pseudo_sqrt_inv_sqrt(n, dtype):
    rng = ref.rng_for(4, n, dtype)
    m = ref.psd(n, rng, rank=n - 1).astype(ref.CT[dtype])                          # one eigenvalue at rounding level: dropped by the cutoff
    cutoff = float(ref.RT[dtype](10 * np.finfo(ref.RT[dtype]).eps))
    H, V0, _ = ref.env_prepare(m, n, dtype)
    assert np.array_equal(H, H.conj().T) and np.array_equal(V0, np.eye(n))
    A, V, _ = ref.eig_factors(H)
    msqrt, proj, _, _, flags, lam, kept = ref.env_finish(A, V, cutoff, dtype)
    osq, oinv = o.pseudo_sqrt_inv_sqrt(m, cutoff)
    assert flags == (0, 0) and kept.sum() == n - 1
    assert _close(msqrt, osq, TOL[dtype]) and _close(proj, osq.astype(np.complex128) @ oinv.astype(np.complex128), TOL[dtype] * 100)
    assert _close(proj @ proj, proj, 1e-12) and _close(msqrt @ proj, msqrt, 1e-12)
    # a negative eigenvalue beyond the cutoff: the oracle raises, the restatement flags it and leaves the column out
    lam2 = np.linspace(0.2, 1.0, n); lam2[1] = -0.3
    A2, V2 = ref.factors_with_spectrum(n, lam2, rng)
    with pytest.raises(ValueError):
        o.pseudo_sqrt_inv_sqrt(((V2 * lam2) @ V2.conj().T).astype(ref.CT[dtype]), cutoff)
    _, _, _, _, flags2, _, kept2 = ref.env_finish(A2, V2, cutoff, dtype)
    assert flags2 == (1, 1) and not kept2[1] and kept2.sum() == n - 1


def test_bound_and_cscale():
    assert ref.bound(17, 2.0, 3.0, 1) == 8 * 21 * 2.0 ** -53 * 2.0
    assert ref.bound(17, 2.0, 3.0, 0) == 8 * 21 * 2.0 ** -53 * 2.0 + 3.0 * 2.0 ** -23
    for dtype in (0, 1):
        x = ref.rng_for(5).standard_normal(7) + 1j * ref.rng_for(6).standard_normal(7)
        v, a = ref.cscale(x, 0.3, -1.7, dtype)
        xt = x.astype(ref.CT[dtype]).astype(np.complex128)
        assert _close(v, xt * (0.3 - 1.7j), 1e-15) and np.all(a >= np.abs(v.real).astype(np.float64) * (1 - 1e-15))
