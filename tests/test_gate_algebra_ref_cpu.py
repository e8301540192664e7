"""Pins tests/gate_algebra_ref.py -- the numpy restatement tests/test_gpu_gate_algebra.py measures the gate path's small-algebra kernels against -- to the parity
oracle (oracle/tnqs_oracle.py simple_update) on random two-site problems, and tests the host-only entry point tnqs_dbg_operator_sum (the gate as an operator sum, as
the engine's gate_items() gets it).  No GPU is needed."""
import ctypes as C

import numpy as np
import pytest

import tnqs_amd as tn
import tnqs_oracle as o
import gate_algebra_ref as ref

lib = C.CDLL(tn.LIB_PATH)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _unitary(rng, n):
    q, r = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    return q * (np.diag(r) / np.abs(np.diag(r)))


def make_gate(name, d1, d2, rng):
    """two-site gates for any (d1, d2): the qubit gates from the oracle, their d-level analogues otherwise"""
    if d1 == 2 and d2 == 2 and name in ("Rzz", "Rxx", "CPHASE"):
        return o.gate_matrix(name, 0.37)
    if d1 == 2 and d2 == 2 and name in ("CNOT", "SWAP"):
        return o.gate_matrix(name)
    z = lambda d: np.diag(np.linspace(1.0, -1.0, d))
    if name == "Rzz":                                     # exp(-i t/2 Z (x) Z): diagonal
        return np.diag(np.exp(-0.5j * 0.37 * np.diag(np.kron(z(d1), z(d2)))))
    if name == "CNOT":                                    # controlled shift: |s1, s2> -> |s1, s2 + s1 mod d2>
        g = np.zeros((d1 * d2, d1 * d2), dtype=complex)
        for s1 in range(d1):
            for s2 in range(d2):
                g[s1 * d2 + (s2 + s1) % d2, s1 * d2 + s2] = 1
        return g
    if name == "SWAP":
        assert d1 == d2
        g = np.zeros((d1 * d2, d1 * d2), dtype=complex)
        for s1 in range(d1):
            for s2 in range(d2):
                g[s2 * d2 + s1, s1 * d2 + s2] = 1
        return g
    if name == "product":
        return np.kron(_unitary(rng, d1), _unitary(rng, d2))
    assert name == "random"
    return _unitary(rng, d1 * d2)


def matricise(psi, bax):
    """Psi[outer, (s, b)] with column s + d b of a tensor [s, ...] whose bond axis is bax"""
    outer = [i for i in range(psi.ndim) if i not in (0, bax)]
    t = np.transpose(psi, outer + [bax, 0])
    return np.ascontiguousarray(t).reshape(-1, psi.shape[bax] * psi.shape[0])


def ref_update(gate, psi1, psi2, maxdim, cutoff, dtype):
    """the reference's simple_update core on the eigen R factors: (theta in the product basis, S, chi', truncerr, two-site tensor after the gate, truncation steps)"""
    d1, d2, chi = psi1.shape[0], psi2.shape[0], psi1.shape[2]
    P1, P2 = matricise(psi1, 2).astype(np.complex128), matricise(psi2, 1).astype(np.complex128)
    tau = 1e-12 if dtype == 0 else 4.0 * max(P1.shape[1], P2.shape[1]) * 2.0 ** -52
    f1, f2 = ref.eigen_factors(P1), ref.eigen_factors(P2)
    _, _, R1, Rp1 = ref.site_R(0, *f1, tau=tau)
    _, _, R2, Rp2 = ref.site_R(0, *f2, tau=tau)
    th, _ = ref.theta(R1, R2, gate, d1, d2, chi)
    Q1, Q2 = P1 @ Rp1, P2 @ Rp2
    r1, r2 = R1.shape[0], R2.shape[0]
    full = np.einsum("oa,xayc,pc->oxpy", Q1, th.reshape(d1, r1, d2, r2), Q2, optimize=True)        # Q1 theta Q2^T: independent of the gauge of R
    sv = np.linalg.svd(th, compute_uv=False)
    n, terr, steps = ref.truncate(sv, maxdim, cutoff, ref.RT[dtype])
    S, X1, X2, P = ref.new_factors(th, n, Rp1, Rp2, d1, d2)
    new = np.einsum("oi,ixjy,pj->oxpy", P1, P, P2, optimize=True)
    return full, S, n, terr, new, steps


CASES = [(d1, d2, chi, gname, trunc)
         for (d1, d2) in ((2, 2), (3, 3), (2, 3))
         for chi in (3, 8)
         for gname in ("Rzz", "CNOT", "SWAP", "random")
         for trunc in ("none", "maxdim", "cutoff")
         if not (gname == "SWAP" and d1 != d2)]


@pytest.mark.parametrize("dtype", (1, 0), ids=("c128", "c64"))
@pytest.mark.parametrize("d1,d2,chi,gname,trunc", CASES, ids=[f"d{a}{b}-chi{c}-{g}-{t}" for a, b, c, g, t in CASES])
def test_reference_matches_simple_update(d1, d2, chi, gname, trunc, dtype):
    rng = np.random.default_rng(1000 * d1 + 100 * d2 + chi + len(gname))
    ct = ref.CT[dtype]
    tol = 1e-10 if dtype == 1 else 2e-4
    o1, o2 = (5, 2 * d2 * chi) if chi == 3 else (2 * d1 * chi, 7)          # one site with fewer fibers than columns (rank-deficient Gram matrix), one tall
    psi1 = (rng.standard_normal((d1, o1, chi)) + 1j * rng.standard_normal((d1, o1, chi))).astype(ct)
    psi2 = (rng.standard_normal((d2, chi, o2)) + 1j * rng.standard_normal((d2, chi, o2))).astype(ct)
    psi1 /= np.linalg.norm(psi1); psi2 /= np.linalg.norm(psi2)
    gate = make_gate(gname, d1, d2, rng)
    maxdim, cutoff = {"none": (None, None), "maxdim": (chi, 1e-10), "cutoff": (None, 3e-2)}[trunc]
    envs = ([(1, np.eye(o1, dtype=ct))], [(2, np.eye(o2, dtype=ct))])
    out, s_o, err_o = o.simple_update(gate, [psi1, psi2], (2, 1), envs, maxdim=maxdim, cutoff=cutoff, normalize_tensors=False)
    full, S, n, terr, new, steps = ref_update(gate, psi1, psi2, maxdim, cutoff, dtype)
    assert ref.decisions_clear(steps), steps               # the inputs leave no truncation decision to rounding
    # theta up to the gauge of R: Q1 theta Q2^T is the gate on the contracted pair
    pair = np.einsum("sob,tbp->ospt", psi1.astype(np.complex128), psi2.astype(np.complex128))
    want = np.einsum("xyst,ospt->oxpy", ref.gate4(gate, d1, d2), pair)
    assert np.max(np.abs(full - want)) <= 1e-12 * max(1.0, np.max(np.abs(want))) * (1e6 if dtype == 0 else 1)
    # S, chi', truncation error
    if trunc == "none":      # nothing but exact zeros is dropped: singular values at the rounding level of a rank-deficient theta are kept or not, either way
        m = min(len(s_o), n)
        assert np.all(np.asarray(s_o)[m:] <= tol * S[0]) and np.all(S[m:] <= tol * S[0])
    else:
        m = n
        assert len(s_o) == n
    assert np.max(np.abs(S[:m] - s_o[:m])) <= tol * S[0]
    assert abs(terr - err_o) <= tol
    # psi1' (x) psi2' over the new bond
    got = np.einsum("xou,yup->oxpy", out[0].astype(np.complex128), out[1].astype(np.complex128))
    assert np.max(np.abs(new - got)) <= tol * np.max(np.abs(got))


def test_truncate_is_the_oracles_rule():
    rng = np.random.default_rng(5)
    for rt in (np.float32, np.float64):
        for _ in range(200):
            s = np.sort(np.abs(rng.standard_normal(rng.integers(1, 12))) * 10.0 ** rng.uniform(-6, 0, 1))[::-1]
            s[rng.random(len(s)) < 0.2] = 0.0
            s = np.sort(s)[::-1].astype(rt)
            md = [None, 1, 3, 50][rng.integers(4)]; co = [None, -1.0, 0.0, 1e-10, 1e-3, 0.3][rng.integers(6)]
            n, e, _ = ref.truncate(s.astype(np.float64), md, co, rt)
            n_o, e_o = o.truncate_spectrum(s * s, md, None if co is None else max(co, 0.0))
            assert n == n_o and (e == pytest.approx(e_o, rel=1e-5, abs=0) or e == e_o), (s, md, co)


# ---- tnqs_dbg_operator_sum --------------------------------------------------------------------------------------------------------------------------------------
def operator_sum(gate, d1, d2):
    g = np.ascontiguousarray(ref.flat(np.asarray(gate, dtype=np.complex128)))
    m = min(d1, d2) ** 2
    fa = np.full(m * d1 * d1, np.nan + 0j); fb = np.full(m * d2 * d2, np.nan + 0j)
    kappa = C.c_int(-1)
    rc = lib.tnqs_dbg_operator_sum(_p(g), d1, d2, C.byref(kappa), _p(fa), _p(fb))
    assert rc == 0, rc
    k = kappa.value
    assert np.all(np.isfinite(fa[:k * d1 * d1])) and np.all(np.isnan(fa[k * d1 * d1:])) and np.all(np.isfinite(fb[:k * d2 * d2])) and np.all(np.isnan(fb[k * d2 * d2:]))
    return k, fa[:k * d1 * d1], fb[:k * d2 * d2]


OPSUM = [("product", 2, 2, 1), ("Rzz", 2, 2, 2), ("Rxx", 2, 2, 2), ("CNOT", 2, 2, 2), ("CPHASE", 2, 2, 2), ("SWAP", 2, 2, 4), ("random", 2, 2, 4),
         ("product", 2, 3, 1), ("product", 3, 2, 1), ("random", 2, 3, 4), ("random", 3, 2, 4), ("SWAP", 3, 3, 9), ("random", 3, 3, 9), ("Rzz", 3, 2, 2)]


@pytest.mark.parametrize("gname,d1,d2,kappa", OPSUM, ids=[f"{g}-d{a}{b}" for g, a, b, _ in OPSUM])
def test_operator_sum(gname, d1, d2, kappa):
    gate = make_gate(gname, d1, d2, np.random.default_rng(d1 * 10 + d2))
    k, fa, fb = operator_sum(gate, d1, d2)
    assert k == kappa
    back = ref.operator_sum_gate(fa, fb, d1, d2)
    assert np.max(np.abs(back - gate)) <= 1e-13 * np.max(np.abs(gate))


def test_operator_sum_refuses_bad_arguments():
    kappa = C.c_int(-1)
    g = np.zeros(16, dtype=np.complex128)
    assert lib.tnqs_dbg_operator_sum(_p(g), 0, 2, C.byref(kappa), None, None) != 0 and kappa.value == -1
