"""Kernel-level GPU tests of the gate path's per-gate small algebra -- csrc/kernels_theta.hip (gate_theta, gate_theta_mm, lowrank_g / lowrank_m / lowrank_bw / lowrank_ll,
theta_scale, qr2_rinv / qr2_compose, gate_finish) and the small_svd_* kernels of csrc/kernels_svd.hip -- through the tnqs_dbg_gate_theta / _gate_finish / _qr2 / _small_svd
entry points of include/tnqs_debug.h, against the numpy reference of tests/gate_algebra_ref.py (pinned to the oracle in tests/test_gate_algebra_ref_cpu.py).

Every launch mixes items of different sizes: chi in 1, 3, 5, 8, 17, 32 (ragged 16 x 16 tiles, inner lengths that are no multiple of 4), one chi = 64 item (128 tiles against
the 64 waves of a gate_finish launch and the 32 of gate_theta_mm: the strided tile loops run), one chi = 128 item (the last entry of the 512-entry LDS tables; gate_theta and
gate_finish only), (d1, d2) in (2, 2), (2, 3), (3, 2).  Every output array carries guard bands that are checked after every call.

Bounds are derived (gate_algebra_ref.prod_bound), none is measured on the kernels: an f64-accumulated complex product of inner length L rounded once to the output type is within
2 (2 L + 16) 2^-53 (|A| |B|)_ij + u_T |ref_ij| of the complex128 reference, per real and imaginary part.  Each stage is compared with the reference of THAT stage on the device's
(already checked) outputs of the stage before, so no bound has to carry another stage's rounding.  Integer outputs and exact power-of-two scalings are compared with ==.
Every discrete decision of a case is asserted to be unambiguous on the test's own inputs before the device is called.  The worst measured ratio error / bound is printed
per test (MEASURED lines)."""
import ctypes as C

import numpy as np
import pytest

import tnqs_amd as tn
import tnqs_oracle as o
import gate_algebra_ref as ref

pytestmark = pytest.mark.gpu
lib = C.CDLL(tn.LIB_PATH)
lib.tnqs_last_error.restype = C.c_char_p
ERR_UNSUPPORTED = -2                                     # include/tnqs.h
GUARD = 3
EPS = 2.0 ** -52
DT_IDS = ["c64", "c128"]


def _ints(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.int32).ravel())


def _dbl(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.float64).ravel())


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _cat(parts, dt):
    parts = [np.asarray(x).ravel(order="F") for x in parts]
    return np.ascontiguousarray(np.concatenate(parts).astype(dt)) if parts else np.zeros(0, dtype=dt)


def _measured(what, ratio):
    print(f"MEASURED {what}: error / bound = {ratio:.3f}")


def _worst(pairs):
    """pairs of (error array, bound array): asserts every element is inside its bound, returns the worst ratio"""
    w = 0.0
    for e, b in pairs:
        e, b = np.atleast_1d(np.asarray(e, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
        b = np.broadcast_to(b, e.shape)
        assert np.all(np.isfinite(e)), "a non-finite output"
        bad = e > b
        assert not bad.any(), f"{int(bad.sum())} elements outside the bound, worst error {e[bad].max():.3e} against {b[bad][np.argmax(e[bad])]:.3e}"
        nz = b > 0
        if nz.any():
            w = max(w, float(np.max(e[nz] / b[nz])))
    return w


class Guarded:
    """an output array as the entry points take it: guard sentinels, item 0, guard sentinels, item 1, ..., guard sentinels"""

    def __init__(self, lens, dt, guard=GUARD):
        self.lens, self.guard = [int(l) for l in lens], guard
        sent = -7.5 + 3.25j
        self.fill = np.asarray(sent).astype(dt) if np.issubdtype(dt, np.complexfloating) else np.asarray(-7).astype(dt)
        self.start = np.cumsum([guard] + [l + guard for l in self.lens])[:-1]
        self.a = np.full(guard + sum(l + guard for l in self.lens), self.fill, dtype=dt)
        self.mask = np.ones(self.a.size, dtype=bool)
        for s, l in zip(self.start, self.lens):
            self.mask[s:s + l] = False

    def item(self, i):
        return self.a[self.start[i]:self.start[i] + self.lens[i]]

    def check(self, touched=True):
        if touched:
            assert np.all(self.a[self.mask] == self.fill), "a guard element was overwritten"
        else:
            assert np.all(self.a == self.fill), "a refused call wrote to an output"


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------------------------
def unitary(rng, n):
    q, r = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    return q * (np.diag(r) / np.abs(np.diag(r)))


def spectrum(n, span, rank=None, noise=0.0):
    """n Gram eigenvalues: `rank` of them geometric from 1 down to `span`, the others +-noise (what a rank-deficient Gram matrix leaves at the rounding level)"""
    rank = n if rank is None else rank
    lam = np.full(n, noise)
    lam[1::2] *= -1
    lam[:rank] = span ** np.linspace(0.0, 1.0, rank) if rank > 1 else 1.0
    return lam


def eigen_site(rng, n, lam):
    V = unitary(rng, n)[:, rng.permutation(n)]
    lam = np.asarray(lam, dtype=np.float64)[rng.permutation(n)]
    return dict(mode=0, F=(V * lam, V, V.copy()), n=n, rk=0)


def chol_site(rng, n, lam):
    V = unitary(rng, n)
    G = (V * lam) @ V.conj().T
    L = np.linalg.cholesky((G + G.conj().T) / 2)
    return dict(mode=1, F=(np.full((n, n), np.nan + 0j), L, np.linalg.inv(L).conj().T), n=n, rk=0)


def graded_chol_site(rng, n, piv):
    """a Cholesky site whose pivots diag(L)^2 are `piv` exactly (the ill-conditioning test of a Cholesky site reads the pivots): L = diag(sqrt(piv)) (I + strictly lower)"""
    L = np.sqrt(np.asarray(piv))[:, None] * (np.eye(n) + 0.2 * np.tril(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)), -1) / np.sqrt(n))
    return dict(mode=1, F=(np.full((n, n), np.nan + 0j), L, np.linalg.inv(L).conj().T), n=n, rk=0)


def explicit_site(rng, n, rk, lam=None, R=None):
    if R is None:
        lam = spectrum(rk, 1e-2) if lam is None else lam
        R = np.sqrt(lam)[:, None] * unitary(rng, n)[:, :rk].conj().T
    GA, GV, GW = ref.explicit_factors(R)
    GA[:] = np.nan
    return dict(mode=2, F=(GA, GV, GW), n=n, rk=rk)


def tau_of(dtype, n, shifted=False):
    t = 1e-12 if dtype == 0 else 4.0 * n * EPS
    return -4.0 * n * EPS if shifted else t


def gate_of(name, d1, d2, rng, angle=0.37):
    if (d1, d2) == (2, 2) and name in ("Rzz", "Rxx"):
        return o.gate_matrix(name, angle)
    if (d1, d2) == (2, 2) and name in ("CNOT", "SWAP"):
        return o.gate_matrix(name)
    if name == "Rzz":
        z = lambda d: np.linspace(1.0, -1.0, d)
        return np.diag(np.exp(-0.5j * angle * np.kron(z(d1), z(d2))))
    if name == "identity":
        return np.eye(d1 * d2, dtype=complex)
    assert name == "random"
    return unitary(rng, d1 * d2)


def gate_item(d1, d2, chi, s1, s2, gate, dtype, maxdim=0, tau=None):
    assert s1["n"] == d1 * chi and s2["n"] == d2 * chi
    tau = (tau_of(dtype, s1["n"]), tau_of(dtype, s2["n"])) if tau is None else tau
    return dict(d1=d1, d2=d2, chi=chi, s=(s1, s2), gate=np.asarray(gate, dtype=np.complex128), maxdim=maxdim, tau=tau)


def assert_rank_decisions_clear(items):
    for it in items:
        for sd in range(2):
            s = it["s"][sd]
            if s["mode"] == 0:
                lam, _ = ref.rayleigh(s["F"][0], s["F"][1])
                assert ref.decision_margin(lam, it["tau"][sd]) >= 100, "an eigenvalue within a factor 100 of tau * lmax"


# ---- tnqs_dbg_gate_theta ----------------------------------------------------------------------------------------------------------------------------------------
def low_sizes(dtype, items, lowrank_on, rc_want=0):
    """the host-only sizing call"""
    n = len(items)
    sizes = np.full(6 * n, -1, dtype=np.int32)
    dims = _ints([[it["d1"], it["d2"], it["chi"]] for it in items]); mode = _ints([[it["s"][0]["mode"], it["s"][1]["mode"]] for it in items])
    rk = _ints([[it["s"][0]["rk"], it["s"][1]["rk"]] for it in items]); tau = _dbl([it["tau"] for it in items]); md = _ints([it["maxdim"] for it in items])
    F1 = _cat([m for it in items for m in it["s"][0]["F"]], np.complex128); F2 = _cat([m for it in items for m in it["s"][1]["F"]], np.complex128)
    g = _cat([it["gate"] for it in items], np.complex128)
    rc = lib.tnqs_dbg_gate_theta(dtype, n, _p(dims), _p(mode), _p(rk), _p(F1), _p(F2), _p(tau), _p(g), _p(md), int(lowrank_on), 0, _p(sizes),
                                 *([None] * 16), GUARD)
    assert rc == rc_want, (rc, lib.tnqs_last_error())
    return sizes.reshape(n, 6), (dims, mode, rk, F1, F2, tau, g, md)


def gate_theta(dtype, items, lowrank_on, stop_after, texp_init=77, rc_want=0):
    n = len(items); ct = ref.CT[dtype]
    if rc_want:
        sizes = np.zeros((n, 6), dtype=np.int32)
        dims = _ints([[it["d1"], it["d2"], it["chi"]] for it in items]); mode = _ints([[it["s"][0]["mode"], it["s"][1]["mode"]] for it in items])
        rk = _ints([[0, 0] for _ in items]); tau = _dbl([it["tau"] for it in items]); md = _ints([it["maxdim"] for it in items])
        F1 = _cat([m for it in items for m in it["s"][0]["F"]], np.complex128); F2 = _cat([m for it in items for m in it["s"][1]["F"]], np.complex128)
        g = _cat([it["gate"] for it in items], np.complex128)
    else:
        sizes, (dims, mode, rk, F1, F2, tau, g, md) = low_sizes(dtype, items, lowrank_on)
    n1 = [it["d1"] * it["chi"] for it in items]; n2 = [it["d2"] * it["chi"] for it in items]
    Mr = [it["d1"] * a for it, a in zip(items, n1)]; Nc = [it["d2"] * b for it, b in zip(items, n2)]
    if rc_want:                                           # a refused launch: small arrays, which must come back untouched
        n1 = n2 = Mr = Nc = [2] * n
    G = dict(lam1=Guarded(n1, np.float64), lam2=Guarded(n2, np.float64), idx1=Guarded(n1, np.int32), idx2=Guarded(n2, np.int32),
             theta=Guarded([a * b for a, b in zip(Mr, Nc)], ct), theta0=Guarded([a * b for a, b in zip(Mr, Nc)], ct), thetaV=Guarded([max(a, b) ** 2 for a, b in zip(Mr, Nc)], ct),
             lowA=Guarded(sizes[:, 0], np.complex128), lowB=Guarded(sizes[:, 1], np.complex128), lowG=Guarded(sizes[:, 2], np.complex128),
             lowL=Guarded(sizes[:, 3], np.complex128), lowQ=Guarded(sizes[:, 4], np.complex128), lowL2c=Guarded(sizes[:, 5], np.complex128))
    info = np.full(8 * n, -9, dtype=np.int32); texp = np.full(n, texp_init, dtype=np.int32); lowfail = np.full(2 * n, -9, dtype=np.int32)
    szs = np.full(6 * n, -1, dtype=np.int32)
    rc = lib.tnqs_dbg_gate_theta(dtype, n, _p(dims), _p(mode), _p(rk), _p(F1), _p(F2), _p(tau), _p(g), _p(md), int(lowrank_on), stop_after, _p(szs), _p(info),
                                 _p(G["lam1"].a), _p(G["lam2"].a), _p(G["idx1"].a), _p(G["idx2"].a), _p(G["theta"].a), _p(G["theta0"].a), _p(G["thetaV"].a),
                                 _p(G["lowA"].a), _p(G["lowB"].a), _p(G["lowG"].a), _p(G["lowL"].a), _p(G["lowQ"].a), _p(G["lowL2c"].a), _p(texp), _p(lowfail), GUARD)
    assert rc == rc_want, (rc, lib.tnqs_last_error())
    for v in G.values():
        v.check(rc == 0)
    if rc:
        assert np.all(info == -9) and np.all(texp == texp_init) and np.all(lowfail == -9)
        return None
    out = []
    for i, it in enumerate(items):
        r = dict(info=info[8 * i:8 * i + 8].copy(), texp=int(texp[i]), lowfail=lowfail[2 * i:2 * i + 2].copy(), sizes=sizes[i].copy())
        for k, v in G.items():
            r[k] = v.item(i).copy()
        out.append(r)
    return out


def site_views(it, r):
    """(lam, idx, R, R^+) of both sites from the device's rank decision"""
    res = []
    for sd in range(2):
        s = it["s"][sd]; rr = int(r["info"][sd])
        res.append(ref.site_R(s["mode"], *s["F"], lam=r["lam%d" % (sd + 1)][:rr], idx=r["idx%d" % (sd + 1)][:rr]))
    return res


def check_rank_decision(it, r, dtype):
    """info[0, 1], idx and lam of both sites, info[6]; returns the (error, bound) pairs of lam"""
    pairs = []; bits = 0
    for sd in range(2):
        s = it["s"][sd]; n = s["n"]; rr = int(r["info"][sd]); lamd = r["lam%d" % (sd + 1)]; idxd = r["idx%d" % (sd + 1)]
        if s["mode"] == 0:
            lam_all, absl = ref.rayleigh(s["F"][0], s["F"][1])
            lam, idx = ref.kept(lam_all, it["tau"][sd])
            assert rr == len(idx) and np.array_equal(idxd[:rr], idx)
            scale = 1.0 + abs(min(it["tau"][sd], 0.0))                       # the shifted pass adds |tau| l_max: its bound is l_max's
            b = ref.prod_bound(absl[idx] + (absl.max() if it["tau"][sd] < 0 else 0.0), n, lam, ref.U64) * scale
            pairs.append((np.abs(lamd[:rr] - lam), b))
        else:
            want = n if s["mode"] == 1 else s["rk"]
            assert rr == want and np.array_equal(idxd[:rr], np.arange(rr)) and np.all(lamd[:rr] == 1.0)
            lam = lamd[:rr]
        bits |= ref.ill_conditioned(s["mode"], s["F"][1], lam) << sd
    assert int(r["info"][6]) == bits
    return pairs


def theta_geometry(it, r):
    r1, r2 = int(r["info"][0]), int(r["info"][1])
    Mr, Nc = r1 * it["d1"], r2 * it["d2"]
    wide = Mr < Nc
    assert int(r["info"][5]) == int(wide)
    return Mr, Nc, wide


def stored(r, key, Mr, Nc, wide):
    """the device's theta (or theta0) as the Mr x Nc matrix it stands for"""
    m = ref.unflat(r[key][:Mr * Nc], Nc, Mr) if wide else ref.unflat(r[key][:Mr * Nc], Mr, Nc)
    return m.conj().T if wide else m


def check_theta_copies(r, Mr, Nc, dtype):
    ne = Mr * Nc
    assert np.array_equal(r["theta0"][:ne].view(ref.RT[dtype]), r["theta"][:ne].view(ref.RT[dtype])), "theta0 != theta bitwise"
    nI = min(Mr, Nc)
    assert np.array_equal(ref.unflat(r["thetaV"][:nI * nI], nI, nI), np.eye(nI, dtype=ref.CT[dtype])), "thetaV is not the identity"


def refusal_item(dtype, rng):
    chi = 129                                             # d^2 chi = 516 > 512
    s = dict(mode=1, F=tuple(np.zeros((2, 2), dtype=complex) for _ in range(3)), n=2 * chi, rk=0)
    return dict(d1=2, d2=2, chi=chi, s=(s, s), gate=np.eye(4, dtype=complex), maxdim=0, tau=(0.0, 0.0))


@pytest.mark.parametrize("dtype", (0, 1), ids=DT_IDS)
def test_refusal_leaves_everything_untouched(dtype):
    rng = np.random.default_rng(1)
    gate_theta(dtype, [refusal_item(dtype, rng)], 1, 3, rc_want=ERR_UNSUPPORTED)
    fin = finish_item(2, 2, 129, None, np.ones(2), np.arange(2), np.eye(2), np.ones(2), np.arange(2), np.eye(2), dtype, raw=(np.eye(4), np.eye(4)), chi_cap=2)
    gate_finish(dtype, [fin], rc_want=ERR_UNSUPPORTED)


def _decision_items(dtype, rng):
    """modes 0 / 1 / 2 mixed; full rank, rank n / 2, rank 1 (a product state), shifted first pass, explicit factor with rk < n; tall and wide thetas"""
    T = lambda n, sh=False: tau_of(dtype, n, sh)
    E = lambda n, **k: eigen_site(rng, n, spectrum(n, k.pop("span", 1e-2), noise=1e-18, **k))
    items = [
        gate_item(2, 2, 1, E(2), E(2), gate_of("CNOT", 2, 2, rng), dtype),
        gate_item(2, 2, 3, E(6), chol_site(rng, 6, spectrum(6, 1e-2)), gate_of("random", 2, 2, rng), dtype),
        gate_item(2, 3, 5, E(10, rank=5), E(15), gate_of("random", 2, 3, rng), dtype),                          # rank n / 2
        gate_item(3, 2, 8, E(24, rank=1), explicit_site(rng, 16, 11), gate_of("Rzz", 3, 2, rng), dtype),         # rank 1; explicit factor, rk < n
        gate_item(2, 2, 17, E(34), E(34, rank=17), gate_of("Rzz", 2, 2, rng), dtype, tau=(T(34, True), T(34))),     # shifted: nothing dropped on site 1
        gate_item(2, 2, 32, chol_site(rng, 64, spectrum(64, 1e-2)), E(64, rank=1), gate_of("SWAP", 2, 2, rng), dtype),
        gate_item(3, 2, 5, explicit_site(rng, 15, 4), E(10), gate_of("random", 3, 2, rng), dtype),
        gate_item(2, 2, 8, E(16, rank=8), E(16, rank=8), gate_of("random", 2, 2, rng), dtype, tau=(T(16, True), T(16, True))),   # shifted with null directions: lam = |tau| lmax
    ]
    return items


@pytest.mark.parametrize("dtype", (0, 1), ids=DT_IDS)
def test_gate_theta_rank_decisions_and_elementwise_theta(dtype):
    """stop_after = gate_theta, operator-sum switch off: the element-wise loop forms theta (both dtypes)"""
    rng = np.random.default_rng(11 + dtype)
    items = _decision_items(dtype, rng)
    assert_rank_decisions_clear(items)
    res = gate_theta(dtype, items, 0, 0)
    pl, pt = [], []
    for it, r in zip(items, res):
        pl += check_rank_decision(it, r, dtype)
        (_, _, R1, _), (_, _, R2, _) = site_views(it, r)
        Mr, Nc, wide = theta_geometry(it, r)
        th, ab = ref.theta(R1, R2, it["gate"], it["d1"], it["d2"], it["chi"])
        pt.append((ref.err(stored(r, "theta", Mr, Nc, wide), th), ref.prod_bound(ab, it["d1"] * it["d2"] * it["chi"], th, ref.UT[dtype])))
        check_theta_copies(r, Mr, Nc, dtype)
        assert int(r["info"][7]) == 0 and np.all(r["sizes"] == 0)
    assert any(int(r["info"][5]) for r in res) and not all(int(r["info"][5]) for r in res)
    _measured(f"gate_theta lam ({DT_IDS[dtype]})", _worst(pl)); _measured(f"gate_theta element-wise theta ({DT_IDS[dtype]})", _worst(pt))


@pytest.mark.parametrize("dtype", (0, 1), ids=DT_IDS)
def test_gate_theta_chi128_last_lds_entry(dtype):
    """d = 2, chi = 128: n = 256, Mr = Nc = 512 -- the last entry of the 512-entry tables of gate_theta"""
    rng = np.random.default_rng(21)
    it = gate_item(2, 2, 128, eigen_site(rng, 256, spectrum(256, 1e-2)), chol_site(rng, 256, spectrum(256, 1e-2)), gate_of("Rzz", 2, 2, rng), dtype)
    assert_rank_decisions_clear([it])
    (r,) = gate_theta(dtype, [it], 0, 0)
    pl = check_rank_decision(it, r, dtype)
    (_, _, R1, _), (_, _, R2, _) = site_views(it, r)
    Mr, Nc, wide = theta_geometry(it, r)
    assert (Mr, Nc) == (512, 512)
    th, ab = ref.theta(R1, R2, it["gate"], 2, 2, 128)
    w = _worst([(ref.err(stored(r, "theta", Mr, Nc, wide), th), ref.prod_bound(ab, 512, th, ref.UT[dtype]))] + pl)
    check_theta_copies(r, Mr, Nc, dtype)
    _measured(f"gate_theta chi = 128 ({DT_IDS[dtype]})", w)


@pytest.mark.parametrize("dtype", (0, 1), ids=DT_IDS)
def test_ill_conditioning_bits(dtype):
    """info[6]: a spectrum spanning 1e-3 is not flagged, one spanning 1e-5 is, for eigen and Cholesky sites; never for an explicit factor"""
    rng = np.random.default_rng(31)
    E = lambda n, span: eigen_site(rng, n, spectrum(n, span))
    Ch = lambda n, span: graded_chol_site(rng, n, spectrum(n, span))
    g = gate_of("CNOT", 2, 2, rng)
    items = [gate_item(2, 2, 3, E(6, 1e-3), E(6, 1e-5), g, dtype), gate_item(2, 2, 5, E(10, 1e-5), Ch(10, 1e-3), g, dtype),
             gate_item(2, 2, 8, Ch(16, 1e-3), Ch(16, 1e-5), g, dtype), gate_item(2, 2, 3, Ch(6, 1e-5), explicit_site(rng, 6, 6, lam=spectrum(6, 1e-7)), g, dtype),
             gate_item(2, 2, 5, explicit_site(rng, 10, 7, lam=spectrum(7, 1e-7)), E(10, 1e-3), g, dtype)]
    assert_rank_decisions_clear(items)
    for it in items:                                      # the Cholesky pivots decide for Cholesky sites: they must be clear of 1e-4 as well
        for s in it["s"]:
            if s["mode"] == 1:
                p = np.diag(s["F"][1]).real ** 2
                assert not 0.5e-4 < p.min() / p.max() < 2e-4
    res = gate_theta(dtype, items, 0, 0)
    assert [int(r["info"][6]) for r in res] == [2, 1, 2, 1, 0]
    for it, r in zip(items, res):
        check_rank_decision(it, r, dtype)


def _mm_items(dtype, rng):
    E = lambda n, **k: eigen_site(rng, n, spectrum(n, 1e-2, noise=1e-18, **k))
    return [
        gate_item(2, 2, 1, E(2), E(2), gate_of("random", 2, 2, rng), dtype),
        gate_item(2, 3, 3, E(6), chol_site(rng, 9, spectrum(9, 1e-2)), gate_of("random", 2, 3, rng), dtype),          # wide at full rank
        gate_item(3, 2, 5, E(15), E(10), gate_of("Rzz", 3, 2, rng), dtype),                                           # tall at full rank
        gate_item(2, 2, 8, E(16, rank=8), E(16), gate_of("Rzz", 2, 2, rng), dtype),                                   # wide through the rank
        gate_item(2, 2, 17, chol_site(rng, 34, spectrum(34, 1e-2)), explicit_site(rng, 34, 20), gate_of("SWAP", 2, 2, rng), dtype),
        gate_item(2, 2, 32, E(64), E(64), gate_of("CNOT", 2, 2, rng), dtype),
        gate_item(2, 2, 64, E(128), E(128), gate_of("Rzz", 2, 2, rng), dtype),                                        # 256 tiles: the strided tile loop
    ]


def check_AB(it, r, dtype, fa, fb):
    """lowA / lowB against the reference on the device's rank decision; returns (A_dev, B_dev, pairs)"""
    (_, _, R1, _), (_, _, R2, _) = site_views(it, r)
    A, aA, B, aB = ref.operator_AB(R1, R2, fa, fb, it["d1"], it["d2"], it["chi"])
    Ad = ref.unflat(r["lowA"][:A.size], *A.shape); Bd = ref.unflat(r["lowB"][:B.size], *B.shape)
    return Ad, Bd, [(ref.err(Ad, A), ref.prod_bound(aA, it["d1"], A, ref.U64)), (ref.err(Bd, B), ref.prod_bound(aB, it["d2"], B, ref.U64))]


def opsum(gate, d1, d2):
    g = np.ascontiguousarray(ref.flat(gate))
    m = min(d1, d2) ** 2
    fa = np.zeros(m * d1 * d1, dtype=np.complex128); fb = np.zeros(m * d2 * d2, dtype=np.complex128); k = C.c_int(-1)
    assert lib.tnqs_dbg_operator_sum(_p(g), d1, d2, C.byref(k), _p(fa), _p(fb)) == 0
    return k.value, fa[:k.value * d1 * d1], fb[:k.value * d2 * d2]


@pytest.mark.parametrize("dtype", (0, 1), ids=DT_IDS)
def test_gate_theta_mm_from_factors(dtype):
    """stop_after = gate_theta_mm with the operator-sum switch on: lowA, lowB, theta = A B^T (a wide theta as the conjugated adjoint)"""
    rng = np.random.default_rng(41 + dtype)
    items = _mm_items(dtype, rng)
    assert_rank_decisions_clear(items)
    res = gate_theta(dtype, items, 1, 1)
    pa, pt = [], []
    for it, r in zip(items, res):
        check_rank_decision(it, r, dtype)
        kappa, fa, fb = opsum(it["gate"], it["d1"], it["d2"])
        Ad, Bd, pairs = check_AB(it, r, dtype, fa, fb); pa += pairs
        Mr, Nc, wide = theta_geometry(it, r)
        K = kappa * it["chi"]
        assert Ad.shape == (Mr, K) and Bd.shape == (Nc, K)
        th = Ad @ Bd.T
        pt.append((ref.err(stored(r, "theta", Mr, Nc, wide), th), ref.prod_bound(np.abs(Ad) @ np.abs(Bd).T, K, th, ref.UT[dtype])))
        check_theta_copies(r, Mr, Nc, dtype)
        # and A B^T is the theta of the element-wise definition (reference against reference: the operator sum reproduces the gate to 1e-13)
        (_, _, R1, _), (_, _, R2, _) = site_views(it, r)
        th_def, ab = ref.theta(R1, R2, it["gate"], it["d1"], it["d2"], it["chi"])
        assert np.max(np.abs(th - th_def)) <= 1e-12 * max(np.max(ab), 1e-300)
    assert any(int(r["info"][5]) for r in res) and not all(int(r["info"][5]) for r in res)
    _measured(f"lowA / lowB ({DT_IDS[dtype]})", _worst(pa)); _measured(f"gate_theta_mm theta ({DT_IDS[dtype]})", _worst(pt))


def _lowrank_items(dtype, rng):
    """Rzz at full rank with maxdim <= 2 chi: the route is taken; last item: handed out by the host (full n) but site 1 is rank-deficient, theta turns wide on the device"""
    E = lambda n, **k: eigen_site(rng, n, spectrum(n, 1e-2, noise=1e-18, **k))
    its = [gate_item(2, 2, chi, E(2 * chi), chol_site(rng, 2 * chi, spectrum(2 * chi, 1e-2)) if chi % 2 else E(2 * chi), gate_of("Rzz", 2, 2, rng), dtype, maxdim=md)
           for chi, md in ((3, 6), (5, 7), (8, 16), (17, 20), (32, 32))]
    its.append(gate_item(3, 2, 5, E(15), E(10), gate_of("Rzz", 3, 2, rng), dtype, maxdim=10))
    its.append(gate_item(2, 2, 8, E(16, rank=7), E(16), gate_of("Rzz", 2, 2, rng), dtype, maxdim=8))
    return its


def host_rule(it, dtype, kappa):
    """gate_items(): K < Nc && K <= 128 && cap <= K && Mr >= Nc && lds_fits, and the lowQ condition (ComplexF32, the preconditioned kernel covers Mr x K, K <= 96)"""
    Mr, Nc, K = it["d1"] ** 2 * it["chi"], it["d2"] ** 2 * it["chi"], kappa * it["chi"]
    cap = min(Mr, Nc) if it["maxdim"] <= 0 else min(Mr, Nc, it["maxdim"])
    lds_fits = dtype == 0 or (Mr + 2) * K * 16 <= 160 * 1024 - 2048
    low = kappa > 0 and K < Nc and K <= 128 and cap <= K and Mr >= Nc and lds_fits
    lowq = low and dtype == 0 and 2 <= K <= 64 and K <= Mr <= 128
    return [Mr * K, Nc * K, K * K * low, K * K * low, Nc * K * lowq, 2 * K * K * (low and dtype == 1)]


@pytest.mark.parametrize("dtype", (0, 1), ids=DT_IDS)
def test_lowrank_route(dtype):
    rng = np.random.default_rng(51 + dtype)
    items = _lowrank_items(dtype, rng)
    assert_rank_decisions_clear(items)
    res = gate_theta(dtype, items, 1, 2)
    pg, pm, pq = [], [], []
    for i, (it, r) in enumerate(zip(items, res)):
        kappa, fa, fb = opsum(it["gate"], it["d1"], it["d2"])
        assert kappa == 2 and list(r["sizes"]) == host_rule(it, dtype, kappa) and r["sizes"][2] > 0
        Ad, Bd, _ = check_AB(it, r, dtype, fa, fb)
        Mr, Nc, wide = theta_geometry(it, r)
        K = kappa * it["chi"]
        G = ref.unflat(r["lowG"], K, K)
        full = stored(r, "theta0", Mr, Nc, wide)
        if i == len(items) - 1:                           # not taken on the device: identity lowG, theta stays the full theta
            # (ComplexF64: the second pass's flag is not asserted here -- with info[7] = 0 lowrank_g leaves G2 unwritten, its Cholesky factors whatever the workspace
            #  held, and lowrank_ll returns before it would fold that flag into the gate's: only lowfail[0] means anything where the route is not taken)
            assert wide and int(r["info"][7]) == 0 and np.array_equal(G, np.eye(K)) and r["lowfail"][0] == 0
            assert np.array_equal(r["theta"][:Mr * Nc].view(ref.RT[dtype]), r["theta0"][:Mr * Nc].view(ref.RT[dtype]))
            continue
        assert not wide and int(r["info"][7]) == K and list(r["lowfail"]) == [0, 0]
        assert np.array_equal(G, G.conj().T), "lowG is not mirrored exactly"
        Gr = Bd.conj().T @ Bd
        pg.append((ref.err(G, Gr), ref.prod_bound(np.abs(Bd).T @ np.abs(Bd), Nc, Gr, ref.U64)))
        L = ref.unflat(r["lowL"], K, K)
        assert np.all(np.triu(L, 1) == 0)
        if dtype == 1:                                    # CholeskyQR2: Lc = L1 L2 lower triangular, theta[:, :K] = A conj(Lc)
            L2 = ref.unflat(r["lowL2c"][:K * K], K, K); Lc = ref.unflat(r["lowL2c"][K * K:], K, K)
            assert np.all(np.triu(Lc, 1) == 0), "Lc is not lower triangular"
            Lr = L @ np.tril(L2)
            pm.append((ref.err(Lc, Lr), ref.prod_bound(np.abs(L) @ np.abs(np.tril(L2)), K, Lr, ref.U64)))
            L = Lc
        M = Ad @ L.conj()
        Md = ref.unflat(r["theta"][:Mr * K], Mr, K)
        pm.append((ref.err(Md, M), ref.prod_bound(np.abs(Ad) @ np.abs(L), K, M, ref.UT[dtype])))
        # theta0 keeps the full theta = A B^T; the columns of theta beyond K keep it too
        th = Ad @ Bd.T
        assert np.max(ref.err(full, th) - ref.prod_bound(np.abs(Ad) @ np.abs(Bd).T, K, th, ref.UT[dtype])) <= 0
        assert np.array_equal(r["theta"][Mr * K:Mr * Nc].view(ref.RT[dtype]), r["theta0"][Mr * K:Mr * Nc].view(ref.RT[dtype]))
        if r["sizes"][4]:                                 # Q = B L^-dagger: Q^dagger Q = I.  CholeskyQR in f64 (Yamamoto et al. 2015, Lemma 3.1 ff.):
            Q = ref.unflat(r["lowQ"], Nc, K)              # ||Q^dagger Q - I||_2 <= (5 / 64) * 64 (m n + n (n + 1)) u kappa(B)^2 = 5 (m n + n (n + 1)) u kappa(B)^2
            e = np.linalg.norm(Q.conj().T @ Q - np.eye(K), 2)
            pq.append((e, 5.0 * (Nc * K + K * (K + 1)) * ref.U64 * np.linalg.cond(Bd) ** 2))
            assert np.linalg.cond(Bd) < 1e3
    assert (dtype == 0) == bool(pq)
    _measured(f"lowG ({DT_IDS[dtype]})", _worst(pg)); _measured(f"lowrank_m / lowrank_ll ({DT_IDS[dtype]})", _worst(pm))
    if pq:
        _measured("Q^dagger Q - I", _worst(pq))


@pytest.mark.parametrize("dtype", (0, 1), ids=DT_IDS)
def test_lowrank_route_withdrawn(dtype):
    """a refused Cholesky pivot of B^dagger B: the failure flag is set, lowrank_m takes info[7] back to 0 and theta stays the full theta.  Item 0 is Rzz with the tiny
    angle 1e-8: kappa = 2, but the operator sum (elimination with complete pivoting: b_1 ~ 1, b_2 = |1><1|) gives a WELL conditioned B, so its route stays -- asserted
    as such.  Items 1, 2 have two equal bond columns in R2, which makes two columns of B equal: a pivot of B^dagger B is zero to rounding.  (ComplexF64: the second
    pass cannot refuse where the first accepted -- a first pivot above 1e-12 of the largest means cond(B) < 1e6, and then B1^dagger B1 = I + O(cond(B)^2 2^-53) has
    pivots within 1e-4 of 1, far from the second pass's 1e-3 -- so the folding of its flag in lowrank_ll has no reachable input; where the route is taken both flags are
    asserted to be 0, test_lowrank_route)"""
    rng = np.random.default_rng(61 + dtype)
    E = lambda n: eigen_site(rng, n, spectrum(n, 1e-2))
    def dup(n, d, chi):
        R = unitary(rng, n).reshape(n, chi, d)
        R[:, chi - 1, :] = R[:, 1, :]
        return explicit_site(rng, n, n, R=R.reshape(n, n))
    items = [gate_item(2, 2, 8, E(16), E(16), gate_of("Rzz", 2, 2, rng, angle=1e-8), dtype, maxdim=16),
             gate_item(2, 2, 5, E(10), dup(10, 2, 5), gate_of("Rzz", 2, 2, rng), dtype, maxdim=10),
             gate_item(2, 2, 17, E(34), dup(34, 2, 17), gate_of("Rzz", 2, 2, rng), dtype, maxdim=20)]
    assert_rank_decisions_clear(items)
    res = gate_theta(dtype, items, 1, 2)
    tau = 1e-12                                           # run_theta: rank_tau(f32) = 1e-12 for ComplexF32 and 1e-12 on the pivots of pass 1 for ComplexF64
    pt = []
    for i, (it, r) in enumerate(zip(items, res)):
        kappa, fa, fb = opsum(it["gate"], 2, 2)
        assert kappa == 2 and r["sizes"][2] > 0
        Ad, Bd, _ = check_AB(it, r, dtype, fa, fb)
        Mr, Nc, wide = theta_geometry(it, r)
        K = 2 * it["chi"]
        G = Bd.conj().T @ Bd
        ev = np.linalg.eigvalsh(G)
        if i == 0:
            assert ev[0] > 1e-3 * np.max(np.diag(G).real)         # well conditioned: every pivot is far above the threshold
            assert int(r["info"][7]) == K and list(r["lowfail"]) == [0, 0]
            continue
        # unambiguous: the smallest pivot is at most the smallest eigenvalue bound ... a zero eigenvalue to rounding, a factor 100 below tau * max diagonal
        assert abs(ev[0]) < 1e-2 * tau * np.max(np.diag(G).real)
        assert r["lowfail"][0] == 1 and int(r["info"][7]) == 0
        th = Ad @ Bd.T
        pt.append((ref.err(stored(r, "theta", Mr, Nc, wide), th), ref.prod_bound(np.abs(Ad) @ np.abs(Bd).T, K, th, ref.UT[dtype])))
        assert np.array_equal(r["theta"][:Mr * Nc].view(ref.RT[dtype]), r["theta0"][:Mr * Nc].view(ref.RT[dtype]))
    _measured(f"theta after the withdrawal ({DT_IDS[dtype]})", _worst(pt))


def _scale_item(dtype, rng, r1diag, second=1.0):
    """chi = 1, d = 2, identity gate, explicit factors R1 = diag(r1diag), R2 = second * identity: theta[(a, s1'), (c, s2')] = R1[a, s1'] R2[c, s2'], exact products"""
    return gate_item(2, 2, 1, explicit_site(rng, 2, 2, R=np.diag(r1diag).astype(complex)), explicit_site(rng, 2, 2, R=second * np.eye(2, dtype=complex)),
                     gate_of("identity", 2, 2, rng), dtype)


@pytest.mark.parametrize("dtype", (0, 1), ids=DT_IDS)
@pytest.mark.parametrize("lowrank_on", (0, 1), ids=("loop", "factors"))
def test_theta_scale_is_exact(dtype, lowrank_on):
    rng = np.random.default_rng(71)
    f32 = lambda x: float(np.float32(x))
    items = [_scale_item(dtype, rng, [2.0 ** 7, 2.0 ** 3]),                       # a largest entry exactly 2^k
             _scale_item(dtype, rng, [2.0 ** -9, 2.0 ** -9 * 0.75]),
             _scale_item(dtype, rng, [f32(1e-30), f32(3e-31)]),
             _scale_item(dtype, rng, [f32(1e30), f32(7e29)]),
             _scale_item(dtype, rng, [0.0, 0.0]),                                 # all-zero theta: texp 0
             _scale_item(dtype, rng, [1.5, -0.3], second=1j)]                     # the largest entry is an imaginary part
    E = lambda n: eigen_site(rng, n, spectrum(n, 1e-2))
    items.append(gate_item(2, 3, 5, E(10), E(15), gate_of("random", 2, 3, rng), dtype))      # a wide, generic theta
    if dtype == 1:                                        # ComplexF64 entries outside the float range: texp 0, as documented at theta_scale_kernel
        items += [_scale_item(dtype, rng, [1e60, 1e59]), _scale_item(dtype, rng, [1e-60, 1e-61])]
    a = gate_theta(dtype, items, lowrank_on, 2); b = gate_theta(dtype, items, lowrank_on, 3)
    want = [-7, 9, None, None, 0, 0, None] + [0, 0]
    for i, (it, ra, rb) in enumerate(zip(items, a, b)):
        Mr, Nc, _ = theta_geometry(it, ra)
        ne = Mr * Nc
        ta = ra["theta0"][:ne]
        assert np.array_equal(ra["info"], rb["info"]) and ra["texp"] == 77         # theta_scale did not run in `a`: texp as the caller filled it
        with np.errstate(over="ignore"):
            mx = float(np.max(np.maximum(np.abs(ta.real), np.abs(ta.imag)).astype(np.float32))) if ne else 0.0
        k = 0
        if 0 < mx < 3e38:
            k = int(np.clip(-(int(np.floor(np.log2(mx)))), -120, 120))
        assert rb["texp"] == k, (i, rb["texp"], k)
        if want[i] is not None:
            assert k == want[i], (i, k)
        if i in (2, 3):
            assert k == (100 if i == 2 else -99)
        for key in ("theta", "theta0"):
            assert np.array_equal((ra[key][:ne] * ref.RT[dtype](2.0) ** k).view(ref.RT[dtype]), rb[key][:ne].view(ref.RT[dtype])), (i, key)
        dyn = np.abs(np.concatenate([ta.real, ta.imag])); dyn = dyn[dyn > 0]
        assert len(dyn) == 0 or dyn.max() / dyn.min() < 2.0 ** 100              # nothing goes subnormal


# ---- tnqs_dbg_gate_finish -----------------------------------------------------------------------------------------------------------------------------------------
def finish_item(d1, d2, chi, th, lam1, idx1, GW1, lam2, idx2, GW2, dtype, maxdim=0, cutoff=-1.0, normalize=0, chi_cap=None, texp=0, K=0, rng=None, shuffle=True, raw=None):
    """th: the reference theta (r1 d1 x r2 d2, complex128).  U Sigma and V of LAPACK's SVD, scaled by 2^texp, rounded to T, columns shuffled; K > 0: only the first K triplets
    are handed over (the low-rank route: columns >= K count as zero and hold NaN here).  raw = (theta columns, thetaV): given as they are instead"""
    ct = ref.CT[dtype]
    r1, r2 = len(lam1), len(lam2)
    Mr, Nc = r1 * d1, r2 * d2
    wide = Mr < Nc
    ncol = min(Mr, Nc)
    if raw is None:
        M = th.conj().T if wide else th
        U, S, Vh = np.linalg.svd(M, full_matrices=False)
        perm = rng.permutation(ncol) if shuffle else np.arange(ncol)
        if K:
            perm = np.concatenate([rng.permutation(K), np.arange(K, ncol)])
        cols = ((U * S) * 2.0 ** texp)[:, perm].astype(ct); tv = Vh.conj().T[:, perm].astype(ct)
        if K:
            cols[:, K:] = np.nan; tv[:, K:] = np.nan
    else:
        cols, tv = (np.asarray(x).astype(ct) for x in raw)
    n1, n2 = d1 * chi, d2 * chi
    pad = lambda v, n, dt: np.concatenate([np.asarray(v, dtype=dt), np.zeros(n - len(v), dtype=dt)])
    return dict(d1=d1, d2=d2, chi=chi, r1=r1, r2=r2, wide=wide, K=K, texp=texp, cols=cols, tv=tv, lam1=pad(lam1, n1, np.float64), lam2=pad(lam2, n2, np.float64),
                idx1=pad(idx1, n1, np.int32), idx2=pad(idx2, n2, np.int32), GW1=np.asarray(GW1, dtype=np.complex128), GW2=np.asarray(GW2, dtype=np.complex128),
                maxdim=maxdim, cutoff=cutoff, normalize=normalize, chi_cap=min(d1 * n1, d2 * n2) if chi_cap is None else chi_cap)


def gate_finish(dtype, items, rc_want=0):
    n = len(items); ct = ref.CT[dtype]
    dims = _ints([[it["d1"], it["d2"], it["chi"]] for it in items]); info_in = _ints([[it["r1"], it["r2"], it["wide"], it["K"]] for it in items])
    texp = _ints([it["texp"] for it in items])
    th = _cat([it["cols"] for it in items], ct); tv = _cat([it["tv"] for it in items], ct)
    lam1 = _cat([it["lam1"] for it in items], np.float64); lam2 = _cat([it["lam2"] for it in items], np.float64)
    idx1 = _cat([it["idx1"] for it in items], np.int32); idx2 = _cat([it["idx2"] for it in items], np.int32)
    W1 = _cat([it["GW1"] for it in items], np.complex128); W2 = _cat([it["GW2"] for it in items], np.complex128)
    md = _ints([it["maxdim"] for it in items]); co = _dbl([it["cutoff"] for it in items]); nz = _ints([it["normalize"] for it in items]); cap = _ints([it["chi_cap"] for it in items])
    small = rc_want != 0
    S = Guarded([2 if small else it["chi_cap"] for it in items], np.float64)
    X1 = Guarded([2 if small else it["d1"] * it["chi"] * it["d1"] * it["chi_cap"] for it in items], ct)
    X2 = Guarded([2 if small else it["d2"] * it["chi"] * it["d2"] * it["chi_cap"] for it in items], ct)
    info = np.full(2 * n, -9, dtype=np.int32); terr = np.full(n, -5.0)
    rc = lib.tnqs_dbg_gate_finish(dtype, n, _p(dims), _p(info_in), _p(texp), _p(th), _p(tv), _p(lam1), _p(lam2), _p(idx1), _p(idx2), _p(W1), _p(W2), _p(md), _p(co), _p(nz), _p(cap),
                                  _p(S.a), _p(info), _p(terr), _p(X1.a), _p(X2.a), GUARD)
    assert rc == rc_want, (rc, lib.tnqs_last_error())
    S.check(rc == 0); X1.check(rc == 0); X2.check(rc == 0)
    if rc:
        assert np.all(info == -9) and np.all(terr == -5.0)
        return None
    out = []
    for i, it in enumerate(items):
        nk = int(info[2 * i])
        assert 1 <= nk <= it["chi_cap"]
        n1, n2 = it["d1"] * it["chi"], it["d2"] * it["chi"]
        out.append(dict(nk=nk, status=int(info[2 * i + 1]), terr=float(terr[i]), S=S.item(i)[:nk].copy(), S_rest=S.item(i)[nk:].copy(),
                        X1=ref.unflat(X1.item(i)[:n1 * it["d1"] * nk], n1, it["d1"] * nk), X2=ref.unflat(X2.item(i)[:n2 * it["d2"] * nk], n2, it["d2"] * nk)))
    return out


def finish_reference(it, dtype):
    """from the item's own (rounded) inputs: sig (ranked, stable), chi', status, truncerr, S, X1, X2 and the bounds of S, truncerr, X1, X2"""
    rt = ref.RT[dtype]; uT = ref.UT[dtype]
    cols = it["cols"].astype(np.complex128); tv = it["tv"].astype(np.complex128)
    ld, ncol = cols.shape
    ncolK = it["K"] if (it["K"] > 0 and not it["wide"]) else ncol
    tsc = 2.0 ** -it["texp"]
    s2 = np.zeros(ncol)
    with np.errstate(invalid="ignore", over="ignore"):
        s2[:ncolK] = np.sum((np.abs(cols[:, :ncolK].real).astype(np.longdouble)) ** 2 + (np.abs(cols[:, :ncolK].imag).astype(np.longdouble)) ** 2, axis=0).astype(np.float64)
    ok = np.isfinite(s2) & (s2 < 1e300)
    sig = np.where(ok, np.sqrt(np.where(ok, s2, 0.0)) * tsc, 0.0)
    perm = np.argsort(-sig, kind="stable")
    nsv = ncol
    n, terr, steps = ref.truncate(sig[perm], it["maxdim"], it["cutoff"], rt)
    status = 0
    if n > it["chi_cap"]:
        status, n = 1, it["chi_cap"]
    sk = sig[perm[:n]]
    rel_s = (2 * ld + 16) * ref.U64
    if it["normalize"] and np.sqrt(np.sum(sk ** 2)) > 0:
        nrm = np.sqrt(np.sum(sk ** 2))
        S = (sk.astype(rt) / rt(nrm)).astype(np.float64)
        a = 2 * rel_s + (n + 2) * ref.U64 + 3 * uT         # s and nrm each within rel_s (nrm: n more additions), three roundings to T; a + a^2 carries the products of these relative errors
        bS = (a + a * a) * np.abs(S)
    else:
        S = sk.astype(rt).astype(np.float64)
        a = rel_s + uT                                     # the column norm, one rounding to T
        bS = (a + a * a) * np.abs(S)
    bterr = (2 * nsv + 8) * uT * terr + 4 * rel_s * terr
    r1, r2, d1, d2 = it["r1"], it["r2"], it["d1"], it["d2"]
    Rp1 = it["GW1"][:, it["idx1"][:r1]] / np.sqrt(it["lam1"][:r1])[None, :]
    Rp2 = it["GW2"][:, it["idx2"][:r2]] / np.sqrt(it["lam2"][:r2])[None, :]
    pos = sk > 0
    sq = np.sqrt(np.where(pos, sk, 1.0))
    z = lambda m: np.where(np.isfinite(m), m, 0.0)
    if not it["wide"]:
        Lf = np.where(pos[None, :], z(cols[:, perm[:n]]) * tsc / sq[None, :], 0.0)              # U sqrt(S), rows a + r1 s1'
        Rf = z(tv[:, perm[:n]]).conj() * np.where(pos, sq, 0.0)[None, :]                       # (sqrt(S) V^dagger)^T, rows c + r2 s2'
    else:
        Lf = np.where(pos[None, :], z(tv[:, perm[:n]]) * sq[None, :], 0.0)
        Rf = np.where(pos[None, :], z(cols[:, perm[:n]]).conj() * tsc / sq[None, :], 0.0)

    def wrap(Rp, F, d, r):                                # X[(s, b), s' + d u] = sum_a Rp[(s, b), a] F[a + r s', u]
        return np.einsum("ia,xau->iux", Rp, F.reshape(d, r, n), optimize=True).reshape(Rp.shape[0], -1)
    X1, X2 = wrap(Rp1, Lf, d1, r1), wrap(Rp2, Rf, d2, r2)
    b1 = ref.prod_bound(wrap(np.abs(Rp1), np.abs(Lf), d1, r1), r1, X1, uT)
    b2 = ref.prod_bound(wrap(np.abs(Rp2), np.abs(Rf), d2, r2), r2, X2, uT)
    return dict(sig=sig, perm=perm, nk=n, status=status, terr=terr, steps=steps, S=S, bS=bS, bterr=bterr, X1=X1, X2=X2, b1=b1, b2=b2, Lf=Lf, Rf=Rf, Rp1=Rp1, Rp2=Rp2)


def check_finish(it, out, dtype, exact_case=False, th=None):
    """the device's result of one item against finish_reference; returns the (error, bound) pairs"""
    fr = finish_reference(it, dtype)
    if not exact_case:
        assert ref.decisions_clear(fr["steps"]), ("an ambiguous truncation decision in the test's inputs", fr["steps"])
    assert out["nk"] == fr["nk"] and out["status"] == fr["status"], (out["nk"], fr["nk"], out["status"], fr["status"])
    nk = fr["nk"]; d1, d2 = it["d1"], it["d2"]
    pairs = [(np.abs(out["S"] - fr["S"]), fr["bS"]), (abs(out["terr"] - fr["terr"]), fr["bterr"]),
             (ref.err(out["X1"], fr["X1"]), fr["b1"]), (ref.err(out["X2"], fr["X2"]), fr["b2"])]
    assert np.all(np.diff(out["S"]) <= 0) and np.all(np.isfinite(out["X1"])) and np.all(np.isfinite(out["X2"]))
    # (i) R1 X1 reshaped to ((a, s1'), u): mutually orthogonal columns of norm sqrt(sigma_u) -- up to what the (rounded) input columns themselves are off by
    lam1 = it["lam1"][:it["r1"]]
    R1 = np.sqrt(lam1)[:, None] * np.linalg.pinv(fr["Rp1"] * np.sqrt(lam1)[None, :])          # R1 with R1 R1^+ = I on the kept columns
    Ld = np.einsum("ai,iux->xau", R1, out["X1"].astype(np.complex128).reshape(-1, nk, d1), optimize=True).reshape(-1, nk)
    Lr = fr["Lf"]
    e = np.einsum("ai,iux->xau", np.abs(R1), fr["b1"].reshape(-1, nk, d1), optimize=True).reshape(-1, nk) + 2 * (2 * R1.shape[1] + 16) * ref.U64 * \
        np.einsum("ai,iux->xau", np.abs(R1), np.abs(fr["X1"]).reshape(-1, nk, d1), optimize=True).reshape(-1, nk)
    Gd = Ld.conj().T @ Ld
    Gr = Lr.conj().T @ Lr
    bG = e.T @ np.abs(Lr) + np.abs(Lr).T @ e + e.T @ e
    cond1 = np.linalg.cond(fr["Rp1"])
    bG = bG + 64 * cond1 * ref.U64 * (np.abs(Lr).T @ np.abs(Lr))                          # pinv in f64: relative error <= c cond u on the reference product itself
    sigk = fr["sig"][fr["perm"][:nk]]
    defect = np.abs(Gr - np.diag(sigk))                                                             # the rounded input columns' own departure from orthogonality
    pairs.append((np.abs(Gd - np.diag(sigk)), bG + defect))
    # (ii) sum_u X1[:, (s1', u)] X2[:, (s2', u)] = R1^+ theta_chi' R2^+T
    Pd = ref.pair_product(out["X1"], out["X2"], d1, d2, nk)
    a1, a2 = np.abs(fr["X1"]).reshape(-1, nk, d1), np.abs(fr["X2"]).reshape(-1, nk, d2)
    e1, e2 = fr["b1"].reshape(-1, nk, d1), fr["b2"].reshape(-1, nk, d2)
    bP = np.einsum("iux,juy->ixjy", e1, a2) + np.einsum("iux,juy->ixjy", a1, e2) + np.einsum("iux,juy->ixjy", e1, e2)
    if th is not None and not np.any(~np.isfinite(it["cols"])) and it["K"] == 0:
        Pt, absP = ref.truncated_theta_product(th, nk, fr["Rp1"], fr["Rp2"], d1, d2)
        L = it["r1"] + it["r2"] + nk
        pairs.append((ref.err(Pd, Pt), bP + (3 * ref.UT[dtype] + 2 * (2 * L + 16) * ref.U64) * absP))
    else:
        Pr = ref.pair_product(fr["X1"], fr["X2"], d1, d2, nk)
        pairs.append((ref.err(Pd, Pr), bP + 2 * (2 * nk + 16) * ref.U64 * np.einsum("iux,juy->ixjy", a1, a2)))
    return pairs, fr


def _finish_problem(rng, d1, d2, chi, r1, r2, dtype, spec=None, **kw):
    """a reference theta with the singular spectrum `spec` (default: geometric over 1e-4) on random R^+ interfaces (idx a proper subset where r < n)"""
    n1, n2 = d1 * chi, d2 * chi
    Mr, Nc = r1 * d1, r2 * d2
    nsv = min(Mr, Nc)
    spec = 1e-4 ** np.linspace(0, 1, nsv) if spec is None else np.asarray(spec, dtype=float)
    U = unitary(rng, Mr)[:, :nsv]; V = unitary(rng, Nc)[:, :nsv]
    th = (U * spec) @ V.conj().T
    idx1 = np.sort(rng.permutation(n1)[:r1]); idx2 = np.sort(rng.permutation(n2)[:r2])
    lam1 = 10.0 ** rng.uniform(-2, 0, r1); lam2 = 10.0 ** rng.uniform(-2, 0, r2)
    return th, finish_item(d1, d2, chi, th, lam1, idx1, unitary(rng, n1), lam2, idx2, unitary(rng, n2), dtype, rng=rng, **kw)


GRID = [(md, co, nz) for md in ("none", 1, "chi", "above") for co in (-1.0, 0.0, 1e-10, 1e-3) for nz in (0, 1)]


@pytest.mark.parametrize("dtype", (0, 1), ids=DT_IDS)
def test_gate_finish_truncation_grid(dtype):
    """maxdim in {none, 1, chi, above nsv} x cutoff in {negative, 0, 1e-10, 1e-3} x normalize, over items of different sizes in ONE launch per shape group"""
    rng = np.random.default_rng(81 + dtype)
    shapes = [(2, 2, 3, 6, 6), (2, 3, 5, 10, 15), (3, 2, 8, 24, 16), (2, 2, 17, 34, 20), (2, 2, 1, 2, 2), (2, 2, 32, 64, 64), (2, 2, 5, 4, 10), (2, 3, 8, 16, 13)]
    items, ths = [], []
    for k, (md, co, nz) in enumerate(GRID):
        d1, d2, chi, r1, r2 = shapes[k % len(shapes)]
        nsv = min(r1 * d1, r2 * d2)
        maxdim = {"none": 0, 1: 1, "chi": chi, "above": nsv + 3}[md]
        # spectrum: geometric in sigma over 1e-4 (p over 1e-8): cutoffs 1e-10 and 1e-3 fall between two of its partial sums unless asserted otherwise
        th, it = _finish_problem(rng, d1, d2, chi, r1, r2, dtype, maxdim=maxdim, cutoff=co, normalize=nz, texp=(k % 5) - 2)
        items.append(it); ths.append(th)
    res = gate_finish(dtype, items)
    pairs = []; kept = set()
    for it, th, out in zip(items, ths, res):
        p, fr = check_finish(it, out, dtype, th=th); pairs += p
        assert out["status"] == 0
        kept.add((out["nk"] == min(it["r1"] * it["d1"], it["r2"] * it["d2"])))
    assert kept == {True, False}
    assert any(it["wide"] for it in items) and not all(it["wide"] for it in items)
    _measured(f"gate_finish grid ({DT_IDS[dtype]})", _worst(pairs))


@pytest.mark.parametrize("dtype", (0, 1), ids=DT_IDS)
def test_gate_finish_cap_texp_lowrank_and_large(dtype):
    """chi_cap below chi' (status 1); a texp != 0 whose factor reappears in S; the low-rank route's info[7] = K < ncol (columns >= K hold NaN and count as zero);
    chi = 64 (128 tiles against 64 waves) and chi = 128 (Mr = Nc = 512: the last entry of the LDS tables)"""
    rng = np.random.default_rng(91 + dtype)
    items, ths = [], []
    def add(*a, **k):
        th, it = _finish_problem(rng, *a, dtype, **k); items.append(it); ths.append(th)
    add(2, 2, 8, 16, 16, chi_cap=5, cutoff=1e-10)                                             # chi' = more than 5 -> status 1, 5 kept
    add(2, 3, 5, 10, 15, chi_cap=3, maxdim=7)
    add(2, 2, 3, 6, 6, texp=37, normalize=0); add(3, 2, 5, 15, 10, texp=-41, normalize=1); add(2, 3, 5, 10, 15, texp=120)
    K = 16
    add(2, 2, 8, 16, 16, spec=np.concatenate([1e-3 ** np.linspace(0, 1, K), np.zeros(16)]), K=K, chi_cap=K, maxdim=K, cutoff=1e-12)
    add(3, 2, 5, 15, 10, spec=np.concatenate([1e-2 ** np.linspace(0, 1, 10), np.zeros(10)]), K=10, chi_cap=10, maxdim=10)
    add(2, 2, 64, 128, 128, maxdim=64, cutoff=1e-10, normalize=1)
    add(2, 2, 128, 256, 256, maxdim=16, cutoff=1e-12, texp=3)
    res = gate_finish(dtype, items)
    pairs = []
    for i, (it, th, out) in enumerate(zip(items, ths, res)):
        p, fr = check_finish(it, out, dtype, th=th); pairs += p
        assert out["status"] == (1 if i < 2 else 0)
        if i < 2:
            assert out["nk"] == it["chi_cap"]
    # the factor 2^texp reappears in S: the same problem at texp = 0 gives the same S bit for bit (power-of-two scaling is exact)
    again = dict(items[2]); again["texp"] = 0; again["cols"] = (items[2]["cols"].astype(np.complex128) * 2.0 ** -37).astype(ref.CT[dtype])
    (o0,) = gate_finish(dtype, [again])
    assert np.array_equal(o0["S"], res[2]["S"]) and o0["terr"] == res[2]["terr"] and np.array_equal(o0["X1"], res[2]["X1"]) and np.array_equal(o0["X2"], res[2]["X2"])
    _measured(f"gate_finish cap / texp / low-rank / chi 64, 128 ({DT_IDS[dtype]})", _worst(pairs))


def _exact_items(dtype):
    """columns sigma e_i with sigma = 1/2 three times and 1/4 four times (d = 1, chi = 7, identity R factors): p = 1/4 x 3, 1/16 x 4, scale exactly 1 in f32 and f64"""
    sig = np.array([0.25, 0.5, 0.25, 0.25, 0.5, 0.25, 0.5])
    cols = np.diag(sig).astype(complex)
    mk = lambda **kw: finish_item(1, 1, 7, None, np.ones(7), np.arange(7), np.eye(7), np.ones(7), np.arange(7), np.eye(7), dtype, raw=(cols, np.eye(7)), **kw)
    return sig, [mk(cutoff=0.125), mk(cutoff=0.125, maxdim=2), mk(cutoff=0.0625), mk(cutoff=0.1875)]


@pytest.mark.parametrize("dtype", (0, 1), ids=DT_IDS)
def test_gate_finish_exact_boundary_and_stable_ranking(dtype):
    """cutoff = 0.125 on p = 1/4, 1/4, 1/4, 1/16 x 4: the <= rule keeps 5 with truncerr = 0.125 exactly (a < would keep 6); maxdim = 2 keeps the two lowest-indexed
    columns of the tie at sigma = 1/2 (stable ranking)"""
    sig, items = _exact_items(dtype)
    res = gate_finish(dtype, items)
    assert (res[0]["nk"], res[0]["terr"]) == (5, 0.125)
    assert np.array_equal(res[0]["S"], [0.5, 0.5, 0.5, 0.25, 0.25])
    # X1[:, u] = sqrt(sigma) e_perm(u): the kept columns in rank order -- the 1/2 columns 1, 4, 6, then the lowest-indexed 1/4 columns 0, 2
    order = [int(np.argmax(np.abs(res[0]["X1"][:, u]))) for u in range(5)]
    assert order == [1, 4, 6, 0, 2]
    assert (res[1]["nk"], res[1]["terr"]) == (2, 0.5) and [int(np.argmax(np.abs(res[1]["X1"][:, u]))) for u in range(2)] == [1, 4]
    assert (res[2]["nk"], res[2]["terr"]) == (6, 0.0625) and (res[3]["nk"], res[3]["terr"]) == (4, 0.1875)
    for it, out in zip(items, res):
        check_finish(it, out, dtype, exact_case=True)
        nk = out["nk"]
        X = np.zeros((7, nk)); p = np.argsort(-sig, kind="stable")[:nk]; X[p, np.arange(nk)] = np.sqrt(sig[p])
        for Xd in (out["X1"], out["X2"]):                 # sqrt(sigma) e_perm(u), nothing else: zeros exactly; the value after a reciprocal square root, a product and the rounding to T
            assert np.array_equal(Xd != 0, X != 0) and np.max(np.abs(Xd - X) - (4 * ref.U64 + ref.UT[dtype]) * X) <= 0


@pytest.mark.parametrize("dtype", (0, 1), ids=DT_IDS)
def test_gate_finish_zero_theta_and_nan_column(dtype):
    rng = np.random.default_rng(101)
    # p0 = 0: chi' = 1, finite output
    zt, zw = [], []
    for (d1, d2, chi, r1, r2) in ((2, 2, 3, 6, 6), (2, 3, 5, 10, 15)):
        th, it = _finish_problem(rng, d1, d2, chi, r1, r2, dtype, spec=np.zeros(min(r1 * d1, r2 * d2)), normalize=1, cutoff=1e-10)
        it["cols"][:] = 0
        zt.append(it)
    # one NaN column: ranked last, never kept
    items = list(zt)
    for (d1, d2, chi, r1, r2, md, co) in ((2, 2, 5, 10, 10, 0, 1e-10), (3, 2, 3, 9, 6, 7, -1.0), (2, 3, 8, 16, 13, 0, 1e-6)):
        th, it = _finish_problem(rng, d1, d2, chi, r1, r2, dtype, maxdim=md, cutoff=co, normalize=1)
        bad = int(rng.integers(0, it["cols"].shape[1]))
        it["cols"][:, bad] = np.nan
        it["bad"] = bad
        items.append(it)
    res = gate_finish(dtype, items)
    pairs = []
    for it, out in zip(items, res):
        p, fr = check_finish(it, out, dtype); pairs += p
        if "bad" in it:
            assert fr["perm"][-1] == it["bad"] and out["nk"] < it["cols"].shape[1]
            assert np.all(np.isfinite(out["S"])) and np.all(out["S"] > 0)
        else:
            assert out["nk"] == 1 and out["S"][0] == 0 and out["terr"] == 0 and not np.any(out["X1"]) and not np.any(out["X2"])
    _measured(f"gate_finish NaN column ({DT_IDS[dtype]})", _worst(pairs))


# ---- the chain: gate_theta -> LAPACK SVD -> gate_finish against the reference's simple_update core on the same R factors ----------------------------------------
@pytest.mark.parametrize("dtype", (0, 1), ids=DT_IDS)
@pytest.mark.parametrize("lowrank_on", (1, 0), ids=("lowrank", "full"))
def test_chain_theta_svd_finish(dtype, lowrank_on):
    """ties the stored layout of theta (adjoint, scale, low-rank factor) to its reader.  Rzz, maxdim = K = 2 chi: theta has rank K exactly, so the truncation at K drops
    singular values at the rounding level only.  With E = the error of the stored theta against the reference theta (its derived element-wise bound, Frobenius norm) plus
    the rounding of U Sigma and V to T (3 u_T ||theta||_F): |S_i - S_ref_i| <= ||E||_F (Weyl), and the rank-K projection moves by at most ||E||_F (1 + 2 sigma_1 / gap) with
    gap = sigma_K - sigma_K+1 (Wedin), which bounds every element of R1^+ theta_K R2^+T after the factor ||R1^+||_2 ||R2^+||_2"""
    rng = np.random.default_rng(111 + 2 * dtype + lowrank_on)
    E = lambda n, **k: eigen_site(rng, n, spectrum(n, 1e-1, noise=1e-18, **k))
    items = []
    for chi in (8, 17):
        n = 2 * chi
        items.append(gate_item(2, 2, chi, E(n), chol_site(rng, n, spectrum(n, 1e-1)), gate_of("Rzz", 2, 2, rng), dtype, maxdim=2 * chi))      # square
        items.append(gate_item(2, 2, chi, E(n, rank=n - 3), E(n), gate_of("Rzz", 2, 2, rng), dtype, maxdim=2 * chi))                          # wide
        items.append(gate_item(2, 2, chi, E(n), E(n, rank=n - 3), gate_of("Rzz", 2, 2, rng), dtype, maxdim=2 * chi))                          # strictly tall: ld = 4 chi > ncol = 4 chi - 6
    assert_rank_decisions_clear(items)
    res = gate_theta(dtype, items, lowrank_on, 3)
    ct = ref.CT[dtype]; uT = ref.UT[dtype]
    fitems, refs = [], []; shapes = set()
    for it, r in zip(items, res):
        (lam1, idx1, R1, Rp1), (lam2, idx2, R2, Rp2) = site_views(it, r)
        Mr, Nc, wide = theta_geometry(it, r)
        K = int(r["info"][7])
        assert (K > 0) == (lowrank_on == 1 and not wide) and (K == 0 or K == 2 * it["chi"])
        shapes.add((Mr > Nc) - (Mr < Nc))
        ld, ncol = max(Mr, Nc), min(Mr, Nc)
        th0 = ref.unflat(r["theta0"][:Mr * Nc], ld, ncol).astype(np.complex128)
        M = ref.unflat(r["theta"][:ld * (K or ncol)], ld, K or ncol).astype(np.complex128)
        U, S, Vh = np.linalg.svd(M, full_matrices=False)
        if K:                                             # V recovered from the unrotated copy: V = theta0^dagger U Sigma^-1
            V = np.full((ncol, ncol), np.nan + 0j); V[:, :K] = th0.conj().T @ (U / S)
            cols = np.full((ld, ncol), np.nan + 0j); cols[:, :K] = U * S
        else:
            V = Vh.conj().T; cols = U * S
        perm = np.concatenate([rng.permutation(K or ncol), np.arange(K or ncol, ncol)])
        n1, n2 = it["s"][0]["n"], it["s"][1]["n"]
        fi = finish_item(2, 2, it["chi"], None, lam1, idx1, it["s"][0]["F"][2], lam2, idx2, it["s"][1]["F"][2], dtype, maxdim=it["maxdim"], cutoff=1e-12, normalize=0,
                         chi_cap=min(n1 * 2, n2 * 2, it["maxdim"]), texp=r["texp"], K=K, raw=(cols[:, perm], V[:, perm]))
        fitems.append(fi)
        th, ab = ref.theta(R1, R2, it["gate"], 2, 2, it["chi"])
        refs.append((th, ab, Rp1, Rp2))
    assert shapes == {-1, 0, 1}                           # wide, square and strictly tall stored thetas
    outs = gate_finish(dtype, fitems)
    pairs = []
    for it, fi, out, (th, ab, Rp1, Rp2) in zip(items, fitems, outs, refs):
        sv = np.linalg.svd(th, compute_uv=False)
        Kc = 2 * it["chi"]
        n, terr, steps = ref.truncate(sv, it["maxdim"], 1e-12, ref.RT[dtype])
        assert n == Kc and (len(sv) == Kc or sv[Kc - 1] > 1e6 * sv[Kc])
        assert out["nk"] == n and out["status"] == 0
        nE = np.linalg.norm(ref.prod_bound(ab, 4 * it["chi"], th, uT)) + 3 * uT * np.linalg.norm(th) + 64 * len(sv) * ref.U64 * np.linalg.norm(th)
        pairs.append((np.abs(out["S"] - sv[:n]), np.full(n, nE + 2 * uT * sv[0])))
        # truncerr: the dropped weight is at the rounding level of the stored theta: both are below (||E||_F / ||theta||_F)^2 * nsv + the f32/f64 floor
        assert abs(out["terr"] - terr) <= len(sv) * (nE / np.linalg.norm(th)) ** 2 + 1e-30
        gap = sv[n - 1] - (sv[n] if len(sv) > n else 0.0)
        Pt, _ = ref.truncated_theta_product(th, n, Rp1, Rp2, 2, 2)
        Pd = ref.pair_product(out["X1"], out["X2"], 2, 2, n)
        bnd = np.linalg.norm(Rp1, 2) * np.linalg.norm(Rp2, 2) * nE * (1 + 2 * sv[0] / gap) * 2 + uT * 4 * np.max(np.abs(Pt))
        pairs.append((np.abs(Pd - Pt), np.full(Pt.shape, bnd)))
    _measured(f"chain ({DT_IDS[dtype]}, {'low-rank' if lowrank_on else 'full'})", _worst(pairs))


# ---- tnqs_dbg_qr2 -----------------------------------------------------------------------------------------------------------------------------------------------
def qr2(stage, ns, GW, GV, lam, idx, r, A2=None, V2=None, tau=None, rc_want=0):
    k = len(ns)
    sq = [n * n for n in ns]
    X1, GVo, GWo = Guarded(sq, np.complex128), Guarded(sq if stage else [0] * k, np.complex128), Guarded(sq if stage else [0] * k, np.complex128)
    rk = np.full(k, -9, dtype=np.int32)
    pad = lambda v, n, dt: np.concatenate([np.asarray(v, dtype=dt), np.zeros(n - len(v), dtype=dt)])
    lamc = _cat([pad(l, n, np.float64) for l, n in zip(lam, ns)], np.float64); idxc = _cat([pad(i, n, np.int32) for i, n in zip(idx, ns)], np.int32)
    a = [_cat(m, np.complex128) if m is not None else None for m in (GW, GV, A2, V2)]
    rc = lib.tnqs_dbg_qr2(stage, k, _p(_ints(ns)), _p(a[0]), _p(a[1]), _p(lamc), _p(idxc), _p(_ints(r)), _p(a[2]), _p(a[3]), _p(_dbl(tau)) if tau is not None else None,
                          _p(X1.a), _p(GVo.a) if stage else None, _p(GWo.a) if stage else None, _p(rk) if stage else None, GUARD)
    assert rc == rc_want, (rc, lib.tnqs_last_error())
    X1.check(rc == 0); GVo.check(rc == 0); GWo.check(rc == 0)
    if rc:
        return None
    um = lambda g: [ref.unflat(g.item(i), n, n) for i, n in enumerate(ns)]
    return um(X1), (um(GVo) if stage else None), (um(GWo) if stage else None), rk


def test_qr2_second_pass():
    """sites whose spectrum spans 1e-6 in sigma (1e-12 in the Gram eigenvalues): the first pass leaves R1 with errors ~1e-4 relative on the small directions; X1 = R1^+;
    with the eigen pair of G2 = Q1^dagger Q1 the composition GVout^dagger is an R of psi~ (R^dagger R = G), GWout its pseudo-inverse; rk.  First passes as the engine
    hands them over: eigen sites of the shifted pass (r = n; one with an exactly dependent column, which the second pass drops), eigen sites under the ordinary threshold
    with three null directions (r = n - 3 < n, idx a scattered subset: X1's columns >= r must be zero, the composition runs over a < r1 only -- the rows >= r1 of V2 are
    poisoned) and Cholesky sites (GV = L, GW = L^-dagger, lambda = 1, idx the identity)"""
    rng = np.random.default_rng(121)
    ns = [6, 10, 34, 16, 64, 10, 34, 17]
    kind = ["shift", "shift", "shift", "shift", "shift", "subset", "subset", "chol"]
    drop = [0, 0, 0, 1, 0, 0, 0, 0]                       # item 3: one direction of psi~ is null -> the second pass drops it
    Psis, firsts = [], []
    for n, dr, kd in zip(ns, drop, kind):
        N = n + 5
        if kd == "subset":                                # factors built directly: V unitary, eigenvalues over 1e-10 and three nulls at the rounding level, scattered
            lam_all = np.concatenate([1e-10 ** np.linspace(0, 1, n - 3), [1e-18, -1e-18, 0.0]])[rng.permutation(n)]
            V = unitary(rng, n)
            Psi = (unitary(rng, N)[:, :n] * np.sqrt(np.maximum(lam_all, 0.0) * (lam_all > 1e-15))) @ V.conj().T
            GA, GV, GW = V * lam_all, V, V.copy()
            tau1 = 4.0 * n * EPS
            assert ref.decision_margin(ref.rayleigh(GA, GV)[0], tau1) >= 100
        else:
            s = 1e-6 ** np.linspace(0, 1, n)
            if dr:
                s[-1] = 0.0
            Psi = (unitary(rng, N)[:, :n] * s) @ unitary(rng, n).conj().T
            GA, GV, GW = ref.chol_factors(Psi) if kd == "chol" else ref.eigen_factors(Psi)
            tau1 = -4.0 * n * EPS
        lam, idx, R1, Rp1 = ref.site_R(1 if kd == "chol" else 0, GA, GV, GW, tau=tau1)
        assert len(idx) == (n - 3 if kd == "subset" else n) and (kd != "subset" or not np.array_equal(idx, np.arange(len(idx))))
        Psis.append(Psi); firsts.append((GW, GV, lam, idx, len(idx), R1, Rp1))
    X1, _, _, _ = qr2(0, ns, [f[0] for f in firsts], None, [f[2] for f in firsts], [f[3] for f in firsts], [f[4] for f in firsts])
    pairs = []; A2s, V2s, taus = [], [], []
    for n, Psi, f, x in zip(ns, Psis, firsts, X1):
        GW, GV, lam, idx, r, R1, Rp1 = f
        want = np.zeros((n, n), dtype=complex); want[:, :r] = Rp1
        assert np.all(x[:, r:] == 0), "columns >= r of X1 are not zero"
        pairs.append((ref.err(x, want), 4 * ref.U64 * np.abs(want)))           # one division by a square root per element
        Q1 = Psi @ x                                       # formed in numpy from the returned X1, with its Gram matrix and LAPACK's eigen pair
        G2 = Q1.conj().T @ Q1; G2 = (G2 + G2.conj().T) / 2
        _, V2 = np.linalg.eigh(G2)
        A2 = G2 @ V2
        if r < n:                                          # Q1's columns >= r are zero, so G2 and A2 vanish there exactly: what stands in V2's rows >= r1 must not matter
            assert not np.any(A2[r:]) and np.all(V2[r:][:, np.abs(ref.rayleigh(A2, V2)[0]) > 0.5] == 0)
            V2 = V2.copy(); V2[r:] = 7.0 - 3.0j
        A2s.append(A2); V2s.append(V2); taus.append(4.0 * n * EPS)
        l2, _ = ref.rayleigh(A2, V2)
        assert ref.decision_margin(l2, taus[-1]) >= 100
    X1b, GVo, GWo, rk = qr2(1, ns, [f[0] for f in firsts], [f[1] for f in firsts], [f[2] for f in firsts], [f[3] for f in firsts], [f[4] for f in firsts], A2s, V2s, taus)
    for i, (n, Psi, f) in enumerate(zip(ns, Psis, firsts)):
        GW, GV, lam, idx, r, R1, Rp1 = f
        assert np.array_equal(X1b[i], X1[i])
        GVr, GWr, rkr, lam2 = ref.qr2_compose(R1, Rp1, A2s[i], V2s[i], taus[i])
        assert rk[i] == rkr == r - drop[i]
        assert np.all(GVo[i][:, rkr:] == 0) and np.all(GWo[i][:, rkr:] == 0)
        l2, sel = ref.kept(lam2, taus[i])
        W2 = V2s[i][:r][:, sel]
        # each column: an inner product of length r1 times sqrt(l2) (or divided by it), all in f64; the Rayleigh quotient's own bound (2 n + 16) u enters through sqrt(l2)
        sc = (2 * r + 16 + 2 * n + 16) * 2 * ref.U64
        pairs.append((ref.err(GVo[i][:, :rkr], GVr), sc * (np.abs(R1).T @ np.abs(W2)) * np.sqrt(l2)[None, :]))
        pairs.append((ref.err(GWo[i][:, :rkr], GWr), sc * (np.abs(Rp1) @ np.abs(W2)) / np.sqrt(l2)[None, :]))
        # GVout^dagger is a valid R of psi~: R^dagger R = G.  R = R2 R1 with R2^dagger R2 = G2 restricted to the kept directions and R1^dagger G2 R1 = G on the range
        # of R1: the defect of the REFERENCE composition is the problem's own error; the device's R is within the element-wise bounds above of it
        R = GVo[i][:, :rkr].conj().T; Rr = GVr.conj().T
        G = Psi.conj().T @ Psi
        eR = sc * ((np.abs(R1).T @ np.abs(W2)) * np.sqrt(l2)[None, :]).T
        bG = eR.T @ np.abs(Rr) + np.abs(Rr).T @ eR + eR.T @ eR
        pairs.append((np.abs(R.conj().T @ R - G), bG + np.abs(Rr.conj().T @ Rr - G)))
        assert np.max(np.abs(Rr.conj().T @ Rr - G)) <= 1e-9 * np.max(np.abs(G))                # the second pass did its job: R^dagger R = G far below the first pass's 1e-4
        # GWout is its pseudo-inverse: R GWout = I on the kept directions
        eW = sc * (np.abs(Rp1) @ np.abs(W2)) / np.sqrt(l2)[None, :]
        bI = eR @ np.abs(GWr) + np.abs(Rr) @ eW + eR @ eW
        pairs.append((np.abs(R @ GWo[i][:, :rkr] - np.eye(rkr)), bI + np.abs(Rr @ GWr - np.eye(rkr))))
    _measured("qr2", _worst(pairs))
    qr2(0, [257], [np.zeros((1, 1))], None, [np.ones(1)], [np.zeros(1)], [1], rc_want=ERR_UNSUPPORTED)


# ---- tnqs_dbg_small_svd -----------------------------------------------------------------------------------------------------------------------------------------
def small_svd(dtype, shapes, psis, rc_want=0):
    ns = [d * cb for d, lo, cb, hi in shapes]
    GA, GV = Guarded([n * n for n in ns], np.complex128), Guarded([n * n for n in ns], np.complex128)
    src = _cat(psis, ref.CT[dtype])
    rc = lib.tnqs_dbg_small_svd(dtype, len(shapes), _p(_ints(shapes)), _p(src), _p(GA.a), _p(GV.a), GUARD)
    assert rc == rc_want, (rc, lib.tnqs_last_error())
    GA.check(rc == 0); GV.check(rc == 0)
    if rc:
        return None
    return [ref.unflat(GA.item(i), n, n) for i, n in enumerate(ns)], [ref.unflat(GV.item(i), n, n) for i, n in enumerate(ns)]


@pytest.mark.parametrize("dtype", (0, 1), ids=DT_IDS)
def test_small_svd_sites(dtype):
    """tensors [d][low][chi_b][hi] with N = low hi < n = d chi_b, among them N = 1, N = n - 1 and d = 3 with the bond leg neither first nor last.
    Bounds.  The f64 Jacobi stops when every pair of columns has |<a_p, a_q>| <= tol |a_p| |a_q|, tol = 2^-52 sqrt(max(n, 4)) (kernels_svd.hip), so the v_j are orthonormal
    to tol plus the rounding e_n = 4 (2 n + 16) 2^-53 of an n-term inner product (the kernel's and this test's).  (M J)^dagger (M J) = diag(sigma^2) + E with
    |E_ij| <= tol sigma_i sigma_j, and at most 60 sweeps (the launch's limit) of rotations, ~8 roundings per element each, were applied to M: the eigenvalues
    l_j = Re(v_j^dagger a_j) are within b = (N tol + 480 N 2^-53) sigma_1^2 of LAPACK's sigma_j^2 (Weyl), and M M^dagger = V diag(l) V^dagger to b per element"""
    rng = np.random.default_rng(131)
    shapes = [(2, 1, 3, 1), (2, 1, 4, 7), (3, 2, 5, 3), (2, 3, 8, 4), (3, 1, 2, 5), (2, 5, 17, 3), (2, 2, 32, 8)]
    assert [lo * hi for d, lo, cb, hi in shapes][:2] == [1, 7] and all(lo * hi < d * cb for d, lo, cb, hi in shapes)
    psis = [((rng.standard_normal((d, lo, cb, hi)) + 1j * rng.standard_normal((d, lo, cb, hi))) / np.sqrt(d * lo * cb * hi)).astype(ref.CT[dtype]) for d, lo, cb, hi in shapes]
    GA, GV = small_svd(dtype, shapes, [p.ravel(order="F") for p in psis])
    sites = []; pairs = []
    for (d, lo, cb, hi), psi, A, V in zip(shapes, psis, GA, GV):
        n, N = d * cb, lo * hi
        assert np.all(A[:, N:] == 0) and np.all(V[:, N:] == 0), "columns >= N are not exactly zero"
        # M[(s, b), (lo, hi)] = conj(psi[s, lo, b, hi])
        M = psi.astype(np.complex128).transpose(0, 2, 1, 3)                       # [s, b, lo, hi]; rows s + d b, columns lo + low hi
        M = M.reshape(d, cb, lo * hi, order="F").reshape(d * cb, lo * hi, order="F").conj()
        sv = np.linalg.svd(M, compute_uv=False)
        l = np.sum(V[:, :N].conj() * A[:, :N], axis=0).real
        tol = 2.0 ** -52 * np.sqrt(max(n, 4)); en = 4 * (2 * n + 16) * ref.U64
        b = (N * tol + 480 * N * ref.U64) * sv[0] ** 2
        Vn = V[:, :N]
        pairs.append((np.abs(np.sort(l)[::-1] - sv ** 2), b))
        pairs.append((np.abs(Vn.conj().T @ Vn - np.eye(N)), tol + en))
        pairs.append((np.abs(A[:, :N] - Vn * l[None, :]), en * sv[0] ** 2))                      # a_j = sigma_j^2 v_j
        pairs.append((np.abs((Vn * l) @ Vn.conj().T - M @ M.conj().T), b + en * sv[0] ** 2))      # G = M M^dagger = V diag(l) V^dagger: the eigen factorisation gate_eigs reads
        sites.append(dict(mode=0, F=(A, V, V.copy()), n=n, rk=0, N=N, d=d, chi=cb))
    _measured(f"small_svd ({DT_IDS[dtype]})", _worst(pairs))
    # fed to gate_theta as a mode-0 site: the rank is N
    items = []
    for s in sites:
        d, chi = s["d"], s["chi"]
        items.append(gate_item(d, 2, chi, s, eigen_site(rng, 2 * chi, spectrum(2 * chi, 1e-2)), gate_of("random", d, 2, rng), dtype))
    assert_rank_decisions_clear(items)
    res = gate_theta(dtype, items, 0, 0)
    for s, it, r in zip(sites, items, res):
        assert int(r["info"][0]) == s["N"] and int(r["info"][1]) == 2 * s["chi"]
        check_rank_decision(it, r, dtype)
    small_svd(dtype, [(2, 2, 3, 3)], [np.zeros(36)], rc_want=ERR_UNSUPPORTED)          # N = n: not a small site
