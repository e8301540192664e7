"""CPU-side checks of the bond entanglement spectrum (bond_spectra / bond_entropies / renyi_entropy; reference src/entanglement.jl): the numpy restatement
tests/bond_spectra_ref.py against the oracle's GHZ pin, against exact Schmidt spectra on a tree, against the singular values the symmetric gauge leaves on the bonds,
in both orientations, and its two routes (eigh / SVD) against each other on the inputs of the kernel test -- the worst deviation there is the recorded baseline of
the device bound (tests/test_gpu_bond_spectra.py).  Then the host-only matrix method of renyi_entropy, which needs no GPU."""
import math

import numpy as np
import pytest

import tnqs_oracle as o
import statevector as sv
import bond_spectra_ref as br

EPS64 = br.EPS64
# max |eigh route - SVD route| over every entry of every spectrum of bond_spectra_ref.kernel_inputs, complex128 and (rounded) complex64 inputs, as MEASURED with this file
# (printed by the test below): the recorded baseline.  The device bound on an entry of a normalised spectrum is max(200 eps chi, 10 x this).  Both routes see the SAME m1,
# its positive semi-definite part (bond_spectra_ref.psd_part): the SVD route is defined for nothing else, and on the raw rank-deficient complex64 inputs the difference
# of the routes (1.3e-8, printed too) is the clipped rounding noise of the stored m1, not a property of either route -- a baseline taken there would let a device error of
# 1e-8 pass at every chi.
SPECTRUM_BASELINE = 1.0e-15
ROUTE_TOLERANCE = 10 * SPECTRUM_BASELINE        # what this file asserts of the two routes: the device bound itself
TREE_TOL = {np.dtype(np.complex128): 200 * EPS64 * 3, np.dtype(np.complex64): 1e-5}


def _ghz(g, dt=np.complex128):
    tensors = {}
    for v in g.vertices:
        t = np.zeros((2,) + (2,) * g.degree(v), dtype=dt)
        t[(0,) * t.ndim] = 1
        t[(1,) * t.ndim] = 1
        tensors[v] = t
    return o.TensorNetworkState(g, tensors)


def _spectrum(bpc, e, route=br.bond_spectrum):
    return route(bpc.message(e), bpc.message((e[1], e[0])), br.cutoff_of(bpc.tns.dtype))


def schmidt_spectrum(vec, g, u, v, chi):
    """sigma^2 / sum sigma^2 of the state vector across the tree bond (u, v), padded with zeros to chi entries"""
    side, todo = {u}, [u]
    while todo:
        a = todo.pop()
        for b in g.nbrs[a]:
            if b not in side and not (a == u and b == v):
                side.add(b); todo.append(b)
    assert v not in side
    ax = [g.pos[a] for a in g.vertices if a in side]
    m = np.moveaxis(vec, ax, list(range(len(ax)))).reshape(2 ** len(ax), -1)
    s2 = np.linalg.svd(m, compute_uv=False) ** 2
    s2 = np.sort(s2)[::-1][:chi] / np.sum(s2)
    return np.concatenate([s2, np.zeros(chi - len(s2))])


def test_ghz_bond_entropy_is_log2_and_matches_the_oracle():
    g = o.named_grid((3, 3))
    bpc = o.update(o.BeliefPropagationCache(_ghz(g)), maxiter=300, tolerance=1e-14)
    thr = br.cutoff_of(np.complex128)
    for e in g.edges:
        lam = _spectrum(bpc, e)
        assert abs(br.renyi(lam, 1, thr) - o.bond_entropy(bpc, e)) < 1e-12
        assert abs(br.renyi(lam, 1, thr) - math.log(2)) < 1e-9 and abs(br.renyi(lam, 2, thr) - math.log(2)) < 1e-9


@pytest.mark.parametrize("dt", [np.complex128, np.complex64])
def test_exact_schmidt_spectrum_on_the_comb_tree(dt):
    g = o.comb_tree((3, 3))
    psi = o.random_state(dt, g, 3, seed=7)
    bpc = o.update(o.BeliefPropagationCache(psi))
    vec = sv.tns_to_statevector(o.TensorNetworkState(g, {v: psi.tensors[v].astype(np.complex128) for v in g.vertices}))
    worst = 0.0
    for (a, b) in g.edges:
        exact = schmidt_spectrum(vec, g, a, b, 3)
        for e in ((a, b), (b, a)):
            lam = _spectrum(bpc, e)
            assert lam.shape == (3,) and abs(lam.sum() - 1) < 1e-12 and np.all(np.diff(lam) <= 0)
            worst = max(worst, float(np.max(np.abs(lam - exact))))
    print(f"MEASURED comb33 chi3 {np.dtype(dt).name}: max |bond spectrum - Schmidt spectrum| = {worst:.3e} (bound {TREE_TOL[np.dtype(dt)]:.1e})")
    assert worst <= TREE_TOL[np.dtype(dt)]


def test_the_two_orientations_have_the_same_spectrum():
    g = o.named_grid((3, 3))
    bpc = o.update(o.BeliefPropagationCache(o.random_state(np.complex128, g, 3, seed=7)), maxiter=300, tolerance=1e-14)
    worst = max(float(np.max(np.abs(_spectrum(bpc, (a, b)) - _spectrum(bpc, (b, a))))) for (a, b) in g.edges)
    print(f"MEASURED grid3x3 chi3: max |spectrum(u, v) - spectrum(v, u)| = {worst:.3e}")
    assert worst <= 200 * EPS64 * 3


def test_spectrum_is_the_squared_gauge_singular_values():
    """after symmetric_gauge both messages of a bond are diag(S); the spectrum taken BEFORE the gauge is S^2 / sum S^2"""
    g = o.named_grid((3, 3))
    bpc = o.update(o.BeliefPropagationCache(o.random_state(np.complex128, g, 3, seed=7)), maxiter=300, tolerance=1e-14)
    gauged = o.symmetric_gauge(bpc)
    worst = 0.0
    for e in g.edges:
        s = np.sort(np.real(np.diag(gauged.message(e))))[::-1]
        worst = max(worst, float(np.max(np.abs(_spectrum(bpc, e) - s * s / np.sum(s * s)))))
    print(f"MEASURED grid3x3 chi3 complex128: max |spectrum - S^2 / sum S^2| = {worst:.3e}")
    assert worst <= 1e-10


def test_the_two_routes_agree_on_the_kernel_inputs():
    worst, raw, per = 0.0, 0.0, {}
    for dt in (np.complex128, np.complex64):
        cutoff = br.cutoff_of(dt)
        for (n, kind, m1, m2, p1, p2) in br.kernel_inputs(dt):
            a, b = br.effective(m1, p1), br.effective(m2, p2)
            # the absolute cutoff must not decide by rounding: every eigenvalue of m2 is far above it or far below it (the computed zeros carry the
            # eigen solver's own noise, a few eps ||m||, hence a tenth of the cutoff here where exact arithmetic has a hundredth)
            w = np.linalg.eigvalsh((b + b.conj().T) / 2)
            assert np.all((w >= 100 * cutoff) | (np.abs(w) <= cutoff / 10)), (np.dtype(dt).name, n, kind, w)
            if kind == "rankhalf":
                assert np.sum(w >= 100 * cutoff) == n // 2 and np.linalg.norm(b, 2) <= br.LOW_RANK_NORM * (1 + 1e-6)
            if kind == "full":
                assert w.min() >= 0.049 * w.max()
            ap = br.psd_part(a)
            e1, e2 = br.bond_spectrum(ap, b, cutoff), br.bond_spectrum_svd(ap, b, cutoff)
            assert e1.shape == (n,) and abs(e1.sum() - 1) <= 4 * n * EPS64
            d = float(np.max(np.abs(e1 - e2)))
            raw = max(raw, float(np.max(np.abs(br.bond_spectrum(a, b, cutoff) - e2))))
            per[(np.dtype(dt).name, kind)] = max(per.get((np.dtype(dt).name, kind), 0.0), d)
            worst = max(worst, d)
    for k, v in sorted(per.items()):
        print(f"MEASURED routes {k[0]} {k[1]}: max |eigh route - SVD route| = {v:.3e}")
    print(f"MEASURED kernel inputs: max |eigh route - SVD route| = {worst:.3e} (recorded baseline {SPECTRUM_BASELINE:.1e}); with the stored m1 in the eigh route: {raw:.3e}")
    assert worst <= ROUTE_TOLERANCE


def test_a_negative_message_eigenvalue_is_a_domain_error():
    m1, m2 = br.negative_item(np.complex128)
    with pytest.raises(br.DomainError):
        br.bond_spectrum(m1, m2, br.cutoff_of(np.complex128))


# ---- the host-only matrix method of the package (entanglement.jl:21-29) ----------------------------------------------------------------------------------
ALPHAS = (0.5, 1, 2, 3)


def _closed_form(p, alpha):
    p = np.asarray(p, dtype=np.float64)
    return float(-np.sum(p * np.log(p))) if alpha == 1 else float(np.log(np.sum(p ** alpha)) / (1 - alpha))


@pytest.mark.parametrize("alpha", ALPHAS)
def test_matrix_method_known_answers(alpha):
    import tnqs_amd as tn
    p = np.array([0.5, 0.3, 0.15, 0.05])
    rng = np.random.default_rng(1)
    q, _ = np.linalg.qr(rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4)))
    for rho in (np.diag(p).astype(np.complex128), (q * p) @ q.conj().T):
        assert abs(tn.renyi_entropy(rho, alpha) - _closed_form(p, alpha)) < 1e-12
        assert abs(tn.renyi_entropy(rho, alpha) - br.renyi_of_matrix(rho, alpha)) < 1e-12
    for d in (1, 2, 5):
        assert abs(tn.renyi_entropy(np.eye(d) / d, alpha) - math.log(d)) < 1e-12           # maximally mixed
        assert abs(tn.renyi_entropy(np.eye(d) * 7.0, alpha) - math.log(d)) < 1e-12         # normalised by its trace first
    v = q[:, 0]
    assert abs(tn.renyi_entropy(np.outer(v, v.conj()), alpha)) < 1e-12                     # a pure state: the zero eigenvalues are dropped
    # normalize = False on an un-normalised matrix: the formula on c p
    c = 0.5
    want = float(-np.sum(c * p * np.log(c * p))) if alpha == 1 else float(np.log(np.sum((c * p) ** alpha)) / (1 - alpha))
    assert abs(tn.renyi_entropy(c * np.diag(p), alpha, normalize=False) - want) < 1e-12
    assert abs(tn.renyi_entropy(c * np.diag(p), alpha, normalize=False) - tn.renyi_entropy(c * np.diag(p), alpha)) > 1e-3
    # float32 matrices: the filter is 10 eps of float32
    rho32 = np.diag([0.75, 0.25, 5e-7, 0.0]).astype(np.float32)
    assert abs(tn.renyi_entropy(rho32, alpha, normalize=False) - _closed_form([0.75, 0.25], alpha)) < 1e-6


def test_matrix_method_wrappers_and_errors():
    import tnqs_amd as tn
    rho = np.diag([0.6, 0.4])
    assert tn.von_neumann_entanglement_entropy(rho) == tn.renyi_entropy(rho, 1)
    assert tn.second_renyi_entanglement_entropy(rho) == tn.renyi_entropy(rho, alpha=2)
    assert abs(tn.renyi_entropy(rho, 0) - math.log(2)) < 1e-12                              # alpha = 0: log of the rank
    for bad in (-1, -0.5, 1j, None, "1"):
        with pytest.raises(tn.TnqsArgumentError):
            tn.renyi_entropy(rho, bad)
    with pytest.raises(tn.TnqsArgumentError):
        tn.renyi_entropy(np.zeros((2, 3)), 1)
    # a kept negative eigenvalue: DomainError where the formula takes its logarithm or a non-integer power, a plain number for an integer power
    neg = np.diag([1.2, -0.2])
    for alpha in (1, 0.5):
        with pytest.raises(tn.TnqsDomainError):
            tn.renyi_entropy(neg, alpha)
    assert abs(tn.renyi_entropy(neg, 2) - (-math.log(1.2 ** 2 + 0.2 ** 2))) < 1e-12


def test_the_package_exports_the_feature():
    import tnqs_amd as tn
    assert "tnqs_bond_spectra" in tn.EXPORTS
    for name in ("bond_spectra", "bond_entropies", "renyi_entropy", "von_neumann_entanglement_entropy", "second_renyi_entanglement_entropy"):
        assert callable(getattr(tn, name))
    # argument errors are raised before any device work
    bpc = object.__new__(tn.BeliefPropagationCache); bpc.graph = tn.named_grid((3, 3)); bpc._h = None
    with pytest.raises(tn.TnqsArgumentError, match="not an edge"):
        tn.bond_spectra(bpc, [((1, 1), (2, 2))])
    with pytest.raises(tn.TnqsArgumentError, match="not an edge"):
        tn.bond_entropies(bpc, 1, [((1, 1), (9, 9))])
    with pytest.raises(tn.TnqsArgumentError, match="not an edge"):
        tn.renyi_entropy(bpc, ((1, 1), (3, 3)), 1)
    with pytest.raises(tn.TnqsArgumentError, match="single vertices and pairs"):
        tn.renyi_entropy(bpc, [(1, 1), (1, 2), (1, 3)], 1)
    with pytest.raises(tn.TnqsArgumentError, match="single vertices and pairs"):
        tn.renyi_entropy(bpc, [(9, 9)], 1)
    with pytest.raises(tn.TnqsError, match="algorithm choice not supported"):
        tn.renyi_entropy(bpc, ((1, 1), (1, 2)), 1, alg="exact")
    with pytest.raises(tn.TnqsArgumentError, match="real and >= 0"):
        tn.renyi_entropy(bpc, ((1, 1), (1, 2)), -1)
    assert tn.bond_spectra(bpc, []) == {} and tn.bond_entropies(bpc, 2, []).shape == (0,)
