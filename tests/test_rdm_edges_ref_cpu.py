"""CPU-side checks of the two-site reduced density matrix of a bond (rdm_edges / expect_edges; reference src/rdm.jl:52-73 for adjacent vertices):
the numpy restatement tests/rdm_edges_ref.py against the oracle's region contraction (every Pauli pair on every bond of a loopy grid), against exact
state vectors on a tree, and with a neighbour of site dimension 1.  The worst deviation found here is the measured baseline of the device's complex128
bound (tests/test_gpu_rdm_edges.py)."""
import numpy as np
import pytest

import tnqs_oracle as o
import statevector as sv
import rdm_edges_ref as er

# max |<P_u P_v> from rdm_edge - oracle.expect_region| over the nine Pauli pairs and the twelve bonds of the 3 x 3 grid at chi = 3 as MEASURED with this file
# (complex128, printed by the test below): the recorded baseline.  The device's complex128 bound is max(200 eps, 10 x this).
REGION_BASELINE = 1.4e-16
# what this file itself asserts (not the baseline: summation order differs between BLAS builds)
REGION_TOLERANCE = 1e-14
TREE_TOLERANCE = 1e-12          # tests/test_oracle_pins.py test_multi_site_expect_bp_exact_on_trees

PAULI = {"X": np.array([[0, 1], [1, 0]], dtype=complex), "Y": np.array([[0, -1j], [1j, 0]]), "Z": np.diag([1.0, -1.0]).astype(complex)}


def _messages(bpc):
    return {e: bpc.message(e) for (a, b) in bpc.g.edges for e in ((a, b), (b, a))}


def test_every_pauli_pair_on_every_bond_of_the_grid_matches_the_region_contraction():
    g = o.named_grid((3, 3))
    psi = o.random_state(np.complex128, g, 3, seed=7)
    bpc = o.update(o.BeliefPropagationCache(psi), maxiter=300)
    ms = _messages(bpc)
    worst = 0.0
    for (a, b) in g.edges:
        rho = er.rdm_edge(psi.tensors, ms, g.nbrs, a, b)
        assert rho.shape == (4, 4)
        n = rho / np.trace(rho)
        assert np.max(np.abs(n - n.conj().T)) < 1e-8            # Hermitian at the fixed point (up to the BP tolerance)
        for pa in "XYZ":
            for pb in "XYZ":
                val = np.trace(np.kron(PAULI[pa], PAULI[pb]) @ n)
                worst = max(worst, abs(val - o.expect_region(bpc, {a: PAULI[pa], b: PAULI[pb]}, [a, b])))
        # the other orientation is the index swap
        swapped = er.rdm_edge(psi.tensors, ms, g.nbrs, b, a).reshape(2, 2, 2, 2).transpose(1, 0, 3, 2).reshape(4, 4)
        assert np.max(np.abs(swapped - rho)) <= 1e-14 * np.max(np.abs(rho))
    print(f"MEASURED grid3x3 chi3: max |edge rdm - expect_region| = {worst:.3e} (recorded baseline {REGION_BASELINE:.1e})")
    assert worst <= REGION_TOLERANCE


def test_exact_on_the_comb_tree():
    g = o.comb_tree((3, 3))
    psi = o.random_state(np.complex128, g, 3, seed=7)
    bpc = o.update(o.BeliefPropagationCache(psi))
    ms = _messages(bpc)
    vec = sv.tns_to_statevector(psi)
    worst = 0.0
    for (a, b) in g.edges:
        for pa in "XYZ":
            for pb in "XZ":
                val = er.expect_edge(psi.tensors, ms, g.nbrs, a, b, PAULI[pa], PAULI[pb])
                worst = max(worst, abs(val - sv.expect_statevector_multi(vec, g, {a: PAULI[pa], b: PAULI[pb]})))
    print(f"MEASURED comb33 chi3: max |edge rdm - state vector| = {worst:.3e}")
    assert worst < TREE_TOLERANCE


def test_a_neighbour_of_site_dimension_one():
    """a projected vertex (site dimension 1, bonds and messages kept): the matrices are (1 * 2) x (1 * 2) in either orientation"""
    g = o.named_grid((3, 3))
    psi = o.random_state(np.complex128, g, 3, seed=9)
    c = (2, 2)
    tensors = dict(psi.tensors); tensors[c] = psi.tensors[c][1:2]
    bpc = o.update(o.BeliefPropagationCache(o.TensorNetworkState(g, tensors)), maxiter=300)
    ms = _messages(bpc)
    one = np.eye(1)
    for w in g.nbrs[c]:
        for (a, b, oa, ob) in ((c, w, one, PAULI["Z"]), (w, c, PAULI["X"], one)):
            rho = er.rdm_edge(tensors, ms, g.nbrs, a, b)
            assert rho.shape == (2, 2)
            val = np.trace(np.kron(oa, ob) @ rho) / np.trace(rho)
            assert abs(val - o.expect_region(bpc, {a: oa, b: ob}, [a, b])) <= REGION_TOLERANCE


def test_the_package_exports_the_feature():
    import tnqs_amd as tn
    assert "tnqs_rdm_edges" in tn.EXPORTS and tn.PROF_CLASSES[13] == "edge_rdm"
    for name in ("rdm_edges", "expect_edges"):
        assert callable(getattr(tn, name))
    # argument errors are raised before any device work
    bpc = object.__new__(tn.BeliefPropagationCache); bpc.graph = tn.named_grid((3, 3)); bpc._h = None
    with pytest.raises(tn.TnqsArgumentError, match="only single vertices and bonds"):
        tn.rdm(bpc, [(1, 1), (3, 3)])
    with pytest.raises(tn.TnqsArgumentError, match="only single vertices and bonds"):
        tn.rdm(bpc, [(1, 1), (1, 2), (1, 3)])
    with pytest.raises(tn.TnqsArgumentError, match="only single vertices and bonds"):
        tn.rdm_edges(bpc, [((1, 1), (2, 2))])
    with pytest.raises(tn.TnqsArgumentError, match="two characters"):
        tn.expect_edges(bpc, "Z")
