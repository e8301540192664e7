"""CPU-side checks of the two-site reduced density matrices of the ends of paths (rdm_paths / rdm_pairs / expect_pairs / correlation_function; reference
src/rdm.jl:52-73 with the path as the Steiner tree): the numpy restatement tests/path_rdm_ref.py against the oracle's region contraction (every Pauli pair on every
prefix of straight, L-shaped and staircase paths of a loopy grid), against exact state vectors on a tree, with a vertex of site dimension 1 as an end and as an inner
vertex, and against the bond restatement for k = 1.  The worst deviation found here is the measured baseline of the device's complex128 bound
(tests/test_gpu_path_rdm.py).  The host-side pieces of the package (exports, argument errors, prefix merging) are checked without a device."""
import numpy as np
import pytest

import tnqs_oracle as o
import statevector as sv
import rdm_edges_ref as er
import path_rdm_ref as pr

# max |<P_u P_w> from path_rdms - oracle.expect_region| over the nine Pauli pairs, the five paths below and all their prefixes on the 3 x 4 grid at chi = 3 as MEASURED
# with this file (complex128, printed by the test below: 1.389e-16), rounded up: the recorded baseline.  The device's complex128 bound is max(200 eps, 10 x this).
PATH_BASELINE = 2e-16
# what this file itself asserts (not the baseline: summation order differs between BLAS builds)
PATH_TOLERANCE = 1e-14
TREE_TOLERANCE = 1e-12

PAULI = {"X": np.array([[0, 1], [1, 0]], dtype=complex), "Y": np.array([[0, -1j], [1j, 0]]), "Z": np.diag([1.0, -1.0]).astype(complex)}
GRID_PATHS = [[(1, 1), (1, 2), (1, 3), (1, 4)],
              [(1, 1), (2, 1), (3, 1)],
              [(2, 2), (2, 3), (3, 3)],
              [(3, 4), (2, 4), (2, 3), (2, 2), (1, 2)],
              [(1, 1), (1, 2), (2, 2), (2, 3), (3, 3), (3, 4)]]
TREE_PATHS = [[(1, 3), (1, 2), (1, 1), (2, 1), (3, 1), (3, 2), (3, 3)],
              [(2, 3), (2, 2), (2, 1), (1, 1)]]


def _messages(bpc):
    return {e: bpc.message(e) for (a, b) in bpc.g.edges for e in ((a, b), (b, a))}


def test_every_pauli_pair_on_every_prefix_matches_the_region_contraction():
    g = o.named_grid((3, 4))
    psi = o.random_state(np.complex128, g, 3, seed=7)
    bpc = o.update(o.BeliefPropagationCache(psi), maxiter=300)
    ms = _messages(bpc)
    worst = 0.0
    for path in GRID_PATHS:
        rhos = pr.path_rdms(psi.tensors, ms, g.nbrs, path)
        assert len(rhos) == len(path) - 1
        for k, rho in enumerate(rhos, start=1):
            assert rho.shape == (4, 4)
            for pa in "XYZ":
                for pb in "XYZ":
                    val = pr.expect_pair(rho, PAULI[pa], PAULI[pb])
                    worst = max(worst, abs(val - o.expect_region(bpc, {path[0]: PAULI[pa], path[k]: PAULI[pb]}, path[:k + 1])))
    print(f"MEASURED grid3x4 chi3: max |path rdm - expect_region| = {worst:.3e} (recorded baseline {PATH_BASELINE:.1e})")
    assert worst <= PATH_TOLERANCE


def test_exact_on_the_comb_tree():
    g = o.comb_tree((3, 3))
    psi = o.random_state(np.complex128, g, 3, seed=7)
    bpc = o.update(o.BeliefPropagationCache(psi))
    ms = _messages(bpc)
    vec = sv.tns_to_statevector(psi)
    worst = 0.0
    for path in TREE_PATHS:
        for k, rho in enumerate(pr.path_rdms(psi.tensors, ms, g.nbrs, path), start=1):
            for pa in "XYZ":
                for pb in "XYZ":
                    val = pr.expect_pair(rho, PAULI[pa], PAULI[pb])
                    worst = max(worst, abs(val - sv.expect_statevector_multi(vec, g, {path[0]: PAULI[pa], path[k]: PAULI[pb]})))
    print(f"MEASURED comb33 chi3: max |path rdm - state vector| = {worst:.3e}")
    assert worst < TREE_TOLERANCE


def test_a_vertex_of_site_dimension_one_as_an_end_and_as_an_inner_vertex():
    g = o.named_grid((3, 4))
    psi = o.random_state(np.complex128, g, 3, seed=9)
    c = (2, 2)
    tensors = dict(psi.tensors); tensors[c] = psi.tensors[c][1:2]
    bpc = o.update(o.BeliefPropagationCache(o.TensorNetworkState(g, tensors)), maxiter=300)
    ms = _messages(bpc)
    one = np.eye(1)
    for path in ([(2, 2), (2, 3), (2, 4)], [(2, 4), (2, 3), (2, 2)], [(2, 1), (2, 2), (2, 3), (3, 3)]):
        rhos = pr.path_rdms(tensors, ms, g.nbrs, path)
        for k, rho in enumerate(rhos, start=1):
            du, dw = tensors[path[0]].shape[0], tensors[path[k]].shape[0]
            assert rho.shape == (du * dw, du * dw)
            oa, ob = (one if du == 1 else PAULI["X"]), (one if dw == 1 else PAULI["Z"])
            assert abs(pr.expect_pair(rho, oa, ob) - o.expect_region(bpc, {path[0]: oa, path[k]: ob}, path[:k + 1])) <= PATH_TOLERANCE


def test_the_first_step_is_the_bond_matrix():
    g = o.named_grid((3, 4))
    psi = o.random_state(np.complex128, g, 3, seed=7)
    bpc = o.update(o.BeliefPropagationCache(psi), maxiter=300)
    ms = _messages(bpc)
    for path in GRID_PATHS:
        first = pr.path_rdms(psi.tensors, ms, g.nbrs, path)[0]
        assert np.array_equal(first, er.rdm_edge(psi.tensors, ms, g.nbrs, path[0], path[1]))
    assert not pr.is_induced_path(g.nbrs, [(1, 1), (1, 2), (2, 2), (2, 1)])          # a chord: (2, 1) - (1, 1)
    assert not pr.is_induced_path(g.nbrs, [(1, 1), (1, 3)]) and not pr.is_induced_path(g.nbrs, [(1, 1), (1, 2), (1, 1)])


def test_the_package_exports_the_feature():
    import tnqs_amd as tn
    assert "tnqs_rdm_paths" in tn.EXPORTS and tn.PROF_CLASSES[14] == "path_rdm" and len(tn.PROF_CLASSES) == 15
    for name in ("rdm_paths", "rdm_pairs", "expect_pairs", "correlation_function"):
        assert callable(getattr(tn, name))
    # argument errors are raised before any device work
    bpc = object.__new__(tn.BeliefPropagationCache); bpc.graph = tn.named_grid((3, 4)); bpc._h = None
    with pytest.raises(tn.TnqsArgumentError, match="chord"):
        tn.rdm_paths(bpc, [[(1, 1), (1, 2), (2, 2), (2, 1)]])
    with pytest.raises(tn.TnqsArgumentError, match="not adjacent"):
        tn.rdm_paths(bpc, [[(1, 1), (1, 2)], [(1, 1), (1, 3)]])
    with pytest.raises(tn.TnqsArgumentError, match="repeated vertex"):
        tn.rdm_paths(bpc, [[(1, 1), (1, 2), (1, 1)]])
    with pytest.raises(tn.TnqsArgumentError, match="at least two"):
        tn.correlation_function(bpc, "ZZ", [(1, 1)])
    with pytest.raises(tn.TnqsArgumentError, match="not a vertex"):
        tn.rdm_pairs(bpc, [((1, 1), (9, 9))])
    with pytest.raises(tn.TnqsArgumentError, match="two different"):
        tn.expect_pairs(bpc, "ZZ", [((1, 1), (1, 1))])
    with pytest.raises(tn.TnqsArgumentError, match="two characters"):
        tn.expect_pairs(bpc, "Z", [((1, 1), (1, 2))])
    with pytest.raises(tn.TnqsArgumentError, match="two characters"):
        tn.correlation_function(bpc, "Z", [(1, 1), (1, 2)])
    # rdm(bpc, [u, w]) for distant vertices keeps raising
    with pytest.raises(tn.TnqsArgumentError, match="only single vertices and bonds"):
        tn.rdm(bpc, [(1, 1), (1, 3)])


def test_prefix_merging_of_pair_paths():
    from tnqs_amd import core
    a, b, c, d, e = "abcde"
    paths = [[a, b], [a, b, c, d], [a, b, c], [b, c], [a, e], [a, b, c, d]]
    merged, where = core._merge_pair_paths(paths)
    assert sorted(map(tuple, merged)) == [(a, b, c, d), (a, e), (b, c)]
    for p, (j, k) in zip(paths, where):
        assert merged[j][:k + 1] == p                        # every request is a prefix of the path it rides on, ending at vertex k
    assert core._merge_pair_paths([]) == ([], [])
    # the path of a pair is the tree path of its Steiner region, from the first vertex to the second
    g = __import__("tnqs_amd").named_grid((3, 4))
    p = core._pair_path(g, (1, 1), (1, 4))
    assert p == [(1, 1), (1, 2), (1, 3), (1, 4)] and core._pair_path(g, (1, 4), (1, 1)) == p[::-1]
    q = core._pair_path(g, (1, 1), (3, 3))
    assert q[0] == (1, 1) and q[-1] == (3, 3) and len(q) == 5 and pr.is_induced_path({v: g.neighbors(v) for v in g.vertices}, q)
