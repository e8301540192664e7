"""CPU-side checks of the loop corrections (norm_sqr, alg = "loopcorrections"; reference src/MessagePassing/loopcorrection.jl): the package's
enumeration of configurations against hand counts and against the brute force of tests/loop_ref.py, and the numpy restatement's full-order sum
(max_configuration_size = |E|) against exact contraction -- every term with a leaf vanishes at the BP fixed point, so the sum over ALL leafless
configurations is the exact norm on any graph.  The deviations found here are the measured baseline of the device's end-to-end bound
(tests/test_gpu_loops.py)."""
import numpy as np
import pytest

import tnqs_oracle as o
import statevector as sv
import loop_ref as lr

# |reference full-order sum - exact| / exact as MEASURED with this file (complex128, BP to 1e-13; printed by the test below): the recorded baseline.
# The device's complex128 end-to-end bound is 10 x these (tests/test_gpu_loops.py).
FULL_ORDER_BASELINE = {"ring4_chi3": 5.6e-16, "grid2x3_chi2": 7.9e-16, "bridged_triangles_chi2": 3.1e-16}
# what this file itself asserts: the messages are a fixed point to 1e-13 and the sum is smooth in them (not the baseline: summation order differs between BLAS builds)
FULL_ORDER_TOLERANCE = 1e-12

BRIDGED = (list(range(6)), [(0, 1), (1, 2), (0, 2), (2, 3), (3, 4), (4, 5), (3, 5)])


def fixtures():
    ring = o.Graph(list(range(4)), [(0, 1), (1, 2), (2, 3), (0, 3)])
    return {"ring4_chi3": (ring, 3, 5), "grid2x3_chi2": (o.named_grid((2, 3)), 2, 6), "bridged_triangles_chi2": (o.Graph(*BRIDGED), 2, 7)}


def _sizes(configs):
    return sorted(len(c) for c in configs)


def _as_sets(configs):
    return sorted(sorted(tuple(sorted(map(repr, e))) for e in c) for c in configs)


def test_enumeration_counts_on_the_3x3_grid():
    import tnqs_amd as tn
    g = tn.named_grid((3, 3))
    # max 4: the only leafless subgraphs of <= 4 edges of a bipartite grid are its unit squares: 2 x 2 = 4 of them
    assert _sizes(tn.leafless_edge_induced_subgraphs(g, 4)) == [4] * 4
    # max 7: + the 1 x 2 rectangles (perimeter 6): 2 horizontal + 2 vertical = 4; + two squares sharing an edge with that edge kept (a theta, 4 + 4 - 1 = 7
    # edges): one per rectangle = 4.  An 8-cycle (the outer boundary), two disjoint squares (none: any two squares of a 3 x 3 grid share the centre
    # vertex) and everything else need 8 or more edges.
    assert _sizes(tn.leafless_edge_induced_subgraphs(g, 7)) == [4] * 4 + [6] * 4 + [7] * 4
    assert _sizes(tn.leafless_edge_induced_subgraphs(g, 3)) == []


def test_enumeration_counts_on_the_hexagonal_lattice():
    import tnqs_amd as tn
    g = tn.named_hexagonal_lattice_graph(2, 2)
    # 16 vertices, 19 edges: 19 - 16 + 1 = 4 independent cycles = the 4 hexagons of the 2 x 2 lattice; the shortest cycle of a honeycomb has 6 edges
    # and two hexagons together need at least 6 + 6 - 1 = 11, so max 6 gives exactly the hexagons
    assert (g.nv(), g.ne()) == (16, 19)
    assert _sizes(tn.leafless_edge_induced_subgraphs(g, 6)) == [6] * 4


def test_enumeration_counts_on_two_bridged_triangles():
    import tnqs_amd as tn
    g = tn.NamedGraph(*BRIDGED)
    # two triangles (3 edges each) joined by the bridge (2, 3).  max 6: triangle, triangle, and their disjoint union (3 + 3 = 6 edges, vertex-disjoint);
    # the bridge alone or with one triangle leaves a leaf.  connected_only drops the union.  max 7 adds the whole graph (both bridge ends have degree 3).
    assert _sizes(tn.leafless_edge_induced_subgraphs(g, 6)) == [3, 3, 6]
    assert _sizes(tn.leafless_edge_induced_subgraphs(g, 6, connected_only=True)) == [3, 3]
    assert _sizes(tn.leafless_edge_induced_subgraphs(g, 7)) == [3, 3, 6, 7]
    assert _sizes(tn.leafless_edge_induced_subgraphs(g, 7, connected_only=True)) == [3, 3, 7]


@pytest.mark.parametrize("name,max_edges", [("grid3x3", 8), ("grid2x4", 10), ("hex", 11), ("bridged", 7), ("k4", 6)])
def test_enumeration_equals_brute_force(name, max_edges):
    import tnqs_amd as tn
    g = {"grid3x3": lambda: tn.named_grid((3, 3)), "grid2x4": lambda: tn.named_grid((2, 4)), "hex": lambda: tn.named_hexagonal_lattice_graph(1, 2),
         "bridged": lambda: tn.NamedGraph(*BRIDGED), "k4": lambda: tn.NamedGraph(range(4), [(a, b) for a in range(4) for b in range(a + 1, 4)])}[name]()
    rg = lr.RefGraph(g.vertices, g.edges)
    for conn in (False, True):
        got = tn.leafless_edge_induced_subgraphs(g, max_edges, connected_only=conn)
        assert len(set(got)) == len(got)                                   # each configuration once
        assert _as_sets(got) == _as_sets(lr.configurations(rg, max_edges, connected_only=conn))
        assert got == tn.leafless_edge_induced_subgraphs(g, max_edges, connected_only=conn)      # deterministic


def test_enumeration_guard_raises_before_any_device_work(monkeypatch):
    import tnqs_amd as tn
    from tnqs_amd import graphs
    monkeypatch.setattr(graphs, "MAX_CONNECTED_CONFIGURATIONS", 10)
    with pytest.raises(tn.TnqsError, match="more than 10 connected configurations"):
        tn.leafless_edge_induced_subgraphs(tn.named_grid((5, 5)), 4)


def test_argument_errors_need_no_device():
    import tnqs_amd as tn
    psi = tn.random_tensornetworkstate(np.complex64, tn.named_grid((2, 2)), 2, seed=1)
    with pytest.raises(tn.TnqsError, match='"bp" and "loopcorrections"'):
        tn.norm_sqr(psi, alg="exact")
    with pytest.raises(tn.TnqsArgumentError, match="max_configuration_size"):
        tn.norm_sqr(psi, alg="loopcorrections")
    for name in ("leafless_edge_induced_subgraphs", "loopcorrected_partitionfunction", "norm_sqr", "norm"):
        assert callable(getattr(tn, name))
    assert "tnqs_loop_weights" in tn.EXPORTS and tn.PROF_CLASSES[12] == "loop"


@pytest.mark.parametrize("name", sorted(FULL_ORDER_BASELINE))
def test_full_order_sum_is_the_exact_norm(name):
    g, chi, seed = fixtures()[name]
    psi = o.random_state(np.complex128, g, chi, seed=seed)
    exact = float(np.sum(np.abs(sv.tns_to_statevector(psi)) ** 2))
    rg = lr.RefGraph(g.vertices, g.edges)
    z, zbp, ws = lr.loopcorrected(psi.tensors, rg, len(g.edges))
    dev = abs(z - exact) / exact
    print(f"MEASURED {name}: |full-order - exact| / exact = {dev:.3e}; Z_bp off by {abs(zbp - exact) / exact:.3e}; {len(ws)} configurations")
    assert abs(zbp - exact) / exact > 1e-6                # the corrections are what closes the gap, not a BP that happens to be exact
    assert dev <= FULL_ORDER_TOLERANCE
    if name == "bridged_triangles_chi2":                  # product rule: the disjoint union of the triangles weighs the product of their weights
        w = {tuple(sorted(c)): x for c, x in ws}
        t1, t2 = ((0, 1), (0, 2), (1, 2)), ((3, 4), (3, 5), (4, 5))
        assert abs(w[tuple(sorted(t1 + t2))] - w[t1] * w[t2]) <= 1e-14 * max(1.0, abs(w[t1] * w[t2]))
    if name == "grid2x3_chi2":                            # the theta (all 7 edges) is there
        assert max(len(c) for c, _ in ws) == 7


def test_cycle_matrices_give_the_configuration_weight():
    """the ring formula W = Tr prod (A_k T_k) of the device path equals the general contraction of loopcorrection.jl:79-89, rectangular T_k included"""
    g = o.Graph(list(range(5)), [(0, 1), (1, 2), (2, 3), (0, 3), (1, 4)])
    rng = np.random.default_rng(3)
    bond = {frozenset((0, 1)): 2, frozenset((1, 2)): 3, frozenset((2, 3)): 2, frozenset((0, 3)): 3, frozenset((1, 4)): 2}
    tensors = {}
    for v in g.vertices:
        shp = (2,) + tuple(bond[frozenset((v, w))] for w in g.nbrs[v])
        tensors[v] = rng.standard_normal(shp) + 1j * rng.standard_normal(shp)
    rg = lr.RefGraph(g.vertices, g.edges)
    ts, ms, _ = lr.rescale(tensors, lr.bp(tensors, rg), rg)
    ring = [0, 1, 2, 3]
    edges = [(0, 1), (1, 2), (2, 3), (0, 3)]
    a, b = lr.cycle_weight(lr.cycle_matrices(ts, ms, rg, ring)), lr.weight(ts, ms, rg, edges)
    assert abs(a - b) <= 1e-13 * max(1.0, abs(b))
    assert abs(lr.cycle_weight(lr.cycle_matrices(ts, ms, rg, [2, 1, 0, 3])) - b) <= 1e-13 * max(1.0, abs(b))      # the other way round, another start
