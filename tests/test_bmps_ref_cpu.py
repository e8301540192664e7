"""tests/bmps_ref.py -- the numpy restatement of the reference's boundary-MPS contraction that tests/test_gpu_bmps.py compares the device against -- pinned on the host:
it equals the dense simulator (oracle/statevector.py) wherever every link is at its full dimension, <I> = 1 at any bond dimension, and the shapes it derives are the
reference's (virtual_index_dimension, src/MessagePassing/boundarympscache.jl:119-143)."""
import numpy as np
import pytest

import bmps_cases as cases
import bmps_ref as ref


@pytest.mark.parametrize("name", sorted(cases.EXACT_CASES))
def test_exact_where_every_link_is_full(name):
    g, tensors, R, by, obs, dense, log_n2 = cases.exact_case(name)
    b = ref.BoundaryMPS(g, tensors, R, partition_by=by)
    nv, ne = len(g.vertices), len(g.edges)
    for (vs, ops), want in zip(obs, dense):
        got = b.expect(vs, ops)
        print(f"MEASURED bmps_ref {name} {vs}: |ref - dense| = {abs(got - want):.3e}")
        assert abs(got - want) < 1e-11
    lz = b.log_norm_sqr()
    print(f"MEASURED bmps_ref {name} log norm^2: |ref - dense| / (nv + ne) = {abs(lz - log_n2) / (nv + ne):.3e}")
    assert abs(lz - log_n2) / (nv + ne) < 1e-11
    assert all(s >= 2 for s in b.sweeps.values())      # a tolerance cannot stop the first sweep: epsilon is measured against cf = 0


def test_reference_case_norm_is_the_dense_norm_without_a_tolerance():
    """norm_sqr(alg = "boundarymps") of the reference's own test (test/test_boundarymps.jl: 3 x 3, chi = 2, R = 4), one sweep, no tolerance"""
    g, tensors, R, by, obs, dense, log_n2 = cases.exact_case("3x3_chi2_R4")
    b = ref.BoundaryMPS(g, tensors, R, partition_by="row", niters=1, tolerance=None)
    assert abs(b.log_norm_sqr() - log_n2) < 1e-10
    assert set(b.sweeps.values()) == {1}


@pytest.mark.parametrize("R", [1, 2, 3])
def test_identity_is_one_at_any_bond_dimension(R):
    g, tensors = cases.grid_state((3, 4), 3, 2, seed=5)
    b = ref.BoundaryMPS(g, tensors, R, partition_by="row")
    for v in [(1, 1), (2, 3), (3, 4)]:
        assert abs(b.expect([v], [np.eye(2)]) - 1) < 1e-12
    assert abs(b.expect([(2, 1), (2, 4)], [np.eye(2), np.eye(2)]) - 1) < 1e-12


def test_link_dimensions_and_qr_shapes():
    """virtual_index_dimension (:119-143): min(x1^2, x2^2, R) with x1 / x2 the products of the bond dimensions above / below the link; every QR has m >= n"""
    assert ref.link_dims([2, 2, 2], 4) == [1, 4, 4, 1]
    assert ref.link_dims([2, 2, 2, 2], 16) == [1, 4, 16, 4, 1]
    assert ref.link_dims([2, 2, 2, 2], 5) == [1, 4, 5, 4, 1]
    assert ref.link_dims([1, 3, 2], 64) == [1, 1, 4, 1]
    assert ref.link_dims([8] * 10, 64) == [1] + [64] * 9 + [1]
    for chis, R in [([2, 2, 2], 4), ([1, 3, 2, 3], 16), ([8] * 10, 64), ([16] * 4, 16), ([3, 1, 1, 2], 7)]:
        for m, n in ref.qr_shapes(chis, R):
            assert m >= n >= 1
    g, tensors = cases.grid_state((3, 3), (1, 2, 3), 2, seed=14)
    b = ref.BoundaryMPS(g, tensors, 5, partition_by="col")
    assert b.qr_log and all(m >= n for m, n in b.qr_log)
    for p in range(b.P - 1):
        chis = [tensors[b.rows[p][l]].shape[1 + list(g.neighbors(b.rows[p][l])).index(b.rows[p + 1][l])] for l in range(b.L)]
        link = ref.link_dims(chis, 5)
        for msgs in (b.down[p], b.up[p]):
            assert [m.shape for m in msgs] == [(link[l], chis[l], chis[l], link[l + 1]) for l in range(b.L)]


def test_seeded_null_space_completion_is_a_qr():
    rng = np.random.default_rng(3)
    for M in (np.ones((12, 4), dtype=complex), rng.standard_normal((9, 3)) @ np.diag([1, 0, 2]) + 0j):
        for seed in range(3):
            Q, Y = ref.qr_random_completion(seed)(M)
            assert np.abs(Q.conj().T @ Q - np.eye(Q.shape[1])).max() < 1e-13
            assert np.abs(Q @ Y - M).max() < 1e-13
    a, b = ref.qr_random_completion(0)(np.ones((12, 4), dtype=complex))[0], ref.qr_random_completion(1)(np.ones((12, 4), dtype=complex))[0]
    assert np.abs(a - b).max() > 1e-3


def test_refusals_of_the_partitioning():
    import tnqs_amd as tn
    with pytest.raises(ValueError, match="does not form a line"):
        ref.partition(tn.named_grid((4, 4), periodic=True), "row")
    with pytest.raises(ValueError, match="pseudo-edges"):
        ref.partition(tn.heavy_hexagonal_lattice(2, 2), "row")


def test_truncated_cases_are_conditioned():
    """the truncated cases of tests/test_gpu_bmps.py as tests/bmps_truncated_select.py recorded them: every fit of every run stopped by its tolerance before niters = 50, and
    the recorded reference values are what bmps_ref gives today (recomputed here for the plain numpy QR at the ComplexF32 tolerance, the cheap half)"""
    import bmps_truncated_select as sel
    kept = cases.truncated_cases()
    assert sorted(kept) == ["4x4_chi2", "4x4_chi3"]
    for name, e in kept.items():
        assert sorted(e["runs"]) == sorted(f"{dt}_R{R}" for dt in sel.TOLERANCES for R in sel.RS)
        g, _, gauged = sel.gauged_state(e["chi"], e["seed"])
        for key, run in e["runs"].items():
            assert max(run["sweeps"]) < 50 and run["tolerance"] == sel.TOLERANCES[key.split("_")[0]]
            floor = 1e-5 if key.startswith("complex64") else 1e-12
            print(f"MEASURED bmps truncated {name} {key}: sweeps {max(run['sweeps'])}, spread {max(run['spread']):.3e}, bound {max(10 * max(run['spread']), floor):.3e}")
            if key.startswith("complex64"):
                vals, sweeps = sel.run(g, gauged, int(key.split("_R")[1]), run["tolerance"], None)
                assert np.abs(np.asarray(vals) - (np.asarray(run["re"]) + 1j * np.asarray(run["im"]))).max() < 1e-9 and sweeps < 50
        # the selection itself, for the cheapest R of the case: all five null-space completions again -- the sweeps and the spread the device's bound comes from
        key = "complex64_R8"
        vals, sweeps = zip(*[sel.run(g, gauged, 8, e["runs"][key]["tolerance"], seed) for seed in sel.COMPLETIONS])
        vals = np.asarray(vals)
        assert list(sweeps) == e["runs"][key]["sweeps"]
        assert np.allclose(np.abs(vals - vals[0]).max(axis=0), e["runs"][key]["spread"], rtol=1e-6, atol=1e-12)
