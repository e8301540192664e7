"""CPU checks of tests/amplitude_ref.py, the numpy restatement tnqs_amplitudes_bp is tested against (tests/test_gpu_amplitudes.py): exact on trees, the condition on
the inputs that the end-to-end bound assumes (no vertex scalar cancels), the all-ones start convention, per-string freezing under a tolerance, the seed of the
sampling tie, and the bounds helpers."""
import numpy as np
import pytest

import tnqs_oracle as o
import inner_ref
import amplitude_ref as ref


def all_strings(nv):
    return np.array([[(n >> i) & 1 for i in range(nv)] for n in range(2 ** nv)], dtype=np.int32)


@pytest.mark.parametrize("name", ["comb33", "path5"])
def test_trees_one_sweep_is_the_dense_amplitude_and_the_overlap_with_the_basis_state(name):
    g, ket, _ = inner_ref.tree_case(name)
    psi = ref.dense_state(g, ket)
    rng = np.random.default_rng(3)
    for x in ref.random_strings(rng, g, 6):
        got = ref.log_amplitude(ref.run(g, ket, dict(zip(g.vertices, x)), 1))
        assert ref.log_close(got, np.log(psi[tuple(x)])) < 1e-12
        basis = {v: np.eye(2)[xv].reshape((2,) + (1,) * len(g.nbrs[v])) for v, xv in zip(g.vertices, x)}
        want = inner_ref.log_inner(inner_ref.run(g, ket, basis, 1))
        assert ref.log_close(got, want) < 1e-12


def test_all_strings_of_a_tree_sum_to_the_dense_norm():
    g, ket, _ = inner_ref.tree_case("comb33")
    la = ref.log_amplitudes(g, ket, all_strings(len(g.vertices)), 1)
    assert abs(np.sum(np.abs(np.exp(la)) ** 2) / np.sum(np.abs(ref.dense_state(g, ket)) ** 2) - 1) < 1e-12


def loopy_inputs():
    """(name, g, tensors, strings) of every loopy end-to-end case of the GPU test"""
    out = []
    for name in sorted(inner_ref.LOOPY_CASES):
        g, t = ref.loopy_state(name)
        out.append((name, g, t, ref.random_strings(np.random.default_rng(5), g, 6)))
    for chi in (16, 32):
        g, t = ref.grid33_state(chi)
        out.append((f"grid3x3 chi {chi}", g, t, ref.random_strings(np.random.default_rng(chi), g, 4)))
    g, t = ref.grid33_state(ref.MIXED_DIMS)
    out.append(("grid3x3 mixed", g, t, ref.random_strings(np.random.default_rng(7), g, 4)))
    return out


def test_no_vertex_scalar_cancels_on_the_loopy_inputs():
    """the end-to-end bound of the GPU test assumes a cancellation factor <= 2 after 3 and after 8 sweeps"""
    for name, g, t, xs in loopy_inputs():
        seq = o.forest_cover_edge_sequence(g)
        worst = 0.0
        for x in xs:
            for ns in ((3,) if "chi" in name else (3, 8)):
                worst = max(worst, ref.cancellation(ref.run(g, t, dict(zip(g.vertices, x)), ns, seq=seq)))
        print(f"MEASURED cancellation {name}: {worst:.4f}")
        assert worst <= 2.0, (name, worst)


def test_the_start_convention_is_all_ones_not_e0():
    """after 3 sweeps on a loopy graph the ones start and inner_ref's delta start (e_0 against a chi = 1 bra) differ far above rounding; both are exact on trees"""
    g, t = ref.loopy_state("grid3x4")
    x = ref.random_strings(np.random.default_rng(5), g, 2)[1]
    seq = o.forest_cover_edge_sequence(g)
    ones = ref.log_amplitude(ref.run(g, t, dict(zip(g.vertices, x)), 3, seq=seq))
    basis = {v: np.eye(2)[xv].reshape((2,) + (1,) * len(g.nbrs[v])) for v, xv in zip(g.vertices, x)}
    e0 = inner_ref.log_inner(inner_ref.run(g, t, basis, 3, seq=seq))
    d = ref.log_close(ones, e0)
    print(f"MEASURED ones start against e0 start after 3 sweeps: {d:.3e}")
    assert 1e-9 < d < 1e-2
    ac = ref.AmpCache(g, t, dict(zip(g.vertices, x)))
    e = seq[0]
    assert np.array_equal(ac.message(e), np.ones(t[e[0]].shape[g.leg(e[0], e[1])]))


def freezing_case():
    g = o.named_grid((3, 3))
    rng = np.random.default_rng(17)
    t = ref.freezing_state(g, 3, rng)
    xs = ref.random_strings(rng, g, 5)
    xs[1] = 1                                           # the all-ones string: every site generic
    return g, t, xs


FREEZE_TOLS = {np.complex64: 1e-6, np.complex128: 1e-9}      # per element type of the GPU test


@pytest.mark.parametrize("FREEZE_TOL", sorted(FREEZE_TOLS.values()))
def test_freezing_each_string_stops_on_its_own(FREEZE_TOL):
    g, t, xs = freezing_case()
    seq = o.forest_cover_edge_sequence(g)
    info = {}
    la = ref.log_amplitudes(g, t, xs, 40, seq=seq, tolerance=FREEZE_TOL, info=info)
    print(f"MEASURED freezing niter {info['niter']}")
    assert all(info["converged"])
    assert info["niter"][0] == 2 and info["niter"][1] > 2      # rank-one slices: the second sweep reproduces the first
    for j, x in enumerate(xs):                                 # each string's result in the batch is its result alone
        i1 = {}
        a1 = ref.log_amplitude(ref.run(g, t, dict(zip(g.vertices, x)), 40, seq=seq, tolerance=FREEZE_TOL, info=i1))
        assert a1 == la[j] and i1["niter"] == info["niter"][j]
    # no diff of a string sits at the tolerance: the device's sweep counts can be held to these exactly
    for x, n in zip(xs, info["niter"]):
        ac = ref.AmpCache(g, t, dict(zip(g.vertices, x)))
        diffs = [ref.sweep(ac, seq) for _ in range(n)]
        assert all(dd > 10 * FREEZE_TOL for dd in diffs[:-1]) and diffs[-1] < FREEZE_TOL / 10, diffs


def test_at_most_a_quarter_of_the_evolved_state_strings_are_dropped():
    """the evolved-state case of the GPU test, evolved by the oracle: the strings whose vertex scalars cancel (factor above 2) are left out; at most a quarter may be"""
    import tnqs_amd as tn
    g, t0, drawn = ref.evolved_case()
    layer = ref.evolved_layer(tn.edge_color(tn.NamedGraph(list(g.vertices), list(g.edges)), 4), g.vertices)
    bpkw = dict(maxiter=20, tolerance=1e-10)
    oc = o.update(o.BeliefPropagationCache(o.TensorNetworkState(g, {v: t.astype(np.complex128) for v, t in t0.items()})), **bpkw)
    oc, _ = o.apply_gates(layer, oc, apply_kwargs=dict(maxdim=3, cutoff=1e-12, normalize_tensors=True), bp_update_kwargs=bpkw)
    tensors = {v: oc.tns.tensors[v] for v in g.vertices}
    assert max(t.shape[1] for t in tensors.values()) > 1
    kept = ref.strings_that_do_not_cancel(g, tensors, drawn, o.forest_cover_edge_sequence(g))
    print(f"MEASURED evolved state: {len(kept)} of {len(drawn)} strings kept")
    assert 4 * len(kept) >= 3 * len(drawn)


def test_the_sampling_tie_meets_no_small_conditional_probability():
    """the bound of the GPU test's sampling tie divides by the smallest conditional probability of the replay"""
    import sampling_ref
    g, t, uniforms = ref.sampling_case()
    bpc = o.update(o.BeliefPropagationCache(o.TensorNetworkState(g, dict(t))), maxiter=1)
    cfg, prob, _ = sampling_ref.sample_ref(bpc, uniforms, maxiter=1)
    print(f"MEASURED sampling tie: smallest conditional probability {prob.min():.4f}")
    assert prob.min() >= ref.SAMPLING_PMIN
    # log q of the replay is the normalised probability of the dense state on a tree
    psi = ref.dense_state(g, t)
    p = np.abs(psi[tuple(cfg.T)]) ** 2 / np.sum(np.abs(psi) ** 2)
    assert np.max(np.abs(np.log(prob).sum(axis=1) - np.log(p))) < 1e-12


def test_bounds_helpers():
    assert ref.unit_roundoff(np.complex64) == 2.0 ** -24 and ref.unit_roundoff(np.complex128) == 2.0 ** -53
    assert ref.dot_bound(np.complex64, 32, 2.0) == 8 * 2.0 ** -24 * 32 * 2.0
    assert ref.dot_bound(np.complex128, 3, 1.0, extra=2) == 8 * 2.0 ** -53 * 5
    g = o.named_grid((3, 3))
    assert ref.log_bound(g, np.complex64) == 1e-6 * 21 and ref.log_bound(g, np.complex128, 2.0) == 2 * 200 * np.finfo(np.float64).eps * 21
