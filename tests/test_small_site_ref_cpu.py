"""The float64 reference of tests/test_gpu_small_site.py (tests/small_site_ref.py) pinned against the oracle's updated_message / message_diff, on states whose
messages are random and NOT Hermitian -- a transposed matrix or a conjugated bra in the reference would show -- and the conditions the GPU tests' tolerances rest
on, checked where no GPU is needed: the complex64 restatement's worst error, the conditioning of every epilogue case, the scale sweep's range."""
import numpy as np
import pytest

import tnqs_oracle as o
import small_site_ref as ref


def _mixed_grid_state(rng):
    """3 x 3 grid, d = 3, a different dimension on every bond (2 .. 5)"""
    g = o.named_grid((3, 3))
    dim = {frozenset(e): 2 + (i % 4) for i, e in enumerate(g.edges)}
    tensors = {}
    for v in g.vertices:
        shp = (3,) + tuple(dim[frozenset((v, k))] for k in g.nbrs[v])
        tensors[v] = ref.crandn(rng, shp).astype(np.complex128)
    return o.TensorNetworkState(g, tensors)


def _random_messages(psi, rng, unset_every):
    """complex random non-Hermitian messages on the directed edges, every unset_every-th one left unset (identity)"""
    msgs = {}
    for i, e in enumerate(psi.g.directed_edges()):
        if unset_every and i % unset_every == 0:
            continue
        c = psi.bond_dim(*e)
        msgs[e] = ref.crandn(rng, (c, c)).astype(np.complex128)
    return msgs


@pytest.mark.parametrize("state", ["comb33_chi3", "grid33_mixed"])
def test_reference_message_and_finalize_match_the_oracle(state):
    rng = np.random.default_rng(5)
    if state == "comb33_chi3":
        psi = o.random_state(np.complex64, o.comb_tree((3, 3)), 3, seed=11)
        psi = o.TensorNetworkState(psi.g, {v: t.astype(np.complex128) for v, t in psi.tensors.items()})
    else:
        psi = _mixed_grid_state(rng)
    g = psi.g
    bpc = o.BeliefPropagationCache(psi, _random_messages(psi, rng, 4))
    assert any(np.max(np.abs(m - m.conj().T)) > 0.1 for m in bpc.messages.values())
    worst = 0.0
    for (u, v) in g.directed_edges():
        Ms = [bpc.messages.get((k, u)) for k in g.nbrs[u]]
        jo = g.leg(u, v) - 1
        raw = ref.message(psi.tensors[u], Ms, jo)
        want_raw = o.updated_message(bpc, (u, v), normalize=False)
        assert ref.rel_err(raw, want_raw) < 1e-13
        old = bpc.messages.get((u, v))
        for normalize in (False, True):
            m, diff = ref.finalize(raw, old, normalize)
            want = o.updated_message(bpc, (u, v), normalize=normalize)
            assert ref.rel_err(m, want) < 1e-13
            want_diff = o.message_diff(want, old if old is not None else np.eye(want.shape[0]))
            assert abs(diff - want_diff) < 1e-13
        # the complex64 restatement states the same contraction
        e32 = ref.rel_err(ref.message_c64(psi.tensors[u], Ms, jo), raw)
        worst = max(worst, e32)
    assert worst < 2e-6, worst


def test_finalize_skips_an_exactly_zero_sum():
    raw = np.array([[1 + 2j, -3j], [3j, -1 - 2j]])
    m, diff = ref.finalize(raw, None, True)
    assert np.array_equal(m, raw) and np.isfinite(diff)


def test_device_layout_round_trip():
    rng = np.random.default_rng(1)
    m = ref.crandn(rng, (3, 3))
    v = ref.flat(m)
    assert v[1 + 3 * 2] == m[1, 2] and np.array_equal(ref.unflat(v, 3), m)


def test_restatement_sweep_sizes_the_kernel_bound():
    """the bound of the GPU tests is four times the worst error of the complex64 restatement over their own cases: it has to be an f32-sized number (a few 1e-7;
    next to the 2-3e-6 the neighbouring kernel tests hold their kernels to)"""
    worst = ref.restatement_worst()
    assert 1e-7 < worst < 2e-6, worst
    assert ref.raw_bound() == 4 * worst


def test_every_epilogue_case_is_well_conditioned():
    """the normalised message's bound is the raw bound divided by |sum(m)| / sum|m|: the inputs are chosen so that this ratio is at least 0.1"""
    worst = 1.0
    for d, chis in ref.EPILOGUE_SHAPES:
        psi, Ms = ref.inputs(d, chis, tag=ref.EPILOGUE_TAG, psd_like=True)
        for jo in range(len(chis)):
            worst = min(worst, ref.conditioning(ref.message(psi, Ms, jo)))
    print(f"small-site epilogue cases: smallest conditioning {worst:.3f}")
    assert worst >= 0.1


def test_scale_sweep_stays_inside_f32_range():
    """psi scaled by 1e-18 .. 1e6: the complex64 restatement stays finite and within the bound, so the kernels are held to the same relative bound there"""
    for d, chis in ref.SCALE_SHAPES:
        psi, Ms = ref.inputs(d, chis, tag=2)
        for scale in ref.SCALES:
            p = (psi.astype(np.complex128) * scale).astype(np.complex64)
            for jo in range(len(chis)):
                got = ref.message_c64(p, Ms, jo)
                want = ref.message(p, Ms, jo)
                assert np.all(np.isfinite(got)) and np.max(np.abs(want)) > 1e-37
                assert ref.rel_err(got, want) < ref.raw_bound(), (d, chis, scale, jo)
