"""CPU pins of tests/site_kernels_ref.py, the references tests/test_gpu_site_kernels.py holds the sampling, one-site gate and form-scalar kernels against: the diagonal
against the oracle's one-site density matrix, the counter-based uniform's range, grid and a handful of literal values, the one-site gate and the form scalar against plain
numpy, and the ownership map of site_prob_partial_kernel for every (n, d, nblocks) the GPU test runs."""
import ctypes as C
import math

import numpy as np
import pytest

import tnqs_oracle as o
import sampling_ref as sr
import site_kernels_ref as ref


def _absorbed(bpc, v):
    g = bpc.g
    t = bpc.tns.tensors[v]
    for k in g.nbrs[v]:
        t = o._absorb(t, g.leg(v, k), bpc.message((k, v)))
    return t


def test_diagonal_is_the_oracles_one_site_density_matrix():
    g = o.comb_tree((3, 2))
    psi = o.random_state(np.complex128, g, 3, d=3, seed=5)
    bpc = o.update(o.BeliefPropagationCache(psi))
    for v in g.vertices:
        t, p = _absorbed(bpc, v), bpc.tns.tensors[v]
        dg, ab = ref.diag(t.ravel(order="F"), p.ravel(order="F"), 3)          # the device layout: site index fastest
        want = np.real(np.diag(o.rdm_1site(bpc, v)))
        assert np.all(np.abs(dg.astype(np.float64) - want) <= 64 * ref.U53 * ab.astype(np.float64)), (v, dg, want)
        assert np.all(ab >= np.abs(dg))
        prob = (dg / dg.sum()).astype(np.float64)
        assert np.allclose(prob, sr.site_probabilities(bpc, v), rtol=0, atol=1e-14)


def test_counter_uniform_range_grid_and_literal_values():
    triples = ref.counter_triples()
    assert 190 <= len(triples) <= 210 and len(set(triples)) == len(triples)
    assert (0, 0, 0) in triples and (ref.M64, ref.M64, ref.M64) in triples
    one_field = [t for t in triples if sum(a != b for a, b in zip(t, (0x0123456789ABCDEF, 7, 11))) == 1]
    assert len(one_field) >= 40
    us = [ref.counter_uniform(*t) for t in triples]
    for t, u in zip(triples, us):
        assert 0.0 <= u < 1.0 and (u * 2.0 ** 53) == int(u * 2.0 ** 53), (t, u)
        assert 0.0 < u < 1.0 - 2.0 ** -53, (t, u)           # what the GPU test's two draws per triple need
    assert len(set(us)) == len(us)                           # every field matters
    # computed once by the mirror; 53-bit integers u * 2^53
    lit = {(0, 0, 0): 1249383295688599, (0, 0, 1): 4847210530293497, (0, 1, 0): 6544642500206708, (1, 0, 0): 6246602021646768,
           (ref.M64, ref.M64, ref.M64): 496843650962290, (0x0123456789ABCDEF, 7, 11): 129941018562968, (42, 3, 5): 6519938698360247}
    for t, k in lit.items():
        assert ref.counter_uniform(*t) == k * 2.0 ** -53, (t, int(ref.counter_uniform(*t) * 2.0 ** 53))
    assert ref.mix64(0) == 0xE220A8397B1DCDAF                # splitmix64's first output for the seed 0


def test_draw_expect_follows_the_rule_of_sampling_ref():
    part = np.zeros((3, 16)); part[:, 0] = (0.25, 0.5, 0.25); part[:, 1] = (1.0, 1.0, 1.0); part[0, 2] = -1e-14
    st, p = ref.draw_expect(part, 3, 1e-8)
    assert st == 0 and p[2] == 0.0 and p[0] == 1.0 / (4.0 - 1e-14) and p[1] == 3.0 / (4.0 - 1e-14)
    assert sr.draw(p, p[0]) == 1 and sr.draw(p, np.nextafter(p[0], 0)) == 0 and sr.draw(p, 0.0) == 0
    assert ref.draw_expect(part, 3, 1e-16)[0] == 2
    for bad in (0.0, -1.0, np.inf, np.nan):
        q = np.zeros((1, 16)); q[0, 0] = bad
        st, p = ref.draw_expect(q, 2, 1e-8)
        assert st == 1 and np.all(p == 0)
    assert ref.seq_sum([1.0, 2.0 ** -53, 2.0 ** -53]) == 1.0 and math.fsum([1.0, 2.0 ** -53, 2.0 ** -53]) > 1.0      # sequential, not exact


def test_site1_reference_against_numpy():
    rng = np.random.default_rng(3)
    G = rng.standard_normal((2, 2)) + 1j * rng.standard_normal((2, 2))
    x = (rng.standard_normal((9, 2)) + 1j * rng.standard_normal((9, 2))).astype(np.complex64)
    out, b = ref.site1(G, x)
    for i in range(9):
        assert np.allclose(out[i], G @ x[i].astype(np.complex128), rtol=0, atol=1e-14)
    assert np.all(b > 0) and np.all(b < 20 * ref.U24 * np.abs(x).sum(axis=1, keepdims=True) * np.abs(G).max())
    abi = ref.gate_abi(G)
    assert abi[2] == G[1, 0].real and abi[3] == G[1, 0].imag and abi[4] == G[0, 1].real and abi[7] == G[1, 1].imag
    assert ref.norm2_fsum(x) == pytest.approx(float(np.sum(np.abs(x.astype(np.complex128)) ** 2)), rel=1e-14)
    assert float(ref.norm2_ld(x)) == pytest.approx(ref.norm2_fsum(x), rel=1e-15)
    assert ref.norm_partial_k(1, 64) == 16 and ref.norm_partial_k(256 * 64 + 1, 64) == 20 and ref.ulp(1.0) == 2.0 ** -52


def test_inner_scalar_reference_against_numpy():
    rng = np.random.default_rng(4)
    for rows, cols in ((1, 1), (2, 3), (3, 2), (17, 31)):
        m = rng.standard_normal(rows * cols) + 1j * rng.standard_normal(rows * cols)
        mr = rng.standard_normal(rows * cols) + 1j * rng.standard_normal(rows * cols)
        I = np.eye(rows, cols).ravel(order="F")                          # the rectangular delta of a null message, flat [a + rows b]
        assert np.array_equal(ref.delta(rows, cols), I)
        v, are, aim = ref.inner_scalar(m, mr, rows, cols, None, 0, None, None)
        assert abs(v - np.sum(m * mr)) <= 1e-13 * (are + aim)
        v, _, _ = ref.inner_scalar(m, None, rows, cols, None, 0, None, None)
        assert abs(v - np.sum(m * I)) <= 1e-13 * (are + aim)
        v, _, _ = ref.inner_scalar(None, None, rows, cols, None, 0, None, None)
        assert v == min(rows, cols)
        rs = 0.5 - 0.25j
        v1, a1, b1 = ref.inner_scalar(m, mr, rows, cols, rs, 1, 3.0, None)
        assert abs(v1 - np.sum(m * mr) * rs * 3.0) <= 1e-13 * (a1 + b1)
        assert ref.inner_scalar(m, mr, rows, cols, rs, 0, None, 2.0)[0] == pytest.approx(np.sum(m * mr) * 2.0, rel=1e-13)
        assert ref.inner_scalar(m, mr, rows, cols, 0j, 1, None, None)[0] == pytest.approx(np.sum(m * mr), rel=1e-13)      # a zero raw sum leaves the value as it is


def _all_cases():
    cases = [(n, d, nb) for d in ref.SITE_DIMS for n, nb in ref.site_prob_cases(d)]
    return cases + [(n, d, 0) for n, d in ref.BIG_CASE.values()]


def test_gpu_case_list_reaches_the_launches_it_is_meant_to():
    cases = _all_cases()
    for d in ref.SITE_DIMS:
        nbs = {nb if nb else ref.plan_site_prob(n, d) for n, dd, nb in cases if dd == d}
        assert {1, 2, 3, 5} <= nbs
        assert any(n == d for n, dd, _ in cases if dd == d) and any(d < n < 256 for n, dd, _ in cases if dd == d)
    assert all(n % d == 0 for n, d, _ in cases)
    assert all(ref.plan_site_prob(n, d) == 1024 and n > 2 ** 20 and 256 % d for n, d in ref.BIG_CASE.values())
    # an offset of the first lane that is not zero: more than one workgroup and d does not divide 256
    assert sum(1 for n, d, nb in cases if 256 % d and (nb or ref.plan_site_prob(n, d)) > 1) >= 15


def test_plan_mirror_is_the_librarys_plan():
    import tnqs_amd as tn
    lib = C.CDLL(tn.LIB_PATH)
    for n, d, _ in _all_cases() + [(1024, 1, 0), (1025, 1, 0), (2 ** 20, 2, 0)]:
        nb = C.c_int(-1)
        assert lib.tnqs_dbg_site_prob(0, n, d, None, None, 0, None, 0, C.byref(nb)) == 0      # host only: no partial array
        assert nb.value == ref.plan_site_prob(n, d), (n, d)
    assert lib.tnqs_dbg_site_prob(0, 7, 3, None, None, 0, None, 0, None) == -1                # n is not a multiple of d
    assert lib.tnqs_dbg_site_prob(0, 17, 17, None, None, 0, None, 0, None) == -1
    assert lib.tnqs_dbg_site_prob(2, 4, 2, None, None, 0, None, 0, None) == -1


@pytest.mark.parametrize("d", ref.SITE_DIMS)
def test_ownership_map_partials_sum_to_the_diagonal(d):
    """for every launch of the GPU test: the per-workgroup, per-site-index partials the map prescribes add up to the reference diagonal, an element's site index is its
    thread's (e mod d = (e mod NT) mod d), idle threads and slots s >= d hold nothing; for the small launches the map is also the kernel's documented loop, thread by thread"""
    cases = [(n, dd, nb) for n, dd, nb in _all_cases() if dd == d]
    for n, _, nb in cases:
        nblocks = nb if nb else ref.plan_site_prob(n, d)
        dtype = 0 if n < 2 ** 20 else [k for k, v in ref.BIG_CASE.items() if v == (n, d)][0]
        t, p = ref.site_inputs(n, d, dtype, 1)
        part, ab = ref.partials(t, p, d, nblocks)
        dg, dab = ref.diag(t, p, d)
        assert part.shape == (nblocks, 16) and np.all(part[:, d:] == 0) and np.all(ab[:, d:] == 0)
        tot = part.sum(axis=0)[:d]
        tol = (n // d + 16) * 2.0 ** -63 * dab                  # two orders of adding n / d longdoubles
        assert np.all(np.abs(tot - dg) <= tol), (n, d, nblocks)
        assert np.all(np.abs(ab.sum(axis=0)[:d] - dab) <= tol)
        NT = 256 * nblocks - (256 * nblocks) % d
        blk, s = ref.owner(n, d, nblocks)
        e = np.arange(n)
        assert np.array_equal(s, (e % NT) % d) and blk.max() < nblocks and NT % d == 0 and NT >= d
        if n <= 6000:
            terms = ref.diag_terms(t, p)
            sim = np.zeros((nblocks, 16), dtype=ref.LD)
            for th in range(NT):                                     # thread th of the launch: e = th, th + NT, ... (threads NT .. 256 nblocks - 1 are idle)
                for k in range(th, n, NT):
                    sim[th // 256, th % d] += terms[k]
            assert np.all(np.abs(sim - part) <= (n // d + 16) * 2.0 ** -63 * ab), (n, d, nblocks)
    # the magnitudes of neighbouring site indices differ by 10^6 in psi
    if d > 1:
        _, p = ref.site_inputs(d * 64, d, 0, 1)
        rms = np.sqrt(np.mean(np.abs(p.reshape(-1, d)) ** 2, axis=0))
        assert rms[0] / rms[1] > 1e5
