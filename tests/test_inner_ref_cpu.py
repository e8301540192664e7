"""The numpy restatement of inner(psi, phi; alg = "bp") (tests/inner_ref.py) against what it must satisfy on its own: exactness on trees, the norm network as
the special case phi = psi, the symmetries of a sesquilinear form, product states, and the cancellation constant the GPU end-to-end bound relies on.  No GPU."""
import numpy as np
import pytest

import tnqs_oracle as o
import inner_ref as ref

EPS = np.finfo(np.float64).eps


def _measured(what, err, bound):
    print(f"MEASURED {what}: {err:.3e} (bound {bound:.3e})")


@pytest.mark.parametrize("name", ["comb33", "path5"])
def test_one_sweep_is_exact_on_trees(name):
    g, ket, bra = ref.tree_case(name)
    z = np.exp(ref.log_inner(ref.run(g, ket, bra, 1)))
    want = ref.dense_inner(g, ket, bra)
    err = abs(z - want) / abs(want)
    _measured(f"tree {name} one sweep against the dense overlap", err, 200 * EPS)
    assert err < 200 * EPS


def test_self_overlap_is_the_partition_function_of_the_norm_network():
    g = o.named_grid((3, 3))
    rng = np.random.default_rng(3)
    psi = ref.tensors_of(g, ref.random_dims(g, rng, 2, 3), rng, bias=1.0)
    seq = o.forest_cover_edge_sequence(g)
    lz = ref.log_inner(ref.run(g, psi, psi, 6, seq=seq))
    bpc = o.update(o.BeliefPropagationCache(o.TensorNetworkState(g, dict(psi))), maxiter=6, edge_sequence=seq)
    want = np.log(complex(o.partitionfunction(bpc)))
    err = ref.log_close(lz, want)
    _measured("log inner(psi, psi) against log partitionfunction", err, 1e-13)
    assert err < 1e-13


def test_conjugate_symmetry_and_linearity():
    g, ket, bra = ref.loopy_case("grid3x4")
    a = ref.log_inner(ref.run(g, ket, bra, 12))
    b = ref.log_inner(ref.run(g, bra, ket, 12))
    err = ref.log_close(b, np.conj(a))
    _measured("inner(phi, psi) against conj(inner(psi, phi))", err, 1e-12)
    assert err < 1e-12
    c = 0.7 - 1.3j
    v0 = g.vertices[4]
    scaled = dict(ket); scaled[v0] = c * ket[v0]
    err = ref.log_close(ref.log_inner(ref.run(g, scaled, bra, 12)), a + np.log(c))
    _measured("inner(c psi, phi) against c inner(psi, phi)", err, 1e-12)
    assert err < 1e-12


def test_product_states_give_the_product_of_site_overlaps():
    g = o.named_grid((3, 3))
    rng = np.random.default_rng(5)
    one = {e: 1 for e in g.edges}
    ket, bra = ref.tensors_of(g, one, rng), ref.tensors_of(g, one, rng)
    want = np.prod([np.sum(ket[v] * bra[v].conj()) for v in g.vertices])
    z = np.exp(ref.log_inner(ref.run(g, ket, bra, 2)))
    err = abs(z - want) / abs(want)
    _measured("product states on the 3 x 3 grid", err, 200 * EPS)
    assert err < 200 * EPS


def test_vertex_scalars_of_the_loopy_gpu_cases_do_not_cancel():
    """sum|t| / |sum t| over the terms of every vertex scalar of every loopy end-to-end case, after 3 and after 8 sweeps: the 1e-6 (nv + ne) bound of
    tests/test_gpu_inner.py counts one f32 contraction of relative error 1e-6 per vertex, which holds only while this stays of order 1"""
    worst = 0.0
    for name in ref.LOOPY_CASES:
        g, ket, bra = ref.loopy_case(name)
        fc = ref.FormCache(g, ket, bra)
        seq = o.forest_cover_edge_sequence(g)
        for i in range(1, 9):
            ref.sweep(fc, seq)
            if i in (3, 8):
                worst = max(worst, ref.cancellation(fc))
    _measured("cancellation factor of the loopy cases", worst, 2.0)
    assert worst <= 2.0
    assert abs(worst - ref.LOOPY_CANCELLATION) < 1e-3
