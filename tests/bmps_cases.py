"""The boundary-MPS cases that tests/test_bmps_ref_cpu.py pins on the host and tests/test_gpu_bmps.py runs on the device: states, observables and the dense answers."""
import functools

import numpy as np

Z = np.diag([1.0, -1.0]).astype(complex)
H3 = np.array([[0.3, 0.2 - 0.1j, 0.5j], [0.2 + 0.1j, -0.7, 0.4], [-0.5j, 0.4, 0.1]])      # a Hermitian operator for the d = 3 case


def grid_state(dims, chi, d=2, seed=0, dtype=np.complex128):
    """a random state on the open grid `dims`; chi: one bond dimension, or a tuple to draw every edge's from"""
    import tnqs_amd as tn
    g = tn.named_grid(dims)
    rng = np.random.default_rng(seed)
    edim = {frozenset(e): (int(rng.choice(chi)) if isinstance(chi, tuple) else chi) for e in g.edges}
    tensors = {}
    for v in g.vertices:
        shp = (d,) + tuple(edim[frozenset((v, w))] for w in g.neighbors(v))
        tensors[v] = ((rng.standard_normal(shp) + 1j * rng.standard_normal(shp)) / np.sqrt(2)).astype(dtype)
    return g, tensors


# name: (dims, chi, d, R, partition_by, seed, observables [(vertices, operators)]) -- every link at its full dimension, so boundary MPS is exact
EXACT_CASES = {
    "3x3_chi2_R4": ((3, 3), 2, 2, 4, "row", 11, [([(2, 1)], [Z]), ([(2, 1), (2, 3)], [Z, Z]), ([(3, 2)], [np.eye(2)])]),      # test/test_boundarymps.jl
    "3x4_chi2_R16_row": ((3, 4), 2, 2, 16, "row", 12, [([(2, 2)], [Z]), ([(1, 1), (1, 4)], [Z, Z]), ([(3, 2), (3, 3)], [Z, Z])]),
    "3x4_chi2_R16_col": ((3, 4), 2, 2, 16, "col", 12, [([(2, 2)], [Z]), ([(1, 3), (3, 3)], [Z, Z]), ([(1, 1), (2, 1)], [Z, Z])]),
    "4x3_chi2_R16_row": ((4, 3), 2, 2, 16, "row", 13, [([(3, 2)], [Z]), ([(4, 1), (4, 3)], [Z, Z])]),
    "4x3_chi2_R16_col": ((4, 3), 2, 2, 16, "col", 13, [([(3, 2)], [Z]), ([(1, 2), (4, 2)], [Z, Z])]),
    "3x3_chi123_R16": ((3, 3), (1, 2, 3), 2, 16, "row", 14, [([(2, 2)], [Z]), ([(1, 1), (1, 3)], [Z, Z])]),
    "3x3_chi2_d3_R4": ((3, 3), 2, 3, 4, "col", 15, [([(2, 2)], [H3]), ([(1, 3), (3, 3)], [H3, H3])]),
}


@functools.lru_cache(maxsize=None)
def exact_case(name):
    """(graph, tensors in complex128, R, partition_by, observables, dense expectation values, dense log norm^2)"""
    import statevector as sv
    import tnqs_oracle as o
    dims, chi, d, R, by, seed, obs = EXACT_CASES[name]
    g, tensors = grid_state(dims, chi, d, seed)
    og = o.Graph(list(g.vertices), list(g.edges))
    psi = sv.tns_to_statevector(o.TensorNetworkState(og, dict(tensors)))
    dense = [complex(sv.expect_statevector_multi(psi, og, dict(zip(vs, ops)))) for vs, ops in obs]
    return g, tensors, R, by, obs, dense, float(np.log(np.vdot(psi, psi).real))


TRUNCATED_OPS = {"Z": Z, "I": np.eye(2)}


@functools.lru_cache(maxsize=None)
def truncated_cases():
    """what tests/bmps_truncated_select.py kept: per case chi, seed, observables, the dense values, and per (element type, R) the tolerance, the reference values and their
    spread over five null-space completions"""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "meta", "bmps_truncated.json")) as f:
        return json.load(f)
