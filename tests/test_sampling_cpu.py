"""CPU-side checks of the sampling feature (sample, alg = "bp"; reference src/sampling.jl:3-46): the C ABI carries the four new entry points,
the numpy restatement the GPU tests replay against (tests/sampling_ref.py) is exact on a tree, and the Python front end refuses bad arguments
before it touches a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import tnqs_oracle as o
import statevector as sv
import sampling_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tnqs_project_site", "tnqs_site_dim", "tnqs_site_probabilities", "tnqs_sample_bp")


def test_sampling_symbols_are_declared_and_exported():
    import tnqs_amd as tn
    lib = ctypes.CDLL(tn.LIB_PATH)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tnqs.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), f"{name} is not declared in include/tnqs.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in tn.EXPORTS
    assert lib.tnqs_version() == 102
    for name in ("sample", "sample_with_probabilities", "site_probabilities"):
        assert callable(getattr(tn, name))
    assert callable(tn.BeliefPropagationCache.project)


def test_reference_sampler_is_exact_on_a_tree():
    """BP is exact on trees: the product of the step probabilities of every drawn x is |<x|psi>|^2 / <psi|psi>"""
    g = o.comb_tree((3, 2))
    assert len(g.vertices) == 6 and g.is_tree()
    psi = o.random_state(np.complex128, g, 3, seed=11)
    bpc = o.update(o.BeliefPropagationCache(psi))
    u = np.random.default_rng(7).random((24, 6))
    cfg, prob, margin = sr.sample_ref(bpc, u)
    amp = sv.tns_to_statevector(psi)
    exact = np.abs(amp) ** 2 / np.sum(np.abs(amp) ** 2)
    assert len({tuple(c) for c in cfg}) > 4                      # the draws are not all the same string
    for j in range(len(u)):
        assert abs(np.prod(prob[j]) - exact[tuple(cfg[j])]) <= 1e-12, (j, np.prod(prob[j]), exact[tuple(cfg[j])])
    assert np.all((margin >= 0) & (margin <= 1))
    # the input cache is untouched (the sampler works on copies)
    assert all(bpc.tns.tensors[v].shape[0] == 2 for v in g.vertices)


def test_reference_draw_rule():
    assert sr.draw([0.25, 0.75], 0.0) == 0 and sr.draw([0.25, 0.75], 0.2499) == 0 and sr.draw([0.25, 0.75], 0.25) == 1
    assert sr.draw([0.5, 0.5 - 1e-9], 1.0 - 1e-12) == 1          # no cdf entry above u: the last configuration
    assert sr.draw([0.2, 0.3, 0.5], 0.5) == 2 and sr.draw([1.0], 0.7) == 0


def test_sample_argument_checks_need_no_device():
    import tnqs_amd as tn
    g = tn.named_comb_tree((3, 2))
    psi = tn.random_tensornetworkstate(np.complex128, g, 2, seed=1)
    with pytest.raises(tn.TnqsError, match='only alg = "bp" is implemented on the HIP path'):
        tn.sample(psi, 3, alg="boundarymps")
    with pytest.raises(tn.TnqsArgumentError, match="nsamples"):
        tn.sample(psi, -1)
    with pytest.raises(tn.TnqsArgumentError, match="shape"):
        tn.sample(psi, 3, uniforms=np.zeros((2, 6)))
    with pytest.raises(tn.TnqsArgumentError, match="shape"):
        tn.sample(psi, 3, uniforms=np.zeros((3, 5)))
    with pytest.raises(tn.TnqsArgumentError, match=r"\[0, 1\)"):
        tn.sample(psi, 3, uniforms=np.ones((3, 6)))
    with pytest.raises(tn.TnqsArgumentError, match=r"\[0, 1\)"):
        tn.sample_with_probabilities(psi, 3, uniforms=np.full((3, 6), -0.1))
