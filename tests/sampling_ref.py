"""CPU restatement of sample(psi, nsamples; alg = "bp") (reference src/sampling.jl:18-43) over the numpy oracle, driven by explicit
uniforms: what the device sampler is replayed against.  Slicing t[x:x+1] keeps the oracle's axis convention (site axis first, dimension 1)."""
import numpy as np

import tnqs_oracle as o


def draw(p, u):
    """x = the first s with u < cdf[s], the last s if there is none (the rule of tnqs_sample_bp)"""
    hit = np.nonzero(u < np.cumsum(np.asarray(p, dtype=np.float64)))[0]
    return int(hit[0]) if len(hit) else len(p) - 1


def site_probabilities(bpc, v):
    diag = np.real(np.diag(o.rdm_1site(bpc, v))).astype(np.float64)
    return diag / diag.sum()


def sample_ref(bpc, uniforms, **bp_update_kwargs):
    """-> (configs [nsamples, nv] int, probs [nsamples, nv] p[x] of every step, margins [nsamples, nv] distance of u to the nearest inner
    cdf boundary of that step).  `bpc` is an updated oracle cache and is not changed."""
    vs = list(bpc.g.vertices)
    uniforms = np.asarray(uniforms, dtype=np.float64)
    cfg = np.zeros(uniforms.shape, dtype=np.int64); prob = np.zeros(uniforms.shape); margin = np.ones(uniforms.shape)
    for j, us in enumerate(uniforms):
        c = bpc.copy()
        for i, v in enumerate(vs):
            p = site_probabilities(c, v)
            x = draw(p, us[i])
            cfg[j, i], prob[j, i] = x, p[x]
            if len(p) > 1:
                margin[j, i] = np.min(np.abs(us[i] - np.cumsum(p)[:-1]))
            c.tns.tensors[v] = c.tns.tensors[v][x:x + 1]
            if i + 1 < len(vs):
                c = o.update(c, **bp_update_kwargs)
    return cfg, prob, margin
