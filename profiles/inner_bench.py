"""Sweeps of inner(psi, phi; alg = "bp") (tnqs_inner_bp) beside sweeps of update(bpc) (tnqs_bp_update) on the same state.  ComplexF32 states generated on the
device as bench.py generates them (tnqs_set_site_random), 7x7 and 20x20; psi at chi = 32, phi at chi = 32 (another seed) and at chi = 16.  A call of k sweeps is
timed on the host clock (both calls end in a stream synchronise; median of the repeats after a warm-up call, profiler off); the time of ONE sweep is
(t(k = 5) - t(k = 1)) / 4, which leaves out what a call does once (the pass for the vertex scalars, the scalars, the read-back).  Reported per lattice: the sweep of
inner(psi, psi), of inner(psi, phi) at 32 / 32 and at 32 / 16, the sweep of update(psi), and the ratio inner(psi, psi) / update(psi) -- the Hermitian path does about
half the mode products and shares partial products between levels, so a ratio near or above 2 is what one expects of a first version.
    python profiles/inner_bench.py [7 | 20] [repeats]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np
import tnqs_amd as tn


def device_state(n, chi, seed, d=2):
    g = tn.named_grid((n, n))
    bpc = tn.BeliefPropagationCache(tn.tensornetworkstate(np.complex64, lambda v: "↑", g))
    for v in g.vertices:
        z = g.degree(v)
        bpc._set_random(v, [chi] * z, seed, scale=1.0 / np.sqrt(d * float(chi) ** z))
    return bpc


def timed(fn, repeats):
    fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def per_sweep(call, repeats):
    t1, t5 = timed(lambda: call(1), repeats), timed(lambda: call(5), repeats)
    return (t5 - t1) / 4, t1


def lattice(n, repeats):
    psi, phi32, phi16 = device_state(n, 32, 1234), device_state(n, 32, 4321), device_state(n, 16, 4321)
    out = dict(lattice=f"{n}x{n}", repeats=repeats)
    for name, bra in (("inner_psi_psi", psi), ("inner_32_32", phi32), ("inner_32_16", phi16)):
        s, t1 = per_sweep(lambda k: tn.log_inner(psi, bra, cache_update_kwargs=dict(maxiter=k)), repeats)
        out[name + "_sweep_ms"], out[name + "_one_sweep_call_ms"] = 1e3 * s, 1e3 * t1
    s, t1 = per_sweep(lambda k: tn.update(psi, maxiter=k), repeats)
    out["update_sweep_ms"], out["update_one_sweep_call_ms"] = 1e3 * s, 1e3 * t1
    out["inner_over_update"] = out["inner_psi_psi_sweep_ms"] / out["update_sweep_ms"]
    return out


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    print(json.dumps(lattice(n, repeats)), flush=True)
