"""log_amplitudes (tnqs_amplitudes_bp) for B in {1, 64, 1024} random bitstrings in ONE call, beside what the library offered before it: a loop of B = 64 calls of
log_inner(psi, |x>) (tnqs_inner_bp), each with the chi = 1 basis state of its string uploaded to a temporary handle -- the loop cannot avoid the uploads, so they are
inside its timed window.  ComplexF32 states generated on the device as bench.py generates them (tnqs_set_site_random), 7x7 and 20x20 at chi = 32; maxiter = 5, no
tolerance, the default sequence on both sides.  A call is timed on the host clock (every call ends in a stream synchronise; median of the repeats after a warm-up call
of the same shape, profiler off).  Reported per lattice: the call times, the loop time, loop / call at B = 64, and the time per string of each call.
    python profiles/amplitude_bench.py [7 | 20] [repeats]
    python profiles/amplitude_bench.py [7 | 20] once B      one warmed-up call of B strings and nothing else (the window of a kernel trace, taken in a run of its own)"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np
import tnqs_amd as tn

SWEEPS = 5


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
    return float(np.median(ts)), float(max(ts) - min(ts))


def basis_state(g, x):
    return tn.TensorNetworkState(g, {v: np.eye(2, dtype=np.complex64)[int(xv)].reshape((2,) + (1,) * g.degree(v)) for v, xv in zip(g.vertices, x)})


def inner_loop(psi, xs):
    kw = dict(maxiter=SWEEPS)
    return [tn.log_inner(psi, basis_state(psi.graph, x), cache_update_kwargs=kw) for x in xs]


def lattice(n, repeats):
    psi = device_state(n, 32, 1234)
    rng = np.random.default_rng(7)
    out = dict(lattice=f"{n}x{n}", chi=32, sweeps=SWEEPS, repeats=repeats)
    for B in (1, 64, 1024):
        xs = rng.integers(0, 2, size=(B, psi.graph.nv())).astype(np.int32)
        t, spread = timed(lambda: tn.log_amplitudes(psi, xs, cache_update_kwargs=dict(maxiter=SWEEPS)), repeats)
        out[f"amplitudes_B{B}_ms"], out[f"amplitudes_B{B}_spread_ms"], out[f"amplitudes_B{B}_ms_per_string"] = 1e3 * t, 1e3 * spread, 1e3 * t / B
        if B == 64:
            tl, sl = timed(lambda: inner_loop(psi, xs), max(1, repeats // 2))
            out["inner_loop_B64_ms"], out["inner_loop_B64_spread_ms"] = 1e3 * tl, 1e3 * sl
            out["loop_over_call_B64"] = tl / t
    return out


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    if len(sys.argv) > 2 and sys.argv[2] == "once":
        B = int(sys.argv[3])
        psi = device_state(n, 32, 1234)
        xs = np.random.default_rng(7).integers(0, 2, size=(B, psi.graph.nv())).astype(np.int32)
        for _ in range(2):
            tn.log_amplitudes(psi, xs, cache_update_kwargs=dict(maxiter=SWEEPS))
        print(json.dumps(dict(lattice=f"{n}x{n}", B=B, calls=2)), flush=True)
    else:
        repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
        print(json.dumps(lattice(n, repeats)), flush=True)
