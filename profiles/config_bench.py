"""Two-loop configurations of the loop corrections on the device (tnqs_config_weights), ComplexF32 states generated on the device as
bench.py generates them (tnqs_set_site_random).
  theta CHI [repeats]     the theta of a 2 x 3 grid (two plaquettes sharing an edge): seconds per configuration_weights call (median after one warm-up call), the
                          TNQS_PROF_LOOP kernel time and GEMM rate of one call (8 m n k flops per product over the class time: a LOWER bound, the class also holds
                          the Grams' stores, permutes, antiprojectors and the dot), device memory in use after the call (the pool keeps its peak)
  norm N CHI [repeats]    norm_sqr(bpc, "loopcorrections", 7, branched = "device") on the N x N grid: plaquettes, 2 x 1 rectangles and thetas
  compare CHI [repeats]   3 x 3 grid: loopcorrected_partitionfunction(bpc, 7) with branched = "host" (the thetas contracted by numpy on the host) against
                          branched = "device" on the same handle; both times and the relative difference of the two results
    python profiles/config_bench.py theta 32"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
import tnqs_amd as tn


def device_state(shape, chi, d=2):
    g = tn.named_grid(shape)
    bpc = tn.BeliefPropagationCache(tn.tensornetworkstate(np.complex64, lambda v: "↑", g))
    for v in g.vertices:
        z = g.degree(v)
        bpc._set_random(v, [chi] * z, 1234, scale=1.0 / np.sqrt(d * float(chi) ** z))
    return tn.update(bpc, maxiter=10, tolerance=None)


def timed(fn, repeats):
    t0 = time.perf_counter(); out = fn(); warm = time.perf_counter() - t0
    secs = []
    for _ in range(repeats):
        t0 = time.perf_counter(); out = fn(); secs.append(time.perf_counter() - t0)
    return out, warm, secs


def theta(chi, repeats):
    r = tn.rescale(device_state((2, 3), chi))
    cfg = [[tuple(e) for e in r.graph.edges]]
    w, warm, secs = timed(lambda: tn.configuration_weights(r, cfg), repeats)
    tn.profile_enable(r, True); tn.profile_reset(r)
    tn.configuration_weights(r, cfg)
    p = tn.profile_get(r)["loop"]
    free, total = torch.cuda.mem_get_info()
    return dict(what="theta 2x3", chi=chi, seconds_per_call_median=float(np.median(secs)), seconds_all=secs, seconds_first_call=warm, prof_loop_ms=p["ms"],
                prof_loop_launches=p["launches"], flops=p["flops"], tflops_lower_bound=p["flops"] / (p["ms"] * 1e-3) / 1e12 if p["ms"] > 0 else None,
                device_bytes_in_use_after_call=int(total - free), abs_w=abs(w[0]))


def norm(n, chi, repeats):
    bpc = device_state((n, n), chi)
    sizes = [len(c) for c in tn.leafless_edge_induced_subgraphs(bpc.graph, 7)]
    z, warm, secs = timed(lambda: tn.norm_sqr(bpc, "loopcorrections", 7, branched="device"), repeats)
    return dict(what=f"norm_sqr {n}x{n} max 7 branched=device", chi=chi, configurations={k: sizes.count(k) for k in sorted(set(sizes))},
                seconds_per_call_median=float(np.median(secs)), seconds_all=secs, seconds_first_call=warm, z_over_zbp=abs(z / tn.partitionfunction(bpc)))


def compare(chi, repeats):
    bpc = tn.update(tn.BeliefPropagationCache(tn.random_tensornetworkstate(np.complex64, tn.named_grid((3, 3)), chi, seed=1)), maxiter=100, tolerance=None)
    zd, wd, sd = timed(lambda: tn.loopcorrected_partitionfunction(bpc, 7, branched="device"), repeats)
    zh, wh, sh = timed(lambda: tn.loopcorrected_partitionfunction(bpc, 7, branched="host"), repeats)
    return dict(what="3x3 max 7: host route against device call", chi=chi, device_seconds_median=float(np.median(sd)), device_seconds_all=sd, host_seconds_median=float(np.median(sh)),
                host_seconds_all=sh, relative_difference=abs(zd - zh) / abs(zh))


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "theta"
    args = [int(a) for a in sys.argv[2:]]
    if what == "theta":
        res = theta(args[0] if args else 16, args[1] if len(args) > 1 else 3)
    elif what == "norm":
        res = norm(args[0], args[1], args[2] if len(args) > 2 else 1)
    else:
        res = compare(args[0] if args else 8, args[1] if len(args) > 1 else 3)
    print(json.dumps(res), flush=True)
