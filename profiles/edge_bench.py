"""<Z_u Z_v> on every bond of a square lattice, two ways on the SAME handle: expect_edges(bpc, "ZZ") (one tnqs_rdm_edges call) and the loop of
expect(bpc, ("ZZ", [u, v])) calls (tnqs_expect_region: two region contractions per bond, each with its own launches, upload and blocking read-back).
ComplexF32 states generated on the device as bench.py generates them (tnqs_set_site_random), 7x7 and 20x20 at chi = 32.  Per lattice: wall seconds of
both (host clock around calls that end in a stream synchronise; median of the repeats after a warm-up call each, profiler off), their ratio, the largest
difference between the two results, and -- from one more batched call with the profiler on -- the time of the classes "edge_rdm" (the bond-contraction
kernel) and "small" (its chains and Grams) with the algorithmic flops booked there.
    python profiles/edge_bench.py [7 | 20] [chi] [repeats] [loop_repeats]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import tnqs_amd as tn


def device_state(n, chi, d=2):
    g = tn.named_grid((n, n))
    bpc = tn.BeliefPropagationCache(tn.tensornetworkstate(np.complex64, lambda v: "↑", g))
    for v in g.vertices:
        z = g.degree(v)
        bpc._set_random(v, [chi] * z, 1234, scale=1.0 / np.sqrt(d * float(chi) ** z))
    return tn.update(bpc, maxiter=10, tolerance=None)


def lattice(n, chi, repeats, loop_repeats):
    bpc = device_state(n, chi)
    edges = list(bpc.graph.edges)
    tn.expect_edges(bpc, "ZZ")                                               # warm-up: code objects, pool
    batched = []
    for _ in range(repeats):
        t0 = time.perf_counter(); zz = tn.expect_edges(bpc, "ZZ"); batched.append(time.perf_counter() - t0)
    for e in edges[:4]:
        tn.expect(bpc, ("ZZ", list(e)))
    loop = []
    for _ in range(loop_repeats):
        t0 = time.perf_counter(); ref = np.array([tn.expect(bpc, ("ZZ", list(e))) for e in edges]); loop.append(time.perf_counter() - t0)
    tn.profile_enable(bpc, True); tn.profile_reset(bpc)
    t0 = time.perf_counter(); tn.expect_edges(bpc, "ZZ"); prof_call = time.perf_counter() - t0
    p = tn.profile_get(bpc)
    tn.profile_enable(bpc, False)
    tb, tl = float(np.median(batched)), float(np.median(loop))
    return dict(lattice=f"{n}x{n}", chi=chi, bonds=len(edges), expect_edges_seconds_median=tb, expect_edges_seconds_all=batched,
                expect_loop_seconds_median=tl, expect_loop_seconds_all=loop, loop_over_batched=tl / tb, max_abs_diff=float(np.max(np.abs(zz - ref))),
                profiled_call_seconds=prof_call, prof_edge_rdm_ms=p["edge_rdm"]["ms"], prof_edge_rdm_launches=p["edge_rdm"]["launches"],
                prof_edge_rdm_bytes=p["edge_rdm"]["bytes"], prof_small_ms=p["small"]["ms"], prof_small_launches=p["small"]["launches"],
                prof_small_flops=p["small"]["flops"], prof_small_bytes=p["small"]["bytes"],
                small_tflops=p["small"]["flops"] / (p["small"]["ms"] * 1e-3) / 1e12 if p["small"]["ms"] > 0 else None)


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    chi = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    loop_repeats = int(sys.argv[4]) if len(sys.argv) > 4 else (3 if n <= 7 else 1)
    print(json.dumps(lattice(n, chi, repeats, loop_repeats)), flush=True)
