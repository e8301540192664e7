"""Loop corrections (loopcorrected_partitionfunction(bpc, 4): every plaquette of a square lattice) on ComplexF32 states generated on the device as bench.py
generates them (tnqs_set_site_random), 7x7 and 20x20 at chi = 32.  Per lattice: seconds per call (median of the repeats after one warm-up call), the
TNQS_PROF_LOOP kernel time of one call, and the algorithmic rate of the batched complex GEMM, 8 m n k flops per product, over that class time -- a LOWER
bound on the GEMM's own rate: the class also holds the message absorption, the permutes, the antiprojector and the trace.
`compare`: the four plaquette weights of a 3x3 chi = 8 grid three ways -- the device path, tests/loop_ref.py on the tensors read back, and
tnqs_expect_region with identity operators on one plaquette (chi^2 tree contractions of the un-projected loop).  A sanity ratio, no pass mark.
    python profiles/loop_bench.py [7 | 20 | compare] [chi] [repeats]"""
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


def lattice(n, chi, repeats):
    bpc = device_state(n, chi)
    t0 = time.perf_counter(); z = tn.loopcorrected_partitionfunction(bpc, 4); warm = time.perf_counter() - t0
    secs = []
    for _ in range(repeats):
        t0 = time.perf_counter(); z = tn.loopcorrected_partitionfunction(bpc, 4); secs.append(time.perf_counter() - t0)
    r = tn.rescale(bpc)
    rings = [tn.core._cycle_order(list(c)) for c in tn.leafless_edge_induced_subgraphs(bpc.graph, 4)]
    tn.loop_weights(r, rings[:1])
    tn.profile_enable(r, True); tn.profile_reset(r)
    t0 = time.perf_counter(); w = tn.loop_weights(r, rings); call = time.perf_counter() - t0
    p = tn.profile_get(r)["loop"]
    return dict(lattice=f"{n}x{n}", chi=chi, plaquettes=len(rings), seconds_per_call_median=float(np.median(secs)), seconds_all=secs, seconds_first_call=warm,
                loop_weights_seconds=call, prof_loop_ms=p["ms"], prof_loop_launches=p["launches"], cgemm_flops=p["flops"],
                cgemm_tflops_lower_bound=p["flops"] / (p["ms"] * 1e-3) / 1e12 if p["ms"] > 0 else None, one_plus_sum_w=abs(1 + np.sum(w)), sum_w=abs(np.sum(w)), z=abs(z))      # (Z_bp = exp(free energy) itself underflows on 400 random sites)


def compare(chi, repeats):
    import loop_ref as lr
    g = tn.named_grid((3, 3))
    r = tn.rescale(tn.update(tn.BeliefPropagationCache(tn.random_tensornetworkstate(np.complex64, g, chi, seed=1)), maxiter=100, tolerance=None))
    rings = [tn.core._cycle_order(list(c)) for c in tn.leafless_edge_induced_subgraphs(g, 4)]
    tn.loop_weights(r, rings)
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter(); w = tn.loop_weights(r, rings); t.append(time.perf_counter() - t0)
    ts = {v: r.tensor(v).astype(np.complex128) for v in g.vertices}
    ms = {e: r.message(e).astype(np.complex128) for (a, b) in g.edges for e in ((a, b), (b, a))}
    rg = lr.RefGraph(g.vertices, g.edges)
    t0 = time.perf_counter(); wr = [lr.cycle_weight(lr.cycle_matrices(ts, ms, rg, ring)) for ring in rings]; tref = time.perf_counter() - t0
    ident = [np.eye(2)] * 4
    tn.expect(r, (ident, rings[0]))
    t0 = time.perf_counter(); tn.expect(r, (ident, rings[0])); treg = time.perf_counter() - t0
    return dict(lattice="3x3", chi=chi, device_four_weights_s=float(np.median(t)), loop_ref_four_weights_s=tref, expect_region_one_plaquette_s=treg,
                max_abs_diff=float(np.max(np.abs(np.asarray(wr) - w))))


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "7"
    chi = int(sys.argv[2]) if len(sys.argv) > 2 else (8 if what == "compare" else 32)
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    print(json.dumps(compare(chi, repeats) if what == "compare" else lattice(int(what), chi, repeats)), flush=True)
