"""<Z_u Z_w> of distant vertex pairs of a square lattice, two ways on the SAME handle: one tnqs_rdm_paths call (correlation_function / rdm_paths / expect_pairs) and
the loop of expect(bpc, ("ZZ", [u, w])) calls (tnqs_expect_region: one region contraction per pair and per numerator / denominator, each with its own launches,
upload and blocking read-back, the path rebuilt for every pair).  ComplexF32 states generated on the device as bench.py generates them (tnqs_set_site_random), chi = 32,
10 BP sweeps.  Workloads:
  a  correlation_function along the middle row of the lattice from its first vertex (n - 1 pairs, one path)
  b  rdm_paths for all rows and all columns from their first vertex (2 n paths, 2 n (n - 1) pairs)
  c  all pairs of the middle row: the n - 1 paths that start at each of its vertices and run to the row's end (n (n - 1) / 2 pairs given to expect_pairs, which lets
     the pairs of one source ride on that source's longest path)
Per workload: wall seconds of both ways (host clock around calls that end in a stream synchronise, profiler off, a warm-up call first; median of the repeats and all of
them), their ratio, the largest difference between the two results over the pairs the loop could answer (loop_pairs_failed: its f32 region contraction underflowed), and -- from one more call with the profiler on -- the time, launches and booked bytes of the classes
"small" (chains and Grams of the ends), "loop" (transfer matrices) and "path_rdm" (apply kernel and bond contractions), the apply kernel's bytes computed from the
shapes (T read + L read once per row block + L written) and those bytes over the class's time: a LOWER bound of path_apply's rate, since the class's time includes the
bond contractions.
"rescaled" as the last argument runs everything on rescale(bpc) (vertex and edge scalars 1), where the loop's f32 contractions do not underflow: the state on which the
two results can be compared at every distance.
    python profiles/path_bench.py [n] [chi] [workloads, e.g. abc] [repeats] [loop_repeats] [rescaled]"""
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


def apply_bytes(paths, chi, d=2, esz=8):
    """T read + L read + L written of every apply step at uniform chi (an upper bound on the L terms: 16 chunks, 4 row blocks at chi = 32)"""
    steps = sum(max(0, len(p) - 2) for p in paths)
    nrb = (chi * chi + 255) // 256
    return steps * (chi ** 4 * esz + (nrb + 1) * 16 * d * d * chi * chi * 16)


def loop_value(bpc, pr):
    """expect(bpc, ("ZZ", [u, w])) or NaN: on a ComplexF32 handle tnqs_expect_region contracts the region in f32, and on the un-rescaled random states of this benchmark
    the denominator of a long region underflows to zero (seen on the 20 x 20 lattice); the call is timed all the same, the pair is counted as failed"""
    try:
        return tn.expect(bpc, ("ZZ", list(pr)))
    except ZeroDivisionError:
        return complex(np.nan, np.nan)


def timed(fn, repeats):
    fn()                                                                     # warm-up: code objects, pool
    ts, val = [], None
    for _ in range(repeats):
        t0 = time.perf_counter(); val = fn(); ts.append(time.perf_counter() - t0)
    return val, ts


def workload(bpc, name, paths, one_call, repeats, loop_repeats, chi):
    pairs = [(p[0], w) for p in paths for w in p[1:]]
    got, tb = timed(one_call, repeats)
    for pr in pairs[:2]:
        tn.expect(bpc, ("ZZ", list(pr)))
    tl, ref = [], None
    for _ in range(loop_repeats):
        t0 = time.perf_counter(); ref = np.array([loop_value(bpc, pr) for pr in pairs]); tl.append(time.perf_counter() - t0)
    tn.profile_enable(bpc, True); tn.profile_reset(bpc)
    t0 = time.perf_counter(); one_call(); prof_call = time.perf_counter() - t0
    p = tn.profile_get(bpc)
    tn.profile_enable(bpc, False)
    ab = apply_bytes(paths, chi)
    ok = np.isfinite(ref) if tl else None
    out = dict(workload=name, paths=len(paths), pairs=len(pairs), one_call_seconds_median=float(np.median(tb)), one_call_seconds_all=tb,
               expect_loop_seconds_median=float(np.median(tl)) if tl else None, expect_loop_seconds_all=tl,
               loop_over_one_call=float(np.median(tl) / np.median(tb)) if tl else None,
               loop_pairs_failed=int(np.sum(~ok)) if tl else None, one_call_all_finite=bool(np.all(np.isfinite(np.asarray(got)))),
               max_abs_diff=float(np.max(np.abs(np.asarray(got).ravel()[ok] - ref[ok]))) if tl and ok.any() else None, profiled_call_seconds=prof_call,
               apply_bytes_from_shapes=ab, apply_bytes_per_second_lower_bound=ab / (p["path_rdm"]["ms"] * 1e-3) if p["path_rdm"]["ms"] > 0 else None)
    for cls in ("small", "loop", "path_rdm"):
        out[f"prof_{cls}"] = {k: p[cls][k] for k in ("ms", "launches", "bytes", "flops")}
    return out


def lattice(n, chi, which, repeats, loop_repeats, rescaled=False):
    bpc = device_state(n, chi)
    if rescaled:
        bpc = tn.rescale(bpc)                                                # every vertex and edge scalar 1: the loop's f32 region contractions stay in range
    mid = (n + 1) // 2
    row = [(i, mid) for i in range(1, n + 1)]
    res = dict(lattice=f"{n}x{n}", chi=chi, rescaled=rescaled, workloads=[])
    if "a" in which:
        res["workloads"].append(workload(bpc, "a", [row], lambda: tn.correlation_function(bpc, "ZZ", row), repeats, loop_repeats, chi))
    if "b" in which:
        lines = [[(i, j) for i in range(1, n + 1)] for j in range(1, n + 1)] + [[(i, j) for j in range(1, n + 1)] for i in range(1, n + 1)]
        zz = np.kron(tn.gate_matrix("Z"), tn.gate_matrix("Z"))
        res["workloads"].append(workload(bpc, "b", lines, lambda: np.array([np.sum(zz * m.T) for dct in tn.rdm_paths(bpc, lines) for m in dct.values()]),
                                         repeats, loop_repeats, chi))
    if "c" in which:
        tails = [row[i:] for i in range(n - 1)]
        pairs = [(p[0], w) for p in tails for w in p[1:]]
        res["workloads"].append(workload(bpc, "c", tails, lambda: tn.expect_pairs(bpc, "ZZ", pairs), repeats, loop_repeats, chi))
    return res


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    chi = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    which = sys.argv[3] if len(sys.argv) > 3 else "abc"
    repeats = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    loop_repeats = int(sys.argv[5]) if len(sys.argv) > 5 else (3 if n <= 7 else 1)
    rescaled = len(sys.argv) > 6 and sys.argv[6] == "rescaled"
    print(json.dumps(lattice(n, chi, which, repeats, loop_repeats, rescaled)), flush=True)
