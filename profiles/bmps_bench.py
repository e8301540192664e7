"""Time of expect(psi, obs; alg = "boundarymps") (tnqs_expect_bmps) on states generated on the device as bench.py generates them (tnqs_set_site_random): <Z> on every
vertex of the middle row and <ZZ> on its neighbouring pairs (L + L - 1 observables, one device call), partition_by = "row", the default fitting options (niters = 50,
default_tolerance of the element type).  The state is taken through gauge_and_scale first (BP with maxiter = 40, rescale, symmetric gauge: the tolerance of the fit is absolute, and
the raw benchmark state's norms are far below it), outside the timing; the cache is then handed over as it stands (no upload).  A call is timed on the host clock (it ends in a stream
synchronise; median of the repeats after a warm-up call, profiler off); reported per configuration: ms per call, the sweeps of every fitted message, and -- with
`ref` as last argument -- the seconds tests/bmps_ref.py takes for the same request on the host's CPUs (tensors read back from the handle).
The share of the time spent in the contraction kernel, the QR kernel and the rest is read off a kernel trace of the same command:
    rocprofv3 --kernel-trace --stats -- python profiles/bmps_bench.py 7 4 16 c64 1
    python profiles/bmps_bench.py [n] [chi] [R] [c64 | c128] [repeats] [ref]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import tnqs_amd as tn


def device_state(n, chi, seed, dtype, d=2):
    g = tn.named_grid((n, n))
    bpc = tn.BeliefPropagationCache(tn.tensornetworkstate(dtype, lambda v: "↑", g))
    for v in g.vertices:
        z = g.degree(v)
        bpc._set_random(v, [chi] * z, seed, scale=1.0 / np.sqrt(d * float(chi) ** z))
    return bpc


def middle_row_observables(n):
    r = (n + 1) // 2
    return [("Z", [(r, c)]) for c in range(1, n + 1)] + [("ZZ", [(r, c), (r, c + 1)]) for c in range(1, n)]


def timed(fn, repeats):
    fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def configuration(n, chi, R, dtype, repeats, with_ref):
    bpc = tn.symmetrize_and_normalize(tn.update(device_state(n, chi, 1234, dtype), maxiter=40))      # what gauge_state = True does to a TensorNetworkState, outside the timing
    obs, info = middle_row_observables(n), {}
    call = lambda: tn.expect(bpc, obs, alg="boundarymps", mps_bond_dimension=R, partition_by="row", info=info)
    out = dict(lattice=f"{n}x{n}", chi=chi, R=R, dtype=np.dtype(dtype).name, observables=len(obs), repeats=repeats, call_ms=1e3 * timed(call, repeats))
    out["fit_sweeps"] = [int(s) for s in info["fit_sweeps"]]
    if with_ref:
        import bmps_ref
        g = bpc.graph
        tensors = {v: bpc.tensor(v).astype(np.complex128) for v in g.vertices}
        t0 = time.perf_counter()
        b = bmps_ref.BoundaryMPS(g, tensors, R, partition_by="row", tolerance=tn.default_tolerance(dtype))
        vals = [b.expect(vs, [tn.gate_matrix(c) for c in op]) for op, vs in obs]
        out["bmps_ref_cpu_s"] = time.perf_counter() - t0
        out["max_abs_diff_to_ref"] = float(np.max(np.abs(np.asarray(vals) - np.asarray(call()))))
    return out


if __name__ == "__main__":
    a = sys.argv[1:]
    n, chi, R = (int(a[0]) if len(a) > 0 else 7), (int(a[1]) if len(a) > 1 else 4), (int(a[2]) if len(a) > 2 else 16)
    dtype = np.complex128 if len(a) > 3 and a[3] == "c128" else np.complex64
    print(json.dumps(configuration(n, chi, R, dtype, int(a[4]) if len(a) > 4 else 3, len(a) > 5 and a[5] == "ref")), flush=True)
