"""BP updates (two sweeps, no tolerance) on a random 7x7 chi = 32 ComplexF32 network, unprojected or with every site projected (site dimension 1), for a
per-kernel trace:   rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python profiles/projected_bp_trace.py [unprojected|projected]"""
import ctypes as C, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import tnqs_amd as tn
L = tn.core.L
mode = sys.argv[1] if len(sys.argv) > 1 else "unprojected"
g = tn.named_grid((7, 7)); chi = 32
bpc = tn.BeliefPropagationCache(tn.tensornetworkstate(np.complex64, lambda v: "↑", g))
for i, v in enumerate(g.vertices):
    n = 2 * chi ** g.degree(v)
    bpc._set_random(v, [chi] * g.degree(v), seed=7 + i, scale=1.0 / np.sqrt(n))
if mode == "projected":
    for i in range(g.nv()):
        L.check(L.lib.tnqs_project_site(bpc._h, i, 0))
bo, keep = tn.core._bp_opts(g, dict(maxiter=2, tolerance=None))
L.check(L.lib.tnqs_bp_update(bpc._h, C.byref(bo), None, None))
ts = []
for _ in range(10):
    t0 = time.perf_counter(); L.check(L.lib.tnqs_bp_update(bpc._h, C.byref(bo), None, None)); ts.append(time.perf_counter() - t0)
print(f"{mode}: median {1e3 * float(np.median(ts)):.3f} ms per update of two sweeps (11 updates in the trace)")
