"""Sampling (sample, alg = "bp") on evolved ComplexF32 states: heavy-hex (5,5) chi = 16 and 7x7 chi = 32.  Per lattice: ms per sample of tnqs_sample_bp,
ms per sample of the host loop over the public primitives (tnqs_copy, tnqs_site_probabilities, host draw, tnqs_project_site, tnqs_bp_update), and ms per
tnqs_bp_update (two sweeps, no tolerance) on the unprojected, the half-projected and the fully projected network.   python profiles/sample_bench.py [hh|grid]"""
import ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import tnqs_amd as tn
L = tn.core.L


def evolved(g, chi):
    groups = tn.edge_color(g)
    layer = [("Rx", [v], 0.5) for v in g.vertices] + [("Rz", [v], 0.4) for v in g.vertices]
    for grp in groups:
        layer += [("Rzz", [a, b], 0.25) for (a, b) in grp]
    bpc = tn.update(tn.BeliefPropagationCache(tn.tensornetworkstate(np.complex64, lambda v: "↑", g)))
    for _ in range(10):                                                            # until every bond that can reach chi has
        bpc, _ = tn.apply_gates(layer, bpc, apply_kwargs=dict(maxdim=chi, cutoff=1e-12))
        if min(bpc.bond_dim(a, b) for (a, b) in g.edges) >= chi:
            break
    bpc, _ = tn.apply_gates(layer, bpc, apply_kwargs=dict(maxdim=chi, cutoff=1e-12))
    return tn.symmetrize_and_normalize(tn.update(bpc))


def draw(p, u):
    hit = np.nonzero(u < np.cumsum(p))[0]
    return int(hit[0]) if len(hit) else len(p) - 1


def fused(bpc, u, bo):
    cfg = np.zeros(u.shape, dtype=np.int32); prob = np.zeros(u.shape)
    L.check(L.lib.tnqs_sample_bp(bpc._h, len(u), C.byref(bo), C.c_uint64(0), u.ctypes.data_as(C.POINTER(C.c_double)), cfg.ctypes.data_as(C.POINTER(C.c_int32)),
                                 prob.ctypes.data_as(C.POINTER(C.c_double)), None))
    return cfg, prob


def host_loop(bpc, u, bo):
    nv = bpc.graph.nv(); vs = list(bpc.graph.vertices)
    cfg = np.zeros(u.shape, dtype=np.int32); prob = np.zeros(u.shape)
    for j in range(len(u)):
        c = bpc.copy()
        for i in range(nv):
            p = tn.site_probabilities(c, vs[i]); x = draw(p, u[j, i]); cfg[j, i], prob[j, i] = x, p[x]
            L.check(L.lib.tnqs_project_site(c._h, i, x))
            if i + 1 < nv:
                L.check(L.lib.tnqs_bp_update(c._h, C.byref(bo), None, None))
    return cfg, prob


def ms_per_update(bpc, reps=5):
    bo, keep = tn.core._bp_opts(bpc.graph, dict(maxiter=2, tolerance=None))
    c = bpc.copy()
    L.check(L.lib.tnqs_bp_update(c._h, C.byref(bo), None, None))
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); L.check(L.lib.tnqs_bp_update(c._h, C.byref(bo), None, None)); ts.append(time.perf_counter() - t0)
    return round(1e3 * float(np.median(ts)), 3)


def run(name, g, chi, nsamples):
    bpc = evolved(g, chi)
    bo, keep = tn.core._bp_opts(g, bpc.default_bp_update_kwargs())
    u = np.random.default_rng(3).random((nsamples, g.nv()))
    out = dict(lattice=name, nv=g.nv(), chi=chi, nsamples=nsamples)
    fused(bpc, u[:1], bo); host_loop(bpc, u[:1], bo)                              # warm-up
    fs, hs = [], []
    for _ in range(3):                                                             # alternate: spread from run to run
        t0 = time.perf_counter(); fc, fp = fused(bpc, u, bo); fs.append((time.perf_counter() - t0) * 1e3 / nsamples)
        t0 = time.perf_counter(); hc, hp = host_loop(bpc, u, bo); hs.append((time.perf_counter() - t0) * 1e3 / nsamples)
    out["identical"] = bool(np.array_equal(fc, hc) and np.array_equal(fp, hp))
    out["fused_ms_per_sample"] = [round(x, 2) for x in fs]; out["host_loop_ms_per_sample"] = [round(x, 2) for x in hs]
    half = bpc.copy(); full = bpc.copy()
    for i, v in enumerate(g.vertices):
        if i % 2 == 0:
            L.check(L.lib.tnqs_project_site(half._h, i, 0))
        L.check(L.lib.tnqs_project_site(full._h, i, 0))
    out["bp_update_ms"] = dict(unprojected=ms_per_update(bpc), half_projected=ms_per_update(half), fully_projected=ms_per_update(full))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    if which in ("hh", "all"):
        run("heavy_hex(5,5)", tn.heavy_hexagonal_lattice(5, 5), 16, 4)
    if which in ("grid", "all"):
        run("grid7x7", tn.named_grid((7, 7)), 32, 2)
