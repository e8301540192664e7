#!/usr/bin/env python
"""bench.py -- two-site gates/sec at fixed chi on an L x L square-lattice TFIM Trotter layer (BASELINE.json metric).

One "step" = one `apply_gates(layer, psi_bpc; apply_kwargs)` call on the named workload, INCLUDING the c+1 BP
updates it triggers -- exactly what examples/2dIsing_dynamics.jl:56-57 times.  Workload at N=1: configs[1] of
BASELINE.json (20x20 TFIM, chi=32, ComplexF32, batched edge-colour apply on one MI355X).  The state is synthetic
(iid complex-normal site tensors at bond dimension chi) and resident in HBM before the timed region.

Prints ONE JSON line (rank 0).  Extra objects: "roofline" for the dominant kernel class (HIP-event timed inside the
library on its own stream).  With --full also "cpu_baseline" (oracle/cpu_port.cpp: the compiled CPU restatement of the same path, timed
on the host cores on a bounded sample, next to the host's measured BLAS rates) and, for the headline configuration, the same command
with the f32 matrix instructions and with the reference's sweep order, each in a child process; a plain run only sets up, warms up,
times the steps and prints the line.  With --gpus N the lattice is sharded by vertex over N ranks and every exchange is an
ncclAllGather the library enqueues on its own stream (RCCL inside the library, tnqs_set_sharding_rccl).

--dump-outputs DIR (one GPU) writes what the last timed step returned -- the truncation errors, a fixed seeded sample of the site
tensors and of the BP messages -- as DIR/<name>.npy (complex values as a trailing (real, imag) axis), so that two builds run with the
same arguments can be compared output for output.
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np


def tfim_layer(tn, g, groups, J=1.0, hx=2.5, dt=0.01):
    """README.md:42-48 circuit: Rx(2 hx dt) on every vertex, Rzz(2 J dt) per edge colour"""
    layer = [("Rx", (v,), 2 * hx * dt) for v in g.vertices]      # (vertex TUPLES: the host keeps the marshalled arrays of an immutable circuit)
    for grp in groups:
        layer += [("Rzz", (a, b), 2 * J * dt) for (a, b) in grp]
    return layer


def random_state_tensors(g, chi, d, seed, dtype, wanted=None, threads=1):
    """iid complex-normal site tensors at bond dimension chi; one counter-based stream per vertex (seed, vertex position), so that a
    rank of a sharded run only generates its own tensors.  Yields (v, tensor) for wanted vertices and (v, shape) for the others, in
    vertex order.  `threads` vertices are generated at a time (numpy's generators release the GIL); the values do not depend on it."""
    def make(i, shp):
        n = int(np.prod(shp))
        rng = np.random.default_rng([seed, i])
        t = rng.standard_normal(2 * n, dtype=np.float32).view(np.complex64).reshape(shp)
        t *= np.float32(1.0 / np.sqrt(n))                       # unit Frobenius norm (f32-friendly scale)
        return t.astype(dtype, copy=False)

    items = [(i, v, (d,) + (chi,) * g.degree(v)) for i, v in enumerate(g.vertices)]
    chunk = 2 * max(1, threads)                                 # (bounds the host memory held at once)
    with ThreadPoolExecutor(max_workers=max(1, threads)) as pool:
        for k in range(0, len(items), chunk):
            part = items[k:k + chunk]
            futs = [None if (wanted is not None and not wanted(v)) else pool.submit(make, i, shp) for i, v, shp in part]
            for (i, v, shp), f in zip(part, futs):
                yield v, (shp if f is None else f.result())


def host_threads():
    """CPUs this process may use for host-side set-up, at most 16 (more only contend with the rest of the host)"""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(16, n))


DUMP_SEED = 20240601
DUMP_MAX_VERTICES, DUMP_MAX_ELEMENTS, DUMP_MAX_EDGES = 32, 65536, 512


def _real_view(a):
    """complex -> trailing (real, imag) axis; float32 for single, float64 for double precision"""
    a = np.asarray(a)
    ft = np.float32 if a.dtype in (np.complex64, np.float32) else np.float64
    if np.iscomplexobj(a):
        return np.stack([a.real, a.imag], axis=-1).astype(ft, copy=False)
    return a.astype(ft, copy=False)


def dump_outputs(path, bpc, g, errs):
    """what a caller of apply_gates received from the last timed step, on a fixed sample: the truncation errors of every gate, up to
    DUMP_MAX_VERTICES site tensors (positions drawn with DUMP_SEED) with up to DUMP_MAX_ELEMENTS entries each (flat C-order positions
    drawn from the stream (DUMP_SEED, vertex position)), and up to DUMP_MAX_EDGES BP messages (directed edges in the order of g.edges,
    each edge followed by its reverse, drawn with DUMP_SEED).  The sample depends only on the lattice and the shapes."""
    os.makedirs(path, exist_ok=True)
    verts = list(g.vertices)
    rng = np.random.default_rng(DUMP_SEED)
    pos = np.arange(len(verts)) if len(verts) <= DUMP_MAX_VERTICES else np.sort(rng.choice(len(verts), DUMP_MAX_VERTICES, replace=False))
    parts = []
    for i in pos:
        t = bpc.tensor(verts[i]).reshape(-1)
        if t.size > DUMP_MAX_ELEMENTS:
            t = t[np.sort(np.random.default_rng([DUMP_SEED, int(i)]).choice(t.size, DUMP_MAX_ELEMENTS, replace=False))]
        parts.append(t)
    directed = [e for (a, b) in g.edges for e in ((a, b), (b, a))]
    epos = np.arange(len(directed)) if len(directed) <= DUMP_MAX_EDGES else np.sort(rng.choice(len(directed), DUMP_MAX_EDGES, replace=False))
    msgs = [bpc.message(directed[k]).reshape(-1) for k in epos]
    out = {"truncation_errors": np.asarray(errs, dtype=np.float64),
           "site_tensor_sample": _real_view(np.concatenate(parts)),
           "message_sample": _real_view(np.concatenate(msgs))}
    total = sum(a.nbytes for a in out.values())
    if total > 64e6:
        raise SystemExit(f"bench.py: --dump-outputs would write {total / 1e6:.1f} MB (limit 64 MB)")
    for name, a in out.items():
        np.save(os.path.join(path, name + ".npy"), a)


def cpu_baseline(chi, L, seed=1234):
    """COMPILED CPU restatement of the reference path (oracle/cpu_port.cpp, round 6: C++ / OpenMP over scipy's OpenBLAS -- mode products as GEMMs on views, thin
    Householder QR in row blocks, cgesdd, f64 Hermitian eigen; pinned against the numpy oracle in tests/test_cpu_port.py) on a bounded sample of the benchmark
    workload: ONE TFIM layer of the benchmark's own L x L OPEN lattice at the same chi / dtype, reference-default BP kwargs, on every core this container may use
    (cpu_port.cpu_budget: the GPU boxes run under a cgroup quota of 16 CPUs of the 2 x 64-core host) -- the messages of a BP dependency level and the gates of a colour
    group on an OpenMP team, one BLAS thread per call.  Next to it: the host's BLAS rates on a square GEMM and on the workload's mode-product shape, same thread count
    (it is NOT the Julia package)."""
    import cpu_port
    import cpu_layer
    from concurrent.futures import ThreadPoolExecutor
    m = cpu_port.measure_host(chi=chi, L=L, periodic=False, seed=seed)
    with ThreadPoolExecutor(max_workers=m["threads_per_process"]) as pool:
        rates = cpu_layer._gemm_rates(chi, m["threads_per_process"], pool)
    host = "unknown CPU"
    try:
        with open("/proc/cpuinfo") as f:
            models = [ln.split(":", 1)[1].strip() for ln in f if ln.startswith("model name")]
        if models:
            host = f"{models[0]} ({len(models)} hardware threads" + (f", cgroup quota {m['cpu_quota']:g} CPUs)" if m.get("cpu_quota") else ")")
    except OSError:
        pass
    return {"value": m["gates_per_s"], "unit": "two-site gates/s", "cores": int(m["threads"]), "kind": "port", "compiled": True, "host": host,
            "processes": m["processes"], "threads_per_process": m["threads_per_process"], "per_process_gates_per_s": m["per_process_gates_per_s"],
            "algorithmic_gflops": m["algorithmic_gflops"], "host_square_cgemm_gflops_per_process": rates["square_cgemm_gflops"],
            "host_mode_product_shape_gflops_per_process": rates["mode_product_shape_gflops"],
            "frac_of_host_square_cgemm": round(m["algorithmic_gflops"] / (m["processes"] * rates["square_cgemm_gflops"]), 3),
            "frac_of_host_mode_product_shape": round(m["algorithmic_gflops"] / (m["processes"] * rates["mode_product_shape_gflops"]), 3),
            "bp_sweeps": m["bp_sweeps"], "thread_seconds_per_layer": m.get("thread_seconds_per_layer"), "wall_seconds_per_layer": m.get("wall_seconds_per_layer"),
            "sample": f"1 TFIM layer ({m['n_two_site']} two-site gates, {len(m['bp_sweeps'])} BP updates, sweeps {m['bp_sweeps']}) of the {L}x{L} open "
                      f"lattice ({m['sites']} sites) per process, {m['processes']} process(es) x {m['threads_per_process']} threads at the same time, chi={chi}, "
                      f"complex64, compiled C++ / OpenMP / OpenBLAS restatement of the reference path (oracle/cpu_port.cpp); {m['seconds_per_layer']:.1f} s per layer"}


def spawn_ranks(n):
    """`python bench.py --gpus N` with no launcher around it (the driver's command shape): re-run this script under torch.distributed.run
    with N ranks on this node, one per GPU (RCCL; TNQS_BENCH_BACKEND=gloo lets the ranks share one device -- a functional test of the
    launch path only).  Fails loudly when fewer than N devices are visible: a silent 1-rank run would print a wrong n_gpus."""
    import socket
    import subprocess
    import torch
    backend = os.environ.get("TNQS_BENCH_BACKEND", "nccl")
    ndev = torch.cuda.device_count()
    if backend == "nccl" and ndev < n:
        raise SystemExit(f"bench.py: --gpus {n} needs {n} visible GPUs (one rank per GPU over RCCL), found {ndev}")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    raise SystemExit(subprocess.run(cmd, env=env).returncode)


def profile_entry(db, kern):
    """the entry of a kernel in a counter-pass summary: rocprofv3 prints every template argument (`x3_pair_gram2_kernel<0, false>`), KERNEL_OF names the kernel as
    the sources call it (`x3_pair_gram2_kernel<0>`, defaults omitted)"""
    if not kern or not db:
        return {}
    if kern in db:
        return db[kern]
    stem = kern[:-1] if kern.endswith(">") else kern
    hits = [k for k in db if k.startswith(stem + ",") or k.startswith(stem + ">") or k == stem]
    return db[hits[0]] if len(hits) == 1 else {}


def profile_db(name):
    """counters of a committed profile of THIS command (profiles/<name>) with their provenance: the build id stored in the file against the
    build id of the tree this script runs from (profiles/buildid.py) -- the JSON line says when the two differ instead of quoting counters
    of another build silently"""
    try:
        sys.path.insert(0, os.path.join(ROOT, "profiles"))
        from buildid import build_id
        with open(os.path.join(ROOT, "profiles", name)) as f:
            doc = json.load(f)
        have, now = doc.get("build_id"), build_id()
        return doc["kernels"], {"file": "profiles/" + name, "profile_build_id": have, "this_build_id": now, "same_build": have == now}
    except Exception:
        return {}, None


def c1_circuit(mod):
    """BASELINE configs[0] = examples/2dIsing_dynamics.jl with the README quick-start numbers (README.md:36-53): 5 x 5 open grid, J = 1, hx = 2.5, dt = 0.01,
    Rx on every vertex then Rzz by edge colour; `mod` is the device package or the oracle (same constructors)"""
    g = mod.named_grid((5, 5))
    groups = mod.edge_color(g, 4)
    layer = [("Rx", [v], 2 * 2.5 * 0.01) for v in g.vertices]
    for grp in groups:
        layer += [("Rzz", [a, b], 2 * 1.0 * 0.01) for (a, b) in grp]
    return g, groups, layer


def main_c1(args, tn, torch):
    """BASELINE configs[0], the configuration the reference itself runs on a CPU: 5 x 5 TFIM, 50 Trotter layers from the product state, maxdim 10, ComplexF64,
    reference-default BP kwargs.  A step = one layer (what examples/2dIsing_dynamics.jl:56-57 times); the timed region is the whole 50-layer run on a fresh state
    (bonds grow 1 -> 10 on the way), after --warmup layers on a scratch copy that only load the kernels.  The CPU leg runs the SAME 50 layers through the parity
    oracle (oracle/tnqs_oracle.py: the reference's algorithm gate by gate, message by message -- numpy / LAPACK, one thread, like the reference's sequential
    Julia loop) on this box's host; 3 MB of state is far too small for a thread pool to pay (oracle/cpu_port.cpp is the many-core organisation, for c2)."""
    chi, dtype = 10, np.complex128
    g, groups, layer = c1_circuit(tn)
    kw = dict(maxdim=chi, cutoff=1e-10, normalize_tensors=True)
    scratch = tn.update(tn.BeliefPropagationCache(tn.tensornetworkstate(dtype, lambda v: "↑", g)))
    for _ in range(max(1, args.warmup)):
        scratch, _e = tn.apply_gates(layer, scratch, apply_kwargs=kw)
    del scratch
    bpc = tn.update(tn.BeliefPropagationCache(tn.tensornetworkstate(dtype, lambda v: "↑", g)))
    tn.profile_enable(bpc, os.environ.get("TNQS_BENCH_NOPROF") != "1"); tn.profile_reset(bpc)
    torch.cuda.synchronize()
    per_layer, sweeps, chis = [], [], []
    t0 = time.perf_counter()
    for _ in range(args.steps):
        t1 = time.perf_counter(); info = {}
        bpc, errs = tn.apply_gates(layer, bpc, apply_kwargs=kw, info=info)
        per_layer.append(1e3 * (time.perf_counter() - t1)); sweeps.append(info["n_sweeps"]); chis.append(int(bpc.maxvirtualdim()))
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    prof_all = tn.profile_get(bpc)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, bpc, g, errs)
    n2 = g.ne()
    sat = [t for t, c in zip(per_layer, chis) if c >= chi]
    out = {"metric": "two-site gates/sec at fixed chi (LxL TFIM Trotter layer)", "value": round(n2 * args.steps / elapsed, 2), "unit": "two-site gates/s", "n_gpus": 1,
           "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 3), "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
           "dtype": "c128 (ComplexF64)", "data": "synthetic (the example's own product state; no random numbers)",
           "config": {"workload": f"5x5 square-lattice TFIM, {args.steps} Trotter layers from the product state, chi=10, ComplexF64, apply_gates incl. BP updates; BASELINE.json configs[0]"
                                  + ("" if args.steps == 50 else f" with {args.steps} instead of 50 layers"),
                      "baseline_config": "c1", "two_site_gates_per_step": n2, "apply_kwargs": {"maxdim": chi, "cutoff": 1e-10, "normalize_tensors": True},
                      "bp_update_kwargs": "reference defaults (maxiter 25, tol 1e-8)", "bp_sweeps_per_step": sweeps, "max_bond_dim_per_step": chis,
                      "ms_per_layer": {"first": round(per_layer[0], 3), "last": round(per_layer[-1], 3), "mean_at_saturated_bonds": (round(float(np.mean(sat)), 3) if sat else None),
                                       "layers_at_saturated_bonds": len(sat)}},
           "roofline": {"bound": "latency", "note": "a 3 MB problem: no kernel of this run moves enough bytes or flops for either roof to mean anything (the largest tensor pass is 320 KB); what is "
                                                    "measured is the dependent chain of ~330 launches per layer, see kernel_classes and DESIGN.md section 7",
                        "achieved": None, "peak": None, "unit": None, "frac": None, "traffic": None},
           "kernel_classes": {k: {"ms": round(v["ms"], 2), "launches": v["launches"]} for k, v in prof_all.items() if v["launches"]}}
    if args.full and not args.no_cpu_baseline:
        try:
            import tnqs_oracle as o
            z_dev = tn.expect_all(bpc, "Z").real
            og, olayer = o.named_grid((5, 5)), layer          # the same gate list (same vertex labels, same colour order) on both sides
            ob = o.update(o.BeliefPropagationCache(o.product_state(dtype, lambda v: "↑", og)))
            t0 = time.perf_counter(); osw = []
            for _ in range(args.steps):
                inf = {}
                ob, _e = o.apply_gates(olayer, ob, apply_kwargs=kw, info=inf); osw.append(int(np.sum(inf.get("sweeps", [0]))))
            cpu_s = time.perf_counter() - t0
            zop = np.diag([1.0, -1.0]).astype(complex)
            z_cpu = np.array([o.expect_1site(ob, zop, v).real for v in og.vertices])
            host = "unknown CPU"
            try:
                with open("/proc/cpuinfo") as f:
                    models = [ln.split(":", 1)[1].strip() for ln in f if ln.startswith("model name")]
                if models:
                    host = f"{models[0]} ({len(models)} hardware threads)"
            except OSError:
                pass
            out["cpu_baseline"] = {"value": round(n2 * args.steps / cpu_s, 2), "unit": "two-site gates/s", "cores": 1, "kind": "port", "host": host,
                                   "ms_per_step": round(1e3 * cpu_s / args.steps, 3), "bp_sweeps_per_step": osw,
                                   "sample": f"the same {args.steps} layers of the same circuit from the same product state: the WHOLE workload, {cpu_s:.1f} s of CPU time, parity oracle "
                                             "(oracle/tnqs_oracle.py, numpy / LAPACK, sequential like the reference's loop, its own default edge sequence); it is NOT the Julia package",
                                   "device_over_cpu": round(cpu_s / elapsed, 2),
                                   "max_abs_dZ_device_vs_cpu_after_the_run": float(np.max(np.abs(z_dev - z_cpu))),
                                   "note": "the two sides sweep BP in different orders to the same tolerance (1e-8): <Z> agrees to that order, not to rounding"}
        except Exception as e:      # the baseline must never take the measured number down with it
            out["cpu_baseline"] = {"value": None, "error": repr(e)}
    print(json.dumps(out))


PEAK_F32_TFLOPS = 157.3      # MI355X_MICROARCH.md: FP32 matrix (= vector) peak
PEAK_BF16_TFLOPS = 2500.0    # MI355X_MICROARCH.md: dense bf16 matrix peak (v_mfma_f32_32x32x16_bf16)
PEAK_HBM_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed steps (default 3; --config c1: 50, the layers of configs[0])")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", choices=["c1", "c2", "c4", "c5"], default="c2",
                    help="BASELINE.json configuration: c2 = configs[1] (L x L TFIM, chi 32; the headline metric), c4 = configs[3] (L^3 periodic cubic 3-D Ising "
                         "layer, chi 16; full size L = 10 needs 8 GPUs), c5 = configs[4] (L x L TFIM, chi 64; full size L = 32 needs 8 GPUs), c1 = configs[0] (5 x 5 TFIM, "
                         "chi 10, ComplexF64, 50 layers from the product state: the reference's own CPU-runnable case, timed on the device; with --full also on the host's CPU oracle)")
    ap.add_argument("--L", type=int, default=0, help="lattice side (default: the BASELINE size of the configuration: 20 / 10 / 32)")
    ap.add_argument("--chi", type=int, default=0, help="bond dimension (default: 32 / 16 / 64)")
    ap.add_argument("--host-init", action="store_true", help="c4 / c5: generate the synthetic state with numpy on the host instead of on the device")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline number does not need: the CPU baseline and, for c2 on one GPU, the same command with the f32 matrix "
                         "instructions and with the reference's sweep order (child processes); --no-cpu-baseline / --no-ab / --no-ref-order drop single legs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one returned (truncation errors, a fixed seeded sample of the site tensors and BP "
                         "messages) as DIR/<name>.npy, float32 / float64; one GPU")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-ref-order", action="store_true", help="skip the third leg: the same command with --bp-order reference (the reference's own default sweep order, what a Julia caller of the shim gets) in a child process")
    ap.add_argument("--no-ab", action="store_true", help="skip the second, untimed-by-the-driver leg: the same command with TNQS_NO_BF16X3=1 (the f32 matrix instructions) in a child process")
    ap.add_argument("--bp-order", choices=["library", "reference"], default="library",
                    help="sweep order of the BP updates: the library default (linear forests, the order the plane kernels share products on) or the reference's "
                         "default forest_cover_edge_sequence (tnqs_bp_opts.n_sequence = -1).  Same fixed point; at the default tolerance both stop after one "
                         "sweep per update on different trajectories")
    ap.add_argument("--evolved", type=int, default=0, metavar="N",
                    help="also time the same lattice on a PHYSICALLY evolved state: N layers of the TFIM circuit at dt = 0.1 from the product state "
                         "(bonds saturate at chi), then --steps timed layers of that circuit; reported as the extra object \"evolved\"")
    args = ap.parse_args()
    if args.steps is None:
        args.steps = 50 if args.config == "c1" else 3
    if args.steps < 1:
        raise SystemExit("bench.py: --steps must be >= 1")
    if args.dump_outputs and args.gpus > 1:
        raise SystemExit("bench.py: --dump-outputs needs the whole state on one rank: --gpus 1")

    import torch
    import torch.distributed as dist
    if args.gpus < 1:
        raise SystemExit("bench.py: --gpus must be >= 1")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        return spawn_ranks(args.gpus)                     # `python bench.py --gpus N` without a launcher: become N ranks
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # one rank per GPU over RCCL; TNQS_BENCH_BACKEND=gloo lets several ranks share one GPU (functional test of this script only)
        local = local % max(1, torch.cuda.device_count())
        torch.cuda.set_device(local)
        dist.init_process_group(os.environ.get("TNQS_BENCH_BACKEND", "nccl"))
    import tnqs_amd as tn

    if args.config == "c1":
        if world > 1:
            raise SystemExit("bench.py: --config c1 is a 3 MB problem: one GPU")
        return main_c1(args, tn, torch)
    cfg = args.config
    L = args.L or {"c2": 20, "c4": 10, "c5": 32}[cfg]
    chi = args.chi or {"c2": 32, "c4": 16, "c5": 64}[cfg]
    d = 2
    dtype = np.complex64
    if cfg == "c4":       # examples/3dIsing_dynamics.jl:15-26: Rz(h dt) on every vertex, Rxx(2 J dt) per edge colour, Rz(h dt) again; h = J = -1, dt = 0.04
        g = tn.named_grid((L, L, L), periodic=True)
        groups = tn.edge_color(g)
        layer = [("Rz", (v,), -0.04) for v in g.vertices]
        for grp in groups:
            layer += [("Rxx", (a, b), -0.08) for (a, b) in grp]
        layer += [("Rz", (v,), -0.04) for v in g.vertices]
        zdeg = 6
        workload = (f"{L}x{L}x{L} periodic cubic lattice, 3-D Ising Trotter layer (Rz + {len(groups)} edge colours of Rxx + Rz; examples/3dIsing_dynamics.jl), chi={chi}, "
                    f"ComplexF32, apply_gates incl. BP updates; BASELINE.json configs[3]" + ("" if L == 10 else f" at L = {L} instead of 10"))
    else:
        g = tn.named_grid((L, L))
        groups = tn.edge_color(g, 4)
        layer = tfim_layer(tn, g, groups)
        zdeg = 4
        workload = (f"{L}x{L} square-lattice TFIM Trotter layer (Rx + 4 edge colours of Rzz), chi={chi}, ComplexF32, apply_gates incl. BP updates; "
                    + (("BASELINE.json configs[1]" + ("" if (L == 20 and chi == 32) else f" at L = {L}, chi = {chi} instead of 20, 32")) if cfg == "c2"
                       else "BASELINE.json configs[4]" + ("" if L == 32 else f" at L = {L} instead of 32")))
    n2 = g.ne()
    apply_kwargs = dict(maxdim=chi, cutoff=1e-10, normalize_tensors=True)
    # None = reference-default bp_update_kwargs with the library's sweep order; "reference": the same defaults (maxiter 25, tolerance 1e-5 for ComplexF32) with
    # the reference's own order
    bp_kwargs = None if args.bp_order == "library" else dict(maxiter=25, tolerance=1e-5, edge_sequence="forest_cover")

    # ---- state: bond dimension 1 handle, then upload the synthetic chi-saturated tensors ---------------------
    free_at_start = torch.cuda.mem_get_info(local if world > 1 else 0)[0]
    psi0 = tn.tensornetworkstate(dtype, lambda v: "↑", g)
    bpc = tn.BeliefPropagationCache(psi0, device=local if world > 1 else 0)
    transport_note = None
    if world > 1:
        from tnqs_amd import dist as tdist
        if dist.get_backend() == "nccl":
            # the library's own RCCL communicator; if it cannot be set up on EVERY rank (the ranks agree through torch's communicator), all of
            # them fall back to the callback transport (the same all-gathers through torch.distributed) and the JSON line says so
            ok, why = 1, ""
            try:
                tdist.shard(bpc, rank, world, transport="rccl", balance_chi=chi)
            except Exception as e:                                   # noqa: BLE001 -- any failure means "no in-library RCCL on this node"
                ok, why = 0, f"{type(e).__name__}: {e}"
            flag = torch.tensor([ok], device=f"cuda:{local}", dtype=torch.int32)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            if int(flag.item()) == 0:
                transport_note = "callback (in-library RCCL set-up failed on at least one rank" + (f": {why}" if why else "") + ")"
                bpc = tn.BeliefPropagationCache(psi0, device=local)
                tdist.shard(bpc, rank, world, transport="callback", balance_chi=chi)
        else:
            tdist.shard(bpc, rank, world, balance_chi=chi)
    # memory: a rank holds its own site tensors; a layer needs about four more copies of them at its peak (new tensors of a batch, the gauge
    # ping-pong buffers, BP partial products kept across levels, Gram partials; measured 4.4 - 5.1 x the site tensors, profiles/r5_bench_c4_L5.json,
    # r5_bench_c5_L11.json) -- refuse before allocating instead of dying in the middle of the upload
    own_bytes = sum(8 * d * chi ** g.degree(v) for v in g.vertices if (world == 1 or bpc.owns(v)))
    free_b, total_b = torch.cuda.mem_get_info(local if world > 1 else 0)
    mem = {"site_tensor_GiB_this_rank": round(own_bytes / 2 ** 30, 2), "estimated_peak_GiB": round(5.0 * own_bytes / 2 ** 30 + 0.5, 2), "free_GiB": round(free_b / 2 ** 30, 1)}
    if 5.0 * own_bytes + (1 << 29) > free_b:
        raise SystemExit(f"bench.py: {workload}: rank {rank} of {world} would hold {mem['site_tensor_GiB_this_rank']} GiB of site tensors (estimated peak "
                         f"{mem['estimated_peak_GiB']} GiB) but the device has {mem['free_GiB']} GiB free -- use more GPUs (--gpus) or a smaller --L")
    if cfg == "c2" or args.host_init:
        for v, t in random_state_tensors(g, chi, d, 1234, dtype, wanted=(None if world == 1 else bpc.owns), threads=host_threads()):
            if isinstance(t, tuple):
                bpc._declare_dims(v, t)
            else:
                bpc._set_tensor(v, t)
    else:       # the big configurations: generated on the device, rank by rank (counter-based: the same state whatever the sharding)
        for v in g.vertices:
            z = g.degree(v)
            bpc._set_random(v, [chi] * z, 1234, scale=1.0 / np.sqrt(d * float(chi) ** z))
    sweeps, updates, svd_sweeps, svd_max, reused, evicted = [], [], [], [], [], []
    for _ in range(args.warmup):
        info = {}
        bpc, errs = tn.apply_gates(layer, bpc, apply_kwargs=apply_kwargs, bp_update_kwargs=bp_kwargs, info=info)
    tn.profile_enable(bpc, os.environ.get("TNQS_BENCH_NOPROF") != "1")      # (experiment: what the per-class HIP events cost)
    tn.profile_reset(bpc)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        info = {}
        bpc, errs = tn.apply_gates(layer, bpc, apply_kwargs=apply_kwargs, bp_update_kwargs=bp_kwargs, info=info)
        sweeps.append(info["n_sweeps"]); updates.append(info["n_updates"]); svd_sweeps.append(info.get("n_svd_sweeps", 0)); svd_max.append(info.get("n_svd_sweeps_max", 0)); reused.append(info.get("n_bp_products_reused", 0)); evicted.append(info.get("n_bp_products_evicted", 0))
    barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        tmax = torch.tensor([elapsed], device="cuda" if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
    prof_all = tn.profile_get(bpc)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, bpc, g, errs)
    phase_prof = {k: v for k, v in prof_all.items() if k.startswith("phase_")}       # whole phases on the handle's stream (critical path)
    prof = {k: v for k, v in prof_all.items() if not k.startswith("phase_")}           # kernel classes
    # the library's pool keeps what it has allocated: device memory taken since the start of the run = the high-water mark of the layer
    mem["measured_peak_GiB"] = round((free_at_start - torch.cuda.mem_get_info(local if world > 1 else 0)[0]) / 2 ** 30, 2)
    ms_per_step = 1e3 * elapsed / max(1, args.steps)
    value = n2 * args.steps / elapsed

    # ---- roofline of the dominant kernel class ----------------------------------------------------------------
    # bound: arithmetic intensity of the class (algorithmic flops / algorithmic bytes) against the ridge
    # 157.3 TFLOP/s / 8 TB/s = 19.7 flop/B (MI355X_MICROARCH.md).  `achieved` = algorithmic bytes (or flops) of the
    # class / HIP-event time of its launches on the library's stream; `traffic` = HBM bytes per launch from the PMC
    # pass of the same command committed under profiles/ (FETCH_SIZE x2 + WRITE_SIZE, see the file's header).
    m3 = os.environ.get("TNQS_NO_3M") != "1"
    tf = "<true>" if m3 else "<false>"
    KERNEL_OF = {"bp_pair": "tnqs::mfma_pair_kernel" + tf, "bp_modeprod": "tnqs::mfma_rowgemm_kernel<1, 1, 1, %s>" % ("true" if m3 else "false"),
                 "gate_modeprod": "tnqs::mfma_pair_kernel" + tf, "bp_fused": "tnqs::mfma_gram32_fused_kernel",
                 "bp_gram": "tnqs::mfma_gram32_kernel", "gate_gram": "tnqs::mfma_gram64_f64_kernel<%s, true>" % ("true" if m3 else "false"),
                 "gate_apply": "tnqs::mfma_rowgemm_kernel<2, 2, 2, %s>" % ("true" if m3 else "false"), "bp_pairgram": "tnqs::mfma_pair_gram2_kernel" + tf}
    # round 5: the chi = 32 plane kernels carry their f32 products on the bf16 matrix cores (csrc/kernels_x3.hip: every f32 operand is the exact sum of three
    # bf16 pieces, six of the nine piece products are kept -- the dropped ones are below one f32 rounding of the product -- and accumulated in f32)
    x3 = os.environ.get("TNQS_NO_BF16X3") != "1"
    X3_CLASSES = ("bp_pair", "bp_pairgram", "gate_modeprod") if x3 else ()
    if x3:
        KERNEL_OF.update({"bp_pair": "tnqs::x3_pair_kernel", "gate_modeprod": "tnqs::x3_pair_kernel", "bp_pairgram": "tnqs::x3_pair_gram2_kernel<0>"})
    if cfg == "c4":
        KERNEL_OF.update({"bp_pair": "tnqs::mfma_pair16_kernel / tnqs::mfma_pair16w_kernel", "gate_modeprod": "tnqs::mfma_pair16_kernel / tnqs::mfma_pair16w_kernel",
                          "bp_pairgram": "tnqs::mfma_pair_gram2x16_kernel", "gate_gram": "tnqs::mfma_gauge_gram32_kernel"})
    elif cfg == "c5":
        KERNEL_OF.update({"bp_modeprod": "tnqs::mfma_rowgemm_kernel<2, 2, 1>", "gate_modeprod": "tnqs::mfma_rowgemm_kernel<2, 2, 1>", "bp_gram": "tnqs::mfma_gram64_kernel",
                          "gate_gram": "tnqs::mfma_gram128_f64_kernel", "gate_apply": "tnqs::mfma_rowgemm_kernel<4, 4, 2>"})
    traffic_db, traffic_src = profile_db(os.environ.get("TNQS_BENCH_PMC_PROFILE", "r6_pmc_traffic.json"))
    mfma_db, mfma_src = profile_db(os.environ.get("TNQS_BENCH_MFMA_PROFILE", "r6_mfma_util.json"))
    dom = max(prof, key=lambda k: prof[k]["ms"] if prof[k]["bytes"] > 0 else -1.0)      # (the tensor-pass class with the most time: the per-gate factorisation classes book no bytes)
    p = prof[dom]
    roofline = None
    if p["ms"] > 0 and p["bytes"] > 0:
        sec = p["ms"] * 1e-3
        tflops, gbs = p["flops"] / sec / 1e12, p["bytes"] / sec / 1e9
        ai = p["flops"] / p["bytes"]
        kern = KERNEL_OF.get(dom)
        headline = world == 1 and cfg == "c2" and L == 20 and chi == 32      # the committed counter passes are of that command
        traffic = profile_entry(traffic_db, kern).get("hbm_bytes_per_launch") if headline else None
        common = {"kernel_class": dom, "kernel": kern, "avg_launch_ms": round(p["ms"] / max(1, p["launches"]), 4), "launches": p["launches"],
                  "arithmetic_intensity_flop_per_B": round(ai, 2), "alg_bytes_per_launch": round(p["bytes"] / max(1, p["launches"])),
                  "alg_TFLOPs": round(tflops, 2), "alg_GBps": round(gbs, 1), "traffic": traffic,
                  # matrix-core utilisation of the same kernel from the committed counter pass (profiles/r2_mfma_util.json: SQ_VALU_MFMA_BUSY_CYCLES /
                  # (GRBM_GUI_ACTIVE / 8 XCDs x 256 CUs x 4 SIMDs)); like `traffic` it is a profile of this command, not re-measured in this run
                  "mfma_busy": (profile_entry(mfma_db, kern).get("mfma_busy") if headline else None),
                  "mfma_executed_TFLOPs": (profile_entry(mfma_db, kern).get("mfma_tflops") if headline else None),
                  # `achieved` counts ALGORITHMIC flops (8 per complex multiply-add).  The plane kernels form the complex product with Gauss' three
                  # real multiplications (csrc/mfma_common.hpp, CAcc32): the matrix cores execute 0.75 x the algorithmic count, so the
                  # algorithmic rate can exceed what `peak` allows a four-multiplication kernel; executed / peak is the matrix-core load
                  "complex_product": ("3M: three real MFMAs per complex update" if m3 else "4M"),
                  "executed_over_peak": round((0.75 if m3 else 1.0) * tflops / PEAK_F32_TFLOPS, 4),
                  # `traffic`, `mfma_busy`, `mfma_executed_TFLOPs` are NOT measured in this run: they are read from the committed counter passes
                  "from_profile": {"traffic": traffic_src, "mfma": mfma_src}}
        if dom in X3_CLASSES and cfg == "c2":
            # bf16 x 3 kernels: four real products per complex one (no Gauss trick: its operand sums would have to be split too), six bf16 instructions per
            # real product -> the matrix cores execute 6 x the algorithmic count in bf16; what bounds an f32 product on this pipe is 2500 / 6 = 417 TFLOP/s
            exe = 6.0 * tflops
            common.update({"complex_product": "4M, every real product = six exact bf16 products (csrc/kernels_x3.hip)", "executed_over_peak": round(exe / PEAK_BF16_TFLOPS, 4),
                           "executed_bf16_TFLOPs": round(exe, 1), "f32_equivalent_peak_TFLOPs": round(PEAK_BF16_TFLOPS / 6.0, 1)})
            if ai < (PEAK_BF16_TFLOPS / 6.0) * 1e12 / (PEAK_HBM_GBS * 1e9):
                roofline = {"bound": "hbm", "achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(gbs / PEAK_HBM_GBS, 4), **common}
            else:
                roofline = {"bound": "mfma", "achieved": round(exe, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": round(exe / PEAK_BF16_TFLOPS, 4),
                            "hbm_frac": round(gbs / PEAK_HBM_GBS, 4), **common}
        elif ai < PEAK_F32_TFLOPS * 1e12 / (PEAK_HBM_GBS * 1e9):
            roofline = {"bound": "hbm", "achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(gbs / PEAK_HBM_GBS, 4), **common}
        else:
            roofline = {"bound": "mfma", "achieved": round(tflops, 3), "peak": PEAK_F32_TFLOPS, "unit": "TFLOP/s", "frac": round(tflops / PEAK_F32_TFLOPS, 4), **common}
    classes = {k: {"ms": round(v["ms"], 2), "launches": v["launches"],
                   "TFLOPs": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 2) if v["ms"] > 0 else None}
               for k, v in prof.items() if v["launches"]}

    # seconds per BP sweep and per colour batch (HIP-event time of the kernel classes of each phase, per step)
    nst = max(1, args.steps)
    bp_ms = sum(prof[k]["ms"] for k in prof if k.startswith("bp_")) / nst
    gate_ms = sum(prof[k]["ms"] for k in ("gate_modeprod", "gate_gram", "gate_apply", "jacobi") if k in prof) / nst
    # critical path (round-4 verdict): events around whole phases on the handle's stream -- side streams join it before a phase ends.  The sums of the kernel classes
    # (`*_class_sum_*`) count kernels that run next to each other twice and exceed the wall time.
    pb, pg = phase_prof.get("phase_bp_update", {"ms": 0.0, "launches": 0}), phase_prof.get("phase_gate_batch", {"ms": 0.0, "launches": 0})
    phases = {"ms_per_bp_sweep": round(pb["ms"] / max(1, pb["launches"]), 3), "ms_per_colour_batch": round(pg["ms"] / max(1, pg["launches"]), 3),
              "bp_ms_per_step": round(pb["ms"] / nst, 2), "gate_ms_per_step": round(pg["ms"] / nst, 2),
              "bp_sweeps_timed": pb["launches"], "gate_batches_timed": pg["launches"],
              "how": "HIP events at the first and the last kernel of every BP update / two-site gate batch on the handle's stream (TNQS_PROF_PHASE_*)",
              "bp_class_sum_ms_per_step": round(bp_ms, 2), "gate_class_sum_ms_per_step": round(gate_ms, 2)}

    # both flop counts of a step (round-3 verdict): what the engine's algorithm executes (algorithmic flops booked per kernel class: 3u instead of 4u per
    # message through shared pair products, Gram / Cholesky instead of Householder QR) and SURVEY.md 8(d)'s count of the REFERENCE's contraction order
    # with the bulk formulas (per gate 2 (2 n d + 3 d^2) chi^(z+1) cMAC, per message (n + 1) d chi^(z+1) cMAC, n = z - 1; an upper bound on open lattices)
    nz = zdeg - 1
    ref_flops = 8.0 * (n2 * 2 * (2 * nz * d + 3 * d * d) * float(chi) ** (zdeg + 1) + float(np.mean(sweeps)) * 2 * n2 * (nz + 1) * d * float(chi) ** (zdeg + 1))
    exe_flops = sum(v["flops"] for v in prof.values()) / nst
    flop_counts = {"executed_algorithm_TFLOP_per_step": round(exe_flops / 1e12, 3), "executed_algorithm_TFLOPs": round(exe_flops / (ms_per_step * 1e-3) / 1e12, 2),
                   "reference_order_TFLOP_per_step": round(ref_flops / 1e12, 3), "reference_order_TFLOPs": round(ref_flops / (ms_per_step * 1e-3) / 1e12, 2),
                   "note": "reference_order = SURVEY.md 8(d) bulk formulas for the reference's contraction sequence; it may exceed the f32 matrix peak because the "
                           "engine does less work for the same result (shared pair products, Gram + Cholesky instead of QR), not because a kernel skips any"}
    out = {"metric": "two-site gates/sec at fixed chi (LxL TFIM Trotter layer)", "value": round(value, 2),
           "unit": "two-site gates/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": round(ms_per_step, 3), "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
           "dtype": ("c64 (ComplexF32; Gram/eigen steps in f64; the chi = 32 plane products as exact bf16 x 3 splits with f32 accumulation, TNQS_NO_BF16X3=1 for f32 matrix instructions)"
                     if x3 and cfg == "c2" else "c64 (ComplexF32; Gram/eigen steps in f64)"), "data": "synthetic",
           "config": {"workload": workload, "baseline_config": cfg,
                      "two_site_gates_per_step": n2, "bp_updates_per_step": updates, "bp_sweeps_per_step": sweeps,
                      "theta_svd_sweeps_per_gate": round(float(np.mean(svd_sweeps)) / max(1, n2), 2), "theta_svd_sweeps_slowest_gate": int(max(svd_max) if svd_max else 0),
                      "bp_partial_products": {"reused_per_step": reused, "evicted_per_step": evicted},
                      "apply_kwargs": {"maxdim": chi, "cutoff": 1e-10, "normalize_tensors": True},
                      "bp_update_kwargs": "reference defaults (maxiter 25, tol 1e-5)",
                      "bp_order": ("library default: linear forests, one level per forest -- on periodic lattices edge sets that close cycles, two levels per set -- (tnqs_bp_opts.n_sequence = 0; the reference's forest_cover_edge_sequence is n_sequence = -1, "
                                   "bench.py --bp-order reference; same fixed point)" if args.bp_order == "library" else
                                   "the reference's default, forest_cover_edge_sequence(graph) (tnqs_bp_opts.n_sequence = -1)"),
                      "state_init": ("host numpy, per-vertex counter streams" if (cfg == "c2" or args.host_init) else "on device (tnqs_set_site_random, counter-based)"),
                      "memory": mem, "parallelism": f"vertex-shard x{world}",
                      "transport": (None if world == 1 else {"kind": type(bpc._shard).__name__, "nranks": world, "backend": dist.get_backend(),
                                                             "partition": {"rule": "contiguous vertex blocks, heaviest block minimised (weight = site-tensor elements at chi)",
                                                                           **tdist.partition_summary(g, bpc._shard.owner, chi)},
                                                             **({"note": transport_note} if transport_note else {}),
                                                             "allgathers_per_step": round(bpc._shard.n_exchanges / max(1, args.steps + args.warmup), 1),
                                                             "MB_gathered_per_step": round(bpc._shard.bytes_exchanged / max(1, args.steps + args.warmup) / 1e6, 2)})},
           "roofline": roofline, "flop_counts": flop_counts, "phases": phases, "kernel_classes": classes}
    if args.evolved > 0 and world == 1:
        # optional second measurement (not the headline value): a state grown by the circuit itself -- BP needs several sweeps per update there,
        # which the synthetic iid state at dt = 0.01 (one sweep per update) does not show
        lay2 = tfim_layer(tn, g, groups, dt=0.1)
        b2 = tn.BeliefPropagationCache(tn.tensornetworkstate(dtype, lambda v: "↑", g))
        for _ in range(args.evolved):
            b2, _e = tn.apply_gates(lay2, b2, apply_kwargs=apply_kwargs)
        torch.cuda.synchronize(); t0 = time.perf_counter(); sw2 = []; nc2 = 0
        for _ in range(args.steps):
            inf2 = {}
            b2, _e = tn.apply_gates(lay2, b2, apply_kwargs=apply_kwargs, info=inf2); sw2.append(inf2["n_sweeps"]); nc2 += inf2.get("bp_not_converged", 0)
        torch.cuda.synchronize(); el2 = time.perf_counter() - t0
        out["evolved"] = {"state": f"{args.evolved} TFIM layers at dt = 0.1 (J = 1, hx = 2.5) from the product state, maxdim {chi}",
                          "max_bond_dim": int(b2.maxvirtualdim()), "ms_per_step": round(1e3 * el2 / max(1, args.steps), 3),
                          "value": round(n2 * args.steps / el2, 2), "bp_sweeps_per_step": sw2, "bp_updates_not_converged": nc2, "max_truncation_error": float(np.max(_e))}
    if args.full and rank == 0 and world == 1 and cfg == "c2" and x3 and not args.no_ab and not args.no_cpu_baseline:
        # A/B in the same run on the same box (not part of `value`): the chi = 32 plane kernels on v_mfma_f32_32x32x2_f32 instead of the bf16 matrix cores.  The
        # switches are read once per process, hence a child; it must never take the measured number down with it
        try:
            import subprocess
            cmd = [sys.executable, os.path.abspath(__file__), "--steps", str(args.steps), "--warmup", str(args.warmup), "--L", str(L), "--chi", str(chi), "--no-cpu-baseline", "--no-ab"]
            r = subprocess.run(cmd, env=dict(os.environ, TNQS_NO_BF16X3="1"), capture_output=True, text=True, timeout=600)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
            d2 = json.loads(line)
            out["ab_f32_matrix_instructions"] = {"env": "TNQS_NO_BF16X3=1", "ms_per_step": d2["ms_per_step"], "value": d2["value"],
                                                 "kernel_classes_ms": {k: v["ms"] for k, v in d2["kernel_classes"].items() if k in ("bp_pair", "bp_pairgram", "gate_modeprod")},
                                                 "this_run_kernel_classes_ms": {k: v["ms"] for k, v in classes.items() if k in ("bp_pair", "bp_pairgram", "gate_modeprod")}}
        except Exception as e:
            out["ab_f32_matrix_instructions"] = {"value": None, "error": repr(e)}
    if args.full and rank == 0 and world == 1 and cfg == "c2" and args.bp_order == "library" and not args.no_ref_order and not args.no_cpu_baseline:
        # the reference's own default sweep order (beliefpropagationcache.jl:28,41 forest_cover_edge_sequence; what the Julia shim passes by default) in the same run
        # on the same box, not part of `value` (round-5 verdict: the headline times the library's order; at the default tolerance both stop after one sweep per update
        # on different trajectories of the same fixed-point iteration)
        try:
            import subprocess
            cmd = [sys.executable, os.path.abspath(__file__), "--steps", str(args.steps), "--warmup", str(args.warmup), "--L", str(L), "--chi", str(chi), "--bp-order", "reference",
                   "--no-cpu-baseline", "--no-ab", "--no-ref-order"]
            r = subprocess.run(cmd, env=dict(os.environ), capture_output=True, text=True, timeout=600)
            d3 = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            out["reference_order"] = {"flag": "--bp-order reference (tnqs_bp_opts.n_sequence = -1)", "ms_per_step": d3["ms_per_step"], "value": d3["value"],
                                      "bp_sweeps_per_step": d3["config"]["bp_sweeps_per_step"], "bp_updates_per_step": d3["config"]["bp_updates_per_step"],
                                      "phases": {k: d3["phases"][k] for k in ("ms_per_bp_sweep", "ms_per_colour_batch", "bp_ms_per_step", "gate_ms_per_step")},
                                      "kernel_launch_classes": {k: v["launches"] for k, v in d3["kernel_classes"].items()}}
        except Exception as e:
            out["reference_order"] = {"value": None, "error": repr(e)}
    if rank == 0:
        if args.full and world == 1 and not args.no_cpu_baseline and cfg == "c2":      # (the CPU leg restates the 2-D chi = 32 path on a bounded sample; the 8-GPU shapes have none)
            try:
                out["cpu_baseline"] = cpu_baseline(chi, L)
            except Exception as e:      # the baseline must never take the measured number down with it; no compiler / no OpenBLAS on the host: the threaded numpy port
                try:
                    import cpu_layer
                    m = cpu_layer.measure_host(chi=chi, L=L, periodic=False)
                    out["cpu_baseline"] = {"value": m["gates_per_s"], "unit": "two-site gates/s", "cores": int(m["threads"]), "kind": "port", "compiled": False,
                                           "sample": f"1 TFIM layer of the {L}x{L} open lattice per process, {m['processes']} process(es) x {m['threads_per_process']} threads, chi={chi}, complex64, "
                                                     f"threaded numpy / LAPACK port (oracle/cpu_layer.py); {m['seconds_per_layer']:.1f} s per layer", "compiled_port_error": repr(e)}
                except Exception as e2:
                    out["cpu_baseline"] = {"value": None, "error": repr(e), "fallback_error": repr(e2)}
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
