"""Selection of the truncated boundary-MPS cases of tests/test_gpu_bmps.py, run on the host: `python tests/bmps_truncated_select.py` writes tests/golden/meta/bmps_truncated.json.

After a few sweeps the truncated result depends on how a QR completes the null space of the rank-deficient guess; only the converged value is comparable between
implementations.  So every candidate (4 x 4, chi, seed, the state taken through gauge_and_scale by the numpy oracle) is run through tests/bmps_ref.py with five seeded
null-space completions per (R, tolerance); it is kept only if every fit of every run stops by its tolerance before niters = 50, otherwise the next seed is tried.  The
spread of the five results, per observable, is what the device is allowed ten times of (floored at the exact-regime bound of its element type)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import bmps_cases as cases      # noqa: E402
import bmps_ref as ref          # noqa: E402

RS = (2, 4, 8)
COMPLETIONS = (None, 1, 2, 3, 4)      # numpy's own completion, then four seeded random ones
TOLERANCES = {"complex64": 1e-5, "complex128": 1e-6}      # past the first few sweeps, and every fit of these random states stops by it before niters = 50 (at 1e-8, the ComplexF64 default, chi = 3 does not)
OBS = [([(2, 2)], "Z"), ([(2, 1), (2, 4)], "ZZ"), ([(3, 3)], "I")]
OPS = {"Z": cases.Z, "I": np.eye(2)}
OUT = os.path.join(HERE, "golden", "meta", "bmps_truncated.json")


def gauged_state(chi, seed):
    """gauge_and_scale (src/symmetric_gauge.jl:76-83) by the numpy oracle: BP with maxiter = 40, rescale, symmetric gauge"""
    import tnqs_oracle as o
    g, tensors = cases.grid_state((4, 4), chi, 2, seed)
    og = o.Graph(list(g.vertices), list(g.edges))
    bpc = o.update(o.BeliefPropagationCache(o.TensorNetworkState(og, dict(tensors))), maxiter=40)
    bpc = o.symmetric_gauge(o.rescale(bpc))
    return g, tensors, {v: np.asarray(bpc.tns.tensors[v]) for v in g.vertices}


def run(g, gauged, R, tol, seed):
    b = ref.BoundaryMPS(g, gauged, R, partition_by="row", tolerance=tol, qr=ref.qr_numpy if seed is None else ref.qr_random_completion(seed))
    return [complex(b.expect(vs, [OPS[c] for c in name])) for vs, name in OBS], max(b.sweeps.values())


def main():
    import statevector as sv
    import tnqs_oracle as o
    out = {}
    for chi in (2, 3):
        for seed in range(40, 60):
            g, tensors, gauged = gauged_state(chi, seed)
            entry = {"chi": chi, "seed": seed, "observables": [[[list(v) for v in vs], name] for vs, name in OBS], "runs": {}}
            ok = True
            for dt, tol in TOLERANCES.items():
                for R in RS:
                    vals, sweeps = zip(*[run(g, gauged, R, tol, s) for s in COMPLETIONS])
                    if max(sweeps) >= 50:
                        ok = False
                        break
                    vals = np.asarray(vals)
                    spread = np.abs(vals - vals[0]).max(axis=0)
                    entry["runs"][f"{dt}_R{R}"] = {"tolerance": tol, "sweeps": list(map(int, sweeps)), "re": vals[0].real.tolist(), "im": vals[0].imag.tolist(), "spread": spread.tolist()}
                if not ok:
                    break
            if not ok:
                print(f"chi = {chi} seed = {seed}: a fit ran into niters, next seed")
                continue
            og = o.Graph(list(g.vertices), list(g.edges))
            psi = sv.tns_to_statevector(o.TensorNetworkState(og, dict(tensors)))
            dense = [complex(sv.expect_statevector_multi(psi, og, {v: OPS[c] for v, c in zip(vs, name)})) for vs, name in OBS]
            entry["dense_re"] = [d.real for d in dense]; entry["dense_im"] = [d.imag for d in dense]
            out[f"4x4_chi{chi}"] = entry
            print(f"chi = {chi}: seed {seed} kept", {k: (max(v["sweeps"]), max(v["spread"])) for k, v in entry["runs"].items()})
            break
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
