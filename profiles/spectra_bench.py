"""von Neumann entropy of every bond of a square lattice, two ways on the SAME handle: bond_entropies(bpc, 1) (one tnqs_bond_spectra call: all eigen problems on the
device, one read-back) and the host loop a user had before it -- per bond two tnqs_get_message read-backs and two numpy.linalg.eigh (the root of one message, then
rho = r m1^T r), the formula of tests/bond_spectra_ref.py.  ComplexF32 states generated on the device as bench.py generates them (tnqs_set_site_random), 7x7 and 20x20
at chi = 32.  Per lattice: wall seconds of both (host clock around calls that end in a stream synchronise; median of the repeats after a warm-up call each, profiler
off), their ratio, and the largest difference between the two results, which must stay under the device bound of tests/test_gpu_bond_spectra.py on the spectra
(max(200 eps chi, 10 x SPECTRUM_BASELINE)) -- the script fails otherwise.
    python profiles/spectra_bench.py [7 | 20] [chi] [repeats] [loop_repeats]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import numpy as np
import tnqs_amd as tn
import bond_spectra_ref as br
from test_bond_spectra_ref_cpu import SPECTRUM_BASELINE


def device_state(n, chi, d=2):
    g = tn.named_grid((n, n))
    bpc = tn.BeliefPropagationCache(tn.tensornetworkstate(np.complex64, lambda v: "↑", g))
    for v in g.vertices:
        z = g.degree(v)
        bpc._set_random(v, [chi] * z, 1234, scale=1.0 / np.sqrt(d * float(chi) ** z))
    return tn.update(bpc, maxiter=10, tolerance=None)


def host_loop(bpc, edges, cutoff):
    """the spectra by the route a user had before tnqs_bond_spectra: 2 read-backs and 2 eigh per bond"""
    return [br.bond_spectrum(bpc.message((u, v)), bpc.message((v, u)), cutoff) for (u, v) in edges]


def lattice(n, chi, repeats, loop_repeats):
    bpc = device_state(n, chi)
    edges = list(bpc.graph.edges)
    cutoff = br.cutoff_of(np.complex64)
    tn.bond_entropies(bpc, 1)                                                # warm-up: code objects, pool
    batched = []
    for _ in range(repeats):
        t0 = time.perf_counter(); s_dev = tn.bond_entropies(bpc, 1); batched.append(time.perf_counter() - t0)
    host_loop(bpc, edges[:4], cutoff)
    loop = []
    for _ in range(loop_repeats):
        t0 = time.perf_counter(); spec_host = host_loop(bpc, edges, cutoff); s_host = np.array([br.renyi(lam, 1, cutoff) for lam in spec_host]); loop.append(time.perf_counter() - t0)
    spec_dev = tn.bond_spectra(bpc)
    d_spec = max(float(np.max(np.abs(spec_dev[e] - lam))) for e, lam in zip(edges, spec_host))
    d_ent = float(np.max(np.abs(s_dev - s_host)))
    bound = max(200 * br.EPS64 * chi, 10 * SPECTRUM_BASELINE)
    assert d_spec <= bound, (d_spec, bound)
    assert d_ent <= 1e-5, d_ent                                              # the project's bound on a ComplexF32 observable
    tb, tl = float(np.median(batched)), float(np.median(loop))
    return dict(lattice=f"{n}x{n}", chi=chi, bonds=len(edges), bond_entropies_seconds_median=tb, bond_entropies_seconds_all=batched,
                host_loop_seconds_median=tl, host_loop_seconds_all=loop, loop_over_batched=tl / tb, max_abs_diff_spectra=d_spec, max_abs_diff_entropy=d_ent,
                spectra_bound=bound, entropy_min=float(s_dev.min()), entropy_max=float(s_dev.max()))


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    chi = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    loop_repeats = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    print(json.dumps(lattice(n, chi, repeats, loop_repeats)), flush=True)
