// engine_spectra.cpp -- entanglement spectra of bonds from the BP messages in one call (tnqs_bond_spectra; the reference's renyi_entropy(bp_cache, e; alpha),
// src/entanglement.jl:73-86, up to the eigenvalues).  For request (u, v) with m1 = message u -> v, m2 = message v -> u:
//   r = m2^{1/2} by the Hermitian eigen decomposition in f64 (safe_eigen), eigenvalues below cutoff = 10 eps(real type) dropped, a negative one beyond it an error
//   (pseudo_sqrt_inv_sqrt, src/utils.jl:18-26);  rho = r m1^T r;  spectrum = eigenvalues of rho / tr rho.
// One item per REQUEST (both orientations and repeats are computed as listed), one launch per stage over all items of the call (each Jacobi stage: one per kernel):
//   A  env_prepare<T> + jacobi<double>:   m2 = V Lambda V^dagger                      (existing kernels, as symmetric_gauge uses them)
//   B  bond_rho<T>:                       W = D V^dagger m1^T V D, Hermitised, tr W   (kernels_spectrum.hip)
//   C  jacobi<double> on W
//   D  bond_spectrum_finish:              signed Rayleigh quotients / tr W, descending, into the call's result buffer
// The call ends with ONE read-back: the spectra of all requests and the flag word behind them.  Nothing of the handle is written.
#include "engine_internal.hpp"

namespace tnqs {

double bond_spectrum_cutoff(int dtype) { return 10.0 * (dtype == TNQS_C64 ? 1.1920928955078125e-07 : 2.220446049250313e-16); }

BondSpecLaunch fill_bond_spec_items(std::vector<BondSpecBufs> b, double cutoff, std::vector<EnvItem>& ei, std::vector<JacobiItem>& j1, std::vector<JacobiItem>& j2,
                                    std::vector<BondSpecItem>& items) {
    // the items whose f64 matrix with V fits the LDS-resident Jacobi come first (n <= 70), so that each Jacobi stage is one launch per kernel over a contiguous range and
    // a single large bond does not send the small ones to the global-memory kernel (engine_batch.cpp svd_batch separates its items the same way)
    auto fits = [](const BondSpecBufs& x) { return jacobi_lds(jacobi_lds_bytes(x.n, x.n, true, 16)) > 0; };
    std::stable_partition(b.begin(), b.end(), fits);
    BondSpecLaunch L{(int)b.size(), 0, 1, 1};
    for (const BondSpecBufs& x : b) {
        if (fits(x)) { ++L.nfit; L.nmax_fit = std::max(L.nmax_fit, x.n); } else L.nmax_rest = std::max(L.nmax_rest, x.n);
        ei.push_back(EnvItem{x.m2, x.H, x.V, x.n});
        j1.push_back(JacobiItem{x.H, x.V, x.n, x.n, nullptr});
        j2.push_back(JacobiItem{x.W, x.V2, x.n, x.n, nullptr});
        items.push_back(BondSpecItem{x.m1, x.H, x.V, /* T1 takes the place of A = H V once the eigenvalues are read */ x.H, x.W, x.V2, x.trace, x.out, x.n, cutoff, x.flag});
    }
    return L;
}
// stages A-D on device-resident descriptor arrays laid out by fill_bond_spec_items: one launch of env_prepare, bond_rho and bond_spectrum_finish over all items; each
// Jacobi stage as the LDS-resident kernel with V over the first nfit items and the global-memory kernel over the rest
template <class T> void launch_bond_spectra_stages(hipStream_t st, const EnvItem* d_env, const JacobiItem* d_j1, const JacobiItem* d_j2, const BondSpecItem* d_items,
                                                   const BondSpecLaunch& L) {
    const size_t lds = jacobi_lds(jacobi_lds_bytes(L.nmax_fit, L.nmax_fit, true, 16));
    auto jacobi = [&](const JacobiItem* d) {
        launch_jacobi<double>(st, d, L.nfit, 60, lds, L.nmax_fit);
        launch_jacobi<double>(st, d + L.nfit, L.nitems - L.nfit, 60, 0, L.nmax_rest);
    };
    launch_env_prepare<T>(st, d_env, L.nitems);
    jacobi(d_j1);
    launch_bond_rho<T>(st, d_items, L.nitems);
    jacobi(d_j2);
    launch_bond_spectrum_finish(st, d_items, L.nitems);
}
template void launch_bond_spectra_stages<float>(hipStream_t, const EnvItem*, const JacobiItem*, const JacobiItem*, const BondSpecItem*, const BondSpecLaunch&);
template void launch_bond_spectra_stages<double>(hipStream_t, const EnvItem*, const JacobiItem*, const JacobiItem*, const BondSpecItem*, const BondSpecLaunch&);

const char* bond_spectrum_flag_message(int flag) {
    if (flag & 1) return "bond_spectra: a message eigenvalue is negative beyond the cutoff (DomainError in the reference, utils.jl:21)";
    return "bond_spectra: the trace of a bond's density matrix is not positive and finite";
}

void bond_spectra(State* s, int n_edges, const int32_t* eu, const int32_t* ev, double* out) {
    const Graph& g = *s->g;
    if (n_edges < 0 && eu && ev) throw Err(TNQS_ERR_INVALID, "bond_spectra: negative count");
    if (s->sharded()) throw Err(TNQS_ERR_UNSUPPORTED, "bond_spectra: sharded handles are not supported");
    // requests as (directed edge of m1 = u -> v); null lists: every edge as (src, dst)
    std::vector<int> req;
    if (!eu || !ev) for (int e = 0; e < g.ne; ++e) req.push_back(2 * e);
    else for (int i = 0; i < n_edges; ++i) {
        if (eu[i] < 0 || eu[i] >= g.nv || ev[i] < 0 || ev[i] >= g.nv) throw Err(TNQS_ERR_INVALID, "bond_spectra: bad vertex");
        const int de = g.dedge(eu[i], ev[i]);
        if (de < 0) throw Err(TNQS_ERR_INVALID, "bond_spectra: not an edge");
        req.push_back(de);
    }
    if (req.empty()) return;
    if (!out) throw Err(TNQS_ERR_INVALID, "bond_spectra: null output");
    size_t total = 0, ws_bytes = 0;
    for (int de : req) {
        const int n = s->chi[de / 2];
        if (n > 256) throw Err(TNQS_ERR_UNSUPPORTED, "bond_spectra: bond dimension > 256");
        total += (size_t)n; ws_bytes += 4 * round256((size_t)n * n * 16);      // H, V, W, V2
    }
    HIPCHK(hipSetDevice(s->device));
    reserve_readback(s, (total + 1) * 8);       // (refuses a result beyond the staging arena before anything is enqueued)
    // result: the spectra one after the other, then the flag word; workspace: four n x n complex128 slots per request
    Buf d_res = dalloc(s, (total + 1) * 8), d_tr = dalloc(s, req.size() * 8), ws = dalloc(s, ws_bytes);
    double* res = reinterpret_cast<double*>(d_res->p);
    int* flag = reinterpret_cast<int*>(res + total);
    HIPCHK(hipMemsetAsync(flag, 0, 8, s->stream));
    std::vector<BondSpecBufs> bufs; size_t off = 0, off_out = 0; double mbytes = 0, flops = 0;
    for (size_t i = 0; i < req.size(); ++i) {
        const int de = req[i], n = s->chi[de / 2]; const size_t slot = round256((size_t)n * n * 16);
        char* p = reinterpret_cast<char*>(ws->p) + off; off += 4 * slot;
        bufs.push_back(BondSpecBufs{s->msg[de] ? s->msg[de]->p : nullptr, s->msg[de ^ 1] ? s->msg[de ^ 1]->p : nullptr, p, p + slot, p + 2 * slot, p + 3 * slot,
                                    reinterpret_cast<double*>(d_tr->p) + i, res + off_out, n, flag});
        off_out += (size_t)n;
        mbytes += 2.0 * n * n * s->esz() + 8.0 * n * n * 16; flops += 16.0 * n * n * n;
    }
    std::vector<EnvItem> ei; std::vector<JacobiItem> j1, j2; std::vector<BondSpecItem> items;
    const BondSpecLaunch L = fill_bond_spec_items(bufs, bond_spectrum_cutoff(s->dtype), ei, j1, j2, items);
    const EnvItem* de_ = upload(s, ei); const JacobiItem* dj1 = upload(s, j1); const JacobiItem* dj2 = upload(s, j2); const BondSpecItem* di = upload(s, items);
    {   // the whole chain is booked as one scope of small kernels (its Jacobi launches included)
        ProfScope ps(s, TNQS_PROF_SMALL, mbytes, flops);
        if (s->dtype == TNQS_C64) launch_bond_spectra_stages<float>(s->stream, de_, dj1, dj2, di, L); else launch_bond_spectra_stages<double>(s->stream, de_, dj1, dj2, di, L);
    }
    const double* h = readback<double>(s, d_res->p, total + 1);      // ONE read-back through the pinned arena: spectra and flag
    sync(s);
    int hflag; std::memcpy(&hflag, h + total, sizeof(int));
    if (hflag) throw Err(TNQS_ERR_NUMERIC, bond_spectrum_flag_message(hflag));
    std::memcpy(out, h, total * 8);
}

}  // namespace tnqs
