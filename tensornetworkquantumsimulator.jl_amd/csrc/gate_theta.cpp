// gate_theta.cpp -- the theta phase of a two-site gate batch (simple_update.jl:51-59): which route a gate is offered and what it is given to work in (theta_route;
// host code, no device call), the launch chain from the Gram factors to the scaled theta (launch_theta_chain), and the item fills / launch sequences of the small-SVD
// route and of the second factorisation pass.  engine_gates.cpp (TwoSiteBatch) and the kernel-level entry points of debug_gate.cpp both run THIS code.
#include "engine_internal.hpp"

namespace tnqs {

ThetaRoute theta_route(bool F32, int d1, int d2, int chi, int kappa, int maxdim) {
    ThetaRoute r{};
    r.n1 = d1 * chi; r.n2 = d2 * chi; r.Mr = r.n1 * d1; r.Nc = r.n2 * d2;
    // theta is at most 512 x 512 (d^2 chi <= 512: chi <= 128 for qubits); up to 256 rows everything has an LDS or MFMA-preprocessed route, beyond
    // that the factorisations run in the global-memory Jacobi kernel (8 rows per lane)
    if ((long long)d1 * d1 * chi > 512 || (long long)d2 * d2 * chi > 512) throw Err(TNQS_ERR_UNSUPPORTED, "two-site gate: d^2*chi > 512 is not supported by the theta SVD kernels");
    r.cap = std::min(r.Mr, r.Nc); if (maxdim > 0) r.cap = std::min(r.cap, maxdim);
    // the operator-sum factors A ((r1 d1) x K), B ((r2 d2) x K), K = kappa chi: theta = A B^T is formed from them (gate_theta_mm_kernel);
    // the low-rank route of the theta SVD (lowG / lowL) only where it can apply -- K below the theta columns and chol_kernel's size
    r.K = kappa * chi; r.opsum = kappa > 0;
    if (!r.opsum) return r;
    const size_t K = (size_t)r.K;
    r.nA = (size_t)r.Mr * K; r.nB = (size_t)r.Nc * K;
    const bool lds_fits = F32 || jacobi_lds(jacobi_lds_bytes(r.Mr, r.K, false, 16)) > 0;      // ComplexF64: only where it buys the LDS route
    r.low = r.K < r.Nc && r.K <= 128 && r.cap <= r.K && r.Mr >= r.Nc && lds_fits;
    if (!r.low) return r;
    r.nG = K * K;
    // ComplexF32, factor of at most 128 x 64: the preconditioned SVD kernel builds V from Q = B L^-dagger (lowrank_m_kernel writes it)
    r.lowq = F32 && use_precond_svd() && theta_svd_pre_covers(r.Mr, r.K) && r.K <= 96;
    if (r.lowq) r.nQ = r.nB;
    if (!F32) { r.nB1 = r.nB; r.nG2 = K * K; }      // ComplexF64: B is orthogonalised by CholeskyQR2 (kernels.hpp LowQr2Item)
    return r;
}

template <class T> void launch_theta_chain(hipStream_t st, const GateItem* d_items, const std::vector<GateItem>& items, const std::vector<ThetaLowWs>& ws,
                                           int* d_fail1, int* d_fail2, DescUpload up, int last_stage) {
    constexpr bool F32 = std::is_same<T, float>::value;
    const int n = (int)items.size();
    launch_gate_theta<T>(st, d_items, n);
    if (last_stage < 1) return;
    bool opsum = false; for (auto& it : items) opsum = opsum || it.lowA;
    if (opsum) launch_gate_theta_mm<T>(st, d_items, n);        // theta = A B^T on the f64 matrix cores (gates with operator-sum factors)
    if (last_stage < 2) return;
    std::vector<CholItem> lc, lc2; int kmax = 1;
    std::vector<GateItem> g2, g3; std::vector<LowQr2Item> qi;
    for (int q = 0; q < n; ++q) {
        if (!items[q].lowG) continue;
        const int K = items[q].kappa * items[q].chi; const ThetaLowWs& w = ws[q];
        int* fail1 = d_fail1 + q;
        // ComplexF32: tau at the f32 noise floor.  ComplexF64: 1e-12 on the pivots of pass 1 keeps kappa(B) <= 1e6, where the second pass restores
        // orthogonality to eps; anything worse falls back to the SVD of the full theta
        lc.push_back(CholItem{items[q].lowG, const_cast<void*>(items[q].lowL), (K <= 96 || !F32) ? w.lowW : nullptr, K, fail1, !F32 ? 1e-12 : rank_tau(true, K)});
        kmax = std::max(kmax, K);
        if (!F32) {
            int* fail2 = d_fail2 + q;      // ComplexF64: second CholeskyQR pass of the low-rank route
            lc2.push_back(CholItem{w.lowG2, w.lowL2, nullptr, K, fail2, 1e-3});      // G2 is the identity up to kappa(G1) eps: a pivot below 1e-3 means pass 1 was not good enough
            GateItem a = items[q]; a.lowB = w.lowB1; a.lowG = w.lowG2; a.lowL = w.lowL2; g2.push_back(a);
            GateItem b = items[q]; b.lowL = w.lowLc; g3.push_back(b);
            qi.push_back(LowQr2Item{items[q].lowB, w.lowW, w.lowB1, items[q].lowL, w.lowL2, w.lowLc, items[q].info, items[q].d2, fail1, fail2});
        }
    }
    auto chol = [&](const CholItem* dc, size_t m) { if (kmax <= 96) launch_chol(st, dc, (int)m, kmax); else launch_chol_packed(st, dc, (int)m, kmax); };
    if (!lc.empty()) {
        const CholItem* dc = up.vec(lc); launch_lowrank_g(st, d_items, n);
        chol(dc, lc.size());      // ComplexF32: only L is used here
        if (F32) launch_lowrank_m<T>(st, d_items, n);
        else {
            const LowQr2Item* dq = up.vec(qi); const GateItem* d2 = up.vec(g2); const GateItem* d3 = up.vec(g3); const CholItem* dc2 = up.vec(lc2);
            launch_lowrank_bw(st, dq, (int)qi.size());                       // B1 = B L1^-dagger
            launch_lowrank_g(st, d2, (int)g2.size());                        // G2 = B1^dagger B1
            chol(dc2, lc2.size());
            launch_lowrank_ll(st, dq, (int)qi.size());                       // Lc = L1 L2 (+ pass-2 failure -> the gate's flag)
            launch_lowrank_m<T>(st, d3, (int)g3.size());                     // theta[:, :K] = A conj(Lc)
        }
    }
    if (last_stage >= 3) launch_theta_scale<T>(st, d_items, n);       // theta (or M) and theta0 to O(1), exponent kept per gate for gate_finish
}
template void launch_theta_chain<float>(hipStream_t, const GateItem*, const std::vector<GateItem>&, const std::vector<ThetaLowWs>&, int*, int*, DescUpload, int);
template void launch_theta_chain<double>(hipStream_t, const GateItem*, const std::vector<GateItem>&, const std::vector<ThetaLowWs>&, int*, int*, DescUpload, int);

void small_svd_items(const void* src, void* M, void* GA, void* GV, int d, int low, int chi_b, int hi, std::vector<SmallSvdItem>& si, std::vector<JacobiItem>& sji) {
    si.push_back(SmallSvdItem{src, M, GA, GV, d, low, chi_b, hi});
    sji.push_back(JacobiItem{M, nullptr, d * chi_b, low * hi, nullptr});
}
template <class T> void launch_small_svd(hipStream_t st, const SmallSvdItem* ds, const JacobiItem* dj, const std::vector<JacobiItem>& sji) {
    launch_small_svd_prepare<T>(st, ds, (int)sji.size());
    size_t lds = 0; for (auto& j : sji) lds = std::max(lds, jacobi_lds_bytes(j.m, j.n, false, 16));
    launch_jacobi<double>(st, dj, (int)sji.size(), 60, jacobi_lds(lds), mmax_of(sji));
    launch_small_svd_finish(st, ds, (int)sji.size());
}
template void launch_small_svd<float>(hipStream_t, const SmallSvdItem*, const JacobiItem*, const std::vector<JacobiItem>&);
template void launch_small_svd<double>(hipStream_t, const SmallSvdItem*, const JacobiItem*, const std::vector<JacobiItem>&);

}  // namespace tnqs
