// fiber_plan.cpp -- which fiber GEMM kernel a pass launches (host code, no device call): the one place that decides between the generic tiled kernel, the f32
// matrix-core tiles, the register-direct kernels and the f64 matrix cores, and lays the items out for the kernel chosen.  The per-kernel layout functions
// (plan_fiber_gemm, plan_rowgemm, plan_fiber_gemm_f64) stay next to their kernels; the engine's runner (engine_batch.cpp FiberPass) and the debug entry points
// (debug_fiber.cpp) launch what this returns through launch_fiber_route.
//
//   route    taken when                                                                        kernel
//   RowGemm  f32, use_mfma, rowgemm_covers(item), D == rg_D, K == 32 or (K == 64 and           mfma_rowgemm_kernel<KB, NB, D> / x3_rowgemm64_kernel
//            use_chi64): item by item; one launch per K, 64 first                              (launch_mfma_rowgemm)
//   F64      f64, use_mfma, Chain: every item left passes fiber_gemm_f64_covers;               mfma_fiber_gemm_f64_kernel<NBLK, KS, GEN>
//            Epilogue: 4 <= KKmax <= 64 and NNmax <= 64
//   Mfma     f32, use_mfma, kk_min <= KKmax <= 64 and NNmax <= 64                              mfma_fiber_gemm_w_kernel<1, 1, 8> / <2, 2, 16>
//   Generic  everything else, and every item of a Plain pass                                   fiber_gemm_kernel<T, 8>
//
// KKmax = max D K, NNmax = max Do No and the tile count behind the Mfma tpw rule are taken over ALL items of the pass, the ones RowGemm took included: a
// chi = 24 leg that shares its pass with a chi = 64 RowGemm leg runs in <2, 2, 16>, not <1, 1, 8>.  The launches have always been sized this way; a change
// here changes which instantiation runs.
#include "kernels.hpp"

namespace tnqs {

FiberRules fiber_rules(FiberUse use, bool f32, bool use_mfma, bool use_chi64) {
    FiberRules r; r.f32 = f32; r.use_mfma = use_mfma; r.use_chi64 = use_chi64;
    switch (use) {
    case FiberUse::Chain: r.rg_D = 1; r.rg_cap = 64; r.matrix = true; break;      // mode products: no site index, no norm; tpw from the size of the pass
    case FiberUse::Epilogue: r.rg_D = 2; r.rg_cap = 32; r.matrix = true; r.general = true; r.mfma_tpw = 16; r.f64_tpw = 32; break;
    case FiberUse::Plain: break;
    }
    return r;
}

std::vector<FiberLaunch> plan_fiber_pass(const FiberItem* items, int n, const FiberRules& r, size_t esz) {
    std::vector<FiberLaunch> plan; plan.reserve(3);
    int KKmax = r.kk_floor, NNmax = 1; double tiles32 = 0;      // (see the head of the file: over all items)
    for (int i = 0; i < n; ++i) {
        KKmax = std::max(KKmax, items[i].D * items[i].K); NNmax = std::max(NNmax, items[i].Do * items[i].No);
        tiles32 += (double)items[i].D * items[i].PA * items[i].PB / 32;
    }
    auto takes_rowgemm = [&](const FiberItem& it) { return r.rg_D && r.f32 && r.use_mfma && it.D == r.rg_D && rowgemm_covers(it) && (it.K != 64 || r.use_chi64); };
    auto open = [&](FiberRoute route, int D, int K) {
        plan.push_back(FiberLaunch{route, D, K, 0, 1, KKmax, NNmax, 0, r.general, {}, {}, {}});
        return &plan.back();
    };
    auto close = [&](FiberLaunch& L, int tpw, int wgs) { L.wgs = wgs; L.tpw = L.items.empty() ? tpw : L.items[0].tpw; };      // (tpw: what was asked for; 0 = the kernel's rule)
    for (int K : {64, 32}) {
        FiberLaunch* L = nullptr;
        for (int i = 0; i < n; ++i) {
            if (items[i].K != K || !takes_rowgemm(items[i])) continue;
            if (!L) L = open(FiberRoute::RowGemm, r.rg_D, K);
            L->items.push_back(items[i]); L->index.push_back(i); rowgemm_tiles(L->items.back());
        }
        if (!L) continue;
        L->TR = 32; L->nwg.resize(L->items.size());
        close(*L, r.rg_tpw, plan_rowgemm(L->items.data(), (int)L->items.size(), r.rg_cap, L->nwg.data(), r.rg_tpw));
    }
    FiberLaunch* L = nullptr; bool all_f64 = true;
    for (int i = 0; i < n; ++i) {
        if (takes_rowgemm(items[i])) continue;
        if (!L) L = open(FiberRoute::Generic, 0, 0);
        L->items.push_back(items[i]); L->index.push_back(i); all_f64 = all_f64 && fiber_gemm_f64_covers(items[i]);
    }
    // the gate epilogue plans this launch even when RowGemm took every item: nothing is launched then (no workgroups), but its norm buffer and norm-factor pass
    // keep their place in the batch's sequence of allocations
    if (!L && r.general && n > 0) L = open(FiberRoute::Generic, 0, 0);
    if (!L) return plan;
    const int ni = (int)L->items.size(); L->nwg.resize(ni);
    const bool matrix = r.matrix && r.use_mfma;
    if (matrix && !r.f32 && (r.general ? KKmax >= 4 && KKmax <= 64 && NNmax <= 64 : all_f64)) {
        L->route = FiberRoute::F64; L->TR = 16;
        close(*L, r.f64_tpw, plan_fiber_gemm_f64(L->items.data(), ni, L->nwg.data(), r.f64_tpw));
    } else if (matrix && r.f32 && KKmax >= r.kk_min && mfma_fiber_tile_rows(KKmax, NNmax) > 0) {
        L->route = FiberRoute::Mfma; L->TR = mfma_fiber_tile_rows(KKmax, NNmax);
        int tpw = r.mfma_tpw;
        if (tpw <= 0) { tpw = (int)std::max(1.0, std::min(32.0, tiles32 / 4096.0)); if (tpw >= 4) tpw &= ~3; }
        close(*L, tpw, plan_fiber_gemm(L->items.data(), ni, L->TR, tpw, L->nwg.data()));
    } else {
        L->TR = pick_TR((size_t)KKmax, esz, 1);
        close(*L, 1, plan_fiber_gemm(L->items.data(), ni, L->TR, 1, L->nwg.data()));
    }
    return plan;
}

}  // namespace tnqs
