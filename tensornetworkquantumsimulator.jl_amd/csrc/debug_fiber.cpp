// debug_fiber.cpp -- kernel-level test entry points (include/tnqs_debug.h) of the fiber GEMM and Gram kernels (kernels.hip, kernels_mfma.hip, kernels_x3.hip,
// kernels_chi64.hip, kernels_gate.hip, kernels_f64.hip) and of their planner (fiber_plan.cpp).
#include "debug_util.hpp"

using namespace tnqs;

// HOST ONLY: the launches of one fiber GEMM pass as the engine plans them (fiber_plan.cpp plan_fiber_pass)
extern "C" int tnqs_dbg_fiber_plan(int use, int dtype, int use_mfma, int use_chi64, int nitems, const int* shape, int* launches, int cap, int* nlaunches_out, int* items_out) {
    return guard([&] {
        if (use < 0 || use > 2 || !is_dtype(dtype) || nitems < 0 || (nitems > 0 && !shape) || !nlaunches_out) throw Err(TNQS_ERR_INVALID, "tnqs_dbg_fiber_plan: bad arguments");
        std::vector<FiberItem> items(nitems);
        for (int i = 0; i < nitems; ++i) {
            const int* q = shape + 6 * i; for (int k = 0; k < 6; ++k) if (q[k] < 1) throw Err(TNQS_ERR_INVALID, "tnqs_dbg_fiber_plan: bad shape");
            FiberItem& it = items[i]; it.D = q[0]; it.PA = q[1]; it.K = q[2]; it.PB = q[3]; it.Do = q[4]; it.No = q[5];
        }
        const FiberUse fu = use == 0 ? FiberUse::Chain : use == 1 ? FiberUse::Epilogue : FiberUse::Plain;
        const std::vector<FiberLaunch> plan = plan_fiber_pass(items.data(), nitems, fiber_rules(fu, dtype == TNQS_C64, use_mfma != 0, use_chi64 != 0), esz_of(dtype));
        *nlaunches_out = (int)plan.size();
        for (int l = 0; l < (int)plan.size(); ++l) {
            const FiberLaunch& L = plan[l];
            if (launches && l < cap) { const int v[10] = {(int)L.route, L.D, L.K, L.TR, L.tpw, L.KKmax, L.NNmax, L.wgs, (int)L.items.size(), L.general ? 1 : 0}; std::copy(v, v + 10, launches + 10 * l); }
            if (items_out) for (size_t k = 0; k < L.items.size(); ++k) { const FiberItem& it = L.items[k]; const int v[7] = {l, it.tile_begin, L.nwg[k], it.TA, it.TB, it.nta, it.ntb}; std::copy(v, v + 7, items_out + 7 * L.index[k]); }
        }
    });
}

extern "C" int tnqs_dbg_fiber_gemm(int dtype, int D, int PA, int K, int PB, int Do, int No, const void* in, const void* X, void* out, double* norm2, int use_mfma) {
    return guard([&] {
        need_gpu();
        const size_t esz = esz_of(dtype);
        size_t nin = (size_t)D * PA * K * PB, nout = (size_t)Do * PA * No * PB, nx = (size_t)D * K * Do * No;
        DBuf dIn(nin * esz), dX(nx * esz), dOut(nout * esz); DevItems<FiberItem> dI(1);
        dIn.up(in, nin * esz); dX.up(X, nx * esz);
        HIPCHK(hipMemset(dOut.p, 0xff, nout * esz));
        FiberItem it{}; it.in = dIn.p; it.out = dOut.p; it.X = dX.p; it.D = D; it.PA = PA; it.K = K; it.PB = PB; it.Do = Do; it.No = No;
        it.want_norm = 1;
        // laid out by the engine's planner under this entry point's own rules: the epilogue's (general f64 kernel) without RowGemm and without the lower bound of
        // the f32 matrix-core route, tiles per workgroup forced to values that do not divide the tile counts of the tests
        FiberRules r = fiber_rules(FiberUse::Epilogue, dtype == TNQS_C64, use_mfma != 0, true); r.rg_D = 0; r.kk_min = 1; r.mfma_tpw = 5; r.f64_tpw = 12;
        const std::vector<FiberLaunch> plan = plan_fiber_pass(&it, 1, r, esz);
        const FiberLaunch& L = plan[0]; const int tiles = L.wgs;
        DBuf dN((size_t)tiles * 8);
        dI.up(L.items[0]);
        by_dtype(dtype, [&](auto t) { launch_fiber_route<decltype(t)>(nullptr, L, dI.get(), (double*)dN.p); });
        HIPCHK(hipDeviceSynchronize());
        dOut.down(out, nout * esz);
        if (norm2) { std::vector<double> np(tiles); dN.down(np.data(), (size_t)tiles * 8); double t = 0; for (double v : np) t += v; *norm2 = t; }
    });
}

extern "C" int tnqs_dbg_gram(int dtype, int D, int PA, int K, int PB, const void* X, const void* Y, void* out, int acc64, int use_mfma) {
    return guard([&] {
        need_gpu();
        const size_t esz = esz_of(dtype);
        size_t nin = (size_t)D * PA * K * PB; int KK = D * K;
        bool same = (X == Y);
        DBuf dX(nin * esz), dY(same ? 1 : nin * esz); DevItems<GramItem> dI(1); DevItems<ReduceItem> dR(1);
        dX.up(X, nin * esz); if (!same) dY.up(Y, nin * esz);
        GramItem it{}; it.X = dX.p; it.Y = same ? dX.p : dY.p; it.D = D; it.PA = PA; it.K = K; it.PB = PB;
        // the engine's rule (gram_route, kernels.hip) on this one item, except where the tests of this entry ask for a kernel the rule would not give it: with f32
        // accumulation Mfma32 below the rule's floor of D K = 8 as well and the vector kernel for 32 < D K <= 64; the vector kernel for 64 < D K <= 128 with f64
        // accumulation (Mfma64 and F64x128 have their own entry, tnqs_dbg_gram_mfma)
        GramRoute r = gram_route(dtype == TNQS_C64, acc64 || dtype == TNQS_C128, false, same, gram_f64in_covers(D, K), (size_t)KK, use_mfma != 0, true);
        if (use_mfma && dtype == TNQS_C64 && !acc64) r = KK <= 32 ? GramRoute::Mfma32 : GramRoute::Generic;
        if (r == GramRoute::F64x128) r = GramRoute::Generic;
        const int TR = gram_tile_rows(r, KK, esz);
        tile_params(PA, PB, TR, it.TA, it.TB, it.nta, it.ntb);
        const char* e = std::getenv("TNQS_DBG_GRAM_CHUNKS");
        int npart = 0; plan_gram(&it, 1, r, false, e ? std::max(1, std::atoi(e)) : 7, &npart);
        bool a64 = acc64 || dtype == TNQS_C128;
        size_t asz = a64 ? 16 : 8;
        DBuf dP((size_t)npart * KK * KK * asz), dO((size_t)KK * KK * asz);
        it.partial = dP.p; dI.up(it);
        if (dtype == TNQS_C128) launch_gram_route<double, double>(nullptr, r, dI.get(), 1, it.nchunks, TR, KK, KK == 64);
        else if (a64) launch_gram_route<float, double>(nullptr, r, dI.get(), 1, it.nchunks, TR, KK, KK == 64);
        else launch_gram_route<float, float>(nullptr, r, dI.get(), 1, it.nchunks, TR, KK);
        dR.up(ReduceItem{dP.p, dO.p, KK * KK, npart, 0, 0});
        if (a64) launch_reduce<double, double>(nullptr, dR.get(), 1, KK * KK); else launch_reduce<float, float>(nullptr, dR.get(), 1, KK * KK);
        HIPCHK(hipDeviceSynchronize());
        dO.down(out, (size_t)KK * KK * asz);
    });
}

extern "C" int tnqs_dbg_gram_fused(int PA, int K, int PB, const void* X, const void* Y, const void* M, void* out) {
    return guard([&] {
        need_gpu();
        size_t nin = (size_t)PA * K * PB;
        DBuf dX(nin * 8), dY(nin * 8), dM(32 * 32 * 8); DevItems<GramItem> dI(1); DevItems<ReduceItem> dR(1);
        dX.up(X, nin * 8); dY.up(Y, nin * 8); dM.up(M, 32 * 32 * 8);
        GramItem it{}; it.X = dX.p; it.Y = dY.p; it.M = dM.p; it.D = 1; it.PA = PA; it.K = K; it.PB = PB;
        tile_params(PA, PB, 64, it.TA, it.TB, it.nta, it.ntb);
        if (it.TA * it.TB != 64) throw Err(TNQS_ERR_INVALID, "dbg_gram_fused: tiles must hold 64 fibers");
        int npart = 0; plan_gram(&it, 1, GramRoute::Fused32, false, 3, &npart);
        DBuf dP((size_t)npart * K * K * 8), dO((size_t)K * K * 8);
        it.partial = dP.p; dI.up(it);
        launch_gram_route<float, float>(nullptr, GramRoute::Fused32, dI.get(), 1, it.nchunks, 64, K);
        dR.up(ReduceItem{dP.p, dO.p, K * K, npart, 0, 0});
        launch_reduce<float, float>(nullptr, dR.get(), 1, K * K);
        HIPCHK(hipDeviceSynchronize());
        dO.down(out, (size_t)K * K * 8);
    });
}
// the gate path's fused gauge + f64 Gram kernels (kernels_gate.hip) on one site tensor: out[i + KK j] = sum_fibers X'[i, .] conj(X'[j, .]),
// X' = X x_r M with r the lowest leg that is not the bond leg, (i, j) = (s, k); chi_b = 32 (mfma_gauge_gram64_kernel) or 16 (mfma_gauge_gram32_kernel)
extern "C" int tnqs_dbg_gauge_gram(int z, const int* chi, int bleg, const void* X, const void* M, void* out) {
    return guard([&] {
        need_gpu();
        if (z < 2 || z > 8 || bleg < 0 || bleg >= z) throw Err(TNQS_ERR_INVALID, "dbg_gauge_gram: bad shape");
        const int rleg = bleg == 0 ? 1 : 0, K = chi[bleg], KK = 2 * K;
        const bool k16 = gauge_gram32_covers(2, z, chi, bleg, rleg), k32 = gauge_gram64_covers(2, z, chi, bleg, rleg);
        if (!k16 && !k32) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_gauge_gram: shape not covered by the fused kernels");
        size_t n = 2; for (int i = 0; i < z; ++i) n *= chi[i];
        long long PA = 1, PB = 1; for (int i = 0; i < bleg; ++i) PA *= chi[i]; for (int i = bleg + 1; i < z; ++i) PB *= chi[i];
        DBuf dX(n * 8), dM((size_t)chi[rleg] * chi[rleg] * 8); DevItems<GramItem> dI(1); DevItems<ReduceItem> dR(1);
        dX.up(X, n * 8); dM.up(M, (size_t)chi[rleg] * chi[rleg] * 8);
        GramItem it{}; it.X = dX.p; it.Y = dX.p; it.M = dM.p; it.D = 2; it.PA = (int)PA; it.K = K; it.PB = (int)PB;
        tile_params(PA, PB, 64, it.TA, it.TB, it.nta, it.ntb);
        if (k16) { it.nta = gauge_gram32_units(z, chi, bleg); it.ntb = 1; }
        const GramRoute r = k16 ? GramRoute::Gauge32 : GramRoute::Gauge64;
        int npart = 0; plan_gram(&it, 1, r, true, 5, &npart);
        DBuf dP((size_t)npart * KK * KK * 16), dO((size_t)KK * KK * 16);
        HIPCHK(hipMemset(dP.p, 0, (size_t)npart * KK * KK * 16));
        it.partial = dP.p; dI.up(it);
        launch_gram_route<float, double>(nullptr, r, dI.get(), 1, it.nchunks, 64, KK);
        dR.up(ReduceItem{dP.p, dO.p, KK * KK, npart, 0, 0});
        launch_reduce<double, double>(nullptr, dR.get(), 1, KK * KK);
        HIPCHK(hipDeviceSynchronize());
        dO.down(out, (size_t)KK * KK * 16);
    });
}

// ---- entry points that reach exactly the kernels of one engine launch: several items per launch, set up as the engine sets them up
// (fiber_plan.cpp, engine_batch.cpp run_chains / run_grams / svd_batch, engine_bp.cpp), a shape the named kernel does not
// take is refused (TNQS_ERR_UNSUPPORTED) and *route says which kernel ran (TNQS_DBG_ROUTE_*, include/tnqs_debug.h) ----

// register-direct fiber GEMM (launch_mfma_rowgemm): items i with (PA[i], PB[i], No[i]), one D and K for the launch; in / X / out are the items'
// arrays one after the other; norm2[i] = the sum of item i's norm partials; tpw <= 0: the engine's rule (D = 2: gate epilogue, D = 1: BP mode product)
extern "C" int tnqs_dbg_rowgemm(int D, int K, int nitems, const int* PA, const int* PB, const int* No, const void* in, const void* X, void* out, double* norm2, int tpw, int* route) {
    return guard([&] {
        need_gpu();
        if (nitems < 1 || !PA || !PB || !No) throw Err(TNQS_ERR_INVALID, "dbg_rowgemm: bad arguments");
        std::vector<FiberItem> items(nitems);
        for (int i = 0; i < nitems; ++i) {
            FiberItem& it = items[i]; it.D = D; it.PA = PA[i]; it.K = K; it.PB = PB[i]; it.Do = D; it.No = No[i];
            if (PA[i] < 1 || PB[i] < 1 || !rowgemm_covers(it)) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_rowgemm: item not covered by the register-direct kernels");
            it.want_norm = 1;
        }
        std::vector<size_t> oi, ox, oo;
        cat_offsets(nitems, oi, [&](int i) { return (size_t)D * PA[i] * K * PB[i]; });
        cat_offsets(nitems, ox, [&](int i) { return (size_t)D * K * D * No[i]; });
        cat_offsets(nitems, oo, [&](int i) { return (size_t)D * PA[i] * No[i] * PB[i]; });
        DBuf dIn(oi[nitems] * 8), dX(ox[nitems] * 8), dOut(oo[nitems] * 8); DevItems<FiberItem> dI(nitems);
        dIn.up(in, oi[nitems] * 8); dX.up(X, ox[nitems] * 8);
        HIPCHK(hipMemset(dOut.p, 0xff, oo[nitems] * 8));
        for (int i = 0; i < nitems; ++i) {
            FiberItem& it = items[i];
            it.in = (char*)dIn.p + oi[i] * 8; it.X = (char*)dX.p + ox[i] * 8; it.out = (char*)dOut.p + oo[i] * 8;
        }
        // the engine's plan of the pass (D = 2: gate epilogue, D = 1: mode product), tpw forced when given: one RowGemm launch over all items
        FiberRules r = fiber_rules(D == 2 ? FiberUse::Epilogue : FiberUse::Chain, true, true, true); r.rg_tpw = tpw;
        const std::vector<FiberLaunch> plan = plan_fiber_pass(items.data(), nitems, r, 8);
        const FiberLaunch& L = plan[0]; const int wgs = L.wgs;
        if (L.route != FiberRoute::RowGemm || (int)L.items.size() != nitems) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_rowgemm: item not covered by the register-direct kernels");
        DBuf dN((size_t)wgs * 8);
        dI.up(L.items);
        launch_fiber_route<float>(nullptr, L, dI.get(), (double*)dN.p);
        HIPCHK(hipDeviceSynchronize());
        dOut.down(out, oo[nitems] * 8);
        std::vector<double> np(wgs); dN.down(np.data(), (size_t)wgs * 8);
        for (int i = 0; i < nitems; ++i) {
            double t = 0; for (int w = 0; w < L.nwg[i]; ++w) t += np[L.items[i].tile_begin + w];
            if (norm2) norm2[i] = t;
        }
        if (route) *route = (D * K == 64 && mfma_use_x3()) ? TNQS_DBG_ROUTE_X3 : TNQS_DBG_ROUTE_F32;
    });
}

// matrix-core Grams of 32 < KK <= 64 (launch_mfma_gram64, f32 accumulation, complex64 out; the BP message Gram) and 64 < KK <= 128
// (launch_mfma_gram128_f64, X == Y, complex128 out; the gate-path Gram at chi = 64).  shape: (D, PA, K, PB) per item; Y == NULL: X == Y;
// nchunks <= 0: the engine's chunking (run_grams), else at most that many chunks per item; partials summed with launch_reduce
extern "C" int tnqs_dbg_gram_mfma(int nitems, const int* shape, const void* X, const void* Y, void* out, int nchunks, int* route) {
    return guard([&] {
        need_gpu();
        if (nitems < 1 || !shape) throw Err(TNQS_ERR_INVALID, "dbg_gram_mfma: bad arguments");
        int KKmax = 0; bool all128 = true;
        for (int i = 0; i < nitems; ++i) {
            const int* q = shape + 4 * i;
            if (q[0] < 1 || q[1] < 1 || q[2] < 1 || q[3] < 1) throw Err(TNQS_ERR_INVALID, "dbg_gram_mfma: bad shape");
            KKmax = std::max(KKmax, q[0] * q[2]); all128 = all128 && q[0] * q[2] == 128;
        }
        const bool f64 = KKmax > 64;
        if (KKmax <= 32 || KKmax > 128) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_gram_mfma: 32 < D K <= 128");
        if (f64 && Y) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_gram_mfma: the 128 x 128 f64 Gram takes X == Y only");
        const size_t asz = f64 ? 16 : 8;
        std::vector<size_t> oi, oo;
        cat_offsets(nitems, oi, [&](int i) { const int* q = shape + 4 * i; return (size_t)q[0] * q[1] * q[2] * q[3]; });
        cat_offsets(nitems, oo, [&](int i) { const int* q = shape + 4 * i; return (size_t)q[0] * q[2] * q[0] * q[2]; });
        DBuf dX(oi[nitems] * 8), dY(Y ? oi[nitems] * 8 : 1), dO(oo[nitems] * asz); DevItems<GramItem> dI(nitems); DevItems<ReduceItem> dR(nitems);
        dX.up(X, oi[nitems] * 8); if (Y) dY.up(Y, oi[nitems] * 8);
        const GramRoute r = f64 ? GramRoute::F64x128 : GramRoute::Mfma64;
        std::vector<GramItem> items(nitems); std::vector<size_t> op(nitems + 1, 0); std::vector<int> npart(nitems);
        for (int i = 0; i < nitems; ++i) {
            const int* q = shape + 4 * i; GramItem& it = items[i];
            it.X = (char*)dX.p + oi[i] * 8; it.Y = Y ? (const void*)((char*)dY.p + oi[i] * 8) : it.X;
            it.D = q[0]; it.PA = q[1]; it.K = q[2]; it.PB = q[3];
            tile_params(it.PA, it.PB, 64, it.TA, it.TB, it.nta, it.ntb);
        }
        const int chunks = plan_gram(items.data(), nitems, r, f64, nchunks, npart.data());
        for (int i = 0; i < nitems; ++i) op[i + 1] = op[i] + (size_t)npart[i] * (oo[i + 1] - oo[i]);
        DBuf dP(op[nitems] * asz);
        std::vector<ReduceItem> ri(nitems);
        for (int i = 0; i < nitems; ++i) {
            items[i].partial = (char*)dP.p + op[i] * asz;
            ri[i] = ReduceItem{items[i].partial, (char*)dO.p + oo[i] * asz, (int)(oo[i + 1] - oo[i]), npart[i], 0, (int)oo[i]};
        }
        dI.up(items); dR.up(ri);
        if (f64) {
            launch_gram_route<float, double>(nullptr, r, dI.get(), nitems, chunks, 64, KKmax, all128);
            launch_reduce<double, double>(nullptr, dR.get(), nitems, (int)oo[nitems]);
        } else {
            launch_gram_route<float, float>(nullptr, r, dI.get(), nitems, chunks, 64, KKmax);
            launch_reduce<float, float>(nullptr, dR.get(), nitems, (int)oo[nitems]);
        }
        HIPCHK(hipDeviceSynchronize());
        dO.down(out, oo[nitems] * asz);
        if (route) *route = f64 ? (all128 ? TNQS_DBG_ROUTE_F64_SHARED : TNQS_DBG_ROUTE_F64) : (mfma_use_x3() ? TNQS_DBG_ROUTE_X3 : TNQS_DBG_ROUTE_F32);
    });
}

// ---- the ComplexF64 kernels of kernels_f64.hip as the engine launches them: items of different sizes in ONE launch, nothing refused for its shape (a launch
// the matrix-core kernel does not take runs on the generic vector kernel, as in the engine; *route says which) ----

// ONE ComplexF64 fiber pass: planned by plan_fiber_pass under the engine's rules of the use (tpw > 0: f64_tpw forced), launched through launch_fiber_route<double>
// as FiberPass::launch<double> does.  in == NULL: the plan alone (route, instantiation, workgroups per item), no device call
extern "C" int tnqs_dbg_fiber_pass_c128(int use, int use_mfma, int nitems, const int* shape, const int* want_norm, const void* in, const void* X, void* out, double* partials,
                                        int tpw, int guard_elems, int* route, int* inst, int* wg_begin, int* nwg) {
    return guard([&] {
        if (use < 0 || use > 1 || nitems < 1 || !shape || !want_norm || guard_elems < 0 || (in && (!X || !out || !partials))) throw Err(TNQS_ERR_INVALID, "dbg_fiber_pass_c128: bad arguments");
        std::vector<FiberItem> items(nitems);
        for (int i = 0; i < nitems; ++i) {
            const int* q = shape + 6 * i; for (int k = 0; k < 6; ++k) if (q[k] < 1) throw Err(TNQS_ERR_INVALID, "dbg_fiber_pass_c128: bad shape");
            if ((long long)q[0] * q[1] * q[2] * q[3] > INT_MAX / 16 || (long long)q[4] * q[1] * q[5] * q[3] > INT_MAX / 16 || (long long)q[0] * q[2] * q[4] * q[5] > INT_MAX / 16)
                throw Err(TNQS_ERR_INVALID, "dbg_fiber_pass_c128: bad shape");
            // a chain stage has no site index and no norm (site_fiber_item(sd, leg, false, chi, false)): the plain kernel ignores both
            if (use == 0 && (q[0] != 1 || q[4] != 1 || want_norm[i])) throw Err(TNQS_ERR_INVALID, "dbg_fiber_pass_c128: a chain stage has D = Do = 1 and no norm");
            FiberItem& it = items[i]; it = FiberItem{}; it.D = q[0]; it.PA = q[1]; it.K = q[2]; it.PB = q[3]; it.Do = q[4]; it.No = q[5]; it.want_norm = want_norm[i] ? 1 : 0;
        }
        FiberRules r = fiber_rules(use == 0 ? FiberUse::Chain : FiberUse::Epilogue, /*f32=*/false, use_mfma != 0, true); if (tpw > 0) r.f64_tpw = tpw;
        const std::vector<FiberLaunch> plan = plan_fiber_pass(items.data(), nitems, r, 16);
        if (plan.size() != 1 || (int)plan[0].items.size() != nitems || (plan[0].route != FiberRoute::F64 && plan[0].route != FiberRoute::Generic) || plan[0].wgs < 1)
            throw Err(TNQS_ERR_HIP, "internal: dbg_fiber_pass_c128: a ComplexF64 pass is one launch");
        const FiberLaunch& L = plan[0];
        const bool f64 = L.route == FiberRoute::F64;
        if (route) *route = !f64 ? TNQS_DBG_ROUTE_FIBER_GENERIC : L.general ? TNQS_DBG_ROUTE_FIBER_F64_GENERAL : TNQS_DBG_ROUTE_FIBER_F64_PLAIN;
        if (inst) { int nb = 0, ks = 0; if (f64) fiber_gemm_f64_inst(L.KKmax, L.NNmax, &nb, &ks); inst[0] = nb; inst[1] = ks; inst[2] = f64 && L.general ? 1 : 0; }
        for (int k = 0; k < nitems; ++k) { if (wg_begin) wg_begin[L.index[k]] = L.items[k].tile_begin; if (nwg) nwg[L.index[k]] = L.nwg[k]; }
        if (!in) return;
        need_gpu();
        Slots sIn, sX; Guarded gO((size_t)guard_elems * 16), gP((size_t)guard_elems * 8);
        for (const FiberItem& it : items) {
            sIn.add((size_t)it.D * it.PA * it.K * it.PB * 16); sX.add((size_t)it.D * it.K * it.Do * it.No * 16); gO.add((size_t)it.Do * it.PA * it.No * it.PB * 16);
        }
        gP.add((size_t)L.wgs * 8);
        alloc_all(sIn, sX, gO, gP); put_all(sIn, in); put_all(sX, X);
        std::vector<FiberItem> li = L.items;
        for (int k = 0; k < nitems; ++k) { const int i = L.index[k]; li[k].in = sIn.at(i); li[k].X = sX.at(i); li[k].out = gO.at(i); }
        DevItems<FiberItem> dI(li);
        up_all(sIn, sX); gO.up(out); gP.up(partials);
        launch_fiber_route<double>(nullptr, L, dI.get(), (double*)gP.at(0));
        HIPCHK(hipDeviceSynchronize());
        gO.down(out, "out"); gP.down(partials, "the norm partials");
    });
}

// ONE ComplexF64 Gram launch + the chunk sum, set up as run_grams<double, double> sets it up: route from gram_route, tiles from gram_tile_rows / tile_params, chunks
// from plan_gram.  X == NULL: route and chunk counts alone, no device call
extern "C" int tnqs_dbg_gram_c128(int use_mfma, int nitems, const int* shape, const int* same, const void* X, const void* Y, void* out, int max_chunks, int* nchunks_out,
                                  int guard_elems, int* route) {
    return guard([&] {
        if (nitems < 1 || !shape || !same || guard_elems < 0 || (X && !out)) throw Err(TNQS_ERR_INVALID, "dbg_gram_c128: bad arguments");
        std::vector<GramItem> items(nitems);
        size_t KKmax = 1; bool all_same = true, f64in = true, all_full = true;
        for (int i = 0; i < nitems; ++i) {
            const int* q = shape + 4 * i;
            if (q[0] < 1 || q[1] < 1 || q[2] < 1 || q[3] < 1 || (long long)q[0] * q[1] * q[2] * q[3] > INT_MAX / 16 || (long long)q[0] * q[2] > 4096) throw Err(TNQS_ERR_INVALID, "dbg_gram_c128: bad shape");
            if (X && !same[i] && !Y) throw Err(TNQS_ERR_INVALID, "dbg_gram_c128: Y == NULL needs every item `same`");
            GramItem& it = items[i]; it = GramItem{}; it.D = q[0]; it.PA = q[1]; it.K = q[2]; it.PB = q[3];
            KKmax = std::max(KKmax, (size_t)q[0] * q[2]); all_same = all_same && same[i] != 0; f64in = f64in && gram_f64in_covers(q[0], q[2]); all_full = all_full && q[0] * q[2] == 64;
        }
        const GramRoute r = gram_route(/*f32=*/false, /*acc64=*/true, false, all_same, f64in, KKmax, use_mfma != 0, true);
        if (r != GramRoute::F64In && r != GramRoute::Generic) throw Err(TNQS_ERR_HIP, "internal: dbg_gram_c128: route of a ComplexF64 Gram");
        const int TR = gram_tile_rows(r, KKmax, 16);
        for (GramItem& it : items) tile_params(it.PA, it.PB, TR, it.TA, it.TB, it.nta, it.ntb);
        std::vector<int> npart(nitems);
        const int chunks = plan_gram(items.data(), nitems, r, false, max_chunks, npart.data());
        if (route) *route = r == GramRoute::F64In ? TNQS_DBG_ROUTE_GRAM_F64IN : TNQS_DBG_ROUTE_GRAM_GENERIC;
        if (nchunks_out) std::copy(npart.begin(), npart.end(), nchunks_out);
        if (!X) return;
        need_gpu();
        const size_t band = 256;                       // guard band behind every item's partials (and in front of the first), 0xff like the gaps
        Slots sX, sY, sP(band); Guarded gO((size_t)guard_elems * 16);
        for (int i = 0; i < nitems; ++i) {
            const GramItem& it = items[i]; const size_t nin = (size_t)it.D * it.PA * it.K * it.PB, n2 = (size_t)it.D * it.K * it.D * it.K;
            sX.add(nin * 16); sY.add(same[i] ? 0 : nin * 16); sP.add((size_t)npart[i] * n2 * 16); gO.add(n2 * 16);
        }
        alloc_all(sX, sY, sP, gO); put_all(sX, X);
        std::vector<ReduceItem> ri(nitems); size_t yo = 0, eb = 0;
        for (int i = 0; i < nitems; ++i) {
            GramItem& it = items[i]; const size_t nin = (size_t)it.D * it.PA * it.K * it.PB; const int n2 = it.D * it.K * it.D * it.K;
            if (!same[i]) sY.put(i, (const char*)Y + yo);
            yo += nin * 16;
            it.X = sX.at(i); it.Y = same[i] ? sX.at(i) : sY.at(i); it.partial = sP.at(i);
            ri[i] = ReduceItem{sP.at(i), gO.at(i), n2, npart[i], 0, (int)eb}; eb += n2;
        }
        DevItems<GramItem> dI(items); DevItems<ReduceItem> dR(ri);
        up_all(sX, sY, sP); gO.up(out);
        launch_gram_route<double, double>(nullptr, r, dI.get(), nitems, chunks, TR, (int)KKmax, all_full);
        launch_reduce<double, double>(nullptr, dR.get(), nitems, (int)eb);
        HIPCHK(hipDeviceSynchronize());
        sP.down("the Gram partials");
        auto untouched = [&](size_t b0, size_t b1) { for (size_t b = b0; b < b1; ++b) if (sP.host[b] != (char)0xff) throw Err(TNQS_ERR_INVALID, "dbg: a kernel wrote outside an item of the Gram partials"); };
        untouched(0, band);
        for (int i = 0; i < nitems; ++i) untouched(sP.off[i] + sP.len[i], sP.off[i] + sP.len[i] + band);
        gO.down(out, "out");
    });
}

// HOST ONLY: gram_route (kernels.hip) on the values given
extern "C" int tnqs_dbg_gram_route(int dtype, int acc64, int has_m, int all_same, int all_f64in, int kkmax, int use_mfma, int use_chi64, int* route) {
    return guard([&] {
        if (!is_dtype(dtype) || kkmax < 1 || !route) throw Err(TNQS_ERR_INVALID, "tnqs_dbg_gram_route: bad arguments");
        *route = (int)gram_route(dtype == TNQS_C64, acc64 != 0, has_m != 0, all_same != 0, all_f64in != 0, (size_t)kkmax, use_mfma != 0, use_chi64 != 0);
    });
}
