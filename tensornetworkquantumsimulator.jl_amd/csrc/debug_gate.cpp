// debug_gate.cpp -- kernel-level test entry points (include/tnqs_debug.h) of the gate path: the step schedule of apply_gates (gate_schedule.cpp), the per-gate small
// algebra (kernels_theta.hip, gate_theta.cpp), the SVD stage (gate_svd.cpp), the second factorisation pass and the small-SVD route (kernels_svd.hip).
#include "debug_util.hpp"

using namespace tnqs;

// HOST ONLY: the step schedule tnqs_apply_gates walks, from the graph and the gates' vertex lists alone
extern "C" int tnqs_dbg_gate_schedule(int nv, int ne, const int32_t* esrc, const int32_t* edst, int ngates, const int32_t* nverts, const int32_t* verts, int update_cache,
                                      int* step_of_gate, int* step_is_bp, int cap, int* nsteps_out) {
    return guard([&] {
        if (nv < 0 || ne < 0 || (ne > 0 && (!esrc || !edst)) || ngates < 0 || (ngates > 0 && (!nverts || !verts)) || !nsteps_out) throw Err(TNQS_ERR_INVALID, "tnqs_dbg_gate_schedule: bad arguments");
        for (int i = 0, o = 0; i < ngates; o += nverts[i], ++i) {
            if (nverts[i] < 1 || nverts[i] > 2) throw Err(TNQS_ERR_INVALID, "tnqs_dbg_gate_schedule: only one- and two-site gates");
            for (int k = 0; k < nverts[i]; ++k) if (verts[o + k] < 0 || verts[o + k] >= nv) throw Err(TNQS_ERR_INVALID, "tnqs_dbg_gate_schedule: vertex out of range");
        }
        auto g = dbg_make_graph(nv, ne, esrc, edst); const GateSchedule steps = build_gate_schedule(*g, ngates, nverts, verts, update_cache != 0); *nsteps_out = (int)steps.size();
        for (int k = 0; k < (int)steps.size(); ++k) {
            if (step_is_bp && k < cap) step_is_bp[k] = steps[k].is_bp ? 1 : 0;
            if (step_of_gate) for (int i = steps[k].begin; i < steps[k].end; ++i) step_of_gate[i] = k;
        }
    });
}

// ---- the gate path's per-gate small algebra (kernels_theta.hip and the small_svd_* kernels of kernels_svd.hip): ONE launch of every kernel over nitems gates / sites of
// different sizes.  The route rule, the launch chain and the item fills are the engine's own (gate_theta.cpp: theta_route, launch_theta_chain, small_svd_items /
// launch_small_svd, Qr2Site); what is written here is where the arrays live.  Inputs: the items' arrays one after the other, every sub-array at a multiple of 256 bytes on
// the device.  Outputs: guard bands (debug_util.hpp).  The small integer arrays (info, texp, failure flags, ranks) are contiguous per launch as in the engine's read-back
// buffer: they go up as filled and come back ----
namespace {
struct GateDims : ThetaRoute { int d1, d2, chi; };
// item i as the engine sees it: dimensions, the refusal of d^2 chi > 512, cap, and -- given the gate's kappa -- the route
GateDims gate_dims(const char* who, bool F32, const int* dims, int i, int kappa = 0, int maxdim = 0) {
    GateDims g; g.d1 = dims[3 * i]; g.d2 = dims[3 * i + 1]; g.chi = dims[3 * i + 2];
    if (g.d1 < 1 || g.d2 < 1 || g.chi < 1) throw Err(TNQS_ERR_INVALID, std::string(who) + ": d1, d2, chi >= 1");
    static_cast<ThetaRoute&>(g) = theta_route(F32, g.d1, g.d2, g.chi, kappa, maxdim);
    return g;
}
const void* upload_dbuf(void* keep, const void* p, size_t bytes) {      // DescUpload into a plain device allocation that lives as long as `keep`
    auto& k = *static_cast<std::vector<std::unique_ptr<DBuf>>*>(keep);
    k.emplace_back(new DBuf(bytes)); k.back()->up(p, bytes); return k.back()->p;
}
}  // namespace
// HOST ONLY: the operator-sum factors of a two-site gate as gate_items() gets them
extern "C" int tnqs_dbg_operator_sum(const void* gate, int d1, int d2, int* kappa_out, void* fa_out, void* fb_out) {
    return guard([&] {
        if (!kappa_out) throw Err(TNQS_ERR_INVALID, "dbg_operator_sum: null output");
        if (!gate || d1 < 1 || d2 < 1 || d1 > 16 || d2 > 16) throw Err(TNQS_ERR_INVALID, "dbg_operator_sum: bad arguments");
        std::vector<std::complex<double>> fa, fb;
        *kappa_out = operator_sum(reinterpret_cast<const double*>(gate), d1, d2, fa, fb);
        if (fa_out && !fa.empty()) std::memcpy(fa_out, fa.data(), fa.size() * 16);
        if (fb_out && !fb.empty()) std::memcpy(fb_out, fb.data(), fb.size() * 16);
    });
}
// TwoSiteBatch::run_theta's launch_theta_chain up to stage stop_after.  info == NULL: only low_sizes is filled (host only)
extern "C" int tnqs_dbg_gate_theta(int dtype, int nitems, const int* dims, const int* mode, const int* rk, const void* F1, const void* F2, const double* tau, const void* gate,
                                   const int* maxdim, int lowrank_on, int stop_after, int* low_sizes, int* info, double* lam1, double* lam2, int* idx1, int* idx2,
                                   void* theta, void* theta0, void* thetaV, void* lowA, void* lowB, void* lowG, void* lowL, void* lowQ, void* lowL2c, int* texp, int* lowfail, int guard_elems) {
    return guard([&] {
        if (!is_dtype(dtype) || nitems < 1 || !dims || !mode || !rk || !F1 || !F2 || !tau || !gate || !maxdim || !low_sizes || stop_after < 0 || stop_after > 3 || guard_elems < 0)
            throw Err(TNQS_ERR_INVALID, "dbg_gate_theta: bad arguments");
        const bool F32 = dtype == TNQS_C64; const size_t esz = esz_of(dtype);
        std::vector<GateDims> gd(nitems); std::vector<int> kappa(nitems, 0);
        std::vector<std::vector<std::complex<double>>> fa(nitems), fb(nitems);
        const char* hg = (const char*)gate; std::vector<size_t> goff(nitems + 1, 0);
        for (int i = 0; i < nitems; ++i) {
            gd[i] = gate_dims("dbg_gate_theta", F32, dims, i);
            for (int sd = 0; sd < 2; ++sd) {
                const int m = mode[2 * i + sd], n = sd ? gd[i].n2 : gd[i].n1;
                if (m < 0 || m > 2 || (m == 2 && (rk[2 * i + sd] < 0 || rk[2 * i + sd] > n))) throw Err(TNQS_ERR_INVALID, "dbg_gate_theta: mode in {0, 1, 2}, 0 <= rk <= n");
            }
            const size_t dd = (size_t)gd[i].d1 * gd[i].d2; goff[i + 1] = goff[i] + dd * dd * 16;
        }
        for (int i = 0; i < nitems; ++i) {      // the operator sum, and what theta_route hands out for it
            if (lowrank_on) kappa[i] = operator_sum(reinterpret_cast<const double*>(hg + goff[i]), gd[i].d1, gd[i].d2, fa[i], fb[i]);
            const ThetaRoute& r = gd[i] = gate_dims("dbg_gate_theta", F32, dims, i, kappa[i], maxdim[i]);
            int* z = low_sizes + 6 * i;
            z[0] = (int)r.nA; z[1] = (int)r.nB; z[2] = z[3] = (int)r.nG; z[4] = (int)r.nQ; z[5] = 2 * (int)r.nG2;
        }
        if (!info) return;
        if (!lam1 || !lam2 || !idx1 || !idx2 || !theta || !theta0 || !thetaV || !lowA || !lowB || !lowG || !lowL || !lowQ || !lowL2c || !texp || !lowfail)
            throw Err(TNQS_ERR_INVALID, "dbg_gate_theta: null output");
        need_gpu();
        const size_t gb = (size_t)guard_elems;
        Slots sF1, sF2, sGate, sOp, sRk, sW, sB1, sG2;
        Guarded gLam1(gb * 8), gLam2(gb * 8), gIdx1(gb * 4), gIdx2(gb * 4), gTh(gb * esz), gTh0(gb * esz), gTv(gb * esz), gA(gb * 16), gB(gb * 16), gG(gb * 16), gL(gb * 16), gQ(gb * 16), gL2c(gb * 16);
        for (int i = 0; i < nitems; ++i) {
            const GateDims& g = gd[i];
            for (int k = 0; k < 3; ++k) { sF1.add((size_t)g.n1 * g.n1 * 16); sF2.add((size_t)g.n2 * g.n2 * 16); }
            sGate.add(goff[i + 1] - goff[i]); sOp.add(fa[i].size() * 16); sOp.add(fb[i].size() * 16); sRk.add(8);
            sW.add(g.nG * 16); sB1.add(g.nB1 * 16); sG2.add(g.nG2 * 16);
            gLam1.add((size_t)g.n1 * 8); gLam2.add((size_t)g.n2 * 8); gIdx1.add((size_t)g.n1 * 4); gIdx2.add((size_t)g.n2 * 4);
            const size_t mx = (size_t)std::max(g.Mr, g.Nc);
            gTh.add((size_t)g.Mr * g.Nc * esz); gTh0.add((size_t)g.Mr * g.Nc * esz); gTv.add(mx * mx * esz);
            gA.add(g.nA * 16); gB.add(g.nB * 16); gG.add(g.nG * 16); gL.add(g.nG * 16); gQ.add(g.nQ * 16); gL2c.add(2 * g.nG2 * 16);      // lowL2c: L2, then Lc
        }
        alloc_all(sF1, sF2, sGate, sOp, sRk, sW, sB1, sG2, gLam1, gLam2, gIdx1, gIdx2, gTh, gTh0, gTv, gA, gB, gG, gL, gQ, gL2c);
        put_all(sF1, F1); put_all(sF2, F2); put_all(sGate, gate);
        for (int i = 0; i < nitems; ++i) { if (!fa[i].empty()) { sOp.put(2 * i, fa[i].data()); sOp.put(2 * i + 1, fb[i].data()); } sRk.put(i, rk + 2 * i); }
        DBuf dInfo(32 * (size_t)nitems), dFail(8 * (size_t)nitems), dTexp(4 * (size_t)nitems);
        HIPCHK(hipMemset(dInfo.p, 0, 32 * (size_t)nitems)); HIPCHK(hipMemset(dFail.p, 0, 8 * (size_t)nitems));      // as run_theta zeroes them in front of the chain
        up_ints(dTexp, texp, nitems);
        std::vector<GateItem> gitems(nitems); std::vector<ThetaLowWs> lows(nitems);
        for (int i = 0; i < nitems; ++i) {
            const GateDims& g = gd[i]; const ThetaRoute& r = g; GateItem& it = gitems[i]; it = GateItem{};
            it.GA1 = sF1.at(3 * i); it.GV1 = sF1.at(3 * i + 1); it.GW1 = sF1.at(3 * i + 2); it.GA2 = sF2.at(3 * i); it.GV2 = sF2.at(3 * i + 1); it.GW2 = sF2.at(3 * i + 2);
            it.chol1 = mode[2 * i]; it.chol2 = mode[2 * i + 1]; it.n1 = r.n1; it.n2 = r.n2; it.d1 = g.d1; it.d2 = g.d2; it.chi = g.chi;
            it.gate = reinterpret_cast<const double*>(sGate.at(i));
            if (r.opsum) {
                it.kappa = kappa[i]; it.opA = reinterpret_cast<const double*>(sOp.at(2 * i)); it.opB = reinterpret_cast<const double*>(sOp.at(2 * i + 1));
                it.lowA = gA.at(i); it.lowB = gB.at(i);
            }
            if (r.low) {
                it.lowG = gG.at(i); it.lowL = gL.at(i);
                if (r.lowq) { it.lowW = sW.at(i); it.lowQ = gQ.at(i); }
                lows[i] = ThetaLowWs{sW.at(i), sB1.at(i), sG2.at(i), gL2c.at(i), gL2c.at(i) + r.nG2 * 16};
            }
            it.lam1 = (double*)gLam1.at(i); it.lam2 = (double*)gLam2.at(i); it.idx1 = (int*)gIdx1.at(i); it.idx2 = (int*)gIdx2.at(i);
            it.theta = gTh.at(i); it.thetaV = gTv.at(i); it.theta0 = gTh0.at(i);
            it.maxdim = maxdim[i]; it.chi_cap = r.cap;
            it.tau1 = tau[2 * i]; it.tau2 = tau[2 * i + 1];
            it.rk1 = mode[2 * i] == 2 ? (const int*)sRk.at(i) : nullptr; it.rk2 = mode[2 * i + 1] == 2 ? (const int*)sRk.at(i) + 1 : nullptr;
            it.info = (int*)dInfo.p + 8 * i; it.lowfail = (const int*)dFail.p + i; it.texp = (int*)dTexp.p + i;
        }
        DevItems<GateItem> dI(gitems);
        up_all(sF1, sF2, sGate, sOp, sRk, sW, sB1, sG2);
        gLam1.up(lam1); gLam2.up(lam2); gIdx1.up(idx1); gIdx2.up(idx2); gTh.up(theta); gTh0.up(theta0); gTv.up(thetaV);
        gA.up(lowA); gB.up(lowB); gG.up(lowG); gL.up(lowL); gQ.up(lowQ); gL2c.up(lowL2c);
        std::vector<std::unique_ptr<DBuf>> keep;
        const DescUpload up{upload_dbuf, &keep};
        by_dtype(dtype, [&](auto t) { launch_theta_chain<decltype(t)>(nullptr, dI.get(), gitems, lows, (int*)dFail.p, (int*)dFail.p + nitems, up, stop_after); });
        HIPCHK(hipDeviceSynchronize());
        sW.down("lowW"); sB1.down("lowB1"); sG2.down("lowG2");
        gLam1.down(lam1, "lam1"); gLam2.down(lam2, "lam2"); gIdx1.down(idx1, "idx1"); gIdx2.down(idx2, "idx2"); gTh.down(theta, "theta"); gTh0.down(theta0, "theta0"); gTv.down(thetaV, "thetaV");
        gA.down(lowA, "lowA"); gB.down(lowB, "lowB"); gG.down(lowG, "lowG"); gL.down(lowL, "lowL"); gQ.down(lowQ, "lowQ"); gL2c.down(lowL2c, "lowL2c");
        dInfo.down(info, 32 * (size_t)nitems); dTexp.down(texp, 4 * (size_t)nitems);
        std::vector<int> hf(2 * (size_t)nitems); dFail.down(hf.data(), 8 * (size_t)nitems);
        for (int i = 0; i < nitems; ++i) { lowfail[2 * i] = hf[i]; lowfail[2 * i + 1] = hf[nitems + i]; }
    });
}
// gate_finish_kernel<T> alone, on what the SVD stage leaves: theta_i (ld x ncol rotated columns, ld = max, ncol = min of (r1 d1, r2 d2)), thetaV_i (ncol x ncol)
extern "C" int tnqs_dbg_gate_finish(int dtype, int nitems, const int* dims, const int* info_in, const int* texp, const void* theta, const void* thetaV, const double* lam1, const double* lam2,
                                    const int* idx1, const int* idx2, const void* GW1, const void* GW2, const int* maxdim, const double* cutoff, const int* normalize, const int* chi_cap,
                                    double* S, int* info_out, double* truncerr, void* X1, void* X2, int guard_elems) {
    return guard([&] {
        if (!is_dtype(dtype) || nitems < 1 || !dims || !info_in || !texp || !theta || !thetaV || !lam1 || !lam2 || !idx1 || !idx2 || !GW1 || !GW2 || !maxdim || !cutoff ||
            !normalize || !chi_cap || !S || !info_out || !truncerr || !X1 || !X2 || guard_elems < 0) throw Err(TNQS_ERR_INVALID, "dbg_gate_finish: bad arguments");
        const bool F32 = dtype == TNQS_C64; const size_t esz = esz_of(dtype);
        std::vector<GateDims> gd(nitems);
        Slots sTh, sTv, sLam1, sLam2, sIdx1, sIdx2, sW1, sW2; Guarded gS((size_t)guard_elems * 8), gX1(guard_elems * esz), gX2(guard_elems * esz);
        size_t i1 = 0, i2 = 0;
        for (int i = 0; i < nitems; ++i) {
            const GateDims g = gd[i] = gate_dims("dbg_gate_finish", F32, dims, i);
            const int r1 = info_in[4 * i], r2 = info_in[4 * i + 1], wide = info_in[4 * i + 2], K = info_in[4 * i + 3];
            if (r1 < 1 || r1 > g.n1 || r2 < 1 || r2 > g.n2) throw Err(TNQS_ERR_INVALID, "dbg_gate_finish: 1 <= r <= n");
            const int Mr = r1 * g.d1, Nc = r2 * g.d2, ncol = std::min(Mr, Nc);
            if ((wide != 0) != (Mr < Nc) || K < 0 || K > ncol || (K > 0 && wide) || chi_cap[i] < 1 || chi_cap[i] > g.cap || texp[i] < -120 || texp[i] > 120)
                throw Err(TNQS_ERR_INVALID, "dbg_gate_finish: inconsistent info / chi_cap / texp");
            for (int a = 0; a < r1; ++a) if (idx1[i1 + a] < 0 || idx1[i1 + a] >= g.n1) throw Err(TNQS_ERR_INVALID, "dbg_gate_finish: idx1 out of range");
            for (int c = 0; c < r2; ++c) if (idx2[i2 + c] < 0 || idx2[i2 + c] >= g.n2) throw Err(TNQS_ERR_INVALID, "dbg_gate_finish: idx2 out of range");
            i1 += g.n1; i2 += g.n2;
            sTh.add((size_t)Mr * Nc * esz); sTv.add((size_t)ncol * ncol * esz); sLam1.add((size_t)g.n1 * 8); sLam2.add((size_t)g.n2 * 8); sIdx1.add((size_t)g.n1 * 4); sIdx2.add((size_t)g.n2 * 4);
            sW1.add((size_t)g.n1 * g.n1 * 16); sW2.add((size_t)g.n2 * g.n2 * 16);
            gS.add((size_t)chi_cap[i] * 8); gX1.add((size_t)g.n1 * g.d1 * chi_cap[i] * esz); gX2.add((size_t)g.n2 * g.d2 * chi_cap[i] * esz);
        }
        need_gpu();
        alloc_all(sTh, sTv, sLam1, sLam2, sIdx1, sIdx2, sW1, sW2, gS, gX1, gX2);
        put_all(sTh, theta); put_all(sTv, thetaV); put_all(sLam1, lam1); put_all(sLam2, lam2); put_all(sIdx1, idx1); put_all(sIdx2, idx2); put_all(sW1, GW1); put_all(sW2, GW2);
        std::vector<int> hinfo(8 * (size_t)nitems, 0);
        for (int i = 0; i < nitems; ++i) {
            hinfo[8 * i] = info_in[4 * i]; hinfo[8 * i + 1] = info_in[4 * i + 1]; hinfo[8 * i + 5] = info_in[4 * i + 2] ? 1 : 0; hinfo[8 * i + 7] = info_in[4 * i + 3];
            hinfo[8 * i + 2] = info_out[2 * i]; hinfo[8 * i + 3] = info_out[2 * i + 1];
        }
        DBuf dInfo(32 * (size_t)nitems), dTexp(4 * (size_t)nitems), dTerr(8 * (size_t)nitems); DevItems<GateItem> dI(nitems);
        up_ints(dInfo, hinfo.data(), 8 * (size_t)nitems); up_ints(dTexp, texp, nitems); dTerr.up(truncerr, 8 * (size_t)nitems);
        std::vector<GateItem> gitems(nitems);
        for (int i = 0; i < nitems; ++i) {
            const GateDims& g = gd[i]; GateItem& it = gitems[i]; it = GateItem{};
            it.GW1 = sW1.at(i); it.GW2 = sW2.at(i); it.n1 = g.n1; it.n2 = g.n2; it.d1 = g.d1; it.d2 = g.d2; it.chi = g.chi;
            it.lam1 = (double*)sLam1.at(i); it.lam2 = (double*)sLam2.at(i); it.idx1 = (int*)sIdx1.at(i); it.idx2 = (int*)sIdx2.at(i);
            it.theta = sTh.at(i); it.thetaV = sTv.at(i); it.X1 = gX1.at(i); it.X2 = gX2.at(i); it.S = (double*)gS.at(i);
            it.info = (int*)dInfo.p + 8 * i; it.truncerr = (double*)dTerr.p + i; it.texp = (int*)dTexp.p + i;
            it.maxdim = maxdim[i]; it.cutoff = cutoff[i]; it.normalize = normalize[i]; it.chi_cap = chi_cap[i];
        }
        dI.up(gitems);
        up_all(sTh, sTv, sLam1, sLam2, sIdx1, sIdx2, sW1, sW2);
        gS.up(S); gX1.up(X1); gX2.up(X2);
        by_dtype(dtype, [&](auto t) { launch_gate_finish<decltype(t)>(nullptr, dI.get(), nitems); });
        HIPCHK(hipDeviceSynchronize());
        gS.down(S, "S"); gX1.down(X1, "X1"); gX2.down(X2, "X2");
        dInfo.down(hinfo.data(), 32 * (size_t)nitems); dTerr.down(truncerr, 8 * (size_t)nitems);
        for (int i = 0; i < nitems; ++i) { info_out[2 * i] = hinfo[8 * i + 2]; info_out[2 * i + 1] = hinfo[8 * i + 3]; }
    });
}
// TwoSiteBatch::svd_and_finish up to and including the recovery of V: launch_theta_svd_stage (gate_svd.cpp) once over nitems gates.  dims: (d1, d2, n1, n2) per item, the
// bounds n_s = d_s chi every buffer and (dyn) every launch is sized from; info: the 8 ints per item the device holds (r1, r2, -, -, -, -, -, K alive), which are also the host
// dims of the static regime.  theta == NULL: only route_out is filled (host only)
extern "C" int tnqs_dbg_theta_svd_stage(int dtype, int dyn, int nitems, const int* dims, const int* info, const int* K, const int* has_q, const void* Q, const int* rank_bounds, const int* cap,
                                        int recover_form, void* theta, void* theta0, void* thetaV, int* sweeps_out, int* route_out, int guard_elems) {
    return guard([&] {
        if (!is_dtype(dtype) || dyn < 0 || dyn > 1 || nitems < 1 || !dims || !info || !K || !has_q || !rank_bounds || !cap || recover_form < 0 || recover_form > 1 ||
            guard_elems < 0 || (theta && (!theta0 || !thetaV))) throw Err(TNQS_ERR_INVALID, "dbg_theta_svd_stage: bad arguments");
        static_assert(ThetaSvdPreLow == TNQS_DBG_ROUTE_SVD_PRE_LOWRANK && ThetaSvdPreTheta == TNQS_DBG_ROUTE_SVD_PRE_THETA && ThetaSvdLds == TNQS_DBG_ROUTE_SVD_LDS &&
                      ThetaSvdGlobal == TNQS_DBG_ROUTE_SVD_GLOBAL && ThetaSvdTall == TNQS_DBG_ROUTE_SVD_TALL, "theta_svd_route returns the header's values");
        const bool F32 = dtype == TNQS_C64; const size_t esz = esz_of(dtype);
        std::vector<ThetaSvdGate> sg(nitems); std::vector<int> MrB(nitems), NcB(nitems);
        for (int i = 0; i < nitems; ++i) {
            const int d1 = dims[4 * i], d2 = dims[4 * i + 1], n1 = dims[4 * i + 2], n2 = dims[4 * i + 3]; const int* h = info + 8 * i;
            if (d1 < 1 || d2 < 1 || n1 < 1 || n2 < 1) throw Err(TNQS_ERR_INVALID, "dbg_theta_svd_stage: d1, d2, n1, n2 >= 1");
            if ((long long)n1 * d1 > 512 || (long long)n2 * d2 > 512) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_theta_svd_stage: d^2*chi > 512 is not supported by the theta SVD kernels");
            MrB[i] = std::max(n1 * d1, n2 * d2); NcB[i] = std::min(n1 * d1, n2 * d2);
            const int Mr = h[0] * d1, Nc = h[1] * d2;
            if (h[0] < 1 || h[0] > n1 || h[1] < 1 || h[1] > n2) throw Err(TNQS_ERR_INVALID, "dbg_theta_svd_stage: 1 <= r <= n");
            if (K[i] < 0 || K[i] > NcB[i] || cap[i] < 0 || rank_bounds[2 * i] < 1 || rank_bounds[2 * i + 1] < 1) throw Err(TNQS_ERR_INVALID, "dbg_theta_svd_stage: K, cap or rank bound out of range");
            // a low-rank factor alive on the device: the one the host expected, of a theta that is not wide, with no more columns than its Q has rows
            if (h[7] < 0 || (h[7] > 0 && (h[7] != K[i] || Mr < Nc || h[7] > Nc))) throw Err(TNQS_ERR_INVALID, "dbg_theta_svd_stage: inconsistent info[7]");
            if (has_q[i] && (K[i] < 1 || n1 * d1 < n2 * d2 || (theta && !Q))) throw Err(TNQS_ERR_INVALID, "dbg_theta_svd_stage: Q needs K >= 1 and a theta whose bounds are not wide");
            // the run-ahead regime: what theta_svd()'s one_trip asks of the bounds
            if (dyn && !(jacobi_lds(jacobi_lds_bytes(MrB[i], NcB[i], false, esz)) > 0 && MrB[i] <= 256))
                throw Err(TNQS_ERR_UNSUPPORTED, "dbg_theta_svd_stage: the run-ahead regime needs every theta within the LDS-resident Jacobi at its bounds");
            sg[i] = ThetaSvdGate{nullptr, nullptr, nullptr, d1, d2, n1, n2, nullptr, K[i], nullptr, rank_bounds[2 * i] * d1, rank_bounds[2 * i + 1] * d2, cap[i]};
        }
        if (route_out) {
            static int stand_in;      // (the route reads no pointer, only whether the gate has a Q)
            for (int i = 0; i < nitems; ++i) { ThetaSvdGate g = sg[i]; if (has_q[i]) g.lowQ = &stand_in; route_out[i] = theta_svd_route(F32, g, dyn ? nullptr : info + 8 * i, info + 8 * i); }
        }
        if (!theta) return;
        need_gpu();
        int dev = 0; HIPCHK(hipGetDevice(&dev));
        std::unique_ptr<State> s(state_create(1, 0, nullptr, nullptr, nullptr, dtype, dev));
        {
            Slots sQ; Guarded gTh(guard_elems * esz), gTh0(guard_elems * esz), gTv(guard_elems * esz);
            for (int i = 0; i < nitems; ++i) {
                const size_t mx = (size_t)MrB[i];
                gTh.add((size_t)MrB[i] * NcB[i] * esz); gTh0.add((size_t)MrB[i] * NcB[i] * esz); gTv.add(mx * mx * esz);
                sQ.add(has_q[i] ? (size_t)NcB[i] * K[i] * 16 : 0);
            }
            alloc_all(sQ, gTh, gTh0, gTv);
            { const char* p = (const char*)Q; for (int i = 0; i < nitems; ++i) if (has_q[i]) { sQ.put(i, p); p += sQ.len[i]; } }
            DBuf dInfo(32 * (size_t)nitems); up_ints(dInfo, info, 8 * (size_t)nitems);
            for (int i = 0; i < nitems; ++i) {
                sg[i].theta = gTh.at(i); sg[i].theta0 = gTh0.at(i); sg[i].thetaV = gTv.at(i); sg[i].info = (int*)dInfo.p + 8 * i;
                sg[i].lowQ = has_q[i] ? sQ.at(i) : nullptr;
            }
            sQ.up(); gTh.up(theta); gTh0.up(theta0); gTv.up(thetaV);
            const bool mfma = recover_form == 0 && F32 && use_mfma();      // 0: the engine's rule
            by_dtype(dtype, [&](auto t) { launch_theta_svd_stage<decltype(t)>(s.get(), sg, dyn ? nullptr : info, mfma); });
            HIPCHK(hipStreamSynchronize(s->stream));
            sQ.down("Q"); gTh.down(theta, "theta"); gTh0.down(theta0, "theta0"); gTv.down(thetaV, "thetaV");
            if (sweeps_out) { std::vector<int> h(8 * (size_t)nitems); dInfo.down(h.data(), 32 * (size_t)nitems); for (int i = 0; i < nitems; ++i) sweeps_out[i] = h[8 * i + 4]; }
        }
    });
}
// qr2_rinv_kernel (stage 0: X1 only), then qr2_compose_kernel (stage 1), as second_pass() runs them.  n x n complex128 matrices per item
extern "C" int tnqs_dbg_qr2(int stage, int nitems, const int* n, const void* GW, const void* GV, const double* lam, const int* idx, const int* r, const void* A2, const void* V2, const double* tau,
                            void* X1, void* GVout, void* GWout, int* rk, int guard_elems) {
    return guard([&] {
        if (stage < 0 || stage > 1 || nitems < 1 || !n || !GW || !lam || !idx || !r || !X1 || guard_elems < 0 || (stage == 1 && (!GV || !A2 || !V2 || !tau || !GVout || !GWout || !rk)))
            throw Err(TNQS_ERR_INVALID, "dbg_qr2: bad arguments");
        size_t io = 0;
        for (int i = 0; i < nitems; ++i) {
            if (n[i] < 1) throw Err(TNQS_ERR_INVALID, "dbg_qr2: n >= 1");
            if (n[i] > 256) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_qr2: n > 256 (d*chi of a site the engine takes is at most 256)");
            if (r[i] < 0 || r[i] > n[i]) throw Err(TNQS_ERR_INVALID, "dbg_qr2: 0 <= r <= n");
            for (int a = 0; a < r[i]; ++a) if (idx[io + a] < 0 || idx[io + a] >= n[i]) throw Err(TNQS_ERR_INVALID, "dbg_qr2: idx out of range");
            io += n[i];
        }
        need_gpu();
        Slots sW, sV, sLam, sIdx, sA2, sV2; Guarded gX((size_t)guard_elems * 16), gGV((size_t)guard_elems * 16), gGW((size_t)guard_elems * 16);
        for (int i = 0; i < nitems; ++i) {
            const size_t nn = (size_t)n[i] * n[i] * 16;
            sW.add(nn); sV.add(nn); sA2.add(nn); sV2.add(nn); sLam.add((size_t)n[i] * 8); sIdx.add((size_t)n[i] * 4); gX.add(nn); gGV.add(stage ? nn : 0); gGW.add(stage ? nn : 0);
        }
        alloc_all(sW, sV, sLam, sIdx, sA2, sV2, gX, gGV, gGW);
        put_all(sW, GW); put_all(sLam, lam); put_all(sIdx, idx);
        if (stage) { put_all(sV, GV); put_all(sA2, A2); put_all(sV2, V2); }
        DBuf dR(4 * (size_t)nitems), dRk(4 * (size_t)nitems); up_ints(dR, r, nitems); if (stage) up_ints(dRk, rk, nitems);
        std::vector<Qr2RinvItem> ri(nitems); std::vector<Qr2ComposeItem> ci(nitems);
        for (int i = 0; i < nitems; ++i) {
            const Qr2Site q{sW.at(i), sV.at(i), (const double*)sLam.at(i), (const int*)sIdx.at(i), (const int*)dR.p + i, n[i], gX.at(i)};
            ri[i] = q.rinv();
            ci[i] = q.compose(sA2.at(i), sV2.at(i), stage ? tau[i] : 0.0, gGV.at(i), gGW.at(i), (int*)dRk.p + i);
        }
        DevItems<Qr2RinvItem> dRi(ri); DevItems<Qr2ComposeItem> dCi(ci);
        up_all(sW, sV, sLam, sIdx, sA2, sV2);
        gX.up(X1); if (stage) { gGV.up(GVout); gGW.up(GWout); }
        launch_qr2_rinv(nullptr, dRi.get(), nitems);
        if (stage) launch_qr2_compose(nullptr, dCi.get(), nitems);
        HIPCHK(hipDeviceSynchronize());
        gX.down(X1, "X1");
        if (stage) { gGV.down(GVout, "GVout"); gGW.down(GWout, "GWout"); dRk.down(rk, 4 * (size_t)nitems); }
    });
}
// small_svd_prepare_kernel<T> -> launch_jacobi<double> -> small_svd_finish_kernel on site tensors [d][low][chi_b][hi] (shape: 4 ints per item) with low * hi < d * chi_b
extern "C" int tnqs_dbg_small_svd(int dtype, int nitems, const int* shape, const void* src, void* GA, void* GV, int guard_elems) {
    return guard([&] {
        if (!is_dtype(dtype) || nitems < 1 || !shape || !src || !GA || !GV || guard_elems < 0) throw Err(TNQS_ERR_INVALID, "dbg_small_svd: bad arguments");
        const size_t esz = esz_of(dtype);
        Slots sSrc, sM; Guarded gA((size_t)guard_elems * 16), gV((size_t)guard_elems * 16);
        for (int i = 0; i < nitems; ++i) {
            const int d = shape[4 * i], lo = shape[4 * i + 1], cb = shape[4 * i + 2], hi = shape[4 * i + 3];
            if (d < 1 || lo < 1 || cb < 1 || hi < 1) throw Err(TNQS_ERR_INVALID, "dbg_small_svd: dimensions >= 1");
            const long long n = (long long)d * cb, N = (long long)lo * hi;
            if (!(N < n && n <= 256)) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_small_svd: the small-SVD route takes sites with fewer fibers than columns (low*hi < d*chi_b <= 256)");
            sSrc.add((size_t)(n * N) * esz); sM.add((size_t)(n * N) * 16); gA.add((size_t)(n * n) * 16); gV.add((size_t)(n * n) * 16);
        }
        need_gpu();
        alloc_all(sSrc, sM, gA, gV);
        put_all(sSrc, src);
        std::vector<SmallSvdItem> si; std::vector<JacobiItem> sji;
        for (int i = 0; i < nitems; ++i) {
            const int d = shape[4 * i], lo = shape[4 * i + 1], cb = shape[4 * i + 2], hi = shape[4 * i + 3];
            small_svd_items(sSrc.at(i), sM.at(i), gA.at(i), gV.at(i), d, lo, cb, hi, si, sji);
        }
        DevItems<SmallSvdItem> dS(si); DevItems<JacobiItem> dJ(sji);
        up_all(sSrc, sM); gA.up(GA); gV.up(GV);
        by_dtype(dtype, [&](auto t) { launch_small_svd<decltype(t)>(nullptr, dS.get(), dJ.get(), sji); });
        HIPCHK(hipDeviceSynchronize());
        sM.down("M"); gA.down(GA, "GA"); gV.down(GV, "GV");
    });
}
