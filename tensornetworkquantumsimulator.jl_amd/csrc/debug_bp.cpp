// debug_bp.cpp -- kernel-level test entry points (include/tnqs_debug.h) of the BP update and of what post-processes a BP cache: the sweep order (bp_schedule.cpp), the
// small-site message kernel and the message epilogue, rescale, edge scalars, environments, symmetric gauge (kernels_bp.hip, kernels_chol.hip), diag and cscale (kernels_util.hip).
#include "debug_util.hpp"

using namespace tnqs;

// ---- HOST ONLY: the default sweep order and its level schedule ---------------------------------------------------------------------------------------------------
extern "C" int tnqs_dbg_default_sequence(tnqs_handle h, int* src, int* dst, int cap, int* n_out) {
    return guard([&] {
        std::vector<int> a, b; dbg_default_sequence(*S(h)->g, a, b); *n_out = (int)a.size();
        for (int i = 0; i < (int)a.size() && i < cap; ++i) { src[i] = a[i]; dst[i] = b[i]; }
    });
}
extern "C" int tnqs_dbg_default_sequence_graph(int nv, int ne, const int32_t* esrc, const int32_t* edst, int* src, int* dst, int* level, int cap, int* n_out) {
    return guard([&] {
        if (nv < 0 || ne < 0 || (ne > 0 && (!esrc || !edst)) || !n_out) throw Err(TNQS_ERR_INVALID, "tnqs_dbg_default_sequence_graph: bad arguments");
        auto g = dbg_make_graph(nv, ne, esrc, edst); std::vector<int> a, b, l; dbg_default_sequence_graph(*g, a, b, l); *n_out = (int)a.size();
        for (int i = 0; i < (int)a.size() && i < cap; ++i) { if (src) src[i] = a[i]; if (dst) dst[i] = b[i]; if (level) level[i] = l[i]; }
    });
}

// ---- the small-site BP message kernel and the message epilogue, set up as engine_bp.cpp sets them up --------------------------------------------------------
// ONE launch_bp_small_site over nitems (site, outgoing leg) pairs (ComplexF32): item i is a site tensor [d[i]][chi_0]..[chi_{z[i]-1}] with the outgoing leg jo[i];
// chi / present: the items' legs one after the other; psi: the items' tensors one after the other; M: one chi_k x chi_k matrix (M[q + chi_k qo]) per leg of every
// item in leg order, read only where present[leg] != 0 (0: a null pointer = identity; the slot of leg jo is handed over as well -- the kernel must skip it).
// form: -1 the engine's rule (matrix-core form iff every leg is 16-dimensional and the element count a multiple of 256), 0 scalar form, 1 matrix-core form or refusal.
// new_msg == NULL: out[i] = the raw message.  Otherwise the epilogue runs as in the engine -- inside the kernel (matrix-core form) or as launch_msg_finalize<float>
// on the one partial (scalar form) -- and out is not written.  out / new_msg / old_msg hold chi_jo^2 numbers per item, one item after the other
extern "C" int tnqs_dbg_small_site(int nitems, const int* d, const int* z, const int* chi, const int* jo, const void* psi, const void* M, const int* present, int form,
                                   const void* old_msg, const int* has_old, int normalize, void* out, void* new_msg, double* diff, int* route) {
    return guard([&] {
        need_gpu();
        if (nitems < 1 || !d || !z || !chi || !jo || !psi || !M || !present || !out || form < -1 || form > 1 || (old_msg && !has_old))
            throw Err(TNQS_ERR_INVALID, "dbg_small_site: bad arguments");
        std::vector<SmallMsgItem> items(nitems); std::vector<int> leg0(nitems + 1, 0);
        Slots sPsi, sM, sOut, sNew, sOld, sRaw;
        int max_elems = 0;
        for (int i = 0; i < nitems; ++i) {
            if (z[i] < 1 || z[i] > 8) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_small_site: 1 <= z <= 8");
            const int* c = chi + leg0[i]; leg0[i + 1] = leg0[i] + z[i];
            size_t n = (size_t)std::max(d[i], 0);
            for (int k = 0; k < z[i]; ++k) { if (c[k] < 1) throw Err(TNQS_ERR_INVALID, "dbg_small_site: leg dimension < 1"); n *= (size_t)c[k]; }
            if (!bp_small_site_covers(d[i], z[i], c, n)) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_small_site: site not covered by bp_small_site_kernel (z <= 8, chi <= 32, <= 8192 elements)");
            if (jo[i] < 0 || jo[i] >= z[i]) throw Err(TNQS_ERR_INVALID, "dbg_small_site: outgoing leg out of range");
            const bool all16 = bp_small_site_mfma_form(z[i], c, n);
            if (form == 1 && !all16) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_small_site: the matrix-core form takes sites whose legs are all 16-dimensional");
            SmallMsgItem& it = items[i]; it = SmallMsgItem{};
            it.d = d[i]; it.z = z[i]; it.jo = jo[i]; it.mfma = (form != 0 && all16) ? 1 : 0; it.normalize = normalize;
            for (int k = 0; k < z[i]; ++k) { it.chi[k] = c[k]; sM.add((size_t)c[k] * c[k] * 8); }
            const size_t mb = (size_t)c[jo[i]] * c[jo[i]] * 8;
            sPsi.add(n * 8); sOut.add(mb); sNew.add(mb); sOld.add(mb); sRaw.add(mb);
            max_elems = std::max(max_elems, (int)n);
        }
        alloc_all(sPsi, sM, sOut, sNew, sOld, sRaw);
        DBuf dDiff(sizeof(double) * nitems); DevItems<SmallMsgItem> dI(nitems); DevItems<MsgFinalItem> dF(nitems);
        std::vector<double> hdiff(nitems, 0.0); if (diff) std::copy(diff, diff + nitems, hdiff.begin());
        std::vector<MsgFinalItem> fin;
        const char *hpsi = (const char*)psi, *hM = (const char*)M, *hold = (const char*)old_msg; char *hout = (char*)out, *hnew = (char*)new_msg;
        size_t opsi = 0, oM = 0, omsg = 0;
        for (int i = 0; i < nitems; ++i) {
            SmallMsgItem& it = items[i];
            sPsi.put(i, hpsi + opsi); opsi += sPsi.len[i];
            for (int k = 0; k < it.z; ++k) {
                const size_t q = (size_t)leg0[i] + k;
                if (present[q]) { sM.put(q, hM + oM); it.M[k] = sM.at(q); }
                oM += sM.len[q];
            }
            sOut.put(i, hout + omsg); if (hnew) sNew.put(i, hnew + omsg);
            const bool old = hold && has_old[i]; if (old) sOld.put(i, hold + omsg);
            omsg += sOut.len[i];
            it.psi = sPsi.at(i); it.out = sOut.at(i);
            if (hnew && it.mfma) { it.new_msg = sNew.at(i); it.old_msg = old ? sOld.at(i) : nullptr; it.diff_out = diff ? (double*)dDiff.p + i : nullptr; }
            else if (hnew) {                                      // the raw message is the one partial of the message's msg_finalize item
                it.out = sRaw.at(i);
                fin.push_back(MsgFinalItem{sRaw.at(i), 1, it.chi[it.jo], old ? sOld.at(i) : nullptr, sNew.at(i), diff ? (double*)dDiff.p + i : nullptr, normalize});
            }
        }
        up_all(sPsi, sM, sOut, sNew, sOld, sRaw);
        dDiff.up(hdiff.data(), sizeof(double) * nitems); dI.up(items); dF.up(fin);
        launch_bp_small_site(nullptr, dI.get(), nitems, max_elems);
        launch_msg_finalize<float>(nullptr, dF.get(), (int)fin.size());
        HIPCHK(hipDeviceSynchronize());
        sOut.down("out"); sNew.down("new_msg"); sRaw.down("the raw message");
        omsg = 0;
        for (int i = 0; i < nitems; ++i) { sOut.get(i, hout + omsg); if (hnew) sNew.get(i, hnew + omsg); omsg += sOut.len[i]; }
        if (diff) dDiff.down(diff, sizeof(double) * nitems);
        if (route) for (int i = 0; i < nitems; ++i) route[i] = items[i].mfma ? TNQS_DBG_ROUTE_SMALL_MFMA16 : TNQS_DBG_ROUTE_SMALL_SCALAR;
    });
}
// ONE launch_msg_finalize<T> over nitems messages: item i has nchunks[i] partials of chi[i]^2 numbers, [chunk][element], the items one after the other; old_msg /
// new_msg: chi[i]^2 numbers per item (has_old[i] == 0 or old_msg == NULL: identity); diff[i] = message_diff(new_i, old_i)
extern "C" int tnqs_dbg_msg_finalize(int dtype, int nitems, const int* chi, const int* nchunks, const void* partials, const void* old_msg, const int* has_old, int normalize,
                                     void* new_msg, double* diff) {
    return guard([&] {
        need_gpu();
        if (!is_dtype(dtype) || nitems < 1 || !chi || !nchunks || !partials || !new_msg || (old_msg && !has_old)) throw Err(TNQS_ERR_INVALID, "dbg_msg_finalize: bad arguments");
        const size_t esz = esz_of(dtype);
        Slots sP, sNew, sOld;
        for (int i = 0; i < nitems; ++i) {
            if (chi[i] < 1 || chi[i] > 128 || nchunks[i] < 1) throw Err(TNQS_ERR_INVALID, "dbg_msg_finalize: 1 <= chi <= 128, nchunks >= 1");
            const size_t mb = (size_t)chi[i] * chi[i] * esz;
            sP.add(mb * nchunks[i]); sNew.add(mb); sOld.add(mb);
        }
        alloc_all(sP, sNew, sOld);
        DBuf dDiff(sizeof(double) * nitems); DevItems<MsgFinalItem> dF(nitems);
        std::vector<double> hdiff(nitems, 0.0); if (diff) std::copy(diff, diff + nitems, hdiff.begin());
        std::vector<MsgFinalItem> fin(nitems);
        size_t op = 0, om = 0;
        for (int i = 0; i < nitems; ++i) {
            sP.put(i, (const char*)partials + op); op += sP.len[i];
            sNew.put(i, (const char*)new_msg + om);
            const bool old = old_msg && has_old[i]; if (old) sOld.put(i, (const char*)old_msg + om);
            om += sNew.len[i];
            fin[i] = MsgFinalItem{sP.at(i), nchunks[i], chi[i], old ? sOld.at(i) : nullptr, sNew.at(i), diff ? (double*)dDiff.p + i : nullptr, normalize};
        }
        up_all(sP, sNew, sOld); dDiff.up(hdiff.data(), sizeof(double) * nitems); dF.up(fin);
        by_dtype(dtype, [&](auto t) { launch_msg_finalize<decltype(t)>(nullptr, dF.get(), nitems); });
        HIPCHK(hipDeviceSynchronize());
        sNew.down("new_msg");
        om = 0;
        for (int i = 0; i < nitems; ++i) { sNew.get(i, (char*)new_msg + om); om += sNew.len[i]; }
        if (diff) dDiff.down(diff, sizeof(double) * nitems);
    });
}

// ---- the kernels that post-process a BP cache and prepare a gate's environments (kernels_bp.hip: msg_rescale, edge_scalar, symg_build, symg_finish; kernels_chol.hip:
// env_prepare, env_finish; kernels_util.hip: diag, cscale): ONE launch over nitems items of different n, the descriptors filled as engine_obs.cpp / engine_gates.cpp
// fill them.  Inputs: the items' arrays one after the other.  Outputs: `guard_elems` caller-filled elements, item 0, `guard_elems` elements, item 1, ..., `guard_elems` elements ----
extern "C" int tnqs_dbg_msg_rescale(int dtype, int nitems, const int* chi, const void* me, const void* mer, const int* present, void* me_out, void* mer_out, int guard_elems) {
    return guard([&] {
        need_gpu();
        post_check("dbg_msg_rescale", dtype, nitems, chi, guard_elems);
        if (!me || !mer || !present || !me_out || !mer_out) throw Err(TNQS_ERR_INVALID, "dbg_msg_rescale: bad arguments");
        const size_t esz = esz_of(dtype);
        Slots sA, sB; Guarded gA(guard_elems * esz), gB(guard_elems * esz);
        for (int i = 0; i < nitems; ++i) { const size_t mb = (size_t)chi[i] * chi[i] * esz; sA.add(mb); sB.add(mb); gA.add(mb); gB.add(mb); }
        alloc_all(sA, sB, gA, gB);
        put_all(sA, me); put_all(sB, mer);
        std::vector<MsgRescaleItem> items(nitems);
        for (int i = 0; i < nitems; ++i) items[i] = MsgRescaleItem{present[2 * i] ? sA.at(i) : nullptr, present[2 * i + 1] ? sB.at(i) : nullptr, gA.at(i), gB.at(i), chi[i]};
        up_all(sA, sB); gA.up(me_out); gB.up(mer_out); DevItems<MsgRescaleItem> dI(items);
        by_dtype(dtype, [&](auto t) { launch_msg_rescale<decltype(t)>(nullptr, dI.get(), nitems); });
        HIPCHK(hipDeviceSynchronize());
        gA.down(me_out, "me_out"); gB.down(mer_out, "mer_out");
    });
}
extern "C" int tnqs_dbg_edge_scalar(int dtype, int nitems, const int* chi, const void* me, const void* mer, const int* present, double* out) {
    return guard([&] {
        need_gpu();
        post_check("dbg_edge_scalar", dtype, nitems, chi, 0);
        if (!me || !mer || !present || !out) throw Err(TNQS_ERR_INVALID, "dbg_edge_scalar: bad arguments");
        const size_t esz = esz_of(dtype);
        Slots sA, sB;
        for (int i = 0; i < nitems; ++i) { const size_t mb = (size_t)chi[i] * chi[i] * esz; sA.add(mb); sB.add(mb); }
        alloc_all(sA, sB);
        put_all(sA, me); put_all(sB, mer);
        DBuf dO(16 * (size_t)nitems); DevItems<EdgeScalarItem> dI(nitems);
        std::vector<EdgeScalarItem> items(nitems);
        for (int i = 0; i < nitems; ++i) items[i] = EdgeScalarItem{present[2 * i] ? sA.at(i) : nullptr, present[2 * i + 1] ? sB.at(i) : nullptr, chi[i], (double*)dO.p + 2 * i};
        up_all(sA, sB); dO.up(out, 16 * (size_t)nitems); dI.up(items);
        by_dtype(dtype, [&](auto t) { launch_edge_scalar<decltype(t)>(nullptr, dI.get(), nitems); });
        HIPCHK(hipDeviceSynchronize());
        dO.down(out, 16 * (size_t)nitems);
    });
}
extern "C" int tnqs_dbg_env_prepare(int dtype, int nitems, const int* n, const void* msg, const int* present, void* H_out, void* V_out, int guard_elems) {
    return guard([&] {
        need_gpu();
        post_check("dbg_env_prepare", dtype, nitems, n, guard_elems);
        if (!msg || !present || !H_out || !V_out) throw Err(TNQS_ERR_INVALID, "dbg_env_prepare: bad arguments");
        const size_t esz = esz_of(dtype);
        Slots sM; Guarded gH((size_t)guard_elems * 16), gV((size_t)guard_elems * 16);
        for (int i = 0; i < nitems; ++i) { const size_t nn = (size_t)n[i] * n[i]; sM.add(nn * esz); gH.add(nn * 16); gV.add(nn * 16); }
        alloc_all(sM, gH, gV);
        put_all(sM, msg);
        std::vector<EnvItem> items(nitems);
        for (int i = 0; i < nitems; ++i) items[i] = EnvItem{present[i] ? sM.at(i) : nullptr, gH.at(i), gV.at(i), n[i]};
        sM.up(); gH.up(H_out); gV.up(V_out); DevItems<EnvItem> dI(items);
        by_dtype(dtype, [&](auto t) { launch_env_prepare<decltype(t)>(nullptr, dI.get(), nitems); });
        HIPCHK(hipDeviceSynchronize());
        gH.down(H_out, "H"); gV.down(V_out, "V");
    });
}
extern "C" int tnqs_dbg_env_finish(int dtype, int nitems, const int* n, const void* A, const void* V, const double* cutoff, void* msqrt_out, void* proj_out, int* flags_out, int guard_elems) {
    return guard([&] {
        need_gpu();
        post_check("dbg_env_finish", dtype, nitems, n, guard_elems);
        if (!A || !V || !cutoff || !msqrt_out || !proj_out || !flags_out) throw Err(TNQS_ERR_INVALID, "dbg_env_finish: bad arguments");
        const size_t esz = esz_of(dtype);
        Slots sA, sV; Guarded gM(guard_elems * esz), gP(guard_elems * esz);
        for (int i = 0; i < nitems; ++i) { const size_t nn = (size_t)n[i] * n[i]; sA.add(nn * 16); sV.add(nn * 16); gM.add(nn * esz); gP.add(nn * esz); }
        alloc_all(sA, sV, gM, gP);
        put_all(sA, A); put_all(sV, V);
        DBuf dF(sizeof(int) * 2 * nitems); DevItems<EnvFinishItem> dI(nitems);
        std::vector<EnvFinishItem> items(nitems);
        for (int i = 0; i < nitems; ++i) items[i] = EnvFinishItem{sA.at(i), sV.at(i), gM.at(i), gP.at(i), n[i], cutoff[i], (int*)dF.p + 2 * i};
        up_all(sA, sV); gM.up(msqrt_out); gP.up(proj_out); dF.up(flags_out, sizeof(int) * 2 * nitems); dI.up(items);
        by_dtype(dtype, [&](auto t) { launch_env_finish<decltype(t)>(nullptr, dI.get(), nitems); });
        HIPCHK(hipDeviceSynchronize());
        gM.down(msqrt_out, "msqrt"); gP.down(proj_out, "proj"); dF.down(flags_out, sizeof(int) * 2 * nitems);
    });
}
// (the pointers of a SymGaugeItem that the launched kernel does not use point at a scratch slot of the item's size)
extern "C" int tnqs_dbg_symg_build(int dtype, int nitems, const int* n, const void* AX, const void* VX, const void* AY, const void* VY, double reg, void* rx, void* ry, void* irx, void* iry,
                                   void* Ce, void* Ce0, int* flag_out, int guard_elems) {
    return guard([&] {
        need_gpu();
        post_check("dbg_symg_build", dtype, nitems, n, guard_elems);
        if (!AX || !VX || !AY || !VY || !rx || !ry || !irx || !iry || !Ce || !Ce0 || !flag_out) throw Err(TNQS_ERR_INVALID, "dbg_symg_build: bad arguments");
        const size_t esz = esz_of(dtype);
        Slots sAX, sVX, sAY, sVY, scr;
        Guarded gRx((size_t)guard_elems * 16), gRy((size_t)guard_elems * 16), gIx((size_t)guard_elems * 16), gIy((size_t)guard_elems * 16), gC(guard_elems * esz), gC0(guard_elems * esz);
        for (int i = 0; i < nitems; ++i) {
            const size_t nn = (size_t)n[i] * n[i];
            for (Slots* s : {&sAX, &sVX, &sAY, &sVY, &scr}) s->add(nn * 16);
            for (Guarded* g : {&gRx, &gRy, &gIx, &gIy}) g->add(nn * 16);
            gC.add(nn * esz); gC0.add(nn * esz);
        }
        alloc_all(sAX, sVX, sAY, sVY, scr, gRx, gRy, gIx, gIy, gC, gC0);
        put_all(sAX, AX); put_all(sVX, VX); put_all(sAY, AY); put_all(sVY, VY);
        DBuf dFlag(sizeof(int)); DevItems<SymGaugeItem> dI(nitems);
        HIPCHK(hipMemset(dFlag.p, 0, sizeof(int)));          // one flag for the whole launch, cleared first (engine_obs.cpp)
        std::vector<SymGaugeItem> items(nitems);
        for (int i = 0; i < nitems; ++i)
            items[i] = SymGaugeItem{sAX.at(i), sVX.at(i), sAY.at(i), sVY.at(i), gRx.at(i), gRy.at(i), gIx.at(i), gIy.at(i), gC.at(i), gC0.at(i), scr.at(i), scr.at(i), scr.at(i),
                                    (double*)scr.at(i), n[i], reg, (int*)dFlag.p};
        up_all(sAX, sVX, sAY, sVY, scr);
        gRx.up(rx); gRy.up(ry); gIx.up(irx); gIy.up(iry); gC.up(Ce); gC0.up(Ce0); dI.up(items);
        by_dtype(dtype, [&](auto t) { launch_symg_build<decltype(t)>(nullptr, dI.get(), nitems); });
        HIPCHK(hipDeviceSynchronize());
        gRx.down(rx, "rx"); gRy.down(ry, "ry"); gIx.down(irx, "irx"); gIy.down(iry, "iry"); gC.down(Ce, "Ce"); gC0.down(Ce0, "Ce0");
        dFlag.down(flag_out, sizeof(int));
    });
}
extern "C" int tnqs_dbg_symg_finish(int dtype, int nitems, const int* n, const void* USigma, const void* Vsvd, const void* irx, const void* iry, void* Xs, void* Xd, double* S, int guard_elems) {
    return guard([&] {
        need_gpu();
        post_check("dbg_symg_finish", dtype, nitems, n, guard_elems);
        if (!USigma || !Vsvd || !irx || !iry || !Xs || !Xd || !S) throw Err(TNQS_ERR_INVALID, "dbg_symg_finish: bad arguments");
        const size_t esz = esz_of(dtype);
        Slots sU, sV, sIx, sIy, scr; Guarded gXs(guard_elems * esz), gXd(guard_elems * esz), gS((size_t)guard_elems * 8);
        for (int i = 0; i < nitems; ++i) {
            const size_t nn = (size_t)n[i] * n[i];
            sU.add(nn * esz); sV.add(nn * esz); sIx.add(nn * 16); sIy.add(nn * 16); scr.add(nn * 16);
            gXs.add(nn * esz); gXd.add(nn * esz); gS.add((size_t)n[i] * 8);
        }
        alloc_all(sU, sV, sIx, sIy, scr, gXs, gXd, gS);
        put_all(sU, USigma); put_all(sV, Vsvd); put_all(sIx, irx); put_all(sIy, iry);
        DBuf dFlag(sizeof(int)); DevItems<SymGaugeItem> dI(nitems);
        HIPCHK(hipMemset(dFlag.p, 0, sizeof(int)));
        std::vector<SymGaugeItem> items(nitems);
        for (int i = 0; i < nitems; ++i)
            items[i] = SymGaugeItem{scr.at(i), scr.at(i), scr.at(i), scr.at(i), scr.at(i), scr.at(i), sIx.at(i), sIy.at(i), sU.at(i), scr.at(i), sV.at(i), gXs.at(i), gXd.at(i),
                                    (double*)gS.at(i), n[i], 0.0, (int*)dFlag.p};
        up_all(sU, sV, sIx, sIy, scr); gXs.up(Xs); gXd.up(Xd); gS.up(S); dI.up(items);
        by_dtype(dtype, [&](auto t) { launch_symg_finish<decltype(t)>(nullptr, dI.get(), nitems); });
        HIPCHK(hipDeviceSynchronize());
        gXs.down(Xs, "Xs"); gXd.down(Xd, "Xd"); gS.down(S, "S");
    });
}
extern "C" int tnqs_dbg_diag(int dtype, int nitems, const int* chi, const double* S, void* out, int guard_elems) {
    return guard([&] {
        need_gpu();
        post_check("dbg_diag", dtype, nitems, chi, guard_elems);
        if (!S || !out) throw Err(TNQS_ERR_INVALID, "dbg_diag: bad arguments");
        const size_t esz = esz_of(dtype);
        Slots sS; Guarded gO(guard_elems * esz);
        for (int i = 0; i < nitems; ++i) { sS.add((size_t)chi[i] * 8); gO.add((size_t)chi[i] * chi[i] * esz); }
        alloc_all(sS, gO);
        put_all(sS, S);
        std::vector<DiagItem> items(nitems);
        for (int i = 0; i < nitems; ++i) items[i] = DiagItem{gO.at(i), (const double*)sS.at(i), chi[i]};
        sS.up(); gO.up(out); DevItems<DiagItem> dI(items);
        by_dtype(dtype, [&](auto t) { launch_diag<decltype(t)>(nullptr, dI.get(), nitems); });
        HIPCHK(hipDeviceSynchronize());
        gO.down(out, "out");
    });
}
extern "C" int tnqs_dbg_cscale(int dtype, int nitems, const int* len, const void* src, const double* re, const double* im, void* dst, int guard_elems) {
    return guard([&] {
        need_gpu();
        if (!is_dtype(dtype) || nitems < 1 || !len || !src || !re || !im || !dst || guard_elems < 0) throw Err(TNQS_ERR_INVALID, "dbg_cscale: bad arguments");
        const size_t esz = esz_of(dtype);
        Slots sS; Guarded gD(guard_elems * esz);
        for (int i = 0; i < nitems; ++i) { if (len[i] < 1) throw Err(TNQS_ERR_INVALID, "dbg_cscale: len >= 1"); sS.add((size_t)len[i] * esz); gD.add((size_t)len[i] * esz); }
        alloc_all(sS, gD);
        put_all(sS, src);
        std::vector<CScaleItem> items(nitems);
        for (int i = 0; i < nitems; ++i) items[i] = CScaleItem{sS.at(i), gD.at(i), (size_t)len[i], re[i], im[i]};
        sS.up(); gD.up(dst); DevItems<CScaleItem> dI(items);
        by_dtype(dtype, [&](auto t) { launch_cscale<decltype(t)>(nullptr, dI.get(), nitems); });
        HIPCHK(hipDeviceSynchronize());
        gD.down(dst, "dst");
    });
}
