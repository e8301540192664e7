// debug_obs.cpp -- kernel-level test entry points (include/tnqs_debug.h) of the observables: loop corrections (kernels_loop.hip), reduced density matrices of bonds and
// paths (kernels_rdm.hip, engine_rdm.cpp, engine_paths.cpp), bond entanglement spectra (kernels_spectrum.hip, engine_spectra.cpp), overlap of two states
// (kernels_inner.hip, engine_inner.cpp), bitstring amplitudes (kernels_amp.hip, engine_amp.cpp).
#include "debug_util.hpp"

using namespace tnqs;

// ---- loop corrections (kernels_loop.hip): ONE launch over nitems items of different shapes, the items' matrices one after the other in A, B (and C, between
// guard bands of `guard_elems` elements that the caller has filled and gets back: whatever the kernel must leave alone is seen to be left alone).  The arrays are
// tightly packed on the device as on the host ----
extern "C" int tnqs_dbg_loop_cgemm(int dtype, int opB, int nitems, const int* m, const int* n, const int* k, const void* A, const void* B, void* C, int guard_elems) {
    return guard([&] {
        need_gpu();
        if (!is_dtype(dtype) || nitems < 1 || !m || !n || !k || !A || !B || !C || guard_elems < 0) throw Err(TNQS_ERR_INVALID, "dbg_loop_cgemm: bad arguments");
        const size_t esz = esz_of(dtype);
        size_t na = 0, nb = 0, nc = (size_t)guard_elems;
        std::vector<LoopGemmItem> items(nitems);
        for (int i = 0; i < nitems; ++i) {
            if (m[i] < 1 || n[i] < 1 || k[i] < 1) throw Err(TNQS_ERR_INVALID, "dbg_loop_cgemm: m, n, k >= 1");
            LoopGemmItem& it = items[i]; it = LoopGemmItem{};
            it.A = (const void*)(na * esz); it.B = (const void*)(nb * esz); it.C = (void*)(nc * esz);      // offsets for now
            it.m = m[i]; it.n = n[i]; it.k = k[i]; it.opB = opB ? 1 : 0; it.I0 = m[i]; it.si0 = 1; it.J0 = n[i]; it.sj0 = m[i];
            na += (size_t)m[i] * k[i]; nb += (size_t)n[i] * k[i]; nc += (size_t)m[i] * n[i] + guard_elems;
        }
        DBuf dA(na * esz), dB(nb * esz), dC(nc * esz); DevItems<LoopGemmItem> dI(nitems);
        for (auto& it : items) { it.A = (char*)dA.p + (size_t)it.A; it.B = (char*)dB.p + (size_t)it.B; it.C = (char*)dC.p + (size_t)it.C; }
        const int tiles = plan_loop_cgemm(items.data(), nitems);
        dA.up(A, na * esz); dB.up(B, nb * esz); dC.up(C, nc * esz); dI.up(items);
        by_dtype(dtype, [&](auto t) { launch_loop_cgemm<decltype(t)>(nullptr, dI.get(), nitems, tiles); });
        HIPCHK(hipDeviceSynchronize());
        dC.down(C, nc * esz);
    });
}
// C_i[(l_p0, l_p0'), (l_p1, l_p1'), (l_p2, l_p2')] = sum_kk A_i[l, kk] conj(B_i[l', kk]); the item is the one the engine builds (branch_gram_item)
extern "C" int tnqs_dbg_loop_branch_gram(int dtype, int nitems, const int* dims, const int* order, const int* k, const void* A, const void* B, void* C, int guard_elems) {
    return guard([&] {
        need_gpu();
        if (!is_dtype(dtype) || nitems < 1 || !dims || !k || !A || !B || !C || guard_elems < 0) throw Err(TNQS_ERR_INVALID, "dbg_loop_branch_gram: bad arguments");
        const size_t esz = esz_of(dtype);
        size_t na = 0, nc = (size_t)guard_elems;
        std::vector<BranchGramItem> items(nitems);
        for (int i = 0; i < nitems; ++i) {
            const int* x = dims + 3 * i; int ord[3] = {0, 1, 2};
            if (order) { for (int p = 0; p < 3; ++p) ord[p] = order[3 * i + p]; }
            if (x[0] < 1 || x[1] < 1 || x[2] < 1 || k[i] < 1 || (size_t)x[0] * x[1] * x[2] > 4096) throw Err(TNQS_ERR_INVALID, "dbg_loop_branch_gram: dims, k >= 1, at most 4096 rows");
            if ((1 << ord[0] | 1 << ord[1] | 1 << ord[2]) != 7 || ord[0] < 0 || ord[1] < 0 || ord[2] < 0) throw Err(TNQS_ERR_INVALID, "dbg_loop_branch_gram: order is no permutation of 0, 1, 2");
            BranchGramItem& it = items[i]; it = branch_gram_item(x, ord, k[i]);
            it.A = (const void*)(na * esz); it.B = (const void*)(na * esz); it.C = (void*)(nc * esz);      // offsets for now
            na += (size_t)it.m * k[i]; nc += (size_t)it.m * it.n + guard_elems;
        }
        DBuf dA(na * esz), dB(na * esz), dC(nc * esz); DevItems<BranchGramItem> dI(nitems);
        for (auto& it : items) { it.A = (char*)dA.p + (size_t)it.A; it.B = (char*)dB.p + (size_t)it.B; it.C = (char*)dC.p + (size_t)it.C; }
        const int tiles = plan_loop_branch_gram(items.data(), nitems);
        dA.up(A, na * esz); dB.up(B, na * esz); dC.up(C, nc * esz); dI.up(items);
        by_dtype(dtype, [&](auto t) { launch_loop_branch_gram<decltype(t)>(nullptr, dI.get(), nitems, tiles); });
        HIPCHK(hipDeviceSynchronize());
        dC.down(C, nc * esz);
    });
}
// T_i (nr[i] x nc[i], in place) <- T_i - f_i (b_i^T T_i); f, b: nr[i] elements per item
extern "C" int tnqs_dbg_loop_antiproject(int dtype, int nitems, const int* nr, const int* nc, void* Tm, const void* f, const void* b) {
    return guard([&] {
        need_gpu();
        if (!is_dtype(dtype) || nitems < 1 || !nr || !nc || !Tm || !f || !b) throw Err(TNQS_ERR_INVALID, "dbg_loop_antiproject: bad arguments");
        const size_t esz = esz_of(dtype);
        size_t nt = 0, nv = 0;
        std::vector<LoopProjItem> items(nitems);
        for (int i = 0; i < nitems; ++i) {
            if (nr[i] < 1 || nc[i] < 1) throw Err(TNQS_ERR_INVALID, "dbg_loop_antiproject: nr, nc >= 1");
            items[i] = LoopProjItem{(void*)(nt * esz), (const void*)(nv * esz), (const void*)(nv * esz), nr[i], nc[i], 0};
            nt += (size_t)nr[i] * nc[i]; nv += (size_t)nr[i];
        }
        DBuf dT(nt * esz), dF(nv * esz), dB(nv * esz); DevItems<LoopProjItem> dI(nitems);
        for (auto& it : items) { it.T = (char*)dT.p + (size_t)it.T; it.f = (char*)dF.p + (size_t)it.f; it.b = (char*)dB.p + (size_t)it.b; }
        const int wgs = plan_loop_antiproject(items.data(), nitems);
        dT.up(Tm, nt * esz); dF.up(f, nv * esz); dB.up(b, nv * esz); dI.up(items);
        by_dtype(dtype, [&](auto t) { launch_loop_antiproject<decltype(t)>(nullptr, dI.get(), nitems, wgs); });
        HIPCHK(hipDeviceSynchronize());
        dT.down(Tm, nt * esz);
    });
}
// out[i] (complex128) = sum_ab X_i[a,b] Y_i[b,a]; X_i: p[i] x q[i], Y_i: q[i] x p[i]
extern "C" int tnqs_dbg_loop_trace(int dtype, int nitems, const int* p, const int* q, const void* X, const void* Y, double* out) {
    return guard([&] {
        need_gpu();
        if (!is_dtype(dtype) || nitems < 1 || !p || !q || !X || !Y || !out) throw Err(TNQS_ERR_INVALID, "dbg_loop_trace: bad arguments");
        const size_t esz = esz_of(dtype);
        size_t ne = 0;
        std::vector<LoopTraceItem> items(nitems);
        DBuf dP(sizeof(double) * 128 * nitems), dO(sizeof(double) * 2 * nitems);
        for (int i = 0; i < nitems; ++i) {
            if (p[i] < 1 || q[i] < 1) throw Err(TNQS_ERR_INVALID, "dbg_loop_trace: p, q >= 1");
            items[i] = LoopTraceItem{(const void*)(ne * esz), (const void*)(ne * esz), p[i], q[i], (double*)dP.p + 128 * (size_t)i, (double*)dO.p + 2 * (size_t)i, 0, 0};
            ne += (size_t)p[i] * q[i];
        }
        DBuf dX(ne * esz), dY(ne * esz); DevItems<LoopTraceItem> dI(nitems);
        for (auto& it : items) { it.X = (char*)dX.p + (size_t)it.X; it.Y = (char*)dY.p + (size_t)it.Y; }
        const int wgs = plan_loop_trace(items.data(), nitems);
        dX.up(X, ne * esz); dY.up(Y, ne * esz); dI.up(items);
        by_dtype(dtype, [&](auto t) { launch_loop_trace<decltype(t)>(nullptr, dI.get(), nitems, wgs); });
        HIPCHK(hipDeviceSynchronize());
        dO.down(out, sizeof(double) * 2 * nitems);
    });
}

// ---- two-site reduced density matrices ----
namespace {
// edge_rdm_kernel<P> (kernels_rdm.hip), ONE launch over nitems bonds set up as engine_rdm.cpp sets them up: the items' Gram partials one after the other in partial_u /
// partial_v (P numbers), scale_u / scale_v one double per item (0: a null pointer), out between guard bands of `guard_elems` complex128 elements
// ptype_u / ptype_v: the partial type of each end (tnqs_dbg_edge_rdm: the same for both)
void edge_rdm_mixed(int ptype_u, int ptype_v, int nitems, const int* du, const int* dv, const int* chi, const int* nchunks_u, const int* nchunks_v, const void* partial_u,
                    const void* partial_v, const double* scale_u, const double* scale_v, void* out, int guard_elems) {
    need_gpu();
    if ((ptype_u != 0 && ptype_u != 1) || (ptype_v != 0 && ptype_v != 1) || nitems < 1 || !du || !dv || !chi || !nchunks_u || !nchunks_v || !partial_u || !partial_v || !scale_u || !scale_v || !out || guard_elems < 0)
        throw Err(TNQS_ERR_INVALID, "dbg_edge_rdm: bad arguments");
    const size_t psz_u = ptype_u == 0 ? 8 : 16, psz_v = ptype_v == 0 ? 8 : 16;
    Slots sU, sV, sS; Guarded gO((size_t)guard_elems * 16);
    for (int i = 0; i < nitems; ++i) {
        if (du[i] < 1 || dv[i] < 1 || chi[i] < 1 || nchunks_u[i] < 1 || nchunks_v[i] < 1) throw Err(TNQS_ERR_INVALID, "dbg_edge_rdm: dimensions and chunk counts >= 1");
        if (edge_rdm_block(du[i], dv[i], chi[i]) < 1) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_edge_rdm: bond too large for the edge kernel");
        const size_t ku = (size_t)du[i] * chi[i], kv = (size_t)dv[i] * chi[i], dd = (size_t)du[i] * dv[i];
        sU.add((size_t)nchunks_u[i] * ku * ku * psz_u); sV.add((size_t)nchunks_v[i] * kv * kv * psz_v); sS.add(16); gO.add(dd * dd * 16);
    }
    alloc_all(sU, sV, sS, gO);
    put_all(sU, partial_u); put_all(sV, partial_v);
    std::vector<EdgeRdmItem> items(nitems);
    for (int i = 0; i < nitems; ++i) {
        const double f[2] = {scale_u[i], scale_v[i]}; sS.put(i, f);
        items[i] = EdgeRdmItem{sU.at(i), sV.at(i), nchunks_u[i], nchunks_v[i], du[i], dv[i], chi[i],
                               f[0] != 0.0 ? reinterpret_cast<const double*>(sS.at(i)) : nullptr, f[1] != 0.0 ? reinterpret_cast<const double*>(sS.at(i)) + 1 : nullptr, gO.at(i)};
    }
    up_all(sU, sV, sS); gO.up(out); DevItems<EdgeRdmItem> dI(items);
    if (ptype_u == ptype_v) { if (ptype_u == 0) launch_edge_rdm<float>(nullptr, dI.get(), nitems); else launch_edge_rdm<double>(nullptr, dI.get(), nitems); }
    else if (ptype_u == 0) launch_edge_rdm_mixed<float, double>(nullptr, dI.get(), nitems); else launch_edge_rdm_mixed<double, float>(nullptr, dI.get(), nitems);
    HIPCHK(hipDeviceSynchronize());
    gO.down(out, "out");
}
}  // namespace
extern "C" int tnqs_dbg_edge_rdm_mixed(int ptype_u, int ptype_v, int nitems, const int* du, const int* dv, const int* chi, const int* nchunks_u, const int* nchunks_v, const void* partial_u,
                                       const void* partial_v, const double* scale_u, const double* scale_v, void* out, int guard_elems) {
    return guard([&] { edge_rdm_mixed(ptype_u, ptype_v, nitems, du, dv, chi, nchunks_u, nchunks_v, partial_u, partial_v, scale_u, scale_v, out, guard_elems); });
}
extern "C" int tnqs_dbg_edge_rdm(int ptype, int nitems, const int* du, const int* dv, const int* chi, const int* nchunks_u, const int* nchunks_v, const void* partial_u, const void* partial_v,
                                 const double* scale_u, const double* scale_v, void* out, int guard_elems) {
    return guard([&] { edge_rdm_mixed(ptype, ptype, nitems, du, dv, chi, nchunks_u, nchunks_v, partial_u, partial_v, scale_u, scale_v, out, guard_elems); });
}
// tnqs_rdm_edges with the bound on a batch's chain workspace given explicitly
extern "C" int tnqs_dbg_rdm_edges_ws(tnqs_handle h, int n_edges, const int32_t* eu, const int32_t* ev, double* out, int64_t workspace_bytes, int* nbatches_out) {
    return guard([&] {
        if (workspace_bytes < 1) throw Err(TNQS_ERR_INVALID, "dbg_rdm_edges_ws: the workspace bound must be positive");
        rdm_edges(S(h), n_edges, eu, ev, out, (size_t)workspace_bytes, nbatches_out);
    });
}
// path_apply_kernel<P, T> (kernels_rdm.hip), ONE launch over nitems (environment, transfer matrix) pairs set up as engine_paths.cpp sets them up: L_in holds the items'
// nchunks_in[i] chunks of (d chi_a)^2 numbers of type P one after the other, T the items' chi_b^2 x chi_a^2 matrices of the state's type, scale one double per item (0: a
// null pointer), L_out ksplit[i] chunks of (d chi_b)^2 complex128 per item between guard bands of `guard_elems` elements; ksplit[i] = 0: as plan_path_apply chooses
extern "C" int tnqs_dbg_path_apply(int ptype_in, int dtype, int nitems, const int* d, const int* chi_a, const int* chi_b, const int* nchunks_in, const int* ksplit, const void* L_in, const void* T,
                                   const double* scale, void* L_out, int guard_elems) {
    return guard([&] {
        need_gpu();
        if ((ptype_in != 0 && ptype_in != 1) || !is_dtype(dtype) || nitems < 1 || !d || !chi_a || !chi_b || !nchunks_in || !ksplit || !L_in || !T || !scale || !L_out || guard_elems < 0)
            throw Err(TNQS_ERR_INVALID, "dbg_path_apply: bad arguments");
        const size_t psz = ptype_in == 0 ? 8 : 16, esz = esz_of(dtype);
        std::vector<PathApplyItem> items(nitems);
        for (int i = 0; i < nitems; ++i) {
            if (d[i] < 1 || chi_a[i] < 1 || chi_b[i] < 1 || nchunks_in[i] < 1 || ksplit[i] < 0) throw Err(TNQS_ERR_INVALID, "dbg_path_apply: dimensions and chunk counts >= 1, splits >= 0");
            if (d[i] * d[i] > 16) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_path_apply: more than 16 rows (d > 4)");
            if ((size_t)chi_a[i] * chi_a[i] * chi_b[i] * chi_b[i] > (size_t)INT_MAX / 4) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_path_apply: bond dimension too large");
            items[i] = PathApplyItem{nullptr, nullptr, nullptr, nullptr, d[i], chi_a[i], chi_b[i], nchunks_in[i], ksplit[i], 0, 0};
        }
        const int wgs = plan_path_apply(items.data(), nitems);
        for (int i = 0; i < nitems; ++i) if (ksplit[i] == 0 ? items[i].ksplit < 1 : items[i].ksplit != ksplit[i]) throw Err(TNQS_ERR_INVALID, "dbg_path_apply: the plan changed a given split");
        Slots sL, sT, sS; Guarded gO((size_t)guard_elems * 16);
        for (int i = 0; i < nitems; ++i) {
            const size_t ka = (size_t)d[i] * chi_a[i], kb = (size_t)d[i] * chi_b[i];
            sL.add((size_t)nchunks_in[i] * ka * ka * psz); sT.add((size_t)chi_a[i] * chi_a[i] * chi_b[i] * chi_b[i] * esz); sS.add(8); gO.add((size_t)items[i].ksplit * kb * kb * 16);
        }
        alloc_all(sL, sT, sS, gO);
        put_all(sL, L_in); put_all(sT, T);
        for (int i = 0; i < nitems; ++i) {
            sS.put(i, &scale[i]);
            items[i].L_in = sL.at(i); items[i].T = sT.at(i); items[i].L_out = gO.at(i); items[i].scale = scale[i] != 0.0 ? reinterpret_cast<const double*>(sS.at(i)) : nullptr;
        }
        up_all(sL, sT, sS); gO.up(L_out); DevItems<PathApplyItem> dI(items);
        if (dtype == TNQS_C64) { if (ptype_in == 0) launch_path_apply<float, float>(nullptr, dI.get(), nitems, wgs); else launch_path_apply<double, float>(nullptr, dI.get(), nitems, wgs); }
        else { if (ptype_in == 0) launch_path_apply<float, double>(nullptr, dI.get(), nitems, wgs); else launch_path_apply<double, double>(nullptr, dI.get(), nitems, wgs); }
        HIPCHK(hipDeviceSynchronize());
        gO.down(L_out, "L_out");
    });
}
// HOST ONLY: plan_path_apply on a launch of nitems items
extern "C" int tnqs_dbg_path_apply_plan(int nitems, const int* chi_a, const int* chi_b, const int* ksplit, int* ksplit_out, int* nrb_out) {
    return guard([&] {
        if (nitems < 1 || !chi_a || !chi_b || !ksplit || !ksplit_out || !nrb_out) throw Err(TNQS_ERR_INVALID, "dbg_path_apply_plan: bad arguments");
        std::vector<PathApplyItem> it(nitems);
        for (int i = 0; i < nitems; ++i) {
            if (chi_a[i] < 1 || chi_b[i] < 1 || ksplit[i] < 0) throw Err(TNQS_ERR_INVALID, "dbg_path_apply_plan: bad item");
            it[i] = PathApplyItem{nullptr, nullptr, nullptr, nullptr, 1, chi_a[i], chi_b[i], 1, ksplit[i], 0, 0};
        }
        plan_path_apply(it.data(), nitems);
        for (int i = 0; i < nitems; ++i) { ksplit_out[i] = it[i].ksplit; nrb_out[i] = it[i].nrb; }
    });
}
// tnqs_rdm_paths with the bound on a batch's workspace given explicitly
extern "C" int tnqs_dbg_rdm_paths_ws(tnqs_handle h, int npaths, const int32_t* path_len, const int32_t* path_verts, double* out, int64_t workspace_bytes, int* nbatches_out) {
    return guard([&] {
        if (workspace_bytes < 1) throw Err(TNQS_ERR_INVALID, "dbg_rdm_paths_ws: the workspace bound must be positive");
        rdm_paths(S(h), npaths, path_len, path_verts, out, (size_t)workspace_bytes, nbatches_out);
    });
}

// bond entanglement spectra (kernels_spectrum.hip), stages A-D over nitems bonds of different chi exactly as engine_spectra.cpp runs them (fill_bond_spec_items,
// launch_bond_spectra_stages): m1 / m2 hold the items' chi x chi messages one after the other in the state's type, present[2 i], present[2 i + 1] = 0 hands the kernels a
// null pointer for m1 / m2 (identity); the cutoff follows from the dtype.  out: chi[i] doubles per item between guard bands of `guard_elems` doubles; flags_out: one int per
// item (bit 1: a message eigenvalue <= -cutoff, bit 2: trace not positive and finite)
extern "C" int tnqs_dbg_bond_spectrum(int dtype, int nitems, const int* chi, const void* m1, const void* m2, const int* present, double* out, int* flags_out, int guard_elems) {
    return guard([&] {
        need_gpu();
        post_check("dbg_bond_spectrum", dtype, nitems, chi, guard_elems);
        if (!m1 || !m2 || !present || !out || !flags_out) throw Err(TNQS_ERR_INVALID, "dbg_bond_spectrum: bad arguments");
        const size_t esz = esz_of(dtype);
        Slots s1, s2, sH, sV, sW, sV2; Guarded gO((size_t)guard_elems * 8);
        for (int i = 0; i < nitems; ++i) {
            const size_t nn = (size_t)chi[i] * chi[i];
            s1.add(nn * esz); s2.add(nn * esz); gO.add((size_t)chi[i] * 8);
            for (Slots* s : {&sH, &sV, &sW, &sV2}) s->add(nn * 16);
        }
        alloc_all(s1, s2, sH, sV, sW, sV2, gO);
        put_all(s1, m1); put_all(s2, m2);
        DBuf dTr(8 * (size_t)nitems), dFlag(sizeof(int) * (size_t)nitems);
        HIPCHK(hipMemset(dFlag.p, 0, sizeof(int) * (size_t)nitems));
        std::vector<BondSpecBufs> bufs(nitems);
        for (int i = 0; i < nitems; ++i)
            bufs[i] = BondSpecBufs{present[2 * i] ? s1.at(i) : nullptr, present[2 * i + 1] ? s2.at(i) : nullptr, sH.at(i), sV.at(i), sW.at(i), sV2.at(i),
                                   (double*)dTr.p + i, (double*)gO.at(i), chi[i], (int*)dFlag.p + i};
        std::vector<EnvItem> ei; std::vector<JacobiItem> j1, j2; std::vector<BondSpecItem> items;
        const BondSpecLaunch L = fill_bond_spec_items(bufs, bond_spectrum_cutoff(dtype), ei, j1, j2, items);
        DevItems<EnvItem> dE(nitems); DevItems<JacobiItem> dJ1(nitems), dJ2(nitems); DevItems<BondSpecItem> dI(nitems);
        up_all(s1, s2, sH, sV, sW, sV2);
        gO.up(out);
        dE.up(ei); dJ1.up(j1); dJ2.up(j2); dI.up(items);
        by_dtype(dtype, [&](auto t) { launch_bond_spectra_stages<decltype(t)>(nullptr, dE.get(), dJ1.get(), dJ2.get(), dI.get(), L); });
        HIPCHK(hipDeviceSynchronize());
        for (Slots* s : {&sH, &sV, &sW, &sV2}) s->down("the bond-spectrum workspace");
        gO.down(out, "out");
        dFlag.down(flags_out, sizeof(int) * (size_t)nitems);
    });
}

// ---- overlap of two states (kernels_inner.hip), the descriptors filled as engine_inner.cpp run_batch fills them -----------------------------------------------
// ONE launch_inner_gram<T> over nitems items (PA, Ka, Kb, PB), then launch_inner_finalize<T> with normalize = 0 as the chunk sum
extern "C" int tnqs_dbg_inner_gram(int dtype, int nitems, const int* shape, const void* X, const void* Y, void* out, int max_chunks, int* nchunks_out, int guard_elems, int* route) {
    return guard([&] {
        if (!is_dtype(dtype) || nitems < 1 || !shape || !X || !out || guard_elems < 0) throw Err(TNQS_ERR_INVALID, "dbg_inner_gram: bad arguments");
        const size_t esz = esz_of(dtype);
        Slots sX, sY, sP; Guarded gO((size_t)guard_elems * esz);
        std::vector<InnerGramItem> gi(nitems); std::vector<int> npart(nitems);
        for (int i = 0; i < nitems; ++i) {
            const int* q = shape + 4 * i;
            if (q[0] < 1 || q[1] < 1 || q[2] < 1 || q[3] < 1 || (long long)q[0] * q[3] > INT_MAX / 64) throw Err(TNQS_ERR_INVALID, "dbg_inner_gram: bad shape");
            if (!inner_gram_covers(q[1], q[2])) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_inner_gram: the rectangular Gram takes 1 <= Ka, Kb <= 64");
            if (!Y && q[1] != q[2]) throw Err(TNQS_ERR_INVALID, "dbg_inner_gram: Y == X needs Ka == Kb");
            gi[i] = InnerGramItem{}; gi[i].PA = q[0]; gi[i].Ka = q[1]; gi[i].Kb = q[2]; gi[i].PB = q[3];
            sX.add((size_t)q[0] * q[1] * q[3] * esz); if (Y) sY.add((size_t)q[0] * q[2] * q[3] * esz); gO.add((size_t)q[1] * q[2] * esz);
        }
        need_gpu();
        const int chunks = plan_inner_gram(gi.data(), nitems, esz, max_chunks, npart.data());
        for (int i = 0; i < nitems; ++i) sP.add((size_t)npart[i] * gi[i].Ka * gi[i].Kb * esz);
        sX.alloc(); if (Y) sY.alloc(); alloc_all(sP, gO);
        put_all(sX, X); if (Y) put_all(sY, Y);
        std::vector<InnerFinalItem> fi(nitems);
        for (int i = 0; i < nitems; ++i) {
            gi[i].X = sX.at(i); gi[i].Y = Y ? sY.at(i) : sX.at(i); gi[i].partial = sP.at(i);
            fi[i] = InnerFinalItem{sP.at(i), npart[i], gi[i].Ka, gi[i].Kb, nullptr, gO.at(i), nullptr, nullptr, 0};
        }
        DevItems<InnerGramItem> dG(gi); DevItems<InnerFinalItem> dF(fi);
        sX.up(); if (Y) sY.up(); sP.up(); gO.up(out);
        by_dtype(dtype, [&](auto t) { launch_inner_gram<decltype(t)>(nullptr, dG.get(), nitems, chunks); launch_inner_finalize<decltype(t)>(nullptr, dF.get(), nitems); });
        HIPCHK(hipDeviceSynchronize());
        sP.down("the Gram partials"); gO.down(out, "out");
        if (nchunks_out) std::copy(npart.begin(), npart.end(), nchunks_out);
        if (route) *route = TNQS_DBG_ROUTE_INNER_MFMA;
    });
}
// ONE launch_inner_finalize<T> over nitems messages of rows[i] x cols[i]
extern "C" int tnqs_dbg_inner_finalize(int dtype, int nitems, const int* rows, const int* cols, const int* nchunks, const void* partials, const void* old_msg, const int* has_old,
                                       const int* normalize, void* new_msg, double* diff, double* sum, int guard_elems) {
    return guard([&] {
        if (!is_dtype(dtype) || nitems < 1 || !rows || !cols || !nchunks || !partials || !normalize || !new_msg || (old_msg && !has_old) || guard_elems < 0)
            throw Err(TNQS_ERR_INVALID, "dbg_inner_finalize: bad arguments");
        const size_t esz = esz_of(dtype);
        Slots sP, sOld; Guarded gN((size_t)guard_elems * esz);
        for (int i = 0; i < nitems; ++i) {
            if (rows[i] < 1 || cols[i] < 1 || nchunks[i] < 1) throw Err(TNQS_ERR_INVALID, "dbg_inner_finalize: rows, cols, nchunks >= 1");
            if (!inner_gram_covers(rows[i], cols[i])) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_inner_finalize: rows, cols <= 64");
            const size_t mb = (size_t)rows[i] * cols[i] * esz;
            sP.add(mb * nchunks[i]); sOld.add(mb); gN.add(mb);
        }
        need_gpu();
        alloc_all(sP, sOld, gN);
        put_all(sP, partials);
        DBuf dD(sizeof(double) * nitems), dS(sizeof(double) * 2 * nitems); DevItems<InnerFinalItem> dF(nitems);
        std::vector<InnerFinalItem> fi(nitems);
        size_t om = 0;
        for (int i = 0; i < nitems; ++i) {
            const bool old = old_msg && has_old[i]; if (old) sOld.put(i, (const char*)old_msg + om);
            om += sOld.len[i];
            fi[i] = InnerFinalItem{sP.at(i), nchunks[i], rows[i], cols[i], old ? sOld.at(i) : nullptr, gN.at(i), diff ? (double*)dD.p + i : nullptr, sum ? (double*)dS.p + 2 * i : nullptr, normalize[i]};
        }
        up_all(sP, sOld); gN.up(new_msg); dF.up(fi);
        by_dtype(dtype, [&](auto t) { launch_inner_finalize<decltype(t)>(nullptr, dF.get(), nitems); });
        HIPCHK(hipDeviceSynchronize());
        gN.down(new_msg, "new_msg");
        if (diff) dD.down(diff, sizeof(double) * nitems);
        if (sum) dS.down(sum, sizeof(double) * 2 * nitems);
    });
}
// ONE launch_inner_scalar<T> over nitems vertex / edge scalars, the descriptors filled as engine_inner.cpp (inner_bp) fills them: present[2 i], [2 i + 1]: m_i, mr_i
// (0: a null pointer = the rectangular delta); has_rawsum[i], has_scale[2 i], [2 i + 1]: 0 hands the kernel a null pointer
extern "C" int tnqs_dbg_inner_scalar(int dtype, int nitems, const int* rows, const int* cols, const void* m, const void* mr, const int* present, const double* rawsum, const int* has_rawsum,
                                     const int* normalize, const double* scale_a, const double* scale_b, const int* has_scale, double* out, int guard_elems) {
    return guard([&] {
        if (!is_dtype(dtype) || nitems < 1 || !rows || !cols || !m || !mr || !present || !rawsum || !has_rawsum || !normalize || !scale_a || !scale_b ||
            !has_scale || !out || guard_elems < 0)
            throw Err(TNQS_ERR_INVALID, "dbg_inner_scalar: bad arguments");
        const size_t esz = esz_of(dtype);
        Slots sM, sR, sSum, sSc; Guarded gO((size_t)guard_elems * 16);
        for (int i = 0; i < nitems; ++i) {
            if (rows[i] < 1 || cols[i] < 1) throw Err(TNQS_ERR_INVALID, "dbg_inner_scalar: rows, cols >= 1");
            if (!inner_gram_covers(rows[i], cols[i])) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_inner_scalar: rows, cols <= 64");
            const size_t mb = (size_t)rows[i] * cols[i] * esz;
            sM.add(mb); sR.add(mb); sSum.add(16); sSc.add(8); sSc.add(8); gO.add(16);
        }
        need_gpu();
        alloc_all(sM, sR, sSum, sSc, gO);
        put_all(sM, m); put_all(sR, mr); put_all(sSum, rawsum);
        std::vector<InnerScalarItem> si(nitems);
        for (int i = 0; i < nitems; ++i) {
            sSc.put(2 * i, scale_a + i); sSc.put(2 * i + 1, scale_b + i);
            si[i] = InnerScalarItem{present[2 * i] ? sM.at(i) : nullptr, present[2 * i + 1] ? sR.at(i) : nullptr, rows[i], cols[i], has_rawsum[i] ? (const double*)sSum.at(i) : nullptr,
                                    normalize[i], has_scale[2 * i] ? (const double*)sSc.at(2 * i) : nullptr, has_scale[2 * i + 1] ? (const double*)sSc.at(2 * i + 1) : nullptr, (double*)gO.at(i)};
        }
        up_all(sM, sR, sSum, sSc); gO.up(out); DevItems<InnerScalarItem> dI(si);
        by_dtype(dtype, [&](auto t) { launch_inner_scalar<decltype(t)>(nullptr, dI.get(), nitems); });
        HIPCHK(hipDeviceSynchronize());
        gO.down(out, "out");
    });
}
// tnqs_inner_bp with the bound on a batch's chain workspace given explicitly
extern "C" int tnqs_dbg_inner_bp_ws(tnqs_handle ket, tnqs_handle bra, const tnqs_bp_opts* opts, double* out_log_re_im, int* niter, double* final_diff, int64_t workspace_bytes, int* nbatches_out) {
    return guard([&] {
        if (workspace_bytes < 1) throw Err(TNQS_ERR_INVALID, "dbg_inner_bp_ws: the workspace bound must be positive");
        inner_bp(S(ket), S(bra), opts, out_log_re_im, niter, final_diff, (size_t)workspace_bytes, nbatches_out);
    });
}

// ---- bitstring amplitudes (kernels_amp.hip), the descriptors filled as engine_amp.cpp run_batch fills them for one chunk of strings ------------------------------------
// ONE launch_amp_leg_gemm<T> over the groups of nitems jobs (d, PA, K, PB, nstr): per job and site value g < d the strings with x = g are one item, an empty group none
extern "C" int tnqs_dbg_amp_leg_gemm(int dtype, int nitems, const int* shape, const void* T, const int32_t* x, const void* M, const int* has_m, void* R, int guard_elems) {
    return guard([&] {
        if (!is_dtype(dtype) || nitems < 1 || !shape || !T || !x || !M || !has_m || !R || guard_elems < 0) throw Err(TNQS_ERR_INVALID, "dbg_amp_leg_gemm: bad arguments");
        const size_t esz = esz_of(dtype);
        Slots sT, sM; Guarded gR((size_t)guard_elems * esz);
        std::vector<int> idx; std::vector<size_t> xoff(nitems + 1, 0);
        for (int i = 0; i < nitems; ++i) {
            const int* q = shape + 5 * i;
            if (q[0] < 1 || q[1] < 1 || q[3] < 1 || q[4] < 1 || (long long)q[1] * q[3] > (1LL << 30) / q[4]) throw Err(TNQS_ERR_INVALID, "dbg_amp_leg_gemm: bad shape");
            if (!amp_covers(q[2])) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_amp_leg_gemm: the leg GEMM takes 1 <= K <= 64");
            xoff[i + 1] = xoff[i] + q[4];
            for (int p = 0; p < q[4]; ++p) if (x[xoff[i] + p] < 0 || x[xoff[i] + p] >= q[0]) throw Err(TNQS_ERR_INVALID, "dbg_amp_leg_gemm: a site value outside 0 .. d - 1");
            sT.add((size_t)q[0] * q[1] * q[2] * q[3] * esz); sM.add((size_t)q[2] * q[4] * esz); gR.add((size_t)q[1] * q[3] * q[4] * esz);
        }
        need_gpu();
        alloc_all(sT, sM, gR);
        put_all(sT, T); put_all(sM, M);
        idx.resize(xoff[nitems]);
        DBuf dIdx(sizeof(int) * idx.size());
        std::vector<AmpGemmItem> gi;
        for (int i = 0; i < nitems; ++i) {
            const int* q = shape + 5 * i; const int32_t* xi = x + xoff[i];
            std::vector<int> off(q[0] + 1, 0);
            for (int p = 0; p < q[4]; ++p) ++off[xi[p] + 1];
            for (int g = 0; g < q[0]; ++g) off[g + 1] += off[g];
            std::vector<int> at(off.begin(), off.end() - 1);
            for (int p = 0; p < q[4]; ++p) idx[xoff[i] + at[xi[p]]++] = p;
            for (int g = 0; g < q[0]; ++g) {
                AmpGemmItem it{};
                it.d = q[0]; it.PA = q[1]; it.K = q[2]; it.PB = q[3]; it.ncols = off[g + 1] - off[g];
                if (!it.ncols) continue;
                it.T = sT.at(i) + (size_t)g * esz; it.M = has_m[i] ? sM.at(i) : nullptr; it.idx = (const int*)dIdx.p + xoff[i] + off[g]; it.R = gR.at(i);
                gi.push_back(it);
            }
        }
        const int tiles = plan_amp_gemm(gi.data(), (int)gi.size());
        up_ints(dIdx, idx.data(), idx.size());
        up_all(sT, sM); gR.up(R); DevItems<AmpGemmItem> dG(gi);
        by_dtype(dtype, [&](auto t) { launch_amp_leg_gemm<decltype(t)>(nullptr, dG.get(), (int)gi.size(), tiles); });
        HIPCHK(hipDeviceSynchronize());
        gR.down(R, "R");
    });
}
// ONE launch_amp_absorb<T> over nitems steps (PA, K, PB, nstr): in_i [PA][K][PB][nstr], m_i [K][nstr] (has_m[i] == 0: a null pointer, all ones), out_i [PA][PB][nstr]
extern "C" int tnqs_dbg_amp_absorb(int dtype, int nitems, const int* shape, const void* in, const void* m, const int* has_m, void* out, int guard_elems) {
    return guard([&] {
        if (!is_dtype(dtype) || nitems < 1 || !shape || !in || !m || !has_m || !out || guard_elems < 0) throw Err(TNQS_ERR_INVALID, "dbg_amp_absorb: bad arguments");
        const size_t esz = esz_of(dtype);
        Slots sI, sM; Guarded gO((size_t)guard_elems * esz);
        for (int i = 0; i < nitems; ++i) {
            const int* q = shape + 4 * i;
            if (q[0] < 1 || q[2] < 1 || q[3] < 1 || (long long)q[0] * q[2] > (1LL << 30) / q[3]) throw Err(TNQS_ERR_INVALID, "dbg_amp_absorb: bad shape");
            if (!amp_covers(q[1])) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_amp_absorb: bond dimensions 1 <= K <= 64");
            sI.add((size_t)q[0] * q[1] * q[2] * q[3] * esz); sM.add((size_t)q[1] * q[3] * esz); gO.add((size_t)q[0] * q[2] * q[3] * esz);
        }
        need_gpu();
        alloc_all(sI, sM, gO);
        put_all(sI, in); put_all(sM, m);
        std::vector<AmpAbsorbItem> ai(nitems);
        for (int i = 0; i < nitems; ++i) {
            const int* q = shape + 4 * i;
            ai[i] = AmpAbsorbItem{}; ai[i].in = sI.at(i); ai[i].m = has_m[i] ? sM.at(i) : nullptr; ai[i].out = gO.at(i); ai[i].PA = q[0]; ai[i].K = q[1]; ai[i].PB = q[2]; ai[i].nstr = q[3];
        }
        const int wgs = plan_amp_absorb(ai.data(), nitems);
        up_all(sI, sM); gO.up(out); DevItems<AmpAbsorbItem> dA(ai);
        by_dtype(dtype, [&](auto t) { launch_amp_absorb<decltype(t)>(nullptr, dA.get(), nitems, wgs); });
        HIPCHK(hipDeviceSynchronize());
        gO.down(out, "out");
    });
}
// ONE launch_amp_finalize<T> over nitems messages of chi[i] x nstr[i]; done: one int per string, the items one after the other (null: no flags)
extern "C" int tnqs_dbg_amp_finalize(int dtype, int nitems, const int* chi, const int* nstr, const void* raw, const void* old_msg, const int* has_old, const int* normalize,
                                     const int* done, void* new_msg, double* diff, double* sum, int guard_elems) {
    return guard([&] {
        if (!is_dtype(dtype) || nitems < 1 || !chi || !nstr || !raw || !old_msg || !has_old || !normalize || !new_msg || !diff || !sum || guard_elems < 0)
            throw Err(TNQS_ERR_INVALID, "dbg_amp_finalize: bad arguments");
        const size_t esz = esz_of(dtype);
        Slots sR, sOld; Guarded gN((size_t)guard_elems * esz);
        std::vector<size_t> soff(nitems + 1, 0);
        for (int i = 0; i < nitems; ++i) {
            if (nstr[i] < 1) throw Err(TNQS_ERR_INVALID, "dbg_amp_finalize: nstr >= 1");
            if (!amp_covers(chi[i])) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_amp_finalize: bond dimensions 1 <= chi <= 64");
            const size_t mb = (size_t)chi[i] * nstr[i] * esz;
            sR.add(mb); sOld.add(mb); gN.add(mb); soff[i + 1] = soff[i] + nstr[i];
        }
        need_gpu();
        alloc_all(sR, sOld, gN);
        put_all(sR, raw); put_all(sOld, old_msg);
        const size_t ns = soff[nitems];
        DBuf dD(sizeof(double) * ns), dS(sizeof(double) * 2 * ns), dDone(sizeof(int) * ns);
        dD.up(diff, sizeof(double) * ns); dS.up(sum, sizeof(double) * 2 * ns); if (done) up_ints(dDone, done, ns);
        std::vector<AmpFinalItem> fi(nitems);
        for (int i = 0; i < nitems; ++i) {
            AmpFinalItem& it = fi[i]; it = AmpFinalItem{};
            it.raw = sR.at(i); it.old_msg = has_old[i] ? sOld.at(i) : nullptr; it.new_msg = gN.at(i); it.done = done ? (const int*)dDone.p + soff[i] : nullptr;
            it.diff_out = (double*)dD.p + soff[i]; it.sum_out = (double*)dS.p + 2 * soff[i]; it.chi = chi[i]; it.nstr = nstr[i]; it.normalize = normalize[i];
        }
        const int wgs = plan_amp_finalize(fi.data(), nitems);
        up_all(sR, sOld); gN.up(new_msg); DevItems<AmpFinalItem> dF(fi);
        by_dtype(dtype, [&](auto t) { launch_amp_finalize<decltype(t)>(nullptr, dF.get(), nitems, wgs); });
        HIPCHK(hipDeviceSynchronize());
        gN.down(new_msg, "new_msg");
        dD.down(diff, sizeof(double) * ns); dS.down(sum, sizeof(double) * 2 * ns);
    });
}
// tnqs_amplitudes_bp with the workspace bound given explicitly: it sizes the batches of jobs and the chunks of strings
extern "C" int tnqs_dbg_amplitudes_bp_ws(tnqs_handle h, int nstrings, const int32_t* configs, const tnqs_bp_opts* opts, double* out_log_re_im, int32_t* niter, double* final_diff,
                                         int32_t* flags, int64_t workspace_bytes, int* nbatches_out) {
    return guard([&] {
        if (workspace_bytes < 1) throw Err(TNQS_ERR_INVALID, "dbg_amplitudes_bp_ws: the workspace bound must be positive");
        amplitudes_bp(S(h), nstrings, configs, opts, out_log_re_im, niter, final_diff, flags, (size_t)workspace_bytes, nbatches_out);
    });
}
