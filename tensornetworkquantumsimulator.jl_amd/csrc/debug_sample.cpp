// debug_sample.cpp -- kernel-level test entry points (include/tnqs_debug.h) of the sampling kernels (kernels_sample.hip) and of the one-site kernels with their
// pending scale factor (kernels_util.hip: site1_c64, norm_factor, scale).
#include "debug_util.hpp"

using namespace tnqs;

// ---- sampling (kernels_sample.hip), launched as engine_sample.cpp launches them ------------------------------------------------------------------------------------
// site_prob_partial_kernel<T> on one site tensor of n = d k elements: the raw nblocks x 16 partial array between guard bands of `guard_elems` doubles.  nblocks == 0: the
// engine's plan_site_prob.  partial == NULL: only *nblocks_out is filled (HOST ONLY)
extern "C" int tnqs_dbg_site_prob(int dtype, int n, int d, const void* tabs, const void* psi, int nblocks, double* partial, int guard_elems, int* nblocks_out) {
    return guard([&] {
        if (!is_dtype(dtype) || n < 1 || d < 1 || d > 16 || n % d || nblocks < 0 || nblocks > 4096 || guard_elems < 0 || (partial && (!tabs || !psi)))
            throw Err(TNQS_ERR_INVALID, "dbg_site_prob: bad arguments");
        const int nb = nblocks ? nblocks : plan_site_prob((size_t)n, d);
        if (nblocks_out) *nblocks_out = nb;
        if (!partial) return;
        need_gpu();
        const size_t esz = esz_of(dtype);
        Slots sT, sP; Guarded gP((size_t)guard_elems * 8);
        sT.add((size_t)n * esz); sP.add((size_t)n * esz); gP.add((size_t)nb * 16 * 8);
        alloc_all(sT, sP, gP);
        sT.put(0, tabs); sP.put(0, psi);
        up_all(sT, sP); gP.up(partial);
        by_dtype(dtype, [&](auto t) { launch_site_prob_partial<decltype(t)>(nullptr, sT.at(0), sP.at(0), (size_t)n, d, nb, (double*)gP.at(0)); });
        HIPCHK(hipDeviceSynchronize());
        gP.down(partial, "partial");
    });
}
// site_draw_kernel, one launch per item (the engine launches one per step): partials: nblocks[i] x 16 doubles per item, one item after the other; use_counter[i] == 0: the
// uniform is uniform[i], else counter-based from counter[3 i .. 3 i + 2] = (seed, sample, step) and the kernel gets a null uniform.  p_out: 16 doubles per item (the kernel
// writes d[i]), x_out, px_out: one number per item, all three between guard bands of `guard_elems` elements; status_out[i]: the item's own status word, cleared before its launch
extern "C" int tnqs_dbg_site_draw(int nitems, const int* nblocks, const int* d, const double* partials, const double* neg_tol, const double* uniform, const int* use_counter,
                                  const uint64_t* counter, const int* draw, double* p_out, int* x_out, double* px_out, int* status_out, int guard_elems) {
    return guard([&] {
        if (nitems < 1 || !nblocks || !d || !partials || !neg_tol || !uniform || !use_counter || !counter || !draw || !p_out || !x_out || !px_out || !status_out || guard_elems < 0)
            throw Err(TNQS_ERR_INVALID, "dbg_site_draw: bad arguments");
        Slots sPart, sU; Guarded gP((size_t)guard_elems * 8), gX((size_t)guard_elems * 4), gPx((size_t)guard_elems * 8);
        for (int i = 0; i < nitems; ++i) {
            if (nblocks[i] < 1 || d[i] < 1 || d[i] > 16) throw Err(TNQS_ERR_INVALID, "dbg_site_draw: nblocks >= 1, 1 <= d <= 16");
            sPart.add((size_t)nblocks[i] * 16 * 8); sU.add(8); gP.add(16 * 8); gX.add(4); gPx.add(8);
        }
        need_gpu();
        alloc_all(sPart, sU, gP, gX, gPx);
        put_all(sPart, partials); put_all(sU, uniform);
        DBuf dSt(sizeof(int) * nitems);
        HIPCHK(hipMemset(dSt.p, 0, sizeof(int) * nitems));
        up_all(sPart, sU); gP.up(p_out); gX.up(x_out); gPx.up(px_out);
        for (int i = 0; i < nitems; ++i)
            launch_site_draw(nullptr, (const double*)sPart.at(i), nblocks[i], d[i], neg_tol[i], use_counter[i] ? nullptr : (const double*)sU.at(i), counter[3 * i], counter[3 * i + 1],
                             counter[3 * i + 2], draw[i] != 0, (double*)gP.at(i), (int*)gX.at(i), (double*)gPx.at(i), (int*)dSt.p + i);
        HIPCHK(hipDeviceSynchronize());
        gP.down(p_out, "p_out"); gX.down(x_out, "x_out"); gPx.down(px_out, "px_out");
        dSt.down(status_out, sizeof(int) * nitems);
    });
}
// site_project_kernel<T>: out[i] = psi[x + d i], i < nout; x_on_device != 0: x goes through device memory and the host argument is one that clamps to another index
extern "C" int tnqs_dbg_site_project(int dtype, int nout, int d, const void* psi, int x, int x_on_device, void* out, int guard_elems) {
    return guard([&] {
        if (!is_dtype(dtype) || nout < 1 || d < 1 || d > 16 || (long long)nout * d > INT_MAX / 2 || !psi || !out || guard_elems < 0)
            throw Err(TNQS_ERR_INVALID, "dbg_site_project: bad arguments");
        need_gpu();
        const size_t esz = esz_of(dtype);
        Slots sP, sX; Guarded gO((size_t)guard_elems * esz);
        sP.add((size_t)nout * d * esz); sX.add(4); gO.add((size_t)nout * esz);
        alloc_all(sP, sX, gO);
        sP.put(0, psi); sX.put(0, &x);
        up_all(sP, sX); gO.up(out);
        const int* dx = x_on_device ? (const int*)sX.at(0) : nullptr;
        const int xh = x_on_device ? (x <= 0 ? INT_MAX : -1) : x;
        by_dtype(dtype, [&](auto t) { launch_site_project<decltype(t)>(nullptr, sP.at(0), gO.at(0), (size_t)nout, d, dx, xh); });
        HIPCHK(hipDeviceSynchronize());
        gO.down(out, "out");
    });
}

// ---- the ComplexF32 d = 2 one-site gate with normalisation (kernels_util.hip), set up as apply_one_site_batch / norm_and_replace / materialize_scale set it up ----------
// ONE launch_site1_c64 over nitems tensors of npairs[i] (s = 0, 1) pairs; gates: 8 doubles per item, column-major G[s' + 2 s] re/im as the C ABI takes them, packed by
// pack_site1_gate.  normalize != 0: the kernel leaves nbx norm partials per item in `partials` (nitems nbx doubles between two guard bands) and ONE launch_norm_factor
// turns them into `factors` (one double per item between guard bands, 256-byte slots on the device); normalize == 0: the kernel gets a null pointer, both stay as they were
extern "C" int tnqs_dbg_site1(int nitems, const int* npairs, const void* in, const double* gates, int nbx, int normalize, void* out, double* partials, double* factors, int guard_elems) {
    return guard([&] {
        if (nitems < 1 || !npairs || !in || !gates || nbx < 1 || nbx > 65535 || !out || !partials || !factors || guard_elems < 0) throw Err(TNQS_ERR_INVALID, "dbg_site1: bad arguments");
        Slots sIn; Guarded gO((size_t)guard_elems * 8), gPart((size_t)guard_elems * 8), gF((size_t)guard_elems * 8);
        for (int i = 0; i < nitems; ++i) {
            if (npairs[i] < 1) throw Err(TNQS_ERR_INVALID, "dbg_site1: npairs >= 1");
            sIn.add((size_t)npairs[i] * 16); gO.add((size_t)npairs[i] * 16); gF.add(8);
        }
        gPart.add((size_t)nitems * nbx * 8);
        need_gpu();
        alloc_all(sIn, gO, gPart, gF);
        put_all(sIn, in);
        std::vector<Site1Item> items(nitems); std::vector<NormFactorItem> nf(nitems);
        for (int i = 0; i < nitems; ++i) {
            Site1Item it{}; it.in = sIn.at(i); it.out = gO.at(i); it.npairs = (size_t)npairs[i];
            pack_site1_gate(gates + 8 * (size_t)i, it.g);
            items[i] = it;
            nf[i] = NormFactorItem{(const double*)gPart.at(0) + (size_t)i * nbx, nbx, (double*)gF.at(i)};
        }
        DevItems<Site1Item> dI(items); DevItems<NormFactorItem> dN(nf);
        sIn.up(); gO.up(out); gPart.up(partials); gF.up(factors);
        launch_site1_c64(nullptr, dI.get(), nitems, nbx, normalize ? (double*)gPart.at(0) : nullptr);
        if (normalize) launch_norm_factor(nullptr, dN.get(), nitems);
        HIPCHK(hipDeviceSynchronize());
        gO.down(out, "out"); gPart.down(partials, "partials"); gF.down(factors, "factors");
    });
}
// ONE launch_norm_factor: item i has npart[i] partials (one item after the other); factors: one double per item between guard bands
extern "C" int tnqs_dbg_norm_factor(int nitems, const int* npart, const double* partials, double* factors, int guard_elems) {
    return guard([&] {
        if (nitems < 1 || !npart || !partials || !factors || guard_elems < 0) throw Err(TNQS_ERR_INVALID, "dbg_norm_factor: bad arguments");
        Slots sP; Guarded gF((size_t)guard_elems * 8);
        for (int i = 0; i < nitems; ++i) { if (npart[i] < 0) throw Err(TNQS_ERR_INVALID, "dbg_norm_factor: npart >= 0"); sP.add((size_t)npart[i] * 8); gF.add(8); }
        need_gpu();
        alloc_all(sP, gF);
        put_all(sP, partials);
        std::vector<NormFactorItem> nf(nitems);
        for (int i = 0; i < nitems; ++i) nf[i] = NormFactorItem{(const double*)sP.at(i), npart[i], (double*)gF.at(i)};
        sP.up(); gF.up(factors); DevItems<NormFactorItem> dN(nf);
        launch_norm_factor(nullptr, dN.get(), nitems);
        HIPCHK(hipDeviceSynchronize());
        gF.down(factors, "factors");
    });
}
// ONE launch_scale<T>: dst_i = src_i * (T)factor[i], len[i] numbers per item, the factor read from device memory as the pending scale factor is
extern "C" int tnqs_dbg_scale(int dtype, int nitems, const int* len, const void* src, const double* factor, void* dst, int guard_elems) {
    return guard([&] {
        if (!is_dtype(dtype) || nitems < 1 || !len || !src || !factor || !dst || guard_elems < 0) throw Err(TNQS_ERR_INVALID, "dbg_scale: bad arguments");
        const size_t esz = esz_of(dtype);
        Slots sS, sF; Guarded gD((size_t)guard_elems * esz);
        for (int i = 0; i < nitems; ++i) { if (len[i] < 1) throw Err(TNQS_ERR_INVALID, "dbg_scale: len >= 1"); sS.add((size_t)len[i] * esz); sF.add(8); gD.add((size_t)len[i] * esz); }
        need_gpu();
        alloc_all(sS, sF, gD);
        put_all(sS, src); put_all(sF, factor);
        std::vector<ScaleItem> items(nitems);
        for (int i = 0; i < nitems; ++i) items[i] = ScaleItem{sS.at(i), gD.at(i), (size_t)len[i], (const double*)sF.at(i)};
        up_all(sS, sF); gD.up(dst); DevItems<ScaleItem> dI(items);
        by_dtype(dtype, [&](auto t) { launch_scale<decltype(t)>(nullptr, dI.get(), nitems); });
        HIPCHK(hipDeviceSynchronize());
        gD.down(dst, "dst");
    });
}
// the pending real scale factor of site v (State::sscale): 1 when none is pending
extern "C" int tnqs_dbg_pending_scale(tnqs_handle h, int v, double* factor) {
    return guard([&] {
        if (!factor) throw Err(TNQS_ERR_INVALID, "dbg_pending_scale: null output");
        State* s = S(h);
        if (v < 0 || v >= s->g->nv) throw Err(TNQS_ERR_INVALID, "dbg_pending_scale: bad vertex");
        double f = 1.0;
        if (s->sscale[v]) {
            HIPCHK(hipSetDevice(s->device));
            HIPCHK(hipStreamSynchronize(s->stream));
            HIPCHK(hipMemcpy(&f, s->sscale[v]->p, 8, hipMemcpyDeviceToHost));
        }
        *factor = f;
    });
}
