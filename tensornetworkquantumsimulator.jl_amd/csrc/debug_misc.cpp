// debug_misc.cpp -- the kernel-level test entry points of the small kernels that run inside larger calls only: the utilities of kernels_util.hip (permutation, random fill,
// identity, sum, record packing), copy_items (kernels_chi64.hip), loop_dot (kernels_loop.hip), bmps_norm (kernels_bmps.hip) and the two closing kernels of the amplitude
// sweep (kernels_amp.hip).  Each calls the engine's own launch_* / plan_* function and nothing else.
#include "debug_util.hpp"

using namespace tnqs;

extern "C" int tnqs_dbg_permute(int dtype, int ndim, const int32_t* dims_out, const int64_t* stride_in, int64_t in_elems, const void* in, void* out, int guard_elems) {
    return guard([&] {
        if (!is_dtype(dtype) || ndim < 1 || ndim > 8 || !dims_out || !stride_in || in_elems < 1 || !in || !out || guard_elems < 0) throw Err(TNQS_ERR_INVALID, "dbg_permute: bad arguments");
        PermItem it{}; it.ndim = ndim; it.n = 1;
        long long lo = 0, hi = 0;       // the smallest and the largest source index
        for (int k = 0; k < ndim; ++k) {
            if (dims_out[k] < 1) throw Err(TNQS_ERR_INVALID, "dbg_permute: bad dimension");
            it.dims_out[k] = dims_out[k]; it.stride_in[k] = stride_in[k]; it.n *= (size_t)dims_out[k];
            const long long span = (long long)(dims_out[k] - 1) * stride_in[k];
            if (span > 0) hi += span; else lo += span;
        }
        if (lo < 0 || hi >= in_elems || it.n > ((size_t)1 << 28)) throw Err(TNQS_ERR_INVALID, "dbg_permute: a source index falls outside the input");
        need_gpu();
        const size_t esz = esz_of(dtype);
        Slots sI; Guarded gO((size_t)guard_elems * esz);
        sI.add((size_t)in_elems * esz); gO.add(it.n * esz);
        alloc_all(sI, gO); sI.put(0, in); sI.up(); gO.up(out);
        it.in = sI.at(0); it.out = gO.at(0);
        by_dtype(dtype, [&](auto t) { launch_permute<decltype(t)>(nullptr, it); });
        HIPCHK(hipDeviceSynchronize());
        gO.down(out, "the permuted tensor");
    });
}

extern "C" int tnqs_dbg_random_fill(int dtype, int64_t n, uint64_t seed, double scale, int real_only, void* out, int guard_elems) {
    return guard([&] {
        if (!is_dtype(dtype) || n < 0 || n > ((int64_t)1 << 28) || !out || guard_elems < 0) throw Err(TNQS_ERR_INVALID, "dbg_random_fill: bad arguments");
        need_gpu();
        const size_t esz = esz_of(dtype);
        Guarded gO((size_t)guard_elems * esz); gO.add((size_t)n * esz); gO.alloc(); gO.up(out);
        by_dtype(dtype, [&](auto t) { launch_random_fill<decltype(t)>(nullptr, gO.at(0), (size_t)n, (unsigned long long)seed, scale, real_only != 0); });
        HIPCHK(hipDeviceSynchronize());
        gO.down(out, "the random fill");
    });
}

extern "C" int tnqs_dbg_identity(int dtype, int n, void* out, int guard_elems) {
    return guard([&] {
        if (!is_dtype(dtype) || n < 1 || n > 4096 || !out || guard_elems < 0) throw Err(TNQS_ERR_INVALID, "dbg_identity: bad arguments");
        need_gpu();
        const size_t esz = esz_of(dtype);
        Guarded gO((size_t)guard_elems * esz); gO.add((size_t)n * n * esz); gO.alloc(); gO.up(out);
        by_dtype(dtype, [&](auto t) { launch_identity<decltype(t)>(nullptr, gO.at(0), n); });
        HIPCHK(hipDeviceSynchronize());
        gO.down(out, "the identity");
    });
}

extern "C" int tnqs_dbg_sum_doubles(int n, const double* in, double* out) {
    return guard([&] {
        if (n < 0 || (n && !in) || !out) throw Err(TNQS_ERR_INVALID, "dbg_sum_doubles: bad arguments");
        need_gpu();
        Slots sI, sO; sI.add(sizeof(double) * (size_t)n); sO.add(sizeof(double));
        alloc_all(sI, sO); if (n) sI.put(0, in); up_all(sI, sO);
        launch_sum_doubles(nullptr, (const double*)sI.at(0), n, (double*)sO.at(0));
        HIPCHK(hipDeviceSynchronize());
        sO.down("the sum"); sO.get(0, out);
    });
}

extern "C" int tnqs_dbg_record_pack(int nitems, const int32_t* info, const double* terr, const double* S, const int32_t* nS, const void* X2, const int64_t* x2_words,
                                    const int64_t* x2_off, const int64_t* dst_bytes, void* dst, double* headers_out, int guard_bytes) {
    return guard([&] {
        if (nitems < 1 || !info || !terr || !S || !nS || !x2_words || !x2_off || !dst_bytes || !dst || !headers_out || guard_bytes < 0) throw Err(TNQS_ERR_INVALID, "dbg_record_pack: bad arguments");
        Slots sInfo, sTerr, sS, sX, sH; Guarded gD((size_t)guard_bytes);
        bool any_x2 = false;
        for (int i = 0; i < nitems; ++i) {
            if (nS[i] < 0 || x2_words[i] < 0 || x2_off[i] < 32 + 8 * (int64_t)nS[i] || (x2_off[i] & 7) || x2_off[i] + 8 * x2_words[i] > dst_bytes[i])
                throw Err(TNQS_ERR_INVALID, "dbg_record_pack: a record does not hold its parts");
            sInfo.add(4 * sizeof(int)); sTerr.add(sizeof(double)); sS.add(sizeof(double) * (size_t)nS[i]); sX.add(8 * (size_t)x2_words[i]); gD.add((size_t)dst_bytes[i]);
            any_x2 = any_x2 || x2_words[i] > 0;
        }
        if (any_x2 && !X2) throw Err(TNQS_ERR_INVALID, "dbg_record_pack: X2 is null");
        need_gpu();
        sH.add(4 * sizeof(double) * (size_t)nitems);
        alloc_all(sInfo, sTerr, sS, sX, sH, gD);
        put_all(sInfo, info); put_all(sTerr, terr); put_all(sS, S); if (any_x2) put_all(sX, X2);
        std::vector<RecordPackItem> ri(nitems); std::vector<const void*> ptrs(nitems);
        for (int i = 0; i < nitems; ++i) {
            ri[i] = RecordPackItem{gD.at(i), (const int*)sInfo.at(i), (const double*)sTerr.at(i), (const double*)sS.at(i), nS[i], x2_words[i] ? sX.at(i) : nullptr, x2_words[i], x2_off[i]};
            ptrs[i] = gD.at(i);
        }
        DevItems<RecordPackItem> dR(ri); DevItems<const void*> dP(ptrs);
        up_all(sInfo, sTerr, sS, sX, sH); gD.up(dst);
        launch_record_pack(nullptr, dR.get(), nitems);
        launch_header_gather(nullptr, dP.get(), nitems, (double*)sH.at(0));
        HIPCHK(hipDeviceSynchronize());
        sH.down("the gathered headers"); sH.get(0, headers_out); gD.down(dst, "the records");
    });
}

extern "C" int tnqs_dbg_copy_items(int nitems, const int64_t* n16, const int32_t* tail8, const void* src, void* dst, int guard_bytes) {
    return guard([&] {
        if (nitems < 1 || !n16 || !src || !dst || guard_bytes < 0) throw Err(TNQS_ERR_INVALID, "dbg_copy_items: bad arguments");
        Slots sS; Guarded gD((size_t)guard_bytes);
        for (int i = 0; i < nitems; ++i) {
            if (n16[i] < 0 || n16[i] > ((int64_t)1 << 26) || (tail8 && (tail8[i] < 0 || tail8[i] > 1))) throw Err(TNQS_ERR_INVALID, "dbg_copy_items: bad length");
            const size_t bytes = 16 * (size_t)n16[i] + (tail8 && tail8[i] ? 8 : 0);
            sS.add(bytes); gD.add(bytes);
        }
        need_gpu();
        alloc_all(sS, gD); put_all(sS, src);
        std::vector<CopyItem> ci(nitems);
        for (int i = 0; i < nitems; ++i) ci[i] = CopyItem{sS.at(i), gD.at(i), (size_t)n16[i], tail8 && tail8[i] ? 1 : 0};
        DevItems<CopyItem> dC(ci);
        sS.up(); gD.up(dst);
        launch_copy_items(nullptr, dC.get(), nitems);
        HIPCHK(hipDeviceSynchronize());
        gD.down(dst, "the copies");
    });
}

extern "C" int tnqs_dbg_loop_dot(int dtype, int nitems, const int64_t* n, const void* X, const void* Y, double* out_re_im, int32_t* nwg_out) {
    return guard([&] {
        if (!is_dtype(dtype) || nitems < 1 || !n || (X && (!Y || !out_re_im))) throw Err(TNQS_ERR_INVALID, "dbg_loop_dot: bad arguments");
        std::vector<LoopDotItem> di(nitems);
        for (int i = 0; i < nitems; ++i) {
            if (n[i] < 0 || (X && n[i] > ((int64_t)1 << 28))) throw Err(TNQS_ERR_INVALID, "dbg_loop_dot: bad length");
            di[i] = LoopDotItem{}; di[i].n = n[i];
        }
        const int wgs = plan_loop_dot(di.data(), nitems);
        if (nwg_out) for (int i = 0; i < nitems; ++i) nwg_out[i] = di[i].nwg;
        if (!X) return;                                                  // host only
        need_gpu();
        const size_t esz = esz_of(dtype);
        Slots sX, sY, sP, sO;                                            // the partials keep the slots' 0xff filling where nothing is written: NaN bytes
        for (int i = 0; i < nitems; ++i) { sX.add((size_t)n[i] * esz); sY.add((size_t)n[i] * esz); sP.add(2 * sizeof(double) * (size_t)di[i].nwg); sO.add(2 * sizeof(double)); }
        alloc_all(sX, sY, sP, sO); put_all(sX, X); put_all(sY, Y);
        for (int i = 0; i < nitems; ++i) { di[i].X = sX.at(i); di[i].Y = sY.at(i); di[i].partial = (double*)sP.at(i); di[i].out = (double*)sO.at(i); }
        DevItems<LoopDotItem> dD(di);
        up_all(sX, sY, sP, sO);
        by_dtype(dtype, [&](auto t) { launch_loop_dot<decltype(t)>(nullptr, dD.get(), nitems, wgs); });
        HIPCHK(hipDeviceSynchronize());
        sP.down("the dot partials"); sO.down("the dot products");
        for (int i = 0; i < nitems; ++i) sO.get(i, out_re_im + 2 * i);
    });
}

extern "C" int tnqs_dbg_bmps_norm(int dtype, int nitems, const int64_t* n, const void* src, const int32_t* normalize, const int32_t* conj, const int32_t* has_dst,
                                  const int32_t* has_norm, void* dst, double* norm_out, int guard_elems) {
    return guard([&] {
        if (!is_dtype(dtype) || nitems < 1 || !n || !src || !normalize || !conj || !has_dst || !has_norm || !dst || !norm_out || guard_elems < 0) throw Err(TNQS_ERR_INVALID, "dbg_bmps_norm: bad arguments");
        const size_t esz = esz_of(dtype);
        Slots sS, sN; Guarded gD((size_t)guard_elems * esz);
        for (int i = 0; i < nitems; ++i) {
            if (n[i] < 1 || n[i] > ((int64_t)1 << 26)) throw Err(TNQS_ERR_INVALID, "dbg_bmps_norm: bad length");
            sS.add((size_t)n[i] * esz); gD.add((size_t)n[i] * esz); sN.add(sizeof(double));
        }
        need_gpu();
        alloc_all(sS, sN, gD); put_all(sS, src); put_all(sN, norm_out);
        std::vector<BmpsNormItem> ni(nitems);
        for (int i = 0; i < nitems; ++i)
            ni[i] = BmpsNormItem{sS.at(i), has_dst[i] ? gD.at(i) : nullptr, n[i], has_norm[i] ? (double*)sN.at(i) : nullptr, normalize[i] ? 1 : 0, conj[i] ? 1 : 0};
        DevItems<BmpsNormItem> dN(ni);
        up_all(sS, sN); gD.up(dst);
        by_dtype(dtype, [&](auto t) { launch_bmps_norm<decltype(t)>(nullptr, dN.get(), nitems); });
        HIPCHK(hipDeviceSynchronize());
        sN.down("the norms"); gD.down(dst, "the normalised vectors");
        for (int i = 0; i < nitems; ++i) sN.get(i, norm_out + i);
    });
}

extern "C" int tnqs_dbg_amp_sweep_end(int nseq, int nstrings, int iter, double tol, const double* diffs, int32_t* done_inout, int32_t* niter_inout, double* fdiff_inout) {
    return guard([&] {
        if (nseq < 1 || nstrings < 1 || !diffs || !done_inout || !niter_inout || !fdiff_inout) throw Err(TNQS_ERR_INVALID, "dbg_amp_sweep_end: bad arguments");
        need_gpu();
        Slots s; s.add(sizeof(double) * (size_t)nseq * nstrings); s.add(sizeof(int) * (size_t)nstrings); s.add(sizeof(int) * (size_t)nstrings); s.add(sizeof(double) * (size_t)nstrings);
        s.alloc(); s.put(0, diffs); s.put(1, done_inout); s.put(2, niter_inout); s.put(3, fdiff_inout); s.up();
        launch_amp_sweep_end(nullptr, (const double*)s.at(0), nseq, nstrings, iter, tol, (int*)s.at(1), (int*)s.at(2), (double*)s.at(3));
        HIPCHK(hipDeviceSynchronize());
        s.down("the sweep's arrays");
        std::vector<double> back((size_t)nseq * nstrings); s.get(0, back.data());
        if (std::memcmp(back.data(), diffs, sizeof(double) * back.size())) throw Err(TNQS_ERR_INVALID, "dbg_amp_sweep_end: the kernel wrote into its input");
        s.get(1, done_inout); s.get(2, niter_inout); s.get(3, fdiff_inout);
    });
}

extern "C" int tnqs_dbg_amp_scalar(int dtype, int nv, int ne, const int32_t* chi, const void* m, const void* mr, const int32_t* present, const double* rawsum, const int32_t* has_rawsum,
                                   const int32_t* normalize, const double* scale, const int32_t* has_scale, const void* site, const int32_t* site_d, const int32_t* is_site,
                                   const int32_t* cfg, int ld, int nstrings, double* out_re_im, int32_t* flags_out, int guard_elems) {
    return guard([&] {
        const int ni = nv + ne;
        if (!is_dtype(dtype) || nv < 0 || ne < 0 || ni < 1 || !chi || !m || !mr || !present || !rawsum || !has_rawsum || !normalize || !scale || !has_scale || !site || !site_d || !is_site ||
            !cfg || ld < nv || nstrings < 1 || !out_re_im || !flags_out || guard_elems < 0) throw Err(TNQS_ERR_INVALID, "dbg_amp_scalar: bad arguments");
        const size_t esz = esz_of(dtype);
        Slots sM, sR, sRaw, sSc, sSite, sCfg; Guarded gO(sizeof(double) * (size_t)guard_elems), gF(sizeof(int) * (size_t)guard_elems);
        for (int i = 0; i < ni; ++i) {
            if (chi[i] < 1 || chi[i] > 64) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_amp_scalar: chi outside 1..64");
            if (site_d[i] < 0 || (is_site[i] && (i >= nv || site_d[i] < 1))) throw Err(TNQS_ERR_INVALID, "dbg_amp_scalar: an isolated vertex is a vertex item with a site vector");
            if (is_site[i]) for (int p = 0; p < nstrings; ++p) { const int c = cfg[(size_t)p * ld + i]; if (c < 0 || c >= site_d[i]) throw Err(TNQS_ERR_INVALID, "dbg_amp_scalar: a site value outside 0 .. d - 1"); }
            sM.add((size_t)chi[i] * nstrings * esz); sR.add((size_t)chi[i] * nstrings * esz); sRaw.add(2 * sizeof(double) * (size_t)nstrings); sSc.add(sizeof(double)); sSite.add((size_t)site_d[i] * esz);
        }
        need_gpu();
        sCfg.add(sizeof(int) * (size_t)ld * nstrings); gO.add(2 * sizeof(double) * (size_t)nstrings); gF.add(sizeof(int) * (size_t)nstrings);
        alloc_all(sM, sR, sRaw, sSc, sSite, sCfg, gO, gF);
        put_all(sM, m); put_all(sR, mr); put_all(sRaw, rawsum); put_all(sSc, scale); put_all(sSite, site); sCfg.put(0, cfg);
        std::vector<AmpScalarItem> si(ni);
        for (int i = 0; i < ni; ++i) {
            AmpScalarItem it{};
            it.chi = chi[i]; it.normalize = normalize[i] ? 1 : 0; it.vertex = i < nv ? i : 0;
            if (is_site[i]) it.site = sSite.at(i);
            else { it.m = present[2 * i] ? sM.at(i) : nullptr; it.mr = present[2 * i + 1] ? sR.at(i) : nullptr; it.rawsum = has_rawsum[i] ? (const double*)sRaw.at(i) : nullptr; }
            it.scale = has_scale[i] ? (const double*)sSc.at(i) : nullptr;
            si[i] = it;
        }
        DevItems<AmpScalarItem> dS(si);
        up_all(sM, sR, sRaw, sSc, sSite, sCfg); gO.up(out_re_im); gF.up(flags_out);
        by_dtype(dtype, [&](auto t) { launch_amp_scalar<decltype(t)>(nullptr, dS.get(), nv, ne, (const int*)sCfg.at(0), ld, nstrings, (double*)gO.at(0), (int*)gF.at(0)); });
        HIPCHK(hipDeviceSynchronize());
        gO.down(out_re_im, "the log amplitudes"); gF.down(flags_out, "the flags");
    });
}
