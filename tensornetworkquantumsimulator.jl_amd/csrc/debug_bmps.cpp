// debug_bmps.cpp -- the kernel-level test entry points of the boundary-MPS kernels (kernels_bmps.hip), the descriptors planned and launched as engine_bmps.cpp does.
#include "debug_util.hpp"

using namespace tnqs;

extern "C" int tnqs_dbg_bmps_contract(int dtype, int nitems, const int32_t* ngroup, const int32_t* dims, const int64_t* strides, const int32_t* conjB, const int64_t* sizes,
                                      const void* A, const void* B, void* C, int guard_elems, int force_chunks, int32_t* nchunks_out) {
    return guard([&] {
        if (!is_dtype(dtype) || nitems < 1 || !ngroup || !dims || !strides || !conjB || !sizes || !A || !B || !C || guard_elems < 0) throw Err(TNQS_ERR_INVALID, "dbg_bmps_contract: bad arguments");
        const size_t esz = esz_of(dtype);
        Slots sA, sB, sP; Guarded gC((size_t)guard_elems * esz);
        std::vector<BmpsContractItem> ci(nitems); std::vector<size_t> npart(nitems);
        for (int i = 0; i < nitems; ++i) {
            BmpsContractItem& f = ci[i]; f = BmpsContractItem{};
            f.nm = ngroup[3 * i]; f.nn = ngroup[3 * i + 1]; f.nk = ngroup[3 * i + 2]; f.conjB = conjB[i] ? 1 : 0;
            if (f.nm < 0 || f.nn < 0 || f.nk < 0 || f.nm > kBmpsMaxLegs || f.nn > kBmpsMaxLegs || f.nk > kBmpsMaxLegs) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_bmps_contract: 0 .. 4 legs per group");
            const int32_t* d = dims + 12 * i; const int64_t* st = strides + 24 * i;
            long long hiA = 0, hiB = 0, hiC = 0;      // the largest offset each array is addressed at
            auto leg = [&](int dim, long long s1, long long s2, long long& h1, long long& h2) {
                if (dim < 1 || s1 < 0 || s2 < 0) throw Err(TNQS_ERR_INVALID, "dbg_bmps_contract: bad dimension or stride");
                h1 += (long long)(dim - 1) * s1; h2 += (long long)(dim - 1) * s2;
            };
            for (int q = 0; q < f.nm; ++q) { f.md[q] = d[q]; f.ma[q] = st[q]; f.mc[q] = st[4 + q]; leg(d[q], st[q], st[4 + q], hiA, hiC); }
            for (int q = 0; q < f.nn; ++q) { f.nd[q] = d[4 + q]; f.nb[q] = st[8 + q]; f.nc[q] = st[12 + q]; leg(d[4 + q], st[8 + q], st[12 + q], hiB, hiC); }
            for (int q = 0; q < f.nk; ++q) { f.kd[q] = d[8 + q]; f.ka[q] = st[16 + q]; f.kb[q] = st[20 + q]; leg(d[8 + q], st[16 + q], st[20 + q], hiA, hiB); }
            const int64_t* z = sizes + 3 * i;
            if (z[0] < 1 || z[1] < 1 || z[2] < 1 || hiA >= z[0] || hiB >= z[1] || hiC >= z[2]) throw Err(TNQS_ERR_INVALID, "dbg_bmps_contract: an index falls outside its array");
            sA.add((size_t)z[0] * esz); sB.add((size_t)z[1] * esz); gC.add((size_t)z[2] * esz);
        }
        need_gpu();
        int wgs[2];
        plan_bmps_contract(ci.data(), nitems, esz, force_chunks, npart.data(), wgs);
        for (int i = 0; i < nitems; ++i) sP.add(npart[i] * esz);
        alloc_all(sA, sB, sP, gC);
        put_all(sA, A); put_all(sB, B);
        for (int i = 0; i < nitems; ++i) { ci[i].A = sA.at(i); ci[i].B = sB.at(i); ci[i].C = gC.at(i); ci[i].partial = npart[i] ? sP.at(i) : nullptr; }
        DevItems<BmpsContractItem> dC(ci);
        up_all(sA, sB, sP); gC.up(C);
        by_dtype(dtype, [&](auto t) {
            launch_bmps_contract<decltype(t)>(nullptr, dC.get(), nitems, wgs[0]);
            if (wgs[1]) launch_bmps_reduce<decltype(t)>(nullptr, dC.get(), nitems, wgs[1]);
        });
        HIPCHK(hipDeviceSynchronize());
        sP.down("the contraction partials"); gC.down(C, "C");
        if (nchunks_out) for (int i = 0; i < nitems; ++i) nchunks_out[i] = ci[i].nchunks;
    });
}

extern "C" int tnqs_dbg_bmps_qr(int dtype, int nitems, const int32_t* m, const int32_t* n, const int32_t* row_major, const void* A, void* Q, void* Y, int guard_elems) {
    return guard([&] {
        if (!is_dtype(dtype) || nitems < 1 || !m || !n || !row_major || !A || !Q || !Y || guard_elems < 0) throw Err(TNQS_ERR_INVALID, "dbg_bmps_qr: bad arguments");
        const size_t esz = esz_of(dtype);
        Slots sA, sW; Guarded gQ((size_t)guard_elems * esz), gY((size_t)guard_elems * esz);
        for (int i = 0; i < nitems; ++i) {
            if (m[i] < 1 || n[i] < 1) throw Err(TNQS_ERR_INVALID, "dbg_bmps_qr: bad shape");
            if (n[i] > kBmpsQrMaxCols || m[i] < n[i] || (long long)m[i] * n[i] > (1LL << 26)) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_bmps_qr: the QR kernel takes m >= n, n <= 64");
            const size_t mn = (size_t)m[i] * n[i];
            sA.add(mn * esz); sW.add(2 * mn * esz); gQ.add(mn * esz); gY.add((size_t)n[i] * n[i] * esz);
        }
        need_gpu();
        alloc_all(sA, sW, gQ, gY);
        put_all(sA, A);
        std::vector<BmpsQrItem> qi(nitems);
        for (int i = 0; i < nitems; ++i) {
            BmpsQrItem& f = qi[i]; f = BmpsQrItem{};
            f.A = sA.at(i); f.Q = gQ.at(i); f.Y = gY.at(i); f.W = sW.at(i); f.W2 = sW.at(i) + (size_t)m[i] * n[i] * esz; f.m = m[i]; f.n = n[i];
            if (row_major[i]) { f.ars = f.qrs = n[i]; f.acs = f.qcs = 1; } else { f.ars = f.qrs = 1; f.acs = f.qcs = m[i]; }
        }
        DevItems<BmpsQrItem> dQ(qi);
        up_all(sA, sW); gQ.up(Q); gY.up(Y);
        by_dtype(dtype, [&](auto t) { launch_bmps_qr<decltype(t)>(nullptr, dQ.get(), nitems); });
        HIPCHK(hipDeviceSynchronize());
        sW.down("the QR workspace"); gQ.down(Q, "Q"); gY.down(Y, "Y");
    });
}
