// debug_plane.cpp -- kernel-level test entry points (include/tnqs_debug.h) of the plane kernels: two legs per pass, pair product and pair-Gram at chi = 32
// (kernels_mfma.hip, kernels_x3.hip) and chi = 16 (kernels_plane.hip), and their timing entry point.
#include "debug_util.hpp"

using namespace tnqs;

extern "C" int tnqs_dbg_pair(int C0, int NMID, int NHI, const void* in, const void* Mx, const void* My, void* out) {
    return guard([&] {
        need_gpu();
        if (C0 % 16) throw Err(TNQS_ERR_INVALID, "dbg_pair: C0 % 16 != 0");
        size_t n = (size_t)C0 * 32 * NMID * 32 * NHI;
        DBuf dIn(n * 8), dOut(n * 8), dX(32 * 32 * 8), dY(32 * 32 * 8); DevItems<PairItem> dI(1);
        dIn.up(in, n * 8); dX.up(Mx, 32 * 32 * 8); dY.up(My, 32 * 32 * 8);
        HIPCHK(hipMemset(dOut.p, 0xff, n * 8));
        PairItem it{}; it.in = dIn.p; it.out = dOut.p; it.Mx = dX.p; it.My = dY.p;
        it.g.cstr = 2; it.g.sx = C0; it.g.sy = (long long)C0 * 32 * NMID; it.g.n0 = C0 / 16; it.g.t0 = 16; it.g.n1 = NMID; it.g.t1 = (long long)C0 * 32;
        it.g.n2 = NHI; it.g.t2 = (long long)C0 * 32 * NMID * 32;
        const int wgs = plan_pair(&it, 1, 3);
        dI.up(it);
        launch_mfma_pair(nullptr, dI.get(), 1, wgs);
        HIPCHK(hipDeviceSynchronize());
        dOut.down(out, n * 8);
    });
}
// pair product on the legs (lx, ly) of a site tensor [d][chi_0..chi_{z-1}] (ComplexF32): out = in x_lx Mx x_ly My
extern "C" int tnqs_dbg_pair_legs(int d, int z, const int* chi, int lx, int ly, const void* in, const void* Mx, const void* My, void* out) {
    return guard([&] {
        need_gpu();
        PairItem it{};
        if (!pair_geometry(d, z, chi, lx, ly, it.g)) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_pair_legs: shape not covered by the pair kernel");
        size_t n = d; for (int i = 0; i < z; ++i) n *= chi[i];
        DBuf dIn(n * 8), dOut(n * 8), dX(32 * 32 * 8), dY(32 * 32 * 8); DevItems<PairItem> dI(1);
        dIn.up(in, n * 8); dX.up(Mx, 32 * 32 * 8); dY.up(My, 32 * 32 * 8);
        HIPCHK(hipMemset(dOut.p, 0xff, n * 8));
        it.in = dIn.p; it.out = dOut.p; it.Mx = dX.p; it.My = dY.p;
        if ((size_t)it.g.n0 * it.g.n1 * it.g.n2 * 16 * 1024 != n) throw Err(TNQS_ERR_INVALID, "dbg_pair_legs: slice count");
        const int wgs = plan_pair(&it, 1, 3);
        dI.up(it);
        launch_mfma_pair(nullptr, dI.get(), 1, wgs);
        HIPCHK(hipDeviceSynchronize());
        dOut.down(out, n * 8);
    });
}
// out[b,b'] = sum (X x_lx M)[.., b, ..] conj(Y[.., b', ..]) with b on leg ly (ComplexF32, 32 x 32 output)
extern "C" int tnqs_dbg_pair_gram(int d, int z, const int* chi, int lx, int ly, const void* X, const void* Y, const void* M, void* out) {
    return guard([&] {
        need_gpu();
        PairGramItem it{};
        if (!pair_geometry(d, z, chi, lx, ly, it.g)) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_pair_gram: shape not covered by the pair kernel");
        size_t n = d; for (int i = 0; i < z; ++i) n *= chi[i];
        const bool x3 = mfma_use_x3();       // the engine's route: the bf16 kernel in its one-message form
        PairGram2Item one{}; one.g = it.g;
        const int nwg = x3 ? plan_x3_pair_gram1(&one, 1, nullptr, 3) : plan_pair_gram(&it, 1, nullptr, 3), npart = nwg;
        DBuf dX(n * 8), dY(n * 8), dM(32 * 32 * 8), dI(sizeof(PairGram2Item)); DevItems<ReduceItem> dR(1); DBuf dP((size_t)npart * 1024 * 8), dO(1024 * 8);
        dX.up(X, n * 8); dY.up(Y, n * 8); dM.up(M, 32 * 32 * 8);
        it.X = dX.p; it.Y = dY.p; it.M = dM.p; it.partial = dP.p;
        if (x3) {
            one.X = it.X; one.Y = it.Y; one.Mx = it.M; one.partial_y = it.partial;
            dI.up(&one, sizeof(one));
            launch_x3_pair_gram1(nullptr, (const PairGram2Item*)dI.p, 1, nwg);
        } else {
            dI.up(&it, sizeof(it));
            launch_mfma_pair_gram(nullptr, (const PairGramItem*)dI.p, 1, nwg);
        }
        dR.up(ReduceItem{dP.p, dO.p, 1024, npart, 0, 0});
        launch_reduce<float, float>(nullptr, dR.get(), 1, 1024);
        HIPCHK(hipDeviceSynchronize());
        dO.down(out, 1024 * 8);
    });
}
// both messages of a plane in one pass: out_y keeps leg ly (lx absorbed with Mx), out_x keeps leg lx (ly absorbed with My)
extern "C" int tnqs_dbg_pair_gram2(int d, int z, const int* chi, int lx, int ly, const void* X, const void* Y, const void* Mx, const void* My, void* out_y, void* out_x) {
    return guard([&] {
        need_gpu();
        PairGram2Item it{};
        if (!pair_geometry(d, z, chi, lx, ly, it.g)) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_pair_gram2: shape not covered");
        size_t n = d; for (int i = 0; i < z; ++i) n *= chi[i];
        const int nwg = plan_pair_gram2(&it, 1, nullptr, 3), npart = nwg;
        DBuf dX(n * 8), dY(n * 8), dMx(1024 * 8), dMy(1024 * 8); DevItems<PairGram2Item> dI(1); DevItems<ReduceItem> dR(2);
        DBuf dP1((size_t)npart * 1024 * 8), dP2((size_t)npart * 1024 * 8), dO(2 * 1024 * 8);
        dX.up(X, n * 8); dY.up(Y, n * 8); dMx.up(Mx, 1024 * 8); dMy.up(My, 1024 * 8);
        it.X = dX.p; it.Y = dY.p; it.Mx = dMx.p; it.My = dMy.p; it.partial_y = dP1.p; it.partial_x = dP2.p;
        dI.up(it);
        launch_mfma_pair_gram2(nullptr, dI.get(), 1, nwg);
        dR.up(std::vector<ReduceItem>{{dP1.p, dO.p, 1024, npart, 0, 0}, {dP2.p, (char*)dO.p + 1024 * 8, 1024, npart, 0, 1024}});
        launch_reduce<float, float>(nullptr, dR.get(), 2, 2048);
        HIPCHK(hipDeviceSynchronize());
        dO.down(out_y, 1024 * 8);
        HIPCHK(hipMemcpy(out_x, (char*)dO.p + 1024 * 8, 1024 * 8, hipMemcpyDeviceToHost));
    });
}

namespace {
// pseudo-random f32 fill in (-0.01, 0.01) for the timing entry points: constant data flatters the matrix kernels (fewer bits toggle, the chip clocks higher:
// the both-messages pair-Gram measured 1.0 ms per 100 sites on constant data and 1.29 in the benchmark)
void fill_random(void* d, size_t nfloats, unsigned seed) {
    const size_t blk = (size_t)1 << 22;                   // 4 Mi floats generated on the host, tiled over the buffer with a shifting offset
    std::vector<float> h(blk + 4096);
    unsigned x = seed * 2654435761u + 12345u;
    for (auto& v : h) { x = x * 1664525u + 1013904223u; v = ((int)(x >> 8) - (1 << 23)) * (0.01f / (1 << 23)); }
    size_t off = 0; unsigned k = 0;
    while (off < nfloats) {
        const size_t m = std::min(blk, nfloats - off);
        HIPCHK(hipMemcpy((char*)d + off * 4, h.data() + (k * 257u) % 4096u, m * 4, hipMemcpyHostToDevice));
        off += m; ++k;
    }
}
// one untimed launch, then the duration of `reps` launches between two HIP events (ms)
template <class F> float time_launches(hipEvent_t e0, hipEvent_t e1, int reps, F&& launch) {
    float t = 0.f;
    launch();
    HIPCHK(hipEventRecord(e0, nullptr));
    for (int r = 0; r < reps; ++r) launch();
    HIPCHK(hipEventRecord(e1, nullptr)); HIPCHK(hipEventSynchronize(e1)); HIPCHK(hipEventElapsedTime(&t, e0, e1));
    return t;
}
// which = 2 / 3: the chi = 16 plane kernels (mfma_pair16_kernel / mfma_pair_gram2x16_kernel, both messages) on degree-6 site tensors
void bench_plane16(int which, int nsites, int lx, int ly, int reps, double* ms) {
    const int chi[6] = {16, 16, 16, 16, 16, 16};
    PlaneGeom g{};
    if (!plane_geometry(2, 6, chi, lx, ly, 16, g)) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_bench_plane: legs not covered");
    const size_t n = (size_t)2 << 24;
    DBuf dA((size_t)nsites * n * 8), dB((size_t)nsites * n * 8), dM(2 * 256 * 8);
    fill_random(dA.p, (size_t)nsites * n * 2, 1); fill_random(dB.p, (size_t)nsites * n * 2, 2); fill_random(dM.p, 2 * 256 * 2, 3);
    hipEvent_t e0, e1; HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    float t = 0.f;
    if (which == 2) {
        std::vector<Pair16Item> items(nsites);
        for (int i = 0; i < nsites; ++i) {
            Pair16Item& it = items[i]; it.g = g; it.in = (char*)dA.p + (size_t)i * n * 8; it.out = (char*)dB.p + (size_t)i * n * 8;
            it.Mx = dM.p; it.My = (char*)dM.p + 256 * 8;
        }
        int w[2]; plan_pair16(items.data(), nsites, w);
        const int wgs = w[pair16_whole_lines(g) ? 1 : 0];
        DevItems<Pair16Item> dI(items);
        t = time_launches(e0, e1, reps, [&] { launch_mfma_pair16(nullptr, dI.get(), nsites, wgs, pair16_whole_lines(g)); });
    } else {
        std::vector<PairGram2x16Item> items(nsites);
        for (auto& it : items) it.g = g;
        const int wgs = plan_pair_gram2x16(items.data(), nsites), nwg = wgs / nsites;      // (identical items)
        DBuf dP((size_t)2 * nsites * nwg * 256 * 8);
        for (int i = 0; i < nsites; ++i) {
            PairGram2x16Item& it = items[i]; it.X = (char*)dA.p + (size_t)i * n * 8; it.Y = (char*)dB.p + (size_t)i * n * 8;
            it.Mx = dM.p; it.My = (char*)dM.p + 256 * 8;
            it.partial_y = (char*)dP.p + (size_t)(2 * i) * nwg * 256 * 8; it.partial_x = (char*)dP.p + (size_t)(2 * i + 1) * nwg * 256 * 8;
        }
        DevItems<PairGram2x16Item> dI(items);
        t = time_launches(e0, e1, reps, [&] { launch_mfma_pair_gram2x16(nullptr, dI.get(), nsites, wgs); });
    }
    HIPCHK(hipDeviceSynchronize());
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *ms = (double)t / reps;
}
}  // namespace
// timing of the chi = 32 plane kernels on `nsites` degree-4 site tensors [2][32]^4 resident in HBM (which: 0 pair product on legs (lx, ly),
// 1 both-messages pair-Gram, 4 one BP level of both); *ms = average launch duration over `reps` launches (HIP events), after one untimed launch
extern "C" int tnqs_dbg_bench_plane(int which, int nsites, int lx, int ly, int reps, double* ms) {
    return guard([&] {
        need_gpu();
        if (which == 2 || which == 3) { bench_plane16(which, nsites, lx, ly, reps, ms); return; }
        const int chi[4] = {32, 32, 32, 32};
        PairGeom g{};
        if (!pair_geometry(2, 4, chi, lx, ly, g)) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_bench_plane: legs not covered");
        const size_t n = (size_t)2 * 32 * 32 * 32 * 32;
        DBuf dA((size_t)nsites * n * 8), dB((size_t)nsites * n * 8), dM(2 * 1024 * 8);
        fill_random(dA.p, (size_t)nsites * n * 2, 1); fill_random(dB.p, (size_t)nsites * n * 2, 2); fill_random(dM.p, 2 * 1024 * 2, 3);
        hipEvent_t e0, e1; HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
        float t = 0.f;
        if (which == 4) {
            // one BP level of a degree-4 site: T = psi x_lx Mx x_ly My (pair product), then both messages through the other two legs from (T, psi).  The sites are
            // processed in groups of TNQS_DBG_GROUP (0: all at once, as the engine does): with a few sites per group T (16 MiB per site) is still in the 256 MiB
            // Infinity Cache when the pair-Gram reads it, and psi is read from memory once instead of twice
            const char* e = std::getenv("TNQS_DBG_GROUP"); int G = e ? std::atoi(e) : 0; if (G <= 0 || G > nsites) G = nsites;
            int ox = -1, oy = -1; for (int q = 0; q < 4; ++q) if (q != lx && q != ly) { if (ox < 0) ox = q; else oy = q; }
            PairGeom g2{}; if (!pair_geometry(2, 4, chi, ox, oy, g2)) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_bench_plane: other legs not covered");
            const int ngroups = (nsites + G - 1) / G;
            std::vector<PairItem> pit(nsites); std::vector<PairGram2Item> git(nsites);
            for (int i = 0; i < nsites; ++i) { pit[i].g = g; git[i].g = g2; }
            // the engine's layout of a group of G sites; the last group keeps the first one's spw
            std::vector<int> pw(ngroups), gwg(ngroups), nwg(nsites);
            for (int gr = 0; gr < ngroups; ++gr) {
                const int cnt = std::min(G, nsites - gr * G);
                pw[gr] = plan_pair(&pit[(size_t)gr * G], cnt, gr ? pit[0].spw : 0);
                gwg[gr] = plan_pair_gram2(&git[(size_t)gr * G], cnt, &nwg[(size_t)gr * G], gr ? git[0].spw : 0);
            }
            const int spw_p = pit[0].spw, spw_g = git[0].spw, nwg_g = nwg[0];
            DBuf dT((size_t)G * n * 8), dP((size_t)2 * nsites * nwg_g * 1024 * 8);
            for (int i = 0; i < nsites; ++i) {
                const int k = i % G;
                PairItem& a = pit[i]; a.in = (char*)dA.p + (size_t)i * n * 8; a.out = (char*)dT.p + (size_t)k * n * 8; a.Mx = dM.p; a.My = (char*)dM.p + 1024 * 8;
                PairGram2Item& b = git[i]; b.X = a.out; b.Y = a.in; b.Mx = dM.p; b.My = (char*)dM.p + 1024 * 8;
                b.partial_y = (char*)dP.p + (size_t)(2 * i) * nwg_g * 1024 * 8; b.partial_x = (char*)dP.p + (size_t)(2 * i + 1) * nwg_g * 1024 * 8;
            }
            DevItems<PairItem> dPI(pit); DevItems<PairGram2Item> dGI(git);
            t = time_launches(e0, e1, reps, [&] {
                for (int gr = 0; gr < ngroups; ++gr) {
                    const int cnt = std::min(G, nsites - gr * G);
                    launch_mfma_pair(nullptr, dPI.get() + (size_t)gr * G, cnt, pw[gr]);
                    launch_mfma_pair_gram2(nullptr, dGI.get() + (size_t)gr * G, cnt, gwg[gr]);
                }
            });
            std::fprintf(stderr, "level bench: group %d, pair spw %d, gram spw %d\n", G, spw_p, spw_g);
        } else if (which == 0) {
            std::vector<PairItem> items(nsites);
            for (int i = 0; i < nsites; ++i) {
                PairItem& it = items[i]; it.g = g; it.in = (char*)dA.p + (size_t)i * n * 8; it.out = (char*)dB.p + (size_t)i * n * 8;
                it.Mx = dM.p; it.My = (char*)dM.p + 1024 * 8;
            }
            const int wgs = plan_pair(items.data(), nsites);
            DevItems<PairItem> dI(items);
            t = time_launches(e0, e1, reps, [&] { launch_mfma_pair(nullptr, dI.get(), nsites, wgs); });
        } else {
            std::vector<PairGram2Item> items(nsites);
            for (auto& it : items) it.g = g;
            const int wgs = plan_pair_gram2(items.data(), nsites, nullptr, 16), nwg = wgs / nsites;      // (identical items)
            DBuf dP((size_t)2 * nsites * nwg * 1024 * 8);
            for (int i = 0; i < nsites; ++i) {
                PairGram2Item& it = items[i]; it.X = (char*)dA.p + (size_t)i * n * 8; it.Y = (char*)dB.p + (size_t)i * n * 8;
                it.Mx = dM.p; it.My = (char*)dM.p + 1024 * 8;
                it.partial_y = (char*)dP.p + (size_t)(2 * i) * nwg * 1024 * 8; it.partial_x = (char*)dP.p + (size_t)(2 * i + 1) * nwg * 1024 * 8;
            }
            DevItems<PairGram2Item> dI(items);
            t = time_launches(e0, e1, reps, [&] { launch_mfma_pair_gram2(nullptr, dI.get(), nsites, wgs); });
        }
        HIPCHK(hipDeviceSynchronize());
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        *ms = (double)t / reps;
    });
}

namespace {
// chi = 16 planes: item i is a site tensor [d][chi_0]..[chi_{z[i]-1}] (chi: the items' dimensions one after the other) with the plane (lx[i], ly[i])
void plane_items(int d, int nitems, const int* z, const int* chi, const int* lx, const int* ly, std::vector<PlaneGeom>& g, std::vector<size_t>& off) {
    if (nitems < 1 || !z || !chi || !lx || !ly || d < 1) throw Err(TNQS_ERR_INVALID, "dbg plane kernels: bad arguments");
    g.resize(nitems);
    int c = 0;
    cat_offsets(nitems, off, [&](int i) {
        if (z[i] < 2 || z[i] > 8) throw Err(TNQS_ERR_INVALID, "dbg plane kernels: 2 <= z <= 8");
        size_t n = d; for (int k = 0; k < z[i]; ++k) n *= chi[c + k];
        if (!plane_geometry(d, z[i], chi + c, lx[i], ly[i], 16, g[i]) || (size_t)g[i].nslices() * 16 * 256 != n)
            throw Err(TNQS_ERR_UNSUPPORTED, "dbg plane kernels: plane not covered by the chi = 16 kernels");
        c += z[i];
        return n;
    });
}
}  // namespace
// pair of mode products on two 16-dimensional legs (launch_mfma_pair16): out = in x_lx Mx x_ly My per item, M = (Mx, My) per item (2 x 256);
// the items of one launch are of one kind (pair16_whole_lines); spw <= 0: the engine's rule (run_chains)
extern "C" int tnqs_dbg_pair16(int d, int nitems, const int* z, const int* chi, const int* lx, const int* ly, const void* in, const void* M, void* out, int spw, int* route) {
    return guard([&] {
        need_gpu();
        std::vector<PlaneGeom> g; std::vector<size_t> off;
        plane_items(d, nitems, z, chi, lx, ly, g, off);
        const bool wl = pair16_whole_lines(g[0]);
        for (int i = 0; i < nitems; ++i) if (pair16_whole_lines(g[i]) != wl) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_pair16: one launch holds items of one kind");
        if (spw > 0 && spw % 4) throw Err(TNQS_ERR_INVALID, "dbg_pair16: spw must be a multiple of 4");
        const size_t n = off[nitems];
        DBuf dIn(n * 8), dOut(n * 8), dM((size_t)nitems * 512 * 8); DevItems<Pair16Item> dI(nitems);
        dIn.up(in, n * 8); dM.up(M, (size_t)nitems * 512 * 8);
        HIPCHK(hipMemset(dOut.p, 0xff, n * 8));
        std::vector<Pair16Item> items(nitems);
        for (int i = 0; i < nitems; ++i) {
            Pair16Item& it = items[i]; it.g = g[i]; it.in = (char*)dIn.p + off[i] * 8; it.out = (char*)dOut.p + off[i] * 8;
            it.Mx = (char*)dM.p + (size_t)i * 512 * 8; it.My = (char*)it.Mx + 256 * 8;
        }
        int wgs[2]; plan_pair16(items.data(), nitems, wgs, spw);
        dI.up(items);
        launch_mfma_pair16(nullptr, dI.get(), nitems, wgs[wl ? 1 : 0], wl);
        HIPCHK(hipDeviceSynchronize());
        dOut.down(out, n * 8);
        if (route) *route = wl ? TNQS_DBG_ROUTE_WHOLE_LINES : TNQS_DBG_ROUTE_HALF_LINES;
    });
}
// both messages of a 16 x 16 plane from one pass (launch_mfma_pair_gram2x16): per item out_y[i] (256 complex64) = sum (X x_lx Mx)[.. b on ly ..]
// conj(Y[.. b' on ly ..]), and when both[i] != 0 out_x[i] = sum (X x_ly My)[.. d on lx ..] conj(Y[.. d' on lx ..]); both[i] == 0 is the single-message
// form of the BP update (My = partial_x = null; out_x[i] is not written).  Partials of a message summed with launch_reduce; spw <= 0: the engine's rule
extern "C" int tnqs_dbg_pair_gram2x16(int d, int nitems, const int* z, const int* chi, const int* lx, const int* ly, const int* both, const void* X, const void* Y, const void* M,
                                      void* out_y, void* out_x, int spw) {
    return guard([&] {
        need_gpu();
        std::vector<PlaneGeom> g; std::vector<size_t> off;
        plane_items(d, nitems, z, chi, lx, ly, g, off);
        if (!both) throw Err(TNQS_ERR_INVALID, "dbg_pair_gram2x16: bad arguments");
        if (spw > 0 && spw % pair_gram2x16_slices_at_a_time()) throw Err(TNQS_ERR_INVALID, "dbg_pair_gram2x16: spw must be a multiple of the slices a workgroup walks at a time");
        const size_t n = off[nitems];
        std::vector<PairGram2x16Item> items(nitems); std::vector<int> nwg(nitems); for (int i = 0; i < nitems; ++i) items[i].g = g[i];
        const int wgs = plan_pair_gram2x16(items.data(), nitems, nwg.data(), spw);
        DBuf dX(n * 8), dY(n * 8), dM((size_t)nitems * 512 * 8); DevItems<PairGram2x16Item> dI(nitems); DBuf dP((size_t)2 * wgs * 256 * 8), dO((size_t)2 * nitems * 256 * 8);
        DevItems<ReduceItem> dR(2 * (size_t)nitems);
        dX.up(X, n * 8); dY.up(Y, n * 8); dM.up(M, (size_t)nitems * 512 * 8);
        HIPCHK(hipMemset(dO.p, 0, (size_t)2 * nitems * 256 * 8));
        std::vector<ReduceItem> ri;
        for (int i = 0; i < nitems; ++i) {
            PairGram2x16Item& it = items[i];
            it.X = (char*)dX.p + off[i] * 8; it.Y = (char*)dY.p + off[i] * 8;
            it.Mx = (char*)dM.p + (size_t)i * 512 * 8; it.My = both[i] ? (const void*)((char*)it.Mx + 256 * 8) : nullptr;
            it.partial_y = (char*)dP.p + (size_t)it.wg_begin * 256 * 8;
            it.partial_x = both[i] ? (void*)((char*)dP.p + ((size_t)wgs + it.wg_begin) * 256 * 8) : nullptr;
            ri.push_back(ReduceItem{it.partial_y, (char*)dO.p + (size_t)i * 256 * 8, 256, nwg[i], 0, (int)ri.size() * 256});
            if (both[i]) ri.push_back(ReduceItem{it.partial_x, (char*)dO.p + ((size_t)nitems + i) * 256 * 8, 256, nwg[i], 0, (int)ri.size() * 256});
        }
        dI.up(items); dR.up(ri);
        launch_mfma_pair_gram2x16(nullptr, dI.get(), nitems, wgs);
        launch_reduce<float, float>(nullptr, dR.get(), (int)ri.size(), (int)ri.size() * 256);
        HIPCHK(hipDeviceSynchronize());
        dO.down(out_y, (size_t)nitems * 256 * 8);
        if (out_x) for (int i = 0; i < nitems; ++i) if (both[i]) HIPCHK(hipMemcpy((char*)out_x + (size_t)i * 256 * 8, (char*)dO.p + ((size_t)nitems + i) * 256 * 8, 256 * 8, hipMemcpyDeviceToHost));
    });
}

namespace {
// chi = 32 planes: item i is a site tensor [d][chi_0]..[chi_{z[i]-1}] (chi: the items' dimensions one after the other) with the plane (lx[i], ly[i]); n[i] = its elements
void pair32_geoms(const char* who, int d, int nitems, const int* z, const int* chi, const int* lx, const int* ly, int spw, int guard_elems, std::vector<PairGeom>& g,
                  std::vector<size_t>& n) {
    if (nitems < 1 || !z || !chi || !lx || !ly || d < 1 || guard_elems < 0 || spw > (1 << 16)) throw Err(TNQS_ERR_INVALID, std::string(who) + ": bad arguments");
    g.resize(nitems); n.resize(nitems);
    int c = 0;
    for (int i = 0; i < nitems; ++i) {
        if (z[i] < 2 || z[i] > 8) throw Err(TNQS_ERR_INVALID, std::string(who) + ": 2 <= z <= 8");
        n[i] = d;
        for (int k = 0; k < z[i]; ++k) { if (chi[c + k] < 1 || chi[c + k] > 1024) throw Err(TNQS_ERR_INVALID, std::string(who) + ": 1 <= chi <= 1024"); n[i] *= chi[c + k]; }
        if (!pair_geometry(d, z[i], chi + c, lx[i], ly[i], g[i]) || (size_t)g[i].n0 * g[i].n1 * g[i].n2 * 16 * 1024 != n[i])
            throw Err(TNQS_ERR_UNSUPPORTED, std::string(who) + ": shape not covered by the chi = 32 plane kernels");
        c += z[i];
    }
}
// what a plan_* function decided, for the caller: the launch's spw, every item's first workgroup and workgroups, the total
template <class Item> void plan_report(const std::vector<Item>& items, int Item::*begin, int total, int* spw_out, int* wg_begin_out, int* nwg_out, int* total_wgs_out) {
    const int n = (int)items.size();
    if (spw_out) *spw_out = items[0].spw;
    for (int i = 0; i < n; ++i) {
        if (wg_begin_out) wg_begin_out[i] = items[i].*begin;
        if (nwg_out) nwg_out[i] = (i + 1 < n ? items[i + 1].*begin : total) - items[i].*begin;
    }
    if (total_wgs_out) *total_wgs_out = total;
}
}  // namespace
// ONE launch_mfma_pair over nitems items planned by plan_pair (x3_pair_kernel, mfma_pair_kernel under TNQS_NO_BF16X3=1): out_i = in_i x_lx Mx_i x_ly My_i
extern "C" int tnqs_dbg_pair32(int d, int nitems, const int* z, const int* chi, const int* lx, const int* ly, const void* in, const void* M, void* out, int spw, int guard_elems,
                               int* route, int* spw_out, int* wg_begin_out, int* nwg_out, int* total_wgs_out) {
    return guard([&] {
        std::vector<PairGeom> g; std::vector<size_t> n;
        pair32_geoms("dbg_pair32", d, nitems, z, chi, lx, ly, spw, guard_elems, g, n);
        if (in && (!M || !out)) throw Err(TNQS_ERR_INVALID, "dbg_pair32: bad arguments");
        std::vector<PairItem> items(nitems);
        for (int i = 0; i < nitems; ++i) { items[i] = PairItem{}; items[i].g = g[i]; }
        const int wgs = plan_pair(items.data(), nitems, spw);
        plan_report(items, &PairItem::slice_begin, wgs, spw_out, wg_begin_out, nwg_out, total_wgs_out);
        if (route) *route = mfma_use_x3() ? TNQS_DBG_ROUTE_X3 : TNQS_DBG_ROUTE_F32;
        if (!in) return;
        need_gpu();
        Slots sIn, sM; Guarded gO((size_t)guard_elems * 8);
        for (int i = 0; i < nitems; ++i) { sIn.add(n[i] * 8); sM.add(2 * 1024 * 8); gO.add(n[i] * 8); }
        alloc_all(sIn, sM, gO); put_all(sIn, in); put_all(sM, M);
        for (int i = 0; i < nitems; ++i) { PairItem& it = items[i]; it.in = sIn.at(i); it.out = gO.at(i); it.Mx = sM.at(i); it.My = sM.at(i) + 1024 * 8; }
        DevItems<PairItem> dI(items);
        up_all(sIn, sM); gO.up(out);
        launch_mfma_pair(nullptr, dI.get(), nitems, wgs);
        HIPCHK(hipDeviceSynchronize());
        gO.down(out, "out");
    });
}
// ONE pair-Gram launch of one form over nitems items, then launch_reduce over every item's partials.  form 0: both messages (plan_pair_gram2, launch_mfma_pair_gram2);
// form 1: one message, on the route launch_plane_grams takes (plan_x3_pair_gram1 / launch_x3_pair_gram1, under TNQS_NO_BF16X3=1 plan_pair_gram / launch_mfma_pair_gram)
extern "C" int tnqs_dbg_pair_gram32(int d, int nitems, const int* z, const int* chi, const int* lx, const int* ly, int form, const void* X, const void* Y, const void* M,
                                    void* out_y, void* out_x, int spw, int guard_elems, int* route, int* spw_out, int* wg_begin_out, int* nwg_out, int* total_wgs_out) {
    return guard([&] {
        std::vector<PairGeom> g; std::vector<size_t> n;
        pair32_geoms("dbg_pair_gram32", d, nitems, z, chi, lx, ly, spw, guard_elems, g, n);
        if ((form != 0 && form != 1) || (X && (!Y || !M || !out_y || (form == 0 && !out_x)))) throw Err(TNQS_ERR_INVALID, "dbg_pair_gram32: bad arguments");
        const bool x3 = mfma_use_x3(), f32_single = form == 1 && !x3;
        std::vector<PairGram2Item> two(nitems); std::vector<PairGramItem> one(f32_single ? nitems : 0);      // one: the items of mfma_pair_gram_kernel
        std::vector<int> nwg(nitems); int wgs = 0;
        for (int i = 0; i < nitems; ++i) { two[i] = PairGram2Item{}; two[i].g = g[i]; if (f32_single) { one[i] = PairGramItem{}; one[i].g = g[i]; } }
        if (form == 0) wgs = plan_pair_gram2(two.data(), nitems, nwg.data(), spw);
        else if (x3) wgs = plan_x3_pair_gram1(two.data(), nitems, nwg.data(), spw);
        else wgs = plan_pair_gram(one.data(), nitems, nwg.data(), spw);
        if (f32_single) plan_report(one, &PairGramItem::wg_begin, wgs, spw_out, wg_begin_out, nwg_out, total_wgs_out);
        else plan_report(two, &PairGram2Item::wg_begin, wgs, spw_out, wg_begin_out, nwg_out, total_wgs_out);
        if (route) *route = x3 ? TNQS_DBG_ROUTE_X3 : TNQS_DBG_ROUTE_F32;
        if (!X) return;
        need_gpu();
        const size_t band = 256, pb = 1024 * 8;        // guard band behind every partial array (and in front of the first), 0xff like the partials themselves
        const int nmsg = form == 0 ? 2 : 1;
        Slots sX, sY, sM, sP(band); Guarded gOy((size_t)guard_elems * 8), gOx((size_t)guard_elems * 8);
        for (int i = 0; i < nitems; ++i) {
            sX.add(n[i] * 8); sY.add(n[i] * 8); sM.add(2 * pb); gOy.add(pb); gOx.add(pb);
            for (int m = 0; m < nmsg; ++m) sP.add((size_t)nwg[i] * pb);
        }
        alloc_all(sX, sY, sM, sP, gOy); put_all(sX, X); put_all(sY, Y); put_all(sM, M);
        if (form == 0) gOx.alloc();
        std::vector<ReduceItem> ri;
        for (int i = 0; i < nitems; ++i) {
            void* py = sP.at((size_t)nmsg * i); void* px = form == 0 ? sP.at((size_t)nmsg * i + 1) : nullptr;
            if (f32_single) { PairGramItem& it = one[i]; it.X = sX.at(i); it.Y = sY.at(i); it.M = sM.at(i); it.partial = py; }
            else { PairGram2Item& it = two[i]; it.X = sX.at(i); it.Y = sY.at(i); it.Mx = sM.at(i); it.My = form == 0 ? sM.at(i) + pb : nullptr; it.partial_y = py; it.partial_x = px; }
            ri.push_back(ReduceItem{py, gOy.at(i), 1024, nwg[i], 0, (int)ri.size() * 1024});
            if (form == 0) ri.push_back(ReduceItem{px, gOx.at(i), 1024, nwg[i], 0, (int)ri.size() * 1024});
        }
        DevItems<PairGram2Item> dTwo(two); DevItems<PairGramItem> dOne(one); DevItems<ReduceItem> dR(ri);
        up_all(sX, sY, sM, sP); gOy.up(out_y); if (form == 0) gOx.up(out_x);
        if (form == 0) launch_mfma_pair_gram2(nullptr, dTwo.get(), nitems, wgs);
        else if (x3) launch_x3_pair_gram1(nullptr, dTwo.get(), nitems, wgs);
        else launch_mfma_pair_gram(nullptr, dOne.get(), nitems, wgs);
        launch_reduce<float, float>(nullptr, dR.get(), (int)ri.size(), (int)ri.size() * 1024);
        HIPCHK(hipDeviceSynchronize());
        sP.down("the pair-Gram partials");
        auto untouched = [&](size_t b0, size_t b1) { for (size_t b = b0; b < b1; ++b) if (sP.host[b] != (char)0xff) throw Err(TNQS_ERR_INVALID, "dbg: a kernel wrote outside an item of the pair-Gram partials"); };
        untouched(0, band);
        for (size_t k = 0; k < sP.off.size(); ++k) untouched(sP.off[k] + sP.len[k], sP.off[k] + sP.len[k] + band);
        gOy.down(out_y, "out_y"); if (form == 0) gOx.down(out_x, "out_x");
    });
}
