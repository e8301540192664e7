// debug.cpp -- kernel-level test entry points (include/tnqs_debug.h): host arrays in, host arrays out.
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <vector>
#include <algorithm>
#include <memory>
#include <string>
#include "engine.hpp"
#include "engine_internal.hpp"
#include "kernels.hpp"
#include "launch_util.hpp"
#include "../../include/tnqs_debug.h"

namespace tnqs {
struct DBuf { void* p = nullptr; explicit DBuf(size_t n) { HIPCHK(hipMalloc(&p, n ? n : 1)); } ~DBuf() { (void)hipFree(p); }
              void up(const void* h, size_t n) { if (n) HIPCHK(hipMemcpy(p, h, n, hipMemcpyHostToDevice)); } void down(void* h, size_t n) { if (n) HIPCHK(hipMemcpy(h, p, n, hipMemcpyDeviceToHost)); } };
static void need_gpu() { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) throw Err(TNQS_ERR_HIP, "no HIP device available"); }

void dbg_jacobi(int dtype, int m, int n, void* A, void* V, int* sweeps) {
    need_gpu();
    if (m < 1 || n < 1 || m > 256 || n > 256) throw Err(TNQS_ERR_INVALID, "dbg_jacobi: 1 <= m, n <= 256");
    size_t esz = dtype == TNQS_C64 ? 8 : 16;
    DBuf dA((size_t)m * n * esz), dV((size_t)n * n * esz), dS(4), dI(sizeof(JacobiItem));
    dA.up(A, (size_t)m * n * esz);
    if (dtype == TNQS_C64) launch_identity<float>(nullptr, dV.p, n); else launch_identity<double>(nullptr, dV.p, n);
    // same residency policy as the engine: A+V in LDS, else A in LDS with V recovered, else global memory
    const size_t lim = 160 * 1024 - 2048;
    size_t lds_av = jacobi_lds_bytes(m, n, true, esz), lds_a = jacobi_lds_bytes(m, n, false, esz);
    const char* fg = std::getenv("TNQS_DBG_NOV_GLOBAL");      // the engine's combination for matrices beyond the LDS: global-memory kernel, V recovered
    const bool force_global_nov = fg && fg[0] == '1';
    const char* ft = std::getenv("TNQS_DBG_THETA_SVD");       // the engine's theta route: A only in LDS, V recovered from the unrotated copy
    const bool theta_route = ft && ft[0] == '1' && dtype == TNQS_C64 && lds_a <= lim;
    const bool nov = force_global_nov || theta_route || (lds_av > lim && lds_a <= lim);
    DBuf dA0((size_t)m * n * esz);
    if (nov) dA0.up(A, (size_t)m * n * esz);
    JacobiItem it{dA.p, nov ? nullptr : dV.p, m, n, (int*)dS.p};
    dI.up(&it, sizeof(it));
    size_t lds = force_global_nov ? 0 : (nov ? lds_a : (lds_av <= lim ? lds_av : 0));
    if (dtype == TNQS_C64) launch_jacobi<float>(nullptr, (const JacobiItem*)dI.p, 1, 60, lds, std::max(m, n)); else launch_jacobi<double>(nullptr, (const JacobiItem*)dI.p, 1, 60, lds, std::max(m, n));
    if (nov) {
        DBuf dRv(sizeof(RecoverItem)); RecoverItem rv{dA0.p, dA.p, dV.p, m, n, n}; dRv.up(&rv, sizeof(rv));
        if (dtype == TNQS_C64) launch_recover_v_mfma(nullptr, (const RecoverItem*)dRv.p, 1, n); else launch_recover_v<double>(nullptr, (const RecoverItem*)dRv.p, 1, n);
        HIPCHK(hipDeviceSynchronize());
    }
    HIPCHK(hipDeviceSynchronize());
    dA.down(A, (size_t)m * n * esz); dV.down(V, (size_t)n * n * esz);
    if (sweeps) dS.down(sweeps, 4);
}

// theta_svd_pre_kernel on one ComplexF32 factor A (m x n) of theta = A Q^T, Q (nq x n, complex128, orthonormal columns): A := U Sigma, V (nq x n) := conj(Q) U_L.
// reps > 0: additionally time `reps` launches on `copies` device-resident copies of A (one workgroup each) with HIP events -> *ms = average per launch
void dbg_theta_svd_pre(int m, int n, int nq, void* A, const void* Q, void* V, int* sweeps, int copies, int reps, double* ms, double* phase_us, int cap) {
    need_gpu();
    if (!Q) nq = n;                                 // no Q: theta itself is factorised, V is n x n
    if (!theta_svd_pre_covers(m, n) || nq < n || nq > m) throw Err(TNQS_ERR_INVALID, "dbg_theta_svd_pre: 2 <= n <= 64, n <= nq <= m <= 128");
    if (copies < 1) copies = 1;
    const size_t ab = (size_t)m * n * 8, vb = (size_t)nq * n * 8;
    DBuf dA(ab * copies), dA0(ab), dQ((size_t)nq * n * 16), dV(vb * copies), dS(4 * (size_t)copies), dInfo(32), dI(sizeof(JacobiItem) * (size_t)copies), dT(64);
    dA0.up(A, ab); if (Q) dQ.up(Q, (size_t)nq * n * 16);
    const int info[8] = {m, nq, 0, 0, 0, 0, 0, Q ? n : 0};      // theta_dims with d1 = d2 = 1: m rows, nq columns of theta, n columns of the factor (0: theta itself)
    dInfo.up(info, 32);
    std::vector<JacobiItem> its(copies);
    for (int c = 0; c < copies; ++c) {
        JacobiItem it{}; it.A = (char*)dA.p + ab * c; it.V = (c == 0 && phase_us) ? dT.p : nullptr; it.m = m; it.n = nq; it.sweeps_out = (int*)dS.p + c; it.dyn = (const int*)dInfo.p; it.dm = 1; it.dn = 1; it.nhint = n;
        it.QB = Q ? dQ.p : nullptr; it.Vout = (char*)dV.p + vb * c; it.pre = 0 /* the dimensions given decide, whatever the size */; it.cap = cap; its[c] = it;
    }
    dI.up(its.data(), sizeof(JacobiItem) * (size_t)copies);
    auto reset = [&]() { for (int c = 0; c < copies; ++c) HIPCHK(hipMemcpyAsync((char*)dA.p + ab * c, dA0.p, ab, hipMemcpyDeviceToDevice, nullptr)); };
    reset();
    launch_theta_svd_pre(nullptr, (const JacobiItem*)dI.p, copies, 60, m, n);
    HIPCHK(hipDeviceSynchronize());
    dA.down(A, ab); dV.down(V, vb);
    if (sweeps) dS.down(sweeps, 4);
    if (phase_us) {      // constant-rate clock (100 MHz) at the seven phase boundaries of workgroup 0 -> six durations in us
        unsigned long long t[8]; dT.down(t, 64);
        for (int k = 0; k < 6; ++k) phase_us[k] = (double)(t[k + 1] - t[k]) * 0.01;
    }
    if (reps > 0 && ms) {
        hipEvent_t e0, e1; HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
        double tot = 0;
        for (int r = 0; r < reps; ++r) {
            reset();
            HIPCHK(hipEventRecord(e0, nullptr));
            launch_theta_svd_pre(nullptr, (const JacobiItem*)dI.p, copies, 60, m, n);
            HIPCHK(hipEventRecord(e1, nullptr)); HIPCHK(hipEventSynchronize(e1));
            float t = 0; HIPCHK(hipEventElapsedTime(&t, e0, e1)); tot += t;
        }
        *ms = tot / reps;
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    }
}
// the plain LDS-resident Jacobi on the same factor, timed the same way (what the preconditioned kernel replaces)
void dbg_time_jacobi_f32(int m, int n, const void* A, int copies, int reps, double* ms, int* sweeps) {
    need_gpu();
    if (copies < 1) copies = 1;
    const size_t ab = (size_t)m * n * 8;
    DBuf dA(ab * copies), dA0(ab), dS(4 * (size_t)copies), dI(sizeof(JacobiItem) * (size_t)copies);
    dA0.up(A, ab);
    std::vector<JacobiItem> its(copies);
    for (int c = 0; c < copies; ++c) { JacobiItem it{}; it.A = (char*)dA.p + ab * c; it.m = m; it.n = n; it.sweeps_out = (int*)dS.p + c; its[c] = it; }
    dI.up(its.data(), sizeof(JacobiItem) * (size_t)copies);
    hipEvent_t e0, e1; HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    double tot = 0;
    for (int r = 0; r < reps + 1; ++r) {
        for (int c = 0; c < copies; ++c) HIPCHK(hipMemcpyAsync((char*)dA.p + ab * c, dA0.p, ab, hipMemcpyDeviceToDevice, nullptr));
        HIPCHK(hipEventRecord(e0, nullptr));
        launch_jacobi<float>(nullptr, (const JacobiItem*)dI.p, copies, 60, jacobi_lds_bytes(m, n, false, 8), std::max(m, n), n);
        HIPCHK(hipEventRecord(e1, nullptr)); HIPCHK(hipEventSynchronize(e1));
        float t = 0; HIPCHK(hipEventElapsedTime(&t, e0, e1)); if (r > 0) tot += t;
    }
    if (ms) *ms = tot / std::max(1, reps);
    if (sweeps) dS.down(sweeps, 4);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
}

// Cholesky kernels on one Hermitian n x n complex128 matrix: L (lower), W = (L^-1)^dagger, *fail; n <= 96: chol_kernel, else packed
void dbg_chol(int n, const void* G, void* Lout, void* Wout, int* fail, double tau) {
    need_gpu();
    if (n < 1 || n > 128) throw Err(TNQS_ERR_INVALID, "dbg_chol: 1 <= n <= 128");
    const size_t b = (size_t)n * n * 16;
    DBuf dG(b), dL(b), dW(b), dF(4), dI(sizeof(CholItem));
    dG.up(G, b); HIPCHK(hipMemset(dF.p, 0, 4)); HIPCHK(hipMemset(dW.p, 0, b));
    CholItem it{dG.p, dL.p, dW.p, n, (int*)dF.p, tau, 0.0};
    dI.up(&it, sizeof(it));
    if (n <= 96) launch_chol(nullptr, (const CholItem*)dI.p, 1, n); else launch_chol_packed(nullptr, (const CholItem*)dI.p, 1, n);
    HIPCHK(hipDeviceSynchronize());
    dL.down(Lout, b); dW.down(Wout, b); dF.down(fail, 4);
}

void dbg_fiber_gemm(int dtype, int D, int PA, int K, int PB, int Do, int No, const void* in, const void* X, void* out, double* norm2, int use_mfma) {
    need_gpu();
    size_t esz = dtype == TNQS_C64 ? 8 : 16;
    size_t nin = (size_t)D * PA * K * PB, nout = (size_t)Do * PA * No * PB, nx = (size_t)D * K * Do * No;
    DBuf dIn(nin * esz), dX(nx * esz), dOut(nout * esz), dI(sizeof(FiberItem));
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
    dI.up(L.items.data(), sizeof(FiberItem));
    if (dtype == TNQS_C64) launch_fiber_route<float>(nullptr, L, (const FiberItem*)dI.p, (double*)dN.p);
    else launch_fiber_route<double>(nullptr, L, (const FiberItem*)dI.p, (double*)dN.p);
    HIPCHK(hipDeviceSynchronize());
    dOut.down(out, nout * esz);
    if (norm2) { std::vector<double> np(tiles); dN.down(np.data(), (size_t)tiles * 8); double t = 0; for (double v : np) t += v; *norm2 = t; }
}

void dbg_gram(int dtype, int D, int PA, int K, int PB, const void* X, const void* Y, void* out, int acc64, int use_mfma) {
    need_gpu();
    size_t esz = dtype == TNQS_C64 ? 8 : 16;
    size_t nin = (size_t)D * PA * K * PB; int KK = D * K;
    bool same = (X == Y);
    DBuf dX(nin * esz), dY(same ? 1 : nin * esz), dI(sizeof(GramItem)), dR(sizeof(ReduceItem));
    dX.up(X, nin * esz); if (!same) dY.up(Y, nin * esz);
    GramItem it{}; it.X = dX.p; it.Y = same ? dX.p : dY.p; it.D = D; it.PA = PA; it.K = K; it.PB = PB;
    const bool mf = use_mfma && dtype == TNQS_C64 && !acc64 && KK <= 32;
    const bool mf64 = use_mfma && dtype == TNQS_C64 && acc64 && same && KK <= 64 && KK >= 16;
    const bool mfz = use_mfma && dtype == TNQS_C128 && gram_f64in_covers(D, K);           // kernels_f64.hip
    const GramRoute r = mfz ? GramRoute::F64In : mf64 ? GramRoute::F64x64 : mf ? GramRoute::Mfma32 : GramRoute::Generic;
    const int TR = gram_tile_rows(r, KK, esz);
    tile_params(PA, PB, TR, it.TA, it.TB, it.nta, it.ntb);
    const char* e = std::getenv("TNQS_DBG_GRAM_CHUNKS");
    int npart = 0; plan_gram(&it, 1, r, false, e ? std::max(1, std::atoi(e)) : 7, &npart);
    bool a64 = acc64 || dtype == TNQS_C128;
    size_t asz = a64 ? 16 : 8;
    DBuf dP((size_t)npart * KK * KK * asz), dO((size_t)KK * KK * asz);
    it.partial = dP.p; dI.up(&it, sizeof(it));
    const GramItem* d = (const GramItem*)dI.p;
    if (dtype == TNQS_C128) launch_gram_route<double, double>(nullptr, r, d, 1, it.nchunks, TR, KK, KK == 64);
    else if (a64) launch_gram_route<float, double>(nullptr, r, d, 1, it.nchunks, TR, KK, KK == 64);
    else launch_gram_route<float, float>(nullptr, r, d, 1, it.nchunks, TR, KK);
    ReduceItem ri{dP.p, dO.p, KK * KK, npart, 0, 0}; dR.up(&ri, sizeof(ri));
    if (a64) launch_reduce<double, double>(nullptr, (const ReduceItem*)dR.p, 1, KK * KK); else launch_reduce<float, float>(nullptr, (const ReduceItem*)dR.p, 1, KK * KK);
    HIPCHK(hipDeviceSynchronize());
    dO.down(out, (size_t)KK * KK * asz);
}
void dbg_pair(int C0, int NMID, int NHI, const void* in, const void* Mx, const void* My, void* out) {
    need_gpu();
    if (C0 % 16) throw Err(TNQS_ERR_INVALID, "dbg_pair: C0 % 16 != 0");
    size_t n = (size_t)C0 * 32 * NMID * 32 * NHI;
    DBuf dIn(n * 8), dOut(n * 8), dX(32 * 32 * 8), dY(32 * 32 * 8), dI(sizeof(PairItem));
    dIn.up(in, n * 8); dX.up(Mx, 32 * 32 * 8); dY.up(My, 32 * 32 * 8);
    HIPCHK(hipMemset(dOut.p, 0xff, n * 8));
    PairItem it{}; it.in = dIn.p; it.out = dOut.p; it.Mx = dX.p; it.My = dY.p;
    it.g.cstr = 2; it.g.sx = C0; it.g.sy = (long long)C0 * 32 * NMID; it.g.n0 = C0 / 16; it.g.t0 = 16; it.g.n1 = NMID; it.g.t1 = (long long)C0 * 32;
    it.g.n2 = NHI; it.g.t2 = (long long)C0 * 32 * NMID * 32;
    const int wgs = plan_pair(&it, 1, 3);
    dI.up(&it, sizeof(it));
    launch_mfma_pair(nullptr, (const PairItem*)dI.p, 1, wgs);
    HIPCHK(hipDeviceSynchronize());
    dOut.down(out, n * 8);
}
// pair product on the legs (lx, ly) of a site tensor [d][chi_0..chi_{z-1}] (ComplexF32): out = in x_lx Mx x_ly My
void dbg_pair_legs(int d, int z, const int* chi, int lx, int ly, const void* in, const void* Mx, const void* My, void* out) {
    need_gpu();
    PairItem it{};
    if (!pair_geometry(d, z, chi, lx, ly, it.g)) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_pair_legs: shape not covered by the pair kernel");
    size_t n = d; for (int i = 0; i < z; ++i) n *= chi[i];
    DBuf dIn(n * 8), dOut(n * 8), dX(32 * 32 * 8), dY(32 * 32 * 8), dI(sizeof(PairItem));
    dIn.up(in, n * 8); dX.up(Mx, 32 * 32 * 8); dY.up(My, 32 * 32 * 8);
    HIPCHK(hipMemset(dOut.p, 0xff, n * 8));
    it.in = dIn.p; it.out = dOut.p; it.Mx = dX.p; it.My = dY.p;
    if ((size_t)it.g.n0 * it.g.n1 * it.g.n2 * 16 * 1024 != n) throw Err(TNQS_ERR_INVALID, "dbg_pair_legs: slice count");
    const int wgs = plan_pair(&it, 1, 3);
    dI.up(&it, sizeof(it));
    launch_mfma_pair(nullptr, (const PairItem*)dI.p, 1, wgs);
    HIPCHK(hipDeviceSynchronize());
    dOut.down(out, n * 8);
}
// out[b,b'] = sum (X x_lx M)[.., b, ..] conj(Y[.., b', ..]) with b on leg ly (ComplexF32, 32 x 32 output)
void dbg_pair_gram(int d, int z, const int* chi, int lx, int ly, const void* X, const void* Y, const void* M, void* out) {
    need_gpu();
    PairGramItem it{};
    if (!pair_geometry(d, z, chi, lx, ly, it.g)) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_pair_gram: shape not covered by the pair kernel");
    size_t n = d; for (int i = 0; i < z; ++i) n *= chi[i];
    const bool x3 = mfma_use_x3();       // the engine's route: the bf16 kernel in its one-message form
    PairGram2Item one{}; one.g = it.g;
    const int nwg = x3 ? plan_x3_pair_gram1(&one, 1, nullptr, 3) : plan_pair_gram(&it, 1, nullptr, 3), npart = nwg;
    DBuf dX(n * 8), dY(n * 8), dM(32 * 32 * 8), dI(sizeof(PairGram2Item)), dR(sizeof(ReduceItem)), dP((size_t)npart * 1024 * 8), dO(1024 * 8);
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
    ReduceItem ri{dP.p, dO.p, 1024, npart, 0, 0}; dR.up(&ri, sizeof(ri));
    launch_reduce<float, float>(nullptr, (const ReduceItem*)dR.p, 1, 1024);
    HIPCHK(hipDeviceSynchronize());
    dO.down(out, 1024 * 8);
}
// psi' = psi x_(s,b) X for d = 2, chi_b = chi_b' = 32 through the plane kernel; returns |psi'|^2 in *norm2
// both messages of a plane in one pass: out_y keeps leg ly (lx absorbed with Mx), out_x keeps leg lx (ly absorbed with My)
void dbg_pair_gram2(int d, int z, const int* chi, int lx, int ly, const void* X, const void* Y, const void* Mx, const void* My, void* out_y, void* out_x) {
    need_gpu();
    PairGram2Item it{};
    if (!pair_geometry(d, z, chi, lx, ly, it.g)) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_pair_gram2: shape not covered");
    size_t n = d; for (int i = 0; i < z; ++i) n *= chi[i];
    const int nwg = plan_pair_gram2(&it, 1, nullptr, 3), npart = nwg;
    DBuf dX(n * 8), dY(n * 8), dMx(1024 * 8), dMy(1024 * 8), dI(sizeof(PairGram2Item)), dR(2 * sizeof(ReduceItem)), dP1((size_t)npart * 1024 * 8), dP2((size_t)npart * 1024 * 8), dO(2 * 1024 * 8);
    dX.up(X, n * 8); dY.up(Y, n * 8); dMx.up(Mx, 1024 * 8); dMy.up(My, 1024 * 8);
    it.X = dX.p; it.Y = dY.p; it.Mx = dMx.p; it.My = dMy.p; it.partial_y = dP1.p; it.partial_x = dP2.p;
    dI.up(&it, sizeof(it));
    launch_mfma_pair_gram2(nullptr, (const PairGram2Item*)dI.p, 1, nwg);
    ReduceItem ri[2] = {{dP1.p, dO.p, 1024, npart, 0, 0}, {dP2.p, (char*)dO.p + 1024 * 8, 1024, npart, 0, 1024}};
    dR.up(ri, sizeof(ri));
    launch_reduce<float, float>(nullptr, (const ReduceItem*)dR.p, 2, 2048);
    HIPCHK(hipDeviceSynchronize());
    dO.down(out_y, 1024 * 8);
    HIPCHK(hipMemcpy(out_x, (char*)dO.p + 1024 * 8, 1024 * 8, hipMemcpyDeviceToHost));
}
// pseudo-random f32 fill in (-0.01, 0.01) for the timing entry points: constant data flatters the matrix kernels (fewer bits toggle, the chip clocks higher:
// the both-messages pair-Gram measured 1.0 ms per 100 sites on constant data and 1.29 in the benchmark)
static void fill_random(void* d, size_t nfloats, unsigned seed) {
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
// timing of the chi = 32 plane kernels on `nsites` degree-4 site tensors [2][32]^4 resident in HBM (which: 0 pair product on legs (lx, ly),
// 1 both-messages pair-Gram); *ms = average launch duration over `reps` launches (HIP events), after one untimed launch
// which = 2 / 3: the chi = 16 plane kernels (mfma_pair16_kernel / mfma_pair_gram2x16_kernel, both messages) on degree-6 site tensors
static void dbg_bench_plane16(int which, int nsites, int lx, int ly, int reps, double* ms) {
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
        DBuf dI(items.size() * sizeof(Pair16Item)); dI.up(items.data(), items.size() * sizeof(Pair16Item));
        launch_mfma_pair16(nullptr, (const Pair16Item*)dI.p, nsites, wgs, pair16_whole_lines(g));
        HIPCHK(hipEventRecord(e0, nullptr));
        for (int r = 0; r < reps; ++r) launch_mfma_pair16(nullptr, (const Pair16Item*)dI.p, nsites, wgs, pair16_whole_lines(g));
        HIPCHK(hipEventRecord(e1, nullptr)); HIPCHK(hipEventSynchronize(e1)); HIPCHK(hipEventElapsedTime(&t, e0, e1));
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
        DBuf dI(items.size() * sizeof(PairGram2x16Item)); dI.up(items.data(), items.size() * sizeof(PairGram2x16Item));
        launch_mfma_pair_gram2x16(nullptr, (const PairGram2x16Item*)dI.p, nsites, wgs);
        HIPCHK(hipEventRecord(e0, nullptr));
        for (int r = 0; r < reps; ++r) launch_mfma_pair_gram2x16(nullptr, (const PairGram2x16Item*)dI.p, nsites, wgs);
        HIPCHK(hipEventRecord(e1, nullptr)); HIPCHK(hipEventSynchronize(e1)); HIPCHK(hipEventElapsedTime(&t, e0, e1));
    }
    HIPCHK(hipDeviceSynchronize());
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *ms = (double)t / reps;
}
void dbg_bench_plane(int which, int nsites, int lx, int ly, int reps, double* ms) {
    need_gpu();
    if (which == 2 || which == 3) { dbg_bench_plane16(which, nsites, lx, ly, reps, ms); return; }
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
        DBuf dPI(pit.size() * sizeof(PairItem)), dGI(git.size() * sizeof(PairGram2Item));
        dPI.up(pit.data(), pit.size() * sizeof(PairItem)); dGI.up(git.data(), git.size() * sizeof(PairGram2Item));
        auto level = [&]() {
            for (int gr = 0; gr < ngroups; ++gr) {
                const int cnt = std::min(G, nsites - gr * G);
                launch_mfma_pair(nullptr, (const PairItem*)dPI.p + (size_t)gr * G, cnt, pw[gr]);
                launch_mfma_pair_gram2(nullptr, (const PairGram2Item*)dGI.p + (size_t)gr * G, cnt, gwg[gr]);
            }
        };
        level();
        HIPCHK(hipEventRecord(e0, nullptr));
        for (int r = 0; r < reps; ++r) level();
        HIPCHK(hipEventRecord(e1, nullptr)); HIPCHK(hipEventSynchronize(e1)); HIPCHK(hipEventElapsedTime(&t, e0, e1));
        std::fprintf(stderr, "level bench: group %d, pair spw %d, gram spw %d\n", G, spw_p, spw_g);
    } else if (which == 0) {
        std::vector<PairItem> items(nsites);
        for (int i = 0; i < nsites; ++i) {
            PairItem& it = items[i]; it.g = g; it.in = (char*)dA.p + (size_t)i * n * 8; it.out = (char*)dB.p + (size_t)i * n * 8;
            it.Mx = dM.p; it.My = (char*)dM.p + 1024 * 8;
        }
        const int wgs = plan_pair(items.data(), nsites);
        DBuf dI(items.size() * sizeof(PairItem)); dI.up(items.data(), items.size() * sizeof(PairItem));
        launch_mfma_pair(nullptr, (const PairItem*)dI.p, nsites, wgs);
        HIPCHK(hipEventRecord(e0, nullptr));
        for (int r = 0; r < reps; ++r) launch_mfma_pair(nullptr, (const PairItem*)dI.p, nsites, wgs);
        HIPCHK(hipEventRecord(e1, nullptr)); HIPCHK(hipEventSynchronize(e1)); HIPCHK(hipEventElapsedTime(&t, e0, e1));
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
        DBuf dI(items.size() * sizeof(PairGram2Item)); dI.up(items.data(), items.size() * sizeof(PairGram2Item));
        launch_mfma_pair_gram2(nullptr, (const PairGram2Item*)dI.p, nsites, wgs);
        HIPCHK(hipEventRecord(e0, nullptr));
        for (int r = 0; r < reps; ++r) launch_mfma_pair_gram2(nullptr, (const PairGram2Item*)dI.p, nsites, wgs);
        HIPCHK(hipEventRecord(e1, nullptr)); HIPCHK(hipEventSynchronize(e1)); HIPCHK(hipEventElapsedTime(&t, e0, e1));
    }
    HIPCHK(hipDeviceSynchronize());
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *ms = (double)t / reps;
}
void dbg_gram_fused(int PA, int K, int PB, const void* X, const void* Y, const void* M, void* out) {
    need_gpu();
    size_t nin = (size_t)PA * K * PB;
    DBuf dX(nin * 8), dY(nin * 8), dM(32 * 32 * 8), dI(sizeof(GramItem)), dR(sizeof(ReduceItem));
    dX.up(X, nin * 8); dY.up(Y, nin * 8); dM.up(M, 32 * 32 * 8);
    GramItem it{}; it.X = dX.p; it.Y = dY.p; it.M = dM.p; it.D = 1; it.PA = PA; it.K = K; it.PB = PB;
    tile_params(PA, PB, 64, it.TA, it.TB, it.nta, it.ntb);
    if (it.TA * it.TB != 64) throw Err(TNQS_ERR_INVALID, "dbg_gram_fused: tiles must hold 64 fibers");
    int npart = 0; plan_gram(&it, 1, GramRoute::Fused32, false, 3, &npart);
    DBuf dP((size_t)npart * K * K * 8), dO((size_t)K * K * 8);
    it.partial = dP.p; dI.up(&it, sizeof(it));
    launch_gram_route<float, float>(nullptr, GramRoute::Fused32, (const GramItem*)dI.p, 1, it.nchunks, 64, K);
    ReduceItem ri{dP.p, dO.p, K * K, npart, 0, 0}; dR.up(&ri, sizeof(ri));
    launch_reduce<float, float>(nullptr, (const ReduceItem*)dR.p, 1, K * K);
    HIPCHK(hipDeviceSynchronize());
    dO.down(out, (size_t)K * K * 8);
}
// the gate path's fused gauge + f64 Gram kernels (kernels_gate.hip) on one site tensor: out[i + KK j] = sum_fibers X'[i, .] conj(X'[j, .]),
// X' = X x_r M with r the lowest leg that is not the bond leg, (i, j) = (s, k); chi_b = 32 (mfma_gauge_gram64_kernel) or 16 (mfma_gauge_gram32_kernel)
void dbg_gauge_gram(int z, const int* chi, int bleg, const void* X, const void* M, void* out) {
    need_gpu();
    if (z < 2 || z > 8 || bleg < 0 || bleg >= z) throw Err(TNQS_ERR_INVALID, "dbg_gauge_gram: bad shape");
    const int rleg = bleg == 0 ? 1 : 0, K = chi[bleg], KK = 2 * K;
    const bool k16 = gauge_gram32_covers(2, z, chi, bleg, rleg), k32 = gauge_gram64_covers(2, z, chi, bleg, rleg);
    if (!k16 && !k32) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_gauge_gram: shape not covered by the fused kernels");
    size_t n = 2; for (int i = 0; i < z; ++i) n *= chi[i];
    long long PA = 1, PB = 1; for (int i = 0; i < bleg; ++i) PA *= chi[i]; for (int i = bleg + 1; i < z; ++i) PB *= chi[i];
    DBuf dX(n * 8), dM((size_t)chi[rleg] * chi[rleg] * 8), dI(sizeof(GramItem)), dR(sizeof(ReduceItem));
    dX.up(X, n * 8); dM.up(M, (size_t)chi[rleg] * chi[rleg] * 8);
    GramItem it{}; it.X = dX.p; it.Y = dX.p; it.M = dM.p; it.D = 2; it.PA = (int)PA; it.K = K; it.PB = (int)PB;
    tile_params(PA, PB, 64, it.TA, it.TB, it.nta, it.ntb);
    if (k16) { it.nta = gauge_gram32_units(z, chi, bleg); it.ntb = 1; }
    const GramRoute r = k16 ? GramRoute::Gauge32 : GramRoute::Gauge64;
    int npart = 0; plan_gram(&it, 1, r, true, 5, &npart);
    DBuf dP((size_t)npart * KK * KK * 16), dO((size_t)KK * KK * 16);
    HIPCHK(hipMemset(dP.p, 0, (size_t)npart * KK * KK * 16));
    it.partial = dP.p; dI.up(&it, sizeof(it));
    launch_gram_route<float, double>(nullptr, r, (const GramItem*)dI.p, 1, it.nchunks, 64, KK);
    ReduceItem ri{dP.p, dO.p, KK * KK, npart, 0, 0}; dR.up(&ri, sizeof(ri));
    launch_reduce<double, double>(nullptr, (const ReduceItem*)dR.p, 1, KK * KK);
    HIPCHK(hipDeviceSynchronize());
    dO.down(out, (size_t)KK * KK * 16);
}

// ---- entry points that reach exactly the kernels of one engine launch: several items per launch, set up as the engine sets them up
// (fiber_plan.cpp, engine_batch.cpp run_chains / run_grams / svd_batch, engine_bp.cpp), a shape the named kernel does not
// take is refused (TNQS_ERR_UNSUPPORTED) and *route says which kernel ran (TNQS_DBG_ROUTE_*, include/tnqs_debug.h) ----
namespace {
template <class F> void cat_offsets(int n, std::vector<size_t>& off, F&& size_of) { off.assign(n + 1, 0); for (int i = 0; i < n; ++i) off[i + 1] = off[i] + size_of(i); }
}
void svd_tall(State* s, const std::vector<JacobiItem>& tall, int* d_fail, int* d_polish_sweeps);

// register-direct fiber GEMM (launch_mfma_rowgemm): items i with (PA[i], PB[i], No[i]), one D and K for the launch; in / X / out are the items'
// arrays one after the other; norm2[i] = the sum of item i's norm partials; tpw <= 0: the engine's rule (D = 2: gate epilogue, D = 1: BP mode product)
void dbg_rowgemm(int D, int K, int nitems, const int* PA, const int* PB, const int* No, const void* in, const void* X, void* out, double* norm2, int tpw, int* route) {
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
    DBuf dIn(oi[nitems] * 8), dX(ox[nitems] * 8), dOut(oo[nitems] * 8), dI(sizeof(FiberItem) * nitems);
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
    dI.up(L.items.data(), sizeof(FiberItem) * nitems);
    launch_fiber_route<float>(nullptr, L, (const FiberItem*)dI.p, (double*)dN.p);
    HIPCHK(hipDeviceSynchronize());
    dOut.down(out, oo[nitems] * 8);
    std::vector<double> np(wgs); dN.down(np.data(), (size_t)wgs * 8);
    for (int i = 0; i < nitems; ++i) {
        double t = 0; for (int w = 0; w < L.nwg[i]; ++w) t += np[L.items[i].tile_begin + w];
        if (norm2) norm2[i] = t;
    }
    if (route) *route = (D * K == 64 && mfma_use_x3()) ? TNQS_DBG_ROUTE_X3 : TNQS_DBG_ROUTE_F32;
}

// matrix-core Grams of 32 < KK <= 64 (launch_mfma_gram64, f32 accumulation, complex64 out; the BP message Gram) and 64 < KK <= 128
// (launch_mfma_gram128_f64, X == Y, complex128 out; the gate-path Gram at chi = 64).  shape: (D, PA, K, PB) per item; Y == NULL: X == Y;
// nchunks <= 0: the engine's chunking (run_grams), else at most that many chunks per item; partials summed with launch_reduce
void dbg_gram_mfma(int nitems, const int* shape, const void* X, const void* Y, void* out, int nchunks, int* route) {
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
    DBuf dX(oi[nitems] * 8), dY(Y ? oi[nitems] * 8 : 1), dO(oo[nitems] * asz), dI(sizeof(GramItem) * nitems), dR(sizeof(ReduceItem) * nitems);
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
    dI.up(items.data(), sizeof(GramItem) * nitems); dR.up(ri.data(), sizeof(ReduceItem) * nitems);
    if (f64) {
        launch_gram_route<float, double>(nullptr, r, (const GramItem*)dI.p, nitems, chunks, 64, KKmax, all128);
        launch_reduce<double, double>(nullptr, (const ReduceItem*)dR.p, nitems, (int)oo[nitems]);
    } else {
        launch_gram_route<float, float>(nullptr, r, (const GramItem*)dI.p, nitems, chunks, 64, KKmax);
        launch_reduce<float, float>(nullptr, (const ReduceItem*)dR.p, nitems, (int)oo[nitems]);
    }
    HIPCHK(hipDeviceSynchronize());
    dO.down(out, oo[nitems] * asz);
    if (route) *route = f64 ? (all128 ? TNQS_DBG_ROUTE_F64_SHARED : TNQS_DBG_ROUTE_F64) : (mfma_use_x3() ? TNQS_DBG_ROUTE_X3 : TNQS_DBG_ROUTE_F32);
}

// chi = 16 planes: item i is a site tensor [d][chi_0]..[chi_{z[i]-1}] (chi: the items' dimensions one after the other) with the plane (lx[i], ly[i])
static void plane_items(int d, int nitems, const int* z, const int* chi, const int* lx, const int* ly, std::vector<PlaneGeom>& g, std::vector<size_t>& off) {
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
// pair of mode products on two 16-dimensional legs (launch_mfma_pair16): out = in x_lx Mx x_ly My per item, M = (Mx, My) per item (2 x 256);
// the items of one launch are of one kind (pair16_whole_lines); spw <= 0: the engine's rule (run_chains)
void dbg_pair16(int d, int nitems, const int* z, const int* chi, const int* lx, const int* ly, const void* in, const void* M, void* out, int spw, int* route) {
    need_gpu();
    std::vector<PlaneGeom> g; std::vector<size_t> off;
    plane_items(d, nitems, z, chi, lx, ly, g, off);
    const bool wl = pair16_whole_lines(g[0]);
    for (int i = 0; i < nitems; ++i) if (pair16_whole_lines(g[i]) != wl) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_pair16: one launch holds items of one kind");
    if (spw > 0 && spw % 4) throw Err(TNQS_ERR_INVALID, "dbg_pair16: spw must be a multiple of 4");
    const size_t n = off[nitems];
    DBuf dIn(n * 8), dOut(n * 8), dM((size_t)nitems * 512 * 8), dI(sizeof(Pair16Item) * nitems);
    dIn.up(in, n * 8); dM.up(M, (size_t)nitems * 512 * 8);
    HIPCHK(hipMemset(dOut.p, 0xff, n * 8));
    std::vector<Pair16Item> items(nitems);
    for (int i = 0; i < nitems; ++i) {
        Pair16Item& it = items[i]; it.g = g[i]; it.in = (char*)dIn.p + off[i] * 8; it.out = (char*)dOut.p + off[i] * 8;
        it.Mx = (char*)dM.p + (size_t)i * 512 * 8; it.My = (char*)it.Mx + 256 * 8;
    }
    int wgs[2]; plan_pair16(items.data(), nitems, wgs, spw);
    dI.up(items.data(), sizeof(Pair16Item) * nitems);
    launch_mfma_pair16(nullptr, (const Pair16Item*)dI.p, nitems, wgs[wl ? 1 : 0], wl);
    HIPCHK(hipDeviceSynchronize());
    dOut.down(out, n * 8);
    if (route) *route = wl ? TNQS_DBG_ROUTE_WHOLE_LINES : TNQS_DBG_ROUTE_HALF_LINES;
}
// both messages of a 16 x 16 plane from one pass (launch_mfma_pair_gram2x16): per item out_y[i] (256 complex64) = sum (X x_lx Mx)[.. b on ly ..]
// conj(Y[.. b' on ly ..]), and when both[i] != 0 out_x[i] = sum (X x_ly My)[.. d on lx ..] conj(Y[.. d' on lx ..]); both[i] == 0 is the single-message
// form of the BP update (My = partial_x = null; out_x[i] is not written).  Partials of a message summed with launch_reduce; spw <= 0: the engine's rule
void dbg_pair_gram2x16(int d, int nitems, const int* z, const int* chi, const int* lx, const int* ly, const int* both, const void* X, const void* Y, const void* M,
                       void* out_y, void* out_x, int spw) {
    need_gpu();
    std::vector<PlaneGeom> g; std::vector<size_t> off;
    plane_items(d, nitems, z, chi, lx, ly, g, off);
    if (!both) throw Err(TNQS_ERR_INVALID, "dbg_pair_gram2x16: bad arguments");
    if (spw > 0 && spw % pair_gram2x16_slices_at_a_time()) throw Err(TNQS_ERR_INVALID, "dbg_pair_gram2x16: spw must be a multiple of the slices a workgroup walks at a time");
    const size_t n = off[nitems];
    std::vector<PairGram2x16Item> items(nitems); std::vector<int> nwg(nitems); for (int i = 0; i < nitems; ++i) items[i].g = g[i];
    const int wgs = plan_pair_gram2x16(items.data(), nitems, nwg.data(), spw);
    DBuf dX(n * 8), dY(n * 8), dM((size_t)nitems * 512 * 8), dI(sizeof(PairGram2x16Item) * nitems), dP((size_t)2 * wgs * 256 * 8), dO((size_t)2 * nitems * 256 * 8),
         dR(sizeof(ReduceItem) * 2 * nitems);
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
    dI.up(items.data(), sizeof(PairGram2x16Item) * nitems); dR.up(ri.data(), sizeof(ReduceItem) * ri.size());
    launch_mfma_pair_gram2x16(nullptr, (const PairGram2x16Item*)dI.p, nitems, wgs);
    launch_reduce<float, float>(nullptr, (const ReduceItem*)dR.p, (int)ri.size(), (int)ri.size() * 256);
    HIPCHK(hipDeviceSynchronize());
    dO.down(out_y, (size_t)nitems * 256 * 8);
    if (out_x) for (int i = 0; i < nitems; ++i) if (both[i]) HIPCHK(hipMemcpy((char*)out_x + (size_t)i * 256 * 8, (char*)dO.p + ((size_t)nitems + i) * 256 * 8, 256 * 8, hipMemcpyDeviceToHost));
}

// svd_batch's tall route (svd_tall: Cholesky-QR, Jacobi on R, A J, polish where the pivot collapsed) on nitems ComplexF32 matrices A_i (m[i] x n[i],
// one after the other): A_i <- U Sigma; chol_fail[i]: the packed Cholesky refused a pivot; polished[i]: the polishing sweeps ran on the item;
// sweeps[i]: the sweeps of the Jacobi on R
void dbg_svd_tall(int nitems, const int* m, const int* n, void* A, int* chol_fail, int* polished, int* sweeps) {
    need_gpu();
    if (nitems < 1 || !m || !n || !A) throw Err(TNQS_ERR_INVALID, "dbg_svd_tall: bad arguments");
    for (int i = 0; i < nitems; ++i)
        if (n[i] < 2 || n[i] > 128 || m[i] < n[i] || m[i] > 512) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_svd_tall: 2 <= n <= 128, n <= m <= 512");
    std::vector<size_t> off; cat_offsets(nitems, off, [&](int i) { return (size_t)m[i] * n[i]; });
    int dev = 0; HIPCHK(hipGetDevice(&dev));
    std::unique_ptr<State> s(state_create(1, 0, nullptr, nullptr, nullptr, TNQS_C64, dev));
    {
        DBuf dA(off[nitems] * 8), dF(sizeof(int) * nitems), dS(sizeof(int) * nitems), dW(sizeof(int) * nitems);
        dA.up(A, off[nitems] * 8);
        HIPCHK(hipMemset(dS.p, 0, sizeof(int) * nitems)); HIPCHK(hipMemset(dW.p, 0xff, sizeof(int) * nitems));      // polish sweeps: -1 = not run
        std::vector<JacobiItem> tall(nitems);
        for (int i = 0; i < nitems; ++i) { JacobiItem j{}; j.A = (char*)dA.p + off[i] * 8; j.m = m[i]; j.n = n[i]; j.sweeps_out = (int*)dS.p + i; tall[i] = j; }
        svd_tall(s.get(), tall, (int*)dF.p, (int*)dW.p);
        HIPCHK(hipStreamSynchronize(s->stream));
        dA.down(A, off[nitems] * 8);
        std::vector<int> f(nitems), w(nitems);
        dF.down(f.data(), sizeof(int) * nitems); dW.down(w.data(), sizeof(int) * nitems);
        if (sweeps) dS.down(sweeps, sizeof(int) * nitems);
        for (int i = 0; i < nitems; ++i) { if (chol_fail) chol_fail[i] = f[i]; if (polished) polished[i] = w[i] >= 0; }
    }
}

// ---- the small-site BP message kernel and the message epilogue, set up as engine_bp.cpp sets them up --------------------------------------------------------
namespace {
// a device array of slots that start at 256-byte multiples (the engine's sub-buffers); the gaps keep a 0xff filling that is checked after the launch, so a
// kernel that writes past its slot is reported instead of going unnoticed.  Plain slots (no guard) are filled with put() and sent with up().
// With guard_bytes the array is an output as the caller hands it over: guard band, item 0, guard band, item 1, ..., guard band.  On the device every item has the band
// that follows it right behind it (the leading band right in front of item 0).  The whole array goes up as the caller filled it (up(src)) and comes back whole
// (down(dst, what)), so a write outside an item shows in a guard band or is reported here
struct Slots {
    size_t gb, total; std::vector<size_t> off, len; std::vector<char> host; std::unique_ptr<DBuf> dev;
    explicit Slots(size_t guard_bytes = 0) : gb(guard_bytes), total(round256(guard_bytes)) {}
    void add(size_t bytes) { off.push_back(total); len.push_back(bytes); total += round256(bytes + gb); }
    void alloc() { host.assign(total ? total : 1, (char)0xff); dev.reset(new DBuf(total)); }
    void put(size_t i, const void* src) { std::memcpy(host.data() + off[i], src, len[i]); }
    void get(size_t i, void* dst) const { std::memcpy(dst, host.data() + off[i], len[i]); }
    char* at(size_t i) const { return (char*)dev->p + off[i]; }
    void up() { dev->up(host.data(), total); }
    void up(const void* src) { caller(const_cast<void*>(src), false); up(); }
    void down(const char* what) { fetch(std::string("dbg: a kernel wrote past the end of a slot of ") + what); }
    void down(void* dst, const char* what) { fetch(std::string("dbg: a kernel wrote outside an item of ") + what); caller(dst, true); }
private:
    void fetch(const std::string& complaint) {
        dev->down(host.data(), total);
        auto gap = [&](size_t b0, size_t b1) { for (size_t b = b0; b < b1; ++b) if (host[b] != (char)0xff) throw Err(TNQS_ERR_INVALID, complaint); };
        gap(0, round256(gb) - gb);
        for (size_t i = 0; i < off.size(); ++i) gap(off[i] + len[i] + gb, off[i] + round256(len[i] + gb));
    }
    void caller(void* arr, bool out) {      // between the caller's contiguous array (bands included) and the slots
        char* p = (char*)arr;
        auto move = [&](char* h, size_t n) { if (out) std::memcpy(p, h, n); else std::memcpy(h, p, n); p += n; };
        move(host.data() + round256(gb) - gb, gb);
        for (size_t i = 0; i < off.size(); ++i) move(host.data() + off[i], len[i] + gb);
    }
};
using Guarded = Slots;      // an output array with guard bands: Guarded g(guard_bytes)
}
// ONE launch_bp_small_site over nitems (site, outgoing leg) pairs (ComplexF32): item i is a site tensor [d[i]][chi_0]..[chi_{z[i]-1}] with the outgoing leg jo[i];
// chi / present: the items' legs one after the other; psi: the items' tensors one after the other; M: one chi_k x chi_k matrix (M[q + chi_k qo]) per leg of every
// item in leg order, read only where present[leg] != 0 (0: a null pointer = identity; the slot of leg jo is handed over as well -- the kernel must skip it).
// form: -1 the engine's rule (matrix-core form iff every leg is 16-dimensional and the element count a multiple of 256), 0 scalar form, 1 matrix-core form or refusal.
// new_msg == NULL: out[i] = the raw message.  Otherwise the epilogue runs as in the engine -- inside the kernel (matrix-core form) or as launch_msg_finalize<float>
// on the one partial (scalar form) -- and out is not written.  out / new_msg / old_msg hold chi_jo^2 numbers per item, one item after the other
void dbg_small_site(int nitems, const int* d, const int* z, const int* chi, const int* jo, const void* psi, const void* M, const int* present, int form,
                    const void* old_msg, const int* has_old, int normalize, void* out, void* new_msg, double* diff, int* route) {
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
    sPsi.alloc(); sM.alloc(); sOut.alloc(); sNew.alloc(); sOld.alloc(); sRaw.alloc();
    DBuf dDiff(sizeof(double) * nitems), dI(sizeof(SmallMsgItem) * nitems), dF(sizeof(MsgFinalItem) * nitems);
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
    sPsi.up(); sM.up(); sOut.up(); sNew.up(); sOld.up(); sRaw.up();
    dDiff.up(hdiff.data(), sizeof(double) * nitems); dI.up(items.data(), sizeof(SmallMsgItem) * nitems);
    if (!fin.empty()) dF.up(fin.data(), sizeof(MsgFinalItem) * fin.size());
    launch_bp_small_site(nullptr, (const SmallMsgItem*)dI.p, nitems, max_elems);
    launch_msg_finalize<float>(nullptr, (const MsgFinalItem*)dF.p, (int)fin.size());
    HIPCHK(hipDeviceSynchronize());
    sOut.down("out"); sNew.down("new_msg"); sRaw.down("the raw message");
    omsg = 0;
    for (int i = 0; i < nitems; ++i) { sOut.get(i, hout + omsg); if (hnew) sNew.get(i, hnew + omsg); omsg += sOut.len[i]; }
    if (diff) dDiff.down(diff, sizeof(double) * nitems);
    if (route) for (int i = 0; i < nitems; ++i) route[i] = items[i].mfma ? TNQS_DBG_ROUTE_SMALL_MFMA16 : TNQS_DBG_ROUTE_SMALL_SCALAR;
}
// ONE launch_msg_finalize<T> over nitems messages: item i has nchunks[i] partials of chi[i]^2 numbers, [chunk][element], the items one after the other; old_msg /
// new_msg: chi[i]^2 numbers per item (has_old[i] == 0 or old_msg == NULL: identity); diff[i] = message_diff(new_i, old_i)
void dbg_msg_finalize(int dtype, int nitems, const int* chi, const int* nchunks, const void* partials, const void* old_msg, const int* has_old, int normalize,
                      void* new_msg, double* diff) {
    need_gpu();
    if ((dtype != TNQS_C64 && dtype != TNQS_C128) || nitems < 1 || !chi || !nchunks || !partials || !new_msg || (old_msg && !has_old))
        throw Err(TNQS_ERR_INVALID, "dbg_msg_finalize: bad arguments");
    const size_t esz = dtype == TNQS_C64 ? 8 : 16;
    Slots sP, sNew, sOld;
    for (int i = 0; i < nitems; ++i) {
        if (chi[i] < 1 || chi[i] > 128 || nchunks[i] < 1) throw Err(TNQS_ERR_INVALID, "dbg_msg_finalize: 1 <= chi <= 128, nchunks >= 1");
        const size_t mb = (size_t)chi[i] * chi[i] * esz;
        sP.add(mb * nchunks[i]); sNew.add(mb); sOld.add(mb);
    }
    sP.alloc(); sNew.alloc(); sOld.alloc();
    DBuf dDiff(sizeof(double) * nitems), dF(sizeof(MsgFinalItem) * nitems);
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
    sP.up(); sNew.up(); sOld.up(); dDiff.up(hdiff.data(), sizeof(double) * nitems); dF.up(fin.data(), sizeof(MsgFinalItem) * nitems);
    if (dtype == TNQS_C64) launch_msg_finalize<float>(nullptr, (const MsgFinalItem*)dF.p, nitems); else launch_msg_finalize<double>(nullptr, (const MsgFinalItem*)dF.p, nitems);
    HIPCHK(hipDeviceSynchronize());
    sNew.down("new_msg");
    om = 0;
    for (int i = 0; i < nitems; ++i) { sNew.get(i, (char*)new_msg + om); om += sNew.len[i]; }
    if (diff) dDiff.down(diff, sizeof(double) * nitems);
}

// ---- loop corrections (kernels_loop.hip): ONE launch over nitems items of different shapes, the items' matrices one after the other in A, B (and C, between
// guard bands of `guard` elements that the caller has filled and gets back: whatever the kernel must leave alone is seen to be left alone) ----
void dbg_loop_cgemm(int dtype, int opB, int nitems, const int* m, const int* n, const int* k, const void* A, const void* B, void* C, int guard) {
    need_gpu();
    if ((dtype != TNQS_C64 && dtype != TNQS_C128) || nitems < 1 || !m || !n || !k || !A || !B || !C || guard < 0) throw Err(TNQS_ERR_INVALID, "dbg_loop_cgemm: bad arguments");
    const size_t esz = dtype == TNQS_C64 ? 8 : 16;
    size_t na = 0, nb = 0, nc = (size_t)guard;
    std::vector<LoopGemmItem> items(nitems);
    for (int i = 0; i < nitems; ++i) {
        if (m[i] < 1 || n[i] < 1 || k[i] < 1) throw Err(TNQS_ERR_INVALID, "dbg_loop_cgemm: m, n, k >= 1");
        LoopGemmItem& it = items[i]; it = LoopGemmItem{};
        it.A = (const void*)(na * esz); it.B = (const void*)(nb * esz); it.C = (void*)(nc * esz);      // offsets for now
        it.m = m[i]; it.n = n[i]; it.k = k[i]; it.opB = opB ? 1 : 0; it.I0 = m[i]; it.si0 = 1; it.J0 = n[i]; it.sj0 = m[i];
        na += (size_t)m[i] * k[i]; nb += (size_t)n[i] * k[i]; nc += (size_t)m[i] * n[i] + guard;
    }
    DBuf dA(na * esz), dB(nb * esz), dC(nc * esz), dI(sizeof(LoopGemmItem) * nitems);
    for (auto& it : items) { it.A = (char*)dA.p + (size_t)it.A; it.B = (char*)dB.p + (size_t)it.B; it.C = (char*)dC.p + (size_t)it.C; }
    const int tiles = plan_loop_cgemm(items.data(), nitems);
    dA.up(A, na * esz); dB.up(B, nb * esz); dC.up(C, nc * esz); dI.up(items.data(), sizeof(LoopGemmItem) * nitems);
    if (dtype == TNQS_C64) launch_loop_cgemm<float>(nullptr, (const LoopGemmItem*)dI.p, nitems, tiles); else launch_loop_cgemm<double>(nullptr, (const LoopGemmItem*)dI.p, nitems, tiles);
    HIPCHK(hipDeviceSynchronize());
    dC.down(C, nc * esz);
}
// T_i (nr[i] x nc[i], in place) <- T_i - f_i (b_i^T T_i); f, b: nr[i] elements per item
void dbg_loop_antiproject(int dtype, int nitems, const int* nr, const int* nc, void* Tm, const void* f, const void* b) {
    need_gpu();
    if ((dtype != TNQS_C64 && dtype != TNQS_C128) || nitems < 1 || !nr || !nc || !Tm || !f || !b) throw Err(TNQS_ERR_INVALID, "dbg_loop_antiproject: bad arguments");
    const size_t esz = dtype == TNQS_C64 ? 8 : 16;
    size_t nt = 0, nv = 0;
    std::vector<LoopProjItem> items(nitems);
    for (int i = 0; i < nitems; ++i) {
        if (nr[i] < 1 || nc[i] < 1) throw Err(TNQS_ERR_INVALID, "dbg_loop_antiproject: nr, nc >= 1");
        items[i] = LoopProjItem{(void*)(nt * esz), (const void*)(nv * esz), (const void*)(nv * esz), nr[i], nc[i], 0};
        nt += (size_t)nr[i] * nc[i]; nv += (size_t)nr[i];
    }
    DBuf dT(nt * esz), dF(nv * esz), dB(nv * esz), dI(sizeof(LoopProjItem) * nitems);
    for (auto& it : items) { it.T = (char*)dT.p + (size_t)it.T; it.f = (char*)dF.p + (size_t)it.f; it.b = (char*)dB.p + (size_t)it.b; }
    const int wgs = plan_loop_antiproject(items.data(), nitems);
    dT.up(Tm, nt * esz); dF.up(f, nv * esz); dB.up(b, nv * esz); dI.up(items.data(), sizeof(LoopProjItem) * nitems);
    if (dtype == TNQS_C64) launch_loop_antiproject<float>(nullptr, (const LoopProjItem*)dI.p, nitems, wgs); else launch_loop_antiproject<double>(nullptr, (const LoopProjItem*)dI.p, nitems, wgs);
    HIPCHK(hipDeviceSynchronize());
    dT.down(Tm, nt * esz);
}
// out[i] (complex128) = sum_ab X_i[a,b] Y_i[b,a]; X_i: p[i] x q[i], Y_i: q[i] x p[i]
void dbg_loop_trace(int dtype, int nitems, const int* p, const int* q, const void* X, const void* Y, double* out) {
    need_gpu();
    if ((dtype != TNQS_C64 && dtype != TNQS_C128) || nitems < 1 || !p || !q || !X || !Y || !out) throw Err(TNQS_ERR_INVALID, "dbg_loop_trace: bad arguments");
    const size_t esz = dtype == TNQS_C64 ? 8 : 16;
    size_t ne = 0;
    std::vector<LoopTraceItem> items(nitems);
    DBuf dP(sizeof(double) * 128 * nitems), dO(sizeof(double) * 2 * nitems);
    for (int i = 0; i < nitems; ++i) {
        if (p[i] < 1 || q[i] < 1) throw Err(TNQS_ERR_INVALID, "dbg_loop_trace: p, q >= 1");
        items[i] = LoopTraceItem{(const void*)(ne * esz), (const void*)(ne * esz), p[i], q[i], (double*)dP.p + 128 * (size_t)i, (double*)dO.p + 2 * (size_t)i, 0, 0};
        ne += (size_t)p[i] * q[i];
    }
    DBuf dX(ne * esz), dY(ne * esz), dI(sizeof(LoopTraceItem) * nitems);
    for (auto& it : items) { it.X = (char*)dX.p + (size_t)it.X; it.Y = (char*)dY.p + (size_t)it.Y; }
    const int wgs = plan_loop_trace(items.data(), nitems);
    dX.up(X, ne * esz); dY.up(Y, ne * esz); dI.up(items.data(), sizeof(LoopTraceItem) * nitems);
    if (dtype == TNQS_C64) launch_loop_trace<float>(nullptr, (const LoopTraceItem*)dI.p, nitems, wgs); else launch_loop_trace<double>(nullptr, (const LoopTraceItem*)dI.p, nitems, wgs);
    HIPCHK(hipDeviceSynchronize());
    dO.down(out, sizeof(double) * 2 * nitems);
}
// ---- the kernels that post-process a BP cache and prepare a gate's environments (kernels_bp.hip: msg_rescale, edge_scalar, symg_build, symg_finish; kernels_chol.hip:
// env_prepare, env_finish; kernels_util.hip: diag, cscale): ONE launch over nitems items of different n, the descriptors filled as engine_obs.cpp / engine_gates.cpp
// fill them.  Inputs: the items' arrays one after the other.  Outputs: `guard` caller-filled elements, item 0, `guard` elements, item 1, ..., `guard` elements ----
namespace {
// input arrays: the items one after the other on the host, 256-byte aligned slots on the device
void put_all(Slots& s, const void* src) { const char* p = (const char*)src; for (size_t i = 0; i < s.off.size(); ++i) { s.put(i, p); p += s.len[i]; } }
void post_check(const char* who, int dtype, int nitems, const int* n, int guard) {
    if ((dtype != TNQS_C64 && dtype != TNQS_C128) || nitems < 1 || !n || guard < 0) throw Err(TNQS_ERR_INVALID, std::string(who) + ": bad arguments");
    for (int i = 0; i < nitems; ++i) {
        if (n[i] < 1) throw Err(TNQS_ERR_INVALID, std::string(who) + ": n >= 1");
        if (n[i] > 256) throw Err(TNQS_ERR_UNSUPPORTED, std::string(who) + ": bond dimension > 256");
    }
}
}
void dbg_msg_rescale(int dtype, int nitems, const int* chi, const void* me, const void* mer, const int* present, void* me_out, void* mer_out, int guard) {
    need_gpu();
    post_check("dbg_msg_rescale", dtype, nitems, chi, guard);
    if (!me || !mer || !present || !me_out || !mer_out) throw Err(TNQS_ERR_INVALID, "dbg_msg_rescale: bad arguments");
    const size_t esz = dtype == TNQS_C64 ? 8 : 16;
    Slots sA, sB; Guarded gA(guard * esz), gB(guard * esz);
    for (int i = 0; i < nitems; ++i) { const size_t mb = (size_t)chi[i] * chi[i] * esz; sA.add(mb); sB.add(mb); gA.add(mb); gB.add(mb); }
    sA.alloc(); sB.alloc(); gA.alloc(); gB.alloc();
    put_all(sA, me); put_all(sB, mer);
    std::vector<MsgRescaleItem> items(nitems);
    for (int i = 0; i < nitems; ++i) items[i] = MsgRescaleItem{present[2 * i] ? sA.at(i) : nullptr, present[2 * i + 1] ? sB.at(i) : nullptr, gA.at(i), gB.at(i), chi[i]};
    DBuf dI(sizeof(MsgRescaleItem) * nitems);
    sA.up(); sB.up(); gA.up(me_out); gB.up(mer_out); dI.up(items.data(), sizeof(MsgRescaleItem) * nitems);
    if (dtype == TNQS_C64) launch_msg_rescale<float>(nullptr, (const MsgRescaleItem*)dI.p, nitems); else launch_msg_rescale<double>(nullptr, (const MsgRescaleItem*)dI.p, nitems);
    HIPCHK(hipDeviceSynchronize());
    gA.down(me_out, "me_out"); gB.down(mer_out, "mer_out");
}
void dbg_edge_scalar(int dtype, int nitems, const int* chi, const void* me, const void* mer, const int* present, double* out) {
    need_gpu();
    post_check("dbg_edge_scalar", dtype, nitems, chi, 0);
    if (!me || !mer || !present || !out) throw Err(TNQS_ERR_INVALID, "dbg_edge_scalar: bad arguments");
    const size_t esz = dtype == TNQS_C64 ? 8 : 16;
    Slots sA, sB;
    for (int i = 0; i < nitems; ++i) { const size_t mb = (size_t)chi[i] * chi[i] * esz; sA.add(mb); sB.add(mb); }
    sA.alloc(); sB.alloc();
    put_all(sA, me); put_all(sB, mer);
    DBuf dO(16 * (size_t)nitems), dI(sizeof(EdgeScalarItem) * nitems);
    std::vector<EdgeScalarItem> items(nitems);
    for (int i = 0; i < nitems; ++i) items[i] = EdgeScalarItem{present[2 * i] ? sA.at(i) : nullptr, present[2 * i + 1] ? sB.at(i) : nullptr, chi[i], (double*)dO.p + 2 * i};
    sA.up(); sB.up(); dO.up(out, 16 * (size_t)nitems); dI.up(items.data(), sizeof(EdgeScalarItem) * nitems);
    if (dtype == TNQS_C64) launch_edge_scalar<float>(nullptr, (const EdgeScalarItem*)dI.p, nitems); else launch_edge_scalar<double>(nullptr, (const EdgeScalarItem*)dI.p, nitems);
    HIPCHK(hipDeviceSynchronize());
    dO.down(out, 16 * (size_t)nitems);
}
void dbg_env_prepare(int dtype, int nitems, const int* n, const void* msg, const int* present, void* H_out, void* V_out, int guard) {
    need_gpu();
    post_check("dbg_env_prepare", dtype, nitems, n, guard);
    if (!msg || !present || !H_out || !V_out) throw Err(TNQS_ERR_INVALID, "dbg_env_prepare: bad arguments");
    const size_t esz = dtype == TNQS_C64 ? 8 : 16;
    Slots sM; Guarded gH((size_t)guard * 16), gV((size_t)guard * 16);
    for (int i = 0; i < nitems; ++i) { const size_t nn = (size_t)n[i] * n[i]; sM.add(nn * esz); gH.add(nn * 16); gV.add(nn * 16); }
    sM.alloc(); gH.alloc(); gV.alloc();
    put_all(sM, msg);
    std::vector<EnvItem> items(nitems);
    for (int i = 0; i < nitems; ++i) items[i] = EnvItem{present[i] ? sM.at(i) : nullptr, gH.at(i), gV.at(i), n[i]};
    DBuf dI(sizeof(EnvItem) * nitems);
    sM.up(); gH.up(H_out); gV.up(V_out); dI.up(items.data(), sizeof(EnvItem) * nitems);
    if (dtype == TNQS_C64) launch_env_prepare<float>(nullptr, (const EnvItem*)dI.p, nitems); else launch_env_prepare<double>(nullptr, (const EnvItem*)dI.p, nitems);
    HIPCHK(hipDeviceSynchronize());
    gH.down(H_out, "H"); gV.down(V_out, "V");
}
void dbg_env_finish(int dtype, int nitems, const int* n, const void* A, const void* V, const double* cutoff, void* msqrt_out, void* proj_out, int* flags_out, int guard) {
    need_gpu();
    post_check("dbg_env_finish", dtype, nitems, n, guard);
    if (!A || !V || !cutoff || !msqrt_out || !proj_out || !flags_out) throw Err(TNQS_ERR_INVALID, "dbg_env_finish: bad arguments");
    const size_t esz = dtype == TNQS_C64 ? 8 : 16;
    Slots sA, sV; Guarded gM(guard * esz), gP(guard * esz);
    for (int i = 0; i < nitems; ++i) { const size_t nn = (size_t)n[i] * n[i]; sA.add(nn * 16); sV.add(nn * 16); gM.add(nn * esz); gP.add(nn * esz); }
    sA.alloc(); sV.alloc(); gM.alloc(); gP.alloc();
    put_all(sA, A); put_all(sV, V);
    DBuf dF(sizeof(int) * 2 * nitems), dI(sizeof(EnvFinishItem) * nitems);
    std::vector<EnvFinishItem> items(nitems);
    for (int i = 0; i < nitems; ++i) items[i] = EnvFinishItem{sA.at(i), sV.at(i), gM.at(i), gP.at(i), n[i], cutoff[i], (int*)dF.p + 2 * i};
    sA.up(); sV.up(); gM.up(msqrt_out); gP.up(proj_out); dF.up(flags_out, sizeof(int) * 2 * nitems); dI.up(items.data(), sizeof(EnvFinishItem) * nitems);
    if (dtype == TNQS_C64) launch_env_finish<float>(nullptr, (const EnvFinishItem*)dI.p, nitems); else launch_env_finish<double>(nullptr, (const EnvFinishItem*)dI.p, nitems);
    HIPCHK(hipDeviceSynchronize());
    gM.down(msqrt_out, "msqrt"); gP.down(proj_out, "proj"); dF.down(flags_out, sizeof(int) * 2 * nitems);
}
// (the pointers of a SymGaugeItem that the launched kernel does not use point at a scratch slot of the item's size)
void dbg_symg_build(int dtype, int nitems, const int* n, const void* AX, const void* VX, const void* AY, const void* VY, double reg, void* rx, void* ry, void* irx, void* iry,
                    void* Ce, void* Ce0, int* flag_out, int guard) {
    need_gpu();
    post_check("dbg_symg_build", dtype, nitems, n, guard);
    if (!AX || !VX || !AY || !VY || !rx || !ry || !irx || !iry || !Ce || !Ce0 || !flag_out) throw Err(TNQS_ERR_INVALID, "dbg_symg_build: bad arguments");
    const size_t esz = dtype == TNQS_C64 ? 8 : 16;
    Slots sAX, sVX, sAY, sVY, scr; Guarded gRx((size_t)guard * 16), gRy((size_t)guard * 16), gIx((size_t)guard * 16), gIy((size_t)guard * 16), gC(guard * esz), gC0(guard * esz);
    for (int i = 0; i < nitems; ++i) {
        const size_t nn = (size_t)n[i] * n[i];
        for (Slots* s : {&sAX, &sVX, &sAY, &sVY, &scr}) s->add(nn * 16);
        for (Guarded* g : {&gRx, &gRy, &gIx, &gIy}) g->add(nn * 16);
        gC.add(nn * esz); gC0.add(nn * esz);
    }
    for (Slots* s : {&sAX, &sVX, &sAY, &sVY, &scr}) s->alloc();
    for (Guarded* g : {&gRx, &gRy, &gIx, &gIy, &gC, &gC0}) g->alloc();
    put_all(sAX, AX); put_all(sVX, VX); put_all(sAY, AY); put_all(sVY, VY);
    DBuf dFlag(sizeof(int)), dI(sizeof(SymGaugeItem) * nitems);
    HIPCHK(hipMemset(dFlag.p, 0, sizeof(int)));          // one flag for the whole launch, cleared first (engine_obs.cpp)
    std::vector<SymGaugeItem> items(nitems);
    for (int i = 0; i < nitems; ++i)
        items[i] = SymGaugeItem{sAX.at(i), sVX.at(i), sAY.at(i), sVY.at(i), gRx.at(i), gRy.at(i), gIx.at(i), gIy.at(i), gC.at(i), gC0.at(i), scr.at(i), scr.at(i), scr.at(i),
                                (double*)scr.at(i), n[i], reg, (int*)dFlag.p};
    sAX.up(); sVX.up(); sAY.up(); sVY.up(); scr.up();
    gRx.up(rx); gRy.up(ry); gIx.up(irx); gIy.up(iry); gC.up(Ce); gC0.up(Ce0); dI.up(items.data(), sizeof(SymGaugeItem) * nitems);
    if (dtype == TNQS_C64) launch_symg_build<float>(nullptr, (const SymGaugeItem*)dI.p, nitems); else launch_symg_build<double>(nullptr, (const SymGaugeItem*)dI.p, nitems);
    HIPCHK(hipDeviceSynchronize());
    gRx.down(rx, "rx"); gRy.down(ry, "ry"); gIx.down(irx, "irx"); gIy.down(iry, "iry"); gC.down(Ce, "Ce"); gC0.down(Ce0, "Ce0");
    dFlag.down(flag_out, sizeof(int));
}
void dbg_symg_finish(int dtype, int nitems, const int* n, const void* USigma, const void* Vsvd, const void* irx, const void* iry, void* Xs, void* Xd, double* S, int guard) {
    need_gpu();
    post_check("dbg_symg_finish", dtype, nitems, n, guard);
    if (!USigma || !Vsvd || !irx || !iry || !Xs || !Xd || !S) throw Err(TNQS_ERR_INVALID, "dbg_symg_finish: bad arguments");
    const size_t esz = dtype == TNQS_C64 ? 8 : 16;
    Slots sU, sV, sIx, sIy, scr; Guarded gXs(guard * esz), gXd(guard * esz), gS((size_t)guard * 8);
    for (int i = 0; i < nitems; ++i) {
        const size_t nn = (size_t)n[i] * n[i];
        sU.add(nn * esz); sV.add(nn * esz); sIx.add(nn * 16); sIy.add(nn * 16); scr.add(nn * 16);
        gXs.add(nn * esz); gXd.add(nn * esz); gS.add((size_t)n[i] * 8);
    }
    for (Slots* s : {&sU, &sV, &sIx, &sIy, &scr}) s->alloc();
    gXs.alloc(); gXd.alloc(); gS.alloc();
    put_all(sU, USigma); put_all(sV, Vsvd); put_all(sIx, irx); put_all(sIy, iry);
    DBuf dFlag(sizeof(int)), dI(sizeof(SymGaugeItem) * nitems);
    HIPCHK(hipMemset(dFlag.p, 0, sizeof(int)));
    std::vector<SymGaugeItem> items(nitems);
    for (int i = 0; i < nitems; ++i)
        items[i] = SymGaugeItem{scr.at(i), scr.at(i), scr.at(i), scr.at(i), scr.at(i), scr.at(i), sIx.at(i), sIy.at(i), sU.at(i), scr.at(i), sV.at(i), gXs.at(i), gXd.at(i),
                                (double*)gS.at(i), n[i], 0.0, (int*)dFlag.p};
    sU.up(); sV.up(); sIx.up(); sIy.up(); scr.up(); gXs.up(Xs); gXd.up(Xd); gS.up(S); dI.up(items.data(), sizeof(SymGaugeItem) * nitems);
    if (dtype == TNQS_C64) launch_symg_finish<float>(nullptr, (const SymGaugeItem*)dI.p, nitems); else launch_symg_finish<double>(nullptr, (const SymGaugeItem*)dI.p, nitems);
    HIPCHK(hipDeviceSynchronize());
    gXs.down(Xs, "Xs"); gXd.down(Xd, "Xd"); gS.down(S, "S");
}
void dbg_diag(int dtype, int nitems, const int* chi, const double* S, void* out, int guard) {
    need_gpu();
    post_check("dbg_diag", dtype, nitems, chi, guard);
    if (!S || !out) throw Err(TNQS_ERR_INVALID, "dbg_diag: bad arguments");
    const size_t esz = dtype == TNQS_C64 ? 8 : 16;
    Slots sS; Guarded gO(guard * esz);
    for (int i = 0; i < nitems; ++i) { sS.add((size_t)chi[i] * 8); gO.add((size_t)chi[i] * chi[i] * esz); }
    sS.alloc(); gO.alloc();
    put_all(sS, S);
    std::vector<DiagItem> items(nitems);
    for (int i = 0; i < nitems; ++i) items[i] = DiagItem{gO.at(i), (const double*)sS.at(i), chi[i]};
    DBuf dI(sizeof(DiagItem) * nitems);
    sS.up(); gO.up(out); dI.up(items.data(), sizeof(DiagItem) * nitems);
    if (dtype == TNQS_C64) launch_diag<float>(nullptr, (const DiagItem*)dI.p, nitems); else launch_diag<double>(nullptr, (const DiagItem*)dI.p, nitems);
    HIPCHK(hipDeviceSynchronize());
    gO.down(out, "out");
}
void dbg_cscale(int dtype, int nitems, const int* len, const void* src, const double* re, const double* im, void* dst, int guard) {
    need_gpu();
    if ((dtype != TNQS_C64 && dtype != TNQS_C128) || nitems < 1 || !len || !src || !re || !im || !dst || guard < 0) throw Err(TNQS_ERR_INVALID, "dbg_cscale: bad arguments");
    const size_t esz = dtype == TNQS_C64 ? 8 : 16;
    Slots sS; Guarded gD(guard * esz);
    for (int i = 0; i < nitems; ++i) { if (len[i] < 1) throw Err(TNQS_ERR_INVALID, "dbg_cscale: len >= 1"); sS.add((size_t)len[i] * esz); gD.add((size_t)len[i] * esz); }
    sS.alloc(); gD.alloc();
    put_all(sS, src);
    std::vector<CScaleItem> items(nitems);
    for (int i = 0; i < nitems; ++i) items[i] = CScaleItem{sS.at(i), gD.at(i), (size_t)len[i], re[i], im[i]};
    DBuf dI(sizeof(CScaleItem) * nitems);
    sS.up(); gD.up(dst); dI.up(items.data(), sizeof(CScaleItem) * nitems);
    if (dtype == TNQS_C64) launch_cscale<float>(nullptr, (const CScaleItem*)dI.p, nitems); else launch_cscale<double>(nullptr, (const CScaleItem*)dI.p, nitems);
    HIPCHK(hipDeviceSynchronize());
    gD.down(dst, "dst");
}
// edge_rdm_kernel<P> (kernels_rdm.hip), ONE launch over nitems bonds set up as engine_rdm.cpp sets them up: the items' Gram partials one after the other in partial_u /
// partial_v (P numbers), scale_u / scale_v one double per item (0: a null pointer), out between guard bands of `guard` complex128 elements
// ptype_u / ptype_v: the partial type of each end (dbg_edge_rdm: the same for both)
void dbg_edge_rdm_mixed(int ptype_u, int ptype_v, int nitems, const int* du, const int* dv, const int* chi, const int* nchunks_u, const int* nchunks_v, const void* partial_u,
                        const void* partial_v, const double* scale_u, const double* scale_v, void* out, int guard) {
    need_gpu();
    if ((ptype_u != 0 && ptype_u != 1) || (ptype_v != 0 && ptype_v != 1) || nitems < 1 || !du || !dv || !chi || !nchunks_u || !nchunks_v || !partial_u || !partial_v || !scale_u || !scale_v || !out || guard < 0)
        throw Err(TNQS_ERR_INVALID, "dbg_edge_rdm: bad arguments");
    const size_t psz_u = ptype_u == 0 ? 8 : 16, psz_v = ptype_v == 0 ? 8 : 16;
    Slots sU, sV, sS; Guarded gO((size_t)guard * 16);
    for (int i = 0; i < nitems; ++i) {
        if (du[i] < 1 || dv[i] < 1 || chi[i] < 1 || nchunks_u[i] < 1 || nchunks_v[i] < 1) throw Err(TNQS_ERR_INVALID, "dbg_edge_rdm: dimensions and chunk counts >= 1");
        if (edge_rdm_block(du[i], dv[i], chi[i]) < 1) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_edge_rdm: bond too large for the edge kernel");
        const size_t ku = (size_t)du[i] * chi[i], kv = (size_t)dv[i] * chi[i], dd = (size_t)du[i] * dv[i];
        sU.add((size_t)nchunks_u[i] * ku * ku * psz_u); sV.add((size_t)nchunks_v[i] * kv * kv * psz_v); sS.add(16); gO.add(dd * dd * 16);
    }
    sU.alloc(); sV.alloc(); sS.alloc(); gO.alloc();
    put_all(sU, partial_u); put_all(sV, partial_v);
    std::vector<EdgeRdmItem> items(nitems);
    for (int i = 0; i < nitems; ++i) {
        const double f[2] = {scale_u[i], scale_v[i]}; sS.put(i, f);
        items[i] = EdgeRdmItem{sU.at(i), sV.at(i), nchunks_u[i], nchunks_v[i], du[i], dv[i], chi[i],
                               f[0] != 0.0 ? reinterpret_cast<const double*>(sS.at(i)) : nullptr, f[1] != 0.0 ? reinterpret_cast<const double*>(sS.at(i)) + 1 : nullptr, gO.at(i)};
    }
    DBuf dI(sizeof(EdgeRdmItem) * nitems);
    sU.up(); sV.up(); sS.up(); gO.up(out); dI.up(items.data(), sizeof(EdgeRdmItem) * nitems);
    const EdgeRdmItem* di = (const EdgeRdmItem*)dI.p;
    if (ptype_u == ptype_v) { if (ptype_u == 0) launch_edge_rdm<float>(nullptr, di, nitems); else launch_edge_rdm<double>(nullptr, di, nitems); }
    else if (ptype_u == 0) launch_edge_rdm_mixed<float, double>(nullptr, di, nitems); else launch_edge_rdm_mixed<double, float>(nullptr, di, nitems);
    HIPCHK(hipDeviceSynchronize());
    gO.down(out, "out");
}
void dbg_edge_rdm(int ptype, int nitems, const int* du, const int* dv, const int* chi, const int* nchunks_u, const int* nchunks_v, const void* partial_u, const void* partial_v,
                  const double* scale_u, const double* scale_v, void* out, int guard) {
    dbg_edge_rdm_mixed(ptype, ptype, nitems, du, dv, chi, nchunks_u, nchunks_v, partial_u, partial_v, scale_u, scale_v, out, guard);
}
// bond entanglement spectra (kernels_spectrum.hip), stages A-D over nitems bonds of different chi exactly as engine_spectra.cpp runs them (fill_bond_spec_items,
// launch_bond_spectra_stages): m1 / m2 hold the items' chi x chi messages one after the other in the state's type, present[2 i], present[2 i + 1] = 0 hands the kernels a
// null pointer for m1 / m2 (identity); the cutoff follows from the dtype.  out: chi[i] doubles per item between guard bands of `guard` doubles; flags_out: one int per item
// (bit 1: a message eigenvalue <= -cutoff, bit 2: trace not positive and finite)
void dbg_bond_spectrum(int dtype, int nitems, const int* chi, const void* m1, const void* m2, const int* present, double* out, int* flags_out, int guard) {
    need_gpu();
    post_check("dbg_bond_spectrum", dtype, nitems, chi, guard);
    if (!m1 || !m2 || !present || !out || !flags_out) throw Err(TNQS_ERR_INVALID, "dbg_bond_spectrum: bad arguments");
    const size_t esz = dtype == TNQS_C64 ? 8 : 16;
    Slots s1, s2, sH, sV, sW, sV2; Guarded gO((size_t)guard * 8);
    for (int i = 0; i < nitems; ++i) {
        const size_t nn = (size_t)chi[i] * chi[i];
        s1.add(nn * esz); s2.add(nn * esz); gO.add((size_t)chi[i] * 8);
        for (Slots* s : {&sH, &sV, &sW, &sV2}) s->add(nn * 16);
    }
    for (Slots* s : {&s1, &s2, &sH, &sV, &sW, &sV2}) s->alloc();
    gO.alloc();
    put_all(s1, m1); put_all(s2, m2);
    DBuf dTr(8 * (size_t)nitems), dFlag(sizeof(int) * (size_t)nitems);
    HIPCHK(hipMemset(dFlag.p, 0, sizeof(int) * (size_t)nitems));
    std::vector<BondSpecBufs> bufs(nitems);
    for (int i = 0; i < nitems; ++i)
        bufs[i] = BondSpecBufs{present[2 * i] ? s1.at(i) : nullptr, present[2 * i + 1] ? s2.at(i) : nullptr, sH.at(i), sV.at(i), sW.at(i), sV2.at(i),
                               (double*)dTr.p + i, (double*)gO.at(i), chi[i], (int*)dFlag.p + i};
    std::vector<EnvItem> ei; std::vector<JacobiItem> j1, j2; std::vector<BondSpecItem> items;
    const BondSpecLaunch L = fill_bond_spec_items(bufs, bond_spectrum_cutoff(dtype), ei, j1, j2, items);
    DBuf dE(sizeof(EnvItem) * nitems), dJ1(sizeof(JacobiItem) * nitems), dJ2(sizeof(JacobiItem) * nitems), dI(sizeof(BondSpecItem) * nitems);
    for (Slots* s : {&s1, &s2, &sH, &sV, &sW, &sV2}) s->up();
    gO.up(out);
    dE.up(ei.data(), sizeof(EnvItem) * nitems); dJ1.up(j1.data(), sizeof(JacobiItem) * nitems); dJ2.up(j2.data(), sizeof(JacobiItem) * nitems);
    dI.up(items.data(), sizeof(BondSpecItem) * nitems);
    if (dtype == TNQS_C64) launch_bond_spectra_stages<float>(nullptr, (const EnvItem*)dE.p, (const JacobiItem*)dJ1.p, (const JacobiItem*)dJ2.p, (const BondSpecItem*)dI.p, L);
    else launch_bond_spectra_stages<double>(nullptr, (const EnvItem*)dE.p, (const JacobiItem*)dJ1.p, (const JacobiItem*)dJ2.p, (const BondSpecItem*)dI.p, L);
    HIPCHK(hipDeviceSynchronize());
    for (Slots* s : {&sH, &sV, &sW, &sV2}) s->down("the bond-spectrum workspace");
    gO.down(out, "out");
    dFlag.down(flags_out, sizeof(int) * (size_t)nitems);
}
// path_apply_kernel<P, T> (kernels_rdm.hip), ONE launch over nitems (environment, transfer matrix) pairs set up as engine_paths.cpp sets them up: L_in holds the items'
// nchunks_in[i] chunks of (d chi_a)^2 numbers of type P one after the other, T the items' chi_b^2 x chi_a^2 matrices of the state's type, scale one double per item (0: a
// null pointer), L_out ksplit[i] chunks of (d chi_b)^2 complex128 per item between guard bands of `guard` elements; ksplit[i] = 0: as plan_path_apply chooses
void dbg_path_apply(int ptype_in, int dtype, int nitems, const int* d, const int* chi_a, const int* chi_b, const int* nchunks_in, const int* ksplit, const void* L_in, const void* T,
                    const double* scale, void* L_out, int guard) {
    need_gpu();
    if ((ptype_in != 0 && ptype_in != 1) || (dtype != TNQS_C64 && dtype != TNQS_C128) || nitems < 1 || !d || !chi_a || !chi_b || !nchunks_in || !ksplit || !L_in || !T || !scale || !L_out || guard < 0)
        throw Err(TNQS_ERR_INVALID, "dbg_path_apply: bad arguments");
    const size_t psz = ptype_in == 0 ? 8 : 16, esz = dtype == TNQS_C64 ? 8 : 16;
    std::vector<PathApplyItem> items(nitems);
    for (int i = 0; i < nitems; ++i) {
        if (d[i] < 1 || chi_a[i] < 1 || chi_b[i] < 1 || nchunks_in[i] < 1 || ksplit[i] < 0) throw Err(TNQS_ERR_INVALID, "dbg_path_apply: dimensions and chunk counts >= 1, splits >= 0");
        if (d[i] * d[i] > 16) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_path_apply: more than 16 rows (d > 4)");
        if ((size_t)chi_a[i] * chi_a[i] * chi_b[i] * chi_b[i] > (size_t)INT_MAX / 4) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_path_apply: bond dimension too large");
        items[i] = PathApplyItem{nullptr, nullptr, nullptr, nullptr, d[i], chi_a[i], chi_b[i], nchunks_in[i], ksplit[i], 0, 0};
    }
    const int wgs = plan_path_apply(items.data(), nitems);
    for (int i = 0; i < nitems; ++i) if (ksplit[i] == 0 ? items[i].ksplit < 1 : items[i].ksplit != ksplit[i]) throw Err(TNQS_ERR_INVALID, "dbg_path_apply: the plan changed a given split");
    Slots sL, sT, sS; Guarded gO((size_t)guard * 16);
    for (int i = 0; i < nitems; ++i) {
        const size_t ka = (size_t)d[i] * chi_a[i], kb = (size_t)d[i] * chi_b[i];
        sL.add((size_t)nchunks_in[i] * ka * ka * psz); sT.add((size_t)chi_a[i] * chi_a[i] * chi_b[i] * chi_b[i] * esz); sS.add(8); gO.add((size_t)items[i].ksplit * kb * kb * 16);
    }
    sL.alloc(); sT.alloc(); sS.alloc(); gO.alloc();
    put_all(sL, L_in); put_all(sT, T);
    for (int i = 0; i < nitems; ++i) {
        sS.put(i, &scale[i]);
        items[i].L_in = sL.at(i); items[i].T = sT.at(i); items[i].L_out = gO.at(i); items[i].scale = scale[i] != 0.0 ? reinterpret_cast<const double*>(sS.at(i)) : nullptr;
    }
    DBuf dI(sizeof(PathApplyItem) * nitems);
    sL.up(); sT.up(); sS.up(); gO.up(L_out); dI.up(items.data(), sizeof(PathApplyItem) * nitems);
    const PathApplyItem* di = (const PathApplyItem*)dI.p;
    if (dtype == TNQS_C64) { if (ptype_in == 0) launch_path_apply<float, float>(nullptr, di, nitems, wgs); else launch_path_apply<double, float>(nullptr, di, nitems, wgs); }
    else { if (ptype_in == 0) launch_path_apply<float, double>(nullptr, di, nitems, wgs); else launch_path_apply<double, double>(nullptr, di, nitems, wgs); }
    HIPCHK(hipDeviceSynchronize());
    gO.down(L_out, "L_out");
}
// the pending real scale factor of site v (State::sscale): 1 when none is pending
double dbg_pending_scale(State* s, int v) {
    if (v < 0 || v >= s->g->nv) throw Err(TNQS_ERR_INVALID, "dbg_pending_scale: bad vertex");
    if (!s->sscale[v]) return 1.0;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipStreamSynchronize(s->stream));
    double f = 1.0; HIPCHK(hipMemcpy(&f, s->sscale[v]->p, 8, hipMemcpyDeviceToHost));
    return f;
}
// ---- the gate path's per-gate small algebra (kernels_theta.hip and the small_svd_* kernels of kernels_svd.hip): ONE launch of every kernel over nitems gates / sites of
// different sizes.  The route rule, the launch chain and the item fills are the engine's own (gate_theta.cpp: theta_route, launch_theta_chain, small_svd_items /
// launch_small_svd, Qr2Site); what is written here is where the arrays live.  Inputs: the items' arrays one after the other, every sub-array at a multiple of 256 bytes on
// the device.  Outputs: guard bands as above.  The small integer arrays (info, texp, failure flags, ranks) are contiguous per launch as in the engine's read-back buffer:
// they go up as filled and come back ----
namespace {
struct GateDims : ThetaRoute { int d1, d2, chi; };
// item i as the engine sees it: dimensions, the refusal of d^2 chi > 512, cap, and -- given the gate's kappa -- the route
GateDims gate_dims(const char* who, bool F32, const int* dims, int i, int kappa = 0, int maxdim = 0) {
    GateDims g; g.d1 = dims[3 * i]; g.d2 = dims[3 * i + 1]; g.chi = dims[3 * i + 2];
    if (g.d1 < 1 || g.d2 < 1 || g.chi < 1) throw Err(TNQS_ERR_INVALID, std::string(who) + ": d1, d2, chi >= 1");
    static_cast<ThetaRoute&>(g) = theta_route(F32, g.d1, g.d2, g.chi, kappa, maxdim);
    return g;
}
void up_ints(DBuf& d, const int* h, size_t n) { d.up(h, sizeof(int) * n); }
const void* upload_dbuf(void* keep, const void* p, size_t bytes) {      // DescUpload into a plain device allocation that lives as long as `keep`
    auto& k = *static_cast<std::vector<std::unique_ptr<DBuf>>*>(keep);
    k.emplace_back(new DBuf(bytes)); k.back()->up(p, bytes); return k.back()->p;
}
}
// HOST ONLY: the operator-sum factors of a two-site gate as gate_items() gets them
int dbg_operator_sum(const void* gate, int d1, int d2, void* fa_out, void* fb_out) {
    if (!gate || d1 < 1 || d2 < 1 || d1 > 16 || d2 > 16) throw Err(TNQS_ERR_INVALID, "dbg_operator_sum: bad arguments");
    std::vector<std::complex<double>> fa, fb;
    const int kappa = operator_sum(reinterpret_cast<const double*>(gate), d1, d2, fa, fb);
    if (fa_out && !fa.empty()) std::memcpy(fa_out, fa.data(), fa.size() * 16);
    if (fb_out && !fb.empty()) std::memcpy(fb_out, fb.data(), fb.size() * 16);
    return kappa;
}
// TwoSiteBatch::run_theta's launch_theta_chain up to stage stop_after.  info == NULL: only low_sizes is filled (host only)
void dbg_gate_theta(int dtype, int nitems, const int* dims, const int* mode, const int* rk, const void* F1, const void* F2, const double* tau, const void* gate,
                    const int* maxdim, int lowrank_on, int stop_after, int* low_sizes, int* info, double* lam1, double* lam2, int* idx1, int* idx2,
                    void* theta, void* theta0, void* thetaV, void* lowA, void* lowB, void* lowG, void* lowL, void* lowQ, void* lowL2c, int* texp, int* lowfail, int guard) {
    if ((dtype != TNQS_C64 && dtype != TNQS_C128) || nitems < 1 || !dims || !mode || !rk || !F1 || !F2 || !tau || !gate || !maxdim || !low_sizes || stop_after < 0 || stop_after > 3 || guard < 0)
        throw Err(TNQS_ERR_INVALID, "dbg_gate_theta: bad arguments");
    const bool F32 = dtype == TNQS_C64; const size_t esz = F32 ? 8 : 16;
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
    Slots sF1, sF2, sGate, sOp, sRk, sW, sB1, sG2;
    Guarded gLam1((size_t)guard * 8), gLam2((size_t)guard * 8), gIdx1((size_t)guard * 4), gIdx2((size_t)guard * 4), gTh(guard * esz), gTh0(guard * esz), gTv(guard * esz),
            gA((size_t)guard * 16), gB((size_t)guard * 16), gG((size_t)guard * 16), gL((size_t)guard * 16), gQ((size_t)guard * 16), gL2c((size_t)guard * 16);
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
    for (Slots* s : {&sF1, &sF2, &sGate, &sOp, &sRk, &sW, &sB1, &sG2}) s->alloc();
    for (Guarded* g : {&gLam1, &gLam2, &gIdx1, &gIdx2, &gTh, &gTh0, &gTv, &gA, &gB, &gG, &gL, &gQ, &gL2c}) g->alloc();
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
    DBuf dI(sizeof(GateItem) * nitems); dI.up(gitems.data(), sizeof(GateItem) * nitems);
    for (Slots* s : {&sF1, &sF2, &sGate, &sOp, &sRk, &sW, &sB1, &sG2}) s->up();
    gLam1.up(lam1); gLam2.up(lam2); gIdx1.up(idx1); gIdx2.up(idx2); gTh.up(theta); gTh0.up(theta0); gTv.up(thetaV);
    gA.up(lowA); gB.up(lowB); gG.up(lowG); gL.up(lowL); gQ.up(lowQ); gL2c.up(lowL2c);
    std::vector<std::unique_ptr<DBuf>> keep;
    const DescUpload up{upload_dbuf, &keep};
    if (F32) launch_theta_chain<float>(nullptr, (const GateItem*)dI.p, gitems, lows, (int*)dFail.p, (int*)dFail.p + nitems, up, stop_after);
    else launch_theta_chain<double>(nullptr, (const GateItem*)dI.p, gitems, lows, (int*)dFail.p, (int*)dFail.p + nitems, up, stop_after);
    HIPCHK(hipDeviceSynchronize());
    sW.down("lowW"); sB1.down("lowB1"); sG2.down("lowG2");
    gLam1.down(lam1, "lam1"); gLam2.down(lam2, "lam2"); gIdx1.down(idx1, "idx1"); gIdx2.down(idx2, "idx2"); gTh.down(theta, "theta"); gTh0.down(theta0, "theta0"); gTv.down(thetaV, "thetaV");
    gA.down(lowA, "lowA"); gB.down(lowB, "lowB"); gG.down(lowG, "lowG"); gL.down(lowL, "lowL"); gQ.down(lowQ, "lowQ"); gL2c.down(lowL2c, "lowL2c");
    dInfo.down(info, 32 * (size_t)nitems); dTexp.down(texp, 4 * (size_t)nitems);
    std::vector<int> hf(2 * (size_t)nitems); dFail.down(hf.data(), 8 * (size_t)nitems);
    for (int i = 0; i < nitems; ++i) { lowfail[2 * i] = hf[i]; lowfail[2 * i + 1] = hf[nitems + i]; }
}
// gate_finish_kernel<T> alone, on what the SVD stage leaves: theta_i (ld x ncol rotated columns, ld = max, ncol = min of (r1 d1, r2 d2)), thetaV_i (ncol x ncol)
void dbg_gate_finish(int dtype, int nitems, const int* dims, const int* info_in, const int* texp, const void* theta, const void* thetaV, const double* lam1, const double* lam2,
                     const int* idx1, const int* idx2, const void* GW1, const void* GW2, const int* maxdim, const double* cutoff, const int* normalize, const int* chi_cap,
                     double* S, int* info_out, double* truncerr, void* X1, void* X2, int guard) {
    if ((dtype != TNQS_C64 && dtype != TNQS_C128) || nitems < 1 || !dims || !info_in || !texp || !theta || !thetaV || !lam1 || !lam2 || !idx1 || !idx2 || !GW1 || !GW2 || !maxdim || !cutoff ||
        !normalize || !chi_cap || !S || !info_out || !truncerr || !X1 || !X2 || guard < 0) throw Err(TNQS_ERR_INVALID, "dbg_gate_finish: bad arguments");
    const bool F32 = dtype == TNQS_C64; const size_t esz = F32 ? 8 : 16;
    std::vector<GateDims> gd(nitems);
    Slots sTh, sTv, sLam1, sLam2, sIdx1, sIdx2, sW1, sW2; Guarded gS((size_t)guard * 8), gX1(guard * esz), gX2(guard * esz);
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
    for (Slots* s : {&sTh, &sTv, &sLam1, &sLam2, &sIdx1, &sIdx2, &sW1, &sW2}) s->alloc();
    gS.alloc(); gX1.alloc(); gX2.alloc();
    put_all(sTh, theta); put_all(sTv, thetaV); put_all(sLam1, lam1); put_all(sLam2, lam2); put_all(sIdx1, idx1); put_all(sIdx2, idx2); put_all(sW1, GW1); put_all(sW2, GW2);
    std::vector<int> hinfo(8 * (size_t)nitems, 0);
    for (int i = 0; i < nitems; ++i) { hinfo[8 * i] = info_in[4 * i]; hinfo[8 * i + 1] = info_in[4 * i + 1]; hinfo[8 * i + 5] = info_in[4 * i + 2] ? 1 : 0; hinfo[8 * i + 7] = info_in[4 * i + 3];
                                       hinfo[8 * i + 2] = info_out[2 * i]; hinfo[8 * i + 3] = info_out[2 * i + 1]; }
    DBuf dInfo(32 * (size_t)nitems), dTexp(4 * (size_t)nitems), dTerr(8 * (size_t)nitems), dI(sizeof(GateItem) * nitems);
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
    dI.up(gitems.data(), sizeof(GateItem) * nitems);
    for (Slots* s : {&sTh, &sTv, &sLam1, &sLam2, &sIdx1, &sIdx2, &sW1, &sW2}) s->up();
    gS.up(S); gX1.up(X1); gX2.up(X2);
    if (F32) launch_gate_finish<float>(nullptr, (const GateItem*)dI.p, nitems); else launch_gate_finish<double>(nullptr, (const GateItem*)dI.p, nitems);
    HIPCHK(hipDeviceSynchronize());
    gS.down(S, "S"); gX1.down(X1, "X1"); gX2.down(X2, "X2");
    dInfo.down(hinfo.data(), 32 * (size_t)nitems); dTerr.down(truncerr, 8 * (size_t)nitems);
    for (int i = 0; i < nitems; ++i) { info_out[2 * i] = hinfo[8 * i + 2]; info_out[2 * i + 1] = hinfo[8 * i + 3]; }
}
// TwoSiteBatch::svd_and_finish up to and including the recovery of V: launch_theta_svd_stage (gate_svd.cpp) once over nitems gates.  dims: (d1, d2, n1, n2) per item, the
// bounds n_s = d_s chi every buffer and (dyn) every launch is sized from; info: the 8 ints per item the device holds (r1, r2, -, -, -, -, -, K alive), which are also the host
// dims of the static regime.  theta == NULL: only route_out is filled (host only)
void dbg_theta_svd_stage(int dtype, int dyn, int nitems, const int* dims, const int* info, const int* K, const int* has_q, const void* Q, const int* rank_bounds, const int* cap,
                         int recover_form, void* theta, void* theta0, void* thetaV, int* sweeps_out, int* route_out, int guard) {
    if ((dtype != TNQS_C64 && dtype != TNQS_C128) || dyn < 0 || dyn > 1 || nitems < 1 || !dims || !info || !K || !has_q || !rank_bounds || !cap || recover_form < 0 || recover_form > 1 ||
        guard < 0 || (theta && (!theta0 || !thetaV))) throw Err(TNQS_ERR_INVALID, "dbg_theta_svd_stage: bad arguments");
    static_assert(ThetaSvdPreLow == TNQS_DBG_ROUTE_SVD_PRE_LOWRANK && ThetaSvdPreTheta == TNQS_DBG_ROUTE_SVD_PRE_THETA && ThetaSvdLds == TNQS_DBG_ROUTE_SVD_LDS &&
                  ThetaSvdGlobal == TNQS_DBG_ROUTE_SVD_GLOBAL && ThetaSvdTall == TNQS_DBG_ROUTE_SVD_TALL, "theta_svd_route returns the header's values");
    const bool F32 = dtype == TNQS_C64; const size_t esz = F32 ? 8 : 16;
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
        Slots sQ; Guarded gTh(guard * esz), gTh0(guard * esz), gTv(guard * esz);
        for (int i = 0; i < nitems; ++i) {
            const size_t mx = (size_t)MrB[i];
            gTh.add((size_t)MrB[i] * NcB[i] * esz); gTh0.add((size_t)MrB[i] * NcB[i] * esz); gTv.add(mx * mx * esz);
            sQ.add(has_q[i] ? (size_t)NcB[i] * K[i] * 16 : 0);
        }
        sQ.alloc(); gTh.alloc(); gTh0.alloc(); gTv.alloc();
        { const char* p = (const char*)Q; for (int i = 0; i < nitems; ++i) if (has_q[i]) { sQ.put(i, p); p += sQ.len[i]; } }
        DBuf dInfo(32 * (size_t)nitems); up_ints(dInfo, info, 8 * (size_t)nitems);
        for (int i = 0; i < nitems; ++i) {
            sg[i].theta = gTh.at(i); sg[i].theta0 = gTh0.at(i); sg[i].thetaV = gTv.at(i); sg[i].info = (int*)dInfo.p + 8 * i;
            sg[i].lowQ = has_q[i] ? sQ.at(i) : nullptr;
        }
        sQ.up(); gTh.up(theta); gTh0.up(theta0); gTv.up(thetaV);
        const bool mfma = recover_form == 0 && F32 && use_mfma();      // 0: the engine's rule
        if (F32) launch_theta_svd_stage<float>(s.get(), sg, dyn ? nullptr : info, mfma); else launch_theta_svd_stage<double>(s.get(), sg, dyn ? nullptr : info, mfma);
        HIPCHK(hipStreamSynchronize(s->stream));
        sQ.down("Q"); gTh.down(theta, "theta"); gTh0.down(theta0, "theta0"); gTv.down(thetaV, "thetaV");
        if (sweeps_out) { std::vector<int> h(8 * (size_t)nitems); dInfo.down(h.data(), 32 * (size_t)nitems); for (int i = 0; i < nitems; ++i) sweeps_out[i] = h[8 * i + 4]; }
    }
}
// qr2_rinv_kernel (stage 0: X1 only), then qr2_compose_kernel (stage 1), as second_pass() runs them.  n x n complex128 matrices per item
void dbg_qr2(int stage, int nitems, const int* n, const void* GW, const void* GV, const double* lam, const int* idx, const int* r, const void* A2, const void* V2, const double* tau,
             void* X1, void* GVout, void* GWout, int* rk, int guard) {
    if (stage < 0 || stage > 1 || nitems < 1 || !n || !GW || !lam || !idx || !r || !X1 || guard < 0 || (stage == 1 && (!GV || !A2 || !V2 || !tau || !GVout || !GWout || !rk)))
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
    Slots sW, sV, sLam, sIdx, sA2, sV2; Guarded gX((size_t)guard * 16), gGV((size_t)guard * 16), gGW((size_t)guard * 16);
    for (int i = 0; i < nitems; ++i) {
        const size_t nn = (size_t)n[i] * n[i] * 16;
        sW.add(nn); sV.add(nn); sA2.add(nn); sV2.add(nn); sLam.add((size_t)n[i] * 8); sIdx.add((size_t)n[i] * 4); gX.add(nn); gGV.add(stage ? nn : 0); gGW.add(stage ? nn : 0);
    }
    for (Slots* s : {&sW, &sV, &sLam, &sIdx, &sA2, &sV2}) s->alloc();
    gX.alloc(); gGV.alloc(); gGW.alloc();
    put_all(sW, GW); put_all(sLam, lam); put_all(sIdx, idx);
    if (stage) { put_all(sV, GV); put_all(sA2, A2); put_all(sV2, V2); }
    DBuf dR(4 * (size_t)nitems), dRk(4 * (size_t)nitems); up_ints(dR, r, nitems); if (stage) up_ints(dRk, rk, nitems);
    std::vector<Qr2RinvItem> ri(nitems); std::vector<Qr2ComposeItem> ci(nitems);
    for (int i = 0; i < nitems; ++i) {
        const Qr2Site q{sW.at(i), sV.at(i), (const double*)sLam.at(i), (const int*)sIdx.at(i), (const int*)dR.p + i, n[i], gX.at(i)};
        ri[i] = q.rinv();
        ci[i] = q.compose(sA2.at(i), sV2.at(i), stage ? tau[i] : 0.0, gGV.at(i), gGW.at(i), (int*)dRk.p + i);
    }
    DBuf dRi(sizeof(Qr2RinvItem) * nitems), dCi(sizeof(Qr2ComposeItem) * nitems);
    dRi.up(ri.data(), sizeof(Qr2RinvItem) * nitems); dCi.up(ci.data(), sizeof(Qr2ComposeItem) * nitems);
    for (Slots* s : {&sW, &sV, &sLam, &sIdx, &sA2, &sV2}) s->up();
    gX.up(X1); if (stage) { gGV.up(GVout); gGW.up(GWout); }
    launch_qr2_rinv(nullptr, (const Qr2RinvItem*)dRi.p, nitems);
    if (stage) launch_qr2_compose(nullptr, (const Qr2ComposeItem*)dCi.p, nitems);
    HIPCHK(hipDeviceSynchronize());
    gX.down(X1, "X1");
    if (stage) { gGV.down(GVout, "GVout"); gGW.down(GWout, "GWout"); dRk.down(rk, 4 * (size_t)nitems); }
}
// small_svd_prepare_kernel<T> -> launch_jacobi<double> -> small_svd_finish_kernel on site tensors [d][low][chi_b][hi] (shape: 4 ints per item) with low * hi < d * chi_b
void dbg_small_svd(int dtype, int nitems, const int* shape, const void* src, void* GA, void* GV, int guard) {
    if ((dtype != TNQS_C64 && dtype != TNQS_C128) || nitems < 1 || !shape || !src || !GA || !GV || guard < 0) throw Err(TNQS_ERR_INVALID, "dbg_small_svd: bad arguments");
    const size_t esz = dtype == TNQS_C64 ? 8 : 16;
    Slots sSrc, sM; Guarded gA((size_t)guard * 16), gV((size_t)guard * 16);
    for (int i = 0; i < nitems; ++i) {
        const int d = shape[4 * i], lo = shape[4 * i + 1], cb = shape[4 * i + 2], hi = shape[4 * i + 3];
        if (d < 1 || lo < 1 || cb < 1 || hi < 1) throw Err(TNQS_ERR_INVALID, "dbg_small_svd: dimensions >= 1");
        const long long n = (long long)d * cb, N = (long long)lo * hi;
        if (!(N < n && n <= 256)) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_small_svd: the small-SVD route takes sites with fewer fibers than columns (low*hi < d*chi_b <= 256)");
        sSrc.add((size_t)(n * N) * esz); sM.add((size_t)(n * N) * 16); gA.add((size_t)(n * n) * 16); gV.add((size_t)(n * n) * 16);
    }
    need_gpu();
    sSrc.alloc(); sM.alloc(); gA.alloc(); gV.alloc();
    put_all(sSrc, src);
    std::vector<SmallSvdItem> si; std::vector<JacobiItem> sji;
    for (int i = 0; i < nitems; ++i) {
        const int d = shape[4 * i], lo = shape[4 * i + 1], cb = shape[4 * i + 2], hi = shape[4 * i + 3];
        small_svd_items(sSrc.at(i), sM.at(i), gA.at(i), gV.at(i), d, lo, cb, hi, si, sji);
    }
    DBuf dS(sizeof(SmallSvdItem) * nitems), dJ(sizeof(JacobiItem) * nitems);
    dS.up(si.data(), sizeof(SmallSvdItem) * nitems); dJ.up(sji.data(), sizeof(JacobiItem) * nitems);
    sSrc.up(); sM.up(); gA.up(GA); gV.up(GV);
    const SmallSvdItem* ds = (const SmallSvdItem*)dS.p; const JacobiItem* dj = (const JacobiItem*)dJ.p;
    if (dtype == TNQS_C64) launch_small_svd<float>(nullptr, ds, dj, sji); else launch_small_svd<double>(nullptr, ds, dj, sji);
    HIPCHK(hipDeviceSynchronize());
    sM.down("M"); gA.down(GA, "GA"); gV.down(GV, "GV");
}

// ---- overlap of two states (kernels_inner.hip), the descriptors filled as engine_inner.cpp run_batch fills them -----------------------------------------------
// ONE launch_inner_gram<T> over nitems items (PA, Ka, Kb, PB), then launch_inner_finalize<T> with normalize = 0 as the chunk sum
void dbg_inner_gram(int dtype, int nitems, const int* shape, const void* X, const void* Y, void* out, int max_chunks, int* nchunks_out, int guard, int* route) {
    if ((dtype != TNQS_C64 && dtype != TNQS_C128) || nitems < 1 || !shape || !X || !out || guard < 0) throw Err(TNQS_ERR_INVALID, "dbg_inner_gram: bad arguments");
    const size_t esz = dtype == TNQS_C64 ? 8 : 16;
    Slots sX, sY, sP; Guarded gO((size_t)guard * esz);
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
    sX.alloc(); if (Y) sY.alloc(); sP.alloc(); gO.alloc();
    put_all(sX, X); if (Y) put_all(sY, Y);
    std::vector<InnerFinalItem> fi(nitems);
    for (int i = 0; i < nitems; ++i) {
        gi[i].X = sX.at(i); gi[i].Y = Y ? sY.at(i) : sX.at(i); gi[i].partial = sP.at(i);
        fi[i] = InnerFinalItem{sP.at(i), npart[i], gi[i].Ka, gi[i].Kb, nullptr, gO.at(i), nullptr, nullptr, 0};
    }
    DBuf dG(sizeof(InnerGramItem) * nitems), dF(sizeof(InnerFinalItem) * nitems);
    dG.up(gi.data(), sizeof(InnerGramItem) * nitems); dF.up(fi.data(), sizeof(InnerFinalItem) * nitems);
    sX.up(); if (Y) sY.up(); sP.up(); gO.up(out);
    if (dtype == TNQS_C64) { launch_inner_gram<float>(nullptr, (const InnerGramItem*)dG.p, nitems, chunks); launch_inner_finalize<float>(nullptr, (const InnerFinalItem*)dF.p, nitems); }
    else { launch_inner_gram<double>(nullptr, (const InnerGramItem*)dG.p, nitems, chunks); launch_inner_finalize<double>(nullptr, (const InnerFinalItem*)dF.p, nitems); }
    HIPCHK(hipDeviceSynchronize());
    sP.down("the Gram partials"); gO.down(out, "out");
    if (nchunks_out) std::copy(npart.begin(), npart.end(), nchunks_out);
    if (route) *route = TNQS_DBG_ROUTE_INNER_MFMA;
}
// ONE launch_inner_finalize<T> over nitems messages of rows[i] x cols[i]
void dbg_inner_finalize(int dtype, int nitems, const int* rows, const int* cols, const int* nchunks, const void* partials, const void* old_msg, const int* has_old,
                        const int* normalize, void* new_msg, double* diff, double* sum, int guard) {
    if ((dtype != TNQS_C64 && dtype != TNQS_C128) || nitems < 1 || !rows || !cols || !nchunks || !partials || !normalize || !new_msg || (old_msg && !has_old) || guard < 0)
        throw Err(TNQS_ERR_INVALID, "dbg_inner_finalize: bad arguments");
    const size_t esz = dtype == TNQS_C64 ? 8 : 16;
    Slots sP, sOld; Guarded gN((size_t)guard * esz);
    for (int i = 0; i < nitems; ++i) {
        if (rows[i] < 1 || cols[i] < 1 || nchunks[i] < 1) throw Err(TNQS_ERR_INVALID, "dbg_inner_finalize: rows, cols, nchunks >= 1");
        if (!inner_gram_covers(rows[i], cols[i])) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_inner_finalize: rows, cols <= 64");
        const size_t mb = (size_t)rows[i] * cols[i] * esz;
        sP.add(mb * nchunks[i]); sOld.add(mb); gN.add(mb);
    }
    need_gpu();
    sP.alloc(); sOld.alloc(); gN.alloc();
    put_all(sP, partials);
    DBuf dD(sizeof(double) * nitems), dS(sizeof(double) * 2 * nitems), dF(sizeof(InnerFinalItem) * nitems);
    std::vector<InnerFinalItem> fi(nitems);
    size_t om = 0;
    for (int i = 0; i < nitems; ++i) {
        const bool old = old_msg && has_old[i]; if (old) sOld.put(i, (const char*)old_msg + om);
        om += sOld.len[i];
        fi[i] = InnerFinalItem{sP.at(i), nchunks[i], rows[i], cols[i], old ? sOld.at(i) : nullptr, gN.at(i), diff ? (double*)dD.p + i : nullptr, sum ? (double*)dS.p + 2 * i : nullptr, normalize[i]};
    }
    sP.up(); sOld.up(); gN.up(new_msg); dF.up(fi.data(), sizeof(InnerFinalItem) * nitems);
    if (dtype == TNQS_C64) launch_inner_finalize<float>(nullptr, (const InnerFinalItem*)dF.p, nitems); else launch_inner_finalize<double>(nullptr, (const InnerFinalItem*)dF.p, nitems);
    HIPCHK(hipDeviceSynchronize());
    gN.down(new_msg, "new_msg");
    if (diff) dD.down(diff, sizeof(double) * nitems);
    if (sum) dS.down(sum, sizeof(double) * 2 * nitems);
}
// ONE launch_inner_scalar<T> over nitems vertex / edge scalars, the descriptors filled as engine_inner.cpp (inner_bp) fills them: present[2 i], [2 i + 1]: m_i, mr_i
// (0: a null pointer = the rectangular delta); has_rawsum[i], has_scale[2 i], [2 i + 1]: 0 hands the kernel a null pointer
void dbg_inner_scalar(int dtype, int nitems, const int* rows, const int* cols, const void* m, const void* mr, const int* present, const double* rawsum, const int* has_rawsum,
                      const int* normalize, const double* scale_a, const double* scale_b, const int* has_scale, double* out, int guard) {
    if ((dtype != TNQS_C64 && dtype != TNQS_C128) || nitems < 1 || !rows || !cols || !m || !mr || !present || !rawsum || !has_rawsum || !normalize || !scale_a || !scale_b ||
        !has_scale || !out || guard < 0)
        throw Err(TNQS_ERR_INVALID, "dbg_inner_scalar: bad arguments");
    const size_t esz = dtype == TNQS_C64 ? 8 : 16;
    Slots sM, sR, sSum, sSc; Guarded gO((size_t)guard * 16);
    for (int i = 0; i < nitems; ++i) {
        if (rows[i] < 1 || cols[i] < 1) throw Err(TNQS_ERR_INVALID, "dbg_inner_scalar: rows, cols >= 1");
        if (!inner_gram_covers(rows[i], cols[i])) throw Err(TNQS_ERR_UNSUPPORTED, "dbg_inner_scalar: rows, cols <= 64");
        const size_t mb = (size_t)rows[i] * cols[i] * esz;
        sM.add(mb); sR.add(mb); sSum.add(16); sSc.add(8); sSc.add(8); gO.add(16);
    }
    need_gpu();
    sM.alloc(); sR.alloc(); sSum.alloc(); sSc.alloc(); gO.alloc();
    put_all(sM, m); put_all(sR, mr); put_all(sSum, rawsum);
    std::vector<InnerScalarItem> si(nitems);
    for (int i = 0; i < nitems; ++i) {
        sSc.put(2 * i, scale_a + i); sSc.put(2 * i + 1, scale_b + i);
        si[i] = InnerScalarItem{present[2 * i] ? sM.at(i) : nullptr, present[2 * i + 1] ? sR.at(i) : nullptr, rows[i], cols[i], has_rawsum[i] ? (const double*)sSum.at(i) : nullptr,
                                normalize[i], has_scale[2 * i] ? (const double*)sSc.at(2 * i) : nullptr, has_scale[2 * i + 1] ? (const double*)sSc.at(2 * i + 1) : nullptr, (double*)gO.at(i)};
    }
    DBuf dI(sizeof(InnerScalarItem) * nitems);
    sM.up(); sR.up(); sSum.up(); sSc.up(); gO.up(out); dI.up(si.data(), sizeof(InnerScalarItem) * nitems);
    if (dtype == TNQS_C64) launch_inner_scalar<float>(nullptr, (const InnerScalarItem*)dI.p, nitems); else launch_inner_scalar<double>(nullptr, (const InnerScalarItem*)dI.p, nitems);
    HIPCHK(hipDeviceSynchronize());
    gO.down(out, "out");
}

// ---- sampling (kernels_sample.hip), launched as engine_sample.cpp launches them ------------------------------------------------------------------------------------
// site_prob_partial_kernel<T> on one site tensor of n = d k elements: the raw nblocks x 16 partial array between guard bands of `guard` doubles.  nblocks == 0: the
// engine's plan_site_prob.  partial == NULL: only *nblocks_out is filled (HOST ONLY)
void dbg_site_prob(int dtype, int n, int d, const void* tabs, const void* psi, int nblocks, double* partial, int guard, int* nblocks_out) {
    if ((dtype != TNQS_C64 && dtype != TNQS_C128) || n < 1 || d < 1 || d > 16 || n % d || nblocks < 0 || nblocks > 4096 || guard < 0 || (partial && (!tabs || !psi)))
        throw Err(TNQS_ERR_INVALID, "dbg_site_prob: bad arguments");
    const int nb = nblocks ? nblocks : plan_site_prob((size_t)n, d);
    if (nblocks_out) *nblocks_out = nb;
    if (!partial) return;
    need_gpu();
    const size_t esz = dtype == TNQS_C64 ? 8 : 16;
    Slots sT, sP; Guarded gP((size_t)guard * 8);
    sT.add((size_t)n * esz); sP.add((size_t)n * esz); gP.add((size_t)nb * 16 * 8);
    sT.alloc(); sP.alloc(); gP.alloc();
    sT.put(0, tabs); sP.put(0, psi);
    sT.up(); sP.up(); gP.up(partial);
    if (dtype == TNQS_C64) launch_site_prob_partial<float>(nullptr, sT.at(0), sP.at(0), (size_t)n, d, nb, (double*)gP.at(0));
    else launch_site_prob_partial<double>(nullptr, sT.at(0), sP.at(0), (size_t)n, d, nb, (double*)gP.at(0));
    HIPCHK(hipDeviceSynchronize());
    gP.down(partial, "partial");
}
// site_draw_kernel, one launch per item (the engine launches one per step): partials: nblocks[i] x 16 doubles per item, one item after the other; use_counter[i] == 0: the
// uniform is uniform[i], else counter-based from counter[3 i .. 3 i + 2] = (seed, sample, step) and the kernel gets a null uniform.  p_out: 16 doubles per item (the kernel
// writes d[i]), x_out, px_out: one number per item, all three between guard bands of `guard` elements; status_out[i]: the item's own status word, cleared before its launch
void dbg_site_draw(int nitems, const int* nblocks, const int* d, const double* partials, const double* neg_tol, const double* uniform, const int* use_counter,
                   const unsigned long long* counter, const int* draw, double* p_out, int* x_out, double* px_out, int* status_out, int guard) {
    if (nitems < 1 || !nblocks || !d || !partials || !neg_tol || !uniform || !use_counter || !counter || !draw || !p_out || !x_out || !px_out || !status_out || guard < 0)
        throw Err(TNQS_ERR_INVALID, "dbg_site_draw: bad arguments");
    Slots sPart, sU; Guarded gP((size_t)guard * 8), gX((size_t)guard * 4), gPx((size_t)guard * 8);
    for (int i = 0; i < nitems; ++i) {
        if (nblocks[i] < 1 || d[i] < 1 || d[i] > 16) throw Err(TNQS_ERR_INVALID, "dbg_site_draw: nblocks >= 1, 1 <= d <= 16");
        sPart.add((size_t)nblocks[i] * 16 * 8); sU.add(8); gP.add(16 * 8); gX.add(4); gPx.add(8);
    }
    need_gpu();
    sPart.alloc(); sU.alloc(); gP.alloc(); gX.alloc(); gPx.alloc();
    put_all(sPart, partials); put_all(sU, uniform);
    DBuf dSt(sizeof(int) * nitems);
    HIPCHK(hipMemset(dSt.p, 0, sizeof(int) * nitems));
    sPart.up(); sU.up(); gP.up(p_out); gX.up(x_out); gPx.up(px_out);
    for (int i = 0; i < nitems; ++i)
        launch_site_draw(nullptr, (const double*)sPart.at(i), nblocks[i], d[i], neg_tol[i], use_counter[i] ? nullptr : (const double*)sU.at(i), counter[3 * i], counter[3 * i + 1],
                         counter[3 * i + 2], draw[i] != 0, (double*)gP.at(i), (int*)gX.at(i), (double*)gPx.at(i), (int*)dSt.p + i);
    HIPCHK(hipDeviceSynchronize());
    gP.down(p_out, "p_out"); gX.down(x_out, "x_out"); gPx.down(px_out, "px_out");
    dSt.down(status_out, sizeof(int) * nitems);
}
// site_project_kernel<T>: out[i] = psi[x + d i], i < nout; x_on_device != 0: x goes through device memory and the host argument is one that clamps to another index
void dbg_site_project(int dtype, int nout, int d, const void* psi, int x, int x_on_device, void* out, int guard) {
    if ((dtype != TNQS_C64 && dtype != TNQS_C128) || nout < 1 || d < 1 || d > 16 || (long long)nout * d > INT_MAX / 2 || !psi || !out || guard < 0)
        throw Err(TNQS_ERR_INVALID, "dbg_site_project: bad arguments");
    need_gpu();
    const size_t esz = dtype == TNQS_C64 ? 8 : 16;
    Slots sP, sX; Guarded gO((size_t)guard * esz);
    sP.add((size_t)nout * d * esz); sX.add(4); gO.add((size_t)nout * esz);
    sP.alloc(); sX.alloc(); gO.alloc();
    sP.put(0, psi); sX.put(0, &x);
    sP.up(); sX.up(); gO.up(out);
    const int* dx = x_on_device ? (const int*)sX.at(0) : nullptr;
    const int xh = x_on_device ? (x <= 0 ? INT_MAX : -1) : x;
    if (dtype == TNQS_C64) launch_site_project<float>(nullptr, sP.at(0), gO.at(0), (size_t)nout, d, dx, xh); else launch_site_project<double>(nullptr, sP.at(0), gO.at(0), (size_t)nout, d, dx, xh);
    HIPCHK(hipDeviceSynchronize());
    gO.down(out, "out");
}

// ---- the ComplexF32 d = 2 one-site gate with normalisation (kernels_util.hip), set up as apply_one_site_batch / norm_and_replace / materialize_scale set it up ----------
// ONE launch_site1_c64 over nitems tensors of npairs[i] (s = 0, 1) pairs; gates: 8 doubles per item, column-major G[s' + 2 s] re/im as the C ABI takes them, packed by
// pack_site1_gate.  normalize != 0: the kernel leaves nbx norm partials per item in `partials` (nitems nbx doubles between two guard bands) and ONE launch_norm_factor
// turns them into `factors` (one double per item between guard bands, 256-byte slots on the device); normalize == 0: the kernel gets a null pointer, both stay as they were
void dbg_site1(int nitems, const int* npairs, const void* in, const double* gates, int nbx, int normalize, void* out, double* partials, double* factors, int guard) {
    if (nitems < 1 || !npairs || !in || !gates || nbx < 1 || nbx > 65535 || !out || !partials || !factors || guard < 0) throw Err(TNQS_ERR_INVALID, "dbg_site1: bad arguments");
    Slots sIn; Guarded gO((size_t)guard * 8), gPart((size_t)guard * 8), gF((size_t)guard * 8);
    for (int i = 0; i < nitems; ++i) {
        if (npairs[i] < 1) throw Err(TNQS_ERR_INVALID, "dbg_site1: npairs >= 1");
        sIn.add((size_t)npairs[i] * 16); gO.add((size_t)npairs[i] * 16); gF.add(8);
    }
    gPart.add((size_t)nitems * nbx * 8);
    need_gpu();
    sIn.alloc(); gO.alloc(); gPart.alloc(); gF.alloc();
    put_all(sIn, in);
    std::vector<Site1Item> items(nitems); std::vector<NormFactorItem> nf(nitems);
    for (int i = 0; i < nitems; ++i) {
        Site1Item it{}; it.in = sIn.at(i); it.out = gO.at(i); it.npairs = (size_t)npairs[i];
        pack_site1_gate(gates + 8 * (size_t)i, it.g);
        items[i] = it;
        nf[i] = NormFactorItem{(const double*)gPart.at(0) + (size_t)i * nbx, nbx, (double*)gF.at(i)};
    }
    DBuf dI(sizeof(Site1Item) * nitems), dN(sizeof(NormFactorItem) * nitems);
    sIn.up(); gO.up(out); gPart.up(partials); gF.up(factors);
    dI.up(items.data(), sizeof(Site1Item) * nitems); dN.up(nf.data(), sizeof(NormFactorItem) * nitems);
    launch_site1_c64(nullptr, (const Site1Item*)dI.p, nitems, nbx, normalize ? (double*)gPart.at(0) : nullptr);
    if (normalize) launch_norm_factor(nullptr, (const NormFactorItem*)dN.p, nitems);
    HIPCHK(hipDeviceSynchronize());
    gO.down(out, "out"); gPart.down(partials, "partials"); gF.down(factors, "factors");
}
// ONE launch_norm_factor: item i has npart[i] partials (one item after the other); factors: one double per item between guard bands
void dbg_norm_factor(int nitems, const int* npart, const double* partials, double* factors, int guard) {
    if (nitems < 1 || !npart || !partials || !factors || guard < 0) throw Err(TNQS_ERR_INVALID, "dbg_norm_factor: bad arguments");
    Slots sP; Guarded gF((size_t)guard * 8);
    for (int i = 0; i < nitems; ++i) { if (npart[i] < 0) throw Err(TNQS_ERR_INVALID, "dbg_norm_factor: npart >= 0"); sP.add((size_t)npart[i] * 8); gF.add(8); }
    need_gpu();
    sP.alloc(); gF.alloc();
    put_all(sP, partials);
    std::vector<NormFactorItem> nf(nitems);
    for (int i = 0; i < nitems; ++i) nf[i] = NormFactorItem{(const double*)sP.at(i), npart[i], (double*)gF.at(i)};
    DBuf dN(sizeof(NormFactorItem) * nitems);
    sP.up(); gF.up(factors); dN.up(nf.data(), sizeof(NormFactorItem) * nitems);
    launch_norm_factor(nullptr, (const NormFactorItem*)dN.p, nitems);
    HIPCHK(hipDeviceSynchronize());
    gF.down(factors, "factors");
}
// ONE launch_scale<T>: dst_i = src_i * (T)factor[i], len[i] numbers per item, the factor read from device memory as the pending scale factor is
void dbg_scale(int dtype, int nitems, const int* len, const void* src, const double* factor, void* dst, int guard) {
    if ((dtype != TNQS_C64 && dtype != TNQS_C128) || nitems < 1 || !len || !src || !factor || !dst || guard < 0) throw Err(TNQS_ERR_INVALID, "dbg_scale: bad arguments");
    const size_t esz = dtype == TNQS_C64 ? 8 : 16;
    Slots sS, sF; Guarded gD((size_t)guard * esz);
    for (int i = 0; i < nitems; ++i) { if (len[i] < 1) throw Err(TNQS_ERR_INVALID, "dbg_scale: len >= 1"); sS.add((size_t)len[i] * esz); sF.add(8); gD.add((size_t)len[i] * esz); }
    need_gpu();
    sS.alloc(); sF.alloc(); gD.alloc();
    put_all(sS, src); put_all(sF, factor);
    std::vector<ScaleItem> items(nitems);
    for (int i = 0; i < nitems; ++i) items[i] = ScaleItem{sS.at(i), gD.at(i), (size_t)len[i], (const double*)sF.at(i)};
    DBuf dI(sizeof(ScaleItem) * nitems);
    sS.up(); sF.up(); gD.up(dst); dI.up(items.data(), sizeof(ScaleItem) * nitems);
    if (dtype == TNQS_C64) launch_scale<float>(nullptr, (const ScaleItem*)dI.p, nitems); else launch_scale<double>(nullptr, (const ScaleItem*)dI.p, nitems);
    HIPCHK(hipDeviceSynchronize());
    gD.down(dst, "dst");
}
}  // namespace tnqs
