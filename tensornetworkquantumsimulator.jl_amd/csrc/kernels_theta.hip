// kernels_theta.hip -- per-gate small algebra of the two-site update: Gram eigenvalues to R factors, theta and its low-rank form, the second QR,
// truncation and the new site tensors.  (kernels_gate.hip holds the fused gauge and f64 Gram kernels.)
// Reference call sites replaced (paths relative to the reference repo):
//   gate_theta / gate_finish : simple_update.jl:51-59 + NDTensors truncate! rule, apply_gates.jl:126-135
#include "kernels.hpp"
#include "device_common.hpp"
#include "jacobi_common.hpp"

namespace tnqs {

// ------------------------------------------------------------------------------------------------------------
// per-gate small algebra.  With G_i = psi~_i^dagger psi~_i = W L W^dagger:  R_i = L^{1/2} W^dagger (any
// orthogonal factorisation psi~ = Q R gives the same gauge-invariant result as the reference's QR).
// ------------------------------------------------------------------------------------------------------------

__device__ void gate_eigs(const cx<double>* A, const cx<double>* V, int n, double* lam_tmp /*LDS n*/, double* lam_out,
                          int* idx_out, int* r_out, int* s_r /*LDS*/, double tau) {
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        double l = 0;
        for (int i = 0; i < n; ++i) { cx<double> v = V[i + n * j], a = A[i + n * j]; l += v.re * a.re + v.im * a.im; }
        lam_tmp[j] = l;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double lmax = 0;
        for (int j = 0; j < n; ++j) lmax = fmax(lmax, lam_tmp[j]);
        int r = 0;
        if (tau < 0) {       // shifted first pass (a second factorisation pass follows): nothing is dropped, l := max(l, 0) + |tau| l_max
            for (int j = 0; j < n; ++j) { lam_out[j] = fmax(lam_tmp[j], 0.0) - tau * lmax; idx_out[j] = j; }
            r = n;
        } else
        for (int j = 0; j < n; ++j)
            if (lam_tmp[j] > tau * lmax && lam_tmp[j] > 0) { lam_out[r] = lam_tmp[j]; idx_out[r] = j; ++r; }
        *r_out = r; *s_r = r;
    }
    __syncthreads();
}

// Cholesky site: R = L^dagger is read through the same (eigenvector, eigenvalue) interface with lambda = 1, all columns kept
__device__ void gate_full_rank(int n, double* lam_out, int* idx_out, int* r_out, int* s_r, const int* rk = nullptr) {
    for (int j = threadIdx.x; j < n; j += blockDim.x) { lam_out[j] = 1.0; idx_out[j] = j; }
    if (threadIdx.x == 0) { const int r = rk ? *rk : n; *r_out = r; *s_r = r; }
    __syncthreads();
}
// is the kept part of the factor ill-conditioned (smallest / largest squared singular value of psi~ below 1e-4: the f64 Gram route alone leaves a relative error eps / that ratio)?  Such ComplexF64
// sites get a second factorisation pass (engine.cpp).  Cholesky: from the pivots diag(L)^2; eigen: from the kept eigenvalues.
__device__ int gate_ill_conditioned(int chol, const cx<double>* L, int n, const double* lam, int r) {
    double lo = 1e300, hi = 0;
    if (chol) for (int j = 0; j < n; ++j) { double d = L[j + (size_t)n * j].re; d *= d; lo = fmin(lo, d); hi = fmax(hi, d); }
    else for (int j = 0; j < r; ++j) { lo = fmin(lo, lam[j]); hi = fmax(hi, lam[j]); }
    return (hi > 0 && lo < 1e-4 * hi) ? 1 : 0;
}

template <class T>
__global__ __launch_bounds__(1024) void gate_theta_kernel(const GateItem* __restrict__ items) {
    __shared__ double lam_tmp[512];
    __shared__ int s_r1, s_r2;
    // grid (gate, part): every part repeats the small serial prologue (identical values) and takes a strided share of the element loops --
    // with one workgroup per gate the kernel was pure latency (0.56 ms per colour batch whatever the batch size)
    const GateItem it = items[blockIdx.x];
    const int part = blockIdx.y, tid0 = part * blockDim.x + threadIdx.x, tstride = gridDim.y * blockDim.x;
    const cx<double>* A1 = reinterpret_cast<const cx<double>*>(it.GA1);
    const cx<double>* V1 = reinterpret_cast<const cx<double>*>(it.GV1);
    const cx<double>* A2 = reinterpret_cast<const cx<double>*>(it.GA2);
    const cx<double>* V2 = reinterpret_cast<const cx<double>*>(it.GV2);
    if (it.chol1) gate_full_rank(it.n1, it.lam1, it.idx1, &it.info[0], &s_r1, it.chol1 == 2 ? it.rk1 : nullptr); else gate_eigs(A1, V1, it.n1, lam_tmp, it.lam1, it.idx1, &it.info[0], &s_r1, it.tau1);
    if (it.chol2) gate_full_rank(it.n2, it.lam2, it.idx2, &it.info[1], &s_r2, it.chol2 == 2 ? it.rk2 : nullptr); else gate_eigs(A2, V2, it.n2, lam_tmp, it.lam2, it.idx2, &it.info[1], &s_r2, it.tau2);
    if (threadIdx.x == 0 && part == 0) {
        it.info[6] = (it.chol1 == 2 ? 0 : gate_ill_conditioned(it.chol1, V1, it.n1, it.lam1, s_r1))
                   | ((it.chol2 == 2 ? 0 : gate_ill_conditioned(it.chol2, V2, it.n2, it.lam2, s_r2)) << 1);
    }
    const int r1 = s_r1, r2 = s_r2, d1 = it.d1, d2 = it.d2, chi = it.chi;
    const int Mr = r1 * d1, Nc = r2 * d2;
    const bool wide = Mr < Nc;
    cx<T>* th = reinterpret_cast<cx<T>*>(it.theta);
    cx<T>* tv = reinterpret_cast<cx<T>*>(it.thetaV);
    const cx<double>* g = reinterpret_cast<const cx<double>*>(it.gate);
    const int dd = d1 * d2;
    // theta[(a,s1'),(c,s2')] = sum_{s1,s2} g[(s1' s2'),(s1 s2)] sum_b R1[a,(s1,b)] R2[c,(s2,b)],  R_i[a,(s,b)] = sqrt(l_a) conj(W_i[(s,b),a])
    // With the gate as an operator sum (opA / opB, lowA / lowB given: every ComplexF32 batch) theta = A B^T is formed from the factors by
    // gate_theta_mm_kernel on the f64 matrix cores; the element-wise loop below (128 dependent, uncoalesced loads per entry: 285 us per
    // 190-gate batch) only serves states without the factorisation (ComplexF64)
    const bool via_factors = it.kappa > 0 && it.lowA && it.lowB;
    if (!via_factors)
    for (int e = tid0; e < Mr * Nc; e += tstride) {
        int row = e % Mr, col = e / Mr;
        int a = row % r1, s1p = row / r1, c = col % r2, s2p = col / r2;
        const cx<double>* w1 = V1 + (size_t)it.n1 * it.idx1[a];
        const cx<double>* w2 = V2 + (size_t)it.n2 * it.idx2[c];
        cx<double> acc = cmake<double>(0, 0);
        for (int s1 = 0; s1 < d1; ++s1)
            for (int s2 = 0; s2 < d2; ++s2) {
                cx<double> gg = g[(s1p * d2 + s2p) + dd * (s1 * d2 + s2)];
                if (gg.re == 0 && gg.im == 0) continue;
                cx<double> cc = cmake<double>(0, 0);
                for (int b = 0; b < chi; ++b) {
                    cx<double> x = w1[s1 + d1 * b], y = w2[s2 + d2 * b];
                    // conj(x) * conj(y)
                    cc.re += x.re * y.re - x.im * y.im;
                    cc.im -= x.re * y.im + x.im * y.re;
                }
                cfma(acc, gg, cc);
            }
        double sc = sqrt(it.lam1[a] * it.lam2[c]);
        // one-sided Jacobi needs rows >= columns: a wide theta is stored as theta^dagger (Nc x Mr)
        cx<T>* th0 = reinterpret_cast<cx<T>*>(it.theta0);
        if (!wide) { cx<T> v = cmake<T>((T)(acc.re * sc), (T)(acc.im * sc)); th[e] = v; if (th0) th0[e] = v; }
        else { cx<T> v = cmake<T>((T)(acc.re * sc), (T)(-acc.im * sc)); th[col + (size_t)Nc * row] = v; if (th0) th0[col + (size_t)Nc * row] = v; }
    }
    const int nI = wide ? Mr : Nc;
    for (int e = tid0; e < nI * nI; e += tstride) tv[e] = cmake<T>((e % nI) == (e / nI) ? (T)1 : (T)0, (T)0);
    // low-rank route (GateItem): A[(a,s1'),(k,b)] = sum_s1 a_k[s1',s1] R1[a,(s1,b)],  B[(c,s2'),(k,b)] = sum_s2 b_k[s2',s2] R2[c,(s2,b)],  G = B^dagger B
    const int K = it.kappa * chi;
    const bool low = it.kappa > 0 && it.lowG && !wide && K < Nc && it.chi_cap <= K;      // (the host only hands out lowG where the route may be taken)
    if (threadIdx.x == 0 && part == 0) { it.info[5] = wide ? 1 : 0; it.info[7] = low ? K : 0; }       // info[7]: lowrank_g / chol / lowrank_m follow
    if (via_factors) {
        cx<double>* LA = reinterpret_cast<cx<double>*>(it.lowA);
        cx<double>* LB = reinterpret_cast<cx<double>*>(it.lowB);
        const cx<double>* oa = reinterpret_cast<const cx<double>*>(it.opA);
        const cx<double>* ob = reinterpret_cast<const cx<double>*>(it.opB);
        for (int e = tid0; e < Mr * K; e += tstride) {
            const int row = e % Mr, l = e / Mr, a = row % r1, s1p = row / r1, b = l % chi, k = l / chi;
            const cx<double>* w1 = V1 + (size_t)it.n1 * it.idx1[a];
            cx<double> acc = cmake<double>(0, 0);
            for (int s1 = 0; s1 < d1; ++s1) { cx<double> x = w1[s1 + d1 * b]; cfma(acc, oa[k * d1 * d1 + s1p + d1 * s1], cmake<double>(x.re, -x.im)); }
            const double sc = sqrt(it.lam1[a]);
            LA[e] = cmake<double>(acc.re * sc, acc.im * sc);
        }
        for (int e = tid0; e < Nc * K; e += tstride) {
            const int row = e % Nc, l = e / Nc, c = row % r2, s2p = row / r2, b = l % chi, k = l / chi;
            const cx<double>* w2 = V2 + (size_t)it.n2 * it.idx2[c];
            cx<double> acc = cmake<double>(0, 0);
            for (int s2 = 0; s2 < d2; ++s2) { cx<double> y = w2[s2 + d2 * b]; cfma(acc, ob[k * d2 * d2 + s2p + d2 * s2], cmake<double>(y.re, -y.im)); }
            const double sc = sqrt(it.lam2[c]);
            LB[e] = cmake<double>(acc.re * sc, acc.im * sc);
        }
    }
    if (!low && it.lowG && it.kappa > 0) {      // low-rank SVD route not taken: give chol_kernel a harmless identity
        cx<double>* LG = reinterpret_cast<cx<double>*>(it.lowG);
        for (int e = tid0; e < K * K; e += tstride) LG[e] = cmake<double>((e % K) == (e / K) ? 1.0 : 0.0, 0.0);
    }
}
// ---- small complex f64 products on v_mfma_f64_16x16x4_f64: one wave per 16 x 16 tile  C[i][j] (+)= sum_k a(i, k) b(k, j) -------------------
// Operand layout of the instruction: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15], C[row = (lane >> 4) + 4 r][col = lane & 15].
// fa(i, k) / fb(k, j) return the operand (zero outside the matrix); four real products per complex step (these kernels are latency, not
// throughput: the gain over the scalar loops is that a tile takes 2 loads per 4 x 256 multiply-adds instead of 2 per multiply-add)
// theta = A B^T from the operator-sum factors gate_theta_kernel wrote (lowA: Mr x K, lowB: Nc x K, complex128), to theta and theta0 in
// the state's precision; a wide theta is stored as its adjoint.  The tile orientation is chosen so that the lanes run along the
// contiguous index of the destination.
template <class T>
__global__ __launch_bounds__(1024) void gate_theta_mm_kernel(const GateItem* __restrict__ items) {
    const GateItem it = items[blockIdx.x];
    if (!(it.kappa > 0 && it.lowA && it.lowB)) return;
    const int Mr = it.info[0] * it.d1, Nc = it.info[1] * it.d2, K = it.kappa * it.chi;
    const bool wide = it.info[5] != 0;
    const cx<double>* LA = reinterpret_cast<const cx<double>*>(it.lowA);
    const cx<double>* LB = reinterpret_cast<const cx<double>*>(it.lowB);
    cx<T>* th = reinterpret_cast<cx<T>*>(it.theta);
    cx<T>* th0 = reinterpret_cast<cx<T>*>(it.theta0);
    const int lane = threadIdx.x & 63, l15 = lane & 15, kq = lane >> 4;
    const int w = blockIdx.y * (blockDim.x >> 6) + (threadIdx.x >> 6), nw = gridDim.y * (blockDim.x >> 6);
    // rows of the tile product = the index that is NOT contiguous in the destination: (c, s2') for theta[i + Mr j], (a, s1') for the adjoint
    const int R = wide ? Mr : Nc, Cn = wide ? Nc : Mr;              // tile rows run over R, tile columns (lanes) over Cn
    const cx<double>* PR = wide ? LA : LB; const cx<double>* PC = wide ? LB : LA;
    const int tr = (R + 15) >> 4, tc = (Cn + 15) >> 4;
    for (int t = w; t < tr * tc; t += nw) {
        const int r0 = 16 * (t % tr), c0 = 16 * (t / tr);
        v4d cr = {0, 0, 0, 0}, ci = {0, 0, 0, 0};
        ztile_mm(K, r0 + l15, c0 + l15,
                 [&](int i, int k) { return (i < R && k < K) ? PR[i + (size_t)R * k] : cmake<double>(0, 0); },
                 [&](int k, int j) { return (j < Cn && k < K) ? PC[j + (size_t)Cn * k] : cmake<double>(0, 0); }, cr, ci);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = r0 + kq + 4 * r, col = c0 + l15;
            if (row < R && col < Cn) {
                // not wide: theta[i = col][j = row] at col + Mr * row;  wide: stored adjoint theta^dagger[j = col][i = row] at col + Nc * row, conjugated
                const cx<T> v = cmake<T>((T)cr[r], (T)(wide ? -ci[r] : ci[r]));
                th[col + (size_t)Cn * row] = v; if (th0) th0[col + (size_t)Cn * row] = v;
            }
        }
    }
}
template <class T> void launch_gate_theta_mm(hipStream_t s, const GateItem* d_items, int nitems) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL((gate_theta_mm_kernel<T>), dim3(nitems, 2), dim3(1024), 0, s, d_items);
    TNQS_CHECK_LAUNCH();
}
template void launch_gate_theta_mm<float>(hipStream_t, const GateItem*, int);
template void launch_gate_theta_mm<double>(hipStream_t, const GateItem*, int);
// G = B^dagger B of the low-rank route (GateItem): upper 16 x 16 tiles on the f64 matrix cores, mirrored
__global__ __launch_bounds__(1024) void lowrank_g_kernel(const GateItem* __restrict__ items) {
    const GateItem it = items[blockIdx.x];
    const int K = it.info[7];
    if (K <= 0) return;
    const int Nc = it.info[1] * it.d2;
    const cx<double>* LB = reinterpret_cast<const cx<double>*>(it.lowB);
    cx<double>* LG = reinterpret_cast<cx<double>*>(it.lowG);
    const int lane = threadIdx.x & 63, l15 = lane & 15, kq = lane >> 4;
    const int w = blockIdx.y * (blockDim.x >> 6) + (threadIdx.x >> 6), nw = gridDim.y * (blockDim.x >> 6);
    const int nt = (K + 15) >> 4;
    for (int t = w; t < nt * nt; t += nw) {
        const int ti = t % nt, tj = t / nt;
        if (ti > tj) continue;
        v4d cr = {0, 0, 0, 0}, ci = {0, 0, 0, 0};
        ztile_mm(Nc, 16 * ti + l15, 16 * tj + l15,                                   // G[i][j] = sum_row conj(B[row, i]) B[row, j]
                 [&](int i, int k) { cx<double> v = (i < K && k < Nc) ? LB[k + (size_t)Nc * i] : cmake<double>(0, 0); v.im = -v.im; return v; },
                 [&](int k, int j) { return (j < K && k < Nc) ? LB[k + (size_t)Nc * j] : cmake<double>(0, 0); }, cr, ci);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = 16 * ti + kq + 4 * r, j = 16 * tj + l15;
            // (the diagonal's imaginary part is zero in exact arithmetic; its two sums of products round differently, so it is written as zero: G is Hermitian exactly)
            if (i < K && j < K && i <= j) { LG[i + (size_t)K * j] = cmake<double>(cr[r], i == j ? 0.0 : ci[r]); if (i != j) LG[j + (size_t)K * i] = cmake<double>(cr[r], -ci[r]); }
        }
    }
}
void launch_lowrank_g(hipStream_t s, const GateItem* d_items, int nitems) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL(lowrank_g_kernel, dim3(nitems, 4), dim3(1024), 0, s, d_items);
    TNQS_CHECK_LAUNCH();
}
// theta[:, 0..K) := M = A conj(L) where G = L L^dagger (chol_kernel); on a collapsed pivot the full theta (already in place) stays.
// Tiles with rows = column index j of M, lanes = row index i (contiguous in theta).
template <class T>
__global__ __launch_bounds__(1024) void lowrank_m_kernel(const GateItem* __restrict__ items) {
    const GateItem it = items[blockIdx.x];
    const int K = it.info[7];
    if (K <= 0) return;
    if (*it.lowfail) { if (threadIdx.x == 0 && blockIdx.y == 0) it.info[7] = 0; return; }
    const int Mr = it.info[0] * it.d1;
    const cx<double>* LA = reinterpret_cast<const cx<double>*>(it.lowA);
    const cx<double>* L = reinterpret_cast<const cx<double>*>(it.lowL);
    cx<T>* th = reinterpret_cast<cx<T>*>(it.theta);
    const int lane = threadIdx.x & 63, l15 = lane & 15, kq = lane >> 4;
    const int w = blockIdx.y * (blockDim.x >> 6) + (threadIdx.x >> 6), nw = gridDim.y * (blockDim.x >> 6);
    const int tr = (K + 15) >> 4, tc = (Mr + 15) >> 4;
    for (int t = w; t < tr * tc; t += nw) {
        const int j0 = 16 * (t % tr), i0 = 16 * (t / tr);
        v4d cr = {0, 0, 0, 0}, ci = {0, 0, 0, 0};
        ztile_mm(K, j0 + l15, i0 + l15,                                              // M[i][j] = sum_{l >= j} A[i, l] conj(L[l, j]), L lower triangular
                 [&](int j, int l) { cx<double> v = (j < K && l < K && l >= j) ? L[l + (size_t)K * j] : cmake<double>(0, 0); v.im = -v.im; return v; },
                 [&](int l, int i) { return (i < Mr && l < K) ? LA[i + (size_t)Mr * l] : cmake<double>(0, 0); }, cr, ci);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = j0 + kq + 4 * r, i = i0 + l15;
            if (i < Mr && j < K) th[i + (size_t)Mr * j] = cmake<T>((T)cr[r], (T)ci[r]);
        }
    }
    // Q = B L^-dagger = B W (Nc x K, orthonormal columns; W upper triangular): theta = M Q^T, so the right singular vectors of theta are
    // conj(Q) times those of M -- what theta_svd_pre_kernel builds V from (no recovery from theta0)
    if (!it.lowQ || !it.lowW) return;
    const int Nc = it.info[1] * it.d2;
    const cx<double>* LB = reinterpret_cast<const cx<double>*>(it.lowB);
    const cx<double>* W = reinterpret_cast<const cx<double>*>(it.lowW);
    cx<double>* Q = reinterpret_cast<cx<double>*>(it.lowQ);
    const int qc = (Nc + 15) >> 4;
    for (int t = w; t < tr * qc; t += nw) {
        const int j0 = 16 * (t % tr), i0 = 16 * (t / tr);
        v4d cr = {0, 0, 0, 0}, ci = {0, 0, 0, 0};
        ztile_mm(K, j0 + l15, i0 + l15,                                              // Q[i][j] = sum_{l <= j} B[i, l] W[l, j]   (tile rows = j, lanes = i)
                 [&](int j, int l) { return (j < K && l < K && l <= j) ? W[l + (size_t)K * j] : cmake<double>(0, 0); },
                 [&](int l, int i) { return (i < Nc && l < K) ? LB[i + (size_t)Nc * l] : cmake<double>(0, 0); }, cr, ci);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = j0 + kq + 4 * r, i = i0 + l15;
            if (i < Nc && j < K) Q[i + (size_t)Nc * j] = cmake<double>(cr[r], ci[r]);
        }
    }
}
// theta, theta0 *= 2^k with k = -exponent of the largest |entry| of theta0 (exact); *texp = k.  Runs after gate_theta / lowrank_m.
template <class T>
__global__ __launch_bounds__(1024) void theta_scale_kernel(const GateItem* __restrict__ items) {
    __shared__ float s_max[16];
    __shared__ int s_k;
    const GateItem it = items[blockIdx.x];
    const int ne = it.info[0] * it.d1 * it.info[1] * it.d2;
    cx<T>* th = reinterpret_cast<cx<T>*>(it.theta);
    cx<T>* th0 = reinterpret_cast<cx<T>*>(it.theta0);
    float mx = 0.f;
    for (int e = threadIdx.x; e < ne; e += blockDim.x) { cx<T> v = th0[e]; mx = fmaxf(mx, fmaxf(fabsf((float)v.re), fabsf((float)v.im))); }
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        float m2 = 0.f; for (int w = 0; w < (int)(blockDim.x >> 6); ++w) m2 = fmaxf(m2, s_max[w]);
        int k = 0;
        if (m2 > 0.f && m2 < 3e38f) { k = -ilogbf(m2); k = k > 120 ? 120 : (k < -120 ? -120 : k); }
        s_k = k; *it.texp = k;
    }
    __syncthreads();
    const int k = s_k;
    if (k == 0) return;
    const T sc = (T)ldexp(1.0, k);
    for (int e = threadIdx.x; e < ne; e += blockDim.x) { cx<T> a = th[e], b = th0[e]; th[e] = cmake<T>(a.re * sc, a.im * sc); th0[e] = cmake<T>(b.re * sc, b.im * sc); }
}
template <class T> void launch_theta_scale(hipStream_t s, const GateItem* d_items, int nitems) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL((theta_scale_kernel<T>), dim3(nitems), dim3(1024), 0, s, d_items); TNQS_CHECK_LAUNCH();
}
template void launch_theta_scale<float>(hipStream_t, const GateItem*, int);
template void launch_theta_scale<double>(hipStream_t, const GateItem*, int);
template <class T> void launch_lowrank_m(hipStream_t s, const GateItem* d_items, int nitems) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL((lowrank_m_kernel<T>), dim3(nitems, 4), dim3(1024), 0, s, d_items);
    TNQS_CHECK_LAUNCH();
}
template void launch_lowrank_m<float>(hipStream_t, const GateItem*, int);
template void launch_lowrank_m<double>(hipStream_t, const GateItem*, int);
// CholeskyQR2 of B (LowQr2Item, kernels.hpp): B1 = B W1, W1 = L1^-dagger upper triangular
__global__ __launch_bounds__(1024) void lowrank_bw_kernel(const LowQr2Item* __restrict__ items) {
    const LowQr2Item it = items[blockIdx.x];
    const int K = it.info[7];
    if (K <= 0 || *it.fail1) return;
    const int Nc = it.info[1] * it.d2;
    const cx<double>* B = reinterpret_cast<const cx<double>*>(it.B);
    const cx<double>* W = reinterpret_cast<const cx<double>*>(it.W1);
    cx<double>* B1 = reinterpret_cast<cx<double>*>(it.B1);
    const int lane = threadIdx.x & 63, l15 = lane & 15, kq = lane >> 4;
    const int w = blockIdx.y * (blockDim.x >> 6) + (threadIdx.x >> 6), nw = gridDim.y * (blockDim.x >> 6);
    const int tr = (K + 15) >> 4, tc = (Nc + 15) >> 4;
    for (int t = w; t < tr * tc; t += nw) {                                             // tile rows = column j of B1, lanes = row i (contiguous)
        const int j0 = 16 * (t % tr), i0 = 16 * (t / tr);
        v4d cr = {0, 0, 0, 0}, ci = {0, 0, 0, 0};
        ztile_mm(K, j0 + l15, i0 + l15,                                                 // B1[i][j] = sum_{l <= j} B[i, l] W[l, j]
                 [&](int j, int l) { return (j < K && l < K && l <= j) ? W[l + (size_t)K * j] : cmake<double>(0, 0); },
                 [&](int l, int i) { return (i < Nc && l < K) ? B[i + (size_t)Nc * l] : cmake<double>(0, 0); }, cr, ci);
#pragma unroll
        for (int r = 0; r < 4; ++r) { const int j = j0 + kq + 4 * r, i = i0 + l15; if (i < Nc && j < K) B1[i + (size_t)Nc * j] = cmake<double>(cr[r], ci[r]); }
    }
}
void launch_lowrank_bw(hipStream_t s, const LowQr2Item* d_items, int nitems) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL(lowrank_bw_kernel, dim3(nitems, 4), dim3(1024), 0, s, d_items); TNQS_CHECK_LAUNCH();
}
// Lc = L1 L2 (both lower triangular), and the second pass's failure folded into the gate's flag
__global__ __launch_bounds__(1024) void lowrank_ll_kernel(const LowQr2Item* __restrict__ items) {
    const LowQr2Item it = items[blockIdx.x];
    const int K = it.info[7];
    if (K <= 0 || *it.fail1) return;
    if (*it.fail2) { if (threadIdx.x == 0) *it.fail1 = 1; return; }
    const cx<double>* L1 = reinterpret_cast<const cx<double>*>(it.L1);
    const cx<double>* L2 = reinterpret_cast<const cx<double>*>(it.L2);
    cx<double>* Lc = reinterpret_cast<cx<double>*>(it.Lc);
    const int lane = threadIdx.x & 63, l15 = lane & 15, kq = lane >> 4;
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int nt = (K + 15) >> 4;
    for (int t = w; t < nt * nt; t += nw) {                                             // tile rows = column j, lanes = row i
        const int j0 = 16 * (t % nt), i0 = 16 * (t / nt);
        v4d cr = {0, 0, 0, 0}, ci = {0, 0, 0, 0};
        if (i0 + 15 >= j0)
        ztile_mm(K, j0 + l15, i0 + l15,                                                 // Lc[i][j] = sum_{j <= l <= i} L1[i, l] L2[l, j]
                 [&](int j, int l) { return (j < K && l < K && l >= j) ? L2[l + (size_t)K * j] : cmake<double>(0, 0); },
                 [&](int l, int i) { return (i < K && l < K && l <= i) ? L1[i + (size_t)K * l] : cmake<double>(0, 0); }, cr, ci);
#pragma unroll
        for (int r = 0; r < 4; ++r) { const int j = j0 + kq + 4 * r, i = i0 + l15; if (i < K && j < K) Lc[i + (size_t)K * j] = (i >= j) ? cmake<double>(cr[r], ci[r]) : cmake<double>(0, 0); }
    }
}
void launch_lowrank_ll(hipStream_t s, const LowQr2Item* d_items, int nitems) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL(lowrank_ll_kernel, dim3(nitems), dim3(1024), 0, s, d_items); TNQS_CHECK_LAUNCH();
}
template <class T> void launch_gate_theta(hipStream_t s, const GateItem* d_items, int nitems) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL((gate_theta_kernel<T>), dim3(nitems, 8), dim3(1024), 0, s, d_items);
    TNQS_CHECK_LAUNCH();
}
template void launch_gate_theta<float>(hipStream_t, const GateItem*, int);
template void launch_gate_theta<double>(hipStream_t, const GateItem*, int);

// ---- second factorisation pass (CholeskyQR2) of ill-conditioned ComplexF64 sites: kernels.hpp, Qr2RinvItem / Qr2ComposeItem ----------
__global__ __launch_bounds__(256) void qr2_rinv_kernel(const Qr2RinvItem* __restrict__ items) {
    const Qr2RinvItem it = items[blockIdx.x];
    const int n = it.n, r = *it.r;
    const cx<double>* W = reinterpret_cast<const cx<double>*>(it.GW);
    cx<double>* X = reinterpret_cast<cx<double>*>(it.X1);
    for (int e = threadIdx.x; e < n * n; e += 256) {
        const int i = e % n, a = e / n;
        if (a < r) { const double sc = 1.0 / sqrt(it.lam[a]); cx<double> w = W[i + (size_t)n * it.idx[a]]; X[e] = cmake<double>(w.re * sc, w.im * sc); }
        else X[e] = cmake<double>(0, 0);
    }
}
void launch_qr2_rinv(hipStream_t s, const Qr2RinvItem* d_items, int nitems) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL(qr2_rinv_kernel, dim3(nitems), dim3(256), 0, s, d_items); TNQS_CHECK_LAUNCH();
}
__global__ __launch_bounds__(256) void qr2_compose_kernel(const Qr2ComposeItem* __restrict__ items) {
    __shared__ double lam2[256]; __shared__ int sel[256]; __shared__ int s_r2;
    const Qr2ComposeItem it = items[blockIdx.x];
    const int n = it.n, r1 = *it.r1;
    const cx<double>* A2 = reinterpret_cast<const cx<double>*>(it.A2);
    const cx<double>* V2 = reinterpret_cast<const cx<double>*>(it.V2);
    const cx<double>* X1 = reinterpret_cast<const cx<double>*>(it.X1);
    const cx<double>* W1 = reinterpret_cast<const cx<double>*>(it.GV1);
    for (int j = threadIdx.x; j < n; j += 256) {          // Rayleigh quotients, as gate_eigs
        double l = 0;
        for (int i = 0; i < n; ++i) { cx<double> v = V2[i + (size_t)n * j], a = A2[i + (size_t)n * j]; l += v.re * a.re + v.im * a.im; }
        lam2[j] = l;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double lmax = 0; for (int j = 0; j < n; ++j) lmax = fmax(lmax, lam2[j]);
        int r = 0; for (int j = 0; j < n; ++j) if (lam2[j] > it.tau * lmax && lam2[j] > 0) sel[r++] = j;
        s_r2 = r; *it.rk = r;
    }
    __syncthreads();
    const int r2 = s_r2;
    cx<double>* GV = reinterpret_cast<cx<double>*>(it.GVout);
    cx<double>* GW = reinterpret_cast<cx<double>*>(it.GWout);
    // GW[:,c] = X1 V2[:,j_c] / sqrt(l2_c);   GV[:,c] = sqrt(l2_c) sum_a sqrt(l1_a) W1[:, idx1_a] V2[a, j_c]   (= conj of row c of R2 R1)
    for (int e = threadIdx.x; e < n * n; e += 256) {
        const int i = e % n, c = e / n;
        if (c >= r2) { GV[e] = cmake<double>(0, 0); GW[e] = cmake<double>(0, 0); continue; }
        const int j = sel[c]; const double sq = sqrt(lam2[j]);
        cx<double> gw = cmake<double>(0, 0), gv = cmake<double>(0, 0);
        for (int a = 0; a < r1; ++a) {
            const cx<double> v = V2[a + (size_t)n * j];
            cfma(gw, X1[i + (size_t)n * a], v);
            const double s1 = sqrt(it.lam1[a]); const cx<double> w = W1[i + (size_t)n * it.idx1[a]];
            cfma(gv, cmake<double>(w.re * s1, w.im * s1), v);
        }
        GW[e] = cmake<double>(gw.re / sq, gw.im / sq); GV[e] = cmake<double>(gv.re * sq, gv.im * sq);
    }
}
void launch_qr2_compose(hipStream_t s, const Qr2ComposeItem* d_items, int nitems) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL(qr2_compose_kernel, dim3(nitems), dim3(256), 0, s, d_items); TNQS_CHECK_LAUNCH();
}

template <class T>
__global__ __launch_bounds__(1024) void gate_finish_kernel(const GateItem* __restrict__ items) {
    __shared__ double sig[512];
    __shared__ int perm[512];
    __shared__ int s_keep;
    // grid (gate, part) as gate_theta_kernel: the ranking / truncation prologue is repeated per part, only part 0 writes its results
    const GateItem it = items[blockIdx.x];
    const int part = blockIdx.y;
    const int r1 = it.info[0], r2 = it.info[1], d1 = it.d1, d2 = it.d2;
    const int Mr = r1 * d1, Nc = r2 * d2;
    const bool wide = it.info[5] != 0;                                // theta stored as theta^dagger (Nc x Mr)
    const int ncol = wide ? Mr : Nc, ld = wide ? Nc : Mr;
    const cx<T>* th = reinterpret_cast<const cx<T>*>(it.theta);      // rotated columns: U Sigma (or V Sigma when wide)
    const cx<T>* tv = reinterpret_cast<const cx<T>*>(it.thetaV);     // accumulated rotations: V (or U when wide)
    const int ncolK = (!wide && it.info[7] > 0) ? it.info[7] : ncol;        // low-rank route: the remaining singular values are zero
    const double tsc = ldexp(1.0, -(*it.texp));                               // theta was scaled by 2^texp
    for (int u = threadIdx.x; u < ncol; u += blockDim.x) {
        double s2 = 0;
        if (u < ncolK) for (int i = 0; i < ld; ++i) { cx<T> v = th[i + (size_t)ld * u]; s2 += (double)v.re * v.re + (double)v.im * v.im; }
        sig[u] = (s2 == s2 && s2 < 1e300) ? sqrt(s2) * tsc : 0.0;     // a NaN / inf column must not poison the ranking below; tsc undoes theta_scale_kernel
    }
    __syncthreads();
    for (int u = threadIdx.x; u < ncol; u += blockDim.x) {    // rank by counting (descending, stable)
        perm[rank_desc(sig, ncol, u)] = u;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        // NDTensors truncate! on P = S^2 (computed in the data's real precision), relative cutoff, mindim = 1
        const int nsv = min(Mr, Nc);     // number of singular values of theta
        int n = nsv;
        int status = 0;
        T truncerr = 0;
        T p0 = (T)sig[perm[0]]; p0 = p0 * p0;
        if (p0 <= 0) { n = 1; }
        else if (nsv > 1) {
            const int md = it.maxdim > 0 ? it.maxdim : nsv;
            while (n > md) { T s = (T)sig[perm[n - 1]]; truncerr += s * s; --n; }
            T scale = 0;
            for (int i = 0; i < nsv; ++i) { T s = (T)sig[perm[i]]; scale += s * s; }
            if (scale == 0) scale = 1;
            const T cut = (T)(it.cutoff < 0 ? 0.0 : it.cutoff);
            while (n > 1) { T s = (T)sig[perm[n - 1]]; T p = s * s; if (truncerr + p <= cut * scale) { truncerr += p; --n; } else break; }
            truncerr = truncerr / scale;
        }
        if (n > it.chi_cap) { status = 1; n = it.chi_cap; }
        double nrm = 0;
        for (int i = 0; i < n; ++i) nrm += sig[perm[i]] * sig[perm[i]];
        nrm = sqrt(nrm);
        if (part == 0) {
            for (int i = 0; i < n; ++i) {
                double s = sig[perm[i]];
                it.S[i] = (it.normalize && nrm > 0) ? (double)((T)s / (T)nrm) : (double)(T)s;
            }
            it.info[2] = n; it.info[3] = status; *it.truncerr = (double)truncerr;
        }
        s_keep = n;
    }
    // per-column factors of R^+ = W diag(lambda^-1/2) (and of the theta scaling), once per workgroup: a square root and a division per
    // INNER iteration were most of this kernel's time
    __shared__ double fa1[512], fa2[512];
    for (int a = threadIdx.x; a < r1; a += blockDim.x) fa1[a] = (wide ? 1.0 : tsc) / sqrt(it.lam1[a]);      // th holds the scaled U Sigma (tv, the recovered vectors, is scale free)
    for (int c = threadIdx.x; c < r2; c += blockDim.x) fa2[c] = (wide ? tsc : 1.0) / sqrt(it.lam2[c]);
    __syncthreads();
    const int nk = s_keep;
    const cx<double>* V1 = reinterpret_cast<const cx<double>*>(it.GW1);       // R^+ = W diag(lambda^-1/2)
    const cx<double>* V2 = reinterpret_cast<const cx<double>*>(it.GW2);
    cx<T>* X1 = reinterpret_cast<cx<T>*>(it.X1);
    cx<T>* X2 = reinterpret_cast<cx<T>*>(it.X2);
    const int n1 = it.n1, n2 = it.n2;
    // X1[(s,b),(s1',u)] = sum_a W1[(s,b),a] / sqrt(l1_a) * (U Sigma)[(a,s1'),pi(u)] / sqrt(sigma_u)
    // X2[(s,b),(s2',u)] = sum_c W2[(s,b),c] / sqrt(l2_c) * sqrt(sigma_u) conj(Vtheta[(c,s2'),pi(u)])
    // Two small complex products (64 x 64 x 64 at chi = 32) on the f64 matrix cores, one wave per 16 x 16 tile (ztile_mm); the tile's lanes
    // run along (s,b), the contiguous index of X.  (The scalar loops these replace chased idx -> W -> multiply-add through L2 once per term:
    // 0.23 ms per launch at chi = 32, most of it load latency.)
    const int lane = threadIdx.x & 63, l15 = lane & 15, kq = lane >> 4;
    const int wv = part * (blockDim.x >> 6) + (threadIdx.x >> 6), nwv = gridDim.y * (blockDim.x >> 6);
    const int N1 = d1 * nk, N2 = d2 * nk;
    const int t1r = (N1 + 15) >> 4, t1c = (n1 + 15) >> 4, t2r = (N2 + 15) >> 4, t2c = (n2 + 15) >> 4;
    for (int t = wv; t < t1r * t1c + t2r * t2c; t += nwv) {
        const bool second = t >= t1r * t1c;
        const int tt = second ? t - t1r * t1c : t;
        const int tr = second ? t2r : t1r;
        const int r0 = 16 * (tt % tr), c0 = 16 * (tt / tr);
        v4d cr = {0, 0, 0, 0}, ci = {0, 0, 0, 0};
        if (!second) {
            ztile_mm(r1, r0 + l15, c0 + l15,
                     [&](int nn, int a2) {
                         if (nn >= N1 || a2 >= r1) return cmake<double>(0, 0);
                         const int s1p = nn % d1, u = nn / d1, pu = perm[u];
                         const double su = sig[pu];
                         if (!(su > 0)) return cmake<double>(0, 0);
                         const cx<T> l = wide ? tv[(a2 + r1 * s1p) + (size_t)Mr * pu] : th[(a2 + r1 * s1p) + (size_t)Mr * pu];
                         const double f = fa1[a2] * (wide ? sqrt(su) : 1.0 / sqrt(su));              // L = U sqrt(S)
                         return cmake<double>(l.re * f, l.im * f);
                     },
                     [&](int a2, int kk) { return (kk < n1 && a2 < r1) ? V1[kk + (size_t)n1 * it.idx1[a2]] : cmake<double>(0, 0); }, cr, ci);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int nn = r0 + kq + 4 * r, kk = c0 + l15;
                if (nn < N1 && kk < n1) X1[kk + (size_t)n1 * nn] = cmake<T>((T)cr[r], (T)ci[r]);
            }
        } else {
            ztile_mm(r2, r0 + l15, c0 + l15,
                     [&](int nn, int c2) {
                         if (nn >= N2 || c2 >= r2) return cmake<double>(0, 0);
                         const int s2p = nn % d2, u = nn / d2, pu = perm[u];
                         const double su = sig[pu];
                         if (wide && !(su > 0)) return cmake<double>(0, 0);
                         const cx<T> v = wide ? th[(c2 + r2 * s2p) + (size_t)Nc * pu] : tv[(c2 + r2 * s2p) + (size_t)Nc * pu];
                         const double f = fa2[c2] * (wide ? 1.0 / sqrt(su) : sqrt(su));              // R = sqrt(S) V^dagger
                         return cmake<double>(v.re * f, -v.im * f);
                     },
                     [&](int c2, int kk) { return (kk < n2 && c2 < r2) ? V2[kk + (size_t)n2 * it.idx2[c2]] : cmake<double>(0, 0); }, cr, ci);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int nn = r0 + kq + 4 * r, kk = c0 + l15;
                if (nn < N2 && kk < n2) X2[kk + (size_t)n2 * nn] = cmake<T>((T)cr[r], (T)ci[r]);
            }
        }
    }
}
template <class T> void launch_gate_finish(hipStream_t s, const GateItem* d_items, int nitems) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL((gate_finish_kernel<T>), dim3(nitems, 4), dim3(1024), 0, s, d_items);
    TNQS_CHECK_LAUNCH();
}
template void launch_gate_finish<float>(hipStream_t, const GateItem*, int);
template void launch_gate_finish<double>(hipStream_t, const GateItem*, int);

}  // namespace tnqs
