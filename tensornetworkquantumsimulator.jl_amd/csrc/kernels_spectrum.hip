// kernels_spectrum.hip -- entanglement spectrum of a bond from its two BP messages (engine_spectra.cpp; src/entanglement.jl:73-86 with pseudo_sqrt_inv_sqrt,
// src/utils.jl:18-26).  For a bond (u, v): m1 = message u -> v, m2 = message v -> u, r = m2^{1/2} (eigenvalues below the cutoff dropped), rho = r m1^T r, spectrum =
// eigenvalues of rho / tr rho.  With m2 = V Lambda V^dagger (stage A: env_prepare + the f64 Jacobi, A = H V) and D = f(Lambda),
//   W = D V^dagger (m1^T V) D = V^dagger rho V
// has the spectrum of rho: two n x n products, r is never formed.
//   bond_rho_kernel<T>            stage B: Rayleigh quotients of m2, the cutoff rule, T1 = m1^T V, W = D (V^dagger T1) D, Hermitised in place, tr W, V2 = I
//   bond_spectrum_finish_kernel   stage D: signed Rayleigh quotients of W (from its Jacobi factorisation, stage C) / tr W, sorted descending
// One workgroup of 256 threads per bond, any 1 <= n <= 256.  Arithmetic: complex128 with plain f64 FMAs, every sum in a fixed order.
#include "device_common.hpp"
#include "jacobi_common.hpp"
#include "kernels.hpp"

namespace tnqs {

namespace {
constexpr int kSpecTile = 32;                 // output tile: 32 x 32 entries, 2 x 2 per thread
constexpr int kSpecK = 16;                    // depth of a staged block
constexpr int kSpecPitch = kSpecTile + 1;     // LDS pitch of a staged row (complex128): consecutive depths land in different banks

// C[r, c] = sum_k X(k, r) Y[k + n c] for all r, c < n by the whole workgroup (256 threads): X^T Y (or X^dagger Y when loadX conjugates).  Blocks of 16 depths of a
// 32-row and a 32-column panel are staged in LDS (As / Bs, kSpecK * kSpecPitch complex128 each); thread (tx, ty) owns rows r0 + tx + 16 p and columns c0 + ty + 16 q.
// Every entry is one accumulator summed over k in ascending order (panel entries beyond n are exact zeros).  store(r, c, value) is called once per entry.
template <class LX, class ST>
__device__ __forceinline__ void wg_xty(int n, LX loadX, const cx<double>* Y, ST store, cx<double>* As, cx<double>* Bs) {
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const cx<double> zero = cmake<double>(0.0, 0.0);
    for (int c0 = 0; c0 < n; c0 += kSpecTile) for (int r0 = 0; r0 < n; r0 += kSpecTile) {
        cx<double> c00 = zero, c10 = zero, c01 = zero, c11 = zero;
        for (int k0 = 0; k0 < n; k0 += kSpecK) {
            __syncthreads();                                   // the previous block has been consumed
            for (int e = tid; e < kSpecK * kSpecTile; e += 256) {
                const int kk = e & (kSpecK - 1), rr = e >> 4, k = k0 + kk, r = r0 + rr, c = c0 + rr;
                double are = 0.0, aim = 0.0, bre = 0.0, bim = 0.0;
                if (k < n && r < n) { const cx<double> t = loadX(k, r); are = t.re; aim = t.im; }
                if (k < n && c < n) { const cx<double> t = Y[k + (size_t)n * c]; bre = t.re; bim = t.im; }
                As[kk * kSpecPitch + rr] = cmake<double>(are, aim);
                Bs[kk * kSpecPitch + rr] = cmake<double>(bre, bim);
            }
            __syncthreads();
#pragma unroll 4
            for (int kk = 0; kk < kSpecK; ++kk) {
                const cx<double> a0 = As[kk * kSpecPitch + tx], a1 = As[kk * kSpecPitch + tx + 16];
                const cx<double> b0 = Bs[kk * kSpecPitch + ty], b1 = Bs[kk * kSpecPitch + ty + 16];
                cfma(c00, a0, b0); cfma(c10, a1, b0); cfma(c01, a0, b1); cfma(c11, a1, b1);
            }
        }
        const int r = r0 + tx, c = c0 + ty;
        if (r < n && c < n) store(r, c, c00);
        if (r + 16 < n && c < n) store(r + 16, c, c10);
        if (r < n && c + 16 < n) store(r, c + 16, c01);
        if (r + 16 < n && c + 16 < n) store(r + 16, c + 16, c11);
    }
}
// Rayleigh quotient Re(v_j^dagger a_j) of column j by one wave (lanes stride over the rows, butterfly sum: the same value in every lane)
__device__ __forceinline__ double wave_rayleigh(const cx<double>* V, const cx<double>* A, int n, int j, int lane) {
    double x = 0;
    for (int i = lane; i < n; i += 64) { const cx<double> v = V[i + (size_t)n * j], a = A[i + (size_t)n * j]; x = fma(v.re, a.re, x); x = fma(v.im, a.im, x); }
    return wave_sum(x);
}
}  // namespace

template <class T>
__global__ __launch_bounds__(256) void bond_rho_kernel(const BondSpecItem* __restrict__ items) {
    __shared__ cx<double> As[kSpecK * kSpecPitch], Bs[kSpecK * kSpecPitch];
    __shared__ double dsc[256];
    __shared__ double sh[17];
    const BondSpecItem it = items[blockIdx.x];
    const int n = it.n, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const cx<double>* A = reinterpret_cast<const cx<double>*>(it.A);
    const cx<double>* V = reinterpret_cast<const cx<double>*>(it.V);
    const cx<T>* m1 = reinterpret_cast<const cx<T>*>(it.m1);
    // eigenvalues of m2 and the factors D = f(Lambda): 0 when |x| < cutoff, sqrt(x) otherwise; x <= -cutoff is the reference's DomainError
    for (int j = w; j < n; j += 4) {
        const double x = wave_rayleigh(V, A, n, j, lane);
        if (lane == 0) {
            double d = 0.0;
            if (!(fabs(x) < it.cutoff)) { if (x > 0) d = sqrt(x); else atomicOr(it.flag, 1); }      // (a NaN lands here as well)
            dsc[j] = d;
        }
    }
    __syncthreads();             // A is not read again: T1 may take its place
    // T1 = m1^T V: T1[i, j] = sum_k m1[k, i] V[k, j]      (m1 in the state's type; null = identity)
    cx<double>* T1 = reinterpret_cast<cx<double>*>(it.T1);
    wg_xty(n, [=](int k, int r) { if (!m1) return cmake<double>(k == r ? 1.0 : 0.0, 0.0); const cx<T> v = m1[k + (size_t)n * r]; return cmake<double>((double)v.re, (double)v.im); },
           V, [=](int r, int c, cx<double> v) { T1[r + (size_t)n * c] = v; }, As, Bs);
    __syncthreads();
    __threadfence_block();
    // W = D (V^dagger T1) D: W[a, b] = d_a d_b sum_i conj(V[i, a]) T1[i, b]
    cx<double>* W = reinterpret_cast<cx<double>*>(it.W);
    wg_xty(n, [=](int k, int r) { const cx<double> v = V[k + (size_t)n * r]; return cmake<double>(v.re, -v.im); },
           T1, [&](int r, int c, cx<double> v) { const double f = dsc[r] * dsc[c]; W[r + (size_t)n * c] = cmake<double>(v.re * f, v.im * f); }, As, Bs);
    __syncthreads();
    __threadfence_block();
    // (W + W^dagger) / 2 in place -- the thread of entry (r, c), r < c, owns both mirror entries --, the trace from the diagonal, V2 = I for the Jacobi of stage C
    cx<double>* V2 = reinterpret_cast<cx<double>*>(it.V2);
    double tr = 0;
    for (int e = tid; e < n * n; e += 256) {
        const int r = e % n, c = e / n;
        V2[e] = cmake<double>(r == c ? 1.0 : 0.0, 0.0);
        if (r > c) continue;
        const cx<double> a = W[r + (size_t)n * c];
        if (r == c) { W[e] = cmake<double>(a.re, 0.0); tr += a.re; continue; }
        const cx<double> b = W[c + (size_t)n * r];
        const double hr = 0.5 * (a.re + b.re), hi = 0.5 * (a.im - b.im);
        W[r + (size_t)n * c] = cmake<double>(hr, hi); W[c + (size_t)n * r] = cmake<double>(hr, -hi);
    }
    tr = block_sum(tr, sh);
    if (tid == 0) *it.trace = tr;
}
template <class T> void launch_bond_rho(hipStream_t s, const BondSpecItem* d_items, int nitems) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL((bond_rho_kernel<T>), dim3(nitems), dim3(256), 0, s, d_items); TNQS_CHECK_LAUNCH();
}
template void launch_bond_rho<float>(hipStream_t, const BondSpecItem*, int);
template void launch_bond_rho<double>(hipStream_t, const BondSpecItem*, int);

// W after its Jacobi factorisation (it.W = W V2, it.V2): lambda_j = Re(v_j^dagger a_j) / tr W with its sign, ranked descending (stable), written to it.out[0 .. n)
__global__ __launch_bounds__(256) void bond_spectrum_finish_kernel(const BondSpecItem* __restrict__ items) {
    __shared__ double lam[256];
    const BondSpecItem it = items[blockIdx.x];
    const int n = it.n, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const cx<double>* A = reinterpret_cast<const cx<double>*>(it.W);
    const cx<double>* V = reinterpret_cast<const cx<double>*>(it.V2);
    const double tr = *it.trace;
    if (tid == 0 && !(tr > 0 && tr <= DBL_MAX)) atomicOr(it.flag, 2);       // zero, negative, infinite or NaN
    for (int j = w; j < n; j += 4) {
        const double y = wave_rayleigh(V, A, n, j, lane);
        if (lane == 0) lam[j] = y / tr;
    }
    __syncthreads();
    for (int u = tid; u < n; u += 256) {
        // a NaN ranks last, so the ranks stay a permutation
        it.out[rank_desc(n, u, [&](int v) { const double lv = lam[v]; return lv == lv ? lv : -DBL_MAX; })] = lam[u];
    }
}
void launch_bond_spectrum_finish(hipStream_t s, const BondSpecItem* d_items, int nitems) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL(bond_spectrum_finish_kernel, dim3(nitems), dim3(256), 0, s, d_items); TNQS_CHECK_LAUNCH();
}

}  // namespace tnqs
