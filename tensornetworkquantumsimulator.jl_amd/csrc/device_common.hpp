// device_common.hpp -- the device-side vocabulary shared by every kernel translation unit: the launch check, vector types, complex numbers,
// wave / workgroup sums, the item lookup of batched launches, the complex 16x16x4 matrix-core product (CMfma16, cmac16), its split-plane multiply phase (cplane_mm16)
// and the f64 tile products built on it.  (mfma_common.hpp adds the MFMA tile machinery on top of it.)
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>
#include <stdexcept>
#include <string>
#define TNQS_CHECK_LAUNCH() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) throw std::runtime_error(std::string("HIP kernel launch failed (") + __func__ + "): " + hipGetErrorString(e_)); } while (0)

namespace tnqs {

typedef float v16f __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));
typedef double v4d __attribute__((ext_vector_type(4)));

template <class T> struct alignas(2 * sizeof(T)) cx { T re, im; };

template <class T> __device__ __forceinline__ cx<T> cmake(T a, T b) { cx<T> r; r.re = a; r.im = b; return r; }
template <class T> __device__ __forceinline__ void cfma(cx<T>& acc, const cx<T>& a, const cx<T>& b) {
    acc.re = fma(a.re, b.re, acc.re); acc.re = fma(-a.im, b.im, acc.re);
    acc.im = fma(a.re, b.im, acc.im); acc.im = fma(a.im, b.re, acc.im);
}
// acc += a * conj(b)
template <class T> __device__ __forceinline__ void cfma_conj(cx<T>& acc, const cx<T>& a, const cx<T>& b) {
    acc.re = fma(a.re, b.re, acc.re); acc.re = fma(a.im, b.im, acc.re);
    acc.im = fma(a.im, b.re, acc.im); acc.im = fma(-a.re, b.im, acc.im);
}
template <class T> __device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
template <class T> __device__ __forceinline__ T eps_of();
template <> __device__ __forceinline__ float eps_of<float>() { return FLT_EPSILON; }
template <> __device__ __forceinline__ double eps_of<double>() { return DBL_EPSILON; }

// block-wide sum of a double (blockDim.x <= 1024); result valid in every thread
__device__ __forceinline__ double block_sum(double v, double* sh /* >= 17 doubles */) {
    v = wave_sum(v);
    int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (lane == 0) sh[w] = v;
    __syncthreads();
    if (threadIdx.x == 0) { double t = 0; for (int i = 0; i < nw; ++i) t += sh[i]; sh[16] = t; }
    __syncthreads();
    return sh[16];
}

// the item of a batched launch that owns workgroup (tile, chunk, element) `id`: the last one whose `begin` is <= id
template <class Item> __device__ __forceinline__ int find_item(const Item* __restrict__ items, int nitems, int Item::*begin, int id) {
    int lo = 0, hi = nitems - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (items[mid].*begin <= id) lo = mid; else hi = mid - 1; }
    return lo;
}

// the two 16x16x4 matrix instructions (v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64): lane (c = lane & 15, g = lane >> 4) supplies A[row c][k = g] and B[k = g][column c]
// and holds C / D[row(g, r)][column c] in register r.  TN, LD: the block of contracted indices and the LDS pitch of the split-plane kernels (cplane_mm16)
template <class T> struct CMfma16;
template <> struct CMfma16<float> {
    using Acc = v4f; static constexpr int TN = 32, LD = 36;      // LD: 16 rows x 4 contraction indices of an operand read fall into 64 distinct banks
    static __device__ __forceinline__ Acc mma(float a, float b, Acc c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int row(int g, int r) { return 4 * g + r; }
};
template <> struct CMfma16<double> {
    using Acc = v4d; static constexpr int TN = 16, LD = 18;
    static __device__ __forceinline__ Acc mma(double a, double b, Acc c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int row(int g, int r) { return g + 4 * r; }      // the f64 instruction's own C / D map
};
// one complex rank-4 update as four real ones, c += a b (CONJ: c += a conj(b)).  The instruction order is part of the contract (results are kept bit for bit):
//   plain       ar br, -ai bi -> re;  ar bi,  ai br -> im
//   conjugated  ar br,  ai bi -> re;  ai br, -ar bi -> im
template <bool CONJ, class T> __device__ __forceinline__ void cmac16(T ar, T ai, T br, T bi, typename CMfma16<T>::Acc& cr, typename CMfma16<T>::Acc& ci) {
    using M = CMfma16<T>;
    if constexpr (CONJ) { cr = M::mma(ar, br, cr); cr = M::mma(ai, bi, cr); ci = M::mma(ai, br, ci); ci = M::mma(-ar, bi, ci); }
    else { cr = M::mma(ar, br, cr); cr = M::mma(-ai, bi, cr); ci = M::mma(ar, bi, ci); ci = M::mma(ai, br, ci); }
}

// the multiply phase of the split-plane kernels (4 waves): one block of TN contracted indices, operands in LDS as (re, im) planes [row][k] of pitch LD.  The live
// 16 x 16 tiles of the nta x (ntiles / nta) grid are dealt round robin to the waves: tile t = w + 4 u = (ta = t % nta rows of x, tb = t / nta rows of y) goes into
// cr[u], ci[u] as x y (CONJ: x conj(y)); A[i = row of x][k], B[k][j = row of y]
template <bool CONJ, class T> __device__ __forceinline__ void cplane_mm16(const T* xr, const T* xi, const T* yr, const T* yi, int nta, int ntiles,
                                                                          typename CMfma16<T>::Acc (&cr)[4], typename CMfma16<T>::Acc (&ci)[4]) {
    constexpr int TN = CMfma16<T>::TN, LD = CMfma16<T>::LD;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int t = w + 4 * u;
        if (t < ntiles) {                                  // (uniform in the wave)
            const int ta = t % nta, tb = t / nta;
            const int xo = (16 * ta + c) * LD + g, yo = (16 * tb + c) * LD + g;
#pragma unroll
            for (int ks = 0; ks < TN / 4; ++ks) cmac16<CONJ>(xr[xo + 4 * ks], xi[xo + 4 * ks], yr[yo + 4 * ks], yi[yo + 4 * ks], cr[u], ci[u]);
        }
    }
}

// one 16 x 16 complex f64 tile product: lane (l15, kq) supplies A[row i][k0 + kq] = fa(i, k) and B[k0 + kq][column j] = fb(k, j)
template <class FA, class FB> __device__ __forceinline__ void ztile_mm(int K, int i, int j, FA fa, FB fb, v4d& cr, v4d& ci) {
    const int kq = (threadIdx.x & 63) >> 4;
    for (int k0 = 0; k0 < K; k0 += 4) {
        const cx<double> a = fa(i, k0 + kq), b = fb(k0 + kq, j);
        cmac16<false>(a.re, a.im, b.re, b.im, cr, ci);
    }
}

// the same tile product for FULL tiles with complex f32 operands in LDS (no guards, loads hoisted by unrolling): this lane supplies A[row l15][k] = ap[k * as]
// (conjugated when CA) and B[k][column l15] = bp[k * bs]; K a multiple of 4
template <bool CA> __device__ __forceinline__ void tile_mm_f32(const cx<float>* ap, int as, const cx<float>* bp, int bs, int K, v4d& cr, v4d& ci) {
    const int kq = (threadIdx.x & 63) >> 4;
    ap += kq * as; bp += kq * bs;
#pragma unroll 4
    for (int k0 = 0; k0 < K; k0 += 4) {
        const cx<float> a = ap[k0 * as], b = bp[k0 * bs];
        const double ar = a.re, ai = CA ? -(double)a.im : (double)a.im, br = b.re, bi = b.im;
        cmac16<false>(ar, ai, br, bi, cr, ci);
    }
}

}  // namespace tnqs
