// device_common.hpp -- the device-side vocabulary shared by every kernel translation unit: the launch check, vector types, complex numbers,
// wave / workgroup sums, the item lookup of batched launches and the f64 matrix-core tile products.  (mfma_common.hpp adds the MFMA tile machinery on top of it.)
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

// one 16 x 16 complex f64 tile product on v_mfma_f64_16x16x4_f64: lane (l15, kq) supplies A[row i][k0 + kq] = fa(i, k) and B[k0 + kq][column j] = fb(k, j)
template <class FA, class FB> __device__ __forceinline__ void ztile_mm(int K, int i, int j, FA fa, FB fb, v4d& cr, v4d& ci) {
    const int kq = (threadIdx.x & 63) >> 4;
    for (int k0 = 0; k0 < K; k0 += 4) {
        const cx<double> a = fa(i, k0 + kq), b = fb(k0 + kq, j);
        cr = __builtin_amdgcn_mfma_f64_16x16x4f64(a.re, b.re, cr, 0, 0, 0);
        cr = __builtin_amdgcn_mfma_f64_16x16x4f64(-a.im, b.im, cr, 0, 0, 0);
        ci = __builtin_amdgcn_mfma_f64_16x16x4f64(a.re, b.im, ci, 0, 0, 0);
        ci = __builtin_amdgcn_mfma_f64_16x16x4f64(a.im, b.re, ci, 0, 0, 0);
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
        cr = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, br, cr, 0, 0, 0);
        cr = __builtin_amdgcn_mfma_f64_16x16x4f64(-ai, bi, cr, 0, 0, 0);
        ci = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, bi, ci, 0, 0, 0);
        ci = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, br, ci, 0, 0, 0);
    }
}

}  // namespace tnqs
