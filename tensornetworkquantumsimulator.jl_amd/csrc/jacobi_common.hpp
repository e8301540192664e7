// jacobi_common.hpp -- the numerical pieces the factorisation kernels share, each written once: the round-robin pair schedule and the plane rotation
// of the one-sided Jacobi kernels (kernels_svd.hip), the power-of-two scaling exponent, the ranking of singular values (also kernels_theta / _bp /
// _spectrum.hip), and the triangular numbering and largest diagonal entry of the Cholesky kernels (kernels_chol.hip, theta_svd_pre_kernel).
#pragma once
#include "device_common.hpp"

namespace tnqs {

// Rotation parameters.  f32: the hardware reciprocal (square root).  f64: the compiler's IEEE sqrt and division are ~55 dependent
// instructions each, and a Jacobi round has three of each on its critical path (most of the 1.2 us per round of the f64 kernels); the
// hardware seeds (v_rsq_f64 / v_rcp_f64, ~2^-23 relative) with two Newton steps are ~8 instructions and good to a few ulp, which is all
// a plane rotation needs (c^2 + s^2 = 1 to 1e-15).  Arguments are normal, positive numbers here (see the guards on g2).
template <class T> __device__ __forceinline__ T fast_rsqrt(T x);
template <> __device__ __forceinline__ float fast_rsqrt<float>(float x) { return __frsqrt_rn(x); }
template <> __device__ __forceinline__ double fast_rsqrt<double>(double x) {
    double y = __builtin_amdgcn_rsq(x);
    double h = x * y; y = y * (1.5 - 0.5 * h * y);
    h = x * y; y = y * (1.5 - 0.5 * h * y);
    return y;
}
template <class T> __device__ __forceinline__ T fast_rcp(T x);
template <> __device__ __forceinline__ float fast_rcp<float>(float x) { return __frcp_rn(x); }
template <> __device__ __forceinline__ double fast_rcp<double>(double x) {
    double y = __builtin_amdgcn_rcp(x);
    y = y * (2.0 - x * y); y = y * (2.0 - x * y);
    return y;
}
template <class T> __device__ __forceinline__ T fast_sqrt(T x);          // x >= 1 at the call sites
template <> __device__ __forceinline__ float fast_sqrt<float>(float x) { return sqrtf(x); }
template <> __device__ __forceinline__ double fast_sqrt<double>(double x) { return x * fast_rsqrt<double>(x); }

// round-robin ordering of the ne (even) columns: the pair (p < q) that slot 0 <= slot < ne / 2 plays in round 0 <= round < ne - 1; every column is in exactly one
// pair of a round.  (round + slot < 2 (ne - 1), so one conditional subtraction is the remainder modulo ne - 1.)
__device__ __forceinline__ void jacobi_pair(int ne, int round, int slot, int& p, int& q) {
    if (slot == 0) { p = ne - 1; q = round; }
    else { p = round + slot; if (p >= ne - 1) p -= ne - 1; q = round - slot; if (q < 0) q += ne - 1; }
    if (p > q) { int t = p; p = q; q = t; }
}
// the rotation that orthogonalises columns a_p, a_q: alpha = |a_p|^2, beta = |a_q|^2, (gre, gim) = <a_p, a_q>, g2 = gre^2 + gim^2 (normal and positive: the
// callers decide whether to rotate at all).  (pre, pim) = e^{-i phi}; the operations and their order are part of the contract (results are kept bit for bit)
template <class T> struct JacobiRot { T pre, pim, c, sn; };
template <class T> __device__ __forceinline__ JacobiRot<T> jacobi_rotation(T alpha, T beta, T gre, T gim, T g2) {
    const T iga = fast_rsqrt<T>(g2);
    const T pre = gre * iga, pim = -gim * iga;
    const T zeta = (beta - alpha) * (T)0.5 * iga;
    const T az = fabs(zeta);
    const T t = (zeta >= 0 ? (T)1 : (T)-1) * fast_rcp<T>(az + fast_sqrt<T>(1 + az * az));
    const T c = fast_rsqrt<T>(1 + t * t), sn = c * t;
    return JacobiRot<T>{pre, pim, c, sn};
}
// one row of the rotated column pair: (op, oq) = (c ap - sn e^{-i phi} aq, sn ap + c e^{-i phi} aq); op, oq may be where ap, aq came from
template <class T> __device__ __forceinline__ void jacobi_rotate(const JacobiRot<T>& R, cx<T> ap, cx<T> aq, cx<T>& op, cx<T>& oq) {
    const T qre = aq.re * R.pre - aq.im * R.pim, qim = aq.re * R.pim + aq.im * R.pre;
    op = cmake<T>(R.c * ap.re - R.sn * qre, R.c * ap.im - R.sn * qim);
    oq = cmake<T>(R.sn * ap.re + R.c * qre, R.sn * ap.im + R.c * qim);
}

// k with 2^(2k) ||A||_F^2 = O(1) (fro = ||A||_F^2), clamped so that 2^k and 2^-k are normal f32 numbers; 0 for a zero or non-finite norm
__device__ __forceinline__ int pow2_exponent(double fro) {
    int kexp = 0;
    if (fro > 0 && fro < 1e300) { kexp = -(ilogb(fro) / 2); kexp = kexp > 120 ? 120 : (kexp < -120 ? -120 : kexp); }
    return kexp;
}

// rank by counting, descending and stable: the position of entry j among key(0) .. key(n - 1), equal keys in index order (the tie rule is part of the contract:
// two kernels that rank the same keys agree).  The ranks of 0 .. n - 1 are a permutation as long as no key is a NaN.
template <class Key> __device__ __forceinline__ int rank_desc(int n, int j, Key key) {
    int rk = 0; const auto kj = key(j);
    for (int v = 0; v < n; ++v) { const auto kv = key(v); rk += (kv > kj) || (kv == kj && v < j); }
    return rk;
}
template <class K> __device__ __forceinline__ int rank_desc(const K* keys, int n, int j) { return rank_desc(n, j, [keys](int v) { return keys[v]; }); }

// row-major triangular numbering e = r (r + 1) / 2 + c, 0 <= c <= r.  It is NESTED: the first m (m + 1) / 2 numbers are the triangle of size m.
__device__ __forceinline__ void tri_decode(int e, int& r, int& c) {
    int t = (int)((sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);
    while (t * (t + 1) / 2 > e) --t;
    while ((t + 1) * (t + 2) / 2 <= e) ++t;
    r = t; c = e - t * (t + 1) / 2;
}

// the largest of diag(0) .. diag(n - 1) and 0, found by the first wave and handed to every thread through *sh (LDS); ends with a workgroup barrier
template <class Diag> __device__ __forceinline__ double max_diag(int n, Diag diag, double* sh) {
    if (threadIdx.x < 64) {
        double m = 0; for (int i = threadIdx.x; i < n; i += 64) m = fmax(m, diag(i));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
        if (threadIdx.x == 0) *sh = m;
    }
    __syncthreads();
    return *sh;
}

}  // namespace tnqs
