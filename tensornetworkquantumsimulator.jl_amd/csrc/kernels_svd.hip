// kernels_svd.hip -- one-sided Jacobi SVD / eigen factorisations: the global-memory and the LDS-resident kernel, the preconditioned theta SVD,
// recovery of V, and the prepare / finish pair of the small sites.  What the sweeps of the three Jacobi kernels share is in jacobi_common.hpp: the pair
// schedule (jacobi_pair), the rotation (jacobi_rotation, jacobi_rotate), the scaling exponent (pow2_exponent) and the ranking (rank_desc); so are the triangular
// numbering (tri_decode) and the largest pivot (max_diag) that theta_svd_pre_kernel shares with kernels_chol.hip.  The sweep loop itself is written out in each
// of the three sweep functions: a shared driver taking the round as a callable cost registers.
// Reference call sites replaced (paths relative to the reference repo):
//   jacobi      : `eigen` (src/utils.jl:29-35,94-108) and `factorize_svd` (simple_update.jl:53-59)
#include "kernels.hpp"
#include "device_common.hpp"
#include "jacobi_common.hpp"
#include "launch_util.hpp"

namespace tnqs {

// ------------------------------------------------------------------------------------------------------------
// one-sided (Hestenes) Jacobi: A <- A J_1 J_2 ..., V <- V J_1 J_2 ...  until the columns of A are orthogonal.
// One workgroup per matrix, one wave per column pair, round-robin pair ordering.  m <= 64 R (R = 4 or 8: up to 512 rows), any n.
// ------------------------------------------------------------------------------------------------------------
template <class T, int R>          // R rows per lane: m <= 64 R
__global__ __launch_bounds__(1024) void jacobi_kernel(const JacobiItem* __restrict__ items, int max_sweeps) {
    __shared__ int s_rot;
    const JacobiItem it = items[blockIdx.x];
    if (it.only_if && *it.only_if == 0) return;          // conditional item (svd_batch: polishing sweeps only where the preprocessing failed)
    if (it.pre && theta_pre_takes(it.dyn, it.dm, it.dn, it.QB != nullptr)) return;      // taken by theta_svd_pre_kernel
    cx<T>* A = reinterpret_cast<cx<T>*>(it.A);
    cx<T>* V = reinterpret_cast<cx<T>*>(it.V);
    int m_ = it.m, n_ = it.n;
    if (it.dyn) { int nf; theta_dims(it.dyn, it.dm, it.dn, m_, nf, n_); }
    const int m = m_, n = n_;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int ne = n + (n & 1);
    // (f32: 2 eps, see jacobi_lds_sweeps)
    const T tol = eps_of<T>() * (sizeof(T) == 4 ? (T)2 : sqrt((T)(m > 4 ? m : 4)));
    // scale to ||A||_F = O(1) by an exact power of two for the sweeps (see jacobi_lds_kernel: squared inner products underflow in f32)
    __shared__ double s_redg[17];
    double frog = 0;
    for (int e = threadIdx.x; e < m * n; e += blockDim.x) { cx<T> v = A[e]; frog += (double)v.re * v.re + (double)v.im * v.im; }
    frog = block_sum(frog, s_redg);
    const int kexp = pow2_exponent(frog);
    const T sc_in = (T)ldexp(1.0, kexp), sc_out = (T)ldexp(1.0, -kexp);
    if (kexp != 0) { for (int e = threadIdx.x; e < m * n; e += blockDim.x) { cx<T> v = A[e]; A[e] = cmake<T>(v.re * sc_in, v.im * sc_in); } }
    __syncthreads();
    int sweep = 0;
    for (; sweep < max_sweeps && n > 1; ++sweep) {
        if (threadIdx.x == 0) s_rot = 0;
        __syncthreads();
        for (int round = 0; round < ne - 1; ++round) {
            for (int pi = w; pi < ne / 2; pi += nw) {
                int p, q; jacobi_pair(ne, round, pi, p, q);
                if (q >= n) continue;
                cx<T> ap[R], aq[R];
                T alpha = 0, beta = 0, gre = 0, gim = 0;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    int i = lane + 64 * r;
                    if (i < m) {
                        ap[r] = A[i + (size_t)m * p]; aq[r] = A[i + (size_t)m * q];
                        alpha += ap[r].re * ap[r].re + ap[r].im * ap[r].im;
                        beta += aq[r].re * aq[r].re + aq[r].im * aq[r].im;
                        gre += ap[r].re * aq[r].re + ap[r].im * aq[r].im;     // conj(ap) * aq
                        gim += ap[r].re * aq[r].im - ap[r].im * aq[r].re;
                    }
                }
                alpha = wave_sum(alpha); beta = wave_sum(beta); gre = wave_sum(gre); gim = wave_sum(gim);
                const T g2 = gre * gre + gim * gim;
                if (g2 > (sizeof(T) == 4 ? (T)1e-36 : (T)1e-290) && g2 > tol * tol * alpha * beta) {      // (g2 normal: see fast_rsqrt)
                    const JacobiRot<T> rot = jacobi_rotation(alpha, beta, gre, gim, g2);
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        int i = lane + 64 * r;
                        if (i < m) jacobi_rotate(rot, ap[r], aq[r], A[i + (size_t)m * p], A[i + (size_t)m * q]);
                    }
                    if (V)
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        int i = lane + 64 * r;
                        if (i < n) { cx<T>& vp = V[i + (size_t)n * p]; cx<T>& vq = V[i + (size_t)n * q]; jacobi_rotate(rot, vp, vq, vp, vq); }
                    }
                    if (lane == 0) s_rot = 1;
                }
            }
            __syncthreads();
        }
        const int rot = s_rot;
        __syncthreads();
        if (!rot) { ++sweep; break; }
    }
    __syncthreads();
    if (kexp != 0) { for (int e = threadIdx.x; e < m * n; e += blockDim.x) { cx<T> v = A[e]; A[e] = cmake<T>(v.re * sc_out, v.im * sc_out); } }
    if (threadIdx.x == 0 && it.sweeps_out) *it.sweeps_out = sweep;
}
// LDS-resident variant: A (and V when it fits / is wanted) live in LDS for the whole factorisation; global memory is
// touched twice.  it.V == nullptr: rotations are not accumulated (the caller recovers V = A0^dagger (U Sigma) Sigma^-2).
// A QUARTER wave (16 lanes) owns one column pair, so a 16-wave workgroup rotates 64 pairs at once (one full round of a
// 128-column matrix); the dot products reduce inside 16-lane rows.  Columns are padded by 2 elements so the four
// quarter-waves of a wave hit different LDS banks.
// all-reduce over a 16-lane row with DPP row rotations (VALU, no LDS crossbar): after adding the rotations by 8, 4, 2, 1 every lane
// holds the row sum (the same summation tree in every lane of the row, so the four quarter-waves' decisions stay uniform per row)
template <int ROR> __device__ __forceinline__ float dpp_ror_f(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x120 + ROR, 0xf, 0xf, false));
}
template <int ROR> __device__ __forceinline__ double dpp_ror_d(double v) {
    long long b = __builtin_bit_cast(long long, v);
    int lo = (int)(b & 0xffffffffll), hi = (int)(b >> 32);
    lo = __builtin_amdgcn_update_dpp(0, lo, 0x120 + ROR, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(0, hi, 0x120 + ROR, 0xf, 0xf, false);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ float row16_sum(float v) {
    v += dpp_ror_f<8>(v); v += dpp_ror_f<4>(v); v += dpp_ror_f<2>(v); v += dpp_ror_f<1>(v);
    return v;
}
__device__ __forceinline__ double row16_sum(double v) {
    v += dpp_ror_d<8>(v); v += dpp_ror_d<4>(v); v += dpp_ror_d<2>(v); v += dpp_ror_d<1>(v);
    return v;
}
// the sweeps of the LDS-resident factorisation.  FULL: m == 16*RQ, n even and n/2 a multiple of 4 -- every quarter-wave of every
// participating wave owns a real pair and all RQ row slots are real rows, so the per-row / per-pair guards (exec-mask juggling in the
// hottest loop) disappear.
template <class T, int RQ, bool FULL>
__device__ __forceinline__ int jacobi_lds_sweeps(cx<T>* A, cx<T>* V, bool hasV, int m, int n, int mp, int np_, int max_sweeps, T tiny, int* s_rot) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int grp = lane >> 4, l16 = lane & 15;
    const int ne = n + (n & 1);
    const int nslots = 4 * nw;
    // Convergence threshold on |<a_p, a_q>| / (|a_p| |a_q|).  f64: eps sqrt(m), the worst-case rounding bound of the inner product.  f32: 2 eps -- the
    // rounding noise of an m-term inner product of nearly orthogonal columns is ~eps / sqrt(m) of |a_p| |a_q| (random signs), so 2 eps is still 20 x
    // above it, and the looser eps sqrt(m) = 1.3e-6 (rounds 1-3) left the singular vectors an order of magnitude less orthogonal than LAPACK's:
    // measured on a ten-layer chi = 32 evolution, <Z> drifted 1-3e-5 from the ComplexF64 run with the old threshold and 1-3e-6 with this one (the
    // oracle's own f32 run: 1-4e-6), for 8.1 instead of 7.1 sweeps per gate.
    const T tol = eps_of<T>() * (sizeof(T) == 4 ? (T)2 : sqrt((T)(m > 4 ? m : 4)));
    const int rq = (m + 15) >> 4, rqv = (n + 15) >> 4;
    int sweep = 0;
    for (; sweep < max_sweeps && n > 1; ++sweep) {
        if (threadIdx.x == 0) *s_rot = 0;
        __syncthreads();
        for (int round = 0; round < ne - 1; ++round) {
            for (int base = 4 * w; base < ne / 2; base += nslots) {
                // wave-uniform trip count (the row reductions need all four quarter-waves); idle quarters are predicated off
                const int pi = base + grp;
                int p = 0, q = 0; bool act = FULL || pi < ne / 2;
                if (act) { jacobi_pair(ne, round, pi, p, q); if (!FULL) act = q < n; }
                cx<T> ap[RQ], aq[RQ];
                T alpha = 0, beta = 0, gre = 0, gim = 0;
#pragma unroll
                for (int r = 0; r < RQ; ++r) {
                    int i = l16 + 16 * r;
                    if (FULL || (r < rq && act && i < m)) {
                        ap[r] = A[i + mp * p]; aq[r] = A[i + mp * q];
                        alpha += ap[r].re * ap[r].re + ap[r].im * ap[r].im;
                        beta += aq[r].re * aq[r].re + aq[r].im * aq[r].im;
                        gre += ap[r].re * aq[r].re + ap[r].im * aq[r].im;
                        gim += ap[r].re * aq[r].im - ap[r].im * aq[r].re;
                    }
                }
                alpha = row16_sum(alpha); beta = row16_sum(beta); gre = row16_sum(gre); gim = row16_sum(gim);
                const T g2 = gre * gre + gim * gim;
                // f32: g2 must be a NORMAL number -- the fast reciprocal square root returns inf for (flushed) denormals
                if (act && g2 > (sizeof(T) == 4 ? (T)1e-36 : (T)1e-290) && g2 > tol * tol * alpha * beta && !(alpha < tiny && beta < tiny)) {
                    const JacobiRot<T> rot = jacobi_rotation(alpha, beta, gre, gim, g2);
#pragma unroll
                    for (int r = 0; r < RQ; ++r) {
                        int i = l16 + 16 * r;
                        if (FULL || (r < rq && i < m)) jacobi_rotate(rot, ap[r], aq[r], A[i + mp * p], A[i + mp * q]);
                    }
                    if (hasV) {
#pragma unroll
                        for (int r = 0; r < RQ; ++r) {
                            int i = l16 + 16 * r;
                            if (r < rqv && i < n) { cx<T>& vp = V[i + np_ * p]; cx<T>& vq = V[i + np_ * q]; jacobi_rotate(rot, vp, vq, vp, vq); }
                        }
                    }
                    if (l16 == 0) *s_rot = 1;
                }
            }
            __syncthreads();
        }
        const int rotd = *s_rot;
        __syncthreads();
        if (!rotd) { ++sweep; break; }
    }
    return sweep;
}
// ComplexF32, full tiles: the same sweeps written on (re, im) pairs so that the compiler emits packed f32 operations
// (v_pk_fma_f32 with operand swizzles): 10 packed operations per row instead of ~22
template <int RQ>
__device__ __forceinline__ int jacobi_lds_sweeps_f32_full(cx<float>* A, int m, int n, int mp, int max_sweeps, float tiny, int* s_rot) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int grp = lane >> 4, l16 = lane & 15;
    const int ne = n;                                   // n is even here
    const int nslots = 4 * nw;
    const float tol = eps_of<float>() * 2.0f;                       // (see jacobi_lds_sweeps)
    v2f* Av = reinterpret_cast<v2f*>(A);
    int sweep = 0;
    for (; sweep < max_sweeps && n > 1; ++sweep) {
        if (threadIdx.x == 0) *s_rot = 0;
        __syncthreads();
        for (int round = 0; round < ne - 1; ++round) {
            for (int base = 4 * w; base < ne / 2; base += nslots) {
                int p, q; jacobi_pair(ne, round, base + grp, p, q);
                v2f* cp = Av + l16 + mp * p; v2f* cq = Av + l16 + mp * q;
                v2f ap[RQ], aq[RQ];
                v2f sa = {0.f, 0.f}, sb = {0.f, 0.f}, g1 = {0.f, 0.f}, g2v = {0.f, 0.f};
#pragma unroll
                for (int r = 0; r < RQ; ++r) {
                    ap[r] = cp[16 * r]; aq[r] = cq[16 * r];
                    sa += ap[r] * ap[r]; sb += aq[r] * aq[r];
                    g1 += ap[r] * aq[r];
                    g2v += ap[r] * __builtin_shufflevector(aq[r], aq[r], 1, 0);
                }
                float alpha = row16_sum(sa.x + sa.y), beta = row16_sum(sb.x + sb.y), gre = row16_sum(g1.x + g1.y), gim = row16_sum(g2v.x - g2v.y);
                const float g2 = gre * gre + gim * gim;
                if (g2 > 1e-36f && g2 > tol * tol * alpha * beta && !(alpha < tiny && beta < tiny)) {
                    const JacobiRot<float> rot = jacobi_rotation(alpha, beta, gre, gim, g2);
                    const v2f e1 = {rot.pre, rot.pim}, e2 = {-rot.pim, rot.pre}, cc = {rot.c, rot.c}, ss = {rot.sn, rot.sn};
#pragma unroll
                    for (int r = 0; r < RQ; ++r) {
                        const v2f qv = __builtin_shufflevector(aq[r], aq[r], 0, 0) * e1 + __builtin_shufflevector(aq[r], aq[r], 1, 1) * e2;
                        cp[16 * r] = cc * ap[r] - ss * qv;
                        cq[16 * r] = ss * ap[r] + cc * qv;
                    }
                    if (l16 == 0) *s_rot = 1;
                }
            }
            __syncthreads();
        }
        const int rotd = *s_rot;
        __syncthreads();
        if (!rotd) { ++sweep; break; }
    }
    return sweep;
}
template <class T, int RQ>              // RQ = rows per lane: m <= 16*RQ
__global__ __launch_bounds__(1024) void jacobi_lds_kernel(const JacobiItem* __restrict__ items, int max_sweeps) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_rot;
    const JacobiItem it = items[blockIdx.x];
    if (it.pre && theta_pre_takes(it.dyn, it.dm, it.dn, it.QB != nullptr)) return;      // taken by theta_svd_pre_kernel
    cx<T>* Ag = reinterpret_cast<cx<T>*>(it.A);
    cx<T>* Vg = reinterpret_cast<cx<T>*>(it.V);
    int m_ = it.m, n_ = it.n;
    if (it.dyn) { int nf; theta_dims(it.dyn, it.dm, it.dn, m_, nf, n_); }      // dimensions found on the device (JacobiItem::dyn)
    const int m = m_, n = n_;
    const int mp = m + 2, np_ = n + 2;     // padded column pitches
    cx<T>* A = reinterpret_cast<cx<T>*>(smem);
    cx<T>* V = A + (size_t)mp * n;
    const bool hasV = Vg != nullptr;
    // Without V the order of the columns is free (the caller ranks the singular values itself): they enter the sweeps sorted by decreasing
    // norm (de Rijk), which the cyclic sweeps converge from in fewer passes than from an arbitrary order
    __shared__ float s_cn[256]; __shared__ unsigned char s_pos[256];
    const bool sorted = !hasV && n <= 256 && n > 2;
    if (sorted) {
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
        for (int j = w; j < n; j += nw) {
            float s2 = 0.f;
            for (int i = lane; i < m; i += 64) { const cx<T> v = Ag[i + (size_t)m * j]; s2 += (float)v.re * (float)v.re + (float)v.im * (float)v.im; }
            s2 = wave_sum(s2);
            if (lane == 0) s_cn[j] = s2 == s2 ? s2 : 0.f;
        }
        __syncthreads();
        for (int j = threadIdx.x; j < n; j += blockDim.x) s_pos[j] = (unsigned char)rank_desc(s_cn, n, j);
        __syncthreads();
        for (int e = threadIdx.x; e < m * n; e += blockDim.x) A[(e % m) + mp * (int)s_pos[e / m]] = Ag[e];
    } else
    for (int e = threadIdx.x; e < m * n; e += blockDim.x) A[(e % m) + mp * (e / m)] = Ag[e];
    if (hasV) for (int e = threadIdx.x; e < n * n; e += blockDim.x) V[(e % n) + np_ * (e / n)] = cmake<T>((e % n) == (e / n) ? (T)1 : (T)0, (T)0);
    __syncthreads();
    // ||A||_F^2 is invariant under the rotations.  A pair of columns that are BOTH below n eps^2 ||A||_F^2 (singular values under
    // ~sqrt(n) eps ||A||_F: rounding noise of a rank-deficient matrix) is left alone -- otherwise noise columns keep rotating
    // against each other for many sweeps without changing any singular value that matters.
    __shared__ double s_red[17];
    double fro = 0;
    for (int e = threadIdx.x; e < m * n; e += blockDim.x) { cx<T> v = A[(e % m) + mp * (e / m)]; fro += (double)v.re * v.re + (double)v.im * v.im; }
    fro = block_sum(fro, s_red);
    // The sweeps square inner products (g^2, alpha*beta): in f32 that underflows for a matrix of small magnitude (theta of a state whose
    // tensors carry a small norm: singular values 1e-5 already put the products of the smaller columns into the denormal range, the
    // rotation phases lose their unit modulus and the "rotations" stop being unitary).  The matrix is therefore scaled by an exact power
    // of two to ||A||_F = O(1) for the sweeps and scaled back when it is written out; V does not change.
    const int kexp = pow2_exponent(fro);
    const T sc_in = (T)ldexp(1.0, kexp), sc_out = (T)ldexp(1.0, -kexp);
    if (kexp != 0) {
        for (int e = threadIdx.x; e < m * n; e += blockDim.x) { cx<T>& v = A[(e % m) + mp * (e / m)]; v.re *= sc_in; v.im *= sc_in; }
        fro = ldexp(fro, 2 * kexp);
        __syncthreads();
    }
    const T tiny = (T)((double)n * (double)eps_of<T>() * (double)eps_of<T>() * fro);
    const bool full = (m == 16 * RQ) && !(n & 1) && !((n >> 1) & 3);
    int sweep;
    if (full && sizeof(T) == 4 && !hasV) sweep = jacobi_lds_sweeps_f32_full<RQ>(reinterpret_cast<cx<float>*>(A), m, n, mp, max_sweeps, (float)tiny, &s_rot);
    else if (full) sweep = jacobi_lds_sweeps<T, RQ, true>(A, V, hasV, m, n, mp, np_, max_sweeps, tiny, &s_rot);
    else sweep = jacobi_lds_sweeps<T, RQ, false>(A, V, hasV, m, n, mp, np_, max_sweeps, tiny, &s_rot);
    __syncthreads();
    for (int e = threadIdx.x; e < m * n; e += blockDim.x) { cx<T> v = A[(e % m) + mp * (e / m)]; Ag[e] = cmake<T>(v.re * sc_out, v.im * sc_out); }
    if (hasV) for (int e = threadIdx.x; e < n * n; e += blockDim.x) Vg[e] = V[(e % n) + np_ * (e / n)];
    if (threadIdx.x == 0 && it.sweeps_out) *it.sweeps_out = sweep;
}

// ------------------------------------------------------------------------------------------------------------
// Preconditioned theta SVD (round 5): ComplexF32, V not wanted, tall or square A (m >= n), n <= 64, m <= 128 -- the 128 x 64 low-rank factor
// of a chi = 32 gate and every smaller theta.  ONE workgroup per gate, everything in LDS:
//   1. A -> LDS, columns sorted by decreasing norm (de Rijk), scaled to ||A||_F = O(1) by a power of two;
//   2. G = A^dagger A in f64 (f32 products are exact in f64: G is the exact Gram matrix of the rounded A);
//   3. G = L L^dagger, right-looking Cholesky with one barrier per column (a collapsed pivot -- A rank deficient, the normal case early in
//      an evolution -- is replaced by 1e-13 of the largest one: directions below 3e-7 sigma_max are f32 noise of A anyway);
//   4. one-sided Jacobi on the COLUMNS OF L (n x n, f32): L J = U_L Sigma.  L = R^dagger of the QR factorisation of A: orthogonalising the rows
//      of R instead of the columns of A is the Drmac-Veselic preconditioning -- the sorted triangular factor is graded, L^dagger L is much
//      closer to diagonal than A^dagger A: 4-5 sweeps instead of 8 on the thetas of the benchmark (scratch numpy model: oracle thetas of a 4 x 4
//      chi = 32 lattice, 7-9 -> 3-5; evolved chi = 16 states, 7-8 -> 5-7), and each sweep rotates n rows instead of m;
//   5. A^dagger A = L L^dagger = U_L Sigma^2 U_L^dagger: the normalised columns of L J ARE the right singular vectors of A, so
//      U Sigma = A U_L -- an (m x n)(n x n) product accumulated in f64 -- goes back to global memory where the rotated A used to go.
// No inverse of R, no accumulated rotations.  What the kernel replaces took 0.46-0.81 ms per colour batch (8.1 sweeps x 63 rounds on 128 rows).
// ------------------------------------------------------------------------------------------------------------
template <int NT>
__global__ __launch_bounds__(NT) void theta_svd_pre_kernel(const JacobiItem* __restrict__ items, int max_sweeps) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_rot;
    __shared__ double s_red[17];
    __shared__ double s_cn[64]; __shared__ double s_piv[64]; __shared__ unsigned char s_pos[64]; __shared__ unsigned char s_perm[64];
    __shared__ double s_dmax; __shared__ double s_sig[64]; __shared__ int s_bad;
    // it.V is never an output here (V is not accumulated); the kernel tests pass a buffer of 8 x 64-bit slots that receives the constant-rate clock at the
    // phase boundaries (engine: null)
#define PRE_STAMP(k) do { if (tstamp && threadIdx.x == 0) tstamp[k] = wall_clock64(); } while (0)
    const JacobiItem it = items[blockIdx.x];
    unsigned long long* tstamp = reinterpret_cast<unsigned long long*>(it.V);
    cx<float>* Ag = reinterpret_cast<cx<float>*>(it.A);
    int m_ = it.m, n_ = it.n;
    if (it.dyn) { int nf; theta_dims(it.dyn, it.dm, it.dn, m_, nf, n_); }
    const int m = m_, n = n_, tid = threadIdx.x;
    const int lane = tid & 63, w = tid >> 6, nw = NT >> 6;
    PRE_STAMP(0);
    // pre != 0 (engine): the item is taken only when the low-rank route survived on the device and its factor fits (theta_pre_takes); the plain Jacobi
    // kernel launched next to this one makes the complementary decision.  pre == 0 (kernel tests): the dimensions given decide
    if (it.pre ? !theta_pre_takes(it.dyn, it.dm, it.dn, it.QB != nullptr) : (n < 2 || m < n || n > 64 || m > 128)) return;
    const int mp = m + 2, gp = n + 1, xp = n + 2;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    cx<float>* Mf = reinterpret_cast<cx<float>*>(smem);                                   // sorted A, column a at mp * a
    const size_t m_bytes = (((size_t)mp * n * sizeof(cx<float>)) + 15) & ~(size_t)15;
    cx<double>* Gd = reinterpret_cast<cx<double>*>(smem + m_bytes);                      // G / L (lower triangle), element (i, j) at i + gp * j
    cx<float>* X = reinterpret_cast<cx<float>*>(smem + m_bytes);                         // later: L in f32, column k at xp * k (over the start of Gd)
    // ---- 1. column norms (first pass over A: 64 KiB, L2 resident afterwards), de Rijk order, SORTED load (column a of the LDS copy = column s_perm[a] of A);
    // the power-of-two scaling is applied to G (exactly) instead of to the entries ------------------------------------------------------------------
    for (int j = w; j < n; j += nw) {
        double s2 = 0;
        for (int i = lane; i < m; i += 64) { const cx<float> v = Ag[i + (size_t)m * j]; s2 += (double)v.re * v.re + (double)v.im * v.im; }
        s2 = wave_sum(s2);
        if (lane == 0) { s_cn[j] = s2 == s2 ? s2 : 0.0; if (!(s2 == s2) || s2 > 1e300) s_bad = 1; }
    }
    __syncthreads();
    for (int j = tid; j < n; j += NT) { const int rk = rank_desc(s_cn, n, j); s_pos[j] = (unsigned char)rk; s_perm[rk] = (unsigned char)j; }
    double fro = 0; for (int j = tid; j < n; j += NT) fro += s_cn[j];
    fro = block_sum(fro, s_red);                                                         // (also orders s_pos before the load below)
    // Degenerate input (round-5 advisor finding).  theta identically ZERO: its SVD is U Sigma = 0 -- A stays as it is, V = 0; before this guard the largest
    // Cholesky pivot was 0, every pivot was replaced by 1, L became the identity and the unformed columns left as sigma_j e_0 with sigma = 1: weight in S and in
    // the truncation error that the matrix does not have.  A NaN / infinite entry: the column norm was mapped to 0 and the column treated as rank deficient
    // instead of flagged -- now A stays as it is (the NaNs reach gate_finish, which reports TNQS_ERR_NUMERIC like the plain Jacobi route) and V is NaN too
    if (s_bad || !(fro > 0)) {
        if (it.Vout) {
            cx<float>* Vg = reinterpret_cast<cx<float>*>(it.Vout);
            int rows = n;
            if (it.QB && it.dyn && it.dyn[7] > 0) { int mq, nq, kq_; theta_dims(it.dyn, it.dm, it.dn, mq, nq, kq_); rows = nq; (void)mq; (void)kq_; }
            const float fill = s_bad ? __builtin_nanf("") : 0.f;
            for (int e = tid; e < rows * n; e += NT) Vg[e] = cmake<float>(fill, fill);
        }
        if (tid == 0 && it.sweeps_out) *it.sweeps_out = 0;
        return;
    }
    const int kexp = pow2_exponent(fro);
    const double sc2 = ldexp(1.0, 2 * kexp), sc_out = ldexp(1.0, -kexp);                 // G is formed at ||A||_F = O(1): L, the sweeps and s_sig live at that scale
    fro = ldexp(fro, 2 * kexp);
    for (int e = tid; e < m * n; e += NT) Mf[(e % m) + mp * (int)s_pos[e / m]] = Ag[e];
    __syncthreads();
    PRE_STAMP(1);
    const int l15 = lane & 15, kq = lane >> 4;
    const bool full16 = !(m & 15) && !(n & 15);          // every 16 x 16 tile is full: the unguarded tile products
    // ---- 2. G = A^dagger A (sorted order), lower triangle, f64 matrix cores: one wave per 16 x 16 tile, operands converted from the f32 columns in LDS ------
    {
        const int nt = (n + 15) >> 4, ntile = nt * (nt + 1) / 2;
        for (int t = w; t < ntile; t += nw) {
            int ti, tj; tri_decode(t, ti, tj);                                          // ti >= tj
            const int ia = 16 * ti + l15, ja = 16 * tj + l15;
            const cx<float>* ci_ = Mf + mp * (ia < n ? ia : 0); const cx<float>* cj_ = Mf + mp * (ja < n ? ja : 0);
            v4d cr = {0, 0, 0, 0}, ci = {0, 0, 0, 0};
            if (full16) tile_mm_f32<true>(ci_, 1, cj_, 1, m, cr, ci);                    // G[i][j] = sum_r conj(A[r][i]) A[r][j]
            else ztile_mm(m, ia, ja,
                     [&](int i, int r) { cx<double> v = cmake<double>(0, 0); if (i < n && r < m) { const cx<float> a = ci_[r]; v = cmake<double>(a.re, -a.im); } return v; },
                     [&](int r, int j) { cx<double> v = cmake<double>(0, 0); if (j < n && r < m) { const cx<float> a = cj_[r]; v = cmake<double>(a.re, a.im); } return v; }, cr, ci);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 16 * ti + kq + 4 * r, j = 16 * tj + l15;
                if (i < n && j < n && i >= j) Gd[i + gp * j] = cmake<double>(cr[r] * sc2, i == j ? 0.0 : ci[r] * sc2);
            }
        }
    }
    __syncthreads();
    PRE_STAMP(2);
    // ---- 3. Cholesky, right-looking from the unscaled column, one barrier per column (see chol_kernel) -------------------------------------
    const double ptiny = 1e-13 * max_diag(n, [&](int i) { return Gd[i + gp * i].re; }, &s_dmax);
    auto pivot_of = [&](int k) { const double d = Gd[k + gp * k].re; return (d > ptiny) ? d : (ptiny > 0 ? ptiny : 1.0); };
    {
        constexpr int UT = (64 * 63 / 2 + NT - 1) / NT;           // trailing-triangle elements a thread owns at most (nested triangular numbering)
        unsigned char tr[UT], tc[UT];
#pragma unroll
        for (int u = 0; u < UT; ++u) {
            int r, c; tri_decode(tid + NT * u, r, c);
            tr[u] = (unsigned char)r; tc[u] = (unsigned char)c;
        }
        for (int k = 0; k < n - 1; ++k) {
            // a collapsed pivot (A rank deficient: the Schur complement left is rounding noise) ends the column: no trailing update from it, its entries below
            // the diagonal are dropped in step 4.  (Continuing with the clamped pivot divides noise by 1e-13: measured on a rank-20 factor, the entries of the
            // 44 noise columns grew to 1e22.)  Every thread reads the same diagonal entry, so the decision is uniform and the barrier count stays the same.
            if (!(Gd[k + gp * k].re > ptiny)) { __syncthreads(); continue; }
            const double dinv = 1.0 / pivot_of(k);
            const int mm = n - k - 1, k1 = k + 1, nt = mm * (mm + 1) / 2;
            const cx<double>* colk = Gd + gp * k;
            cx<double> li[UT], lj[UT], v[UT];
#pragma unroll
            for (int u = 0; u < UT; ++u) if (tid + NT * u < nt) { const int i = k1 + tr[u], j = k1 + tc[u]; li[u] = colk[i]; lj[u] = colk[j]; v[u] = Gd[i + gp * j]; }
#pragma unroll
            for (int u = 0; u < UT; ++u) if (tid + NT * u < nt) {
                const double sr = li[u].re * dinv, si = li[u].im * dinv;
                v[u].re -= sr * lj[u].re + si * lj[u].im; v[u].im -= si * lj[u].re - sr * lj[u].im;
                Gd[(k1 + tr[u]) + gp * (k1 + tc[u])] = v[u];
            }
            __syncthreads();
        }
    }
    for (int k = tid; k < n; k += NT) s_piv[k] = 1.0 / sqrt(pivot_of(k));
    __syncthreads();
    // ---- 4. X = L in f32 (over the start of the f64 array: everything is read before anything is written) --------------------------------
    {
        constexpr int UX = (64 * 64 + NT - 1) / NT;
        cx<float> xv[UX];
#pragma unroll
        for (int u = 0; u < UX; ++u) {
            const int e = tid + NT * u; const int i = e % n, k = e / n;
            xv[u] = cmake<float>(0.f, 0.f);
            if (e < n * n && i >= k) {
                const cx<double> a = Gd[i + gp * k]; const double r = s_piv[k];
                const bool dead = !(Gd[k + gp * k].re > ptiny);                      // collapsed pivot: the column is (0, ..., sqrt(ptiny), 0, ..., 0)
                xv[u] = (i == k) ? cmake<float>((float)(pivot_of(k) * r), 0.f) : (dead ? cmake<float>(0.f, 0.f) : cmake<float>((float)(a.re * r), (float)(a.im * r)));
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < UX; ++u) { const int e = tid + NT * u; if (e < n * n) X[(e % n) + xp * (e / n)] = xv[u]; }
    }
    __syncthreads();
    PRE_STAMP(3);
    // ---- 5. sweeps on the columns of L (n rows): the quarter-wave sweeps of jacobi_lds_kernel (an eighth-wave layout with four waves measured the same 45 us
    // per 64 x 64 sweep and, with its two-level rotation formulas, singular values 6-9 x less accurate) -------------------------------------------------------
    const float tiny = (float)((double)n * (double)eps_of<float>() * (double)eps_of<float>() * fro);
    int sweep;
    if (n == 64) sweep = jacobi_lds_sweeps_f32_full<4>(X, n, n, xp, max_sweeps, tiny, &s_rot);
    else if (n == 32) sweep = jacobi_lds_sweeps_f32_full<2>(X, n, n, xp, max_sweeps, tiny, &s_rot);      // chi = 16 gates: 16 full pairs on four waves, no guards
    else sweep = jacobi_lds_sweeps<float, 4, false>(X, (cx<float>*)nullptr, false, n, n, xp, 0, max_sweeps, tiny, &s_rot);
    __syncthreads();
    PRE_STAMP(4);
    // ---- 6. sigma_j = |x_j| (relative accuracy: what the truncation is decided on), U_L = normalised columns.  Only the `cap` largest singular values can survive
    // the truncation (JacobiItem::cap = the bond dimension cap of the gate): U Sigma and V are formed for those columns only; the others leave as sigma_j e_0,
    // which carries their weight into the truncation error and nothing else ------------------------------------------------------------------------------
    __shared__ unsigned char s_keep[64]; __shared__ int s_nk;
    for (int j = w; j < n; j += nw) {
        double s2 = 0;
        for (int i = lane; i < n; i += 64) { const cx<float> v = X[i + xp * j]; s2 += (double)v.re * v.re + (double)v.im * v.im; }
        s2 = wave_sum(s2);
        if (lane == 0) { s_cn[j] = s2 > 0 ? 1.0 / sqrt(s2) : 0.0; s_sig[j] = sqrt(s2); }
    }
    __syncthreads();
    const int cap = (it.cap > 0 && it.cap < n) ? it.cap : n;
    __shared__ unsigned char s_rank[64];
    for (int j = tid; j < n; j += NT) { const int rk = rank_desc(s_sig, n, j); s_keep[rk] = (unsigned char)j; s_rank[j] = (unsigned char)rk; }      // columns by decreasing singular value
    __syncthreads();
    // the consumer (gate_finish) ranks the columns again, by their f32 norms: everything within 1e-4 of the cap-th singular value is formed as well, so that a tie
    // at the cap -- the equal pseudo-values of collapsed pivots, or a degenerate pair -- can never make it pick a column that was not formed
    if (tid == 0) { int k = cap; const double thr = s_sig[s_keep[cap - 1]] * (1.0 - 1e-4); while (k < n && s_sig[s_keep[k]] >= thr) ++k; s_nk = k; }
    __syncthreads();
    const int nk = s_nk;
    for (int j = tid; j < n; j += NT)
        if ((int)s_rank[j] >= nk) for (int i = 0; i < m; ++i) Ag[i + (size_t)m * j] = cmake<float>(i == 0 ? (float)(s_sig[j] * sc_out) : 0.f, 0.f);
    const bool fullk = full16 && !(nk & 15);
    {
        // U Sigma = A U_L on the f64 matrix cores, computed TRANSPOSED (tile rows = kept column c of the result, lanes = row i: stores run along i).  A wave keeps
        // its (at most four) tiles in registers until the column norms are complete: the columns leave with the norm the sweeps found for them (s_sig) -- A u_j
        // carries an error of eps sigma_max in norm and direction like any product in working precision, the singular VALUE does not have to
        double* s_on = s_piv;                                        // column norms^2 of A X_final
        for (int j = tid; j < n; j += NT) s_on[j] = 0.0;
        __syncthreads();
        const int tr = (nk + 15) >> 4, tc = (m + 15) >> 4;           // tr * tc <= 4 * 8 = 32 tiles, at most four per wave
        v4d acr[4], aci[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int t = w + nw * q;
            acr[q] = v4d{0, 0, 0, 0}; aci[q] = v4d{0, 0, 0, 0};
            if (t < tr * tc) {
                const int c0 = 16 * (t % tr), i0 = 16 * (t / tr);
                const int jl = (int)s_keep[c0 + l15 < nk ? c0 + l15 : 0];              // this lane's column of X (A operand)
                if (fullk) tile_mm_f32<false>(X + xp * jl, 1, Mf + (i0 + l15), mp, n, acr[q], aci[q]);      // out[i][j] = sum_k A[i][k] X[k][j] (sorted columns of A)
                else ztile_mm(n, c0 + l15, i0 + l15,
                         [&](int c, int k) { cx<double> v = cmake<double>(0, 0); if (c < nk && k < n) { const cx<float> a = X[k + xp * jl]; v = cmake<double>(a.re, a.im); } return v; },
                         [&](int k, int i) { cx<double> v = cmake<double>(0, 0); if (i < m && k < n) { const cx<float> a = Mf[i + mp * k]; v = cmake<double>(a.re, a.im); } return v; },
                         acr[q], aci[q]);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    double p2 = acr[q][r] * acr[q][r] + aci[q][r] * aci[q][r];            // row c = c0 + kq + 4 r of the tile, column i = i0 + l15
                    if (i0 + l15 >= m) p2 = 0;
                    p2 = row16_sum(p2);
                    if (l15 == 0 && c0 + kq + 4 * r < nk) atomicAdd(&s_on[s_keep[c0 + kq + 4 * r]], p2);
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int t = w + nw * q;
            if (t < tr * tc) {
                const int c0 = 16 * (t % tr), i0 = 16 * (t / tr);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int c = c0 + kq + 4 * r, i = i0 + l15;
                    if (c < nk && i < m) {
                        const int j = s_keep[c];
                        const double f = s_on[j] > 0 ? s_sig[j] / sqrt(s_on[j]) * sc_out : 0.0;
                        Ag[i + (size_t)m * j] = cmake<float>((float)(acr[q][r] * f), (float)(aci[q][r] * f));
                    }
                }
            }
        }
    }
    PRE_STAMP(5);
    // ---- 7. right singular vectors, kept columns only.  Low-rank theta = A Q^T (Q = B L^-dagger, (r2 d2) x n, f64; written by lowrank_m_kernel):
    // V = conj(Q) U_L on the f64 matrix cores.  A theta factorised as it stands (QB null): V = U_L itself, rows back in the original column order.  U_L is
    // orthonormal to f32 rounding whatever the spectrum, so V needs no division by Sigma^2 -- the recovery from the unrotated theta this replaces amplified the
    // error of a column of U Sigma by (sigma_max / sigma_j)^2 and therefore needed U Sigma orthogonal relative to each column's own norm ---------------------
    const bool lowrank = it.QB && (!it.dyn || it.dyn[7] > 0);          // (an item offered with its Q whose low-rank route was withdrawn on the device is theta itself)
    if (it.Vout && !lowrank) {
        cx<float>* Vg = reinterpret_cast<cx<float>*>(it.Vout);
        for (int e = tid; e < n * (n - nk); e += NT) Vg[(e % n) + (size_t)n * (int)s_keep[nk + e / n]] = cmake<float>(0.f, 0.f);      // columns that were not formed: zero, never garbage
        for (int e = tid; e < n * nk; e += NT) {
            const int k = e % n, j = s_keep[e / n];
            const cx<float> v = X[k + xp * j]; const float f = (float)s_cn[j];
            Vg[(int)s_perm[k] + (size_t)n * j] = cmake<float>(v.re * f, v.im * f);
        }
    } else if (it.Vout && it.dyn) {
        int mq, nq, kq_; theta_dims(it.dyn, it.dm, it.dn, mq, nq, kq_);      // nq = r2 d2: rows of Q and of V
        (void)mq; (void)kq_;
        const cx<double>* Q = reinterpret_cast<const cx<double>*>(it.QB);
        cx<float>* Vg = reinterpret_cast<cx<float>*>(it.Vout);
        const int tr = (nk + 15) >> 4, tc = (nq + 15) >> 4;
        for (int e = tid; e < nq * (n - nk); e += NT) Vg[(e % nq) + (size_t)nq * (int)s_keep[nk + e / nq]] = cmake<float>(0.f, 0.f);      // columns that were not formed: zero, never garbage
        for (int t = w; t < tr * tc; t += nw) {
            const int c0 = 16 * (t % tr), i0 = 16 * (t / tr);
            const int jl = (int)s_keep[c0 + l15 < nk ? c0 + l15 : 0];
            v4d cr = {0, 0, 0, 0}, ci = {0, 0, 0, 0};
            ztile_mm(n, c0 + l15, i0 + l15,                                              // V[i][j] = sum_k conj(Q[i][perm k]) X[k][j] / |x_j|
                     [&](int c, int k) { cx<double> v = cmake<double>(0, 0); if (c < nk && k < n) { const cx<float> a = X[k + xp * jl]; v = cmake<double>(a.re, a.im); } return v; },
                     [&](int k, int i) { cx<double> v = cmake<double>(0, 0); if (i < nq && k < n) { v = Q[i + (size_t)nq * (int)s_perm[k]]; v.im = -v.im; } return v; }, cr, ci);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = c0 + kq + 4 * r, i = i0 + l15;
                if (c < nk && i < nq) { const int j = s_keep[c]; const double f = s_cn[j]; Vg[i + (size_t)nq * j] = cmake<float>((float)(cr[r] * f), (float)(ci[r] * f)); }
            }
        }
    }
    PRE_STAMP(6);
#undef PRE_STAMP
    if (tid == 0 && it.sweeps_out) *it.sweeps_out = sweep;
}
void launch_theta_svd_pre(hipStream_t s, const JacobiItem* d_items, int nitems, int max_sweeps, int mmax, int nmax) {
    if (nitems <= 0) return;
    const size_t lds = theta_svd_pre_lds_bytes(mmax, nmax);
    set_max_dynamic_lds((const void*)theta_svd_pre_kernel<512>, (size_t)(160 * 1024 - 4096));
    hipLaunchKernelGGL((theta_svd_pre_kernel<512>), dim3(nitems), dim3(512), lds, s, d_items, max_sweeps); TNQS_CHECK_LAUNCH();
}

// V[:,u] = A0^dagger a_u / |a_u|^2   (a_u = column u of U Sigma), for the factorisations run without accumulating V.
// grid (item, column block of 8): a wave owns one output column u and keeps a_u in registers (lanes = rows, coalesced);
// every V[col, u] is one coalesced column read of A0 and a wave reduction.
template <class T, int R>                  // m <= 64 R rows
__global__ __launch_bounds__(512) void recover_v_kernel(const RecoverItem* __restrict__ items) {
    const RecoverItem it = items[blockIdx.x];
    if (it.pre && theta_pre_takes(it.dyn, it.dm, it.dn, it.pre == 2)) return;      // V already written by theta_svd_pre_kernel
    const cx<T>* A0 = reinterpret_cast<const cx<T>*>(it.A0);
    const cx<T>* A = reinterpret_cast<const cx<T>*>(it.A);
    cx<T>* V = reinterpret_cast<cx<T>*>(it.V);
    int m_ = it.m, n_ = it.n, nu_ = it.nu;
    if (it.dyn) theta_dims(it.dyn, it.dm, it.dn, m_, n_, nu_);
    const int m = m_, n = n_, nu = nu_;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int u = blockIdx.y * 8 + w;
    if (u >= nu) return;
    double are[R], aim[R], s2 = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        int i = lane + 64 * r;
        cx<T> a = (i < m) ? A[i + (size_t)m * u] : cmake<T>((T)0, (T)0);
        are[r] = a.re; aim[r] = a.im; s2 += are[r] * are[r] + aim[r] * aim[r];
    }
    s2 = wave_sum(s2);
    const double inv = s2 > 0 ? 1.0 / s2 : 0.0;
    constexpr int CU = 8;                    // columns in flight per iteration (loads of 8 columns overlap the reductions)
    for (int col0 = 0; col0 < n; col0 += CU) {
        double re[CU], im[CU];
#pragma unroll
        for (int c = 0; c < CU; ++c) {
            re[c] = 0; im[c] = 0;
            const int col = col0 + c;
            if (col < n) {
                const cx<T>* b0 = A0 + (size_t)m * col;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    int i = lane + 64 * r;
                    if (i < m) { cx<T> b = b0[i]; re[c] += (double)b.re * are[r] + (double)b.im * aim[r]; im[c] += (double)b.re * aim[r] - (double)b.im * are[r]; }   // conj(b) * a
                }
            }
        }
#pragma unroll
        for (int c = 0; c < CU; ++c) { re[c] = wave_sum(re[c]); im[c] = wave_sum(im[c]); }
        if (lane < CU && col0 + lane < n) {
            double rr = 0, ii = 0;
#pragma unroll
            for (int c = 0; c < CU; ++c) if (lane == c) { rr = re[c]; ii = im[c]; }
            V[col0 + lane + (size_t)n * u] = cmake<T>((T)(rr * inv), (T)(ii * inv));
        }
    }
}
template <class T> void launch_recover_v(hipStream_t s, const RecoverItem* d_items, int nitems, int nmax) {
    if (nitems <= 0) return;
    // (rows: at most 512 = theta of d^2 chi <= 512; R = 8 costs registers only when it is needed, and the caller cannot know m per item here)
    hipLaunchKernelGGL((recover_v_kernel<T, 8>), dim3(nitems, (nmax + 7) / 8), dim3(512), 0, s, d_items); TNQS_CHECK_LAUNCH();
}
template void launch_recover_v<float>(hipStream_t, const RecoverItem*, int, int);
template void launch_recover_v<double>(hipStream_t, const RecoverItem*, int, int);

// lds_bytes: max over the items of (m*n + (V ? n*n : 0)) * sizeof(complex<T>); 0 selects the global-memory kernel
// A quarter wave rotates one column pair, so a round of an n-column matrix keeps n / 8 waves busy; waves beyond that only add to every
// barrier of the sweep (and a 1024-thread workgroup per 32 x 32 message matrix left three quarters of each CU's wave slots idling at
// barriers: 1140 such matrices per colour batch).  The workgroup is sized for the columns the matrices are expected to have (`ncols`;
// more columns than that still work: the slots loop).
template <class T, int RQ> static void launch_jacobi_lds(hipStream_t s, const JacobiItem* d_items, int nitems, int max_sweeps, size_t lds_bytes, int ncols) {
    set_max_dynamic_lds((const void*)jacobi_lds_kernel<T, RQ>, (size_t)(160 * 1024 - 2048));
    int waves = (ncols + 7) / 8; waves = waves < 4 ? 4 : (waves > 16 ? 16 : waves);
    hipLaunchKernelGGL((jacobi_lds_kernel<T, RQ>), dim3(nitems), dim3(64 * waves), lds_bytes, s, d_items, max_sweeps); TNQS_CHECK_LAUNCH();
}
// mmax: largest row count among the items (selects the rows-per-lane instantiation); ncols: expected column count (0: mmax)
template <class T> void launch_jacobi(hipStream_t s, const JacobiItem* d_items, int nitems, int max_sweeps, size_t lds_bytes, int mmax, int ncols) {
    if (nitems <= 0) return;
    if (ncols <= 0) ncols = mmax;
    if (lds_bytes > 0 && lds_bytes <= 160 * 1024 - 2048 && mmax <= 256) {
        if (mmax <= 32) launch_jacobi_lds<T, 2>(s, d_items, nitems, max_sweeps, lds_bytes, ncols);
        else if (mmax <= 64) launch_jacobi_lds<T, 4>(s, d_items, nitems, max_sweeps, lds_bytes, ncols);
        else if (mmax <= 96) launch_jacobi_lds<T, 6>(s, d_items, nitems, max_sweeps, lds_bytes, ncols);
        else if (mmax <= 128) launch_jacobi_lds<T, 8>(s, d_items, nitems, max_sweeps, lds_bytes, ncols);
        else launch_jacobi_lds<T, 16>(s, d_items, nitems, max_sweeps, lds_bytes, ncols);
    } else {
        if (mmax > 512) throw std::runtime_error("launch_jacobi: more than 512 rows");
        if (mmax <= 256) { hipLaunchKernelGGL((jacobi_kernel<T, 4>), dim3(nitems), dim3(1024), 0, s, d_items, max_sweeps); }
        else { hipLaunchKernelGGL((jacobi_kernel<T, 8>), dim3(nitems), dim3(1024), 0, s, d_items, max_sweeps); }
        TNQS_CHECK_LAUNCH();
    }
}
template void launch_jacobi<float>(hipStream_t, const JacobiItem*, int, int, size_t, int, int);
template void launch_jacobi<double>(hipStream_t, const JacobiItem*, int, int, size_t, int, int);

// ------------------------------------------------------------------------------------------------------------
// small sites (N < n): matricise psi~ to f64, and turn the rotated columns (U Sigma) into the (A, V) pair gate_eigs reads
// ------------------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void small_svd_prepare_kernel(const SmallSvdItem* __restrict__ items) {
    const SmallSvdItem it = items[blockIdx.x];
    const cx<T>* src = reinterpret_cast<const cx<T>*>(it.src);
    cx<double>* M = reinterpret_cast<cx<double>*>(it.M);
    const int n = it.d * it.chi_b; const size_t tot = (size_t)n * it.low * it.hi;
    for (size_t e = threadIdx.x; e < tot; e += 256) {
        int s = (int)(e % it.d); size_t r = e / it.d; int lo = (int)(r % it.low); size_t r2 = r / it.low; int ib = (int)(r2 % it.chi_b); int hi = (int)(r2 / it.chi_b);
        cx<T> v = src[e];
        M[(s + it.d * ib) + (size_t)n * (lo + (size_t)it.low * hi)] = cmake<double>((double)v.re, -(double)v.im);     // M = Psi^dagger: G = M M^dagger, eigenvectors = left singular vectors
    }
}
template <class T> void launch_small_svd_prepare(hipStream_t s, const SmallSvdItem* d_items, int nitems) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL((small_svd_prepare_kernel<T>), dim3(nitems), dim3(256), 0, s, d_items); TNQS_CHECK_LAUNCH();
}
template void launch_small_svd_prepare<float>(hipStream_t, const SmallSvdItem*, int);
template void launch_small_svd_prepare<double>(hipStream_t, const SmallSvdItem*, int);
// column j of M J = sigma_j u_j:  V[:,j] = u_j, A[:,j] = sigma_j^2 u_j (so that Re(v_j^dagger a_j) = sigma_j^2 = the eigenvalue of G)
__global__ __launch_bounds__(256) void small_svd_finish_kernel(const SmallSvdItem* __restrict__ items) {
    const SmallSvdItem it = items[blockIdx.x];
    const cx<double>* M = reinterpret_cast<const cx<double>*>(it.M);
    cx<double>* A = reinterpret_cast<cx<double>*>(it.GA);
    cx<double>* V = reinterpret_cast<cx<double>*>(it.GV);
    const int n = it.d * it.chi_b, N = it.low * it.hi;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int j = w; j < n; j += 4) {
        double s2 = 0;
        if (j < N) for (int i = lane; i < n; i += 64) { cx<double> v = M[i + (size_t)n * j]; s2 += v.re * v.re + v.im * v.im; }
        s2 = wave_sum(s2);
        const double sg = sqrt(s2), inv = sg > 0 ? 1.0 / sg : 0.0;
        for (int i = lane; i < n; i += 64) {
            cx<double> v = (j < N) ? M[i + (size_t)n * j] : cmake<double>(0, 0);
            V[i + (size_t)n * j] = cmake<double>(v.re * inv, v.im * inv);
            A[i + (size_t)n * j] = cmake<double>(v.re * sg, v.im * sg);
        }
    }
}
void launch_small_svd_finish(hipStream_t s, const SmallSvdItem* d_items, int nitems) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL(small_svd_finish_kernel, dim3(nitems), dim3(256), 0, s, d_items); TNQS_CHECK_LAUNCH();
}

}  // namespace tnqs
