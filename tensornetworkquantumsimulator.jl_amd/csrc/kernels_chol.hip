// kernels_chol.hip -- Cholesky factor (and inverse) of a Gram matrix, and the environment square roots' prepare / finish pair.
#include "kernels.hpp"
#include "device_common.hpp"
#include "jacobi_common.hpp"
#include "launch_util.hpp"

namespace tnqs {

// ------------------------------------------------------------------------------------------------------------
// Cholesky factor of the Gram matrix (the R factor of the thin QR, simple_update.jl:45-48, when G has full rank)
// ------------------------------------------------------------------------------------------------------------
// Right-looking, ONE workgroup barrier per column: the trailing update of step k works from the UNSCALED column k,
//   A[i][j] -= A[i][k] conj(A[j][k]) / A[k][k]     (columns j > k; column k itself is never written again),
// every thread derives the pivot from A[k][k] by the same rule, and the scaling L[i][k] = A[i][k] / sqrt(A[k][k]) happens for all columns
// at once at the end.  With Lt = unit lower triangular, Lt[i][k] = A[i][k] / A[k][k], this is G = Lt D Lt^dagger, L = Lt D^1/2.
// The INVERSE rides along in the same steps (round 3): M = Lt^-1 is what the same row operations make of the identity,
//   M[i][c] -= Lt[i][k] M[k][c]     (rows i > k, columns c <= k, M[k][k] = 1),
// kept in the free strict upper triangle (M[i][c] at A[c + np i]); L^-1 = D^-1/2 M.  No separate substitution phase, no extra barrier.
// Within a step every element update is independent: a thread takes elements e = tid + 256 u of the trailing triangle (row-major
// triangular numbering, which is NESTED: the first m (m + 1) / 2 numbers are the triangle of size m, so a thread's (row, column) pairs
// are decoded once for the whole factorisation) and of the (rows > k) x (columns <= k) rectangle, eight at a time with all their LDS
// loads issued before the first store -- the column step is then one LDS round trip deep instead of one per element.
// (History: a first version scaled the column between two extra barriers per step and inverted L with one serial thread per column:
// 214 us per launch on a 64 x 64 matrix; the one-barrier version with a per-thread loop over columns and a 4-lane substitution for the
// inverse: 122 us = 10 load + 64 column loop (1 us per column, a chain of LDS latencies) + 45 inverse.)
template <int NT, int UT>      // threads, and the trailing-triangle elements a thread owns at most (UT a multiple of 3; NT * UT >= 96 * 97 / 2)
__global__ __launch_bounds__(NT) void chol_kernel(const CholItem* __restrict__ items) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ double s_dmax;
    const CholItem it = items[blockIdx.x];
    // (NT = 1024, sixteen waves: the other waves of a SIMD cover a wave's LDS round trips)
    const int n = it.n, np = n + 1, tid = threadIdx.x;
    cx<double>* A = reinterpret_cast<cx<double>*>(smem);          // [col j][row i] at i + np*j, lower triangle becomes L (unscaled), strict upper M
    const cx<double>* G = reinterpret_cast<const cx<double>*>(it.G);
    for (int e = tid; e < n * n; e += NT) {                       // Hermitian part, as the eigen path sees it; zeros above the diagonal
        int i = e % n, j = e / n;
        cx<double> v = cmake<double>(0, 0);
        if (i >= j) { cx<double> a = G[i + (size_t)n * j], b = G[j + (size_t)n * i]; v = cmake<double>(0.5 * (a.re + b.re), 0.5 * (a.im - b.im)); }
        A[i + np * j] = v;
    }
    __syncthreads();
    const double tiny = it.tau * max_diag(n, [&](int i) { return A[i + np * i].re; }, &s_dmax);
    // the pivot rule: a pivot at or below tiny (or not a number) flags the item and is replaced, so that the factorisation completes
    auto pivot_of = [&](int k, bool& bad) { double d = A[k + np * k].re; bad = !(d > tiny); return bad ? (tiny > 0 ? tiny : 1.0) : d; };
    // this thread's elements of the trailing triangle: number e = r (r + 1) / 2 + c, 0 <= c <= r  (n <= 96: at most 4560 / 1024 -> 5)
    unsigned char tr[UT], tc[UT];
#pragma unroll
    for (int u = 0; u < UT; ++u) {
        int r, c; tri_decode(tid + NT * u, r, c);
        tr[u] = (unsigned char)r; tc[u] = (unsigned char)c;
    }
    const bool wantW = it.Winv != nullptr;
    for (int k = 0; k < n; ++k) {
        bool bad; const double d = pivot_of(k, bad);
        if (bad && tid == 0) *it.fail = 1;
        const double dinv = 1.0 / d;
        const int m = n - k - 1, k1 = k + 1;
        const cx<double>* colk = A + np * k;                       // colk[i] = A[i][k]
        // ---- trailing triangle: A[i][j] -= (A[i][k] / d) conj(A[j][k]),  i = k1 + r,  j = k1 + c ----------------------------------------
        const int nt = m * (m + 1) / 2;
#pragma unroll
        for (int u0 = 0; u0 < UT; u0 += 3) {
            if (NT * u0 >= nt) break;                               // (workgroup-uniform)
            cx<double> li[3], lj[3], v[3];
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                if (u0 + u < UT && tid + NT * (u0 + u) < nt) { const int i = k1 + tr[u0 + u], j = k1 + tc[u0 + u]; li[u] = colk[i]; lj[u] = colk[j]; v[u] = A[i + np * j]; }
            }
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                if (u0 + u < UT && tid + NT * (u0 + u) < nt) {
                    const double sr = li[u].re * dinv, si = li[u].im * dinv;
                    v[u].re -= sr * lj[u].re + si * lj[u].im; v[u].im -= si * lj[u].re - sr * lj[u].im;
                    A[(k1 + tr[u0 + u]) + np * (k1 + tc[u0 + u])] = v[u];
                }
            }
        }
        // ---- inverse: M[i][c] -= (A[i][k] / d) M[k][c],  i = k1 + ri,  c <= k;  M[i][c] at A[c + np i], M[k][k] = 1 ------------------------
        if (wantW) {
            const int nr = m * k1;
            const float rk1 = 1.0f / (float)k1;
            for (int q0 = 0; q0 < nr; q0 += NT * 2) {
                cx<double> li[2], mk[2], v[2]; int ii[2], cc[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int q = q0 + tid + NT * u;
                    int ri = (int)((float)q * rk1); if (ri * k1 > q) --ri; if ((ri + 1) * k1 <= q) ++ri;
                    ii[u] = k1 + ri; cc[u] = q - ri * k1;
                    if (q < nr) {
                        li[u] = colk[ii[u]];
                        mk[u] = cc[u] == k ? cmake<double>(1.0, 0.0) : A[cc[u] + np * k];
                        v[u] = A[cc[u] + np * ii[u]];
                    }
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int q = q0 + tid + NT * u;
                    if (q < nr) {
                        const double sr = li[u].re * dinv, si = li[u].im * dinv;
                        v[u].re -= sr * mk[u].re - si * mk[u].im; v[u].im -= sr * mk[u].im + si * mk[u].re;
                        A[cc[u] + np * ii[u]] = v[u];
                    }
                }
            }
        }
        __syncthreads();
    }
    // L[i][k] = A[i][k] / sqrt(pivot_k), L[k][k] = sqrt(pivot_k);  W = (L^-1)^dagger: W[i + n a] = conj(M[a][i]) / sqrt(pivot_a) above the diagonal
    __shared__ double s_piv[96];
    for (int k = tid; k < n; k += NT) { bool bad; s_piv[k] = sqrt(pivot_of(k, bad)); }
    __syncthreads();
    cx<double>* L = reinterpret_cast<cx<double>*>(it.L);
    cx<double>* W = reinterpret_cast<cx<double>*>(it.Winv);
    for (int e = tid; e < n * n; e += NT) {
        const int i = e % n, k = e / n;
        const cx<double> a = A[i + np * k];
        const double r = 1.0 / s_piv[k];
        cx<double> l = cmake<double>(0, 0), w = cmake<double>(0, 0);
        if (i == k) { l = cmake<double>(s_piv[k], 0.0); w = cmake<double>(r, 0.0); }
        else if (i > k) l = cmake<double>(a.re * r, a.im * r);
        else w = cmake<double>(a.re * r, -a.im * r);
        L[e] = l;
        if (W) W[e] = w;
    }
}
// Same factorisation with the lower triangle PACKED in LDS (column j holds rows j..n-1): n up to 128 fits (132 KB), which the low-rank theta
// route needs at chi = 64 (K = kappa chi = 128).  Only L is produced (CholItem::Winv is not written: the packed layout has no spare triangle
// for the inverse: when CholItem::Winv is given, (L^-1)^dagger is built in place in global memory by a second phase).
__global__ __launch_bounds__(1024) void chol_packed_kernel(const CholItem* __restrict__ items) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ double s_dmax;
    const CholItem it = items[blockIdx.x];
    constexpr int NT = 1024;                                         // sixteen waves: a thread's column loop is at most 8 long, and the other waves of its SIMD cover its LDS round trips
    const int n = it.n, tid = threadIdx.x;
    cx<double>* A = reinterpret_cast<cx<double>*>(smem);
    auto at = [n](int i, int j) { return (size_t)j * n - (size_t)j * (j - 1) / 2 + (i - j); };      // i >= j
    const cx<double>* G = reinterpret_cast<const cx<double>*>(it.G);
    for (int e = tid; e < n * n; e += NT) {
        int i = e % n, j = e / n; if (i < j) continue;
        cx<double> a = G[i + (size_t)n * j], b = G[j + (size_t)n * i];
        A[at(i, j)] = cmake<double>(0.5 * (a.re + b.re), 0.5 * (a.im - b.im));
    }
    __syncthreads();
    const double dmax = max_diag(n, [&](int i) { return A[at(i, i)].re; }, &s_dmax);
    if (it.shift > 0) { for (int i = tid; i < n; i += NT) A[at(i, i)].re += it.shift * dmax; __syncthreads(); }
    const double tiny = it.tau * dmax;
    // right-looking with ONE barrier per column, as chol_kernel: trailing updates from the unscaled column, pivots by the same rule in every
    // thread, all columns scaled at the end
    auto pivot_of = [&](int k, bool& bad) { double d = A[at(k, k)].re; bad = !(d > tiny); return bad ? (tiny > 0 ? tiny : 1.0) : d; };
    const int ti = tid & 63, tj = tid >> 6;
    for (int k = 0; k < n; ++k) {
        bool bad; const double d = pivot_of(k, bad);
        if (bad && tid == 0) *it.fail = 1;
        const double dinv = 1.0 / d;
        for (int i = k + 1 + ti; i < n; i += 64) {
            const cx<double> li = A[at(i, k)];
            const cx<double> ls = cmake<double>(li.re * dinv, li.im * dinv);
            int j = k + 1 + tj;
            for (; j <= i; j += NT / 64) {
                const cx<double> lj = A[at(j, k)];
                cx<double> v = A[at(i, j)];
                v.re -= ls.re * lj.re + ls.im * lj.im; v.im -= ls.im * lj.re - ls.re * lj.im;
                A[at(i, j)] = v;
            }
        }
        __syncthreads();
    }
    __shared__ double s_pivs[128];
    for (int k = tid; k < n; k += NT) { bool bad; s_pivs[k] = sqrt(pivot_of(k, bad)); }
    __syncthreads();
    for (int e = tid; e < n * n; e += NT) {
        const int i = e % n, k = e / n;
        if (i < k) continue;
        if (i == k) A[at(k, k)] = cmake<double>(s_pivs[k], 0.0);
        else { const cx<double> v = A[at(i, k)]; const double r = 1.0 / s_pivs[k]; A[at(i, k)] = cmake<double>(v.re * r, v.im * r); }
    }
    __syncthreads();
    cx<double>* L = reinterpret_cast<cx<double>*>(it.L);
    for (int e = tid; e < n * n; e += NT) { int i = e % n, j = e / n; L[e] = (i >= j) ? A[at(i, j)] : cmake<double>(0, 0); }
    if (!it.Winv) return;
    // W = (L^-1)^dagger (upper triangular), W[c + n*i] = conj(Linv[i, c]).  L^-1 is built IN PLACE in the packed triangle, from the last column
    // to the first: column j of the inverse is  -Linv[j+1:, j+1:] L[j+1:, j] / L[j, j]  -- the trailing block is already inverted, column j still
    // holds L.  Eight threads per row i split the sum over k (one LDS read of Linv[i, k], consecutive in i, and one broadcast read of L[k, j] per
    // term); two barriers per column.  (Round 2 ran one thread per column of the inverse against global memory: 0.6 of the kernel's 0.78 ms
    // at n = 128.)  L itself has been written out above.
    __syncthreads();
    cx<double>* W = reinterpret_cast<cx<double>*>(it.Winv);
    const int row = tid >> 3, half = tid & 7;                     // eight threads per row split the sum over k
    for (int j = n - 1; j >= 0; --j) {
        const double dj = 1.0 / A[at(j, j)].re;
        const int i = j + 1 + row;
        double ar = 0, ai = 0;
        if (i < n) {
            int k = j + 1 + half;
            for (; k + 24 <= i; k += 32) {                       // four independent terms in flight
                cx<double> x[4], l[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) { x[u] = A[at(i, k + 8 * u)]; l[u] = A[at(k + 8 * u, j)]; }
#pragma unroll
                for (int u = 0; u < 4; ++u) { ar -= x[u].re * l[u].re - x[u].im * l[u].im; ai -= x[u].re * l[u].im + x[u].im * l[u].re; }
            }
            for (; k <= i; k += 8) {
                const cx<double> x = A[at(i, k)], l = A[at(k, j)];
                ar -= x.re * l.re - x.im * l.im; ai -= x.re * l.im + x.im * l.re;
            }
        }
        ar += __shfl_xor(ar, 1, 64); ai += __shfl_xor(ai, 1, 64);
        ar += __shfl_xor(ar, 2, 64); ai += __shfl_xor(ai, 2, 64);
        ar += __shfl_xor(ar, 4, 64); ai += __shfl_xor(ai, 4, 64);
        __syncthreads();                                   // column j has been read by everybody
        if (i < n && half == 0) A[at(i, j)] = cmake<double>(ar * dj, ai * dj);
        if (tid == 0) A[at(j, j)] = cmake<double>(dj, 0.0);
        __syncthreads();
    }
    for (int e = tid; e < n * n; e += NT) {
        const int c = e % n, i = e / n;
        cx<double> v = cmake<double>(0, 0);
        if (i >= c) { v = A[at(i, c)]; v.im = -v.im; }
        W[e] = v;
    }
}
void launch_chol_packed(hipStream_t s, const CholItem* d_items, int nitems, int nmax) {
    if (nitems <= 0) return;
    const size_t lds = (size_t)nmax * (nmax + 1) / 2 * 16;
    set_max_dynamic_lds((const void*)chol_packed_kernel, (size_t)(160 * 1024 - 2048));      // (+ ~1 KB of static LDS: pivots)
    hipLaunchKernelGGL(chol_packed_kernel, dim3(nitems), dim3(1024), lds, s, d_items); TNQS_CHECK_LAUNCH();
}
void launch_chol(hipStream_t s, const CholItem* d_items, int nitems, int nmax) {
    if (nitems <= 0) return;
    const size_t lds = (size_t)nmax * (nmax + 1) * 16;
    set_max_dynamic_lds((const void*)chol_kernel<1024, 6>, (size_t)(160 * 1024 - 1024));       // (the kernel also has ~0.8 KB of static LDS: pivots)
    hipLaunchKernelGGL((chol_kernel<1024, 6>), dim3(nitems), dim3(1024), lds, s, d_items); TNQS_CHECK_LAUNCH();
}

// ------------------------------------------------------------------------------------------------------------
// environment square roots  (src/utils.jl:18-27 with safe_eigen :94-108: always f64)
// ------------------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void env_prepare_kernel(const EnvItem* __restrict__ items) {
    const EnvItem it = items[blockIdx.x];
    const int n = it.n;
    const cx<T>* M = reinterpret_cast<const cx<T>*>(it.msg);
    cx<double>* H = reinterpret_cast<cx<double>*>(it.H);
    cx<double>* V = reinterpret_cast<cx<double>*>(it.V);
    for (int e = threadIdx.x; e < n * n; e += 256) {
        int i = e % n, j = e / n;
        double re, im;
        if (M) {
            cx<T> a = M[i + n * j], b = M[j + n * i];
            re = 0.5 * ((double)a.re + (double)b.re); im = 0.5 * ((double)a.im - (double)b.im);
        } else { re = (i == j) ? 1.0 : 0.0; im = 0; }
        H[e] = cmake<double>(re, im);
        V[e] = cmake<double>(i == j ? 1.0 : 0.0, 0.0);
    }
}
template <class T> void launch_env_prepare(hipStream_t s, const EnvItem* d_items, int nitems) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL((env_prepare_kernel<T>), dim3(nitems), dim3(256), 0, s, d_items); TNQS_CHECK_LAUNCH();
}
template void launch_env_prepare<float>(hipStream_t, const EnvItem*, int);
template void launch_env_prepare<double>(hipStream_t, const EnvItem*, int);

template <class T>
__global__ __launch_bounds__(256) void env_finish_kernel(const EnvFinishItem* __restrict__ items) {
    __shared__ double lam[256], sq[256];
    __shared__ int s_full, s_err;
    const EnvFinishItem it = items[blockIdx.x];
    const int n = it.n;
    const cx<double>* A = reinterpret_cast<const cx<double>*>(it.A);
    const cx<double>* V = reinterpret_cast<const cx<double>*>(it.V);
    if (threadIdx.x == 0) { s_full = 1; s_err = 0; }
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += 256) {
        double l = 0;       // Rayleigh quotient v_j^dagger H v_j = Re(v_j^dagger a_j)
        for (int i = 0; i < n; ++i) { cx<double> v = V[i + n * j], a = A[i + n * j]; l += v.re * a.re + v.im * a.im; }
        lam[j] = l;
        // (sq[j]: sqrt(lambda_j) of the eigenvalues that are kept, -1 for the dropped ones -- once per eigenvalue instead of once per term below)
        // the reference casts the eigenvalues back to the message precision BEFORE the cutoff test (safe_eigen, src/utils.jl:100-107, then
        // `abs(x) < cutoff` on the Float32 value, :21-22): an eigenvalue within an f32 ulp of the cutoff must land on the same side here
        const double lt = (double)(T)l;
        const bool zero = (lt == 0) || (fabs(lt) < it.cutoff);
        if (zero) s_full = 0;
        else if (lt < 0) s_err = 1;       // Julia: sqrt(negative) -> DomainError (src/utils.jl:21)
        sq[j] = (zero || lt < 0) ? -1.0 : sqrt(l);
    }
    __syncthreads();
    cx<T>* ms = reinterpret_cast<cx<T>*>(it.msqrt);
    cx<T>* pr = reinterpret_cast<cx<T>*>(it.proj);
    for (int e = threadIdx.x; e < n * n; e += 256) {
        int i = e % n, l = e / n;
        cx<double> s1 = cmake<double>(0, 0), s2 = cmake<double>(0, 0);
        for (int j = 0; j < n; ++j) {
            const double sj = sq[j];
            if (sj < 0) continue;
            cx<double> vi = V[i + n * j], vl = V[l + n * j];
            cx<double> o = cmake<double>(vi.re * vl.re + vi.im * vl.im, vi.im * vl.re - vi.re * vl.im);  // vi conj(vl)
            s1.re += sj * o.re; s1.im += sj * o.im;
            s2.re += o.re; s2.im += o.im;
        }
        ms[e] = cmake<T>((T)s1.re, (T)s1.im);
        pr[e] = cmake<T>((T)s2.re, (T)s2.im);
    }
    if (threadIdx.x == 0) { it.flags[0] = s_full; it.flags[1] = s_err; }
}
template <class T> void launch_env_finish(hipStream_t s, const EnvFinishItem* d_items, int nitems) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL((env_finish_kernel<T>), dim3(nitems), dim3(256), 0, s, d_items); TNQS_CHECK_LAUNCH();
}
template void launch_env_finish<float>(hipStream_t, const EnvFinishItem*, int);
template void launch_env_finish<double>(hipStream_t, const EnvFinishItem*, int);

}  // namespace tnqs
