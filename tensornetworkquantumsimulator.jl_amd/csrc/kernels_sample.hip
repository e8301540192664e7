// kernels_sample.hip -- sampling from a BP cache (reference: src/sampling.jl:18-43, the alg = "bp" branch).
//
// One step of the loop at vertex v, site tensor psi_v[s, l] (s fastest, l = all bond legs), T = psi_v with every incoming message absorbed:
//   site_prob_partial_kernel   diag[s] = Re sum_l T[s, l] conj psi_v[s, l]    one streaming pass over T and psi_v, f64 accumulation for both element types.
//                              Thread t of the launch owns the elements e = t + k * NT with NT = the thread count rounded DOWN to a multiple of d, so its
//                              site index e mod d = t mod d is the same in every iteration (one accumulator in a register) and the 64 lanes of a wave read 64
//                              consecutive elements: whole 128-byte lines.  One partial per workgroup and site index.
//   site_draw_kernel           sums the partials in workgroup order, p = diag / tr, checks tr and the sign of the diagonal, draws x from ONE uniform by the
//                              cumulative sum and leaves x, p[x] and p in device memory.  The uniform is the caller's or counter-based: a function of
//                              (seed, sample, step) alone, 53 bits, never 1.
//   site_project_kernel        out[i] = psi_v[x + d i] with x read from device memory: the host enqueues it (and the BP update behind it) without knowing x.
// Every reduction runs in a fixed order, so the same inputs give the same bits whichever entry point (tnqs_site_probabilities, tnqs_sample_bp) launched them.
#include <stdexcept>
#include "kernels.hpp"
#include "device_common.hpp"

namespace tnqs {

template <class T> struct Vec2;
template <> struct Vec2<float> { typedef float2 type; };
template <> struct Vec2<double> { typedef double2 type; };
template <class T> __global__ __launch_bounds__(256) void site_prob_partial_kernel(const typename Vec2<T>::type* __restrict__ tabs, const typename Vec2<T>::type* __restrict__ psi, size_t n, int d,
                                                                                   double* __restrict__ partial /* gridDim.x x 16 */) {
    __shared__ double red[256];
    const size_t nthreads = (size_t)gridDim.x * 256;
    const size_t NT = nthreads - nthreads % (size_t)d;            // (the launcher guarantees nthreads >= d)
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    double acc = 0;
    if (t < NT) {
        for (size_t e = t; e < n; e += NT) {
            const typename Vec2<T>::type a = tabs[e], b = psi[e];            // one 8- / 16-byte load per element: a wave reads 512 / 1024 contiguous bytes
            acc += (double)a.x * (double)b.x + (double)a.y * (double)b.y;
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    if ((int)threadIdx.x < d) {
        // lanes of this workgroup whose site index is threadIdx.x: (blockIdx.x * 256 + q) mod d == threadIdx.x, in ascending q
        const int first = (int)(((size_t)threadIdx.x + (size_t)d - ((size_t)blockIdx.x * 256) % (size_t)d) % (size_t)d);
        double sum = 0;
        for (int q = first; q < 256; q += d) sum += red[q];
        partial[(size_t)blockIdx.x * 16 + threadIdx.x] = sum;
    }
}

__device__ __forceinline__ unsigned long long sample_mix64(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull; x = (x ^ (x >> 27)) * 0x94D049BB133111EBull; return x ^ (x >> 31);
}

// status bits: 1 = tr rho is zero / negative / not finite, 2 = a diagonal entry below -neg_tol * tr
__global__ __launch_bounds__(64) void site_draw_kernel(const double* __restrict__ partial, int nblocks, int d, double neg_tol,
                                                       const double* __restrict__ uniform /* null: counter-based */, unsigned long long seed, unsigned long long sample,
                                                       unsigned long long step, int draw, double* __restrict__ p_out /* d, may be null */, int* __restrict__ x_out,
                                                       double* __restrict__ px_out, int* __restrict__ status) {
    __shared__ double diag[16];
    if ((int)threadIdx.x < d) {
        double sum = 0;
        for (int b = 0; b < nblocks; ++b) sum += partial[(size_t)b * 16 + threadIdx.x];
        diag[threadIdx.x] = sum;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double tr = 0;
    for (int j = 0; j < d; ++j) tr += diag[j];
    int bad = 0;
    if (!(tr > 0) || !(tr <= 1.79769313486231570e308)) bad |= 1;
    else for (int j = 0; j < d; ++j) if (diag[j] < -neg_tol * tr) bad |= 2;
    double p[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) p[j] = 0;
    if (!bad) {
#pragma unroll
        for (int j = 0; j < 16; ++j) if (j < d) p[j] = (diag[j] < 0 ? 0.0 : diag[j]) / tr;       // a negative entry within rounding counts as 0
    }
    if (p_out) {
#pragma unroll
        for (int j = 0; j < 16; ++j) if (j < d) p_out[j] = p[j];
    }
    if (bad) atomicOr(status, bad);
    if (!draw) return;
    double u;
    if (uniform) u = *uniform;
    else {
        const unsigned long long r = sample_mix64(sample_mix64(sample_mix64(seed) + 0xD1B54A32D192ED03ull * sample) + 0xC2B2AE3D27D4EB4Full * step);
        u = (double)(r >> 11) * (1.0 / 9007199254740992.0);
    }
    int x = d - 1; double px = 0, cdf = 0; bool found = false;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if (j < d) { cdf += p[j]; if (!found && u < cdf) { x = j; found = true; } }
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) if (j == x) px = p[j];
    if (bad) { x = 0; px = 0; }
    *x_out = x; *px_out = px;
}

template <class T> __global__ __launch_bounds__(256) void site_project_kernel(const T* __restrict__ psi, T* __restrict__ out, size_t nout, int d,
                                                                              const int* __restrict__ x_dev, int x_host) {
    int x = x_dev ? *x_dev : x_host;
    x = x < 0 ? 0 : (x >= d ? d - 1 : x);                        // never outside the tensor, whatever the draw left behind
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nout; i += (size_t)gridDim.x * 256) {
        const size_t e = (size_t)x + (size_t)d * i;
        out[2 * i] = psi[2 * e]; out[2 * i + 1] = psi[2 * e + 1];
    }
}

int plan_site_prob(size_t n, int d) {
    size_t blocks = (n + 1023) / 1024;                            // four elements per thread and more
    if (blocks > 1024) blocks = 1024;
    if (blocks < 1) blocks = 1;
    (void)d;                                                      // 256 threads >= d for every d the library accepts (<= 16)
    return (int)blocks;
}
template <class T> void launch_site_prob_partial(hipStream_t s, const void* tabs, const void* psi, size_t n, int d, int nblocks, double* d_partial) {
    if (d < 1 || d > 16) throw std::runtime_error("site_prob_partial: site dimension out of range");
    hipLaunchKernelGGL((site_prob_partial_kernel<T>), dim3(nblocks), dim3(256), 0, s, reinterpret_cast<const typename Vec2<T>::type*>(tabs), reinterpret_cast<const typename Vec2<T>::type*>(psi), n, d, d_partial);
    TNQS_CHECK_LAUNCH();
}
template void launch_site_prob_partial<float>(hipStream_t, const void*, const void*, size_t, int, int, double*);
template void launch_site_prob_partial<double>(hipStream_t, const void*, const void*, size_t, int, int, double*);

void launch_site_draw(hipStream_t s, const double* d_partial, int nblocks, int d, double neg_tol, const double* d_uniform, unsigned long long seed,
                      unsigned long long sample, unsigned long long step, bool draw, double* d_p, int* d_x, double* d_px, int* d_status) {
    hipLaunchKernelGGL(site_draw_kernel, dim3(1), dim3(64), 0, s, d_partial, nblocks, d, neg_tol, d_uniform, seed, sample, step, draw ? 1 : 0, d_p, d_x, d_px, d_status);
    TNQS_CHECK_LAUNCH();
}
template <class T> void launch_site_project(hipStream_t s, const void* psi, void* out, size_t nout, int d, const int* d_x, int x_host) {
    if (!nout) return;
    size_t blocks = (nout + 255) / 256; if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL((site_project_kernel<T>), dim3((int)blocks), dim3(256), 0, s, reinterpret_cast<const T*>(psi), reinterpret_cast<T*>(out), nout, d, d_x, x_host);
    TNQS_CHECK_LAUNCH();
}
template void launch_site_project<float>(hipStream_t, const void*, void*, size_t, int, const int*, int);
template void launch_site_project<double>(hipStream_t, const void*, void*, size_t, int, const int*, int);

}  // namespace tnqs
