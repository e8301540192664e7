// kernels_util.hip -- small utilities: diagonals, norms, scaling, record packing, permutation, identity / random fill, one-site gates, sums.
#include "kernels.hpp"
#include "device_common.hpp"

namespace tnqs {

// ------------------------------------------------------------------------------------------------------------
// small utilities
// ------------------------------------------------------------------------------------------------------------
template <class T> __global__ void diag_kernel(const DiagItem* __restrict__ items) {
    const DiagItem it = items[blockIdx.x];
    cx<T>* out = reinterpret_cast<cx<T>*>(it.out);
    for (int e = threadIdx.x; e < it.chi * it.chi; e += blockDim.x) {
        int i = e % it.chi, j = e / it.chi;
        out[e] = cmake<T>(i == j ? (T)it.S[i] : (T)0, (T)0);
    }
}
template <class T> void launch_diag(hipStream_t s, const DiagItem* d_items, int nitems) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL((diag_kernel<T>), dim3(nitems), dim3(256), 0, s, d_items); TNQS_CHECK_LAUNCH();
}
template void launch_diag<float>(hipStream_t, const DiagItem*, int);
template void launch_diag<double>(hipStream_t, const DiagItem*, int);

__global__ __launch_bounds__(256) void norm_factor_kernel(const NormFactorItem* __restrict__ items) {
    __shared__ double sh[17];
    const NormFactorItem it = items[blockIdx.x];
    double t = 0;
    for (int i = threadIdx.x; i < it.npart; i += 256) t += it.norm_partials[i];
    // fixed-order reduction would need a second pass; the block_sum order is deterministic for a given launch shape
    t = block_sum(t, sh);
    if (threadIdx.x == 0) *it.factor = (t > 0) ? 1.0 / sqrt(t) : 1.0;
}
void launch_norm_factor(hipStream_t s, const NormFactorItem* d_items, int nitems) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL(norm_factor_kernel, dim3(nitems), dim3(256), 0, s, d_items); TNQS_CHECK_LAUNCH();
}
template <class T> __global__ __launch_bounds__(256) void scale_kernel(const ScaleItem* __restrict__ items) {
    const ScaleItem it = items[blockIdx.y];
    const T f = (T)(*it.factor);
    const cx<T>* __restrict__ p = reinterpret_cast<const cx<T>*>(it.src);
    cx<T>* __restrict__ q = reinterpret_cast<cx<T>*>(it.dst);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < it.n; i += (size_t)gridDim.x * 256) {
        cx<T> v = p[i]; q[i] = cmake<T>(v.re * f, v.im * f);
    }
}
template <class T> void launch_scale(hipStream_t s, const ScaleItem* d_items, int nitems) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL((scale_kernel<T>), dim3(64, nitems), dim3(256), 0, s, d_items); TNQS_CHECK_LAUNCH();
}
template void launch_scale<float>(hipStream_t, const ScaleItem*, int);
template void launch_scale<double>(hipStream_t, const ScaleItem*, int);

template <class T> __global__ __launch_bounds__(256) void cscale_kernel(const CScaleItem* __restrict__ items) {
    const CScaleItem it = items[blockIdx.y];
    const double fr = it.re, fi = it.im;
    const cx<T>* __restrict__ p = reinterpret_cast<const cx<T>*>(it.src);
    cx<T>* __restrict__ q = reinterpret_cast<cx<T>*>(it.dst);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < it.n; i += (size_t)gridDim.x * 256) {
        cx<T> v = p[i]; q[i] = cmake<T>((T)(v.re * fr - v.im * fi), (T)(v.re * fi + v.im * fr));
    }
}
template <class T> void launch_cscale(hipStream_t s, const CScaleItem* d_items, int nitems) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL((cscale_kernel<T>), dim3(64, nitems), dim3(256), 0, s, d_items); TNQS_CHECK_LAUNCH();
}
template void launch_cscale<float>(hipStream_t, const CScaleItem*, int);
template void launch_cscale<double>(hipStream_t, const CScaleItem*, int);

__global__ __launch_bounds__(256) void record_pack_kernel(const RecordPackItem* __restrict__ items) {
    const RecordPackItem it = items[blockIdx.x];
    char* dst = reinterpret_cast<char*>(it.dst);
    if (threadIdx.x == 0) { double* h = reinterpret_cast<double*>(dst); h[0] = (double)it.info[2]; h[1] = (double)it.info[3]; h[2] = *it.terr; h[3] = 0.0; }
    double* sd = reinterpret_cast<double*>(dst + 32);
    for (int i = threadIdx.x; i < it.nS; i += 256) sd[i] = it.S[i];
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(it.X2);
    unsigned long long* xd = reinterpret_cast<unsigned long long*>(dst + it.x2_off);
    for (long long i = threadIdx.x; i < it.x2_words; i += 256) xd[i] = src[i];
}
void launch_record_pack(hipStream_t s, const RecordPackItem* d_items, int nitems) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL(record_pack_kernel, dim3(nitems), dim3(256), 0, s, d_items); TNQS_CHECK_LAUNCH();
}
__global__ void header_gather_kernel(const void* const* __restrict__ srcs, int n, double* __restrict__ out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 4 * n) out[i] = reinterpret_cast<const double*>(srcs[i >> 2])[i & 3];
}
void launch_header_gather(hipStream_t s, const void* const* d_srcs, int n, double* d_out) {
    if (n <= 0) return;
    hipLaunchKernelGGL(header_gather_kernel, dim3((4 * n + 255) / 256), dim3(256), 0, s, d_srcs, n, d_out); TNQS_CHECK_LAUNCH();
}

template <class T> __global__ __launch_bounds__(256) void permute_kernel(PermItem it) {
    const cx<T>* in = reinterpret_cast<const cx<T>*>(it.in);
    cx<T>* out = reinterpret_cast<cx<T>*>(it.out);
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < it.n; e += (size_t)gridDim.x * 256) {
        size_t rem = e; long long off = 0;
        for (int k = 0; k < it.ndim; ++k) { int idx = (int)(rem % it.dims_out[k]); rem /= it.dims_out[k]; off += idx * it.stride_in[k]; }
        out[e] = in[off];     // pure data movement: bit-exact
    }
}
template <class T> void launch_permute(hipStream_t s, const PermItem& item) {
    if (item.n == 0) return;
    int blocks = (int)((item.n + 255) / 256); if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL((permute_kernel<T>), dim3(blocks), dim3(256), 0, s, item); TNQS_CHECK_LAUNCH();
}
template void launch_permute<float>(hipStream_t, const PermItem&);
template void launch_permute<double>(hipStream_t, const PermItem&);

template <class T> __global__ void identity_kernel(cx<T>* out, int n) {
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n * n; e += gridDim.x * blockDim.x)
        out[e] = cmake<T>((e % n) == (e / n) ? (T)1 : (T)0, (T)0);
}
// iid standard-normal (re, im) pairs from a counter-based generator: entry e <- splitmix64(seed + e) -> two uniforms -> Box-Muller
__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull; x = (x ^ (x >> 27)) * 0x94D049BB133111EBull; return x ^ (x >> 31);
}
template <class T> __global__ __launch_bounds__(256) void random_fill_kernel(cx<T>* out, size_t n, unsigned long long seed, double scale, int real_only) {
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const unsigned long long r = splitmix64(seed + 0xD1B54A32D192ED03ull * (unsigned long long)e);
        const double u1 = ((double)(r >> 32) + 1.0) * (1.0 / 4294967296.0), u2 = (double)(r & 0xffffffffull) * (1.0 / 4294967296.0);
        const double rad = sqrt(-2.0 * log(u1)) * scale; double sn, cs; sincospi(2.0 * u2, &sn, &cs);
        out[e] = cmake<T>((T)(rad * cs), real_only ? (T)0 : (T)(rad * sn));
    }
}
template <class T> void launch_random_fill(hipStream_t s, void* out, size_t n, unsigned long long seed, double scale, bool real_only) {
    if (!n) return;
    const int blocks = (int)std::min<size_t>((n + 255) / 256, 65536);
    hipLaunchKernelGGL((random_fill_kernel<T>), dim3(blocks), dim3(256), 0, s, reinterpret_cast<cx<T>*>(out), n, seed, scale, real_only ? 1 : 0); TNQS_CHECK_LAUNCH();
}
template void launch_random_fill<float>(hipStream_t, void*, size_t, unsigned long long, double, bool);
template void launch_random_fill<double>(hipStream_t, void*, size_t, unsigned long long, double, bool);
template <class T> void launch_identity(hipStream_t s, void* out, int n) {
    hipLaunchKernelGGL((identity_kernel<T>), dim3((n * n + 255) / 256), dim3(256), 0, s, reinterpret_cast<cx<T>*>(out), n); TNQS_CHECK_LAUNCH();
}
template void launch_identity<float>(hipStream_t, void*, int);
template void launch_identity<double>(hipStream_t, void*, int);

// one-site gate, d = 2, ComplexF32: out[s'] = sum_s G[s',s] in[s] on 16-byte (s=0,1) pairs; K11 of SURVEY.md 2
__global__ __launch_bounds__(256) void site1_c64_kernel(const Site1Item* __restrict__ items, double* __restrict__ norm_partials) {
    __shared__ double sh[17];
    const Site1Item it = items[blockIdx.y];
    const float4* __restrict__ in = reinterpret_cast<const float4*>(it.in);
    float4* __restrict__ out = reinterpret_cast<float4*>(it.out);
    const float g00r = it.g[0], g00i = it.g[1], g01r = it.g[2], g01i = it.g[3], g10r = it.g[4], g10i = it.g[5], g11r = it.g[6], g11i = it.g[7];
    double nrm = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < it.npairs; i += (size_t)gridDim.x * 256) {
        float4 a = in[i];                       // (a0.re, a0.im, a1.re, a1.im)
        float4 o;
        o.x = g00r * a.x - g00i * a.y + g01r * a.z - g01i * a.w;
        o.y = g00r * a.y + g00i * a.x + g01r * a.w + g01i * a.z;
        o.z = g10r * a.x - g10i * a.y + g11r * a.z - g11i * a.w;
        o.w = g10r * a.y + g10i * a.x + g11r * a.w + g11i * a.z;
        out[i] = o;
        nrm += (double)o.x * o.x + (double)o.y * o.y + (double)o.z * o.z + (double)o.w * o.w;
    }
    if (norm_partials) {
        double t = block_sum(nrm, sh);
        if (threadIdx.x == 0) norm_partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
    }
}
void launch_site1_c64(hipStream_t s, const Site1Item* d_items, int nitems, int nbx, double* d_norm_partials) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL(site1_c64_kernel, dim3(nbx, nitems), dim3(256), 0, s, d_items, d_norm_partials); TNQS_CHECK_LAUNCH();
}

__global__ void sum_doubles_kernel(const double* in, int n, double* out) {
    __shared__ double sh[17];
    double t = 0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) t += in[i];
    t = block_sum(t, sh);
    if (threadIdx.x == 0) *out = t;
}
void launch_sum_doubles(hipStream_t s, const double* in, int n, double* out) {
    hipLaunchKernelGGL(sum_doubles_kernel, dim3(1), dim3(256), 0, s, in, n, out); TNQS_CHECK_LAUNCH();
}

}  // namespace tnqs
