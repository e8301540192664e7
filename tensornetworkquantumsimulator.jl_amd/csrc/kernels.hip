// kernels.hip -- generic (any dims, c64/c128) HIP kernels of the BP-gauged gate-application path, gfx950.
// These are the always-correct fiber-tile kernels; the MFMA fast paths for the hot shapes live in
// kernels_mfma.hip and are validated against these.  (The other kernel families: the file map of engine_internal.hpp.)
//
// Reference call sites replaced (paths relative to the reference repo):
//   fiber_gemm  : ITensors `contract`/`apply` in src/Apply/simple_update.jl:27,43-44,62-64 and the message
//                 absorptions of src/MessagePassing/abstractbeliefpropagationcache.jl:180
//   gram        : final contraction with dag(prime(psi)) (abstract...:180) and the R-factor Gram of the QR
//                 step (simple_update.jl:47-48, replaced by an f64 Gram + eigen factorisation)
#include "kernels.hpp"
#include "device_common.hpp"

namespace tnqs {

// ------------------------------------------------------------------------------------------------------------
// fiber_gemm
// ------------------------------------------------------------------------------------------------------------
template <class T, int NB>
__global__ __launch_bounds__(256) void fiber_gemm_kernel(const FiberItem* __restrict__ items, int nitems, int TR,
                                                         double* __restrict__ norm_partials) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cx<T>* tile = reinterpret_cast<cx<T>*>(smem);
    __shared__ double sh_red[17];
    const int tid = threadIdx.x;
    const int gt = blockIdx.x;
    const int lo = find_item(items, nitems, &FiberItem::tile_begin, gt);
    const FiberItem it = items[lo];
    const int lt = gt - it.tile_begin;
    const int ta = lt % it.nta, tb = lt / it.nta;
    const int a0 = ta * it.TA, b0 = tb * it.TB;
    const int na = min(it.TA, it.PA - a0), nb = min(it.TB, it.PB - b0);
    const int D = it.D, K = it.K, TA = it.TA, TB = it.TB, KK = D * K;
    const size_t PA = it.PA;
    const cx<T>* __restrict__ in = reinterpret_cast<const cx<T>*>(it.in);
    const int ntile_el = D * TA * K * TB;
    for (int e = tid; e < ntile_el; e += 256) {
        int s = e % D; int r1 = e / D; int al = r1 % TA; int r2 = r1 / TA; int k = r2 % K; int bl = r2 / K;
        cx<T> v = cmake<T>(0, 0);
        if (al < na && bl < nb) v = in[s + D * ((size_t)(a0 + al) + PA * ((size_t)k + (size_t)K * (b0 + bl)))];
        tile[(s + D * k) * TR + (al + TA * bl)] = v;
    }
    __syncthreads();
    const int Do = it.Do, No = it.No, NN = Do * No;
    const int r = tid % TR, g = tid / TR, G = 256 / TR;
    const int al = r % TA, bl = r / TA;
    const bool valid = (r < TA * TB) && al < na && bl < nb;
    const cx<T>* __restrict__ X = reinterpret_cast<const cx<T>*>(it.X);
    cx<T>* __restrict__ out = reinterpret_cast<cx<T>*>(it.out);
    double nrm = 0;
    for (int nn0 = g * NB; nn0 < NN; nn0 += G * NB) {
        cx<T> acc[NB];
        int col[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) { acc[j] = cmake<T>(0, 0); col[j] = min(nn0 + j, NN - 1) * KK; }
        for (int kk = 0; kk < KK; ++kk) {
            const cx<T> a = tile[kk * TR + r];
#pragma unroll
            for (int j = 0; j < NB; ++j) cfma(acc[j], a, X[col[j] + kk]);
        }
        if (valid) {
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                int nn = nn0 + j;
                if (nn < NN) {
                    int sp = nn % Do, n = nn / Do;
                    out[sp + Do * ((size_t)(a0 + al) + PA * ((size_t)n + (size_t)No * (b0 + bl)))] = acc[j];
                    nrm += (double)acc[j].re * acc[j].re + (double)acc[j].im * acc[j].im;
                }
            }
        }
    }
    if (it.want_norm) {   // uniform per block
        double t = block_sum(nrm, sh_red);
        if (tid == 0) norm_partials[gt] = t;
    }
}

template <class T>
void launch_fiber_gemm(hipStream_t s, const FiberItem* d_items, int nitems, int total_tiles, int TR, int KKmax,
                       double* d_norm_partials) {
    if (total_tiles <= 0) return;
    size_t lds = (size_t)KKmax * TR * sizeof(cx<T>);
    hipLaunchKernelGGL((fiber_gemm_kernel<T, 8>), dim3(total_tiles), dim3(256), lds, s, d_items, nitems, TR, d_norm_partials); TNQS_CHECK_LAUNCH();
}
template void launch_fiber_gemm<float>(hipStream_t, const FiberItem*, int, int, int, int, double*);
template void launch_fiber_gemm<double>(hipStream_t, const FiberItem*, int, int, int, int, double*);
// a planned launch (plan_fiber_pass, fiber_plan.cpp) on the launcher of its route
template <class T>
void launch_fiber_route(hipStream_t s, const FiberLaunch& L, const FiberItem* d, double* np) {
    const int n = (int)L.items.size();
    switch (L.route) {
    case FiberRoute::RowGemm: launch_mfma_rowgemm(s, d, n, L.wgs, L.D, L.K, np); break;
    case FiberRoute::F64: launch_mfma_fiber_gemm_f64(s, d, n, L.wgs, L.KKmax, L.NNmax, np, L.general); break;
    case FiberRoute::Mfma: launch_mfma_fiber_gemm(s, d, n, L.wgs, L.KKmax, L.NNmax, np); break;
    case FiberRoute::Generic: launch_fiber_gemm<T>(s, d, n, L.wgs, L.TR, L.KKmax, np); break;
    }
}
template void launch_fiber_route<float>(hipStream_t, const FiberLaunch&, const FiberItem*, double*);
template void launch_fiber_route<double>(hipStream_t, const FiberLaunch&, const FiberItem*, double*);

// ------------------------------------------------------------------------------------------------------------
// gram
// ------------------------------------------------------------------------------------------------------------
template <class T, class Acc, int MAXB>
__global__ __launch_bounds__(256) void gram_kernel(const GramItem* __restrict__ items, int nitems, int TR) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int gc = blockIdx.x;
    const int lo = find_item(items, nitems, &GramItem::chunk_begin, gc);
    const GramItem it = items[lo];
    const int lc = gc - it.chunk_begin;
    const int D = it.D, K = it.K, TA = it.TA, TB = it.TB, KK = D * K;
    const int KKp = KK + 1;                      // row pitch of the LDS tiles [row][kk]
    const size_t PA = it.PA;
    const bool same = (it.X == it.Y);
    cx<T>* Xt = reinterpret_cast<cx<T>*>(smem);
    cx<T>* Yt = same ? Xt : Xt + (size_t)TR * KKp;
    const cx<T>* __restrict__ Xg = reinterpret_cast<const cx<T>*>(it.X);
    const cx<T>* __restrict__ Yg = reinterpret_cast<const cx<T>*>(it.Y);
    const int KB = (KK + 1) >> 1;                // 2x2 output blocks per dimension
    const int nblk = KB * KB;
    const int ntiles = it.nta * it.ntb;
    const int t_begin = lc * it.tiles_per_chunk;
    const int t_end = min(ntiles, t_begin + it.tiles_per_chunk);
    cx<Acc>* __restrict__ part = reinterpret_cast<cx<Acc>*>(it.partial) + (size_t)lc * KK * KK;
    const int ntile_el = D * TA * K * TB;
    for (int pass0 = 0; pass0 < nblk; pass0 += 256 * MAXB) {
        cx<Acc> acc[MAXB][4];
        int bi[MAXB], bj[MAXB];
#pragma unroll
        for (int j = 0; j < MAXB; ++j) {
            int q = pass0 + tid + 256 * j;
            int qq = min(q, nblk - 1);
            bi[j] = qq % KB; bj[j] = qq / KB;
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[j][c] = cmake<Acc>(0, 0);
        }
        for (int t = t_begin; t < t_end; ++t) {
            const int ta = t % it.nta, tb = t / it.nta;
            const int a0 = ta * TA, b0 = tb * TB;
            const int na = min(TA, it.PA - a0), nb = min(TB, it.PB - b0);
            __syncthreads();
            for (int e = tid; e < ntile_el; e += 256) {
                int s = e % D; int r1 = e / D; int al = r1 % TA; int r2 = r1 / TA; int k = r2 % K; int bl = r2 / K;
                cx<T> vx = cmake<T>(0, 0), vy = cmake<T>(0, 0);
                if (al < na && bl < nb) {
                    size_t off = s + D * ((size_t)(a0 + al) + PA * ((size_t)k + (size_t)K * (b0 + bl)));
                    vx = Xg[off];
                    if (!same) vy = Yg[off];
                }
                int li = (al + TA * bl) * KKp + (s + D * k);
                Xt[li] = vx;
                if (!same) Yt[li] = vy;
            }
            // zero the pad column so clamped reads of index KK (odd KK) are harmless
            for (int e = tid; e < TA * TB; e += 256) { Xt[e * KKp + KK] = cmake<T>(0, 0); if (!same) Yt[e * KKp + KK] = cmake<T>(0, 0); }
            __syncthreads();
            const int nrow = TA * TB;
            for (int rr = 0; rr < nrow; ++rr) {
                const cx<T>* xr = Xt + rr * KKp;
                const cx<T>* yr = Yt + rr * KKp;
#pragma unroll
                for (int j = 0; j < MAXB; ++j) {
                    cx<T> x0 = xr[2 * bi[j]], x1 = xr[2 * bi[j] + 1];
                    cx<T> y0 = yr[2 * bj[j]], y1 = yr[2 * bj[j] + 1];
                    cx<Acc> X0 = cmake<Acc>(x0.re, x0.im), X1 = cmake<Acc>(x1.re, x1.im);
                    cx<Acc> Y0 = cmake<Acc>(y0.re, y0.im), Y1 = cmake<Acc>(y1.re, y1.im);
                    cfma_conj(acc[j][0], X0, Y0); cfma_conj(acc[j][1], X1, Y0);
                    cfma_conj(acc[j][2], X0, Y1); cfma_conj(acc[j][3], X1, Y1);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < MAXB; ++j) {
            int q = pass0 + tid + 256 * j;
            if (q < nblk) {
                int i0 = 2 * bi[j], j0 = 2 * bj[j];
                part[i0 + (size_t)KK * j0] = acc[j][0];
                if (i0 + 1 < KK) part[i0 + 1 + (size_t)KK * j0] = acc[j][1];
                if (j0 + 1 < KK) {
                    part[i0 + (size_t)KK * (j0 + 1)] = acc[j][2];
                    if (i0 + 1 < KK) part[i0 + 1 + (size_t)KK * (j0 + 1)] = acc[j][3];
                }
            }
        }
    }
}

template <class T, class Acc>
void launch_gram(hipStream_t s, const GramItem* d_items, int nitems, int total_chunks, int TR, int KKmax) {
    if (total_chunks <= 0) return;
    size_t lds = 2 * (size_t)TR * (KKmax + 1) * sizeof(cx<T>);
    hipLaunchKernelGGL((gram_kernel<T, Acc, 4>), dim3(total_chunks), dim3(256), lds, s, d_items, nitems, TR); TNQS_CHECK_LAUNCH();
}
template void launch_gram<float, float>(hipStream_t, const GramItem*, int, int, int, int);
template void launch_gram<float, double>(hipStream_t, const GramItem*, int, int, int, int);
template void launch_gram<double, double>(hipStream_t, const GramItem*, int, int, int, int);

// M set: the BP Gram absorbs the first row leg (f32 accumulation, mfma_gram32_fused_kernel); the gate-path Gram (f64 accumulation)
// absorbs the last gauge leg (mfma_gauge_gram64_kernel; 16-dimensional legs: the wave-private mfma_gauge_gram32_kernel) -- a batch is one or the other
GramRoute gram_route(bool f32, bool acc64, bool has_M, bool all_same, bool all_f64in, size_t KKmax, bool use_mfma, bool use_chi64) {
    const bool f32_acc64 = f32 && acc64;
    if (has_M) return f32_acc64 ? (KKmax == 32 ? GramRoute::Gauge32 : GramRoute::Gauge64) : GramRoute::Fused32;
    if (f32_acc64 && use_mfma && all_same && KKmax <= 64 && KKmax >= 16) return GramRoute::F64x64;
    if (f32_acc64 && use_mfma && use_chi64 && all_same && KKmax <= 128 && KKmax > 64) return GramRoute::F64x128;
    if (!f32 && use_mfma && all_f64in) return GramRoute::F64In;          // ComplexF64 operands: tiles of 32 fibers through LDS, f64 matrix cores (kernels_f64.hip)
    if (f32 && !acc64 && use_mfma && KKmax <= (use_chi64 ? 64u : 32u) && KKmax >= 8) return KKmax <= 32 ? GramRoute::Mfma32 : GramRoute::Mfma64;
    return GramRoute::Generic;
}
int gram_tile_rows(GramRoute r, size_t KKmax, size_t esz) {
    const int tr = pick_TR(KKmax + 1, esz, 2);          // the generic kernel: two operand blocks in LDS
    return r == GramRoute::Generic ? tr : r == GramRoute::F64In ? 32 : 64;
}
// The f64 Grams of f32 data write one 64 KiB partial per (site, chunk, tile parity) which reduce_kernel reads back: 2048 chunks per launch were 268 MB and
// 85-90 us per colour batch of the gate path WHATEVER its size; 1024 (four workgroups per CU) halves that and costs the Gram pass nothing measurable.
// Partials per chunk: one per wave on the 32 x 32 f32 matrix-core kernels, one per tile parity on the f64 64 x 64 one, one otherwise.
int plan_gram(GramItem* it, int n, GramRoute r, bool f32_acc64, int max_chunks, int* npart) {
    if (max_chunks <= 0) max_chunks = std::max(1, (f32_acc64 ? 1024 : 2048) / n);
    const int per_chunk = (r == GramRoute::Mfma32 || r == GramRoute::Fused32) ? 4 : (r == GramRoute::F64x64 || r == GramRoute::Gauge64) ? 2 : 1;
    const int chunks = lay_out(it, n, &GramItem::chunk_begin, npart, [&](GramItem& g) {
        const int ntiles = g.nta * g.ntb, nch = std::min(max_chunks, ntiles);
        g.tiles_per_chunk = (ntiles + nch - 1) / nch; g.nchunks = (ntiles + g.tiles_per_chunk - 1) / g.tiles_per_chunk;
        return g.nchunks; });
    if (npart) for (int i = 0; i < n; ++i) npart[i] *= per_chunk;
    return chunks;
}
template <class T, class Acc>
void launch_gram_route(hipStream_t s, GramRoute r, const GramItem* d, int n, int chunks, int TR, int KKmax, bool all_full) {
    switch (r) {
    case GramRoute::Gauge32: launch_mfma_gauge_gram32(s, d, n, chunks); break; case GramRoute::Gauge64: launch_mfma_gauge_gram64(s, d, n, chunks); break;
    case GramRoute::F64x64: launch_mfma_gram64_f64(s, d, n, chunks, KKmax, all_full); break; case GramRoute::F64x128: launch_mfma_gram128_f64(s, d, n, chunks, KKmax, all_full); break;
    case GramRoute::Mfma32: launch_mfma_gram32(s, d, n, chunks, KKmax); break; case GramRoute::Mfma64: launch_mfma_gram64(s, d, n, chunks, KKmax); break;
    case GramRoute::Fused32: launch_mfma_gram32_fused(s, d, n, chunks); break; case GramRoute::F64In: launch_mfma_gram_f64in(s, d, n, chunks); break;
    case GramRoute::Generic: launch_gram<T, Acc>(s, d, n, chunks, TR, KKmax); break;
    }
}
template void launch_gram_route<float, float>(hipStream_t, GramRoute, const GramItem*, int, int, int, int, bool);
template void launch_gram_route<float, double>(hipStream_t, GramRoute, const GramItem*, int, int, int, int, bool);
template void launch_gram_route<double, double>(hipStream_t, GramRoute, const GramItem*, int, int, int, int, bool);

// ------------------------------------------------------------------------------------------------------------
// reduce partials
// ------------------------------------------------------------------------------------------------------------
template <class Acc, class Out>
__global__ __launch_bounds__(256) void reduce_kernel(const ReduceItem* __restrict__ items, int nitems, int total) {
    int ge = blockIdx.x * 256 + threadIdx.x;
    if (ge >= total) return;
    const int lo = find_item(items, nitems, &ReduceItem::elem_begin, ge);
    const ReduceItem it = items[lo];
    int e = ge - it.elem_begin;
    const cx<Acc>* p = reinterpret_cast<const cx<Acc>*>(it.partial);
    Acc re = 0, im = 0;
    for (int c = 0; c < it.nchunks; ++c) { cx<Acc> v = p[(size_t)c * it.n2 + e]; re += v.re; im += v.im; }
    if (it.conj) im = -im;
    reinterpret_cast<cx<Out>*>(it.out)[e] = cmake<Out>((Out)re, (Out)im);
}
template <class Acc, class Out>
void launch_reduce(hipStream_t s, const ReduceItem* d_items, int nitems, int total_elems) {
    if (total_elems <= 0) return;
    hipLaunchKernelGGL((reduce_kernel<Acc, Out>), dim3((total_elems + 255) / 256), dim3(256), 0, s, d_items, nitems, total_elems); TNQS_CHECK_LAUNCH();
}
template void launch_reduce<double, double>(hipStream_t, const ReduceItem*, int, int);
template void launch_reduce<float, float>(hipStream_t, const ReduceItem*, int, int);
template void launch_reduce<double, float>(hipStream_t, const ReduceItem*, int, int);

}  // namespace tnqs
