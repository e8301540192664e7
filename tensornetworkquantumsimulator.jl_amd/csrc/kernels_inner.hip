// kernels_inner.hip -- the overlap of two states by belief propagation (inner(psi, phi; alg = "bp"), src/inner.jl:65-69 over BilinearForm(ket, bra),
// src/Forms/bilinearform.jl:16-25): the kernels that differ from the norm network's, where bra = conj(ket) makes every message square and Hermitian.
//   inner_gram_kernel<T>      out[a + Ka b] = sum_{p, q} X[p, a, q] conj(Y[p, b, q]),  X = [PA][Ka][PB], Y = [PA][Kb][PB], Ka != Kb allowed, 1 <= Ka, Kb <= 64:
//                             the last step of updated_message (abstractbeliefpropagationcache.jl:162-190) with the ket tensor (messages absorbed) as X and the bra
//                             tensor as Y.  Matrix cores: v_mfma_f32_16x16x4_f32 (ComplexF32, f32 accumulation, as the BP message Gram) / v_mfma_f64_16x16x4_f64
//                             (ComplexF64).  The contracted range n = p + PA q is cut into blocks of TN = 32 (f32) / 16 (f64) indices; a workgroup (4 waves) owns one
//                             CHUNK of consecutive blocks of one item and writes one [Ka Kb] partial.  Per block the operands go through LDS as split (re, im) planes
//                             [row][n], rows padded with zeros to the 16 x 16 tile grid (ceil(Ka / 16) x ceil(Kb / 16) tiles, dealt round robin to the waves) and the
//                             tail of the range zero-filled: loads are masked, and only entries a < Ka, b < Kb of the item's own partials are stored.
//                             The instruction trait and the multiply phase of a block are CMfma16 and cplane_mm16<true> of device_common.hpp, which
//                             bmps_contract_kernel (kernels_bmps.hip) shares.
//                             A dimension beyond 64 is NOT taken (inner_gram_covers): the engine and the debug entry point answer TNQS_ERR_UNSUPPORTED, there is no
//                             scalar form.
//   inner_finalize_kernel<T>  the epilogue of a bilinear message (the contract of msg_finalize_kernel with rows x cols in place of chi^2): chunks summed in f64,
//                             m / sum(m) when the sum is not exactly zero (abstract...:182-187), message_diff (beliefpropagationcache.jl:17-21) against the previous
//                             message or the rectangular delta (delta(virtualinds(form, e))), the raw element sum kept for the vertex scalar.
//   inner_scalar_kernel<T>    sum_ab m[a, b] m'[a, b] in f64 (edge_scalar, beliefpropagationcache.jl:47-49, generalised to rows x cols), optionally times the raw element
//                             sum of m (vertex scalar from the normalised raw message) and the pending scale factors of the two site tensors.
#include "kernels.hpp"
#include "device_common.hpp"
#include "launch_util.hpp"

namespace tnqs {

namespace {
// several block-wide sums with one pair of barriers per call (blockDim.x <= 1024); results valid in every thread
template <int N> __device__ __forceinline__ void inner_block_sums(double (&v)[N], double* sh /* 17 N doubles */) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = wave_sum(v[k]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) sh[N * w + k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < N) { double t = 0; for (int i = 0; i < nw; ++i) t += sh[N * i + threadIdx.x]; sh[16 * N + threadIdx.x] = t; }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = sh[16 * N + k];
}
}  // namespace

template <class T>
__global__ __launch_bounds__(256) void inner_gram_kernel(const InnerGramItem* __restrict__ items, int nitems) {
    using M = CMfma16<T>;
    constexpr int TN = M::TN, LD = M::LD;
    __shared__ T xr[64 * LD], xi[64 * LD], yr[64 * LD], yi[64 * LD];
    const InnerGramItem it = items[find_item(items, nitems, &InnerGramItem::chunk_begin, (int)blockIdx.x)];
    const int chunk = (int)blockIdx.x - it.chunk_begin;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, g = lane >> 4;
    const int Ka = it.Ka, Kb = it.Kb, PA = it.PA;
    const int nta = (Ka + 15) >> 4, ntb = (Kb + 15) >> 4, ntiles = nta * ntb;
    const long long N = (long long)PA * it.PB;
    const long long nblk = (N + TN - 1) / TN;
    const long long b0 = (long long)chunk * it.blocks_per_chunk;
    long long b1 = b0 + it.blocks_per_chunk; if (b1 > nblk) b1 = nblk;
    const cx<T>* __restrict__ X = reinterpret_cast<const cx<T>*>(it.X);
    const cx<T>* __restrict__ Y = reinterpret_cast<const cx<T>*>(it.Y);
    typename M::Acc cr[4], ci[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) { cr[u][r] = 0; ci[u][r] = 0; }
    const int nl = tid % TN, r0 = tid / TN;
    constexpr int RS = 256 / TN;
    for (long long blk = b0; blk < b1; ++blk) {
        const long long n = blk * TN + nl;
        const bool live = n < N;
        const long long p = live ? n % PA : 0, q = live ? n / PA : 0;
        const cx<T>* xs = X + p + (size_t)PA * Ka * q;
        const cx<T>* ys = Y + p + (size_t)PA * Kb * q;
        __syncthreads();                                   // the previous block's operands have been consumed
        for (int a = r0; a < 16 * nta; a += RS) {
            cx<T> v = cmake<T>((T)0, (T)0);
            if (live && a < Ka) v = xs[(size_t)PA * a];
            xr[a * LD + nl] = v.re; xi[a * LD + nl] = v.im;
        }
        for (int b = r0; b < 16 * ntb; b += RS) {
            cx<T> v = cmake<T>((T)0, (T)0);
            if (live && b < Kb) v = ys[(size_t)PA * b];
            yr[b * LD + nl] = v.re; yi[b * LD + nl] = v.im;
        }
        __syncthreads();
        cplane_mm16<true>(xr, xi, yr, yi, nta, ntiles, cr, ci);      // x conj(y)
    }
    cx<T>* out = reinterpret_cast<cx<T>*>(it.partial) + (size_t)chunk * Ka * Kb;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int t = w + 4 * u;
        if (t < ntiles) {
            const int ta = t % nta, tb = t / nta, b = 16 * tb + c;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int a = 16 * ta + M::row(g, r);
                if (a < Ka && b < Kb) out[a + (size_t)Ka * b] = cmake<T>(cr[u][r], ci[u][r]);
            }
        }
    }
}

// chunks of a batch: blocks of TN contracted indices, `bpc` consecutive blocks per chunk.  max_chunks > 0: at most that many chunks per item (debug entry point);
// otherwise about 2048 chunks over the launch.  npart[i]: the partials item i leaves; returns the launch's workgroups
int plan_inner_gram(InnerGramItem* it, int n, size_t esz, int max_chunks, int* npart) {
    const int TN = esz == 8 ? 32 : 16;
    std::vector<long long> nblk(n); long long total = 0;
    for (int i = 0; i < n; ++i) { nblk[i] = ((long long)it[i].PA * it[i].PB + TN - 1) / TN; total += nblk[i]; }
    const long long launch_bpc = std::max<long long>(1, (total + 2047) / 2048);
    return lay_out(it, n, &InnerGramItem::chunk_begin, npart, [&](InnerGramItem& f) {
        const long long nb = nblk[&f - it];
        long long bpc = launch_bpc;
        if (max_chunks > 0) { const long long want = std::min<long long>(max_chunks, nb); bpc = (nb + want - 1) / want; }
        f.blocks_per_chunk = (int)bpc; f.nchunks = (int)((nb + bpc - 1) / bpc);
        return f.nchunks;
    });
}
template <class T> void launch_inner_gram(hipStream_t s, const InnerGramItem* d_items, int nitems, int total_chunks) {
    if (nitems <= 0 || total_chunks <= 0) return;
    hipLaunchKernelGGL((inner_gram_kernel<T>), dim3(total_chunks), dim3(256), 0, s, d_items, nitems); TNQS_CHECK_LAUNCH();
}
template void launch_inner_gram<float>(hipStream_t, const InnerGramItem*, int, int);
template void launch_inner_gram<double>(hipStream_t, const InnerGramItem*, int, int);

// ------------------------------------------------------------------------------------------------------------
// epilogue of a bilinear message: one workgroup per message, rows, cols <= 64 (at most four elements per thread, kept in f64 between the two passes)
// ------------------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(1024) void inner_finalize_kernel(const InnerFinalItem* __restrict__ items) {
    __shared__ double sh[17 * 4];
    const InnerFinalItem it = items[blockIdx.x];
    const int n2 = it.rows * it.cols, tid = threadIdx.x;
    const cx<T>* __restrict__ p = reinterpret_cast<const cx<T>*>(it.partial);
    const cx<T>* __restrict__ old = reinterpret_cast<const cx<T>*>(it.old_msg);
    cx<T>* out = reinterpret_cast<cx<T>*>(it.new_msg);
    double vr[4] = {0, 0, 0, 0}, vi[4] = {0, 0, 0, 0}, s2[2] = {0, 0};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int e = tid + 1024 * u;
        if (e < n2) {
            double ar[4] = {0, 0, 0, 0}, ai[4] = {0, 0, 0, 0};      // four independent sums, fixed order
            int ch = 0;
            for (; ch + 4 <= it.nchunks; ch += 4) {
#pragma unroll
                for (int k = 0; k < 4; ++k) { const cx<T> v = p[(size_t)(ch + k) * n2 + e]; ar[k] += (double)v.re; ai[k] += (double)v.im; }
            }
            for (; ch < it.nchunks; ++ch) { const cx<T> v = p[(size_t)ch * n2 + e]; ar[ch & 3] += (double)v.re; ai[ch & 3] += (double)v.im; }
            vr[u] = (ar[0] + ar[1]) + (ar[2] + ar[3]); vi[u] = (ai[0] + ai[1]) + (ai[2] + ai[3]);
            s2[0] += vr[u]; s2[1] += vi[u];
        }
    }
    inner_block_sums<2>(s2, sh);
    const double sre = s2[0], sim = s2[1];
    double ire = 1, iim = 0;
    if (it.normalize && (sre != 0 || sim != 0)) { const double d = sre * sre + sim * sim; ire = sre / d; iim = -sim / d; }
    double d4[4] = {0, 0, 0, 0};       // Re, Im of dot(new, old), |new|^2, |old|^2
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int e = tid + 1024 * u;
        if (e < n2) {
            const cx<T> wv = cmake<T>((T)(vr[u] * ire - vi[u] * iim), (T)(vr[u] * iim + vi[u] * ire));
            out[e] = wv;
            double ore, oim;
            if (old) { ore = old[e].re; oim = old[e].im; } else { ore = (e % it.rows == e / it.rows) ? 1.0 : 0.0; oim = 0; }
            d4[0] += (double)wv.re * ore + (double)wv.im * oim;
            d4[1] += (double)wv.re * oim - (double)wv.im * ore;
            d4[2] += (double)wv.re * wv.re + (double)wv.im * wv.im;
            d4[3] += ore * ore + oim * oim;
        }
    }
    inner_block_sums<4>(d4, sh);
    if (tid == 0) {
        if (it.diff_out) *it.diff_out = 1.0 - (d4[0] * d4[0] + d4[1] * d4[1]) / (d4[2] * d4[3]);
        if (it.sum_out) { it.sum_out[0] = sre; it.sum_out[1] = sim; }
    }
}
template <class T> void launch_inner_finalize(hipStream_t s, const InnerFinalItem* d_items, int nitems) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL((inner_finalize_kernel<T>), dim3(nitems), dim3(1024), 0, s, d_items); TNQS_CHECK_LAUNCH();
}
template void launch_inner_finalize<float>(hipStream_t, const InnerFinalItem*, int);
template void launch_inner_finalize<double>(hipStream_t, const InnerFinalItem*, int);

// ------------------------------------------------------------------------------------------------------------
// vertex and edge scalars of the form network, one workgroup each
// ------------------------------------------------------------------------------------------------------------
template <class T> __device__ __forceinline__ cx<double> inner_msg_elem(const cx<T>* m, int e, int rows) {
    if (m) return cmake<double>((double)m[e].re, (double)m[e].im);
    return cmake<double>((e % rows) == (e / rows) ? 1.0 : 0.0, 0.0);
}
template <class T> __global__ __launch_bounds__(256) void inner_scalar_kernel(const InnerScalarItem* __restrict__ items) {
    __shared__ double sh[17 * 2];
    const InnerScalarItem it = items[blockIdx.x];
    const cx<T>* a = reinterpret_cast<const cx<T>*>(it.m); const cx<T>* b = reinterpret_cast<const cx<T>*>(it.mr);
    const int n2 = it.rows * it.cols;
    double pr[2] = {0, 0};
    for (int e = threadIdx.x; e < n2; e += 256) {
        const cx<double> x = inner_msg_elem(a, e, it.rows), y = inner_msg_elem(b, e, it.rows);
        pr[0] += x.re * y.re - x.im * y.im; pr[1] += x.re * y.im + x.im * y.re;
    }
    inner_block_sums<2>(pr, sh);
    if (threadIdx.x == 0) {
        double re = pr[0], im = pr[1];
        if (it.rawsum) {                                   // m is raw / sum(raw) unless the epilogue left it as it was
            const double sr = it.rawsum[0], si = it.rawsum[1];
            if (it.normalize && (sr != 0 || si != 0)) { const double t = re * sr - im * si; im = re * si + im * sr; re = t; }
        }
        double f = 1.0;
        if (it.scale_a) f *= *it.scale_a;
        if (it.scale_b) f *= *it.scale_b;
        it.out[0] = re * f; it.out[1] = im * f;
    }
}
template <class T> void launch_inner_scalar(hipStream_t s, const InnerScalarItem* d_items, int nitems) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL((inner_scalar_kernel<T>), dim3(nitems), dim3(256), 0, s, d_items); TNQS_CHECK_LAUNCH();
}
template void launch_inner_scalar<float>(hipStream_t, const InnerScalarItem*, int);
template void launch_inner_scalar<double>(hipStream_t, const InnerScalarItem*, int);

}  // namespace tnqs
