// kernels_bmps.hip -- boundary MPS (src/MessagePassing/boundarympscache.jl): the kernels of the fitting update of an interpartition message and of the measurement.
//   bmps_contract_kernel<T>   C[m, n] = sum_k A[m, k] B[k, n] (B conjugated on request) where m, n and k are each a group of up to four legs with their own element
//                             strides in A, B and C (BmpsContractItem, kernels.hpp): every step of updated_message (abstractbeliefpropagationcache.jl:162-190) on a double-layer
//                             site with its incoming MPS tensors and environments is one such product, and no operand is ever written out in a permuted layout.
//                             Matrix cores: v_mfma_f32_16x16x4_f32 (ComplexF32, f32 accumulation) / v_mfma_f64_16x16x4_f64 (ComplexF64), four real products per complex
//                             rank-4 update.  A workgroup (4 waves) owns a 64 x 64 tile of (m, n) and one chunk of consecutive blocks of TN = 32 (f32) / 16 (f64)
//                             contracted indices; per block the operands go through LDS as split (re, im) planes [row][k], rows padded with zeros to the 16 x 16 tile
//                             grid of the tile's live part and the tail of the range zero-filled: loads are masked, and only entries m < M, n < N of the item's own
//                             output are stored.  The instruction trait and the multiply phase of a block are CMfma16 and cplane_mm16<false> of device_common.hpp
//                             (B is conjugated while it is staged), which inner_gram_kernel (kernels_inner.hip) shares.  Items of different shape share a launch (find_item).
//   bmps_reduce_kernel<T>     the chunks of an item summed in f64 and stored through the output strides -- as complex128 for the scalars of a call.
//   bmps_qr_kernel<T>         thin Householder QR A = Q Y, m >= n, n <= 64 (gauge_step!, boundarympscache.jl:270-285: factorize(...; ortho = "left")), one workgroup per
//                             matrix.  Householder because the initial guess of a message (:180-202) is a product state: its matricisations have rank 1, and Q^dagger Q = I
//                             has to hold for them.  A reflector built from a column that is zero below the diagonal is the identity (tau = 0), one built from rounding noise
//                             is still unitary.  Dot products are accumulated in f64 for both element types.
//   bmps_norm_kernel<T>       ||m||_2 in f64, m / ||m||, conjugated: norm, normalize and inserter! of the sweep (:352-358) in one pass.
#include "kernels.hpp"
#include "device_common.hpp"
#include "launch_util.hpp"
#include <algorithm>
#include <string>

namespace tnqs {

namespace {
// offsets of the combined index idx of a leg group in two tensors / in one
__device__ __forceinline__ void bmps_split2(long long idx, int n, const int* dim, const long long* s1, const long long* s2, long long& o1, long long& o2) {
    o1 = 0; o2 = 0;
    for (int q = 0; q < n; ++q) { const long long i = idx % dim[q]; idx /= dim[q]; o1 += i * s1[q]; o2 += i * s2[q]; }
}
__device__ __forceinline__ long long bmps_split1(long long idx, int n, const int* dim, const long long* s1) {
    long long o = 0;
    for (int q = 0; q < n; ++q) { const long long i = idx % dim[q]; idx /= dim[q]; o += i * s1[q]; }
    return o;
}
}  // namespace

template <class T>
__global__ __launch_bounds__(256) void bmps_contract_kernel(const BmpsContractItem* __restrict__ items, int nitems) {
    using Mf = CMfma16<T>;
    constexpr int TN = Mf::TN, LD = Mf::LD, RS = 256 / TN, NR = 64 / RS;
    __shared__ T xr[64 * LD], xi[64 * LD], yr[64 * LD], yi[64 * LD];
    __shared__ BmpsContractItem it;
    if (threadIdx.x == 0) it = items[find_item(items, nitems, &BmpsContractItem::wg_begin, (int)blockIdx.x)];
    __syncthreads();
    const int local = (int)blockIdx.x - it.wg_begin, ntile = it.ntm * it.ntn;
    const int tile = local % ntile, chunk = local / ntile;
    if (chunk >= it.nchunks) return;                       // (uniform; the plan leaves no such workgroup)
    const int tm = tile % it.ntm, tn = tile / it.ntm;
    const long long m0 = 64LL * tm, n0 = 64LL * tn;
    const int mrows = (int)(it.M - m0 < 64 ? it.M - m0 : 64), ncols = (int)(it.N - n0 < 64 ? it.N - n0 : 64);
    const int nta = (mrows + 15) >> 4, ntb = (ncols + 15) >> 4, ntiles = nta * ntb;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, g = lane >> 4;
    const int nl = tid % TN, r0 = tid / TN;
    const cx<T>* __restrict__ A = reinterpret_cast<const cx<T>*>(it.A);
    const cx<T>* __restrict__ B = reinterpret_cast<const cx<T>*>(it.B);
    long long offA[NR], offB[NR];                          // this thread's rows of the two operand tiles (-1: beyond the item)
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const int a = r0 + RS * i;
        offA[i] = a < mrows ? bmps_split1(m0 + a, it.nm, it.md, it.ma) : -1;
        offB[i] = a < ncols ? bmps_split1(n0 + a, it.nn, it.nd, it.nb) : -1;
    }
    typename Mf::Acc cr[4], ci[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) { cr[u][r] = 0; ci[u][r] = 0; }
    const long long nblk = (it.K + TN - 1) / TN;
    const long long b0 = (long long)chunk * it.blocks_per_chunk;
    long long b1 = b0 + it.blocks_per_chunk; if (b1 > nblk) b1 = nblk;
    const bool conj = it.conjB != 0;
    for (long long blk = b0; blk < b1; ++blk) {
        const long long k = blk * TN + nl;
        const bool live = k < it.K;
        long long oka = 0, okb = 0;
        if (live) bmps_split2(k, it.nk, it.kd, it.ka, it.kb, oka, okb);
        __syncthreads();                                   // the previous block's operands have been consumed
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int a = r0 + RS * i;
            if (a < 16 * nta) {
                cx<T> v = cmake<T>((T)0, (T)0);
                if (live && offA[i] >= 0) v = A[offA[i] + oka];
                xr[a * LD + nl] = v.re; xi[a * LD + nl] = v.im;
            }
            if (a < 16 * ntb) {
                cx<T> v = cmake<T>((T)0, (T)0);
                if (live && offB[i] >= 0) v = B[offB[i] + okb];
                yr[a * LD + nl] = v.re; yi[a * LD + nl] = conj ? -v.im : v.im;
            }
        }
        __syncthreads();
        cplane_mm16<false>(xr, xi, yr, yi, nta, ntiles, cr, ci);      // (B was conjugated on the way in)
    }
    const bool direct = it.partial == nullptr;
    cx<T>* out = direct ? reinterpret_cast<cx<T>*>(it.C) : reinterpret_cast<cx<T>*>(it.partial) + (size_t)chunk * it.M * it.N;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int t = w + 4 * u;
        if (t < ntiles) {
            const int ta = t % nta, tb = t / nta, b = 16 * tb + c;
            if (b < ncols) {
                const long long oc_n = direct ? bmps_split1(n0 + b, it.nn, it.nd, it.nc) : it.M * (n0 + b);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int a = 16 * ta + Mf::row(g, r);
                    if (a < mrows) {
                        const long long oc_m = direct ? bmps_split1(m0 + a, it.nm, it.md, it.mc) : m0 + a;
                        out[oc_m + oc_n] = cmake<T>(cr[u][r], ci[u][r]);
                    }
                }
            }
        }
    }
}

template <class T>
__global__ __launch_bounds__(256) void bmps_reduce_kernel(const BmpsContractItem* __restrict__ items, int nitems) {
    __shared__ BmpsContractItem it;
    if (threadIdx.x == 0) it = items[find_item(items, nitems, &BmpsContractItem::red_begin, (int)blockIdx.x)];
    __syncthreads();
    if (!it.partial) return;
    const long long mn = it.M * it.N, e = ((long long)blockIdx.x - it.red_begin) * 256 + threadIdx.x;
    if (e >= mn) return;
    const cx<T>* __restrict__ p = reinterpret_cast<const cx<T>*>(it.partial);
    double ar[4] = {0, 0, 0, 0}, ai[4] = {0, 0, 0, 0};      // four independent sums, fixed order
    for (int ch = 0; ch < it.nchunks; ++ch) { const cx<T> v = p[(size_t)ch * mn + e]; ar[ch & 3] += (double)v.re; ai[ch & 3] += (double)v.im; }
    const double re = (ar[0] + ar[1]) + (ar[2] + ar[3]), im = (ai[0] + ai[1]) + (ai[2] + ai[3]);
    const long long off = bmps_split1(e % it.M, it.nm, it.md, it.mc) + bmps_split1(e / it.M, it.nn, it.nd, it.nc);
    if (it.out_f64) reinterpret_cast<cx<double>*>(it.C)[off] = cmake<double>(re, im);
    else reinterpret_cast<cx<T>*>(it.C)[off] = cmake<T>((T)re, (T)im);
}

void plan_bmps_contract(BmpsContractItem* it, int n, size_t esz, int force_chunks, size_t* npartial, int wgs[2]) {
    const int TN = esz == 8 ? 32 : 16;
    long long total = 0, rtotal = 0;
    for (int i = 0; i < n; ++i) {
        BmpsContractItem& f = it[i];
        if (f.nm < 0 || f.nn < 0 || f.nk < 0 || f.nm > kBmpsMaxLegs || f.nn > kBmpsMaxLegs || f.nk > kBmpsMaxLegs) throw_unsupported("bmps contraction: more than four legs in a group");
        f.M = f.N = f.K = 1;
        for (int q = 0; q < f.nm; ++q) f.M *= f.md[q];
        for (int q = 0; q < f.nn; ++q) f.N *= f.nd[q];
        for (int q = 0; q < f.nk; ++q) f.K *= f.kd[q];
        if (f.M < 1 || f.N < 1 || f.K < 1) throw_unsupported("bmps contraction: an empty leg");
        const long long ntm = (f.M + 63) / 64, ntn = (f.N + 63) / 64, tiles = ntm * ntn, nblk = (f.K + TN - 1) / TN;
        long long nch = 1;
        if (force_chunks > 0) nch = std::min<long long>(force_chunks, nblk);
        else if (tiles < 128) nch = std::max<long long>(1, std::min<long long>(std::min<long long>(256 / tiles, 64), nblk / 4));
        const long long bpc = (nblk + nch - 1) / nch;
        nch = (nblk + bpc - 1) / bpc;
        if (tiles * nch > (1LL << 30) || total + tiles * nch > (1LL << 30)) throw_unsupported("bmps contraction: more than 2^30 workgroups in a launch");
        f.ntm = (int)ntm; f.ntn = (int)ntn; f.nchunks = (int)nch; f.blocks_per_chunk = (int)bpc;
        const bool part = nch > 1 || f.out_f64;
        if (npartial) npartial[i] = part ? (size_t)nch * f.M * f.N : 0;
        f.wg_begin = (int)total; total += tiles * nch;
        f.red_begin = (int)rtotal; if (part) rtotal += (f.M * f.N + 255) / 256;
        if (rtotal > (1LL << 30)) throw_unsupported("bmps contraction: more than 2^30 workgroups in a launch");
    }
    wgs[0] = (int)total; wgs[1] = (int)rtotal;
}
template <class T> void launch_bmps_contract(hipStream_t s, const BmpsContractItem* d_items, int nitems, int wgs) {
    if (nitems <= 0 || wgs <= 0) return;
    hipLaunchKernelGGL((bmps_contract_kernel<T>), dim3(wgs), dim3(256), 0, s, d_items, nitems); TNQS_CHECK_LAUNCH();
}
template <class T> void launch_bmps_reduce(hipStream_t s, const BmpsContractItem* d_items, int nitems, int wgs) {
    if (nitems <= 0 || wgs <= 0) return;
    hipLaunchKernelGGL((bmps_reduce_kernel<T>), dim3(wgs), dim3(256), 0, s, d_items, nitems); TNQS_CHECK_LAUNCH();
}
template void launch_bmps_contract<float>(hipStream_t, const BmpsContractItem*, int, int);
template void launch_bmps_contract<double>(hipStream_t, const BmpsContractItem*, int, int);
template void launch_bmps_reduce<float>(hipStream_t, const BmpsContractItem*, int, int);
template void launch_bmps_reduce<double>(hipStream_t, const BmpsContractItem*, int, int);

// ------------------------------------------------------------------------------------------------------------
// thin Householder QR, one workgroup of 16 waves per matrix.  W (m x n, column-major) is factorised in place: R on and above the diagonal, the reflector vectors
// (v_j[j] = 1 implied) below it, as LAPACK's geqrf leaves them; H_j = I - tau_j v_j v_j^dagger, H_j^dagger (alpha; x) = (beta; 0) with beta real (zlarfg).  The columns
// behind j are dealt to the waves: a wave forms v^dagger a in f64 and updates its column, so a step costs two workgroup barriers.  Q = H_0 .. H_{n-1} (I; 0) is formed
// in W2 from the last reflector to the first.
// RANGE: the column norm and 1 / (alpha - beta) are formed from plain squares in f64, without LAPACK zlarfg's rescaling: a column whose entries lie below about 1e-154 (squares underflow,
// a non-zero column then reads as zero and gets the identity reflector, or the division meets a zero) or above about 1e154 (squares overflow) is outside what the kernel takes.  The
// fitting driver normalises every tensor it inserts and the gauge walk only meets those and the O(1) guess, so its columns are many orders inside; ComplexF32 data cannot leave the range.
// ------------------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(1024) void bmps_qr_kernel(const BmpsQrItem* __restrict__ items) {
    __shared__ double sh[17];
    __shared__ double tau_re[kBmpsQrMaxCols], tau_im[kBmpsQrMaxCols], hs[4];
    const BmpsQrItem it = items[blockIdx.x];
    const int m = it.m, n = it.n, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const cx<T>* __restrict__ A = reinterpret_cast<const cx<T>*>(it.A);
    cx<T>* W = reinterpret_cast<cx<T>*>(it.W);
    cx<T>* Q = reinterpret_cast<cx<T>*>(it.W2);
    cx<T>* Y = reinterpret_cast<cx<T>*>(it.Y);
    const long long mn = (long long)m * n;
    for (long long e = tid; e < mn; e += 1024) { const long long r = e % m, cc = e / m; W[e] = A[r * it.ars + cc * it.acs]; }
    __syncthreads();
    for (int j = 0; j < n; ++j) {
        cx<T>* col = W + (size_t)m * j;
        double s = 0;
        for (int r = j + 1 + tid; r < m; r += 1024) { const double a = col[r].re, b = col[r].im; s += a * a + b * b; }
        s = block_sum(s, sh);
        if (tid == 0) {
            const double are = col[j].re, aim = col[j].im;
            double tr = 0, ti = 0, sr = 0, si = 0, beta = are;
            if (s != 0 || aim != 0) {
                const double nx = sqrt(are * are + aim * aim + s);
                beta = are >= 0 ? -nx : nx;
                tr = (beta - are) / beta; ti = -aim / beta;
                const double dr = are - beta, di = aim, dd = dr * dr + di * di;      // 1 / (alpha - beta)
                sr = dr / dd; si = -di / dd;
                col[j] = cmake<T>((T)beta, (T)0);
            }
            tau_re[j] = tr; tau_im[j] = ti; hs[0] = sr; hs[1] = si;
        }
        __syncthreads();
        const double tr = tau_re[j], ti = tau_im[j];
        if (tr != 0 || ti != 0) {                            // (uniform)
            const double sr = hs[0], si = hs[1];
            for (int r = j + 1 + tid; r < m; r += 1024) { const double a = col[r].re, b = col[r].im; col[r] = cmake<T>((T)(a * sr - b * si), (T)(a * si + b * sr)); }
        }
        __syncthreads();
        if (tr != 0 || ti != 0) {
            for (int cc = j + 1 + wv; cc < n; cc += 16) {        // a_c <- (I - conj(tau) v v^dagger) a_c
                cx<T>* ac = W + (size_t)m * cc;
                double wr = 0, wi = 0;
                for (int r = j + 1 + lane; r < m; r += 64) { const double vr = col[r].re, vi = col[r].im, xr = ac[r].re, xi = ac[r].im; wr += vr * xr + vi * xi; wi += vr * xi - vi * xr; }
                wr = wave_sum(wr); wi = wave_sum(wi);
                wr += (double)ac[j].re; wi += (double)ac[j].im;
                const double fr = tr * wr + ti * wi, fi = tr * wi - ti * wr;      // conj(tau) w
                for (int r = j + 1 + lane; r < m; r += 64) { const double vr = col[r].re, vi = col[r].im; ac[r] = cmake<T>((T)((double)ac[r].re - (vr * fr - vi * fi)), (T)((double)ac[r].im - (vr * fi + vi * fr))); }
                if (lane == 0) ac[j] = cmake<T>((T)((double)ac[j].re - fr), (T)((double)ac[j].im - fi));
            }
        }
        __syncthreads();
    }
    for (int e = tid; e < n * n; e += 1024) { const int r = e % n, cc = e / n; Y[e] = r <= cc ? W[r + (size_t)m * cc] : cmake<T>((T)0, (T)0); }
    for (long long e = tid; e < mn; e += 1024) { const long long r = e % m, cc = e / m; Q[e] = cmake<T>(r == cc ? (T)1 : (T)0, (T)0); }
    __syncthreads();
    for (int j = n - 1; j >= 0; --j) {
        const double tr = tau_re[j], ti = tau_im[j];
        if (tr != 0 || ti != 0) {
            const cx<T>* col = W + (size_t)m * j;
            for (int cc = j + wv; cc < n; cc += 16) {            // q_c <- (I - tau v v^dagger) q_c on rows j ..
                cx<T>* qc = Q + (size_t)m * cc;
                double wr = 0, wi = 0;
                for (int r = j + 1 + lane; r < m; r += 64) { const double vr = col[r].re, vi = col[r].im, xr = qc[r].re, xi = qc[r].im; wr += vr * xr + vi * xi; wi += vr * xi - vi * xr; }
                wr = wave_sum(wr); wi = wave_sum(wi);
                wr += (double)qc[j].re; wi += (double)qc[j].im;
                const double fr = tr * wr - ti * wi, fi = tr * wi + ti * wr;      // tau w
                for (int r = j + 1 + lane; r < m; r += 64) { const double vr = col[r].re, vi = col[r].im; qc[r] = cmake<T>((T)((double)qc[r].re - (vr * fr - vi * fi)), (T)((double)qc[r].im - (vr * fi + vi * fr))); }
                if (lane == 0) qc[j] = cmake<T>((T)((double)qc[j].re - fr), (T)((double)qc[j].im - fi));
            }
        }
        __syncthreads();
    }
    cx<T>* out = reinterpret_cast<cx<T>*>(it.Q);
    for (long long e = tid; e < mn; e += 1024) { const long long r = e % m, cc = e / m; out[r * it.qrs + cc * it.qcs] = Q[e]; }
}
template <class T> void launch_bmps_qr(hipStream_t s, const BmpsQrItem* d_items, int nitems) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL((bmps_qr_kernel<T>), dim3(nitems), dim3(1024), 0, s, d_items); TNQS_CHECK_LAUNCH();
}
template void launch_bmps_qr<float>(hipStream_t, const BmpsQrItem*, int);
template void launch_bmps_qr<double>(hipStream_t, const BmpsQrItem*, int);

template <class T>
__global__ __launch_bounds__(1024) void bmps_norm_kernel(const BmpsNormItem* __restrict__ items) {
    __shared__ double sh[17];
    const BmpsNormItem it = items[blockIdx.x];
    const cx<T>* __restrict__ src = reinterpret_cast<const cx<T>*>(it.src);
    cx<T>* dst = reinterpret_cast<cx<T>*>(it.dst);
    double s = 0;
    for (long long e = threadIdx.x; e < it.n; e += 1024) { const double a = src[e].re, b = src[e].im; s += a * a + b * b; }
    s = block_sum(s, sh);
    const double nrm = sqrt(s), f = (it.normalize && nrm != 0) ? 1.0 / nrm : 1.0;
    if (threadIdx.x == 0 && it.norm_out) *it.norm_out = nrm;
    if (dst) for (long long e = threadIdx.x; e < it.n; e += 1024) { const cx<T> v = src[e]; dst[e] = cmake<T>((T)((double)v.re * f), (T)((it.conj ? -(double)v.im : (double)v.im) * f)); }
}
template <class T> void launch_bmps_norm(hipStream_t s, const BmpsNormItem* d_items, int nitems) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL((bmps_norm_kernel<T>), dim3(nitems), dim3(1024), 0, s, d_items); TNQS_CHECK_LAUNCH();
}
template void launch_bmps_norm<float>(hipStream_t, const BmpsNormItem*, int);
template void launch_bmps_norm<double>(hipStream_t, const BmpsNormItem*, int);

}  // namespace tnqs
