// kernels_amp.hip -- amplitudes <x|psi> of a batch of bitstrings by belief propagation on the single-layer network A_v = T_v[x_v, ...] (the reference's
// contract(tn; alg = "bp") over TensorNetwork, src/contract.jl:7-9, with vector messages that start as all ones, src/TensorNetworks/tensornetwork.jl:62-64; what
// certify_sample contracts, src/sampling.jl:258-285).  Every string reads the same site tensors; a message of string n is a vector, kept as column n of a [chi][string]
// matrix in the state's type.
//   amp_leg_gemm_kernel<T>   the first absorption of a message into T_u[x_u] for the strings of one group (x_u = g):
//                                R[a, b', p] = sum_k T_u[g + d (a + PA (k + K b'))] M[k, p],   p = idx[n] the position of the group's n-th string in the chunk.
//                            The slice is read IN PLACE with stride d, the contracted leg anywhere among the bond legs (PA = 1: first, PB = 1: last); 1 <= K <= 64.
//                            Matrix cores: v_mfma_f32_16x16x4_f32 (ComplexF32, f32 accumulation) / v_mfma_f64_16x16x4_f64 (ComplexF64), four real products per complex
//                            one (CMfma16, cmac16 of device_common.hpp).  A workgroup (4 waves) owns 64 rows (a, b') x 64 columns; a wave loads its 16 rows x K of the slice ONCE into registers (lane (c, q):
//                            row c, k = 4 ks + q) and walks the four 16-column tiles with them.  Rows, columns and k beyond the edge are zero operands (masked loads,
//                            nothing padded in memory) and are not stored.
//                            OUTPUT LAYOUT [row a + PA b'][string p]: string p's intermediate is the contiguous tensor of the site's remaining legs, so the next
//                            step streams it with a fastest -- whatever group the string was in.
//   amp_absorb_kernel<T>     a remaining leg, each string with its own vector: out[a, b', p] = sum_k in[a, k, b', p] m_p[k], one thread per output element, k ascending
//                            (f32 / f64 fused multiply-adds).  The last step of a chain leaves the raw message [chi_out][p].
//   amp_finalize_kernel<T>   per message and string (one wave each): raw element sum in f64 (kept for the vertex scalar), m / sum(m) when the sum is not exactly zero
//                            (abstractbeliefpropagationcache.jl:182-187), message_diff (beliefpropagationcache.jl:17-21) against the previous message or all ones.  A
//                            string whose done flag is set has converged: nothing of it is stored, its previous message is carried over bit for bit.
//   amp_sweep_end_kernel     per string: message_diff averaged over the sequence, the sweep count, the done flag.
//   amp_scalar_kernel<T>     per string: every vertex scalar sum_j raw_{v -> w}[j] m_{w -> v}[j] and edge scalar sum_j m_{u -> v}[j] m_{v -> u}[j] in f64, the sum of
//                            their complex logs, the flags.
#include "kernels.hpp"
#include "device_common.hpp"
#include "launch_util.hpp"

namespace tnqs {

template <class T>
__global__ __launch_bounds__(256) void amp_leg_gemm_kernel(const AmpGemmItem* __restrict__ items, int nitems) {
    using M = CMfma16<T>;
    const AmpGemmItem it = items[find_item(items, nitems, &AmpGemmItem::tile_begin, (int)blockIdx.x)];
    const int t = (int)blockIdx.x - it.tile_begin, tr = t % it.ntr, tc = t / it.ntr;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, q = lane >> 4;
    const int K = it.K, PA = it.PA;
    const long long NR = (long long)PA * it.PB;
    const long long row0 = 64LL * tr + 16 * w;
    if (row0 >= NR) return;                                    // (uniform in the wave; the kernel has no barrier)
    const long long row = row0 + c;
    const bool rlive = row < NR;
    const long long a = rlive ? row % PA : 0, b = rlive ? row / PA : 0;
    const cx<T>* __restrict__ tp = reinterpret_cast<const cx<T>*>(it.T) + (size_t)it.d * ((size_t)a + (size_t)PA * K * (size_t)b);
    const size_t ks_stride = (size_t)it.d * PA;
    T ar[16], ai[16];
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
        ar[ks] = 0; ai[ks] = 0;
        const int k = 4 * ks + q;
        if (rlive && k < K) { const cx<T> v = tp[ks_stride * k]; ar[ks] = v.re; ai[ks] = v.im; }
    }
    const cx<T>* __restrict__ Mm = reinterpret_cast<const cx<T>*>(it.M);
    cx<T>* __restrict__ R = reinterpret_cast<cx<T>*>(it.R);
    for (int ct = 0; ct < 4; ++ct) {
        const int col0 = 64 * tc + 16 * ct;
        if (col0 >= it.ncols) break;                           // (uniform)
        const int col = col0 + c;
        const bool clive = col < it.ncols;
        const int p = clive ? it.idx[col] : 0;
        typename M::Acc cr, ci;
#pragma unroll
        for (int r = 0; r < 4; ++r) { cr[r] = 0; ci[r] = 0; }
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            if (4 * ks < K) {                                  // (uniform)
                const int k = 4 * ks + q;
                T br = 0, bi = 0;
                if (clive && k < K) { if (Mm) { const cx<T> v = Mm[(size_t)K * p + k]; br = v.re; bi = v.im; } else br = 1; }
                cmac16<false>(ar[ks], ai[ks], br, bi, cr, ci);      // A[i = row][k] B[k][j = column]
            }
        }
        if (clive) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long orow = row0 + M::row(q, r);
                if (orow < NR) R[(size_t)orow + (size_t)NR * p] = cmake<T>(cr[r], ci[r]);
            }
        }
    }
}

int plan_amp_gemm(AmpGemmItem* it, int n) {
    return lay_out(it, n, &AmpGemmItem::tile_begin, nullptr, [&](AmpGemmItem& f) {
        f.ntr = (int)(((long long)f.PA * f.PB + 63) / 64); f.ntc = (f.ncols + 63) / 64;
        return f.ntr * f.ntc;
    });
}
template <class T> void launch_amp_leg_gemm(hipStream_t s, const AmpGemmItem* d_items, int nitems, int total_tiles) {
    if (nitems <= 0 || total_tiles <= 0) return;
    hipLaunchKernelGGL((amp_leg_gemm_kernel<T>), dim3(total_tiles), dim3(256), 0, s, d_items, nitems); TNQS_CHECK_LAUNCH();
}
template void launch_amp_leg_gemm<float>(hipStream_t, const AmpGemmItem*, int, int);
template void launch_amp_leg_gemm<double>(hipStream_t, const AmpGemmItem*, int, int);

// ------------------------------------------------------------------------------------------------------------
// a remaining leg: 256 output elements per workgroup
// ------------------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void amp_absorb_kernel(const AmpAbsorbItem* __restrict__ items, int nitems) {
    const AmpAbsorbItem it = items[find_item(items, nitems, &AmpAbsorbItem::wg_begin, (int)blockIdx.x)];
    const long long o = 256LL * ((int)blockIdx.x - it.wg_begin) + threadIdx.x;
    const long long total = (long long)it.PA * it.PB * it.nstr;
    if (o >= total) return;
    const int PA = it.PA, K = it.K;
    const long long a = o % PA, rest = o / PA, p = rest / it.PB;      // rest = b' + PB p
    const cx<T>* __restrict__ in = reinterpret_cast<const cx<T>*>(it.in) + (size_t)a + (size_t)PA * K * (size_t)rest;
    const cx<T>* __restrict__ m = it.m ? reinterpret_cast<const cx<T>*>(it.m) + (size_t)K * p : nullptr;
    cx<T> acc = cmake<T>((T)0, (T)0);
    if (m) { for (int k = 0; k < K; ++k) cfma(acc, in[(size_t)PA * k], m[k]); }
    else { for (int k = 0; k < K; ++k) { const cx<T> v = in[(size_t)PA * k]; acc.re += v.re; acc.im += v.im; } }
    reinterpret_cast<cx<T>*>(it.out)[o] = acc;
}
int plan_amp_absorb(AmpAbsorbItem* it, int n) {
    return lay_out(it, n, &AmpAbsorbItem::wg_begin, nullptr, [&](AmpAbsorbItem& f) { return (int)(((long long)f.PA * f.PB * f.nstr + 255) / 256); });
}
template <class T> void launch_amp_absorb(hipStream_t s, const AmpAbsorbItem* d_items, int nitems, int total_wgs) {
    if (nitems <= 0 || total_wgs <= 0) return;
    hipLaunchKernelGGL((amp_absorb_kernel<T>), dim3(total_wgs), dim3(256), 0, s, d_items, nitems); TNQS_CHECK_LAUNCH();
}
template void launch_amp_absorb<float>(hipStream_t, const AmpAbsorbItem*, int, int);
template void launch_amp_absorb<double>(hipStream_t, const AmpAbsorbItem*, int, int);

// ------------------------------------------------------------------------------------------------------------
// epilogue: one wave per (message, string), four strings per workgroup; lane k holds element k (chi <= 64)
// ------------------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void amp_finalize_kernel(const AmpFinalItem* __restrict__ items, int nitems) {
    const AmpFinalItem it = items[find_item(items, nitems, &AmpFinalItem::wg_begin, (int)blockIdx.x)];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int p = 4 * ((int)blockIdx.x - it.wg_begin) + w;
    if (p >= it.nstr) return;                                  // (uniform in the wave; no barrier)
    const int chi = it.chi;
    const bool live = lane < chi;
    const cx<T>* __restrict__ old = it.old_msg ? reinterpret_cast<const cx<T>*>(it.old_msg) + (size_t)chi * p : nullptr;
    cx<T>* out = reinterpret_cast<cx<T>*>(it.new_msg) + (size_t)chi * p;
    if (it.done && it.done[p]) {                               // a finished string: its message stays what it is
        if (live && old && old != out) out[lane] = old[lane];
        return;
    }
    double vr = 0, vi = 0;
    if (live) { const cx<T> v = reinterpret_cast<const cx<T>*>(it.raw)[(size_t)chi * p + lane]; vr = (double)v.re; vi = (double)v.im; }
    const double sre = wave_sum(vr), sim = wave_sum(vi);
    double ire = 1, iim = 0;
    if (it.normalize && (sre != 0 || sim != 0)) { const double d = sre * sre + sim * sim; ire = sre / d; iim = -sim / d; }
    double d0 = 0, d1 = 0, d2 = 0, d3 = 0;                     // Re, Im of dot(new, old), |new|^2, |old|^2
    if (live) {
        const cx<T> wv = cmake<T>((T)(vr * ire - vi * iim), (T)(vr * iim + vi * ire));
        double ore = 1, oim = 0;
        if (old) { ore = old[lane].re; oim = old[lane].im; }
        out[lane] = wv;
        d0 = (double)wv.re * ore + (double)wv.im * oim;
        d1 = (double)wv.re * oim - (double)wv.im * ore;
        d2 = (double)wv.re * wv.re + (double)wv.im * wv.im;
        d3 = ore * ore + oim * oim;
    }
    d0 = wave_sum(d0); d1 = wave_sum(d1); d2 = wave_sum(d2); d3 = wave_sum(d3);
    if (lane == 0) {
        if (it.diff_out) it.diff_out[p] = 1.0 - (d0 * d0 + d1 * d1) / (d2 * d3);
        if (it.sum_out) { it.sum_out[2 * (size_t)p] = sre; it.sum_out[2 * (size_t)p + 1] = sim; }
    }
}
int plan_amp_finalize(AmpFinalItem* it, int n) {
    return lay_out(it, n, &AmpFinalItem::wg_begin, nullptr, [&](AmpFinalItem& f) { return (f.nstr + 3) / 4; });
}
template <class T> void launch_amp_finalize(hipStream_t s, const AmpFinalItem* d_items, int nitems, int total_wgs) {
    if (nitems <= 0 || total_wgs <= 0) return;
    hipLaunchKernelGGL((amp_finalize_kernel<T>), dim3(total_wgs), dim3(256), 0, s, d_items, nitems); TNQS_CHECK_LAUNCH();
}
template void launch_amp_finalize<float>(hipStream_t, const AmpFinalItem*, int, int);
template void launch_amp_finalize<double>(hipStream_t, const AmpFinalItem*, int, int);

__global__ __launch_bounds__(256) void amp_sweep_end_kernel(const double* __restrict__ diffs, int nseq, int nstrings, int iter, double tol, int* done, int* niter, double* fdiff) {
    const int n = 256 * (int)blockIdx.x + threadIdx.x;
    if (n >= nstrings || done[n]) return;
    double s = 0;
    for (int t = 0; t < nseq; ++t) s += diffs[(size_t)t * nstrings + n];
    const double avg = s / (double)nseq;
    niter[n] = iter; fdiff[n] = avg;
    if (tol >= 0 && avg <= tol) done[n] = 1;
}
void launch_amp_sweep_end(hipStream_t s, const double* diffs, int nseq, int nstrings, int iter, double tol, int* done, int* niter, double* fdiff) {
    if (nstrings <= 0 || nseq <= 0) return;
    hipLaunchKernelGGL(amp_sweep_end_kernel, dim3((nstrings + 255) / 256), dim3(256), 0, s, diffs, nseq, nstrings, iter, tol, done, niter, fdiff); TNQS_CHECK_LAUNCH();
}

// ------------------------------------------------------------------------------------------------------------
// vertex and edge scalars and their log sum: one wave per string
// ------------------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void amp_scalar_kernel(const AmpScalarItem* __restrict__ items, int nv, int ne, const int* __restrict__ cfg, int ld, int nstrings,
                                                          double* out, int* flags) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int n = 4 * (int)blockIdx.x + w;
    if (n >= nstrings) return;                                 // (uniform in the wave; no barrier)
    const double pi = 3.14159265358979323846;
    double lre = 0, lim = 0; int flag = 0;
    for (int i = 0; i < nv + ne; ++i) {
        const AmpScalarItem it = items[i];
        double re = 0, im = 0;
        if (it.site) {                                         // a vertex without neighbours: the entry itself
            const cx<T> v = reinterpret_cast<const cx<T>*>(it.site)[cfg[(size_t)n * ld + it.vertex]];
            re = (double)v.re; im = (double)v.im;
        } else {
            if (lane < it.chi) {
                const size_t e = (size_t)it.chi * n + lane;
                double xr = 1, xi = 0, yr = 1, yi = 0;
                if (it.m) { const cx<T> v = reinterpret_cast<const cx<T>*>(it.m)[e]; xr = (double)v.re; xi = (double)v.im; }
                if (it.mr) { const cx<T> v = reinterpret_cast<const cx<T>*>(it.mr)[e]; yr = (double)v.re; yi = (double)v.im; }
                re = xr * yr - xi * yi; im = xr * yi + xi * yr;
            }
            re = wave_sum(re); im = wave_sum(im);
            if (it.rawsum) {                                   // m is raw / sum(raw) unless the epilogue left it as it was
                const double sr = it.rawsum[2 * (size_t)n], si = it.rawsum[2 * (size_t)n + 1];
                if (it.normalize && (sr != 0 || si != 0)) { const double tt = re * sr - im * si; im = re * si + im * sr; re = tt; }
            }
        }
        if (it.scale) { const double f = *it.scale; re *= f; im *= f; }
        if (!isfinite(re) || !isfinite(im)) { flag |= 2; continue; }
        if (re == 0 && im == 0) { flag |= 1; continue; }
        const double lr = log(hypot(re, im)), li = atan2(im, re);
        if (i < nv) { lre += lr; lim += li; } else { lre -= lr; lim -= li; }
    }
    if (lane == 0) {
        if (flag & 2) { lre = nan(""); lim = nan(""); }
        else if (flag & 1) { lre = -INFINITY; lim = 0; }
        else { lim = fmod(lim, 2 * pi); if (lim > pi) lim -= 2 * pi; else if (lim <= -pi) lim += 2 * pi; }
        out[2 * (size_t)n] = lre; out[2 * (size_t)n + 1] = lim; flags[n] = flag;
    }
}
template <class T> void launch_amp_scalar(hipStream_t s, const AmpScalarItem* d_items, int nv, int ne, const int* cfg, int ld, int nstrings, double* out, int* flags) {
    if (nstrings <= 0) return;
    hipLaunchKernelGGL((amp_scalar_kernel<T>), dim3((nstrings + 3) / 4), dim3(256), 0, s, d_items, nv, ne, cfg, ld, nstrings, out, flags); TNQS_CHECK_LAUNCH();
}
template void launch_amp_scalar<float>(hipStream_t, const AmpScalarItem*, int, int, const int*, int, int, double*, int*);
template void launch_amp_scalar<double>(hipStream_t, const AmpScalarItem*, int, int, const int*, int, int, double*, int*);

}  // namespace tnqs
