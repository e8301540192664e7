// kernels_rdm.hip -- two-site reduced density matrices of bonds (tnqs_rdm_edges; the reference's reduced_density_matrix(cache, [u, v]; alg = "bp")
// for adjacent u, v, where the Steiner tree is the bond itself).
//   edge_rdm_kernel<Pu, Pv>   rho_uv[s_u, s_v ; s_u', s_v'] = fac_u^2 fac_v^2 sum_{a, a'} E_u[(s_u, a), (s_u', a')] E_v[(s_v, a), (s_v', a')]
// from the Gram partials of both ends of the bond as run_grams leaves them (P_x = float or double, one type per end): E_x = sum over the end's chunks of
// partial_x[chunk][i + KK j], i = s + d a, j = s' + d a'.  The kernel sums the chunks itself (f64), so no reduce launch runs in between.
// and of the ends of paths (tnqs_rdm_paths: the Steiner tree is the path p_0 .. p_n):
//   path_apply_kernel<P, T>   L_k[s, s'; b, b'] = fac_k^2 sum_{a, a'} L_{k-1}[s, s'; a, a'] T_k[(b, b'), (a, a')]
// the environment of p_0 carried through the transfer matrix of the inner vertex p_k (engine_loops.cpp build_transfer_matrices), in the Gram-partial layout, so that
// rho(p_0, p_k) is edge_rdm_kernel<double, P> on (L_{k-1}, E_{p_k -> p_{k-1}}).
#include "kernels.hpp"
#include "device_common.hpp"
#include "launch_util.hpp"

namespace tnqs {

// One workgroup (256 threads = 4 waves) per bond.  The bra bond index a' is walked in blocks of nb = edge_rdm_block(): for a block, both ends' columns
// j = (s', a') of E -- contiguous in the partials, so every lane of a load instruction reads the element next to its neighbour's -- are summed over the
// chunks into LDS as complex128; then, for every output entry in turn, the lanes stride over the block's (a, a'), a wave sums its lanes and adds the
// result to ITS slot of the entry (acc[wave][entry], LDS).  The four slots of an entry are added in a fixed order at the end and stored with plain vector
// stores: a bond's result does not depend on what else is in the launch.
template <class Pu, class Pv> __global__ __launch_bounds__(256) void edge_rdm_kernel(const EdgeRdmItem* __restrict__ items) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const EdgeRdmItem it = items[blockIdx.x];
    const int du = it.du, dv = it.dv, chi = it.chi, dd = du * dv, nout = dd * dd;
    const int KKu = du * chi, KKv = dv * chi;
    const int nb = edge_rdm_block(du, dv, chi);
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    cx<double>* const acc = reinterpret_cast<cx<double>*>(smem);      // [wave][entry]
    cx<double>* const Eu = acc + 4 * nout;                            // [(s', a' - a0)][(s, a)], KKu rows
    cx<double>* const Ev = Eu + (size_t)du * du * chi * nb;
    for (int o = tid; o < 4 * nout; o += 256) acc[o] = cmake<double>(0, 0);
    auto sum_chunks = [&](auto tag, const void* partial, int nchunks, int KK, int first, int count, cx<double>* dst) {
        using P = decltype(tag);
        const cx<P>* __restrict__ p = reinterpret_cast<const cx<P>*>(partial) + first;
        const size_t n2 = (size_t)KK * KK;
        for (int e = tid; e < count; e += 256) {
            double re = 0, im = 0;
#pragma unroll 8                                                      // eight independent loads in flight per lane; the sums stay in chunk order
            for (int c = 0; c < nchunks; ++c) { const cx<P> v = p[(size_t)c * n2 + e]; re += (double)v.re; im += (double)v.im; }
            dst[e] = cmake<double>(re, im);
        }
    };
    for (int a0 = 0; a0 < chi; a0 += nb) {
        const int nbk = min(nb, chi - a0);
        __syncthreads();                                              // the previous block's products have read Eu, Ev (first block: acc is zero)
        sum_chunks(Pu(), it.partial_u, it.nchunks_u, KKu, KKu * du * a0, KKu * du * nbk, Eu);
        sum_chunks(Pv(), it.partial_v, it.nchunks_v, KKv, KKv * dv * a0, KKv * dv * nbk, Ev);
        __syncthreads();
        const int npair = chi * nbk;
        for (int o = 0; o < nout; ++o) {                              // entry (row, col) = (s_v + d_v s_u, s_v' + d_v s_u')
            const int row = o % dd, col = o / dd;
            const cx<double>* eu = Eu + row / dv + KKu * (col / dv);
            const cx<double>* ev = Ev + row % dv + KKv * (col % dv);
            double re = 0, im = 0;
            for (int p = tid; p < npair; p += 256) {
                const int a = p % chi, al = p / chi;
                const cx<double> x = eu[du * a + KKu * du * al], y = ev[dv * a + KKv * dv * al];
                re += x.re * y.re - x.im * y.im; im += x.re * y.im + x.im * y.re;
            }
            re = wave_sum(re); im = wave_sum(im);
            if (lane == 0) { cx<double> t = acc[w * nout + o]; t.re += re; t.im += im; acc[w * nout + o] = t; }
        }
    }
    __syncthreads();
    const double fu = it.scale_u ? *it.scale_u : 1.0, fv = it.scale_v ? *it.scale_v : 1.0, f = fu * fu * fv * fv;
    cx<double>* __restrict__ out = reinterpret_cast<cx<double>*>(it.out);
    for (int o = tid; o < nout; o += 256) {
        double re = 0, im = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) { re += acc[q * nout + o].re; im += acc[q * nout + o].im; }
        out[o] = cmake<double>(re * f, im * f);
    }
}

template <class Pu, class Pv> void launch_edge_rdm_mixed(hipStream_t s, const EdgeRdmItem* d_items, int nitems) {
    if (nitems <= 0) return;
    set_max_dynamic_lds((const void*)edge_rdm_kernel<Pu, Pv>, kEdgeRdmLds);
    hipLaunchKernelGGL((edge_rdm_kernel<Pu, Pv>), dim3(nitems), dim3(256), kEdgeRdmLds, s, d_items); TNQS_CHECK_LAUNCH();
}
template void launch_edge_rdm_mixed<float, float>(hipStream_t, const EdgeRdmItem*, int);
template void launch_edge_rdm_mixed<double, double>(hipStream_t, const EdgeRdmItem*, int);
template void launch_edge_rdm_mixed<float, double>(hipStream_t, const EdgeRdmItem*, int);
template void launch_edge_rdm_mixed<double, float>(hipStream_t, const EdgeRdmItem*, int);
template <class P> void launch_edge_rdm(hipStream_t s, const EdgeRdmItem* d_items, int nitems) { launch_edge_rdm_mixed<P, P>(s, d_items, nitems); }
template void launch_edge_rdm<float>(hipStream_t, const EdgeRdmItem*, int);
template void launch_edge_rdm<double>(hipStream_t, const EdgeRdmItem*, int);

// ---- path_apply_kernel --------------------------------------------------------------------------------------------------------------------------------
// A skinny product L_out (R x chi_b^2) = L_in (R x chi_a^2) T with R = d^2 <= 16 rows that reads all of T once: bandwidth-bound on T.  L is complex128 with f64
// accumulation whatever the state's type (connected correlators are differences of nearly equal numbers); only T keeps the state's precision and is widened exactly.
// Workgroup (row block rb, column range j) of an item: 256 lanes, lane = one row (b, b') with R complex accumulators in registers (R a template parameter of the row
// loop: 64 VGPRs at R = 16).  The column range is walked in passes of kPathApplyCols columns: the pass's columns of L_in are summed over the input's chunks in chunk order
// (f64) into LDS as [column][r], then every lane reads ITS element of T for eight columns at a time -- eight independent loads in flight, each a coalesced run over the
// lanes since (b, b') is T's contiguous axis -- and multiplies each by the R values of L of that column (one LDS address for the whole wave: a broadcast read).
// The lane's R results go to chunk j of L_out with plain vector stores: no atomics, no zero-fill, and a range without columns (ksplit > chi_a^2) writes zeros.
template <class P, class T, int RR> __device__ __forceinline__ void path_apply_rows(const PathApplyItem& it, int rb, int j, cx<double>* sh) {
    const int d = it.d, ca = it.chi_a, cb = it.chi_b, nrows = cb * cb, ncols = ca * ca, KA = d * ca, KB = d * cb;
    const int c_lo = (int)((long long)j * ncols / it.ksplit), c_hi = (int)((long long)(j + 1) * ncols / it.ksplit);
    const int tid = threadIdx.x, row = rb * 256 + tid;
    const bool live = row < nrows;
    const cx<P>* __restrict__ Lin = reinterpret_cast<const cx<P>*>(it.L_in);
    const cx<T>* __restrict__ Tm = reinterpret_cast<const cx<T>*>(it.T) + (live ? row : 0);
    const size_t n2 = (size_t)KA * KA;
    cx<double> acc[RR];
#pragma unroll
    for (int r = 0; r < RR; ++r) acc[r] = cmake<double>(0, 0);
    for (int c0 = c_lo; c0 < c_hi; c0 += kPathApplyCols) {
        const int cnt = min(kPathApplyCols, c_hi - c0);
        __syncthreads();                                              // the previous pass's products have read sh
        for (int e = tid; e < cnt * RR; e += 256) {
            const int r = e % RR, col = c0 + e / RR, s = r % d, sp = r / d, a = col % ca, ap = col / ca;
            const cx<P>* __restrict__ p = Lin + (size_t)(s + d * a) + (size_t)KA * (sp + d * ap);
            double re = 0, im = 0;
#pragma unroll 4
            for (int c = 0; c < it.nchunks_in; ++c) { const cx<P> v = p[(size_t)c * n2]; re += (double)v.re; im += (double)v.im; }
            sh[e] = cmake<double>(re, im);
        }
        __syncthreads();
        if (live)
            for (int c = 0; c < cnt; c += 8) {
                cx<T> t[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) t[q] = Tm[(size_t)nrows * (c0 + min(c + q, cnt - 1))];      // past the pass's end: the last column again, not used
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    if (c + q >= cnt) break;
                    const cx<double> td = cmake<double>((double)t[q].re, (double)t[q].im);
                    const cx<double>* l = sh + (c + q) * RR;
#pragma unroll
                    for (int r = 0; r < RR; ++r) cfma(acc[r], l[r], td);
                }
            }
    }
    if (!live) return;
    const double f = it.scale ? *it.scale : 1.0, f2 = f * f;
    const int b = row % cb, bp = row / cb;
    cx<double>* __restrict__ out = reinterpret_cast<cx<double>*>(it.L_out) + (size_t)j * KB * KB;
#pragma unroll
    for (int r = 0; r < RR; ++r) {
        const int s = r % d, sp = r / d;
        out[(size_t)(s + d * b) + (size_t)KB * (sp + d * bp)] = cmake<double>(acc[r].re * f2, acc[r].im * f2);
    }
}

template <class P, class T> __global__ __launch_bounds__(256) void path_apply_kernel(const PathApplyItem* __restrict__ items, int nitems) {
    __shared__ __attribute__((aligned(16))) cx<double> sh[kPathApplyCols * 16];
    const int gt = blockIdx.x;
    const int lo = find_item(items, nitems, &PathApplyItem::wg_begin, gt);
    const PathApplyItem it = items[lo];
    const int lw = gt - it.wg_begin;
    if (lw >= it.nrb * it.ksplit) return;
    const int rb = lw % it.nrb, j = lw / it.nrb;
    switch (it.d) {
    case 1: path_apply_rows<P, T, 1>(it, rb, j, sh); break;
    case 2: path_apply_rows<P, T, 4>(it, rb, j, sh); break;
    case 3: path_apply_rows<P, T, 9>(it, rb, j, sh); break;
    case 4: path_apply_rows<P, T, 16>(it, rb, j, sh); break;
    default: break;                                                   // refused on the host
    }
}

int plan_path_apply(PathApplyItem* it, int n) {
    long long blocks = 0;
    for (int i = 0; i < n; ++i) { it[i].nrb = (it[i].chi_b * it[i].chi_b + 255) / 256; blocks += it[i].nrb; }
    const int want = blocks ? (int)((kPathApplyTargetWgs + blocks - 1) / blocks) : 1;
    return lay_out(it, n, &PathApplyItem::wg_begin, nullptr, [&](PathApplyItem& p) {
        if (p.ksplit <= 0) p.ksplit = std::max(1, std::min({kPathApplyMaxSplit, p.chi_a * p.chi_a / kPathApplyCols, want}));
        return p.nrb * p.ksplit; });
}
template <class P, class T> void launch_path_apply(hipStream_t s, const PathApplyItem* d_items, int nitems, int total_wgs) {
    if (nitems <= 0 || total_wgs <= 0) return;
    hipLaunchKernelGGL((path_apply_kernel<P, T>), dim3(total_wgs), dim3(256), 0, s, d_items, nitems); TNQS_CHECK_LAUNCH();
}
template void launch_path_apply<float, float>(hipStream_t, const PathApplyItem*, int, int);
template void launch_path_apply<double, float>(hipStream_t, const PathApplyItem*, int, int);
template void launch_path_apply<float, double>(hipStream_t, const PathApplyItem*, int, int);
template void launch_path_apply<double, double>(hipStream_t, const PathApplyItem*, int, int);

}  // namespace tnqs
