// kernels_rdm.hip -- two-site reduced density matrices of bonds (tnqs_rdm_edges; the reference's reduced_density_matrix(cache, [u, v]; alg = "bp")
// for adjacent u, v, where the Steiner tree is the bond itself).
//   edge_rdm_kernel<P>   rho_uv[s_u, s_v ; s_u', s_v'] = fac_u^2 fac_v^2 sum_{a, a'} E_u[(s_u, a), (s_u', a')] E_v[(s_v, a), (s_v', a')]
// from the Gram partials of both ends of the bond as run_grams leaves them (P = float or double): E_x = sum over the end's chunks of
// partial_x[chunk][i + KK j], i = s + d a, j = s' + d a'.  The kernel sums the chunks itself (f64), so no reduce launch runs in between.
#include "kernels.hpp"
#include "device_common.hpp"
#include "launch_util.hpp"

namespace tnqs {

// One workgroup (256 threads = 4 waves) per bond.  The bra bond index a' is walked in blocks of nb = edge_rdm_block(): for a block, both ends' columns
// j = (s', a') of E -- contiguous in the partials, so every lane of a load instruction reads the element next to its neighbour's -- are summed over the
// chunks into LDS as complex128; then, for every output entry in turn, the lanes stride over the block's (a, a'), a wave sums its lanes and adds the
// result to ITS slot of the entry (acc[wave][entry], LDS).  The four slots of an entry are added in a fixed order at the end and stored with plain vector
// stores: a bond's result does not depend on what else is in the launch.
template <class P> __global__ __launch_bounds__(256) void edge_rdm_kernel(const EdgeRdmItem* __restrict__ items) {
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
    auto sum_chunks = [&](const void* partial, int nchunks, int KK, int first, int count, cx<double>* dst) {
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
        sum_chunks(it.partial_u, it.nchunks_u, KKu, KKu * du * a0, KKu * du * nbk, Eu);
        sum_chunks(it.partial_v, it.nchunks_v, KKv, KKv * dv * a0, KKv * dv * nbk, Ev);
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

template <class P> void launch_edge_rdm(hipStream_t s, const EdgeRdmItem* d_items, int nitems) {
    if (nitems <= 0) return;
    set_max_dynamic_lds((const void*)edge_rdm_kernel<P>, kEdgeRdmLds);
    hipLaunchKernelGGL((edge_rdm_kernel<P>), dim3(nitems), dim3(256), kEdgeRdmLds, s, d_items); TNQS_CHECK_LAUNCH();
}
template void launch_edge_rdm<float>(hipStream_t, const EdgeRdmItem*, int);
template void launch_edge_rdm<double>(hipStream_t, const EdgeRdmItem*, int);

}  // namespace tnqs
