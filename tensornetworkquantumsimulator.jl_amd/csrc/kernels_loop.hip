// kernels_loop.hip -- loop corrections (src/MessagePassing/loopcorrection.jl): the double-layer transfer matrices of a loop and their ring product.
//   loop_cgemm_kernel<T>        batched complex C = A op(B) on the matrix cores, arbitrary m, n, k per item, four-index output map
//   loop_antiproject_kernel<T>  T <- T - f (b^T T): the antiprojector of one bond applied to the rows of a transfer matrix
//   loop_trace_kernel<T>        sum_ij X[i,j] Y[j,i] in f64 (partials per workgroup) + loop_trace_tail_kernel (one complex128 per item)
//   loop_branch_gram_kernel<T>  batched complex C = A B^H, rows and columns each split into three sub-indices with 64-bit strides:
//                               the three-leg double-layer tensor of a branch vertex, interleaved [(a,a'),(b,b'),(c,c')], without a permuted copy
//   loop_tile_body              the ONE tile code of these two kernels (staging, predication, multiply loops, store walk); a kernel is its item lookup and its
//                               output index map, passed as two lambdas
//   loop_dot_kernel<T>          sum_i X[i] Y[i] in f64 over a 64-bit length (the full contraction of two tensors of one layout) + its tail kernel
// Matrices are column-major with no padding between columns.
#include "kernels.hpp"
#include "mfma_common.hpp"

namespace tnqs {

// ---- batched complex GEMM ----------------------------------------------------------------------------------------------------------------
// One workgroup (256 threads = 4 waves) owns a 64 x 64 tile of C; wave (wr, wc) owns its 32 x 32 quarter.  A k-chunk of KT columns of A and of
// op(B) is staged in LDS as interleaved complex numbers, [k][row] with a pitch of 66 elements: the lanes of a wave read consecutive elements
// of one k-slice (no bank conflict), and the operand of the matrix instruction is one LDS read.  Rows / columns / k beyond the matrix are
// ZERO in LDS (the global loads are predicated), and the store is predicated: nothing is read or written past the end of a matrix.
// The matrix instruction gets op(B) as its first operand and A as its second, so a lane holds one ROW i of C and its registers run over
// columns: the lanes of a store instruction write consecutive elements of the contiguous output axis.
// ComplexF32: v_mfma_f32_32x32x2_f32, four real products per complex one (CAcc32<false>); ComplexF64: v_mfma_f64_16x16x4_f64 (cmac16), 2 x 2 blocks per wave.
constexpr int kLoopTile = 64, kLoopPitch = 66;
template <class T> struct LoopKT { static constexpr int v = sizeof(T) == 4 ? 16 : 8; };

// two memory-adjacent elements p[0], p[1] (ok0 / ok1: inside the matrix); vec: p is 16-byte aligned (ComplexF32: one 16-byte word)
template <class T> __device__ __forceinline__ void loop_load2(const cx<T>* p, bool vec, bool ok0, bool ok1, cx<T>& v0, cx<T>& v1) {
    v0 = cmake<T>(0, 0); v1 = cmake<T>(0, 0);
    if constexpr (sizeof(T) == 4) {
        if (vec && ok0 && ok1) { const v4f t = ldg4(p); v0 = cmake<T>(t[0], t[1]); v1 = cmake<T>(t[2], t[3]); return; }
    }
    if (ok0) v0 = p[0];
    if (ok1) v1 = p[1];
}

// The tile code of loop_cgemm_kernel and loop_branch_gram_kernel: the tile lt of item `it` (m, n, k, A, B, C, ntm, ntn; opB unless ALWAYS_H), staged, multiplied and
// stored at C[row_off(i) + col_off(j)].  ALWAYS_H: op(B) = B^H whatever the item says (it need not say), the other staging is not compiled.
template <class T, bool ALWAYS_H, class Item, class RowOff, class ColOff>
__device__ __forceinline__ void loop_tile_body(const Item& it, int lt, RowOff row_off, ColOff col_off) {
    constexpr int KT = LoopKT<T>::v, P = kLoopPitch;
    __shared__ __attribute__((aligned(16))) cx<T> As[KT * P];
    __shared__ __attribute__((aligned(16))) cx<T> Bs[KT * P];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, wr = w & 1, wc = w >> 1;
    if (lt >= it.ntm * it.ntn) return;
    const int i0 = (lt % it.ntm) * kLoopTile, j0 = (lt / it.ntm) * kLoopTile;
    const int m = it.m, n = it.n, k = it.k;
    const cx<T>* __restrict__ A = reinterpret_cast<const cx<T>*>(it.A);
    const cx<T>* __restrict__ B = reinterpret_cast<const cx<T>*>(it.B);
    bool conjB = true;
    if constexpr (!ALWAYS_H) conjB = it.opB != 0;
    const bool avec = sizeof(T) == 4 && (m & 1) == 0 && (reinterpret_cast<uintptr_t>(A) & 15) == 0;
    const bool bvec = sizeof(T) == 4 && (((conjB ? n : k) & 1) == 0) && (reinterpret_cast<uintptr_t>(B) & 15) == 0;

    CAcc32<false> acc;                           // ComplexF32
    v4d cr[2][2], ci[2][2];                      // ComplexF64: [row block][column block]
    if constexpr (sizeof(T) == 4) acc.zero();
    else {
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) { cr[a][b] = (v4d)(0.0); ci[a][b] = (v4d)(0.0); }
    }

    for (int k0 = 0; k0 < k; k0 += KT) {
        // A: rows (i0 + 2 rp, + 1) of k-slice kk -- memory-adjacent
        {
            const int rp = tid & 31;
#pragma unroll
            for (int q = 0; q < KT / 8; ++q) {
                const int kk = (tid >> 5) + 8 * q, gk = k0 + kk, row = i0 + 2 * rp;
                cx<T> v0, v1;
                const bool kin = gk < k;
                loop_load2<T>(A + (size_t)row + (size_t)m * (kin ? gk : 0), avec, kin && row < m, kin && row + 1 < m, v0, v1);
                As[kk * P + 2 * rp] = v0; As[kk * P + 2 * rp + 1] = v1;
            }
        }
        if (conjB) {                             // op(B) = B^H, B is n x k: element (j, kk) at j + n kk, conjugated on the way in
            const int rp = tid & 31;
#pragma unroll
            for (int q = 0; q < KT / 8; ++q) {
                const int kk = (tid >> 5) + 8 * q, gk = k0 + kk, col = j0 + 2 * rp;
                cx<T> v0, v1;
                const bool kin = gk < k;
                loop_load2<T>(B + (size_t)col + (size_t)n * (kin ? gk : 0), bvec, kin && col < n, kin && col + 1 < n, v0, v1);
                v0.im = -v0.im; v1.im = -v1.im;
                Bs[kk * P + 2 * rp] = v0; Bs[kk * P + 2 * rp + 1] = v1;
            }
        } else if constexpr (!ALWAYS_H) {        // B is k x n: element (kk, j) at kk + k j -- k-slices (2 kp, + 1) are memory-adjacent
            constexpr int KH = KT / 2, JP = 256 / KH;
            const int kp = tid % KH;
#pragma unroll
            for (int q = 0; q < kLoopTile / JP; ++q) {
                const int jl = tid / KH + JP * q, col = j0 + jl, gk = k0 + 2 * kp;
                cx<T> v0, v1;
                const bool cin = col < n;
                loop_load2<T>(B + (size_t)gk + (size_t)k * (cin ? col : 0), bvec, cin && gk < k, cin && gk + 1 < k, v0, v1);
                Bs[(2 * kp) * P + jl] = v0; Bs[(2 * kp + 1) * P + jl] = v1;
            }
        }
        __syncthreads();
        if constexpr (sizeof(T) == 4) {
            const int ln = lane & 31, h = lane >> 5;
#pragma unroll
            for (int kk = 0; kk < KT; kk += 2) {
                const cx<T> a = As[(kk + h) * P + 32 * wr + ln], b = Bs[(kk + h) * P + 32 * wc + ln];
                acc.mac(b.re, b.im, a.re, a.im);          // D[column = register][row = lane]
            }
        } else {
            const int l15 = lane & 15, kq = lane >> 4;
#pragma unroll
            for (int k4 = 0; k4 < KT; k4 += 4) {
                cx<T> av[2], bv[2];
#pragma unroll
                for (int q = 0; q < 2; ++q) { av[q] = As[(k4 + kq) * P + 32 * wr + 16 * q + l15]; bv[q] = Bs[(k4 + kq) * P + 32 * wc + 16 * q + l15]; }
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b) cmac16<false>(bv[b].re, bv[b].im, av[a].re, av[a].im, cr[a][b], ci[a][b]);      // (operands swapped, as above)
            }
        }
        __syncthreads();
    }

    cx<T>* __restrict__ C = reinterpret_cast<cx<T>*>(it.C);
    if constexpr (sizeof(T) == 4) {
        const int ln = lane & 31, h = lane >> 5;
        const int i = i0 + 32 * wr + ln;
        if (i < m) {
            const long long ro = row_off(i);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = j0 + 32 * wc + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (j < n) C[ro + col_off(j)] = cmake<T>(acc.a[r], acc.b[r]);
            }
        }
    } else {
        const int l15 = lane & 15, kq = lane >> 4;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int i = i0 + 32 * wr + 16 * a + l15;
            if (i >= m) continue;
            const long long ro = row_off(i);
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = j0 + 32 * wc + 16 * b + kq + 4 * r;
                    if (j < n) C[ro + col_off(j)] = cmake<T>(cr[a][b][r], ci[a][b][r]);
                }
        }
    }
}
template <class Item> int plan_loop_tiles(Item* it, int n) {
    return lay_out(it, n, &Item::tile_begin, nullptr, [](Item& g) {
        g.ntm = (g.m + kLoopTile - 1) / kLoopTile; g.ntn = (g.n + kLoopTile - 1) / kLoopTile; return g.ntm * g.ntn; });
}
template <class Item> void launch_loop_tiles(void (*kernel)(const Item*, int), hipStream_t s, const Item* d_items, int nitems, int total_tiles) {
    if (nitems <= 0 || total_tiles <= 0) return;
    hipLaunchKernelGGL(kernel, dim3(total_tiles), dim3(256), 0, s, d_items, nitems); TNQS_CHECK_LAUNCH();
}

// the output map: row i = i0 + I0 i1 at i0 si0 + i1 si1, column j = j0 + J0 j1 at j0 sj0 + j1 sj1
template <class T> __global__ __launch_bounds__(256) void loop_cgemm_kernel(const LoopGemmItem* __restrict__ items, int nitems) {
    const LoopGemmItem it = items[find_item(items, nitems, &LoopGemmItem::tile_begin, (int)blockIdx.x)];
    loop_tile_body<T, false>(it, (int)blockIdx.x - it.tile_begin,
                             [&](int i) { return (long long)(i % it.I0) * it.si0 + (long long)(i / it.I0) * it.si1; },
                             [&](int j) { return (long long)(j % it.J0) * it.sj0 + (long long)(j / it.J0) * it.sj1; });
}
int plan_loop_cgemm(LoopGemmItem* it, int n) { return plan_loop_tiles(it, n); }
template <class T> void launch_loop_cgemm(hipStream_t s, const LoopGemmItem* d_items, int nitems, int total_tiles) {
    launch_loop_tiles(loop_cgemm_kernel<T>, s, d_items, nitems, total_tiles);
}
template void launch_loop_cgemm<float>(hipStream_t, const LoopGemmItem*, int, int);
template void launch_loop_cgemm<double>(hipStream_t, const LoopGemmItem*, int, int);

// ---- three-leg Gram of a branch vertex: C = A B^H, A m x k, B n x k, written through a SIX-index output map -----------------------------------
// Row i = i0 + R0 (i1 + R1 i2) goes to i0 sr[0] + i1 sr[1] + i2 sr[2], column j = j0 + C0 (j1 + C1 j2) to j0 sc[0] + j1 sc[1] + j2 sc[2]: with A = phi and
// B = psi of a vertex as [(a, b, c), rest] this writes B[(a,a'),(b,b'),(c,c')] (or any order of the three double legs) without a permuted copy of it.
// The tile code is loop_tile_body with op(B) = B^H; a kernel of its own, so that the integer divides of this map stay out of loop_cgemm_kernel's store.
template <class T> __global__ __launch_bounds__(256) void loop_branch_gram_kernel(const BranchGramItem* __restrict__ items, int nitems) {
    const BranchGramItem it = items[find_item(items, nitems, &BranchGramItem::tile_begin, (int)blockIdx.x)];
    loop_tile_body<T, true>(it, (int)blockIdx.x - it.tile_begin,
                            [&](int i) { return (long long)(i % it.R0) * it.sr[0] + (long long)((i / it.R0) % it.R1) * it.sr[1] + (long long)(i / it.R0 / it.R1) * it.sr[2]; },
                            [&](int j) { return (long long)(j % it.C0) * it.sc[0] + (long long)((j / it.C0) % it.C1) * it.sc[1] + (long long)(j / it.C0 / it.C1) * it.sc[2]; });
}
int plan_loop_branch_gram(BranchGramItem* it, int n) { return plan_loop_tiles(it, n); }
template <class T> void launch_loop_branch_gram(hipStream_t s, const BranchGramItem* d_items, int nitems, int total_tiles) {
    launch_loop_tiles(loop_branch_gram_kernel<T>, s, d_items, nitems, total_tiles);
}
template void launch_loop_branch_gram<float>(hipStream_t, const BranchGramItem*, int, int);
template void launch_loop_branch_gram<double>(hipStream_t, const BranchGramItem*, int, int);

// ---- antiprojector: T <- T - f (b^T T), bilinear (no conjugate).  One wave per column: w = sum_i b[i] T[i, c], then T[i, c] -= f[i] w ------
template <class T> __global__ __launch_bounds__(256) void loop_antiproject_kernel(const LoopProjItem* __restrict__ items, int nitems) {
    const int gt = blockIdx.x;
    const int lo = find_item(items, nitems, &LoopProjItem::wg_begin, gt);
    const LoopProjItem it = items[lo];
    const int c = 4 * (gt - it.wg_begin) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= it.nc) return;
    cx<T>* __restrict__ col = reinterpret_cast<cx<T>*>(it.T) + (size_t)it.nr * c;
    const cx<T>* __restrict__ f = reinterpret_cast<const cx<T>*>(it.f);
    const cx<T>* __restrict__ b = reinterpret_cast<const cx<T>*>(it.b);
    cx<T> wv = cmake<T>(0, 0);
    for (int i = lane; i < it.nr; i += 64) cfma(wv, b[i], col[i]);
    wv.re = wave_sum(wv.re); wv.im = wave_sum(wv.im);
    wv.re = -wv.re; wv.im = -wv.im;
    for (int i = lane; i < it.nr; i += 64) { cx<T> v = col[i]; cfma(v, f[i], wv); col[i] = v; }
}
int plan_loop_antiproject(LoopProjItem* it, int n) {
    return lay_out(it, n, &LoopProjItem::wg_begin, nullptr, [](LoopProjItem& p) { return (p.nc + 3) / 4; });
}
template <class T> void launch_loop_antiproject(hipStream_t s, const LoopProjItem* d_items, int nitems, int total_wgs) {
    if (nitems <= 0 || total_wgs <= 0) return;
    hipLaunchKernelGGL((loop_antiproject_kernel<T>), dim3(total_wgs), dim3(256), 0, s, d_items, nitems); TNQS_CHECK_LAUNCH();
}
template void launch_loop_antiproject<float>(hipStream_t, const LoopProjItem*, int, int);
template void launch_loop_antiproject<double>(hipStream_t, const LoopProjItem*, int, int);

// ---- trace of a product: out = sum_ij X[i,j] Y[j,i], X p x q, Y q x p; f64 accumulation.  Workgroup g of an item takes the columns j = g, g + nwg, ...
// of X and leaves one complex128 partial; the tail kernel (one workgroup per item) sums an item's partials ---------------------------------------------
template <class T> __global__ __launch_bounds__(256) void loop_trace_kernel(const LoopTraceItem* __restrict__ items, int nitems) {
    __shared__ double sh[17];
    const int gt = blockIdx.x;
    const int lo = find_item(items, nitems, &LoopTraceItem::wg_begin, gt);
    const LoopTraceItem it = items[lo];
    const int lw = gt - it.wg_begin;
    if (lw >= it.nwg) return;
    const cx<T>* __restrict__ X = reinterpret_cast<const cx<T>*>(it.X);
    const cx<T>* __restrict__ Y = reinterpret_cast<const cx<T>*>(it.Y);
    double re = 0, im = 0;
    for (int j = lw; j < it.q; j += it.nwg)
        for (int i = threadIdx.x; i < it.p; i += 256) {
            const cx<T> x = X[(size_t)i + (size_t)it.p * j], y = Y[(size_t)j + (size_t)it.q * i];
            re += (double)x.re * (double)y.re - (double)x.im * (double)y.im;
            im += (double)x.re * (double)y.im + (double)x.im * (double)y.re;
        }
    re = block_sum(re, sh); im = block_sum(im, sh);
    if (threadIdx.x == 0) { it.partial[2 * lw] = re; it.partial[2 * lw + 1] = im; }
}
__global__ __launch_bounds__(256) void loop_trace_tail_kernel(const LoopTraceItem* __restrict__ items) {
    __shared__ double sh[17];
    const LoopTraceItem it = items[blockIdx.x];
    double re = 0, im = 0;
    for (int g = threadIdx.x; g < it.nwg; g += 256) { re += it.partial[2 * g]; im += it.partial[2 * g + 1]; }
    re = block_sum(re, sh); im = block_sum(im, sh);
    if (threadIdx.x == 0) { it.out[0] = re; it.out[1] = im; }
}
int plan_loop_trace(LoopTraceItem* it, int n) {
    return lay_out(it, n, &LoopTraceItem::wg_begin, nullptr, [](LoopTraceItem& t) { t.nwg = std::max(1, std::min(t.q, 64)); return t.nwg; });
}
template <class T> void launch_loop_trace(hipStream_t s, const LoopTraceItem* d_items, int nitems, int total_wgs) {
    if (nitems <= 0 || total_wgs <= 0) return;
    hipLaunchKernelGGL((loop_trace_kernel<T>), dim3(total_wgs), dim3(256), 0, s, d_items, nitems); TNQS_CHECK_LAUNCH();
    hipLaunchKernelGGL(loop_trace_tail_kernel, dim3(nitems), dim3(256), 0, s, d_items); TNQS_CHECK_LAUNCH();
}
template void launch_loop_trace<float>(hipStream_t, const LoopTraceItem*, int, int);
template void launch_loop_trace<double>(hipStream_t, const LoopTraceItem*, int, int);

// ---- full contraction of two tensors in the same layout: out = sum_i X[i] Y[i] (bilinear), f64 accumulation, 64-bit length.  Workgroup g of an item takes
// the elements g 256 + t, + nwg 256, ...; partials and tail as for the trace --------------------------------------------------------------------------------
template <class T> __global__ __launch_bounds__(256) void loop_dot_kernel(const LoopDotItem* __restrict__ items, int nitems) {
    __shared__ double sh[17];
    const int gt = blockIdx.x;
    const int lo = find_item(items, nitems, &LoopDotItem::wg_begin, gt);
    const LoopDotItem it = items[lo];
    const int lw = gt - it.wg_begin;
    if (lw >= it.nwg) return;
    const cx<T>* __restrict__ X = reinterpret_cast<const cx<T>*>(it.X);
    const cx<T>* __restrict__ Y = reinterpret_cast<const cx<T>*>(it.Y);
    double re = 0, im = 0;
    for (long long i = (long long)lw * 256 + threadIdx.x; i < it.n; i += (long long)it.nwg * 256) {
        const cx<T> x = X[i], y = Y[i];
        re += (double)x.re * (double)y.re - (double)x.im * (double)y.im;
        im += (double)x.re * (double)y.im + (double)x.im * (double)y.re;
    }
    re = block_sum(re, sh); im = block_sum(im, sh);
    if (threadIdx.x == 0) { it.partial[2 * lw] = re; it.partial[2 * lw + 1] = im; }
}
__global__ __launch_bounds__(256) void loop_dot_tail_kernel(const LoopDotItem* __restrict__ items) {
    __shared__ double sh[17];
    const LoopDotItem it = items[blockIdx.x];
    double re = 0, im = 0;
    for (int g = threadIdx.x; g < it.nwg; g += 256) { re += it.partial[2 * g]; im += it.partial[2 * g + 1]; }
    re = block_sum(re, sh); im = block_sum(im, sh);
    if (threadIdx.x == 0) { it.out[0] = re; it.out[1] = im; }
}
int plan_loop_dot(LoopDotItem* it, int n) {
    return lay_out(it, n, &LoopDotItem::wg_begin, nullptr, [](LoopDotItem& t) {
        t.nwg = (int)std::max<long long>(1, std::min<long long>((t.n + 4095) / 4096, kLoopDotMaxWgs)); return t.nwg; });
}
template <class T> void launch_loop_dot(hipStream_t s, const LoopDotItem* d_items, int nitems, int total_wgs) {
    if (nitems <= 0 || total_wgs <= 0) return;
    hipLaunchKernelGGL((loop_dot_kernel<T>), dim3(total_wgs), dim3(256), 0, s, d_items, nitems); TNQS_CHECK_LAUNCH();
    hipLaunchKernelGGL(loop_dot_tail_kernel, dim3(nitems), dim3(256), 0, s, d_items); TNQS_CHECK_LAUNCH();
}
template void launch_loop_dot<float>(hipStream_t, const LoopDotItem*, int, int);
template void launch_loop_dot<double>(hipStream_t, const LoopDotItem*, int, int);

}  // namespace tnqs
