// kernels_bp.hip -- belief propagation, any dims, c64/c128: the message epilogue, the one-kernel message of a small site, the BP normalisation
// (rescale, edge scalars) and the symmetric gauge.
// Reference call sites replaced (paths relative to the reference repo):
//   msg_finalize: abstract...:182-187 (m / sum(m)) + message_diff beliefpropagationcache.jl:17-21
#include "kernels.hpp"
#include "device_common.hpp"
#include "jacobi_common.hpp"
#include "launch_util.hpp"

namespace tnqs {

// ------------------------------------------------------------------------------------------------------------
// BP message epilogue: reduce partials, normalise by the sum of all elements, message_diff
// ------------------------------------------------------------------------------------------------------------
// several block-wide sums with ONE pair of barriers (blockDim.x <= 1024); results valid in every thread
template <int N>
__device__ __forceinline__ void block_sum_n(double (&v)[N], double* sh /* >= 17 N doubles */) {
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
// 1024 threads per message (round 5): with 256 a chi = 32 message was four elements per thread x 16 partials in dependent groups of eight loads, then six
// block-wide sums of three barriers each -- 50 us per launch on the critical path of every BP level, whatever the lattice size; now one element per thread and
// two reductions (element sum; the four sums of message_diff together)
template <class T>
__global__ __launch_bounds__(1024) void msg_finalize_kernel(const MsgFinalItem* __restrict__ items) {
    __shared__ double sh[17 * 4];
    const MsgFinalItem it = items[blockIdx.x];
    const int n2 = it.chi * it.chi;
    const int NT = blockDim.x;
    const cx<T>* p = reinterpret_cast<const cx<T>*>(it.partial);
    cx<T>* out = reinterpret_cast<cx<T>*>(it.new_msg);
    const cx<T>* old = reinterpret_cast<const cx<T>*>(it.old_msg);
    // pass 1: reduce chunks (fixed order) into new_msg, accumulate the element sum
    double s2[2] = {0, 0};
    for (int e = threadIdx.x; e < n2; e += NT) {
        // eight independent partial sums (fixed order): the loads of a thread do not depend on each other, so eight are in flight at a
        // time instead of one -- a message with thousands of partials took a millisecond here
        T pr[8] = {0, 0, 0, 0, 0, 0, 0, 0}, pi[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        int c = 0;
        // (32 loads in flight, added in the same order as the groups of eight below: a level of the forest-cover order has a few messages of a few hundred
        //  partials each -- many short workgroups per site -- and their 32 dependent rounds of eight loads were 25 us of a 60 us level)
        for (; c + 32 <= it.nchunks; c += 32) {
            cx<T> v[32];
#pragma unroll
            for (int u = 0; u < 32; ++u) v[u] = p[(size_t)(c + u) * n2 + e];
#pragma unroll
            for (int u = 0; u < 32; ++u) { pr[u & 7] += v[u].re; pi[u & 7] += v[u].im; }
        }
        for (; c + 8 <= it.nchunks; c += 8) {
#pragma unroll
            for (int u = 0; u < 8; ++u) { cx<T> v = p[(size_t)(c + u) * n2 + e]; pr[u] += v.re; pi[u] += v.im; }
        }
        for (; c < it.nchunks; ++c) { cx<T> v = p[(size_t)c * n2 + e]; pr[c & 7] += v.re; pi[c & 7] += v.im; }
        const T re = ((pr[0] + pr[1]) + (pr[2] + pr[3])) + ((pr[4] + pr[5]) + (pr[6] + pr[7]));
        const T im = ((pi[0] + pi[1]) + (pi[2] + pi[3])) + ((pi[4] + pi[5]) + (pi[6] + pi[7]));
        out[e] = cmake<T>(re, im);
        s2[0] += re; s2[1] += im;
    }
    block_sum_n<2>(s2, sh);
    const double sre = s2[0], sim = s2[1];
    // m / sum(m)   (abstractbeliefpropagationcache.jl:182-187; skipped when the sum is exactly zero)
    double ire = 1, iim = 0;
    if (it.normalize && (sre != 0 || sim != 0)) { double d = sre * sre + sim * sim; ire = sre / d; iim = -sim / d; }
    double d4[4] = {0, 0, 0, 0};       // Re, Im of dot(new, old), |new|^2, |old|^2
    for (int e = threadIdx.x; e < n2; e += NT) {
        cx<T> v = out[e];              // (written by this thread above)
        double re = v.re * ire - v.im * iim, im = v.re * iim + v.im * ire;
        cx<T> w = cmake<T>((T)re, (T)im);
        out[e] = w;
        double ore, oim;
        if (old) { ore = old[e].re; oim = old[e].im; } else { ore = (e % it.chi == e / it.chi) ? 1.0 : 0.0; oim = 0; }
        // dot(a, b) = sum conj(a) b with a = new, b = old  (beliefpropagationcache.jl:17-21)
        d4[0] += (double)w.re * ore + (double)w.im * oim;
        d4[1] += (double)w.re * oim - (double)w.im * ore;
        d4[2] += (double)w.re * w.re + (double)w.im * w.im;
        d4[3] += ore * ore + oim * oim;
    }
    block_sum_n<4>(d4, sh);
    if (threadIdx.x == 0 && it.diff_out) {
        double f = (d4[0] * d4[0] + d4[1] * d4[1]) / (d4[2] * d4[3]);
        *it.diff_out = 1.0 - f;
    }
}
template <class T> void launch_msg_finalize(hipStream_t s, const MsgFinalItem* d_items, int nitems) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL((msg_finalize_kernel<T>), dim3(nitems), dim3(1024), 0, s, d_items); TNQS_CHECK_LAUNCH();
}
template void launch_msg_finalize<float>(hipStream_t, const MsgFinalItem*, int);
template void launch_msg_finalize<double>(hipStream_t, const MsgFinalItem*, int);

// ------------------------------------------------------------------------------------------------------------
// BP message of a SMALL site in one kernel (round 5): a site tensor of at most 8192 elements (64 KiB: heavy-hex chi = 16, every boundary site of a chi <= 16
// lattice) lives in LDS for the whole message -- absorb the incoming messages leg by leg (ping-pong between two LDS copies), then contract with conj(psi) over
// everything but the outgoing leg.  One workgroup per (site, outgoing message); the result is the raw message (one partial for msg_finalize).  The generic route
// streamed such a tensor through one fiber-GEMM launch per leg plus a Gram launch, each with its descriptor copy: 16 launch groups of ~90 us per heavy-hex layer at
// 0.09 TB/s (updated_message, abstractbeliefpropagationcache.jl:162-190)
// ------------------------------------------------------------------------------------------------------------
// The same message with EVERY leg 16-dimensional (heavy-hex at chi = 16: the shape the kernel exists for) on v_mfma_f32_16x16x4_f32 -- the scalar form below reads
// two LDS operands per multiply-add and is bound by the LDS bandwidth of its CU (55 us per degree-3 message); here an operand is read once per 16 multiply-adds.
// Lane l = (c = l & 15, g = l >> 4) supplies A[i = c][k = g] and B[k = g][j = c] and receives C[row = 4 g + r][col = c]; instruction t of a product takes
// contraction index 4 g + t (kernels_plane.hip).  Four real products per complex one.
//   absorb leg k (stride P):  out[fiber, qo] = sum_q cur[fiber, q] M[q, qo], computed transposed: A = M^T from registers, B = 16 fibers x 16 q from LDS,
//                             C[qo][fiber] stored along the fibers (contiguous); a wave takes tiles of 16 fibers
//   Gram over all but leg jo: out[i, j] = sum_rest cur[rest, i] conj psi[rest, j]: A, B = 4 rest values x 16 from the two LDS copies per instruction; the waves split
//                             the rest index and their 16 x 16 partial sums meet in LDS
template <int NT>
__device__ __forceinline__ void bp_small_site_mfma16(const SmallMsgItem& it, int E, char* smem, size_t smem_bytes) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = NT >> 6, c = lane & 15, g = lane >> 4;
    cx<float>* cur = reinterpret_cast<cx<float>*>(smem);
    cx<float>* nxt = cur + E;
    // psi: 16-byte loads, all in flight at once, kept in registers for the second copy (E <= 8192: at most four per thread); the message matrices of all legs
    // are fetched behind them (A[i = qo = c][k = q = 4 g + t] = M[q, qo]: four consecutive numbers per lane) -- one exposed memory latency per message
    const v4f* p4 = reinterpret_cast<const v4f*>(it.psi);
    const int n4 = E >> 1;
    v4f keep[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) if (tid + NT * u < n4) keep[u] = p4[tid + NT * u];
    float mr[8][4], mi[8][4];
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (k < it.z && k != it.jo && it.M[k]) {
            const cx<float>* Mg = reinterpret_cast<const cx<float>*>(it.M[k]);
#pragma unroll
            for (int t = 0; t < 4; ++t) { const cx<float> v = Mg[(4 * g + t) + 16 * c]; mr[k][t] = v.re; mi[k][t] = v.im; }
        }
#pragma unroll
    for (int u = 0; u < 4; ++u) if (tid + NT * u < n4) reinterpret_cast<v4f*>(cur)[tid + NT * u] = keep[u];
    __syncthreads();
    const int ntile = E >> 8;                                         // tiles of 16 fibers of 16
    int P = it.d;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (k >= it.z) break;
        if (k != it.jo && it.M[k]) {
            for (int T = w; T < ntile; T += nw) {
                const int F = 16 * T + c, pre = F % P, post = F / P;
                const size_t base = pre + (size_t)P * 16 * post;
                v4f Cr = {0.f, 0.f, 0.f, 0.f}, Ci = Cr;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const cx<float> x = cur[base + (size_t)P * (4 * g + t)];                                               // B[k = q][j = fiber c]
                    Cr = __builtin_amdgcn_mfma_f32_16x16x4f32(mr[k][t], x.re, Cr, 0, 0, 0);
                    Cr = __builtin_amdgcn_mfma_f32_16x16x4f32(-mi[k][t], x.im, Cr, 0, 0, 0);
                    Ci = __builtin_amdgcn_mfma_f32_16x16x4f32(mr[k][t], x.im, Ci, 0, 0, 0);
                    Ci = __builtin_amdgcn_mfma_f32_16x16x4f32(mi[k][t], x.re, Ci, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) nxt[base + (size_t)P * (4 * g + r)] = cmake<float>(Cr[r], Ci[r]);              // C[row = qo = 4 g + r][col = fiber c]
            }
            __syncthreads();
            cx<float>* t_ = cur; cur = nxt; nxt = t_;
        }
        P *= 16;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) if (tid + NT * u < n4) reinterpret_cast<v4f*>(nxt)[tid + NT * u] = keep[u];
    __syncthreads();
    int Po = it.d; for (int k = 0; k < it.jo; ++k) Po *= 16;
    const int nstep = E >> 6;                                         // instructions' worth of the rest index: 4 rest values each
    int na = nw < nstep ? nw : nstep;                                 // waves that take part; their 2 KiB partials must fit the kernel's LDS
    if ((size_t)na * 2048 > smem_bytes) na = (int)(smem_bytes / 2048);
    v4f Or = {0.f, 0.f, 0.f, 0.f}, Oi = Or;
    if (w < na)
        for (int st = w; st < nstep; st += na) {
            const int R = 4 * st + g, pre = R % Po, post = R / Po;
            const size_t base = pre + (size_t)Po * 16 * post + (size_t)Po * c;
            const cx<float> a = cur[base], b = nxt[base];             // A[i = c][k = rest], B[k = rest][j = c]
            Or = __builtin_amdgcn_mfma_f32_16x16x4f32(a.re, b.re, Or, 0, 0, 0);
            Or = __builtin_amdgcn_mfma_f32_16x16x4f32(a.im, b.im, Or, 0, 0, 0);
            Oi = __builtin_amdgcn_mfma_f32_16x16x4f32(a.im, b.re, Oi, 0, 0, 0);
            Oi = __builtin_amdgcn_mfma_f32_16x16x4f32(-a.re, b.im, Oi, 0, 0, 0);
        }
    __syncthreads();                                                  // both copies have been consumed: the partial sums go over them
    cx<float>* part = reinterpret_cast<cx<float>*>(smem);
    if (w < na) {
#pragma unroll
        for (int r = 0; r < 4; ++r) part[256 * w + (4 * g + r) + 16 * c] = cmake<float>(Or[r], Oi[r]);                     // out[i + 16 j], i = 4 g + r, j = c
    }
    __syncthreads();
    static_assert(NT >= 256, "one thread per element of the 16 x 16 message");
    cx<float> val = cmake<float>(0.f, 0.f);
    if (tid < 256) {
        float sr = 0.f, si = 0.f;
        for (int u = 0; u < na; ++u) { const cx<float> v = part[256 * u + tid]; sr += v.re; si += v.im; }
        val = cmake<float>(sr, si);
    }
    if (!it.new_msg) { if (tid < 256) reinterpret_cast<cx<float>*>(it.out)[tid] = val; return; }
    // ---- the epilogue of msg_finalize_kernel on the message this workgroup holds: m / sum(m) (abstractbeliefpropagationcache.jl:182-187; skipped when the sum is
    // exactly zero), message_diff against the previous message (beliefpropagationcache.jl:17-21) -------------------------------------------------------------
    __shared__ double sh[17 * 4];
    double s2[2] = {(double)val.re, (double)val.im};
    block_sum_n<2>(s2, sh);
    const double sre = s2[0], sim = s2[1];
    double ire = 1, iim = 0;
    if (it.normalize && (sre != 0 || sim != 0)) { const double d = sre * sre + sim * sim; ire = sre / d; iim = -sim / d; }
    double d4[4] = {0, 0, 0, 0};       // Re, Im of dot(new, old), |new|^2, |old|^2
    if (tid < 256) {
        const double re = val.re * ire - val.im * iim, im = val.re * iim + val.im * ire;
        const cx<float> wv = cmake<float>((float)re, (float)im);
        reinterpret_cast<cx<float>*>(it.new_msg)[tid] = wv;
        const cx<float>* old = reinterpret_cast<const cx<float>*>(it.old_msg);
        double ore, oim;
        if (old) { ore = old[tid].re; oim = old[tid].im; } else { ore = ((tid & 15) == (tid >> 4)) ? 1.0 : 0.0; oim = 0; }
        d4[0] = (double)wv.re * ore + (double)wv.im * oim;
        d4[1] = (double)wv.re * oim - (double)wv.im * ore;
        d4[2] = (double)wv.re * wv.re + (double)wv.im * wv.im;
        d4[3] = ore * ore + oim * oim;
    }
    block_sum_n<4>(d4, sh);
    if (tid == 0 && it.diff_out) *it.diff_out = 1.0 - (d4[0] * d4[0] + d4[1] * d4[1]) / (d4[2] * d4[3]);
}
template <int NT>
__global__ __launch_bounds__(NT) void bp_small_site_kernel(const SmallMsgItem* __restrict__ items) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const SmallMsgItem it = items[blockIdx.x];
    const int tid = threadIdx.x;
    int E = it.d; for (int k = 0; k < it.z; ++k) E *= it.chi[k];
    cx<float>* cur = reinterpret_cast<cx<float>*>(smem);
    cx<float>* nxt = cur + E;
    cx<float>* Ms = nxt + E;                                          // one message matrix, TRANSPOSED: Ms[qo + c q] = M[q + c qo] (<= 32 x 32)
    const cx<float>* psi = reinterpret_cast<const cx<float>*>(it.psi);
    if (it.mfma) { bp_small_site_mfma16<NT>(it, E, smem, (size_t)E * 16 + 32 * 32 * 8); return; }
    for (int e = tid; e < E; e += NT) cur[e] = psi[e];
    __syncthreads();
    int P = it.d;                                                     // stride of leg k
    for (int k = 0; k < it.z; ++k) {
        const int c = it.chi[k];
        if (k != it.jo && it.M[k]) {
            const cx<float>* Mg = reinterpret_cast<const cx<float>*>(it.M[k]);
            for (int e = tid; e < c * c; e += NT) Ms[(e / c) + c * (e % c)] = Mg[e];
            __syncthreads();
            // one OUTPUT element per thread and step: out[pre, qo, post] = sum_q cur[pre, q, post] M[q, qo].  Consecutive threads take consecutive output
            // elements: the stores are contiguous, the lanes of a wave read few distinct fibers (broadcasts) and consecutive entries of the transposed matrix
            // (pre, qo, post) of e = tid + NT t by carries instead of divisions: an integer division is ~40 instructions, more than the 16-term sum it would index
            int pre = tid % P, qo = (tid / P) % c, post = tid / (P * c);
            const int dpre = NT % P, dq = (NT / P) % c, dpost = NT / (P * c);
            for (int e = tid; e < E; e += NT, pre += dpre, qo += dq, post += dpost) {
                if (pre >= P) { pre -= P; ++qo; }
                if (qo >= c) { qo -= c; ++post; }
                const cx<float>* src = cur + pre + (size_t)P * c * post;
                const cx<float>* mrow = Ms + qo;
                float ar = 0.f, ai = 0.f, br = 0.f, bi = 0.f;
                int q = 0;
                for (; q + 1 < c; q += 2) {
                    const cx<float> v0 = src[(size_t)P * q], m0 = mrow[c * q], v1 = src[(size_t)P * (q + 1)], m1 = mrow[c * (q + 1)];
                    ar += v0.re * m0.re - v0.im * m0.im; ai += v0.re * m0.im + v0.im * m0.re;
                    br += v1.re * m1.re - v1.im * m1.im; bi += v1.re * m1.im + v1.im * m1.re;
                }
                if (q < c) { const cx<float> v0 = src[(size_t)P * q], m0 = mrow[c * q]; ar += v0.re * m0.re - v0.im * m0.im; ai += v0.re * m0.im + v0.im * m0.re; }
                nxt[e] = cmake<float>(ar + br, ai + bi);
            }
            __syncthreads();
            cx<float>* t = cur; cur = nxt; nxt = t;
        }
        P *= c;
    }
    // psi again, into the free copy; then out[i + co j] = sum_rest cur[rest, i] conj(psi[rest, j]) over everything but the outgoing leg
    for (int e = tid; e < E; e += NT) nxt[e] = psi[e];
    __syncthreads();
    int Po = it.d; for (int k = 0; k < it.jo; ++k) Po *= it.chi[k];
    const int co = it.chi[it.jo], nrest = E / co;
    cx<float>* out = reinterpret_cast<cx<float>*>(it.out);
    // thread = (output element o, slice of the rest index): co^2 outputs x nsl slices fill the workgroup; partial sums meet in LDS (behind the message matrix)
    const int no = co * co;
    int nsl = NT / no; if (nsl < 1) nsl = 1; if (nsl > 16) nsl = 16;
    float* red = reinterpret_cast<float*>(Ms);                        // 2 * NT floats <= 8 KiB (the matrix slot holds 8 KiB)
    for (int o0 = 0; o0 < no; o0 += NT / nsl) {
        const int o = o0 + tid / nsl, sl = tid % nsl;
        float ar = 0.f, ai = 0.f;
        if (o < no && tid < (NT / nsl) * nsl) {
            const int i = o % co, j = o / co;
            int pre = sl % Po, post = sl / Po; const int dpre = nsl % Po, dpost = nsl / Po;
            for (int r = sl; r < nrest; r += nsl, pre += dpre, post += dpost) {
                if (pre >= Po) { pre -= Po; ++post; }
                const size_t base = pre + (size_t)Po * co * post;
                const cx<float> a = cur[base + (size_t)Po * i], b = nxt[base + (size_t)Po * j];
                ar += a.re * b.re + a.im * b.im; ai += a.im * b.re - a.re * b.im;
            }
        }
        __syncthreads();
        red[2 * tid] = ar; red[2 * tid + 1] = ai;
        __syncthreads();
        if (sl == 0 && o < no && tid < (NT / nsl) * nsl) {
            float sr = 0.f, si = 0.f;
            for (int u = 0; u < nsl; ++u) { sr += red[2 * (tid + u)]; si += red[2 * (tid + u) + 1]; }
            out[o] = cmake<float>(sr, si);
        }
    }
}
void launch_bp_small_site(hipStream_t s, const SmallMsgItem* d_items, int nitems, int max_elems) {
    if (nitems <= 0) return;
    const size_t lds = (size_t)max_elems * 16 + 32 * 32 * 8;
    // 1024 threads: the LDS footprint allows one workgroup per CU, and with 256 threads (one wave per SIMD) every LDS read of the dependent sums was exposed --
    // 107 us per message of a heavy-hex degree-3 site whatever the number of messages in the launch
    set_max_dynamic_lds((const void*)bp_small_site_kernel<1024>, (size_t)(160 * 1024 - 1024));
    hipLaunchKernelGGL(bp_small_site_kernel<1024>, dim3(nitems), dim3(1024), lds, s, d_items); TNQS_CHECK_LAUNCH();
}

// ------------------------------------------------------------------------------------------------------------
// BP normalisation (rescale!, beliefpropagationcache.jl:82-140)
// ------------------------------------------------------------------------------------------------------------
template <class T> __device__ __forceinline__ cx<double> msg_elem(const cx<T>* m, int e, int chi) {
    if (m) return cmake<double>((double)m[e].re, (double)m[e].im);
    return cmake<double>((e % chi) == (e / chi) ? 1.0 : 0.0, 0.0);
}
template <class T> __global__ __launch_bounds__(256) void msg_rescale_kernel(const MsgRescaleItem* __restrict__ items) {
    __shared__ double sh[17];
    const MsgRescaleItem it = items[blockIdx.x];
    const cx<T>* a = reinterpret_cast<const cx<T>*>(it.me); const cx<T>* b = reinterpret_cast<const cx<T>*>(it.mer);
    const int n2 = it.chi * it.chi;
    double na = 0, nb = 0, pr = 0, pi = 0;
    for (int e = threadIdx.x; e < n2; e += 256) {
        cx<double> x = msg_elem(a, e, it.chi), y = msg_elem(b, e, it.chi);
        na += x.re * x.re + x.im * x.im; nb += y.re * y.re + y.im * y.im;
        pr += x.re * y.re - x.im * y.im; pi += x.re * y.im + x.im * y.re;
    }
    na = block_sum(na, sh); nb = block_sum(nb, sh); pr = block_sum(pr, sh); pi = block_sum(pi, sh);
    const double ia = na > 0 ? 1.0 / sqrt(na) : 0.0, ib = nb > 0 ? 1.0 / sqrt(nb) : 0.0;
    double nr = pr * ia * ib, ni = pi * ia * ib;             // n = scalar(normalize(me) * normalize(mer))
    double sgn = 1.0;
    if (ni == 0.0) { sgn = (nr > 0) - (nr < 0); nr *= sgn; }  // isreal(n): me *= sign(n), n *= sign(n)
    // 1/sqrt(n), principal branch
    const double mod = sqrt(nr * nr + ni * ni), arg = atan2(ni, nr);
    const double r = mod > 0 ? 1.0 / sqrt(mod) : 0.0, ph = -0.5 * arg;
    const double fr = r * cos(ph), fi = r * sin(ph);
    cx<T>* ao = reinterpret_cast<cx<T>*>(it.me_out); cx<T>* bo = reinterpret_cast<cx<T>*>(it.mer_out);
    for (int e = threadIdx.x; e < n2; e += 256) {
        cx<double> x = msg_elem(a, e, it.chi), y = msg_elem(b, e, it.chi);
        x.re *= ia * sgn; x.im *= ia * sgn; y.re *= ib; y.im *= ib;
        ao[e] = cmake<T>((T)(x.re * fr - x.im * fi), (T)(x.re * fi + x.im * fr));
        bo[e] = cmake<T>((T)(y.re * fr - y.im * fi), (T)(y.re * fi + y.im * fr));
    }
}
template <class T> void launch_msg_rescale(hipStream_t s, const MsgRescaleItem* d_items, int nitems) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL((msg_rescale_kernel<T>), dim3(nitems), dim3(256), 0, s, d_items); TNQS_CHECK_LAUNCH();
}
template void launch_msg_rescale<float>(hipStream_t, const MsgRescaleItem*, int);
template void launch_msg_rescale<double>(hipStream_t, const MsgRescaleItem*, int);
template <class T> __global__ __launch_bounds__(256) void edge_scalar_kernel(const EdgeScalarItem* __restrict__ items) {
    __shared__ double sh[17];
    const EdgeScalarItem it = items[blockIdx.x];
    const cx<T>* a = reinterpret_cast<const cx<T>*>(it.me); const cx<T>* b = reinterpret_cast<const cx<T>*>(it.mer);
    const int n2 = it.chi * it.chi;
    double pr = 0, pi = 0;
    for (int e = threadIdx.x; e < n2; e += 256) {
        cx<double> x = msg_elem(a, e, it.chi), y = msg_elem(b, e, it.chi);
        pr += x.re * y.re - x.im * y.im; pi += x.re * y.im + x.im * y.re;
    }
    pr = block_sum(pr, sh); pi = block_sum(pi, sh);
    if (threadIdx.x == 0) { it.out[0] = pr; it.out[1] = pi; }
}
template <class T> void launch_edge_scalar(hipStream_t s, const EdgeScalarItem* d_items, int nitems) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL((edge_scalar_kernel<T>), dim3(nitems), dim3(256), 0, s, d_items); TNQS_CHECK_LAUNCH();
}
template void launch_edge_scalar<float>(hipStream_t, const EdgeScalarItem*, int);
template void launch_edge_scalar<double>(hipStream_t, const EdgeScalarItem*, int);

// ------------------------------------------------------------------------------------------------------------
// symmetric gauge (src/symmetric_gauge.jl)
// ------------------------------------------------------------------------------------------------------------
template <class T> __global__ __launch_bounds__(256) void symg_build_kernel(const SymGaugeItem* __restrict__ items) {
    __shared__ double lx[256], ly[256];
    const SymGaugeItem it = items[blockIdx.x];
    const int n = it.n;
    const cx<double>* AX = reinterpret_cast<const cx<double>*>(it.AX); const cx<double>* VX = reinterpret_cast<const cx<double>*>(it.VX);
    const cx<double>* AY = reinterpret_cast<const cx<double>*>(it.AY); const cx<double>* VY = reinterpret_cast<const cx<double>*>(it.VY);
    for (int j = threadIdx.x; j < n; j += 256) {
        double a = 0, b = 0;            // Rayleigh quotients v_j^dagger H v_j
        for (int i = 0; i < n; ++i) { cx<double> v = VX[i + n * j], w = AX[i + n * j]; a += v.re * w.re + v.im * w.im;
                                      cx<double> p = VY[i + n * j], q = AY[i + n * j]; b += p.re * q.re + p.im * q.im; }
        a += it.reg; b += it.reg;       // map_diag(x -> x + regularization) (:15-16)
        if (a < 0 || b < 0) *it.flag = 1;     // sqrt of a negative real: DomainError in the reference
        lx[j] = a; ly[j] = b;
    }
    __syncthreads();
    cx<double>* rx = reinterpret_cast<cx<double>*>(it.rx); cx<double>* ry = reinterpret_cast<cx<double>*>(it.ry);
    cx<double>* irx = reinterpret_cast<cx<double>*>(it.irx); cx<double>* iry = reinterpret_cast<cx<double>*>(it.iry);
    // ITensors.eigen without index sets diagonalises M^T (the primed index is the row index), so every function of the message
    // enters as f(M)^T = conj(f(M)) [l, l']  (:13-24)
    for (int e = threadIdx.x; e < n * n; e += 256) {
        int i = e % n, l = e / n;
        cx<double> sx = cmake<double>(0, 0), ix = sx, sy = sx, iy = sx;
        for (int j = 0; j < n; ++j) {
            cx<double> vi = VX[i + n * j], vl = VX[l + n * j];
            cx<double> o = cmake<double>(vi.re * vl.re + vi.im * vl.im, -(vi.im * vl.re - vi.re * vl.im));      // conj(vi conj(vl))
            double r = lx[j] > 0 ? sqrt(lx[j]) : 0.0, ir = lx[j] > 0 ? 1.0 / r : 0.0;
            sx.re += r * o.re; sx.im += r * o.im; ix.re += ir * o.re; ix.im += ir * o.im;
            cx<double> wi = VY[i + n * j], wl = VY[l + n * j];
            cx<double> p = cmake<double>(wi.re * wl.re + wi.im * wl.im, -(wi.im * wl.re - wi.re * wl.im));
            double q = ly[j] > 0 ? sqrt(ly[j]) : 0.0, iq = ly[j] > 0 ? 1.0 / q : 0.0;
            sy.re += q * p.re; sy.im += q * p.im; iy.re += iq * p.re; iy.im += iq * p.im;
        }
        rx[e] = sx; irx[e] = ix; ry[e] = sy; iry[e] = iy;
    }
    __syncthreads();
    __threadfence_block();
    cx<T>* Ce = reinterpret_cast<cx<T>*>(it.Ce); cx<T>* Ce0 = reinterpret_cast<cx<T>*>(it.Ce0);
    for (int e = threadIdx.x; e < n * n; e += 256) {          // Ce[l, c] = sum_l' rootX[l, l'] rootY[c, l']   (:29-30)
        int l = e % n, c = e / n;
        cx<double> acc = cmake<double>(0, 0);
        for (int k = 0; k < n; ++k) cfma(acc, rx[l + n * k], ry[c + n * k]);
        cx<T> v = cmake<T>((T)acc.re, (T)acc.im);
        Ce[e] = v; Ce0[e] = v;
    }
}
template <class T> void launch_symg_build(hipStream_t s, const SymGaugeItem* d_items, int nitems) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL((symg_build_kernel<T>), dim3(nitems), dim3(256), 0, s, d_items); TNQS_CHECK_LAUNCH();
}
template void launch_symg_build<float>(hipStream_t, const SymGaugeItem*, int);
template void launch_symg_build<double>(hipStream_t, const SymGaugeItem*, int);
template <class T> __global__ __launch_bounds__(256) void symg_finish_kernel(const SymGaugeItem* __restrict__ items) {
    __shared__ double sig[256];
    __shared__ int perm[256];
    const SymGaugeItem it = items[blockIdx.x];
    const int n = it.n;
    const cx<T>* A = reinterpret_cast<const cx<T>*>(it.Ce);       // U Sigma
    const cx<T>* V = reinterpret_cast<const cx<T>*>(it.Vsvd);
    for (int u = threadIdx.x; u < n; u += 256) {
        double s2 = 0;
        for (int i = 0; i < n; ++i) { cx<T> v = A[i + (size_t)n * u]; s2 += (double)v.re * v.re + (double)v.im * v.im; }
        sig[u] = (s2 == s2 && s2 < 1e300) ? sqrt(s2) : 0.0;
    }
    __syncthreads();
    for (int u = threadIdx.x; u < n; u += 256) {                  // descending order, stable
        perm[rank_desc(sig, n, u)] = u;
    }
    __syncthreads();
    for (int u = threadIdx.x; u < n; u += 256) it.S[u] = (double)(T)sig[perm[u]];
    const cx<double>* irx = reinterpret_cast<const cx<double>*>(it.irx); const cx<double>* iry = reinterpret_cast<const cx<double>*>(it.iry);
    cx<T>* Xs = reinterpret_cast<cx<T>*>(it.Xs); cx<T>* Xd = reinterpret_cast<cx<T>*>(it.Xd);
    for (int e = threadIdx.x; e < n * n; e += 256) {
        int l = e % n, u = e / n; int pu = perm[u]; double su = sig[pu];
        cx<double> a = cmake<double>(0, 0), b = cmake<double>(0, 0);
        if (su > 0) {
            for (int k = 0; k < n; ++k) {
                cx<T> x = A[k + (size_t)n * pu], y = V[k + (size_t)n * pu];
                cfma(a, irx[l + n * k], cmake<double>((double)x.re, (double)x.im));
                cfma(b, iry[l + n * k], cmake<double>((double)y.re, -(double)y.im));      // V^T of ITensors = conj of the right singular vectors
            }
            const double f = 1.0 / sqrt(su), gq = sqrt(su);       // U = A / sigma, times sqrt(sigma)
            a.re *= f; a.im *= f; b.re *= gq; b.im *= gq;
        }
        Xs[e] = cmake<T>((T)a.re, (T)a.im); Xd[e] = cmake<T>((T)b.re, (T)b.im);
    }
}
template <class T> void launch_symg_finish(hipStream_t s, const SymGaugeItem* d_items, int nitems) {
    if (nitems <= 0) return;
    hipLaunchKernelGGL((symg_finish_kernel<T>), dim3(nitems), dim3(256), 0, s, d_items); TNQS_CHECK_LAUNCH();
}
template void launch_symg_finish<float>(hipStream_t, const SymGaugeItem*, int);
template void launch_symg_finish<double>(hipStream_t, const SymGaugeItem*, int);

}  // namespace tnqs
