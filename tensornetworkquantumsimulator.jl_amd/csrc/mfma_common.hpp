// mfma_common.hpp -- the MFMA tile machinery shared by the matrix-core translation units (kernels_mfma.hip, kernels_plane.hip, kernels_chi64.hip, ...),
// on top of the vocabulary of device_common.hpp.
#pragma once
#include "device_common.hpp"
#include "gram_item.hpp"

namespace tnqs {

struct alignas(8) cf { float re, im; };

// GLOBAL-memory loads / stores.  The tensor pointers reach the kernels through item structs in device memory, so the compiler knows
// nothing about their address space and emits FLAT instructions; a flat load counts on BOTH vmcnt and lgkmcnt and returns out of order
// with respect to LDS traffic, so the first `s_waitcnt lgkmcnt(0)` in front of an LDS-fed MFMA also waits for every prefetch load in
// flight -- the "prefetch" is synchronous and a full memory latency is exposed per tile (seen in the ISA of every kernel of round 1).
// Casting to address space 1 gives global_load / global_store, which count on vmcnt only.
#define TNQS_AS1 __attribute__((address_space(1)))
__device__ __forceinline__ v4f ldg4(const void* p) { return *(const v4f TNQS_AS1*)(p); }
__device__ __forceinline__ v2f ldg2(const void* p) { return *(const v2f TNQS_AS1*)(p); }
__device__ __forceinline__ void stg4(void* p, v4f v) { *(v4f TNQS_AS1*)(p) = v; }
__device__ __forceinline__ void stg2(void* p, v2f v) { *(v2f TNQS_AS1*)(p) = v; }
__device__ __forceinline__ cf ldgc(const cf* p) { const v2f t = ldg2(p); cf r; r.re = t[0]; r.im = t[1]; return r; }
__device__ __forceinline__ void stgc(cf* p, cf v) { v2f t = {v.re, v.im}; stg2(p, t); }

// LDS-only workgroup barrier: __syncthreads() also drains vmcnt (global loads AND stores in flight), which would
// serialise the prefetch / store streams against the LDS hand-offs (cdna_hip_programming.md, "Pipelining across barriers").
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ------------------------------------------------------------------------------------------------------------
// complex 32 x 32 accumulator tile for v_mfma_f32_32x32x2_f32 (k = 2 per instruction: lanes 0..31 hold k = 0, lanes 32..63 k = 1).
//   M3 = false: the textbook product, four real MFMAs per complex rank-2 update, two accumulators (re, im).
//   M3 = true : Gauss' three-multiplication product, three real MFMAs and three accumulators
//                   k1 = (ar + ai) br,   k2 = ar (bi - br),   k3 = ai (br + bi);      re = k1 - k3,  im = k1 + k2
//               The operand sums cost three VALU instructions per update (they overlap the 3 x 64 matrix-core cycles); the recombination
//               is two VALU instructions per accumulator register, once per tile.  Error: |delta| <= c u (|a_r| + |a_i|)(|b_r| + |b_i|) per
//               term, i.e. the same NORMWISE bound as the four-multiplication product; the componentwise bound of the imaginary part is
//               lost (a tiny imaginary part next to a large real one carries the large one's rounding), which the BP messages and site
//               tensors -- compared and used normwise everywhere -- do not rely on.
// ------------------------------------------------------------------------------------------------------------
template <bool M3> struct CAcc32 {
    v16f a, b, c;
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int r = 0; r < 16; ++r) { a[r] = 0.f; b[r] = 0.f; if (M3) c[r] = 0.f; }
    }
    // acc += (ar + i ai) (br + i bi)
    __device__ __forceinline__ void mac(float ar, float ai, float br, float bi) {
        if (M3) {
            a = __builtin_amdgcn_mfma_f32_32x32x2f32(ar + ai, br, a, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x2f32(ar, bi - br, c, 0, 0, 0);
            b = __builtin_amdgcn_mfma_f32_32x32x2f32(ai, br + bi, b, 0, 0, 0);
        } else {
            a = __builtin_amdgcn_mfma_f32_32x32x2f32(ar, br, a, 0, 0, 0);
            a = __builtin_amdgcn_mfma_f32_32x32x2f32(-ai, bi, a, 0, 0, 0);
            b = __builtin_amdgcn_mfma_f32_32x32x2f32(ar, bi, b, 0, 0, 0);
            b = __builtin_amdgcn_mfma_f32_32x32x2f32(ai, br, b, 0, 0, 0);
        }
    }
    // the same update with the A-side combination supplied by the caller (a0 = ar + ai when M3, -ai otherwise: a constant of the wave in
    // the kernels that keep their matrix in registers); FIRST: the accumulators start from zero (inline constant, no register clearing)
    template <bool FIRST> __device__ __forceinline__ void mac_pre(float a0, float ar, float ai, float br, float bi) {
        const v16f z = (v16f)(0.f);
        if (M3) {
            a = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, br, FIRST ? z : a, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x2f32(ar, bi - br, FIRST ? z : c, 0, 0, 0);
            b = __builtin_amdgcn_mfma_f32_32x32x2f32(ai, br + bi, FIRST ? z : b, 0, 0, 0);
        } else {
            a = __builtin_amdgcn_mfma_f32_32x32x2f32(ar, br, FIRST ? z : a, 0, 0, 0);
            a = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bi, a, 0, 0, 0);
            b = __builtin_amdgcn_mfma_f32_32x32x2f32(ar, bi, FIRST ? z : b, 0, 0, 0);
            b = __builtin_amdgcn_mfma_f32_32x32x2f32(ai, br, b, 0, 0, 0);
        }
    }
    // the same update with the B-side combinations supplied by the caller: (bd, bs) = (bi - br, br + bi) when M3, (bi, -bi) otherwise
    template <bool FIRST> __device__ __forceinline__ void mac_bpre(float ar, float ai, float br, float bd, float bs) {
        const v16f z = (v16f)(0.f);
        if (M3) {
            a = __builtin_amdgcn_mfma_f32_32x32x2f32(ar + ai, br, FIRST ? z : a, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x2f32(ar, bd, FIRST ? z : c, 0, 0, 0);
            b = __builtin_amdgcn_mfma_f32_32x32x2f32(ai, bs, FIRST ? z : b, 0, 0, 0);
        } else {
            a = __builtin_amdgcn_mfma_f32_32x32x2f32(ar, br, FIRST ? z : a, 0, 0, 0);
            a = __builtin_amdgcn_mfma_f32_32x32x2f32(ai, bs, a, 0, 0, 0);
            b = __builtin_amdgcn_mfma_f32_32x32x2f32(ar, bd, FIRST ? z : b, 0, 0, 0);
            b = __builtin_amdgcn_mfma_f32_32x32x2f32(ai, br, b, 0, 0, 0);
        }
    }
    // (re, im) of every accumulator register, in place: a <- re, b <- im  (after mac / mac_pre / mac_bpre)
    __device__ __forceinline__ void finish() {
        if (M3) {
#pragma unroll
            for (int r = 0; r < 16; ++r) { const float k1 = a[r]; a[r] = k1 - b[r]; b[r] = k1 + c[r]; }
        }
    }
    // the same, one register at a time (the accumulators stay as they are): for accumulator tiles that are the next product's A operand
    __device__ __forceinline__ float re(int r) const { return M3 ? a[r] - b[r] : a[r]; }
    __device__ __forceinline__ float im(int r) const { return M3 ? a[r] + c[r] : b[r]; }
    // acc += (ar + i ai) conj(br + i bi); M3 keeps  sum (ar + ai) br,  sum ar (bi + br),  sum ai (br - bi)  -- no negated operand -- and
    // finish_conj() recombines  re = k1 - k3,  im = k1 - sum ar (bi + br)
    __device__ __forceinline__ void mac_conj(float ar, float ai, float br, float bi) {
        if (M3) {
            a = __builtin_amdgcn_mfma_f32_32x32x2f32(ar + ai, br, a, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x2f32(ar, bi + br, c, 0, 0, 0);
            b = __builtin_amdgcn_mfma_f32_32x32x2f32(ai, br - bi, b, 0, 0, 0);
        } else {
            a = __builtin_amdgcn_mfma_f32_32x32x2f32(ar, br, a, 0, 0, 0);
            a = __builtin_amdgcn_mfma_f32_32x32x2f32(ai, bi, a, 0, 0, 0);
            b = __builtin_amdgcn_mfma_f32_32x32x2f32(ai, br, b, 0, 0, 0);
            b = __builtin_amdgcn_mfma_f32_32x32x2f32(-ar, bi, b, 0, 0, 0);
        }
    }
    __device__ __forceinline__ void finish_conj() {
        if (M3) {
#pragma unroll
            for (int r = 0; r < 16; ++r) { const float k1 = a[r]; a[r] = k1 - b[r]; b[r] = k1 - c[r]; }
        }
    }
};

// ------------------------------------------------------------------------------------------------------------
// f64 Gram tiles (v_mfma_f64_16x16x4_f64; LDS tile: planes Xr / Xi, element (column c, tile row r) at c * TRP + r; lane = (l15, kq): column
// l15 of a 16-column panel, tile rows 16 kq .. 16 kq + 15).  A set of upper-triangle blocks that share one panel P: ROW = P supplies the rows
// (A operand) of every block and Q[j] the columns, !ROW = P supplies the columns (B operand) and Q[j] the rows; DIAGJ >= 0: block DIAGJ is (P, P).
// The shared panel's values are read from LDS, converted to f64 and combined ONCE per four k-steps for all N blocks (a block on its own
// converts four values and forms three sums per k-step).  out[i][j] += x[i] conj(x[j]) as three multiplications: (cr, ci, cc) accumulate
// sum (ar+ai) br, sum ai (br-bi), sum ar (bi+br), i.e. re = cr - ci, im = cr - cc.
// ------------------------------------------------------------------------------------------------------------
template <int N, bool ROW, int DIAGJ>
__device__ __forceinline__ void gram_f64_shared(const float* __restrict__ Xr, const float* __restrict__ Xi, int TRP, int l15, int kq, int P,
                                                const int (&Q)[N], v4d (&cr)[N], v4d (&ci)[N], v4d (&cc)[N]) {
#pragma unroll 1
    for (int hq = 0; hq < 4; ++hq) {                              // tile rows 16 kq + 4 hq .. + 3
        const int ro = (16 * P + l15) * TRP + 16 * kq + 4 * hq;
        const v4f p0 = *reinterpret_cast<const v4f*>(Xr + ro), p1 = *reinterpret_cast<const v4f*>(Xi + ro);
        double pr[4], pi[4], ps[4], pd[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) { pr[c] = (double)p0[c]; pi[c] = (double)p1[c]; ps[c] = pr[c] + pi[c]; pd[c] = pr[c] - pi[c]; }
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const bool dg = (j == DIAGJ);
            v4f o0 = p0, o1 = p1;
            if (!dg) { const int rb = (16 * Q[j] + l15) * TRP + 16 * kq + 4 * hq; o0 = *reinterpret_cast<const v4f*>(Xr + rb); o1 = *reinterpret_cast<const v4f*>(Xi + rb); }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const double qr = dg ? pr[c] : (double)o0[c], qi = dg ? pi[c] : (double)o1[c];
                if (ROW) {                                           // a = p, b = q
                    cr[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ps[c], qr, cr[j], 0, 0, 0);
                    ci[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(pi[c], qr - qi, ci[j], 0, 0, 0);
                    cc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(pr[c], qi + qr, cc[j], 0, 0, 0);
                } else {                                             // a = q, b = p
                    cr[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(qr + qi, pr[c], cr[j], 0, 0, 0);
                    ci[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(qi, pd[c], ci[j], 0, 0, 0);
                    cc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(qr, ps[c], cc[j], 0, 0, 0);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------
// tile <-> thread map (division-free inner loops).  A tile holds TA x TB fibers; one "unit" is VEC memory-adjacent
// elements of one k-slice ((s=0,s=1) of a fiber when D == 2, fibers (a, a+1) when D == 1 and TA is even).  Thread t
// owns unit u = t % U of the k-slices kp, kp+KP, ... ; t counts over NT threads (a 256-thread workgroup, or the 64 lanes of one wave).
// ------------------------------------------------------------------------------------------------------------
struct TileMap {
    int U, KP, u, kp;          // units per k-slice, k phases, this thread's unit / first k
    int row0, row1, c0, c1;    // LDS row and (s) column offset of the unit's two elements (row1 < 0: single)
    int al, bl, al1;           // tile-local fiber coordinates (validity tests)
    int vec;                   // elements per unit (1 or 2)
    long long off;             // element offset of the unit inside the tile's origin (k = 0)
    bool active;
};
__device__ __forceinline__ TileMap make_map(int tid, int D, int TA, int TB, long long PA, int K, int NT = 256) {
    TileMap m;
    const int rows = TA * TB;
    m.vec = (D == 2) ? 2 : ((D == 1 && (TA % 2 == 0) && (PA % 2 == 0)) ? 2 : 1);
    m.U = D * rows / m.vec;
    m.KP = m.U >= NT ? 1 : NT / m.U;
    m.u = tid % m.U; m.kp = tid / m.U;
    m.active = tid < m.U * m.KP;
    int e0 = m.u * m.vec;                 // first element index in (s, al, bl) order
    int s = e0 % D; int row = e0 / D;
    m.al = row % TA; m.bl = row / TA;
    m.row0 = row; m.c0 = s;
    if (m.vec == 2) { if (D == 2) { m.row1 = row; m.c1 = 1; m.al1 = m.al; } else { m.row1 = row + 1; m.c1 = 0; m.al1 = m.al + 1; } }
    else { m.row1 = -1; m.c1 = 0; m.al1 = m.al; }
    m.off = s + (long long)D * (m.al + PA * (long long)K * m.bl);
    return m;
}

// ------------------------------------------------------------------------------------------------------------
// Gram (f32 accumulate), KK = D*K <= 64:  partial[c][i + KK*j] = sum_{rows of chunk c} X[i,row] conj(Y[j,row])
// Tiles of 64 fibers, LDS layout [kk][row] (rows contiguous = memory order); the next tile's loads are in flight during the matrix block.
// Wave w: output rows block a = w & 1 (i in [32 a, 32 a + 32)) x all 64 columns, tile rows 32 (w >> 1) .. + 32 -- 64 accumulator
// registers per wave instead of 128, so that TWO workgroups fit a CU (one's barriers and LDS commits hide behind the other's MFMAs).
// Product: the two 32 x 32 complex accumulator blocks b = 0, 1 (columns 32 b ..) of a wave and how they are multiplied --
//   zero();  mac_half(xr, xi, yr, yi): block b += x conj(y[b]) over the sixteen tile rows of a half (this lane's eight);
//   finish();  then re(b, r) / im(b, r) of accumulator register r.        Gram64F32 below, Gram64X3 (x3_common.hpp).
// ------------------------------------------------------------------------------------------------------------
struct Gram64F32 {               // v_mfma_f32_32x32x2_f32, three-multiplication product
    CAcc32<true> C[2];
    __device__ __forceinline__ void zero() { C[0].zero(); C[1].zero(); }
    __device__ __forceinline__ void mac_half(const float (&xr)[8], const float (&xi)[8], const float (&yr)[2][8], const float (&yi)[2][8]) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
#pragma unroll
            for (int b = 0; b < 2; ++b) C[b].mac_conj(xr[q], xi[q], yr[b][q], yi[b][q]);       // out[i][j] += x[i] * conj(y[j])
        }
    }
    __device__ __forceinline__ void finish() { C[0].finish_conj(); C[1].finish_conj(); }
    __device__ __forceinline__ float re(int b, int r) const { return C[b].a[r]; }
    __device__ __forceinline__ float im(int b, int r) const { return C[b].b[r]; }
};
template <class Product>
__device__ __forceinline__ void gram64_body(const GramItem* __restrict__ items, int nitems, char* smem) {
    constexpr int TR = 64, TRP = TR + 4, NU = 8;
    float* const Xr = reinterpret_cast<float*>(smem);
    float* const Xi = Xr + 64 * TRP;
    float* const Yr = Xi + 64 * TRP;
    float* const Yi = Yr + 64 * TRP;
    const int tid = threadIdx.x;
    const int gc = blockIdx.x;
    const int lo = find_item(items, nitems, &GramItem::chunk_begin, gc);
    const GramItem it = items[lo];
    const int lc = gc - it.chunk_begin;
    const int D = it.D, K = it.K, TA = it.TA, TB = it.TB, KK = D * K;
    const long long PA = it.PA;
    const bool same = (it.X == it.Y);
    const cf* __restrict__ Xg = reinterpret_cast<const cf*>(it.X);
    const cf* __restrict__ Yg = reinterpret_cast<const cf*>(it.Y);
    const int ntiles = it.nta * it.ntb;
    const int t_begin = lc * it.tiles_per_chunk;
    const int t_end = min(ntiles, t_begin + it.tiles_per_chunk);
    const int lane = tid & 63, w = tid >> 6, ln = lane & 31, h = lane >> 5;
    const int a = w & 1, rh = w >> 1;
    Product C; C.zero();
    for (int e = tid; e < 64 * TRP; e += 256) { Xr[e] = 0.f; Xi[e] = 0.f; Yr[e] = 0.f; Yi[e] = 0.f; }
    const TileMap m = make_map(tid, D, TA, TB, PA, K);
    const long long kstride = (long long)D * PA;
    const bool fast = m.U <= 256 && (K + m.KP - 1) / m.KP <= NU;
    v4f px[NU], py[NU];
    auto tile_origin = [&](int t, int& a0, int& b0, int& na, int& nb) {
        int ta = t % it.nta, tb = t / it.nta;
        a0 = ta * TA; b0 = tb * TB; na = min(TA, it.PA - a0); nb = min(TB, it.PB - b0);
    };
    // full tiles of the usual shape (every thread owns NU two-element units): straight-line loads.  The guarded path below compiles
    // into one branch per load with an s_waitcnt vmcnt(0) in front of the next one, i.e. the NU loads of a tile are SERIALISED (seen in the
    // ISA; a 64-row tile then costs NU memory latencies, ~10 us instead of the 3.4 us of its matrix work)
    const bool straight = fast && m.active && m.vec == 2 && K == m.KP * NU;
    auto issue_loads = [&](int t) {
        int a0, b0, na, nb; tile_origin(t, a0, b0, na, nb);
        const long long org = (long long)D * (a0 + PA * (long long)K * b0);
        if (straight && na == TA && nb == TB) {
            const cf* px0 = Xg + org + m.off + kstride * m.kp; const cf* py0 = Yg + org + m.off + kstride * m.kp;
            const long long st = kstride * m.KP;
            if (same) {
#pragma unroll
                for (int j = 0; j < NU; ++j) { px[j] = ldg4(px0 + st * j); py[j] = px[j]; }
            } else {
#pragma unroll
                for (int j = 0; j < NU; ++j) { px[j] = ldg4(px0 + st * j); py[j] = ldg4(py0 + st * j); }
            }
            return;
        }
        const bool v0 = m.active && m.al < na && m.bl < nb, v1 = v0 && m.al1 < na;
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            int k = m.kp + m.KP * j;
            v4f vx, vy; vx[0] = vx[1] = vx[2] = vx[3] = 0.f; vy = vx;
            if (k < K && v0) {
                const long long o = org + m.off + kstride * k;
                if (m.vec == 2 && v1) { vx = ldg4(Xg + o); vy = same ? vx : ldg4(Yg + o); }
                else { cf x = ldgc(Xg + o); vx[0] = x.re; vx[1] = x.im; if (same) vy = vx; else { cf y = ldgc(Yg + o); vy[0] = y.re; vy[1] = y.im; } }
            }
            px[j] = vx; py[j] = vy;
        }
    };
    auto commit_loads = [&]() {                  // invalid cells were loaded as zeros, so edge tiles need no extra clearing
        if (!m.active) return;
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            int k = m.kp + m.KP * j;
            if (k < K) {
                int o0 = (m.c0 + D * k) * TRP + m.row0;
                Xr[o0] = px[j][0]; Xi[o0] = px[j][1]; Yr[o0] = py[j][0]; Yi[o0] = py[j][1];
                if (m.vec == 2) { int o1 = (m.c1 + D * k) * TRP + m.row1; Xr[o1] = px[j][2]; Xi[o1] = px[j][3]; Yr[o1] = py[j][2]; Yi[o1] = py[j][3]; }
            }
        }
    };
    if (fast && t_begin < t_end) issue_loads(t_begin);
    for (int t = t_begin; t < t_end; ++t) {
        lds_barrier();
        if (fast) commit_loads();
        else {
            int a0, b0, na, nb; tile_origin(t, a0, b0, na, nb);
            const int ntile_el = D * TA * K * TB;
            for (int e = tid; e < ntile_el; e += 256) {
                int s = e % D; int r1 = e / D; int al = r1 % TA; int r2 = r1 / TA; int k = r2 % K; int bl = r2 / K;
                cf vx, vy; vx.re = vx.im = vy.re = vy.im = 0.f;
                if (al < na && bl < nb) {
                    long long off = s + D * ((long long)(a0 + al) + PA * ((long long)k + (long long)K * (b0 + bl)));
                    vx = Xg[off]; vy = same ? vx : Yg[off];
                }
                int o = (s + D * k) * TRP + (al + TA * bl);
                Xr[o] = vx.re; Xi[o] = vx.im; Yr[o] = vy.re; Yi[o] = vy.im;
            }
        }
        lds_barrier();
        if (fast && t + 1 < t_end) issue_loads(t + 1);
        // rows 32 rh .. 32 rh + 31 in two halves of 16 (lane half h takes 8 of them): bounds the operand registers
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const int r0 = 32 * rh + 16 * hf + 8 * h;
            float xr[8], xi[8], yr[2][8], yi[2][8];
            {
                const int ro = (32 * a + ln) * TRP + r0;
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    v4f t0 = *reinterpret_cast<const v4f*>(Xr + ro + 4 * q), t1 = *reinterpret_cast<const v4f*>(Xi + ro + 4 * q);
#pragma unroll
                    for (int c = 0; c < 4; ++c) { xr[4 * q + c] = t0[c]; xi[4 * q + c] = t1[c]; }
                }
            }
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int ro = (32 * b + ln) * TRP + r0;
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    v4f t2 = *reinterpret_cast<const v4f*>(Yr + ro + 4 * q), t3 = *reinterpret_cast<const v4f*>(Yi + ro + 4 * q);
#pragma unroll
                    for (int c = 0; c < 4; ++c) { yr[b][4 * q + c] = t2[c]; yi[b][4 * q + c] = t3[c]; }
                }
            }
            C.mac_half(xr, xi, yr, yi);
        }
    }
    // one partial per chunk: the two row halves (waves w, w + 2) are summed through the free tile buffers
    lds_barrier();
    C.finish();
    v2f* const R = reinterpret_cast<v2f*>(smem);                // [rh][j][i], pitch 65: 2 * 64 * 65 * 8 B = 66.5 KB
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = 32 * a + (r & 3) + 8 * (r >> 2) + 4 * h, j = 32 * b + ln;
            v2f v = {C.re(b, r), C.im(b, r)};
            R[(rh * 64 + j) * 65 + i] = v;
        }
    lds_barrier();
    cf* __restrict__ part = reinterpret_cast<cf*>(it.partial) + (size_t)lc * KK * KK;
    for (int e = tid; e < KK * KK; e += 256) {
        const int i = e % KK, j = e / KK;
        const v2f u = R[j * 65 + i], v = R[(64 + j) * 65 + i];
        cf o; o.re = u[0] + v[0]; o.im = u[1] + v[1]; part[e] = o;
    }
}

// ------------------------------------------------------------------------------------------------------------
// pieces of the f64 Gram kernels (mfma_gram64_f64_kernel, mfma_gram128_f64_kernel, mfma_gauge_gram64_kernel; tile layout and the three
// accumulators (cr, ci, cc) per 16 x 16 block as for gram_f64_shared above).  G is Hermitian: only the blocks (I, J >= I) are computed.
// ------------------------------------------------------------------------------------------------------------
// one k-step of  out[i][j] += a[i] conj(b[j])  in three multiplications
__device__ __forceinline__ void gram_f64_mac3(double ar, double ai, double br, double bi, v4d& cr, v4d& ci, v4d& cc) {
    cr = __builtin_amdgcn_mfma_f64_16x16x4f64(ar + ai, br, cr, 0, 0, 0);
    ci = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, br - bi, ci, 0, 0, 0);
    cc = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, bi + br, cc, 0, 0, 0);
}
// block (I, J) on its own over the 64 rows of a tile: lane quarter kq takes rows 16 kq .. + 15, in two halves of 8 to bound registers
__device__ __forceinline__ void gram_f64_block(const float* __restrict__ Xr, const float* __restrict__ Xi, int TRP, int l15, int kq, int I, int J,
                                               v4d& cr, v4d& ci, v4d& cc) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int ro = (16 * I + l15) * TRP + 16 * kq + 8 * half;
        const int rb = (16 * J + l15) * TRP + 16 * kq + 8 * half;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const v4f t0 = *reinterpret_cast<const v4f*>(Xr + ro + 4 * q), t1 = *reinterpret_cast<const v4f*>(Xi + ro + 4 * q);
            const v4f u0 = *reinterpret_cast<const v4f*>(Xr + rb + 4 * q), u1 = *reinterpret_cast<const v4f*>(Xi + rb + 4 * q);
#pragma unroll
            for (int c = 0; c < 4; ++c) gram_f64_mac3((double)t0[c], (double)t1[c], (double)u0[c], (double)u1[c], cr, ci, cc);
        }
    }
}
// block (I, J) of a KK x KK partial and its mirror; FULL: KK is a multiple of 16, nothing to guard
template <bool FULL>
__device__ __forceinline__ void gram_f64_store(cx<double>* __restrict__ part, int KK, int l15, int kq, int I, int J, const v4d& cr, const v4d& ci, const v4d& cc) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = 16 * I + kq + 4 * r, j = 16 * J + l15;
        if (FULL || (i < KK && j < KK)) {
            cx<double> v; v.re = cr[r] - ci[r]; v.im = cr[r] - cc[r]; part[i + (size_t)KK * j] = v;
            if (I != J) { cx<double> c; c.re = v.re; c.im = -v.im; part[j + (size_t)KK * i] = c; }     // G[j][i] = conj(G[i][j])
        }
    }
}
// the upper-triangle blocks of nb panels in row-major order: block idx -> (I, J)
__device__ __forceinline__ void gram_block_of(int nb, int idx, int& I, int& J) { I = 0; int rem = idx; while (rem >= nb - I) { rem -= nb - I; ++I; } J = I + rem; }

// A wave of the 64 x 64 f64 Gram: waves 0, 1 own three blocks on even tiles (set A) and two on odd tiles (set B), waves 2, 3 the other way
// round, so every wave (= SIMD) does 5 blocks per two tiles; the two tile parities accumulate into separate partials (2 per chunk) because
// a block changes wave with the parity.  deal(): blocks round-robin, forwards on one parity and backwards on the other.  deal_shared(),
// KK = 64 (four panels, ten blocks): sets that share a panel (gram_f64_shared) --
//   even waves: A = {(0,0),(0,1),(0,2)} (rows from panel 0), B = {(1,1),(1,2)} (rows from panel 1)
//   odd waves : A = {(0,3),(1,3),(2,3)} (columns from panel 3), B = {(2,2),(3,3)}
struct Gram64F64Wave {
    int w, parA;                                               // parA: tile parity on which this wave uses set A
    int aI[3], aJ[3], bI[2], bJ[2]; bool aOn[3], bOn[2];
    v4d CAr[3], CAi[3], CAc[3], CBr[2], CBi[2], CBc[2];
    __device__ __forceinline__ explicit Gram64F64Wave(int w_) : w(w_), parA((w_ < 2) ? 0 : 1) {}
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) { CAr[j][r] = 0.0; CAi[j][r] = 0.0; CAc[j][r] = 0.0; }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) { CBr[j][r] = 0.0; CBi[j][r] = 0.0; CBc[j][r] = 0.0; }
    }
    __device__ __forceinline__ void deal(int KK) {
        const int nb = (KK + 15) >> 4, nblk = nb * (nb + 1) / 2;
#pragma unroll
        for (int q = 0; q < 3; ++q) { const int wv = parA ? 3 - w : w; int idx = wv + 4 * q; aOn[q] = idx < nblk; gram_block_of(nb, aOn[q] ? idx : 0, aI[q], aJ[q]); }
#pragma unroll
        for (int q = 0; q < 2; ++q) { const int wv = parA ? w : 3 - w; int idx = wv + 4 * q; bOn[q] = idx < nblk; gram_block_of(nb, bOn[q] ? idx : 0, bI[q], bJ[q]); }
    }
    __device__ __forceinline__ void deal_shared() {
#pragma unroll
        for (int q = 0; q < 3; ++q) { aOn[q] = true; aI[q] = (w & 1) ? q : 0; aJ[q] = (w & 1) ? 3 : q; }
        bOn[0] = bOn[1] = true;
        bI[0] = (w & 1) ? 2 : 1; bJ[0] = (w & 1) ? 2 : 1; bI[1] = (w & 1) ? 3 : 1; bJ[1] = (w & 1) ? 3 : 2;
    }
    // one tile (parity = its index in the chunk & 1) of the sets of deal_shared()
    __device__ __forceinline__ void tile_shared(const float* __restrict__ Xr, const float* __restrict__ Xi, int TRP, int l15, int kq, int parity) {
        if (parity == parA) {                                  // wave-uniform
            const int q3[3] = {0, 1, 2};
            if (w & 1) gram_f64_shared<3, false, -1>(Xr, Xi, TRP, l15, kq, 3, q3, CAr, CAi, CAc);
            else       gram_f64_shared<3, true, 0>(Xr, Xi, TRP, l15, kq, 0, q3, CAr, CAi, CAc);
        } else if (w & 1) {
            const int q2[1] = {2}, q3b[1] = {3};
#pragma unroll
            for (int b = 0; b < 2; ++b) {                      // two diagonal blocks, each on its own panel (register copies, no address taken)
                v4d r1[1] = {CBr[b]}, i1[1] = {CBi[b]}, c1[1] = {CBc[b]};
                if (b == 0) gram_f64_shared<1, true, 0>(Xr, Xi, TRP, l15, kq, 2, q2, r1, i1, c1);
                else        gram_f64_shared<1, true, 0>(Xr, Xi, TRP, l15, kq, 3, q3b, r1, i1, c1);
                CBr[b] = r1[0]; CBi[b] = i1[0]; CBc[b] = c1[0];
            }
        } else {
            const int q12[2] = {1, 2};
            gram_f64_shared<2, true, 0>(Xr, Xi, TRP, l15, kq, 1, q12, CBr, CBi, CBc);
        }
    }
    // one tile of the blocks of deal()
    __device__ __forceinline__ void tile_blocks(const float* __restrict__ Xr, const float* __restrict__ Xi, int TRP, int l15, int kq, int parity) {
        if (parity == parA) {                                  // wave-uniform
#pragma unroll
            for (int q = 0; q < 3; ++q) if (aOn[q]) gram_f64_block(Xr, Xi, TRP, l15, kq, aI[q], aJ[q], CAr[q], CAi[q], CAc[q]);
        } else {
#pragma unroll
            for (int q = 0; q < 2; ++q) if (bOn[q]) gram_f64_block(Xr, Xi, TRP, l15, kq, bI[q], bJ[q], CBr[q], CBi[q], CBc[q]);
        }
    }
    // partial 2 lc + p of the item collects the blocks accumulated on tiles of parity p (each block exactly once per parity)
    template <bool FULL> __device__ __forceinline__ void store(void* partial, int lc, int KK, int l15, int kq) const {
        cx<double>* __restrict__ partA = reinterpret_cast<cx<double>*>(partial) + (size_t)(2 * lc + parA) * KK * KK;
        cx<double>* __restrict__ partB = reinterpret_cast<cx<double>*>(partial) + (size_t)(2 * lc + (parA ^ 1)) * KK * KK;
#pragma unroll
        for (int q = 0; q < 3; ++q) if (aOn[q]) gram_f64_store<FULL>(partA, KK, l15, kq, aI[q], aJ[q], CAr[q], CAi[q], CAc[q]);
#pragma unroll
        for (int q = 0; q < 2; ++q) if (bOn[q]) gram_f64_store<FULL>(partB, KK, l15, kq, bI[q], bJ[q], CBr[q], CBi[q], CBc[q]);
    }
};

}  // namespace tnqs
