// engine_internal.hpp -- declarations shared by the translation units of the host engine:
//   engine_core.cpp   pool, graph, state container, tensor / message I/O
//   engine_batch.cpp  batched building blocks: fiber GEMM passes (FiberPass), mode-product chains, Gram jobs, the SVD batch
//   fiber_plan.cpp    which fiber GEMM kernel a pass launches and its layout (FiberRoute, plan_fiber_pass; host code, no device call)
//   bp_schedule.cpp   BP sweep order: default sequence, forest-cover sequence, level schedule (BPPlan; host graph code, no device call)
//   engine_bp.cpp     BP update: sweep driver (BpUpdate), the launches of one level (BpLevelBatch), products kept across levels (ProdCache)
//   gate_schedule.cpp apply_gates: validation of the gate list, the step schedule (GateSchedule; host code, no device call)
//   engine_runahead.cpp  deferred verification: checks, snapshots, the driver that runs a GateSchedule ahead of the device (RunAhead)
//   engine_gates.cpp  apply_gates, one- and two-site gate batches, truncate
//   gate_theta.cpp    the theta phase of a gate batch: route rule (theta_route; no device call), launch chain, small-SVD and second-pass items
//   engine_obs.cpp    observables, BP scalars / rescale, symmetric gauge
//   engine_sample.cpp site probabilities, projection, the sample(alg = "bp") loop
//   engine_loops.cpp  loop corrections: transfer matrices of simple cycles, ring products, traces (batched)
//   engine_configs.cpp  loop corrections: configurations with two independent loops (theta, dumbbell, figure-eight): decomposition, branch Grams, chain products
//   engine_rdm.cpp    two-site reduced density matrices of bonds (batched chains + Grams, one contraction kernel)
//   engine_paths.cpp  two-site reduced density matrices of the ends of paths (environments, transfer matrices, the sweep along the path)
//   engine_inner.cpp  overlap of two states: BP on the bilinear form (rectangular messages, mode products that change a leg's dimension, form scalars)
//   engine_amp.cpp    amplitudes of a batch of bitstrings: BP on the single-layer network T_v[x_v] (vector messages per string, groups of strings per site value)
//   engine_spectra.cpp  entanglement spectra of bonds from the two messages (batched eigen problems, one read-back)
//   engine_bmps.cpp   boundary MPS on open rectangular grids: partition plan, the fitting update of the interpartition messages, measurement and norm
//   sharding.cpp      exchange step (RCCL or host callback)
//   api.cpp           the extern "C" boundary of include/tnqs.h (api_guard.hpp: the exception guard every entry point runs in)
//   debug_*.cpp       the kernel-level test entry points of include/tnqs_debug.h, one file per kernel family: svd, fiber, plane, bp, gate, obs, sample, bmps (debug_util.hpp)
// and the kernel translation units behind kernels.hpp (device vocabulary: device_common.hpp, with the complex 16x16x4 matrix-core product CMfma16 / cmac16 and the
// split-plane multiply phase cplane_mm16 that kernels_inner.hip and kernels_bmps.hip share; MFMA tile machinery: mfma_common.hpp, x3_common.hpp):
//   kernels.hip        generic fiber GEMM, Gram, Gram route, reduce      kernels_mfma.hip   chi = 32 matrix-core mode products / Grams
//   kernels_bp.hip     message epilogue, small-site message, rescale,    kernels_x3.hip     the same on the bf16 matrix cores (three-way split)
//                      edge scalars, symmetric gauge                     kernels_plane.hip  16-dimensional planes (chi = 16)
//   kernels_svd.hip    Jacobi (global / LDS), preconditioned theta SVD,  kernels_chi64.hip  chi = 64 family
//                      V recovery, small-SVD prepare / finish            kernels_gate.hip   fused gauge + f64 Gram of the gate path
//   kernels_chol.hip   Cholesky (square / packed), env prepare / finish  kernels_f64.hip    ComplexF64 on the f64 matrix cores
//   kernels_theta.hip  per-gate small algebra: gate_eigs .. gate_finish  kernels_sample.hip sampling
//   kernels_util.hip   diag, norm factor, scale, pack, permute, fills       kernels_loop.hip   loop corrections: batched complex GEMM and branch Gram (one tile body), antiprojector, trace, dot
//   kernels_rdm.hip    bond contraction of two Gram partials (edge RDMs), environment through a transfer matrix (path RDMs)
//   kernels_inner.hip  overlap of two states: rectangular two-operand Gram (f32 / f64 matrix cores), bilinear message epilogue, form scalars
//   kernels_amp.hip    bitstring amplitudes: strided-slice GEMM over groups of strings (f32 / f64 matrix cores), per-string vector absorption, epilogue, scalars
//   kernels_spectrum.hip  bond entanglement spectra: W = D V^dagger m1^T V D from a message's eigen factorisation, signed sorted spectrum
//   kernels_bmps.hip   boundary MPS: batched complex contraction over strided leg groups (f32 / f64 matrix cores), chunk reduction, thin Householder QR, norm / scale / conjugate
#pragma once
#include "engine.hpp"
#include "kernels.hpp"
#include <algorithm>
#include <array>
#include <chrono>
#include <climits>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <memory>
#include <mutex>
#include <numeric>
#include <set>
#include <type_traits>
#include <unordered_map>

namespace tnqs {

#define HIPCHK(x) hipchk((x), #x)

// ---- environment switches (all default off; read once per process).  ONE alternative route per kernel family (round 6: the table had grown to ~45 switches,
// most of them A/B levers of decisions that are long made -- each one a route that had to stay correct): they serve the route-equivalence tests
// (tests/test_gpu_toggles.py) and the A/B legs of bench.py; nothing else steers the hot path. ------------------------------------------------------------
inline bool envflag(const char* name) { const char* e = std::getenv(name); return e && e[0] == '1'; }
#define TNQS_SWITCH(fn, expr) inline bool fn() { static const bool v = (expr); return v; }
TNQS_SWITCH(use_mfma, !envflag("TNQS_NO_MFMA"))                  // no matrix-core kernel at all: the generic tiled kernels (kernels.hip), any dims / element type
TNQS_SWITCH(use_pair, !envflag("TNQS_NO_PAIR"))                  // no plane kernels (two legs per pass, pair-Gram, chi = 16 / 32): single-leg matrix-core products
TNQS_SWITCH(use_bra_products, !envflag("TNQS_NO_BRA_PRODUCTS"))  // BP: every message absorbed on the ket side (engine_bp.cpp: sites of degree >= 6 absorb half of them on the bra side)
TNQS_SWITCH(use_prodcache, !envflag("TNQS_NO_PRODCACHE"))        // BP: no partial product kept from one level to the next (engine_bp.cpp ProdCache)
TNQS_SWITCH(use_chol, !envflag("TNQS_NO_CHOL"))                  // R factor from the eigen factorisation of the Gram matrix instead of Cholesky (the route a collapsed pivot falls back to)
TNQS_SWITCH(use_qr2, !envflag("TNQS_NO_QR2"))                    // ComplexF64: no second factorisation pass
TNQS_SWITCH(use_lowrank, !envflag("TNQS_NO_LOWRANK"))            // theta SVD on the full theta instead of the low-rank factor (the route a refused pivot falls back to)
TNQS_SWITCH(use_precond_svd, !envflag("TNQS_NO_PRECOND_SVD"))    // low-rank theta SVD on the plain LDS Jacobi instead of the preconditioned one-kernel route (kernels_svd.hip theta_svd_pre_kernel)
TNQS_SWITCH(use_small_svd, !envflag("TNQS_NO_SMALLSVD"))         // sites with fewer fibers than columns: Gram + eigen instead of the direct SVD
TNQS_SWITCH(defer_site1, !envflag("TNQS_NO_DEFER_1SITE"))        // unitary one-site gates are applied in a pass of their own instead of being carried to the next two-site gate
TNQS_SWITCH(use_chi64, !envflag("TNQS_NO_CHI64"))                // the chi = 64 kernel family (kernels_chi64.hip: register-direct fiber GEMM, 64 x 64 / 128 x 128 Grams, packed Cholesky, Cholesky-QR theta SVD)
TNQS_SWITCH(speculation_on, !envflag("TNQS_NO_SPECULATION"))     // apply_gates never runs ahead of the device: every batch reads its results back, every BP update waits for its verdict
#undef TNQS_SWITCH
// TNQS_NO_BF16X3=1 (launch_util.hpp): the chi = 32 / 64 plane kernels on v_mfma_f32_32x32x2_f32 instead of the bf16 matrix cores with exact three-way operand splits
//                   (kernels_x3.hip; bench.py's A/B leg);
// TNQS_NO_SMALL_SITE_BP=1 (engine_bp.cpp): sites of at most 8192 elements take the generic chain + Gram route instead of the one-kernel LDS-resident message;
// TNQS_JACOBI_GLOBAL=1: every Jacobi factorisation in the global-memory kernel (the route matrices beyond the LDS take);
// tunables: TNQS_ARENA_KB (pinned staging arena; tests of its overflow path), TNQS_BP_WS_MB (workspace bound of a BP sub-batch), TNQS_BP_CACHE_MB, TNQS_RCCL_LIB (sharding.cpp),
//           TNQS_FORCE_EXCHANGE (a one-rank RCCL handle takes the sharded path); diagnostics: TNQS_HOST_TIMING, TNQS_DEBUG_SWEEPS.
// The kernel-level entry points of include/tnqs_debug.h (debug_*.cpp) read TNQS_DBG_* themselves and are not part of the hot path.
// TNQS_BP_CACHE_MB: bound on the partial products kept across BP levels (MiB, default 49152)
inline size_t bp_cache_budget() { static const size_t v = [] { const char* e = std::getenv("TNQS_BP_CACHE_MB"); return (e ? (size_t)std::atoll(e) : (size_t)49152) << 20; }(); return v; }
inline size_t bp_ws_budget() { static const size_t v = [] { const char* e = std::getenv("TNQS_BP_WS_MB"); return (e ? (size_t)std::atoll(e) : (size_t)24576) << 20; }(); return v; }
inline size_t jacobi_lds(size_t bytes) { static const bool g = envflag("TNQS_JACOBI_GLOBAL"); return (g || bytes > 160 * 1024 - 2048) ? 0 : bytes; }
inline int mmax_of(const std::vector<JacobiItem>& ji) { int m = 1; for (auto& j : ji) m = std::max(m, std::max(j.m, j.n)); return m; }

// optional host-side phase timing (TNQS_HOST_TIMING=1): printed when the process exits
struct HostTimer {
    static double acc[16]; static long cnt[16];
    int k; std::chrono::steady_clock::time_point t0; bool on;
    explicit HostTimer(int kk) : k(kk), t0(std::chrono::steady_clock::now()), on(true) {}
    void stop() { if (on) { static std::mutex mu; std::lock_guard<std::mutex> lk(mu); acc[k] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); cnt[k]++; on = false; } }
    ~HostTimer() { stop(); }
};

void sync(State* s);                                   // stream synchronise + release of the batch's descriptor buffers
hipStream_t aux_stream_of(State* s);                  // the State's side stream (+ its events), created on first use / recycled with the State
void recycle_arena(HostArena ar);                     // back to the free list (nothing on the device may still read it)
HostArena acquire_arena();                             // a recycled or freshly pinned 32 MiB arena (engine_core.cpp)
// The staging arena is about to be reused from its start: everything that may still read it must have run -- on the current stream and on the other
// stream this State enqueues on (the side stream of the early small-SVD launches and of the BP levels' boundary sites)
inline void drain_for_arena_reuse(State* s) {
    HIPCHK(hipStreamSynchronize(s->stream));
    if (s->aux_stream && s->aux_stream != s->stream) HIPCHK(hipStreamSynchronize(s->aux_stream));
}
// Read-back through the pinned staging arena: the copy is enqueued and the staged host pointer returned; it holds the data once the stream
// has been synchronised (a read-back into pageable memory is staged by the runtime and BLOCKS per call).  The staged bytes stay valid until the
// next upload() / readback() after a sync(s) reuses the arena.
template <class X> const X* readback(State* s, const void* dsrc, size_t count) {
    const size_t bytes = count * sizeof(X);
    HostArena& ar = s->arena;
    if (!ar.base) ar = acquire_arena();
    const size_t aligned = (std::max<size_t>(bytes, 1) + 255) & ~size_t(255);
    if (aligned > ar.cap) throw Err(TNQS_ERR_UNSUPPORTED, "read-back too large for the staging arena");
    if (ar.off + aligned > ar.cap) { drain_for_arena_reuse(s); ar.off = 0; }     // pending uploads have been copied: the host side is free
    char* h = ar.base + ar.off; ar.off += aligned;
    if (bytes) HIPCHK(hipMemcpyAsync(h, dsrc, bytes, hipMemcpyDeviceToHost, s->stream));
    return reinterpret_cast<const X*>(h);
}
// room for `bytes` of staged read-backs without a wrap in between (several read-backs that are consumed after one synchronisation)
inline void reserve_readback(State* s, size_t bytes) {
    HostArena& ar = s->arena;
    if (!ar.base) ar = acquire_arena();
    if (bytes > ar.cap) throw Err(TNQS_ERR_UNSUPPORTED, "read-backs of one batch too large for the staging arena");
    if (ar.off + bytes > ar.cap) { drain_for_arena_reuse(s); ar.off = 0; }
}
// End of a phase WITHOUT draining the stream: everything in the keep-alive list so far may go once the stream has been synchronised for some
// other reason (the next read-back), so the host can start preparing the next phase while this one's last kernels still run.
inline void soft_sync(State* s) { s->keep_mark = s->keepalive.size(); }
// after a raw hipStreamSynchronize(s->stream): release what soft_sync() marked (later entries belong to the phase in progress)
inline void drained(State* s) {
    s->prof->chain = false;                    // the host waited: the next profiled scope records its own start event
    s->arena.off = 0;                          // every staged upload has been copied; staged read-backs are consumed by the caller before its next upload
    if (s->keep_mark) { s->keepalive.erase(s->keepalive.begin(), s->keepalive.begin() + (std::ptrdiff_t)std::min(s->keep_mark, s->keepalive.size())); s->keep_mark = 0; }
}
void materialize_scale(State* s, const std::vector<int>& verts);
void materialize_scale_all(State* s);
void materialize_pending(State* s, const std::vector<int>& verts);      // apply the pending one-site gates of these vertices (State::pend1)
void materialize_pending_all(State* s);
inline Buf dalloc(State* s, size_t bytes) {
    auto b = std::make_shared<DevBuf>();
    b->pool = s->pool; b->bytes = bytes;
    b->p = s->pool->alloc(bytes ? bytes : 1, &b->rounded);
    return b;
}
// descriptor upload through the handle's pinned staging arena (reset at host sync points)
template <class Item> const Item* upload(State* s, const std::vector<Item>& v) {
    if (v.empty()) return nullptr;
    size_t bytes = v.size() * sizeof(Item);
    HostArena& ar = s->arena;
    if (!ar.base) ar = acquire_arena();
    size_t aligned = (bytes + 255) & ~size_t(255);
    if (aligned > ar.cap) throw Err(TNQS_ERR_UNSUPPORTED, "descriptor batch too large");
    // arena full: wait for the copies that still read it and start over.  ONLY the host staging is recycled here -- the device buffers of
    // earlier uploads (descriptor arrays whose kernels are not launched yet) stay in the keep-alive list: a sync(s) at this point would hand
    // them back to the pool in the middle of a phase and the next dalloc of the same size class could alias them
    if (ar.off + aligned > ar.cap) { drain_for_arena_reuse(s); ar.off = 0; s->prof->chain = false; }
    char* h = ar.base + ar.off; ar.off += aligned;
    std::memcpy(h, v.data(), bytes);
    Buf b = dalloc(s, bytes);
    HIPCHK(hipMemcpyAsync(b->p, h, bytes, hipMemcpyHostToDevice, s->stream));
    s->keepalive.push_back(b);
    return reinterpret_cast<const Item*>(b->p);
}

// The same for the descriptor arrays of the ONE-WORKGROUP-PER-ITEM kernels (items[blockIdx.x]: env / Cholesky / theta / Jacobi / finish / diag ...):
// no copy at all -- the kernel reads its item straight from the pinned arena (hipHostMalloc memory is mapped into the device's address space under the
// same pointer).  A dependent chain of 20-60 us kernels paid ~5 us of stream time and ~8 us of host time per descriptor copy (two dozen per gate
// batch); a workgroup's single ~100-byte read over the host link costs it 1-2 us.  NOT for kernels that binary-search their item list per workgroup
// (the tensor passes, reduce) or re-read the data in inner loops (gate matrices).  The bytes stay valid until the arena is reset, which only
// happens after the stream has been synchronised (drained / sync / wrap below) -- by then every kernel that reads them has run.  Hence: only for
// arrays whose kernels are ALL launched before the next host synchronisation of the phase (the GateItem array of a batch is read again after the
// read-back of the ranks in the two-trip flow: it keeps its device copy).
inline const void* upload_small_bytes(State* s, const void* p, size_t bytes) {
    HostArena& ar = s->arena;
    if (!ar.base) ar = acquire_arena();
    const size_t aligned = (bytes + 255) & ~size_t(255);
    if (aligned > ar.cap) throw Err(TNQS_ERR_UNSUPPORTED, "descriptor batch too large");
    if (ar.off + aligned > ar.cap) { drain_for_arena_reuse(s); ar.off = 0; s->prof->chain = false; }
    char* h = ar.base + ar.off; ar.off += aligned;
    std::memcpy(h, p, bytes);
    return h;
}
template <class Item> const Item* upload_small(State* s, const std::vector<Item>& v) {
    return v.empty() ? nullptr : static_cast<const Item*>(upload_small_bytes(s, v.data(), v.size() * sizeof(Item)));
}

struct ProfScope {
    State* s; int cls; hipEvent_t a = nullptr, b = nullptr; bool own_a = true;
    ProfScope(State* st, int c, double bytes, double flops) : s(st), cls(c) {
        Prof& P = *s->prof;
        if (!P.on) return;
        P.cls[c].bytes += bytes; P.cls[c].flops += flops; P.cls[c].launches += 1;
        auto get = [&]() { hipEvent_t e; if (!P.ev_free.empty()) { e = P.ev_free.back(); P.ev_free.pop_back(); } else HIPCHK(hipEventCreate(&e)); return e; };
        if (P.chain && P.last_b && P.last_stream == s->stream) { a = P.last_b; own_a = false; }
        else { a = get(); own_a = true; HIPCHK(hipEventRecord(a, s->stream)); }
        b = get();
    }
    ~ProfScope() {
        if (!a) return;
        Prof& P = *s->prof;
        (void)hipEventRecord(b, s->stream);
        P.pending.push_back({cls, a, b, own_a});
        P.last_b = b; P.chain = true; P.last_stream = s->stream;
    }
};

// a whole phase on the handle's stream (TNQS_PROF_PHASE_*): own events, outside the chaining of the kernel-class scopes; `count` is added to the class's launches
struct PhaseScope {
    State* s; int cls; hipEvent_t a = nullptr, b = nullptr; long count = 1;
    PhaseScope(State* st, int c) : s(st), cls(c) {
        Prof& P = *s->prof;
        if (!P.on) return;
        auto get = [&]() { hipEvent_t e; if (!P.ev_free.empty()) { e = P.ev_free.back(); P.ev_free.pop_back(); } else HIPCHK(hipEventCreate(&e)); return e; };
        a = get(); b = get();
        HIPCHK(hipEventRecord(a, s->stream));
    }
    ~PhaseScope() {
        if (!a) return;
        Prof& P = *s->prof;
        (void)hipEventRecord(b, s->stream);
        P.cls[cls].launches += count;
        P.pending.push_back({cls, a, b, true});
    }
};

// bond dimensions of a site's legs without a heap allocation for degrees up to 8 (site_dims is called several times per message and per gate on the host:
// on the latency-bound lattices the allocations were a measurable share of the BP preparation)
struct ChiVec {
    int inl[8]; int n = 0; std::vector<int> big;          // big: only when the degree exceeds 8
    void push_back(int c) { if (n < 8 && big.empty()) inl[n++] = c; else { if (big.empty()) big.assign(inl, inl + n); big.push_back(c); ++n; } }
    int* data() { return big.empty() ? inl : big.data(); }
    const int* data() const { return big.empty() ? inl : big.data(); }
    int& operator[](size_t i) { return data()[i]; }
    const int& operator[](size_t i) const { return data()[i]; }
    size_t size() const { return (size_t)n; }
    bool empty() const { return n == 0; }
    const int* begin() const { return data(); }
    const int* end() const { return data() + n; }
};
struct SD {       // dims of a site tensor in canonical layout
    int z = 0, d = 1; ChiVec chi; size_t n = 1;
    size_t pre(int j) const { size_t p = d; for (int i = 0; i < j; ++i) p *= chi[i]; return p; }
    size_t post(int j) const { size_t p = 1; for (int i = j + 1; i < z; ++i) p *= chi[i]; return p; }
};
inline SD site_dims(const State* s, int v) {
    SD r; const Graph& g = *s->g;
    r.z = (int)g.nbr[v].size(); r.d = s->d[v]; r.n = r.d;
    for (int j = 0; j < r.z; ++j) { int c = s->chi[g.nbr_e[v][j]]; r.chi.push_back(c); r.n *= c; }
    return r;
}

// number of elements of a site tensor (no allocation: site_dims builds a vector)
inline size_t site_nelem(const State* s, int v) { size_t n = (size_t)s->d[v]; for (int e : s->g->nbr_e[v]) n *= (size_t)s->chi[e]; return n; }
inline size_t round256(size_t b) { return (b + 255) & ~size_t(255); }
// the two-site gate as an operator sum g = sum_k a_k (x) b_k (engine_gates.cpp): returns kappa; fa: kappa x d1^2, fb: kappa x d2^2 numbers, appended
int operator_sum(const double* mat, int d1, int d2, std::vector<std::complex<double>>& fa, std::vector<std::complex<double>>& fb);
void exchange(State* s, size_t bytes_per_rank);                       // sharding.cpp
void check_exchange(const State* s, size_t bytes_per_rank);           // call BEFORE enqueuing anything that writes into s->exch
// host-only helpers of the kernel-level entry points (debug_bp.cpp, debug_gate.cpp): the default BP order as (src, dst) vertex pairs, with the level of every message
// (bp_schedule.cpp), and the graph of a handle without the handle (engine_core.cpp)
void dbg_default_sequence(const Graph& g, std::vector<int>& src, std::vector<int>& dst);
void dbg_default_sequence_graph(const Graph& g, std::vector<int>& src, std::vector<int>& dst, std::vector<int>& level);
std::shared_ptr<Graph> dbg_make_graph(int nv, int ne, const int32_t* es, const int32_t* ed);

// ---- the theta phase of a two-site gate (gate_theta.cpp): TwoSiteBatch (engine_gates.cpp) and the kernel-level entry points (debug_gate.cpp) run the same code --------
// What a gate of operator-Schmidt rank kappa (0: no operator-sum factors) on a bond of dimension chi is offered, and the element counts (complex128) of its low-rank
// workspaces, 0 where one is not handed out: nA = lowA (Mr K), nB = lowB (Nc K); low-rank route: nG = lowG, lowL, lowW each (K K); its preconditioned SVD (ComplexF32):
// nQ = lowQ (Nc K); its second CholeskyQR pass (ComplexF64): nB1 = lowB1 (Nc K), nG2 = lowG2, lowL2, lowLc each (K K).  Host code, no device call; d^2 chi > 512 throws
struct ThetaRoute { int n1, n2, Mr, Nc, cap, K; bool opsum, low, lowq; size_t nA, nB, nG, nQ, nB1, nG2; };
ThetaRoute theta_route(bool F32, int d1, int d2, int chi, int kappa, int maxdim);
struct ThetaLowWs { void *lowW, *lowB1, *lowG2, *lowL2, *lowLc; };      // a low-rank gate's workspaces that no GateItem field names (lowB1 .. lowLc: ComplexF64)
// where the chain's own descriptor arrays go: the engine's pinned arena (upload_small) or a plain device allocation -- a function pointer, no heap traffic per call
struct DescUpload {
    const void* (*fn)(void* ctx, const void* p, size_t bytes); void* ctx;
    template <class Item> const Item* vec(const std::vector<Item>& v) const { return v.empty() ? nullptr : static_cast<const Item*>(fn(ctx, v.data(), v.size() * sizeof(Item))); }
};
// gate_theta -> gate_theta_mm -> lowrank_g -> chol / chol_packed -> lowrank_m (ComplexF64: -> lowrank_bw -> lowrank_g -> chol -> lowrank_ll -> lowrank_m) -> theta_scale over
// the gates of `items` (d_items: their device copy; ws[q]: of gate q, read where items[q].lowG is set).  d_fail1 / d_fail2: one zeroed failure flag per gate for the two
// Cholesky passes.  last_stage: 0 gate_theta, 1 gate_theta_mm, 2 the low-rank block, 3 theta_scale (the engine always runs all of it)
template <class T> void launch_theta_chain(hipStream_t st, const GateItem* d_items, const std::vector<GateItem>& items, const std::vector<ThetaLowWs>& ws,
                                           int* d_fail1, int* d_fail2, DescUpload up, int last_stage = 3);
// R = Sigma U^dagger of a site with fewer fibers than columns, from the SVD of the n x N matricised psi~ (f64; src [d][low][chi_b][hi], n = d chi_b, N = low hi, M: n N
// complex128 of scratch): the two items of the site, appended, and the three dependent launches on `st`
void small_svd_items(const void* src, void* M, void* GA, void* GV, int d, int low, int chi_b, int hi, std::vector<SmallSvdItem>& si, std::vector<JacobiItem>& sji);
template <class T> void launch_small_svd(hipStream_t st, const SmallSvdItem* ds, const JacobiItem* dj, const std::vector<JacobiItem>& sji);
// a site of the second factorisation pass: its first-pass factor (GW, GV, lam, idx, *r kept columns, n x n) and where X1 = R1^+ goes -> the items of qr2_rinv / qr2_compose
struct Qr2Site {
    const void *GW, *GV; const double* lam; const int* idx; const int* r; int n; void* X1;
    Qr2RinvItem rinv() const { return Qr2RinvItem{GW, lam, idx, r, n, X1}; }
    Qr2ComposeItem compose(const void* A2, const void* V2, double tau, void* GVout, void* GWout, int* rk) const { return Qr2ComposeItem{A2, V2, X1, GV, lam, idx, r, n, tau, GVout, GWout, rk}; }
};



// a chain = one site tensor pushed through several mode products (leg j with matrix X_j, chi_j x chi_j)
struct Chain {
    int v = -1; const void* src = nullptr; SD sd;
    const void* y = nullptr;                     // the untouched site tensor when src is a shared partial product of it (BP prefix sharing)
    std::vector<std::pair<int, const void*>> steps;
    const void* result = nullptr; Buf tmp[2];
    bool ordered = false;                        // steps are in the caller's priority order: the two-leg stages take them from the front
    std::vector<std::vector<int>> trail;         // legs absorbed by each pass, in order; pass k wrote tmp[k & 1] (the last two are intact afterwards)
};


struct GramJob {      // out[i,j] = sum X[i,.] conj(Y[j,.]) over everything but the kept index (s and/or leg)
    const void* X; const void* Y; SD sd; int leg;  /* -1: keep the site index only */ bool keep_site;
    Buf partial; int nchunks = 0; int KK = 0;
    const void* M = nullptr;       // fused path: message absorbed on the first row leg inside the Gram kernel
    Buf final_msg;                 // set: the kernel that computed the message normalised and diffed it too (bp_small_site_kernel, matrix-core form): no msg_finalize item
};

// ---- fiber GEMM passes (out = in x_(s,leg) X: mode products, gate epilogue, one-site operators): every call site builds its items with the two helpers
// below and runs them through a FiberPass; which kernel a pass launches is decided in fiber_plan.cpp alone ---------------------------------------------------
// the item of a site tensor contracted over `leg` (keep_site: the site index takes part, D = Do = d) into a leg of dimension No; pointers left to the caller
inline FiberItem site_fiber_item(const SD& sd, int leg, bool keep_site, int No, bool want_norm) {
    FiberItem it{}; it.D = it.Do = keep_site ? sd.d : 1;
    it.PA = (int)(sd.pre(leg) / it.D); it.K = sd.chi[leg]; it.PB = (int)sd.post(leg); it.No = No; it.want_norm = want_norm ? 1 : 0;
    return it;
}
// one-site operators as operands: out[s'] = sum_s O[s', s] psi[s] (simple_update.jl:27) is the fiber GEMM with D = d, K = 1 and X[s + d s'] = O[s', s].
// The operators of a pass (d x d, column-major O[s' + d s] as (re, im) pairs) travel in ONE upload
template <class T> struct SiteOps {
    std::vector<T> hx; std::vector<size_t> off; const T* dx = nullptr;
    void add(const double* m, int d) {
        off.push_back(hx.size());
        for (int nn = 0; nn < d; ++nn) for (int kk = 0; kk < d; ++kk) { hx.push_back((T)m[2 * (nn + d * kk)]); hx.push_back((T)m[2 * (nn + d * kk) + 1]); }
    }
    void send(State* s) { dx = upload(s, hx); }
    FiberItem item(size_t k, const SD& sd, const void* in, void* out, bool want_norm) const {
        FiberItem it{}; it.in = in; it.out = out; it.X = dx + off[k];
        it.D = it.Do = sd.d; it.PA = (int)(sd.n / sd.d); it.K = it.PB = it.No = 1; it.want_norm = want_norm ? 1 : 0;
        return it;
    }
};
// One pass, planned when it is constructed (plan_fiber_pass; the items' pointers may be filled in afterwards through plan[k].items / index) and run launch by
// launch: prepare(k) allocates launch k's norm partials (norms: one double per workgroup) and uploads its descriptors, launch(k) enqueues it under a ProfScope of
// class cls (cls < 0: none).  The two are separate because the gate epilogue prepares its register-direct launches before the batch's read-back and launches them
// after it.  Bytes and flops come from the items; those of all RowGemm launches of a pass are booked on the first of them; book = false books none.
struct FiberPass {
    std::vector<FiberLaunch> plan; std::vector<const FiberItem*> d_items; std::vector<Buf> np;
    std::vector<Buf> outs;      // the caller's: output buffers by position in ITS list, where it wants them to live and die with the pass
    bool valid = false;
    FiberPass() = default;
    FiberPass(const std::vector<FiberItem>& items, const FiberRules& r, size_t esz)
        : plan(plan_fiber_pass(items.data(), (int)items.size(), r, esz)), d_items(plan.size(), nullptr), np(plan.size()), valid(true) {}
    void prepare(State* s, size_t k, bool norms);
    template <class T> void launch(State* s, size_t k, int cls, bool book = true) const;
    template <class T> void run(State* s, int cls, bool norms, bool book = true) { for (size_t k = 0; k < plan.size(); ++k) { prepare(s, k, norms); launch<T>(s, k, cls, book); } }
};
inline FiberRules fiber_rules_of(const State* s, FiberUse use) { return fiber_rules(use, s->dtype == TNQS_C64, use_mfma(), use_chi64()); }
template <class T> void run_chains(State* s, std::vector<Chain>& chains, int cls, int cls_pair = -1);
template <class T, class Acc> void run_grams(State* s, std::vector<GramJob>& jobs, int cls);
// one end (u, leg) of a bond and its environment E_u[(s, a), (s', a')] as Gram partials (engine_rdm.cpp run_env_ends; shared by rdm_edges and rdm_paths).
// cls: the Gram route class -- 0 = f64 accumulation (partials double), 1 / 2 = the f32 matrix-core Grams (partials float; ComplexF32 states with env_f32_class(KK) != 0 only)
struct EnvEnd { int u = -1, leg = -1; SD sd; int KK = 0; size_t ws_bytes = 0; int cls = 0; Buf partial; int nchunks = 0; };
int env_f32_class(int KK);
template <class T> void run_env_ends(State* s, std::vector<EnvEnd>& ends, size_t e0, size_t e1);
// a vertex with an in-leg ja (bond dimension ca) and an out-leg jb (cb), and its double-layer transfer matrix T[(b + cb b') + cb^2 (a + ca a')] (engine_loops.cpp
// build_transfer_matrices; shared by loop_weights and rdm_paths); phi / psi: the permuted operands of the GEMM that wrote T
struct TransferVertex { int v, ja, jb, ca, cb; SD sd; Buf phi, psi, T; };
template <class T> void build_transfer_matrices(State* s, const std::vector<TransferVertex*>& lvs, const char* who);
// the three-leg Gram of a branch vertex (engine_configs.cpp, tnqs_dbg_loop_branch_gram): legs of dimensions x[0 .. 2] (the row index of both operands, leg 0 fastest),
// contraction length k; the output holds the pairs (ket, bra) of the legs ord[0], ord[1], ord[2] in this order, ket faster.  Pointers are left to the caller
inline BranchGramItem branch_gram_item(const int x[3], const int ord[3], int k) {
    BranchGramItem it{}; it.m = it.n = x[0] * x[1] * x[2]; it.k = k; it.R0 = it.C0 = x[0]; it.R1 = it.C1 = x[1];
    long long base = 1;
    for (int p = 0; p < 3; ++p) { const int l = ord[p]; it.sr[l] = base; it.sc[l] = base * x[l]; base *= (long long)x[l] * x[l]; }
    return it;
}
template <class T> void svd_batch(State* s, const std::vector<JacobiItem>& all, bool with_v);
void svd_tall(State* s, const std::vector<JacobiItem>& tall, int* d_fail = nullptr, int* d_polish_sweeps = nullptr);     // svd_batch's Cholesky-QR route (ComplexF32, no V)
// the launch of svd_batch an item is put into, decided from the sizes the host knows (upper bounds where JacobiItem::dyn is set); none: an empty matrix
enum class SvdList { none, fit, tall, rest };      // LDS-resident Jacobi, Cholesky-QR route (svd_tall), global-memory Jacobi
template <class T> SvdList svd_batch_list(const JacobiItem& j, bool with_v, size_t esz);
// ---- the SVD stage of a two-site gate (gate_svd.cpp): TwoSiteBatch::svd_and_finish (engine_gates.cpp) and tnqs_dbg_theta_svd_stage (debug_gate.cpp) run the same code --------
// One gate: theta (in: the matrix the SVD runs on, out: U Sigma), theta0 (the unrotated full theta), thetaV (out: V), all on the device; the bounds n_s = d_s chi; the
// device info array (GateItem::info; info[4] receives the sweep count); K = the columns of the low-rank factor the host expects (kappa chi, 0: no low-rank route); lowQ =
// the orthonormal factor Q of that route (null: none); a1, a2 = (rank a site CAN have) * d of the two sites, behind the pre = 1 offer; cap = the bond dimension cap
struct ThetaSvdGate { void* theta; const void* theta0; void* thetaV; int d1, d2, n1, n2; int* info; int K; const void* lowQ; int a1, a2, cap; };
// svd_batch over the gates' items, then the recovery of V (recover_mfma: recover_v_mfma_kernel, else recover_v_kernel<T, 8>).  dims = the gates' info arrays on the host
// (8 ints per gate), or null: the kernels read them on the device (JacobiItem::dyn), the launches are sized from the bounds and the ComplexF32 gates are offered to
// theta_svd_pre_kernel by the rules above (K, lowQ, a1, a2 and cap are read in that case only)
template <class T> void launch_theta_svd_stage(State* s, const std::vector<ThetaSvdGate>& gates, const int* dims, bool recover_mfma);
// which kernel factorises the gate, from the same item and the same predicates on the host -- info: the 8 ints the device holds (dims where dims is given).  The values
// of TNQS_DBG_ROUTE_SVD_* (include/tnqs_debug.h)
enum { ThetaSvdNone = 0, ThetaSvdPreLow = 10, ThetaSvdPreTheta = 11, ThetaSvdLds = 12, ThetaSvdGlobal = 13, ThetaSvdTall = 14 };
int theta_svd_route(bool F32, const ThetaSvdGate& g, const int* dims, const int* info);
// optimistic: (apply_gates, a tolerance given) return after ENQUEUING the first sweep with its verdict left as a Check (engine.hpp); iters_before: sweeps this
// update has already run (the continuation after a verdict turned out negative)
template <class T> void bp_update_t(State* s, const tnqs_bp_opts* o, int* niter_out, double* diff_out, bool optimistic = false, int iters_before = 0);

// ---- deferred verification (round 6; engine_runahead.cpp) ---------------------------------------------------------------------------------
// apply_gates runs ahead of the device: a gate batch whose outcome is predictable (every bond already at its cap: the new bond dimension is the cap, no
// factorisation falls back) and a BP update that is expected to converge in its first sweep are ENQUEUED on those assumptions -- no host round trip in the
// dependent launch chains -- and leave a Check behind: the staged copy of what decides the assumption, an event behind that copy, and the decision.  Site tensors
// and messages are never mutated in place, so the state before any step is a vector of references (Snapshot); a check that fails (rare: a cutoff that bites at a
// saturated bond, a collapsed pivot, a sweep that misses the tolerance) puts the snapshot back, drains the stream and runs the step again the careful way.
// Checks are settled in order; every host synchronisation point of the path settles what is pending, and apply_gates settles everything before it returns.
constexpr size_t kMaxPendingChecks = 12;      // apply_gates waits for the oldest check before it leaves more than this many pending
static_assert(kMaxPendingChecks < (size_t)kCheckEvents, "a pending check's event must not be handed out again (HostArena::cev is a ring)");
constexpr int kPenaltySteps = 12;             // steps a handle and its copies run one step deep after a failed verification (Graph::spec_penalty)
// Running ahead keeps the state in front of every unverified step alive (the site tensors a batch replaced): up to a layer's worth of extra copies.  Handles with
// more site tensors than this stay one step deep.  (measured, round 6: heavy-hex 3.0 -> 2.6 ms per layer, 7 x 7 unchanged -- its launch chain is 97 % busy either
// way --, 20 x 20 112.6 against 111.5 ms and 37 against 22 GiB at the peak: where the tensor passes fill the device there is no idle time to win, only memory to lose)
constexpr size_t kRunAheadMaxSiteBytes = size_t(2) << 30;

struct Snapshot {      // everything of a State that a step of apply_gates replaces
    std::vector<int> chi; std::vector<Buf> site, sscale, msg; std::vector<std::vector<double>> pend1; std::vector<char> unit_norm;
    tnqs_apply_stats stats{}; bool real_io = false;
    explicit Snapshot(const State& s) : chi(s.chi), site(s.site), sscale(s.sscale), msg(s.msg), pend1(s.pend1), unit_norm(s.unit_norm), stats(s.stats), real_io(s.real_io) {}
    void restore(State& s) const { s.chi = chi; s.site = site; s.sscale = sscale; s.msg = msg; s.pend1 = pend1; s.unit_norm = unit_norm; s.stats = stats; s.real_io = real_io; }
};
struct SpecFailed { int kind, step, iters_done; };       // thrown by settle() for the first check that does not hold (the fields of its Check)

// Evaluate the pending checks, oldest first.  block: wait for each; otherwise stop at the first whose event has not fired.  The first check that does not
// hold is removed and thrown as SpecFailed -- the caller (RunAhead) drains the stream, drops the younger checks and puts the snapshot back.  Call it only
// where nothing of the State has been replaced since the last consistent point, or where a snapshot covers what has.
void settle(State* s, bool block);
// `bytes` of pinned staging for a check's read-back (valid until the check is settled); makes room by settling what is pending when the ring is full -- so it may
// throw SpecFailed: call it before anything is enqueued on assumptions.  nullptr: too large for the ring (the caller takes the careful route)
char* ring_alloc(State* s, size_t bytes);
// Leave a check behind: the copy of `bytes` at dsrc into `stage` (from ring_alloc) is enqueued, an event taken and recorded behind it, the Check pushed
void post_check(State* s, char* stage, const void* dsrc, size_t bytes, int kind, int cur_step, int iters_done, std::function<bool(State*)> eval);
// drop every pending check unevaluated (the stream has been drained, a snapshot is about to be put back)
void drop_checks(State* s);

// ---- bond entanglement spectra (engine_spectra.cpp), shared with tnqs_dbg_bond_spectrum ----------------------------------------------------------------------------
// the buffers of one request: m1, m2 in the state's type (null = identity); H, V, W, V2: n x n complex128 scratch; trace: one double; out: n doubles; flag: one int
struct BondSpecBufs { const void* m1; const void* m2; void* H; void* V; void* W; void* V2; double* trace; double* out; int n; int* flag; };
double bond_spectrum_cutoff(int dtype);                  // 10 eps of the state's real type (absolute)
const char* bond_spectrum_flag_message(int flag);        // flag bit 1: message eigenvalue <= -cutoff; bit 2: trace not positive and finite
// layout of a call's descriptor arrays: the first nfit items fit the LDS-resident f64 Jacobi with V (largest n: nmax_fit), the rest take the global-memory kernel (nmax_rest)
struct BondSpecLaunch { int nitems, nfit, nmax_fit, nmax_rest; };
BondSpecLaunch fill_bond_spec_items(std::vector<BondSpecBufs> b, double cutoff, std::vector<EnvItem>& ei, std::vector<JacobiItem>& j1, std::vector<JacobiItem>& j2,
                                    std::vector<BondSpecItem>& items);
template <class T> void launch_bond_spectra_stages(hipStream_t st, const EnvItem* d_env, const JacobiItem* d_j1, const JacobiItem* d_j2, const BondSpecItem* d_items,
                                                   const BondSpecLaunch& L);

// Executes a GateSchedule AHEAD of the device: a batch whose outcome is predictable and an update expected to converge in one sweep are enqueued without waiting
// for their results, the state in front of every unverified step is remembered, and a step whose check fails is run again the careful way from that state.
// Results are those of the sequential walk either way.
struct RunAhead {
    using BatchFn = std::function<void(const GateStep&, bool ahead)>;      // one batch step; ahead: it may leave a Check instead of reading its results back
    using UpdateFn = std::function<void(int iters_before)>;               // a BP update; 0: optimistic (its verdict may stay a Check), n > 0: the sweeps after the first n
    RunAhead(State* s, const GateSchedule& steps, BatchFn batch, UpdateFn update);
    void run();      // returns with every check settled; on an error the handle holds the last verified state it could be put back to
private:
    State* const s; const Graph& g; const GateSchedule& steps; const BatchFn batch; const UpdateFn update;
    struct InApply { State* s; explicit InApply(State* st) : s(st) { s->in_apply = true; } ~InApply() { s->in_apply = false; s->cur_step = -1; } } in_apply;
    const bool deep;                                     // the depth policy of the call: false = one step deep (sharded, large, or switched off)
    std::vector<std::unique_ptr<Snapshot>> snaps;        // snaps[k]: the state in front of step k, kept while a check of step k - 1 or later is pending
    size_t k = 0; bool careful = false;                  // the step to run next; careful: it failed its check a moment ago
    bool ahead() const { return deep && g.spec_penalty == 0 && !careful; }
    void step();
    void snapshot_in_front();
    void settle_behind(bool was_ahead);
    void drop_old_snaps();
    const Snapshot* snapshot_for(const SpecFailed& f) const;
    void recover(const SpecFailed& f);
    void unwind();
};

}  // namespace tnqs
