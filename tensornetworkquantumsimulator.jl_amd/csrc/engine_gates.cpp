// engine_gates.cpp -- apply_gates (src/Apply/apply_gates.jl:46-143), simple_update as batched launches, truncate (src/truncate.jl).
#include "engine_internal.hpp"

namespace tnqs {

// ---------------------------------------------------------------------------------------------------------------
// gates
// ---------------------------------------------------------------------------------------------------------------
struct Gate1 { int v; const double* mat; };
struct Gate2 { int v1, v2; const double* mat; int index; };

// apply the pending scale factors of `verts` (out of place: site buffers may be shared with copies of the handle)
template <class T> static void materialize_scale_t(State* s, const std::vector<int>& verts) {
    std::vector<ScaleItem> sc; std::vector<Buf> outs; std::vector<int> vs;
    for (int v : verts) {
        if (v < 0 || v >= (int)s->site.size() || !s->site[v] || !s->sscale[v]) continue;
        Buf out = dalloc(s, s->site[v]->bytes);
        ScaleItem it{}; it.src = s->site[v]->p; it.dst = out->p; it.n = s->site[v]->bytes / s->esz(); it.factor = reinterpret_cast<const double*>(s->sscale[v]->p);
        sc.push_back(it); outs.push_back(out); vs.push_back(v);
    }
    if (sc.empty()) return;
    HIPCHK(hipSetDevice(s->device));
    const ScaleItem* d = upload(s, sc);
    { ProfScope ps(s, TNQS_PROF_SMALL, 0, 0); launch_scale<T>(s->stream, d, (int)sc.size()); }
    for (size_t i = 0; i < vs.size(); ++i) { s->keepalive.push_back(s->site[vs[i]]); s->keepalive.push_back(s->sscale[vs[i]]); s->site[vs[i]] = outs[i]; s->sscale[vs[i]] = nullptr; }
}
void materialize_scale(State* s, const std::vector<int>& verts) {
    if (s->dtype == TNQS_C64) materialize_scale_t<float>(s, verts); else materialize_scale_t<double>(s, verts);
}
void materialize_scale_all(State* s) {
    std::vector<int> all(s->site.size()); std::iota(all.begin(), all.end(), 0);
    materialize_scale(s, all);
}
template <class T> static void apply_one_site_batch(State* s, const std::vector<Gate1>& gates_in, bool normalize, bool force);
// apply the pending one-site gates of `verts` (State::pend1) in one streaming pass; they are unitary, so norms, pending scale factors
// and unit_norm stay as they are
void materialize_pending(State* s, const std::vector<int>& verts) {
    std::vector<std::vector<double>> mats; std::vector<Gate1> gs; std::vector<char> norm_was;
    for (int v : verts) {
        if (v < 0 || v >= (int)s->pend1.size() || s->pend1[v].empty()) continue;
        mats.push_back(std::move(s->pend1[v])); s->pend1[v].clear(); norm_was.push_back(s->unit_norm[v]);
        gs.push_back(Gate1{v, nullptr});
    }
    if (gs.empty()) return;
    for (size_t k = 0; k < gs.size(); ++k) gs[k].mat = mats[k].data();
    HIPCHK(hipSetDevice(s->device));
    if (s->dtype == TNQS_C64) apply_one_site_batch<float>(s, gs, false, true); else apply_one_site_batch<double>(s, gs, false, true);
    for (size_t k = 0; k < gs.size(); ++k) s->unit_norm[gs[k].v] = norm_was[k];
}
void materialize_pending_all(State* s) {
    std::vector<int> all(s->site.size()); std::iota(all.begin(), all.end(), 0);
    materialize_pending(s, all);
}

// the new site tensors replace the old ones; with `normalize` their norm (from the producing kernel's partial sums) becomes
// the pending scale factor 1/||psi|| instead of a scaling pass over the tensor (simple_update.jl:66-72 normalises eagerly;
// every later step of the path is invariant under a real rescaling of a site tensor, see engine.hpp State::sscale)
template <class T> static void norm_and_replace(State* s, const std::vector<int>& verts, const std::vector<Buf>& outs, const Buf& norm_partials,
                                                const std::vector<int>& tile_begin, const std::vector<int>& ntiles, bool normalize) {
    if (normalize) {
        std::vector<NormFactorItem> nf;
        Buf fac = dalloc(s, verts.size() * 256);           // one factor per site, 256-byte slots (aliased Bufs below)
        for (size_t i = 0; i < verts.size(); ++i) {
            NormFactorItem it{}; it.norm_partials = reinterpret_cast<const double*>(norm_partials->p) + tile_begin[i]; it.npart = ntiles[i];
            it.factor = reinterpret_cast<double*>(reinterpret_cast<char*>(fac->p) + 256 * i);
            nf.push_back(it);
        }
        const NormFactorItem* d = upload_small(s, nf);
        { ProfScope ps(s, TNQS_PROF_SMALL, 0, 0); launch_norm_factor(s->stream, d, (int)nf.size()); }
        for (size_t i = 0; i < verts.size(); ++i) { s->site[verts[i]] = outs[i]; s->sscale[verts[i]] = sub_buffer(fac, 256 * i, 8); }
    } else {
        for (size_t i = 0; i < verts.size(); ++i) s->site[verts[i]] = outs[i];       // a pending factor of the input carries over (linear map)
    }
}

// the same for launch k of a fiber GEMM pass: vert_of[i] = the vertex of the pass's item i, whose output is P.outs[i]
template <class T> static void norm_and_replace(State* s, const FiberPass& P, size_t k, const std::vector<int>& vert_of, bool normalize) {
    const FiberLaunch& L = P.plan[k];
    std::vector<int> verts, tb; std::vector<Buf> outs;
    for (size_t i = 0; i < L.items.size(); ++i) { verts.push_back(vert_of[L.index[i]]); outs.push_back(P.outs[L.index[i]]); tb.push_back(L.items[i].tile_begin); }
    norm_and_replace<T>(s, verts, outs, P.np[k], tb, L.nwg, normalize);
}

// d x d complex matrices, column-major [s' + d s] as (re, im) pairs
static bool is_unitary(const double* m, int d, double tol) {
    for (int a = 0; a < d; ++a) for (int b = 0; b < d; ++b) {
        double re = 0, im = 0;                                    // (G^dagger G)[a][b] = sum_s conj(G[s][a]) G[s][b]
        for (int t = 0; t < d; ++t) { const double* x = m + 2 * (t + d * a); const double* y = m + 2 * (t + d * b); re += x[0] * y[0] + x[1] * y[1]; im += x[0] * y[1] - x[1] * y[0]; }
        if (std::fabs(re - (a == b ? 1.0 : 0.0)) > tol || std::fabs(im) > tol) return false;
    }
    return true;
}
static std::vector<double> matmul_dd(const double* a, const double* b, int d) {       // a . b
    std::vector<double> c(2 * (size_t)d * d, 0.0);
    for (int i = 0; i < d; ++i) for (int j = 0; j < d; ++j) {
        double re = 0, im = 0;
        for (int t = 0; t < d; ++t) { const double* x = a + 2 * (i + d * t); const double* y = b + 2 * (t + d * j); re += x[0] * y[0] - x[1] * y[1]; im += x[0] * y[1] + x[1] * y[0]; }
        c[2 * (i + d * j)] = re; c[2 * (i + d * j) + 1] = im;
    }
    return c;
}

template <class T> static void apply_one_site_batch(State* s, const std::vector<Gate1>& gates_in, bool normalize, bool force) {
    if (gates_in.empty()) return;
    const size_t esz = s->esz();
    // ---- deferral (State::pend1): a unitary gate on a tensor that needs no normalisation pass is only recorded -- BP does not see it, the
    // next two-site gate on the vertex absorbs it.  Anything else is applied now, composed with what was pending on the vertex.
    std::vector<std::vector<double>> composed; composed.reserve(gates_in.size());
    std::vector<Gate1> gates;
    const bool may_defer = !force && defer_site1() && (!s->sharded() || s->in_apply);      // (sharded handles: only inside apply_gates, State::in_apply)
    // unitary to what the state's precision resolves: a gate the caller built in complex64 is unitary to ~1e-7 only, and BP messages of a
    // ComplexF32 state do not see a deviation of that size either
    const double utol = s->dtype == TNQS_C64 ? 1e-6 : 1e-13;
    for (auto& g1 : gates_in) {
        const int d = s->d[g1.v];
        std::vector<double>& pend = s->pend1[g1.v];
        if (may_defer && is_unitary(g1.mat, d, utol) && (!normalize || s->unit_norm[g1.v])) {
            pend = pend.empty() ? std::vector<double>(g1.mat, g1.mat + 2 * (size_t)d * d) : matmul_dd(g1.mat, pend.data(), d);
            s->stats.n_deferred_1site += 1;
            continue;
        }
        if (!pend.empty()) { composed.push_back(matmul_dd(g1.mat, pend.data(), d)); pend.clear(); gates.push_back(Gate1{g1.v, composed.back().data()}); }
        else gates.push_back(g1);
        s->unit_norm[g1.v] = normalize ? 1 : 0;
    }
    if (gates.empty()) return;
    if (std::is_same<T, float>::value) {
        bool all2 = true; for (auto& g1 : gates) all2 = all2 && s->d[g1.v] == 2;
        if (all2) {         // streaming 2x2 kernel (HBM-bound: read + write each site tensor once)
            const int NBX = 64;
            std::vector<Site1Item> items; std::vector<int> verts, tb, nt; std::vector<Buf> outs; double bytes = 0, flops = 0;
            for (auto& g1 : gates) {
                if (!s->owns(g1.v)) continue;
                SD sd = site_dims(s, g1.v);
                Site1Item it{}; Buf out = dalloc(s, sd.n * esz);
                it.in = s->site[g1.v]->p; it.out = out->p; it.npairs = sd.n / 2;
                pack_site1_gate(g1.mat, it.g);
                verts.push_back(g1.v); outs.push_back(out); tb.push_back((int)items.size() * NBX); nt.push_back(NBX);
                items.push_back(it);
                bytes += 2.0 * sd.n * esz; flops += 8.0 * sd.n * 2;
            }
            if (items.empty()) return;
            Buf np = dalloc(s, items.size() * NBX * sizeof(double));
            const Site1Item* d = upload(s, items);
            { ProfScope ps(s, TNQS_PROF_GATE_APPLY, bytes, flops);
              launch_site1_c64(s->stream, d, (int)items.size(), NBX, normalize ? reinterpret_cast<double*>(np->p) : nullptr); }
            norm_and_replace<T>(s, verts, outs, np, tb, nt, normalize);
            return;
        }
    }
    std::vector<FiberItem> items; std::vector<int> verts; std::vector<Buf> outs;
    FiberRules rules = fiber_rules_of(s, FiberUse::Plain);
    SiteOps<T> ops;
    for (auto& g1 : gates) { rules.kk_floor = std::max(rules.kk_floor, s->d[g1.v]); ops.add(g1.mat, s->d[g1.v]); }
    ops.send(s);
    for (size_t gi = 0; gi < gates.size(); ++gi) {
        const int v = gates[gi].v;
        if (!s->owns(v)) continue;
        SD sd = site_dims(s, v);
        Buf out = dalloc(s, sd.n * esz);
        items.push_back(ops.item(gi, sd, s->site[v]->p, out->p, normalize));
        verts.push_back(v); outs.push_back(out);
    }
    if (items.empty()) return;
    FiberPass P(items, rules, esz); P.outs = std::move(outs);
    P.run<T>(s, TNQS_PROF_GATE_APPLY, /*norms=*/true);
    norm_and_replace<T>(s, P, 0, verts, normalize);
}

// ---------------------------------------------------------------------------------------------------------------
// two-site gates: simple_update (simple_update.jl:21-77) for a batch of vertex-disjoint gates at once
// ---------------------------------------------------------------------------------------------------------------
// pending one-site gates of the gate vertices are absorbed into the gate matrix: g' = g . (G1 (x) G2) is exactly what simple_update sees
// when the one-site gates were applied to the tensors first (State::pend1); cleared once the batch has replaced the tensors
static std::vector<Gate2> absorb_pending(const State* s, const std::vector<Gate2>& gates_in, std::vector<std::vector<double>>& absorbed) {
    absorbed.reserve(gates_in.size());
    std::vector<Gate2> gates = gates_in;
    for (auto& g2 : gates) {
        const std::vector<double>& p1 = s->pend1[g2.v1]; const std::vector<double>& p2 = s->pend1[g2.v2];
        if (p1.empty() && p2.empty()) continue;
        const int d1 = s->d[g2.v1], d2 = s->d[g2.v2], dd = d1 * d2;
        std::vector<double> kron(2 * (size_t)dd * dd, 0.0);                 // (G1 (x) G2)[(t1 t2),(s1 s2)], first vertex most significant
        for (int t1 = 0; t1 < d1; ++t1) for (int s1 = 0; s1 < d1; ++s1) for (int t2 = 0; t2 < d2; ++t2) for (int s2 = 0; s2 < d2; ++s2) {
            const double ar = p1.empty() ? (t1 == s1 ? 1.0 : 0.0) : p1[2 * (t1 + d1 * s1)], ai = p1.empty() ? 0.0 : p1[2 * (t1 + d1 * s1) + 1];
            const double br = p2.empty() ? (t2 == s2 ? 1.0 : 0.0) : p2[2 * (t2 + d2 * s2)], bi = p2.empty() ? 0.0 : p2[2 * (t2 + d2 * s2) + 1];
            const size_t e = (size_t)(t1 * d2 + t2) + (size_t)dd * (s1 * d2 + s2);
            kron[2 * e] = ar * br - ai * bi; kron[2 * e + 1] = ar * bi + ai * br;
        }
        absorbed.push_back(matmul_dd(g2.mat, kron.data(), dd));
        g2.mat = absorbed.back().data();
    }
    return gates;
}

// the gate as an operator sum g = sum_k a_k (x) b_k: O[(s1',s1),(s2',s2)] = g[(s1' s2'),(s1 s2)] factorised by elimination with complete pivoting
// (exact rank factorisation).  Returns kappa, the operator Schmidt rank (2 for Rzz / Rxx / CNOT / CPHASE, 4 for SWAP); fa gets the kappa columns a_k
// (d1^2 each), fb the kappa rows b_k (d2^2 each).  (Declared in engine_internal.hpp: debug_gate.cpp tnqs_dbg_gate_theta / tnqs_dbg_operator_sum call it too.)
int operator_sum(const double* mat, int d1, int d2, std::vector<std::complex<double>>& fa, std::vector<std::complex<double>>& fb) {
    const int dd = d1 * d2, na = d1 * d1, nb = d2 * d2;
    std::vector<std::complex<double>> O((size_t)na * nb);
    const std::complex<double>* gm = reinterpret_cast<const std::complex<double>*>(mat);
    double amax = 0;
    for (int s1p = 0; s1p < d1; ++s1p) for (int s1 = 0; s1 < d1; ++s1) for (int s2p = 0; s2p < d2; ++s2p) for (int s2 = 0; s2 < d2; ++s2) {
        auto v = gm[(s1p * d2 + s2p) + (size_t)dd * (s1 * d2 + s2)];
        O[(s1p + d1 * s1) + (size_t)na * (s2p + d2 * s2)] = v; amax = std::max(amax, std::abs(v));
    }
    int kp = 0;
    for (; kp < std::min(na, nb); ++kp) {
        int pi = 0, pj = 0; double best = 0;
        for (int j = 0; j < nb; ++j) for (int i = 0; i < na; ++i) { double a = std::abs(O[i + (size_t)na * j]); if (a > best) { best = a; pi = i; pj = j; } }
        if (!(best > 1e-13 * amax)) break;
        const std::complex<double> piv = O[pi + (size_t)na * pj];
        std::vector<std::complex<double>> col(na), row(nb);
        for (int i = 0; i < na; ++i) col[i] = O[i + (size_t)na * pj];
        for (int j = 0; j < nb; ++j) row[j] = O[pi + (size_t)na * j] / piv;
        for (int j = 0; j < nb; ++j) for (int i = 0; i < na; ++i) O[i + (size_t)na * j] -= col[i] * row[j];
        fa.insert(fa.end(), col.begin(), col.end()); fb.insert(fb.end(), row.begin(), row.end());
    }
    return kp;
}

// Everything of a batch the host zeroes and reads back lives in ONE buffer -- [info | low-rank failure flags (two passes) | truncation errors | Cholesky failure
// flags | message-eigenvalue flags]: one memset, one device-to-host copy (5 us of stream time each in a chain of 20-60 us kernels).  Offsets, typed host views.
struct ReadBack {
    size_t info = 0, low = 0, low2 = 0, terr = 0, chol = 0, env = 0, total = 0;
    ReadBack(size_t ngates, size_t nsites, size_t nflags)
        : low(round256(ngates * 32)), low2(low + round256(ngates * 4)), terr(low2 + round256(ngates * 4)), chol(terr + round256(ngates * 8)),
          env(chol + round256(nsites * sizeof(int))), total(env + round256(nflags * sizeof(int))) {}
    const int* info_of(const char* st) const { return reinterpret_cast<const int*>(st + info); }       // per gate (r1, r2, chi', status, sweeps, wide, flagged sites, SVD columns)
    const double* terr_of(const char* st) const { return reinterpret_cast<const double*>(st + terr); }
    const int* chol_of(const char* st) const { return reinterpret_cast<const int*>(st + chol); }
    const int* env_of(const char* st) const { return reinterpret_cast<const int*>(st + env); }
};

// what a gate's read-back books in the statistics: the careful route books it after its read-back, the deferred one when its check holds
struct GateBook {
    int index, cap, d1, d2, K, chi_cap; bool low;
    void book(tnqs_apply_stats& st, const int* hi) const {
        int Mr, Nc, ncolJ; theta_dims(hi, d1, d2, Mr, Nc, ncolJ);
        st.n_lowrank_svd += (ncolJ < Nc) ? 1 : 0; st.n_svd_sweeps += hi[4]; st.n_svd_sweeps_max = std::max(st.n_svd_sweeps_max, hi[4]);
        // qualified for the low-rank route by its ranks, but gate_theta's offer was withdrawn on the device (lowrank_m: a refused pivot)
        const int r1d = hi[0] * d1, r2d = hi[1] * d2;
        if (low && ncolJ == Nc && r1d >= r2d && K < r2d && chi_cap <= K) st.n_lowrank_fallbacks += 1;
    }
};

// eigen factorisation of Hermitian f64 matrices G = V Lambda V^dagger by the Jacobi kernel, V starting from the identity (env_prepare with msg == null: H := I, V := I)
template <class T> static void launch_eigen_from_identity(State* s, const EnvItem* di, const JacobiItem* dj, const std::vector<JacobiItem>& ji) {
    size_t lds = 0; for (auto& j : ji) lds = std::max(lds, jacobi_lds_bytes(j.n, j.n, true, 16));
    { ProfScope ps(s, TNQS_PROF_SMALL, 0, 0); launch_env_prepare<T>(s->stream, di, (int)ji.size()); }
    { ProfScope ps(s, TNQS_PROF_JACOBI, 0, 0); launch_jacobi<double>(s->stream, dj, (int)ji.size(), 60, jacobi_lds(lds), mmax_of(ji)); }
}

enum class ReadRoute { deferred, one_trip, two_trips };      // results staged for a deferred check, one host round trip, or two (theta sized from the ranks read back)

// One two-site batch: the phases of apply_two_site_batch below, in its order, over the state they share.  Nothing of the State is replaced before
// step 5, after every gate's status has been checked: a failing batch leaves the state as it was.
template <class T> struct TwoSiteBatch {
    static constexpr bool F32 = std::is_same<T, float>::value;
    struct SiteJob { int v, other, bleg; bool owned; SD sd; std::vector<int> env_idx; std::vector<int> env_leg; };
    struct EnvRec { int de; int n; void *H, *V, *msq, *prj; };      // views into one arena (env_arena): thousands of 16 KiB pool allocations per batch
                                                                    // were a third of the host time between a BP update and the first kernel of a batch
    struct GateWS { Buf lam1, lam2, idx1, idx2, theta, thetaV, theta0, X1, X2, S, lowA, lowB, lowG, lowL, lowW, lowQ, lowB1, lowG2, lowL2, lowLc; int n1, n2, chi, cap; };

    State* s; const Graph& g; const tnqs_apply_opts& ao; double* errs;
    const size_t esz; const bool sharded;
    // ComplexF64, single rank: ill-conditioned sites get a second factorisation pass (second_pass), which sorts out what is signal and what is
    // noise among the smallest directions -- so the first pass keeps everything above the f64 noise floor instead of rank_tau
    const bool qr2;
    bool may_defer = false; double sqrt_cutoff = 0;
    std::vector<std::vector<double>> absorbed; std::vector<Gate2> gates; int ng;
    std::vector<SiteJob> sj; std::vector<char> part;            // part: this rank runs the small algebra of the gate
    std::vector<EnvRec> envs; Buf env_arena;
    std::vector<int> own_idx;                                   // indices into sj of the owned sites
    std::vector<Chain> chains; std::vector<const void*> fused_M, gauged_of; std::vector<GramJob> jobs;
    std::vector<Buf> GA, GV, GW; std::vector<char> is_chol, is_small, small_done;
    hipEvent_t ev_small = nullptr;
    std::vector<size_t> slot; size_t stride = 0; std::vector<char> cross;      // G slots of the cross-rank Gram exchange (grams)
    ReadBack rb{0, 0, 0}; Buf d_rb, d_texp; const char* st_all = nullptr;               // st_all: the staged copy of d_rb
    std::vector<int> h_flags, h_cholfail, hinfo, info; std::vector<double> hterr, terr;
    std::vector<GateWS> ws; std::vector<int> pg; int npg = 0;                  // pg: gates this rank takes part in
    std::vector<GateItem> gitems; const GateItem* d_gitems = nullptr; std::vector<ThetaLowWs> lows; int cap_max = 1; size_t x2_max = 0;
    ReadRoute route = ReadRoute::two_trips;
    FiberPass spec_plan;                                        // the epilogue pass planned before the read-back (plan_epilogue)
    std::vector<const double*> Sptr; Buf S_keep;
    std::vector<Chain> pch;                                     // the projector passes of step 5

    TwoSiteBatch(State* st, const std::vector<Gate2>& gates_in, const tnqs_apply_opts& o, double* e, bool allow_spec)
        : s(st), g(*st->g), ao(o), errs(e), esz(st->esz()), sharded(st->sharded()), qr2(!F32 && use_qr2()), ng((int)gates_in.size()) {
        // ---- run on assumptions?  Every bond of the batch already sits at its cap (a saturated evolution: the new bond dimension is the cap again unless the cutoff
        // bites), the whole chain can be sized from upper bounds (ComplexF32, every theta within the LDS-resident kernels), single rank.  Then the read-back of the
        // batch -- ranks, new bond dimensions, statuses, truncation errors, every fallback flag -- is only STAGED, the epilogue is launched for bond dimension = cap,
        // and the verification happens when the staged copy has arrived (settle).  Anything the assumptions do not cover fails the check and the batch is redone.
        // (ComplexF64 with the second factorisation pass: an evolution flags ill-conditioned sites in almost every batch -- 40 per layer of a 4 x 4 lattice --, which is a
        //  read-back the careful route needs anyway: nothing to run ahead on)
        may_defer = allow_spec && !sharded && ao.maxdim > 0 && !qr2;
        for (size_t k = 0; k < gates_in.size() && may_defer; ++k) {
            const int v1 = gates_in[k].v1, v2 = gates_in[k].v2; const int chi = s->chi[g.edge(v1, v2)];
            const int Mr = std::max(s->d[v1], s->d[v2]) * std::max(s->d[v1], s->d[v2]) * chi, Nc = std::min(s->d[v1], s->d[v2]) * std::min(s->d[v1], s->d[v2]) * chi;
            may_defer = chi == ao.maxdim && Nc >= chi && Mr <= 256 && jacobi_lds(jacobi_lds_bytes(Mr, Nc, false, esz)) > 0;
        }
        sqrt_cutoff = ao.sqrt_cutoff >= 0 ? ao.sqrt_cutoff : 10.0 * (s->dtype == TNQS_C64 ? 1.1920928955078125e-07 : 2.220446049250313e-16);
        gates = absorb_pending(s, gates_in, absorbed);
    }
    // whatever happens before the regular wait (theta_svd) -- an exception in the Gram / reduce / Cholesky steps -- the main stream is ordered behind the side
    // stream of the early small-SVD launches before the batch releases M / GA / GV to the stream-ordered pool (round-4 advisor finding)
    ~TwoSiteBatch() { if (ev_small) (void)hipStreamWaitEvent(s->stream, ev_small, 0); }

    int nof(size_t i) const { return sj[i].sd.d * sj[i].sd.chi[sj[i].bleg]; }
    // sites with fewer fibers than columns are factorised by their owner without a Gram matrix (small-SVD route) and never refined; the
    // criterion must not depend on ownership, every rank taking part in a gate has to reach the same decision
    bool small_shape(size_t i) const { const int n = nof(i); return sj[i].sd.n / (size_t)n < (size_t)n && n <= 256 && use_small_svd(); }
    template <class X> X* dev(size_t off) const { return reinterpret_cast<X*>(reinterpret_cast<char*>(d_rb->p) + off); }     // into d_rb
    GateBook book_of(int q) const { const GateItem& it = gitems[q]; return GateBook{gates[pg[q]].index, ws[pg[q]].cap, it.d1, it.d2, it.kappa * it.chi, it.chi_cap, it.lowG != nullptr}; }

    // without the final normalisation the result scales with the inputs: apply pending factors first
    void materialize_inputs() { std::vector<int> vs; for (auto& g2 : gates) { vs.push_back(g2.v1); vs.push_back(g2.v2); } materialize_scale(s, vs); }

    // ---- 1. environments: sqrt(M) and projector for every incoming message of an owned site (utils.jl:18-27) ------
    void environments() {
        sj.resize(2 * (size_t)ng); part.assign(ng, 0);
        for (int gi = 0; gi < ng; ++gi) {
            for (int side = 0; side < 2; ++side) {
                SiteJob& j = sj[2 * gi + side];
                j.v = side == 0 ? gates[gi].v1 : gates[gi].v2; j.other = side == 0 ? gates[gi].v2 : gates[gi].v1;
                j.sd = site_dims(s, j.v); j.bleg = g.leg(j.v, j.other); j.owned = s->owns(j.v);
                if (j.owned) part[gi] = 1;
                if (!j.owned) continue;
                for (int l = 0; l < j.sd.z; ++l) {
                    if (l == j.bleg) continue;
                    int de = g.dedge(g.nbr[j.v][l], j.v);
                    if (!s->msg[de]) continue;                  // identity message: sqrt = I, nothing to absorb
                    EnvRec r; r.de = de; r.n = j.sd.chi[l];
                    j.env_idx.push_back((int)envs.size()); j.env_leg.push_back(l);
                    envs.push_back(r);
                }
            }
        }
        for (int gi = 0; gi < ng; ++gi) if (part[gi]) pg.push_back(gi);
        npg = (int)pg.size();
        h_flags.assign(2 * envs.size() + 2, 0); h_cholfail.assign(sj.size(), 0);
        rb = ReadBack((size_t)npg, sj.size(), h_flags.size());
        d_rb = dalloc(s, rb.total);
        std::vector<EnvItem> ei; std::vector<JacobiItem> ji; std::vector<EnvFinishItem> fi;
        size_t env_bytes = 0;
        for (auto& r : envs) { const size_t nn = (size_t)r.n * r.n; env_bytes += 2 * round256(nn * 16) + 2 * round256(nn * esz); }
        env_arena = dalloc(s, std::max<size_t>(256, env_bytes));
        char* ap = reinterpret_cast<char*>(env_arena->p);
        ei.reserve(envs.size()); ji.reserve(envs.size()); fi.reserve(envs.size());
        for (size_t i = 0; i < envs.size(); ++i) {
            EnvRec& r = envs[i]; size_t nn = (size_t)r.n * r.n;
            r.H = ap; ap += round256(nn * 16); r.V = ap; ap += round256(nn * 16); r.msq = ap; ap += round256(nn * esz); r.prj = ap; ap += round256(nn * esz);
            ei.push_back(EnvItem{s->msg[r.de]->p, r.H, r.V, r.n});
            ji.push_back(JacobiItem{r.H, r.V, r.n, r.n, nullptr});
            fi.push_back(EnvFinishItem{r.H, r.V, r.msq, r.prj, r.n, sqrt_cutoff, dev<int>(rb.env) + 2 * i});
        }
        // everything up to here was host preparation.  The environment chain (small kernels that only READ the messages and write fresh buffers) is
        // enqueued behind the pending BP sweep right away; the verdict is awaited after that, in front of the tensor passes
        if (envs.empty()) return;
        const EnvItem* de = upload_small(s, ei); const JacobiItem* dj = upload_small(s, ji); const EnvFinishItem* df = upload_small(s, fi);
        { ProfScope ps(s, TNQS_PROF_SMALL, 0, 0); launch_env_prepare<T>(s->stream, de, (int)ei.size()); }
        size_t lds = 0; for (auto& r : envs) lds = std::max(lds, jacobi_lds_bytes(r.n, r.n, true, 16));
        { ProfScope ps(s, TNQS_PROF_JACOBI, 0, 0); launch_jacobi<double>(s->stream, dj, (int)ji.size(), 60, jacobi_lds(lds), mmax_of(ji)); }
        { ProfScope ps(s, TNQS_PROF_SMALL, 0, 0); launch_env_finish<T>(s->stream, df, (int)fi.size()); }
    }

    // ---- 2. gauge: psi~ = psi x_outer M^{1/2}  (simple_update.jl:43-44), owned sites only -----------------------------
    void gauge() {
        for (size_t i = 0; i < sj.size(); ++i) if (sj[i].owned) own_idx.push_back((int)i);
        chains.resize(own_idx.size());
        // bulk shape (d = 2, chi = 32, three gauged legs): the LAST gauge leg -- the fastest outer leg, which the two-leg kernel leaves over -- is
        // absorbed inside the Gram kernel instead of in a pass of its own (kernels_gate.hip); fused_M[q] = its matrix
        fused_M.assign(own_idx.size(), nullptr);
        for (size_t q = 0; q < own_idx.size(); ++q) {
            const SiteJob& j = sj[own_idx[q]];
            Chain& c = chains[q]; c.v = j.v; c.src = s->site[j.v]->p; c.sd = j.sd;
            for (size_t e = 0; e < j.env_idx.size(); ++e) c.steps.push_back({j.env_leg[e], envs[j.env_idx[e]].msq});
            if (!(F32 && use_mfma() && use_pair() && !c.steps.empty() && c.steps[0].first == (j.bleg == 0 ? 1 : 0))) continue;
            const bool bulk = c.steps.size() == 3 && j.sd.n / ((size_t)j.sd.d * j.sd.chi[j.bleg]) >= (size_t)j.sd.d * j.sd.chi[j.bleg] &&
                              gauge_gram64_covers(j.sd.d, j.sd.z, j.sd.chi.data(), j.bleg, c.steps[0].first);
            // 16-dimensional legs (degree 6, chi = 16: five gauge legs): the same with mfma_gauge_gram32_kernel -- four legs in two two-leg passes, the fifth inside the Gram
            const bool legs16 = j.sd.n >= (size_t)(1u << 14) && gauge_gram32_covers(j.sd.d, j.sd.z, j.sd.chi.data(), j.bleg, c.steps[0].first);
            if (bulk || legs16) { fused_M[q] = c.steps[0].second; c.steps.erase(c.steps.begin()); }
        }
        if (!may_defer) settle(s, true);      // the careful route waits for what is pending (the BP update's verdict) in front of its tensor passes: a failure costs the environment chain only
        run_chains<T>(s, chains, TNQS_PROF_GATE_MODEPROD);
        GA.resize(sj.size()); GV.resize(sj.size()); GW.resize(sj.size()); is_chol.assign(sj.size(), 0); is_small.assign(sj.size(), 0); small_done.assign(sj.size(), 0);
        gauged_of.assign(sj.size(), nullptr);      // psi~ of the owned sites
        for (size_t q = 0; q < own_idx.size(); ++q) gauged_of[own_idx[q]] = chains[q].result;
    }

    // the small-SVD items of site i (its n x N matricised psi~ goes to a fresh M)
    void add_small_svd(size_t i, std::vector<SmallSvdItem>& si, std::vector<JacobiItem>& sji) {
        const SD& sd = sj[i].sd; const int b = sj[i].bleg;
        Buf M = dalloc(s, sd.n * 16); s->keepalive.push_back(M);
        small_svd_items(gauged_of[i], M->p, GA[i]->p, GV[i]->p, sd.d, (int)(sd.pre(b) / sd.d), sd.chi[b], (int)sd.post(b), si, sji);
    }

    // ---- 2b. sites with fewer fibers than columns (corners, low bond dimensions) are factorised without a Gram matrix, by a one-sided Jacobi of
    // the small matricised psi~ (f64): three dependent launches (0.2 ms on a 7 x 7 lattice) that only need the gauged tensor.  They start NOW on a
    // side stream, under the Gram pass, instead of in front of the Cholesky kernels afterwards (single rank) -------------------------------------
    void early_small_svd() {
        if (sharded) return;
        std::vector<SmallSvdItem> si; std::vector<JacobiItem> sji;
        for (size_t q = 0; q < own_idx.size(); ++q) {
            const size_t i = own_idx[q];
            if (!small_shape(i) || fused_M[q]) continue;
            const int n = nof(i);
            GA[i] = dalloc(s, (size_t)n * n * 16); GV[i] = dalloc(s, (size_t)n * n * 16); GW[i] = GV[i]; is_small[i] = 1; small_done[i] = 1;
            add_small_svd(i, si, sji);
        }
        if (si.empty()) return;
        const SmallSvdItem* ds = upload_small(s, si); const JacobiItem* dj = upload_small(s, sji);
        hipStream_t side = aux_stream_of(s);
        HIPCHK(hipEventRecord(s->ev_fork, s->stream)); HIPCHK(hipStreamWaitEvent(side, s->ev_fork, 0));
        launch_small_svd<T>(side, ds, dj, sji);
        HIPCHK(hipEventRecord(s->ev_join, side)); ev_small = s->ev_join;
    }

    // G slots: in the sharded case both ranks of a gate that STRADDLES two ranks need G1 and G2 -> all-gather those (a gate whose two sites live on
    // one rank is that rank's business alone: a contiguous partition of the 20 x 20 lattice needs 20 gates' worth per cut of a 25 MB colour batch).  The same layout serves the Gram matrices of the second factorisation pass.
    // Every rank derives the same slots from the gate list and the owner map (grams), so the collective is entered by all ranks or by none.
    void* my_slot(size_t i) const { return reinterpret_cast<char*>(s->exch) + (size_t)s->rank * stride + slot[i]; }
    // all-gather of the G slots, then one private copy of the gathered block (the exchange buffer is reused by the record exchange of this batch);
    // the G of every cross site is a view into it (gathered)
    Buf gather_grams() {
        exchange(s, stride);
        Buf keep = dalloc(s, std::max<size_t>(256, stride * (size_t)s->nranks));
        HIPCHK(hipMemcpyAsync(keep->p, s->exch, stride * (size_t)s->nranks, hipMemcpyDeviceToDevice, s->stream));
        return keep;
    }
    Buf gathered(const Buf& keep, size_t i) const { return sub_buffer(keep, (size_t)s->owner[sj[i].v] * stride + slot[i], (size_t)nof(i) * nof(i) * 16); }

    // ---- 3. G = psi~^dagger psi~ over the outer legs, f64 accumulation (replaces the thin QR, simple_update.jl:45-48) --
    void grams() {
        std::vector<int> job_of(own_idx.size(), -1);
        for (size_t q = 0; q < own_idx.size(); ++q) {
            const SiteJob& sjq = sj[own_idx[q]];
            if (small_done[own_idx[q]]) continue;              // factorised without a Gram matrix (2b)
            GramJob j{}; j.X = chains[q].result; j.Y = chains[q].result; j.sd = sjq.sd; j.leg = sjq.bleg; j.keep_site = true; j.M = fused_M[q];
            job_of[q] = (int)jobs.size(); jobs.push_back(j);
        }
        {   // the fused and the plain Gram are different kernels: two batches, job order kept
            std::vector<GramJob> jf, jf16, jp; std::vector<size_t> idf, idf16, idp;
            for (size_t q = 0; q < jobs.size(); ++q) {
                if (jobs[q].M && jobs[q].sd.chi[jobs[q].leg] == 16) { jf16.push_back(jobs[q]); idf16.push_back(q); }
                else if (jobs[q].M) { jf.push_back(jobs[q]); idf.push_back(q); } else { jp.push_back(jobs[q]); idp.push_back(q); }
            }
            run_grams<T, double>(s, jf, TNQS_PROF_GATE_GRAM);
            run_grams<T, double>(s, jf16, TNQS_PROF_GATE_GRAM);
            run_grams<T, double>(s, jp, TNQS_PROF_GATE_GRAM);
            for (size_t q = 0; q < jf.size(); ++q) jobs[idf[q]] = jf[q];
            for (size_t q = 0; q < jf16.size(); ++q) jobs[idf16[q]] = jf16[q];
            for (size_t q = 0; q < jp.size(); ++q) jobs[idp[q]] = jp[q];
        }
        slot.assign(sj.size(), 0); cross.assign(sj.size(), 0);        // cross: the site's gate partner lives on another rank
        if (sharded) {
            std::vector<size_t> rank_bytes(s->nranks, 0);
            for (size_t i = 0; i < sj.size(); ++i) {
                if (s->owner[sj[i].v] == s->owner[sj[i].other]) continue;
                cross[i] = 1;
                int r = s->owner[sj[i].v]; slot[i] = rank_bytes[r]; rank_bytes[r] += round256((size_t)nof(i) * nof(i) * 16);
            }
            for (size_t b : rank_bytes) stride = std::max(stride, b);
            if (stride) check_exchange(s, stride);
        }
        std::vector<ReduceItem> ri; int elems = 0;
        for (size_t q = 0; q < own_idx.size(); ++q) {
            if (job_of[q] < 0) continue;
            const GramJob& jb = jobs[job_of[q]];
            size_t i = own_idx[q]; int n = jb.KK; size_t nn = (size_t)n * n;
            GA[i] = dalloc(s, nn * 16);
            ri.push_back(ReduceItem{jb.partial->p, cross[i] ? my_slot(i) : GA[i]->p, (int)nn, jb.nchunks, 1, elems}); elems += (int)nn;
        }
        const ReduceItem* dr = upload(s, ri);
        { ProfScope ps(s, TNQS_PROF_SMALL, 0, 0); launch_reduce<double, double>(s->stream, dr, (int)ri.size(), elems); }
        if (sharded && stride) {
            Buf keep = gather_grams();
            for (size_t i = 0; i < sj.size(); ++i) if (part[i / 2] && cross[i]) GA[i] = gathered(keep, i);
        }
    }

    // R factor of psi~ = Q R from G = R^dagger R: Cholesky (R = L^dagger) where G has full rank by construction (at least as
    // many fibers as columns); the f64 Jacobi eigen factorisation R = Lambda^1/2 W^dagger otherwise, and for the sites whose Cholesky
    // pivot collapsed (numerically rank-deficient G; the eigen path drops the null space, rank_tau in kernels.hpp): the fallback pass
    void factor_G(bool allow_chol, bool fallback = false) {
        std::vector<JacobiItem> ji, sji; std::vector<EnvItem> idn; std::vector<CholItem> ci; std::vector<SmallSvdItem> si; int cmax = 1;
        int* d_cholfail = dev<int>(rb.chol);      // one flag per site: only the sites whose pivot collapsed are redone
        if (!fallback) HIPCHK(hipMemsetAsync(d_cholfail, 0, std::max<size_t>(1, sj.size()) * sizeof(int), s->stream));
        for (size_t i = 0; i < sj.size(); ++i) {
            if (!part[i / 2] || small_done[i]) continue;
            if (fallback && !(is_chol[i] && h_cholfail[i])) continue;      // fallback pass: only the Cholesky sites whose pivot collapsed (the eigen sites are factorised, GA rotated in place)
            int n = nof(i);
            if (!GV[i]) GV[i] = dalloc(s, (size_t)n * n * 16);
            const size_t Nout = sj[i].sd.n / (size_t)n;
            const bool ch = allow_chol && n <= (use_chi64() ? 128 : 96) && Nout >= (size_t)n;
            is_chol[i] = ch ? 1 : 0;
            if (!ch && sj[i].owned && Nout < (size_t)n && n <= 256 && use_small_svd()) {
                // fewer fibers than columns: R = Sigma U^dagger straight from the SVD of the n x N matricised psi~ (no rank-deficient G)
                GW[i] = GV[i]; is_small[i] = 1;
                add_small_svd(i, si, sji);
                continue;
            }
            if (ch) {
                GW[i] = dalloc(s, (size_t)n * n * 16);
                ci.push_back(CholItem{GA[i]->p, GV[i]->p, GW[i]->p, n, d_cholfail + i, qr2 ? 1e-15 : rank_tau(F32, n)}); cmax = std::max(cmax, n);
            } else {
                GW[i] = GV[i];
                idn.push_back(EnvItem{nullptr, GV[i]->p, GV[i]->p, n});
                ji.push_back(JacobiItem{GA[i]->p, GV[i]->p, n, n, nullptr});
            }
        }
        if (!si.empty()) {
            const SmallSvdItem* ds = upload_small(s, si); const JacobiItem* dj = upload_small(s, sji);
            ProfScope ps(s, TNQS_PROF_JACOBI, 0, 0);
            launch_small_svd<T>(s->stream, ds, dj, sji);
        }
        if (!ci.empty()) {      // n <= 96: square LDS array; 96 < n <= 128 (chi = 64 sites): packed triangle
            const CholItem* dc = upload_small(s, ci); ProfScope ps(s, TNQS_PROF_JACOBI, 0, 0);
            if (cmax <= 96) launch_chol(s->stream, dc, (int)ci.size(), cmax); else launch_chol_packed(s->stream, dc, (int)ci.size(), cmax);
        }
        if (!ji.empty()) {
            const EnvItem* di = upload_small(s, idn); const JacobiItem* dj = upload_small(s, ji);
            launch_eigen_from_identity<T>(s, di, dj, ji);
        }
    }

    // ---- 4. theta = gate . (R1 R2), SVD, truncation, X1 / X2  (simple_update.jl:51-59): the per-gate workspaces and GateItems -------------
    void gate_items() {
        ws.resize(ng); gitems.resize(pg.size()); lows.assign(pg.size(), ThetaLowWs{});
        // gate matrices and their operator-sum factors, one upload.  ComplexF64 takes the low-rank route as well (round 4): B is orthogonalised by
        // CholeskyQR2 (kernels.hpp LowQr2Item), and the 128 x 64 factor of a chi = 32 gate fits the LDS-resident Jacobi where the 128 x 128 theta
        // (256 KiB) ran in the global-memory kernel
        const bool lowrank_on = use_lowrank();
        std::vector<char> raw;
        std::vector<size_t> off(pg.size()), offA(pg.size(), 0), offB(pg.size(), 0); std::vector<int> kappa(ng, 0);
        for (size_t q = 0; q < pg.size(); ++q) {
            const Gate2& g2 = gates[pg[q]];
            const int d1 = s->d[g2.v1], d2 = s->d[g2.v2], dd = d1 * d2;
            off[q] = raw.size();
            const char* p = reinterpret_cast<const char*>(g2.mat);
            raw.insert(raw.end(), p, p + (size_t)dd * dd * 16);
            if (!lowrank_on) continue;
            std::vector<std::complex<double>> fa, fb;
            kappa[pg[q]] = operator_sum(g2.mat, d1, d2, fa, fb);
            offA[q] = raw.size(); raw.insert(raw.end(), reinterpret_cast<const char*>(fa.data()), reinterpret_cast<const char*>(fa.data()) + fa.size() * 16);
            offB[q] = raw.size(); raw.insert(raw.end(), reinterpret_cast<const char*>(fb.data()), reinterpret_cast<const char*>(fb.data()) + fb.size() * 16);
        }
        std::vector<ThetaRoute> routes(ng);
        for (int gi = 0; gi < ng; ++gi) {
            GateWS& w = ws[gi];
            const SiteJob& a = sj[2 * gi]; const SiteJob& b = sj[2 * gi + 1];
            const ThetaRoute& r = routes[gi] = theta_route(F32, a.sd.d, b.sd.d, a.sd.chi[a.bleg], kappa[gi], ao.maxdim);
            w.n1 = r.n1; w.n2 = r.n2; w.chi = a.sd.chi[a.bleg];
            w.cap = r.cap; cap_max = std::max(cap_max, r.cap);
            x2_max = std::max(x2_max, (size_t)r.Nc * r.cap * esz);
        }
        const char* d_gm = pg.empty() ? nullptr : upload(s, raw);
        // the per-gate workspaces (sixteen small buffers per gate, all of them dead at the end of the batch) are views into a few 4 MiB slabs: ~1100 pool round
        // trips per heavy-hex batch, 0.13 ms of host time in front of gate_theta, were what the chip waited for after the Cholesky kernels
        struct BatchArena { State* s; Buf cur; size_t off = 0, cap = 0;
            Buf get(size_t bytes) {
                const size_t b = round256(std::max<size_t>(bytes, 1));
                if (b > ((size_t)1 << 20)) return dalloc(s, bytes);
                if (!cur || off + b > cap) { cap = (size_t)4 << 20; cur = dalloc(s, cap); off = 0; }
                Buf v = sub_buffer(cur, off, bytes); off += b; return v;
            } } arena{s};
        for (size_t q = 0; q < pg.size(); ++q) {
            int gi = pg[q];
            GateWS& w = ws[gi]; GateItem& it = gitems[q];
            const SiteJob& a = sj[2 * gi]; const SiteJob& b = sj[2 * gi + 1];
            const ThetaRoute& r = routes[gi]; const int Mr = r.Mr, Nc = r.Nc, cap = r.cap;
            // SVD of theta: the right factor is never accumulated from the rotations (in f32 its orthogonality degrades with the
            // rotation count, ~1e-5 at 150 columns) but recovered from an unrotated copy theta0: V = theta0^dagger (U S) S^-2
            w.lam1 = arena.get(w.n1 * 8); w.lam2 = arena.get(w.n2 * 8); w.idx1 = arena.get(w.n1 * 4); w.idx2 = arena.get(w.n2 * 4);
            w.theta = arena.get((size_t)Mr * Nc * esz); w.thetaV = arena.get((size_t)std::max(Mr, Nc) * std::max(Mr, Nc) * esz);
            w.theta0 = arena.get((size_t)Mr * Nc * esz);
            w.X1 = arena.get((size_t)w.n1 * a.sd.d * cap * esz); w.X2 = arena.get((size_t)w.n2 * b.sd.d * cap * esz);
            w.S = arena.get(cap * 8);
            it.GA1 = GA[2 * gi]->p; it.GV1 = GV[2 * gi]->p; it.GA2 = GA[2 * gi + 1]->p; it.GV2 = GV[2 * gi + 1]->p;
            it.GW1 = GW[2 * gi]->p; it.GW2 = GW[2 * gi + 1]->p; it.chol1 = is_chol[2 * gi]; it.chol2 = is_chol[2 * gi + 1];
            it.n1 = w.n1; it.n2 = w.n2; it.d1 = a.sd.d; it.d2 = b.sd.d; it.chi = w.chi;
            it.gate = reinterpret_cast<const double*>(d_gm + off[q]);
            it.kappa = 0; it.opA = it.opB = nullptr; it.lowA = it.lowB = it.lowG = nullptr; it.lowL = nullptr; it.lowfail = nullptr; it.lowW = nullptr; it.lowQ = nullptr;
            // the operator-sum factors and the low-rank workspaces, where theta_route hands them out
            if (r.opsum) {
                w.lowA = arena.get(r.nA * 16); w.lowB = arena.get(r.nB * 16);
                it.kappa = kappa[gi]; it.opA = reinterpret_cast<const double*>(d_gm + offA[q]); it.opB = reinterpret_cast<const double*>(d_gm + offB[q]);
                it.lowA = w.lowA->p; it.lowB = w.lowB->p;
            }
            if (r.low) {
                w.lowG = arena.get(r.nG * 16); w.lowL = arena.get(r.nG * 16); w.lowW = arena.get(r.nG * 16);
                it.lowG = w.lowG->p; it.lowL = w.lowL->p;
                if (r.lowq) { w.lowQ = arena.get(r.nQ * 16); it.lowW = w.lowW->p; it.lowQ = w.lowQ->p; }
                if (!F32) { w.lowB1 = arena.get(r.nB1 * 16); w.lowG2 = arena.get(r.nG2 * 16); w.lowL2 = arena.get(r.nG2 * 16); w.lowLc = arena.get(r.nG2 * 16); }
                auto ptr = [](const Buf& b) -> void* { return b ? b->p : nullptr; };
                lows[q] = ThetaLowWs{w.lowW->p, ptr(w.lowB1), ptr(w.lowG2), ptr(w.lowL2), ptr(w.lowLc)};
            }
            it.lam1 = (double*)w.lam1->p; it.lam2 = (double*)w.lam2->p; it.idx1 = (int*)w.idx1->p; it.idx2 = (int*)w.idx2->p;
            it.theta = w.theta->p; it.thetaV = w.thetaV->p; it.theta0 = w.theta0->p; it.X1 = w.X1->p; it.X2 = w.X2->p; it.S = (double*)w.S->p;
            it.maxdim = ao.maxdim; it.cutoff = ao.cutoff; it.normalize = ao.normalize_tensors; it.chi_cap = cap;
            // second-pass mode: the eigen route of the first pass is shifted (negative tau, gate_eigs) -- it must not drop a direction the
            // second pass could still resolve
            // (the small-SVD sites are factorised without a Gram matrix and are never refined: ordinary threshold)
            auto site_tau = [&](size_t i, int n) { return (qr2 && !small_shape(i)) ? -rank_tau(false, n) : rank_tau(F32, n); };
            it.tau1 = site_tau(2 * (size_t)gi, w.n1); it.tau2 = site_tau(2 * (size_t)gi + 1, w.n2); it.rk1 = nullptr; it.rk2 = nullptr;
        }
        // per-gate (r1, r2, chi', status, sweeps, wide, -, -) and truncation error live in two contiguous arrays of d_rb (zeroed by run_theta);
        // low-rank route: one failure flag per gate for the Cholesky factorisation of B^dagger B
        d_texp = dalloc(s, std::max<size_t>(1, (size_t)npg * sizeof(int)));
        for (int q = 0; q < npg; ++q) {
            gitems[q].info = dev<int>(rb.info) + 8 * q; gitems[q].truncerr = dev<double>(rb.terr) + q;
            gitems[q].lowfail = dev<const int>(rb.low) + q; gitems[q].texp = reinterpret_cast<int*>(d_texp->p) + q;
        }
        d_gitems = upload(s, gitems);       // (read again after the host synchronisations of the batch: a device copy, not upload_small)
    }

    void run_theta() {
        HIPCHK(hipMemsetAsync(d_rb->p, 0, rb.terr, s->stream));       // info and both low-rank failure flag arrays (contiguous)
        ProfScope ps(s, TNQS_PROF_SMALL, 0, 0);
        const DescUpload up{[](void* st, const void* p, size_t bytes) { return upload_small_bytes(static_cast<State*>(st), p, bytes); }, s};
        launch_theta_chain<T>(s->stream, d_gitems, gitems, lows, dev<int>(rb.low), dev<int>(rb.low2), up);
    }

    // SVD of theta (rotated in place to U Sigma), recovery of V from the unrotated copy, truncation and X1 / X2.  `dims` = the ranks
    // read back from the device, or null: the kernels read them from the gates' info arrays themselves (JacobiItem::dyn) and the
    // host sizes the launches with upper bounds
    void svd_and_finish(const int* dims) {
        std::vector<ThetaSvdGate> sg;
        auto rub = [&](size_t i) { const int n = nof(i); return (int)std::min<size_t>((size_t)n, sj[i].sd.n / (size_t)n); };      // the rank a site CAN have (fewer fibers than columns: a corner)
        for (int q = 0; q < npg; ++q) {
            const int gi = pg[q]; const GateItem& it = gitems[q];
            sg.push_back(ThetaSvdGate{ws[gi].theta->p, ws[gi].theta0->p, ws[gi].thetaV->p, it.d1, it.d2, ws[gi].n1, ws[gi].n2, it.info, it.lowG ? it.kappa * it.chi : 0, it.lowQ,
                                      rub(2 * (size_t)gi) * it.d1, rub(2 * (size_t)gi + 1) * it.d2, ws[gi].cap});
        }
        launch_theta_svd_stage<T>(s, sg, dims, F32 && use_mfma());      // gate_svd.cpp
        { ProfScope ps(s, TNQS_PROF_SMALL, 0, 0); launch_gate_finish<T>(s->stream, d_gitems, npg); }
    }

    // (r1, r2, chi', status, ...), the truncation errors of every gate and every flag of the batch: one copy, one synchronisation
    void read_results() {
        st_all = readback<char>(s, d_rb->p, rb.total);
        HIPCHK(hipStreamSynchronize(s->stream)); drained(s);
        if (npg) { const int* a = rb.info_of(st_all); const double* b = rb.terr_of(st_all);
                   std::copy(a, a + (size_t)npg * 8, hinfo.begin()); std::copy(b, b + npg, hterr.begin()); }
    }
    void read_and_settle() {
        read_results();
        if (!envs.empty()) std::copy(rb.env_of(st_all), rb.env_of(st_all) + 2 * envs.size(), h_flags.begin());
        if (!sj.empty()) std::copy(rb.chol_of(st_all), rb.chol_of(st_all) + sj.size(), h_cholfail.begin());
        settle(s, true);              // (the stream is drained: what was pending has fired; a failed check unwinds this batch before it has replaced anything)
    }
    // the factors of some sites changed: theta once more, its ranks read back
    void retheta() {
        d_gitems = upload(s, gitems);
        run_theta();
        if (npg) HIPCHK(hipMemcpyAsync(hinfo.data(), dev<int>(rb.info), (size_t)npg * 32, hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream)); drained(s);
    }
    bool chol_failures() const { for (size_t i = 0; i < sj.size(); ++i) if (part[i / 2] && is_chol[i] && h_cholfail[i]) return true; return false; }
    // numerically rank-deficient Gram matrix somewhere in the batch: those sites take the eigen path, theta is formed again
    void redo_with_eigen() {
        factor_G(false, true);
        for (int q = 0; q < npg; ++q) { int gi = pg[q]; GateItem& it = gitems[q]; it.GW1 = GW[2 * gi]->p; it.GW2 = GW[2 * gi + 1]->p; it.chol1 = is_chol[2 * gi]; it.chol2 = is_chol[2 * gi + 1]; }
        retheta();
        s->stats.n_chol_fallbacks += 1;
    }

    // ---- second factorisation pass (CholeskyQR2) of the sites gate_theta flagged as ill-conditioned: a Gram matrix resolves the
    // singular directions of psi~ only down to sigma_rel ~ 1e-7, the reference's QR to eps.  Q1 = psi~ R1^+ is formed explicitly;
    // its Gram matrix is close to the identity on everything the first pass resolved and shows the true weight of what it did not,
    // so R = R2 R1 is as accurate as a Householder R.  
    // Sharded: the owner of a site forms Q1 and its Gram matrix, one more all-gather (same slots as the first Gram exchange, issued
    // by every rank whether or not it has a flagged site -- it is a collective) hands it to the partner rank, and both compose the
    // same factor from the same inputs.
    void second_pass() {
        std::vector<size_t> rs; std::vector<int> rq;
        for (int q = 0; q < npg; ++q) for (int side = 0; side < 2; ++side) {
            const size_t i = 2 * (size_t)pg[q] + side;
            if (((hinfo[8 * q + 6] >> side) & 1) && !small_shape(i)) { rs.push_back(i); rq.push_back(q); }
        }
        if (!sharded && rs.empty()) return;
        const size_t m = rs.size();
        std::vector<Buf> X1(m), Q1(m), G2(m), V2(m), GVn(m), GWn(m); Buf d_rk = dalloc(s, std::max<size_t>(1, m) * sizeof(int));
        std::vector<Qr2Site> qs; std::vector<Qr2RinvItem> ri; std::vector<FiberItem> fi; std::vector<GramJob> gj; std::vector<size_t> own_k;
        for (size_t k = 0; k < m; ++k) {
            const size_t i = rs[k]; const int q = rq[k]; const bool second = (i & 1) != 0; const int n = nof(i); const size_t nn = (size_t)n * n;
            X1[k] = dalloc(s, nn * 16); V2[k] = dalloc(s, nn * 16); GVn[k] = dalloc(s, nn * 16); GWn[k] = dalloc(s, nn * 16);
            qs.push_back(Qr2Site{GW[i]->p, GV[i]->p, second ? gitems[q].lam2 : gitems[q].lam1, second ? gitems[q].idx2 : gitems[q].idx1, gitems[q].info + (second ? 1 : 0), n, X1[k]->p});
            ri.push_back(qs[k].rinv());
            if (sj[i].owned) { own_k.push_back(k); Q1[k] = dalloc(s, sj[i].sd.n * esz); }
        }
        for (size_t k : own_k) {
            const size_t i = rs[k]; const SiteJob& j = sj[i];
            FiberItem it = site_fiber_item(j.sd, j.bleg, true, j.sd.chi[j.bleg], false); it.in = gauged_of[i]; it.out = Q1[k]->p; it.X = X1[k]->p;
            fi.push_back(it);
            GramJob g2{}; g2.X = Q1[k]->p; g2.Y = Q1[k]->p; g2.sd = j.sd; g2.leg = j.bleg; g2.keep_site = true; gj.push_back(g2);
        }
        if (m) { const Qr2RinvItem* d = upload(s, ri); ProfScope ps(s, TNQS_PROF_SMALL, 0, 0); launch_qr2_rinv(s->stream, d, (int)m); }
        if (!fi.empty()) {
            // (Plain: these ComplexF64 sites stay on the generic kernel, whatever the f64 matrix-core kernel would take)
            FiberPass Q(fi, fiber_rules_of(s, FiberUse::Plain), esz);
            Q.prepare(s, 0, /*norms=*/true); Q.launch<T>(s, 0, TNQS_PROF_GATE_APPLY, /*book=*/false);
            s->keepalive.push_back(Q.np[0]);
            run_grams<T, double>(s, gj, TNQS_PROF_GATE_GRAM);
            std::vector<ReduceItem> rd; int elems = 0;
            for (size_t t = 0; t < own_k.size(); ++t) {
                const size_t k = own_k[t], i = rs[k]; const int nn = gj[t].KK * gj[t].KK;
                void* dst;
                if (cross[i]) dst = my_slot(i);
                else { G2[k] = dalloc(s, (size_t)nn * 16); dst = G2[k]->p; }
                rd.push_back(ReduceItem{gj[t].partial->p, dst, nn, gj[t].nchunks, 1, elems}); elems += nn;
            }
            const ReduceItem* d2 = upload(s, rd); ProfScope ps(s, TNQS_PROF_SMALL, 0, 0); launch_reduce<double, double>(s->stream, d2, (int)rd.size(), elems);
        }
        if (sharded && stride) {
            Buf keep = gather_grams();
            for (size_t k = 0; k < m; ++k) if (cross[rs[k]]) G2[k] = gathered(keep, rs[k]);
        }
        if (!m) return;
        std::vector<EnvItem> idn; std::vector<JacobiItem> ji;
        for (size_t k = 0; k < m; ++k) { const int n = nof(rs[k]); idn.push_back(EnvItem{nullptr, V2[k]->p, V2[k]->p, n}); ji.push_back(JacobiItem{G2[k]->p, V2[k]->p, n, n, nullptr}); }
        const EnvItem* di = upload(s, idn); const JacobiItem* dj = upload(s, ji);
        launch_eigen_from_identity<T>(s, di, dj, ji);
        std::vector<Qr2ComposeItem> ci;
        for (size_t k = 0; k < m; ++k) ci.push_back(qs[k].compose(G2[k]->p, V2[k]->p, rank_tau(false, qs[k].n), GVn[k]->p, GWn[k]->p, reinterpret_cast<int*>(d_rk->p) + k));
        { const Qr2ComposeItem* d = upload(s, ci); ProfScope ps(s, TNQS_PROF_SMALL, 0, 0); launch_qr2_compose(s->stream, d, (int)m); }
        for (size_t k = 0; k < m; ++k) {
            const size_t i = rs[k]; GateItem& it = gitems[rq[k]];
            GV[i] = GVn[k]; GW[i] = GWn[k]; s->keepalive.push_back(X1[k]); if (Q1[k]) s->keepalive.push_back(Q1[k]); s->keepalive.push_back(G2[k]); s->keepalive.push_back(V2[k]);
            if (i & 1) { it.GV2 = GV[i]->p; it.GW2 = GW[i]->p; it.chol2 = 2; it.rk2 = reinterpret_cast<int*>(d_rk->p) + k; }
            else { it.GV1 = GV[i]->p; it.GW1 = GW[i]->p; it.chol1 = 2; it.rk1 = reinterpret_cast<int*>(d_rk->p) + k; }
        }
        s->keepalive.push_back(d_rk);
        retheta();      // gate_theta reads the first-pass (lambda, idx, r) of the untouched partner site again and overwrites them with the same values
        for (size_t k = 0; k < m; ++k) s->stats.n_qr2_sites += sj[rs[k]].owned ? 1 : 0;
    }

    // no host round trip: the results travel to the check's staging and are verified when they have arrived; the rest of the batch runs on what they are
    // expected to be -- every factor of full rank, every new bond dimension at its cap, no fallback taken
    void defer(char* stage) {
        std::vector<GateBook> books(npg);
        for (int q = 0; q < npg; ++q) books[q] = book_of(q);
        std::vector<char> chol_site(sj.size(), 0);
        for (size_t i = 0; i < sj.size(); ++i) chol_site[i] = (part[i / 2] && is_chol[i]) ? 1 : 0;
        post_check(s, stage, d_rb->p, rb.total, /*kind=*/0, s->cur_step, 0, [st = (const char*)stage, L = rb, books = std::move(books), chol_site = std::move(chol_site), nenv = envs.size(), errs = errs, qr2 = qr2](State* z) {
            const int* hi = L.info_of(st); const double* ht = L.terr_of(st); const int* fl = L.env_of(st); const int* cf = L.chol_of(st);
            for (size_t q = 0; q < books.size(); ++q) if (hi[8 * q + 2] != books[q].cap || hi[8 * q + 3] != 0 || (qr2 && hi[8 * q + 6] != 0)) return false;      // a bond below its cap, a failed gate, an ill-conditioned ComplexF64 site (second factorisation pass)
            for (size_t i = 0; i < nenv; ++i) if (!fl[2 * i] || fl[2 * i + 1]) return false;                                  // a rank-deficient message (projector pass), or a negative eigenvalue
            for (size_t i = 0; i < chol_site.size(); ++i) if (chol_site[i] && cf[i]) return false;                           // a collapsed Cholesky pivot
            for (size_t q = 0; q < books.size(); ++q) {       // the assumptions held: book what the careful route books after its read-back
                books[q].book(z->stats, hi + 8 * q);
                if (errs) errs[books[q].index] = ht[q];
            }
            return true;
        });
        for (size_t i = 0; i < envs.size(); ++i) { h_flags[2 * i] = 1; h_flags[2 * i + 1] = 0; }
        s->stats.n_spec_batches += 1;
    }

    // theta, its SVD and the read-back of the results by one of the three routes; ht_a / ht_s4 stop where the host starts waiting for the device
    void theta_svd(HostTimer& ht_a, HostTimer& ht_s4) {
        if (ev_small) { HIPCHK(hipStreamWaitEvent(s->stream, ev_small, 0)); ev_small = nullptr; }      // the early small-SVD factors (2b) are inputs of gate_theta
        run_theta();
        info.assign(8 * (size_t)ng, 0); terr.assign(ng, 0.0);
        hinfo.assign(8 * (size_t)std::max(1, npg), 0); hterr.assign(std::max(1, npg), 0.0);
        // ONE host round trip per batch where the whole chain can be sized from upper bounds: ComplexF32 (no second factorisation pass), every
        // theta small enough for the LDS-resident Jacobi at its largest possible size.  The ranks of the R factors stay on the device; the
        // Cholesky failure flags and the message-eigenvalue flags are read together with the results, and a failure (rare) redoes the chain
        bool one_trip = (!qr2 || may_defer) && npg > 0;      // (ComplexF64 on assumptions: no site flagged for the second factorisation pass -- part of the check)
        for (int q = 0; q < npg && one_trip; ++q) {
            const int gi = pg[q];
            const int Mr = std::max(ws[gi].n1 * gitems[q].d1, ws[gi].n2 * gitems[q].d2), Nc = std::min(ws[gi].n1 * gitems[q].d1, ws[gi].n2 * gitems[q].d2);
            one_trip = jacobi_lds(jacobi_lds_bytes(Mr, Nc, false, esz)) > 0 && Mr <= 256;
        }
        // the four staged read-backs of a batch (flags, Cholesky flags, info, truncation errors) are consumed together after ONE synchronisation:
        // room for all of them is made up front, so that none of them can wrap the arena on top of another (round-3 advisor finding)
        const size_t rb_bytes = rb.total + 1024;
        char* stage = (may_defer && one_trip) ? ring_alloc(s, rb.total) : nullptr;      // (may settle -- and throw -- first: nothing of the state has been touched)
        route = stage ? ReadRoute::deferred : one_trip ? ReadRoute::one_trip : ReadRoute::two_trips;
        auto run_ahead = [&]() {        // the whole chain, sized from upper bounds, and the epilogue plan for new bond dimensions at their caps
            svd_and_finish(nullptr);
            if (!sharded && ao.maxdim > 0) spec_plan = plan_epilogue([&](int gi) { return ws[gi].cap; }, [&](size_t q) { return (const void*)s->site[sj[own_idx[q]].v]->p; });
            ht_a.stop(); ht_s4.stop();
        };
        switch (route) {
        case ReadRoute::deferred:
            run_ahead();
            defer(stage);
            break;
        case ReadRoute::one_trip:
            run_ahead();
            reserve_readback(s, rb_bytes);
            read_and_settle();
            if (chol_failures()) { redo_with_eigen(); svd_and_finish(hinfo.data()); read_results(); }
            break;
        case ReadRoute::two_trips:      // theta dims depend on the ranks found on the device: read them back (also where message-eigenvalue errors surface)
            reserve_readback(s, rb_bytes);
            ht_a.stop(); ht_s4.stop();
            read_and_settle();
            if (chol_failures()) redo_with_eigen();
            if (qr2) second_pass();
            svd_and_finish(hinfo.data());
            read_results();
            break;
        }
    }

    // message-eigenvalue errors, and the per-gate results of the read-back (a deferred batch: chi' = cap, what its check expects; booked by the check)
    void book_results() {
        for (size_t i = 0; i < envs.size(); ++i)
            if (h_flags[2 * i + 1]) throw Err(TNQS_ERR_NUMERIC, "simple_update: incoming message has a negative eigenvalue above sqrt_cutoff (DomainError in the reference, src/utils.jl:21)");
        for (int q = 0; q < npg; ++q) {
            if (route == ReadRoute::deferred) { info[8 * (size_t)pg[q] + 2] = ws[pg[q]].cap; continue; }
            const int* hi = hinfo.data() + 8 * q;
            std::copy(hi, hi + 8, info.begin() + 8 * (size_t)pg[q]);
            { static const bool dbg = envflag("TNQS_DEBUG_SWEEPS");      // diagnostics: which thetas the SVD launch of a batch waits for
              if (dbg) { int Mr, Nc, ncolJ; theta_dims(hi, gitems[q].d1, gitems[q].d2, Mr, Nc, ncolJ);
                         std::fprintf(stderr, "[tnqs sweeps] gate %d: r1 %d r2 %d theta %d x %d, SVD on %d columns, %d sweeps, chi' %d\n", pg[q], hi[0], hi[1], Mr, Nc, ncolJ, hi[4], hi[2]); } }
            book_of(q).book(s->stats, hi);
            terr[pg[q]] = hterr[q];
        }
    }

    // ---- 4b. the singular values of every gate; sharded: the owner of the first vertex publishes (chi', status, truncerr, S, X2) of each gate ----------------
    void share_records() {
        Sptr.assign(ng, nullptr);
        if (!sharded) { for (int gi = 0; gi < ng; ++gi) Sptr[gi] = (const double*)ws[gi].S->p; return; }
        // every rank needs (chi', status, truncerr, S) of every gate (bond dimensions and messages are replicated); X2 only travels for a gate that straddles two ranks
        std::vector<size_t> slot(ng, 0); std::vector<size_t> rank_bytes(s->nranks, 0);
        for (int gi = 0; gi < ng; ++gi) {
            int r = s->owner[gates[gi].v1]; slot[gi] = rank_bytes[r];
            rank_bytes[r] += round256(32 + (size_t)cap_max * 8 + (s->owner[gates[gi].v1] != s->owner[gates[gi].v2] ? x2_max : 0));
        }
        size_t stride = 0; for (size_t b : rank_bytes) stride = std::max(stride, b);
        check_exchange(s, stride);
        char* base = reinterpret_cast<char*>(s->exch);
        std::vector<RecordPackItem> rp;          // pack the records of the gates whose first vertex is ours (one launch)
        std::vector<int> qof(ng, -1); for (int q = 0; q < npg; ++q) qof[pg[q]] = q;
        for (int gi = 0; gi < ng; ++gi) {
            if (s->owner[gates[gi].v1] != s->rank) continue;
            const SiteJob& b = sj[2 * gi + 1]; const int q = qof[gi];
            const bool straddles = s->owner[gates[gi].v1] != s->owner[gates[gi].v2];
            rp.push_back(RecordPackItem{base + (size_t)s->rank * stride + slot[gi], gitems[q].info, gitems[q].truncerr, reinterpret_cast<const double*>(ws[gi].S->p),
                                        ws[gi].cap, ws[gi].X2->p, straddles ? (long long)((size_t)ws[gi].n2 * b.sd.d * ws[gi].cap * esz / 8) : 0LL, (long long)(32 + (size_t)cap_max * 8)});
        }
        if (!rp.empty()) { const RecordPackItem* d = upload(s, rp); launch_record_pack(s->stream, d, (int)rp.size()); }
        exchange(s, stride);
        // keep a private copy of the gathered block: the exchange buffer is reused by the next batch
        S_keep = dalloc(s, std::max<size_t>(256, stride * (size_t)s->nranks));
        HIPCHK(hipMemcpyAsync(S_keep->p, base, stride * (size_t)s->nranks, hipMemcpyDeviceToDevice, s->stream));
        std::vector<double> allhdr(4 * (size_t)std::max(1, ng));      // all headers in one gather + one D2H
        std::vector<const void*> srcs(ng);
        for (int gi = 0; gi < ng; ++gi) srcs[gi] = reinterpret_cast<char*>(S_keep->p) + (size_t)s->owner[gates[gi].v1] * stride + slot[gi];
        Buf d_hdr = dalloc(s, (size_t)std::max(1, ng) * 32);
        const void* const* d_srcs = upload(s, srcs);
        launch_header_gather(s->stream, d_srcs, ng, reinterpret_cast<double*>(d_hdr->p));
        if (ng) HIPCHK(hipMemcpyAsync(allhdr.data(), d_hdr->p, (size_t)ng * 32, hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream)); drained(s);
        for (int gi = 0; gi < ng; ++gi) {
            info[8 * gi + 2] = (int)allhdr[4 * gi]; info[8 * gi + 3] = (int)allhdr[4 * gi + 1]; terr[gi] = allhdr[4 * gi + 2];
            const size_t off = (size_t)s->owner[gates[gi].v1] * stride + slot[gi];
            Sptr[gi] = reinterpret_cast<const double*>(reinterpret_cast<const char*>(S_keep->p) + off + 32);
            const SiteJob& b = sj[2 * gi + 1];
            if (b.owned && s->owner[gates[gi].v1] != s->rank)          // the partner rank computed the SVD: its X2 is used in place (a view)
                ws[gi].X2 = sub_buffer(S_keep, off + 32 + (size_t)cap_max * 8, (size_t)ws[gi].n2 * b.sd.d * ws[gi].cap * esz);
        }
    }

    // ---- epilogue pass (step 5): the fiber GEMM psi' = psi~ x_(s,b) X of every owned site, planned for the new bond dimensions chi_of(gate), with its
    // register-direct launches PREPARED -- output buffers, norm partials, uploaded descriptors.  Built twice at most: speculatively BEFORE the read-back of the
    // batch -- assuming every new bond dimension equals its cap and no projector pass is needed, which is the steady state of a saturated evolution -- so that
    // after the synchronisation the epilogue is launched at once instead of after 0.25 ms of host preparation with an idle chip (20x20: 380 items and output
    // buffers); and again after the read-back when the assumption did not hold ----------------------------------------------------------------------------
    // output buffers of the pass's RowGemm launches (rowgemm) or of its other launch, in site order
    void alloc_outs(FiberPass& P, bool rowgemm) {
        std::vector<FiberItem*> at(own_idx.size(), nullptr);
        for (auto& L : P.plan) if ((L.route == FiberRoute::RowGemm) == rowgemm) for (size_t k = 0; k < L.items.size(); ++k) at[L.index[k]] = &L.items[k];
        for (size_t q = 0; q < at.size(); ++q) if (at[q]) { P.outs[q] = dalloc(s, (size_t)at[q]->Do * at[q]->PA * at[q]->No * at[q]->PB * esz); at[q]->out = P.outs[q]->p; }
    }
    template <class ChiOf, class InOf> FiberPass plan_epilogue(ChiOf chi_of, InOf in_of) {
        std::vector<FiberItem> items;
        for (size_t q = 0; q < own_idx.size(); ++q) {
            const size_t i = own_idx[q]; const int gi = (int)i / 2;
            FiberItem it = site_fiber_item(sj[i].sd, sj[i].bleg, true, chi_of(gi), ao.normalize_tensors != 0);
            it.in = in_of(q); it.X = (i & 1) ? ws[gi].X2->p : ws[gi].X1->p;
            items.push_back(it);
        }
        FiberPass P(items, fiber_rules_of(s, FiberUse::Epilogue), esz); P.outs.resize(items.size());
        alloc_outs(P, true);
        for (size_t k = 0; k < P.plan.size(); ++k) if (P.plan[k].route == FiberRoute::RowGemm) P.prepare(s, k, /*norms=*/true);
        return P;
    }

    // ---- 5. psi' = (psi x_outer P) x_(s,b) X  (simple_update.jl:62-64, net effect of gauge + ungauge) ----------------
    void epilogue() {
        pch.resize(own_idx.size());
        for (size_t q = 0; q < own_idx.size(); ++q) {
            const SiteJob& j = sj[own_idx[q]];
            Chain& c = pch[q]; c.v = j.v; c.src = s->site[j.v]->p; c.sd = j.sd;
            for (size_t e = 0; e < j.env_idx.size(); ++e)
                if (!h_flags[2 * j.env_idx[e]]) c.steps.push_back({j.env_leg[e], envs[j.env_idx[e]].prj});  // rank-deficient message only
        }
        run_chains<T>(s, pch, TNQS_PROF_GATE_MODEPROD);
        if (own_idx.empty()) return;
        // the speculative pass built before the read-back when it came true, a fresh one otherwise
        bool spec_ok = spec_plan.valid;
        for (size_t q = 0; q < own_idx.size() && spec_ok; ++q) { const int gi = (int)own_idx[q] / 2; spec_ok = info[8 * gi + 2] == ws[gi].cap && pch[q].steps.empty() && pch[q].result == s->site[sj[own_idx[q]].v]->p; }
        FiberPass fresh_plan;
        if (!spec_ok) {
            spec_plan = FiberPass{};              // (its output buffers go back to the pool)
            fresh_plan = plan_epilogue([&](int gi) { return info[8 * gi + 2]; }, [&](size_t q) { return pch[q].result; });
        }
        FiberPass& P = spec_ok ? spec_plan : fresh_plan;
        std::vector<int> vert_of; for (int i : own_idx) vert_of.push_back(sj[i].v);
        const bool norm = ao.normalize_tensors != 0;
        // the register-direct launches first (one per contracted dimension), then what they left: prepared only now, behind them
        for (size_t k = 0; k < P.plan.size(); ++k) if (P.plan[k].route == FiberRoute::RowGemm) { P.launch<T>(s, k, TNQS_PROF_GATE_APPLY); norm_and_replace<T>(s, P, k, vert_of, norm); }
        alloc_outs(P, false);
        for (size_t k = 0; k < P.plan.size(); ++k) if (P.plan[k].route != FiberRoute::RowGemm) { P.prepare(s, k, /*norms=*/true); P.launch<T>(s, k, TNQS_PROF_GATE_APPLY); norm_and_replace<T>(s, P, k, vert_of, norm); }
    }

    // ---- 6. both bond messages := diag(S)  (apply_gates.jl:126-135), new bond dimension ---------------------------
    void bond_messages() {
        std::vector<DiagItem> di;
        for (int gi = 0; gi < ng; ++gi) {
            int e = g.edge(gates[gi].v1, gates[gi].v2); int chin = info[8 * gi + 2];
            s->chi[e] = chin;
            for (int dir = 0; dir < 2; ++dir) {
                Buf m = dalloc(s, (size_t)chin * chin * esz);
                di.push_back(DiagItem{m->p, Sptr[gi], chin});
                s->msg[2 * e + dir] = m;
            }
            if (errs && route != ReadRoute::deferred) errs[gates[gi].index] = terr[gi];      // (deferred: written by the check, from the staged truncation errors)
        }
        const DiagItem* d = upload_small(s, di);
        { ProfScope ps(s, TNQS_PROF_SMALL, 0, 0); launch_diag<T>(s->stream, d, (int)di.size()); }
        for (auto& g2 : gates) { s->pend1[g2.v1].clear(); s->pend1[g2.v2].clear(); s->unit_norm[g2.v1] = s->unit_norm[g2.v2] = ao.normalize_tensors ? 1 : 0; }
        s->stats.n_two_site += ng;
    }
};

// allow_spec: the batch may be enqueued WITHOUT its host round trip when its outcome is predictable (TwoSiteBatch::may_defer); it then leaves a Check behind (engine_internal.hpp)
template <class T> static void apply_two_site_batch(State* s, const std::vector<Gate2>& gates_in, const tnqs_apply_opts& ao, double* errs, bool allow_spec = false) {
    if (gates_in.empty()) return;
    TwoSiteBatch<T> b(s, gates_in, ao, errs, allow_spec);
    PhaseScope phase_scope(s, TNQS_PROF_PHASE_GATE_BATCH);
    HostTimer ht_a(3);                 // TNQS_HOST_TIMING=1: host time of the batch up to the first read-back (3), between the read-backs (4), after them (5)
    if (!ao.normalize_tensors) b.materialize_inputs();
    HostTimer ht_s1(8);
    b.environments();                  // 1. sqrt(M) and projector of every incoming message
    ht_s1.stop(); HostTimer ht_s2(9);
    b.gauge();                         // 2. psi~ = psi x_outer M^{1/2}
    b.early_small_svd();               // 2b. R of the sites with fewer fibers than columns, on the side stream
    ht_s2.stop(); HostTimer ht_s3(10);
    b.grams();                         // 3. G = psi~^dagger psi~ (all-gathered across ranks where a gate straddles two)
    b.factor_G(use_chol());            //    R from G
    ht_s3.stop(); HostTimer ht_s4(11);
    b.gate_items();                    // 4. theta = gate . (R1 R2), SVD, truncation, X1 / X2
    b.theta_svd(ht_a, ht_s4);
    { HostTimer ht_b(4); b.book_results(); }
    b.share_records();                 // 4b. S (sharded: every gate's record from its owner)
    HostTimer ht_c(5);
    // every gate's status is checked before anything of the handle is replaced: a failing batch leaves the state as it was
    for (int gi = 0; gi < b.ng; ++gi) if (b.info[8 * gi + 3] != 0) throw Err(TNQS_ERR_NUMERIC, "simple_update: internal bond capacity exceeded");
    b.epilogue();                      // 5. psi' = (psi x_outer P) x_(s,b) X
    b.bond_messages();                 // 6. both bond messages := diag(S)
    soft_sync(s);   // workspace of this batch goes back to the pool at the next stream synchronisation (the BP update's first read-back)
}

// ---------------------------------------------------------------------------------------------------------------
// apply_gates (src/Apply/apply_gates.jl:46-98)
// ---------------------------------------------------------------------------------------------------------------
// Options, validation and the step schedule (gate_schedule.cpp: a function of the vertex lists alone); the schedule is then executed AHEAD of the device by
// the run-ahead driver (engine_runahead.cpp), which is handed the two kinds of step: a batch of gates of the list, a BP update.
template <class T> static void apply_gates_t(State* s, int ngates, const int32_t* nverts, const int32_t* verts, const double* mats,
                                             const tnqs_apply_opts* opts, const tnqs_bp_opts* bp, double* errs) {
    HIPCHK(hipSetDevice(s->device));
    tnqs_apply_opts ao; ao.maxdim = 0; ao.cutoff = -1; ao.normalize_tensors = 1; ao.sqrt_cutoff = -1; ao.update_cache = 1;
    if (opts) ao = *opts;
    std::vector<int> voff; std::vector<size_t> moff;
    validate_gates(*s, ngates, nverts, verts, voff, moff);
    if (errs) std::fill(errs, errs + ngates, 0.0);
    if (s->real_io) {       // adapt_gate (apply_gates.jl:41-44): a real gate takes the state's real type, a complex gate stays complex and promotes
        bool cplx = false;
        for (size_t k = 1; k < moff[ngates] && !cplx; k += 2) cplx = mats[k] != 0.0;
        if (cplx) s->real_io = false;
    }
    const GateSchedule steps = build_gate_schedule(*s->g, ngates, nverts, verts, ao.update_cache != 0);
    auto batch = [&](const GateStep& st, bool ahead) {
        std::vector<Gate1> b1; std::vector<Gate2> b2;
        for (int i = st.begin; i < st.end; ++i) {
            const int32_t* vs = verts + voff[i];
            if (nverts[i] == 1) b1.push_back(Gate1{vs[0], mats + moff[i]}); else b2.push_back(Gate2{vs[0], vs[1], mats + moff[i], i});
        }
        apply_one_site_batch<T>(s, b1, ao.normalize_tensors != 0, false);
        apply_two_site_batch<T>(s, b2, ao, errs, /*allow_spec=*/ahead);
        s->stats.n_batches += 1;
        soft_sync(s);
    };
    auto update = [&](int iters_before) { bp_update_t<T>(s, bp, nullptr, nullptr, /*optimistic=*/iters_before == 0, iters_before); };
    RunAhead run_ahead(s, steps, batch, update);
    run_ahead.run();
    if (s->sharded()) materialize_pending_all(s);      // sharded: nothing stays pending between calls (State::in_apply)
    sync(s);                                                                                        // the call returns with the stream drained
}

void apply_gates(State* s, int ngates, const int32_t* nverts, const int32_t* verts, const double* mats,
                 const tnqs_apply_opts* opts, const tnqs_bp_opts* bp, double* errs) {
    s->stats = tnqs_apply_stats{};
    if (s->dtype == TNQS_C64) apply_gates_t<float>(s, ngates, nverts, verts, mats, opts, bp, errs);
    else apply_gates_t<double>(s, ngates, nverts, verts, mats, opts, bp, errs);
}

// ---------------------------------------------------------------------------------------------------------------
// truncate (src/truncate.jl:12-38)
// ---------------------------------------------------------------------------------------------------------------
template <class T> static void truncate_t(State* s, int maxdim, double cutoff, int normalize, int ngroups, const int32_t* offs,
                                          const int32_t* eu, const int32_t* ev, const tnqs_bp_opts* bp) {
    const Graph& g = *s->g;
    HIPCHK(hipSetDevice(s->device));
    if (maxdim <= 0) throw Err(TNQS_ERR_INVALID, "truncate: maxdim must be a positive integer");
    tnqs_apply_opts ao; ao.maxdim = maxdim; ao.cutoff = cutoff; ao.normalize_tensors = normalize; ao.sqrt_cutoff = -1; ao.update_cache = 1;
    std::vector<std::vector<double>> idmats;
    auto ident = [&](int dd) { std::vector<double> m(2 * (size_t)dd * dd, 0.0); for (int i = 0; i < dd; ++i) m[2 * (size_t)(i + (size_t)dd * i)] = 1.0; return m; };
    auto run_group = [&](const std::vector<std::pair<int, int>>& edges) {
        std::vector<Gate2> b2; std::set<int> seen; idmats.clear(); idmats.reserve(edges.size());
        for (auto& pr : edges) {
            int e = g.edge(pr.first, pr.second);
            if (e < 0) throw Err(TNQS_ERR_INVALID, "truncate: colour group contains a non-edge");
            if (s->chi[e] == 1) continue;                                   // truncatable_edge (:5-10)
            if (seen.count(pr.first) || seen.count(pr.second)) throw Err(TNQS_ERR_INVALID, "truncate: edges of one colour group must be vertex-disjoint");
            seen.insert(pr.first); seen.insert(pr.second);
            idmats.push_back(ident(s->d[pr.first] * s->d[pr.second]));
            b2.push_back(Gate2{pr.first, pr.second, idmats.back().data(), 0});
        }
        apply_two_site_batch<T>(s, b2, ao, nullptr);
        if (!b2.empty()) s->stats.n_batches += 1;
        bp_update_t<T>(s, bp, nullptr, nullptr);                               // :28 / :34
    };
    if (ngroups > 0) {
        for (int c = 0; c < ngroups; ++c) {
            std::vector<std::pair<int, int>> edges;
            for (int i = offs[c]; i < offs[c + 1]; ++i) edges.push_back({eu[i], ev[i]});
            run_group(edges);
        }
    } else {
        for (int e = 0; e < g.ne; ++e) run_group({{g.esrc[e], g.edst[e]}});
    }
    sync(s);
}
void truncate_bp(State* s, int maxdim, double cutoff, int normalize, int ngroups, const int32_t* offs,
                 const int32_t* eu, const int32_t* ev, const tnqs_bp_opts* bp) {
    s->stats = tnqs_apply_stats{};
    if (s->dtype == TNQS_C64) truncate_t<float>(s, maxdim, cutoff, normalize, ngroups, offs, eu, ev, bp);
    else truncate_t<double>(s, maxdim, cutoff, normalize, ngroups, offs, eu, ev, bp);
}

}  // namespace tnqs
