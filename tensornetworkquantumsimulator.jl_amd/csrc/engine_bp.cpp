// engine_bp.cpp -- BP update (abstractbeliefpropagationcache.jl:223-259): the sweep driver and the launches of one level.  The sweep order and its level
// schedule (BPPlan) are host graph code of their own: bp_schedule.cpp.
#include "engine_internal.hpp"
#include "launch_util.hpp"

namespace tnqs {

// can the last absorption of a BP message be fused into the Gram?  (c64, d = 2, the first row leg r has chi_r = 32,
// kept leg <= 32, tiles of 64 fibers = (s, i_r) aligned)
static int fused_leg(const State* s, const SD& sd, int jo) {
    if (s->dtype != TNQS_C64 || !use_mfma() || sd.d != 2 || sd.z < 2) return -1;
    int r = (jo == 0) ? 1 : 0;
    if (sd.chi[r] != 32 || sd.chi[jo] > 32 || sd.chi[jo] < 8) return -1;
    return r;
}

static double default_tol(const State* s) { return s->dtype == TNQS_C64 ? 1e-5 : 1e-8; }   // beliefpropagationcache.jl:104-108
static bool small_site_on() { static const bool v = !envflag("TNQS_NO_SMALL_SITE_BP"); return v; }

// ---- shared pair products ---------------------------------------------------------------------------------------
// A degree-4 site sends four messages per sweep, each needing the other three incoming messages absorbed.  Its legs are
// split into two pairs {A, B} by the level at which their outgoing message is computed; for an outgoing leg in A the pair
// product T_B = psi x m_b1 x m_b2 is shared with the other leg of A (the messages entering through B do not change between
// the two levels of A in the level-scheduled sequences), so a sweep costs 2 pair products + 4 (absorb + Gram) passes instead of
// 4 + 4.  Validity is not assumed but checked: an entry is reused only while the very same site / message buffers are current.
struct SharedT { Buf site, ma, mb, T; int la = -1, lb = -1; };

// ---- partial products kept ACROSS levels (sites the plane kernels of the bulk shape do not cover) -------------------------------------
// A message leaving a site absorbs the messages on all its other legs; which of them are absorbed in two-leg passes and which one inside
// the Gram pass is free.  Two facts make most of those passes redundant on lattices whose forests are straight lines: (i) the levels of one
// axis (a path and the edge that closes it on a periodic lattice) need the SAME product over the other axes' legs -- only messages along
// the axis change in between; (ii) the products of two axes share the factor over the third axis' legs.  So every product a chain writes
// (the final one and the one before it: the ping-pong buffers are both intact) is remembered with the exact buffers it was built from,
// and a later chain continues from the largest remembered product whose (leg, message buffer) pairs are a subset of what it needs.
// Legs are absorbed most-stable first (the messages that stay unchanged for the most levels to come), so that the early products are the
// reusable ones and the leg whose message changes next is left for the Gram pass.  Validity is by buffer identity, never assumed: the
// entries hold references, so an address cannot be recycled while an entry names it.  3 x 3 x 3 periodic cubic lattice, chi = 16: 5
// two-leg passes per site and sweep instead of 6.8.
typedef std::vector<std::pair<int, Buf>> LegBufs;        // (leg, the message buffer absorbed through it)
struct ProdEntry { Buf site; LegBufs legs; Buf prod; long long next_use = 0; };
// `want` without the legs of `have`, order kept
static void drop_legs(LegBufs& want, const LegBufs& have) {
    LegBufs rest; for (auto& w : want) { bool in = false; for (auto& b : have) in = in || b.first == w.first; if (!in) rest.push_back(w); }
    want.swap(rest);
}
struct SweepClock { int level = 0, iter = 1, maxiter = 1; };      // where the update stands: level of the schedule, sweep of the call (1-based), sweeps the call may run
// Which entries stay is decided by the level schedule, which is known in advance (round 5; least-recently-used before): `next_use` = the level, counted
// through the sweeps, at which the site next sends a message that can continue from the entry while every message it was built from is still current
// (next_use below).  A product without such a level is not stored at all, an entry that has served its last use is dropped when it is found,
// and what has to go -- more than `per_site` entries of a site, more bytes than `cap` -- is the entry whose next use is farthest away.
struct ProdCache {
    const BPPlan& plan; const SweepClock& at;              // the schedule and the update's position in it (BpUpdate)
    std::unordered_map<int, std::vector<ProdEntry>> by_site; int per_site = 3; size_t bytes = 0, cap = bp_cache_budget();
    int n_hits = 0, n_evicted = 0;          // diagnostics (tnqs_apply_stats): lookups that found a product; entries dropped by the per-site or the byte bound
    ProdCache(const BPPlan& p, const SweepClock& c) : plan(p), at(c) {}
    // the level (counted through the sweeps of this call) at which site v next sends a message that can continue from a product over `legs`: a message through
    // a leg outside `legs`, in a level where v sends nothing through a leg of `legs`, no later than the first level that recomputes a message entering through
    // `legs` (a message recomputed in the very level of the use is still read in its old value there).  -1: no such level
    long long next_use(int v, const LegBufs& legs) const {
        if (plan.in_place) return 0;
        const std::vector<int>& out_level = plan.out_level[v]; const std::vector<int>& in_level = plan.in_level[v];
        const int Lc = at.level, z = (int)out_level.size();
        auto has = [&](int j) { for (auto& lm : legs) if (lm.first == j) return true; return false; };
        int life = INT_MAX;
        for (auto& lm : legs) { const int L = in_level[lm.first]; if (L < 0) continue; life = std::min(life, plan.levels_until(L, Lc)); }
        int best = INT_MAX;
        for (int j = 0; j < z; ++j) {
            const int L = out_level[j]; if (L < 0 || has(j)) continue;
            const int d = plan.levels_until_next(L, Lc);
            if (d > life || d >= best) continue;
            bool clash = false; for (int j2 = 0; j2 < z; ++j2) if (out_level[j2] == L && has(j2)) clash = true;
            if (!clash) best = d;
        }
        if (best == INT_MAX) return -1;
        if (Lc + best >= plan.nlev && at.iter >= at.maxiter) return -1;              // the use lies in a sweep that will not happen
        return (long long)(at.iter - 1) * plan.nlev + Lc + best;
    }
    // the largest entry of site v whose legs all occur in `want` with the same buffer; returns false when there is none
    bool find(int v, const Buf& site, const LegBufs& want, ProdEntry& out) {
        auto it = by_site.find(v); if (it == by_site.end()) return false;
        ProdEntry* best = nullptr;
        for (auto& e : it->second) {
            if (e.site != site || (best && e.legs.size() <= best->legs.size())) continue;
            bool sub = true;
            for (auto& lm : e.legs) { bool f = false; for (auto& w : want) if (w.first == lm.first && w.second == lm.second) { f = true; break; } if (!f) { sub = false; break; } }
            if (sub) best = &e;
        }
        if (!best) return false;
        out = *best; ++n_hits;
        const long long nu = next_use(v, best->legs);
        if (nu < 0) { bytes -= best->prod->bytes; it->second.erase(it->second.begin() + (best - it->second.data())); }      // its last use: the caller holds the buffer
        else best->next_use = nu;
        return true;
    }
    void put(int v, const Buf& site, LegBufs legs, const Buf& prod) {
        if (legs.size() < 2 || !prod) return;
        std::sort(legs.begin(), legs.end(), [](const std::pair<int, Buf>& a, const std::pair<int, Buf>& b) { return a.first < b.first; });
        const long long nu = next_use(v, legs);
        if (nu < 0) return;
        auto& vec = by_site[v];
        for (auto& e : vec) if (e.site == site && e.legs == legs) { bytes += prod->bytes; bytes -= e.prod->bytes; e.prod = prod; e.next_use = nu; return; }
        if ((int)vec.size() >= per_site) {
            size_t far = 0; for (size_t i = 1; i < vec.size(); ++i) if (vec[i].next_use > vec[far].next_use) far = i;
            if (vec[far].next_use <= nu) return;                                       // everything kept is needed sooner than the new product
            bytes -= vec[far].prod->bytes; vec.erase(vec.begin() + (std::ptrdiff_t)far); ++n_evicted;
        }
        ProdEntry e; e.site = site; e.legs = std::move(legs); e.prod = prod; e.next_use = nu; bytes += prod->bytes; vec.push_back(std::move(e));
        if (bytes > cap) {                         // over the byte bound: the entries needed last go, in ONE pass -- down to 7/8 of the bound, so that a long
            // level under memory pressure does not rescan every entry for every product it stores (round-3 advisor finding)
            std::vector<std::pair<long long, int>> order;          // (next use, site)
            for (auto& kv : by_site) for (auto& en : kv.second) order.push_back({en.next_use, kv.first});
            std::sort(order.begin(), order.end(), [](const std::pair<long long, int>& a, const std::pair<long long, int>& b) { return a.first > b.first; });
            const size_t target = cap - cap / 8;
            for (auto& o : order) {
                if (bytes <= target) break;
                auto& vv = by_site[o.second];
                for (size_t i = 0; i < vv.size(); ++i) if (vv[i].next_use == o.first) { bytes -= vv[i].prod->bytes; vv.erase(vv.begin() + (std::ptrdiff_t)i); ++n_evicted; break; }
            }
        }
    }
};

// ---------------------------------------------------------------------------------------------------------------
// BP update  (abstractbeliefpropagationcache.jl:223-259; Gauss-Seidel over edge_sequence, executed level by level)
// ---------------------------------------------------------------------------------------------------------------
enum class BpVerdict { Continue, Converged, Deferred };

// What lives for the whole call: the plan, the options resolved once, the message buffers, the products shared between levels.
template <class T> struct BpUpdate {
    State* const s; const Graph& g; const BPPlan& plan;
    const size_t esz, nseq;
    const int normalize, iters_before;
    double tol; bool compute_error, cache_on, bra_on, go_optimistic;
    Buf d_diffs, d_sum;                        // message_diff of every position of the sequence; their sum
    std::vector<Buf> cur;                      // the messages as of the last finished sweep
    // shared pair products (see SharedT): partner[v][j] = the leg paired with j, -1 when the site is not covered
    std::vector<std::array<int, 4>> partner; std::vector<std::array<SharedT, 2>> tshare;
    SweepClock at; ProdCache pcache;
    std::vector<Buf> fresh;                    // the messages this sweep has computed so far
    int niter; double avg = 0; bool converged = false;

    BpUpdate(State* st, const BPPlan& p, const tnqs_bp_opts* o, bool optimistic, int iters_before_)
        : s(st), g(*st->g), plan(p), esz(st->esz()), nseq(p.seq.size()), normalize(o ? o->normalize : 1), iters_before(iters_before_), pcache(p, at) {
        at.maxiter = (o && o->maxiter > 0) ? o->maxiter : (g.is_tree ? 1 : 25);                  // :39,:103
        if (!o || std::isnan(o->tolerance)) tol = g.is_tree ? -1.0 : default_tol(s); else tol = o->tolerance;
        compute_error = tol >= 0;
        d_diffs = dalloc(s, nseq * sizeof(double));
        d_sum = dalloc(s, sizeof(double));
        cur = s->msg;
        niter = at.maxiter;
        pair_up_legs();
        {   // never more than a third of what the device has free right now (the products are an optimisation, the workspace is not)
            size_t fr = 0, tot = 0;
            if (hipMemGetInfo(&fr, &tot) == hipSuccess) pcache.cap = std::min(pcache.cap, (fr + s->pool->bytes_cached()) / 3);
        }
        cache_on = use_prodcache() && !plan.in_place;
        bra_on = use_bra_products() && s->msg_hermitian && !plan.in_place;
        // (sharded handles too, round 5: messages are replicated and every rank normalises / diffs all of them, so the verdict is the same on every rank)
        go_optimistic = optimistic && speculation_on() && compute_error && iters_before == 0;
    }
    ~BpUpdate() { s->stats.n_bp_products_reused += pcache.n_hits; s->stats.n_bp_products_evicted += pcache.n_evicted; }

    // degree-4 sites with four 32-dimensional legs: the legs paired by the level at which their outgoing message is computed
    void pair_up_legs() {
        partner.assign(g.nv, std::array<int, 4>{{-1, -1, -1, -1}});
        if (!(std::is_same<T, float>::value && use_mfma() && use_pair())) return;
        tshare.resize(g.nv);
        for (int v = 0; v < g.nv; ++v) {
            if (!s->owns(v) || g.nbr[v].size() != 4 || s->d[v] != 2) continue;
            bool ok = true; std::array<std::pair<int, int>, 4> ord;
            for (int j = 0; j < 4; ++j) {
                if (s->chi[g.nbr_e[v][j]] != 32) ok = false;
                ord[j] = {plan.out_level[v][j] >= 0 ? plan.out_level[v][j] : INT_MAX, j};
            }
            if (!ok) continue;
            std::sort(ord.begin(), ord.end());
            partner[v][ord[0].second] = ord[1].second; partner[v][ord[1].second] = ord[0].second;
            partner[v][ord[2].second] = ord[3].second; partner[v][ord[3].second] = ord[2].second;
        }
    }
    // THE Gauss-Seidel rule: the version of the message entering src through leg j that position t of the sequence reads -- this sweep's when it was computed at
    // an earlier position (in place: whenever there is one), the last sweep's otherwise.  Null: unset = identity
    const Buf& incoming(int src, int j, int t) const {
        const int din = g.dedge(g.nbr[src][j], src), pp = plan.pos_of[din];
        return ((plan.in_place || (pp >= 0 && pp < t)) && fresh[din]) ? fresh[din] : cur[din];
    }
    // small sites (<= 8192 elements, ComplexF32): the whole message in ONE kernel with the tensor resident in LDS (kernels_bp.hip bp_small_site_kernel);
    // TNQS_NO_SMALL_SITE_BP=1: the generic chain + Gram route
    bool small_site(const SD& sd) const {
        return small_site_on() && std::is_same<T, float>::value && sd.n >= 64 && bp_small_site_covers(sd.d, sd.z, sd.chi.data(), sd.n);
    }
    // the legs whose messages stay unchanged for the most levels to come first
    void by_stability(LegBufs& w, int src, int t) const {
        std::stable_sort(w.begin(), w.end(), [&](const std::pair<int, Buf>& a, const std::pair<int, Buf>& b) { return plan.horizon(src, a.first, t) > plan.horizon(src, b.first, t); });
    }
    // every product a chain wrote that is still intact (its last two passes), with the buffers it was built from
    void remember(const Chain& c, const Buf& site, const LegBufs& base, const LegBufs& absorbed) {
        const int np = (int)c.trail.size();
        LegBufs acc = base;
        for (int k = 0; k < np; ++k) {
            for (int leg : c.trail[k]) for (auto& lm : absorbed) if (lm.first == leg) { acc.push_back(lm); break; }
            if (k >= np - 2 && c.tmp[k & 1]) pcache.put(c.v, site, acc, c.tmp[k & 1]);
        }
    }
    void sweep(int iter);
    // after a sweep: Converged / Continue from the blocking read-back of the summed diffs -- or Deferred: the verdict travels to a pinned slot and stays a Check
    // (engine.hpp), the messages are committed and the caller goes on enqueuing meanwhile
    BpVerdict verdict(int iter) {
        if (!compute_error) return BpVerdict::Continue;
        launch_sum_doubles(s->stream, reinterpret_cast<const double*>(d_diffs->p), (int)nseq, reinterpret_cast<double*>(d_sum->p));
        if (go_optimistic) {
            double* slot = reinterpret_cast<double*>(ring_alloc(s, sizeof(double)));       // (may settle older checks -- and throw -- first: nothing is committed yet)
            const size_t nseq_ = nseq; const int maxiter_ = at.maxiter; const double tol_ = tol;
            post_check(s, reinterpret_cast<char*>(slot), d_sum->p, sizeof(double), /*kind=*/1, s->cur_step, iter, [slot, tol_, nseq_, iter, maxiter_](State* st) {
                const double a = *slot / (double)nseq_;
                st->stats.last_bp_diff = a;
                if (a <= tol_) return true;
                if (iter >= maxiter_) { st->stats.bp_not_converged += 1; return true; }      // the reference stops here too (and warns)
                return false;
            });
            s->keepalive.push_back(d_diffs); s->keepalive.push_back(d_sum);
            s->msg = cur; s->stats.n_bp_updates += 1;
            soft_sync(s);
            return BpVerdict::Deferred;
        }
        const double* st_tot = readback<double>(s, d_sum->p, 1);
        sync(s);
        const double tot = *st_tot;                                  // (the arena's memory is untouched until the next upload)
        settle(s, true);                                             // (the stream is drained: whatever was pending has fired; a failed check unwinds this update, s->msg is untouched)
        avg = tot / (double)nseq;
        if (avg <= tol) { converged = true; niter = iter; return BpVerdict::Converged; }
        return BpVerdict::Continue;
    }
    void commit(int* niter_out, double* diff_out) {
        sync(s);
        settle(s, true);
        s->msg = cur;
        if (iters_before == 0) s->stats.n_bp_updates += 1;
        if (compute_error && !converged) s->stats.bp_not_converged += 1;
        s->stats.last_bp_diff = avg;
        if (niter_out) *niter_out = niter;
        if (diff_out) *diff_out = compute_error ? avg : -1.0;
    }
};

// One workspace-bounded sub-batch of a level: its messages are independent of each other.  The phases, in order: take the extent, build the products several
// messages of a site share, route every message to the kernels that compute its Gram, pair up the chi = 16 plane items, launch, finalize.
template <class T> struct BpLevelBatch {
    // the kernels that compute a message's Gram matrix
    enum class Route { Small,              // the whole message in one LDS-resident kernel
                       Pair32Single,       // chi = 32 bulk site: shared pair product, then last absorption + Gram on a plane (one message per item)
                       Pair32Double,       // the same with the partner message of the forest in one pass
                       Plane16Double,      // chi = 16: two messages of a site continuing from one shared product, one pass over (T, psi)
                       Plane16Single,      // chi = 16: the chain stops one leg early, that leg is absorbed in the Gram pass
                       GenericFused,       // chain, then the Gram kernel that absorbs the first row leg itself
                       GenericPlain };     // chain, then the plain Gram
    struct Msg { int t, src, jo; Route route; const void* fused = nullptr; int item = -1; };     // fused: message of the leg absorbed inside the generic Gram kernel; item: its entry in pair32_items
    struct Prefix { Buf site; std::vector<std::pair<int, const void*>> legs; Buf prod, bra; bool has_bra = false; };      // legs: of both products
    struct Pend { int msg, jo, r; };                                                                // first message of a (site, T) seen in this level
    struct Continued { LegBufs base, absorbed; };      // legs of the remembered product a chain starts from / legs it absorbs

    BpUpdate<T>& u; State* const s; const Graph& g; const BPPlan& plan; const std::vector<int>& lev; const size_t start, esz; size_t end;
    std::vector<Msg> msgs; std::vector<Chain> chains;         // index-aligned (run_chains takes the plain vector); a routed message's chain may be empty
    // chain index -> what to remember of it.  Kept a hash map, iterated as one: the order of the puts decides what the cache's bounds evict (ProdCache::put),
    // and it has been this map's order since the cache exists
    std::unordered_map<size_t, Continued> continued;
    std::vector<PairItem> sh_pair; std::vector<PairGramItem> pair32_items;                          // shared-T path; pair32_items: one per message routed there, doubles included
    std::vector<PairGram2Item> sh_dbl; std::vector<std::pair<int, int>> sh_dbl_msg;              // both messages of a forest in one pass
    std::vector<SmallMsgItem> small_items; std::vector<int> small_msg; int small_max = 0;
    std::unordered_map<long long, Pend> pend;
    double sh_pair_slices = 0, sh_dbl_slices = 0;
    std::unordered_map<int, Prefix> prefix;
    std::vector<Buf> hits_alive;          // remembered products this sub-batch continues from: the cache may drop its entry (last use, or the byte bound) before the launches
    std::vector<PairGram2x16Item> g16; std::vector<std::pair<int, int>> g16_msg;       // (message through ly, through lx; -1: a single item)
    std::vector<int> g16_single;                          // index into g16 of the single items (their chain runs first, X is set after it)
    hipStream_t main_stream = nullptr, side_stream = nullptr; bool split_level = false;
    std::vector<size_t> slot;                                 // (sharded) offset of message q - start inside its owner's block of the exchange buffer
    std::vector<GramJob> jobs;                                // index-aligned with msgs, filled after the chains have run

    BpLevelBatch(BpUpdate<T>& up, const std::vector<int>& level, size_t first)
        : u(up), s(up.s), g(up.g), plan(up.plan), lev(level), start(first), esz(up.esz), end(first) {}
    // the byte-bounded extent [start, end) of the level
    void take() {
        const size_t budget = bp_ws_budget(); size_t used = 0;
        while (end < lev.size()) {
            const size_t need = 2 * site_dims(s, g.src_of(plan.seq[lev[end]])).n * esz;
            if (end > start && used + need > budget) break;
            used += need; ++end;
        }
    }
    static bool generic(Route r) { return r == Route::GenericFused || r == Route::GenericPlain; }

    // continue chain c from the largest remembered product over a subset of `want`: c reads the product, `want` keeps what is left to absorb
    bool continue_from_remembered(Chain& c, LegBufs& want, LegBufs& base) {
        ProdEntry hit;
        if (!u.pcache.find(c.v, s->site[c.v], want, hit)) return false;
        base = hit.legs; c.src = hit.prod->p; hits_alive.push_back(hit.prod);
        drop_legs(want, base);
        return true;
    }

    // ---- shared partial products for the sites the plane kernels do not cover (any degree, any bond dimension): a site that sends
    // several messages in this level absorbs the messages on its OTHER legs once (T = psi x_{legs not going out here} m) and every
    // outgoing message continues from T.  With the default linear-forest order a site sends two messages per level, so a degree-6
    // site does 4 + 2 x 1 absorption passes per level instead of 2 x 5.  Reuse is decided by buffer identity per message (the
    // Gauss-Seidel rule may give two messages of a site different versions of an incoming message), never assumed.
    void shared_prefixes() {
        if (plan.in_place) return;
        std::unordered_map<int, std::vector<int>> outl;            // source site -> legs going out in this sub-batch
        auto generic_site = [&](int src, int jo) { const SD sd = site_dims(s, src); return (u.tshare.empty() || sd.z != 4 || u.partner[src][jo] < 0) && !u.small_site(sd); };
        for (size_t q = start; q < end; ++q) {
            const int de = plan.seq[lev[q]], src = g.src_of(de), jo = g.leg(src, g.dst_of(de));
            if (s->owns(src) && generic_site(src, jo)) outl[src].push_back(jo);
        }
        std::vector<Chain> pch; std::vector<int> psrc, pside; std::vector<LegBufs> pbase, pabs;
        // one product of the level: the legs `w` of site src absorbed into psi (continuing from a remembered product when there is one); side 1 = the bra product
        auto start_product = [&](int src, LegBufs w, int side) {
            Prefix& pf = prefix[src];
            Chain cp; cp.v = src; cp.src = s->site[src]->p; cp.sd = site_dims(s, src);
            LegBufs base;
            if (u.cache_on) {
                cp.ordered = true;
                if (continue_from_remembered(cp, w, base)) (side ? pf.bra : pf.prod) = hits_alive.back();      // (the product itself when nothing is left to absorb)
            }
            for (auto& x : w) cp.steps.push_back({x.first, x.second->p});
            if (cp.steps.empty()) return;                                              // the whole product was remembered
            pch.push_back(std::move(cp)); psrc.push_back(src); pside.push_back(side); pbase.push_back(std::move(base)); pabs.push_back(std::move(w));
        };
        for (size_t q = start; q < end; ++q) {
            const int t = lev[q], src = g.src_of(plan.seq[t]);
            auto ol = outl.find(src);
            if (ol == outl.end() || ol->second.size() < 2 || prefix.count(src)) continue;
            const SD sd = site_dims(s, src);
            Prefix pf; pf.site = s->site[src];
            LegBufs want;
            for (int j = 0; j < sd.z; ++j) {
                if (std::find(ol->second.begin(), ol->second.end(), j) != ol->second.end()) continue;
                const Buf& mb = u.incoming(src, j, t);
                if (!mb) continue;
                want.push_back({j, mb});
            }
            if (want.empty()) continue;
            if (u.cache_on || u.bra_on) u.by_stability(want, src, t);
            // ---- half of the messages on the BRA side (round 6).  m_out = sum (psi x_K m_k x_B m_b) conj(psi) with the messages of the legs B moved over:
            // sum_b' m[b][b'] conj(psi[b']) = conj(sum_b' psi[b'] m[b'][b]) for a Hermitian m, i.e. conj(psi x_B m_b) -- the SAME two-leg product a ket
            // side would use.  So the Gram pass takes X = psi x_K m_k and Y = psi x_B m_b, both one pass away from psi, instead of X = a product over
            // K and B (two passes deep) and Y = psi; and the halves are split by how long their messages stay unchanged (an axis of a lattice each), so
            // that the product over an axis is built once per sweep and serves first as the ket, then as the bra factor of the other axes' levels: a
            // degree-6 site does 3 two-leg passes per sweep instead of 5.  Messages are Hermitian to rounding by construction (State::msg_hermitian).
            const size_t nket = (u.bra_on && want.size() >= 4) ? (want.size() + 1) / 2 : want.size();
            for (size_t i = 0; i < want.size(); ++i) pf.legs.push_back({want[i].first, want[i].second->p});
            prefix[src] = pf;
            start_product(src, LegBufs(want.begin(), want.begin() + (std::ptrdiff_t)nket), 0);
            if (nket < want.size()) { prefix[src].has_bra = true; start_product(src, LegBufs(want.begin() + (std::ptrdiff_t)nket, want.end()), 1); }
        }
        if (pch.empty()) return;
        run_chains<T>(s, pch, TNQS_PROF_BP_MODEPROD, TNQS_PROF_BP_PAIR);
        for (size_t i = 0; i < pch.size(); ++i) {
            Prefix& pf = prefix[psrc[i]];
            for (int k = 0; k < 2; ++k) if (pch[i].tmp[k] && pch[i].tmp[k]->p == pch[i].result) (pside[i] ? pf.bra : pf.prod) = pch[i].tmp[k];
            if (u.cache_on) u.remember(pch[i], pf.site, pbase[i], pabs[i]);
        }
    }

    // ---- one route per message --------------------------------------------------------------------------------------------------------------
    void route_messages() {
        for (size_t q = start; q < end; ++q) {
            const int t = lev[q], de = plan.seq[t], src = g.src_of(de);
            if (!s->owns(src)) continue;
            Chain c; c.v = src; c.src = s->site[src]->p; c.sd = site_dims(s, src);
            Msg m{}; m.t = t; m.src = src; m.jo = g.leg(src, g.dst_of(de));
            if (u.small_site(c.sd)) route_small(m, c);
            else if (!route_pair32(m, c)) route_generic(m, c);
            msgs.push_back(m); chains.push_back(std::move(c));
        }
    }
    // small site: one kernel for the whole message (no shared products, no remembered ones: nothing of the generic bookkeeping applies)
    void route_small(Msg& m, const Chain& c) {
        SmallMsgItem si{}; si.psi = c.src; si.d = c.sd.d; si.z = c.sd.z; si.jo = m.jo;
        for (int j = 0; j < c.sd.z; ++j) {
            si.chi[j] = c.sd.chi[j]; si.M[j] = nullptr;
            if (j == m.jo) continue;
            const Buf& mb = u.incoming(m.src, j, m.t);
            if (mb) si.M[j] = mb->p;                 // unset message = identity: nothing to absorb
        }
        si.mfma = bp_small_site_mfma_form(c.sd.z, c.sd.chi.data(), c.sd.n) ? 1 : 0;
        small_items.push_back(si); small_msg.push_back((int)msgs.size()); small_max = std::max(small_max, (int)c.sd.n);
        m.route = Route::Small;
    }
    // degree-4 site with 32-dimensional legs: the pair product over the two legs of the OTHER pair (shared with the partner message), then the partner leg absorbed
    // inside the Gram pass.  false: the site is not covered, or a message is unset -- the generic route
    bool route_pair32(Msg& m, const Chain& c) {
        const int src = m.src, jo = m.jo;
        if (u.tshare.empty() || c.sd.z != 4 || u.partner[src][jo] < 0) return false;
        const int r = u.partner[src][jo];
        int pa = -1, pb = -1;
        for (int j = 0; j < 4; ++j) if (j != jo && j != r) { if (pa < 0) pa = j; else pb = j; }
        const Buf& ma = u.incoming(src, pa, m.t); const Buf& mb = u.incoming(src, pb, m.t); const Buf& mr = u.incoming(src, r, m.t);
        PairGramItem gi{}; PairItem pi{};
        if (!(ma && mb && mr && pair_geometry(c.sd.d, c.sd.z, c.sd.chi.data(), pa, pb, pi.g) && pair_geometry(c.sd.d, c.sd.z, c.sd.chi.data(), r, jo, gi.g))) return false;
        const int slot = std::min(pa, pb) < std::min(r, jo) ? 0 : 1;      // slot of the pair {pa, pb}
        SharedT& sh = u.tshare[src][slot];
        if (!(sh.T && sh.site == s->site[src] && sh.ma == ma && sh.mb == mb && sh.la == pa && sh.lb == pb)) {
            sh.site = s->site[src]; sh.ma = ma; sh.mb = mb; sh.la = pa; sh.lb = pb;
            sh.T = dalloc(s, c.sd.n * esz);
            pi.in = c.src; pi.out = sh.T->p; pi.Mx = ma->p; pi.My = mb->p;
            sh_pair.push_back(pi); sh_pair_slices += (double)c.sd.n / 16384.0;
        }
        gi.X = sh.T->p; gi.Y = c.src; gi.M = mr->p;
        m.item = (int)pair32_items.size(); pair32_items.push_back(gi);
        const long long key = ((long long)src << 1) | slot;
        auto pit = pend.find(key);
        if (pit != pend.end() && pit->second.jo == r && pit->second.r == jo && pair32_items[msgs[pit->second.msg].item].X == gi.X) {
            // the partner message of the same forest is in this level too: one pass computes both
            Msg& mf = msgs[pit->second.msg]; const PairGramItem& first = pair32_items[mf.item];       // plane (lx = r_first = jo, ly = jo_first = r)
            PairGram2Item d2{}; d2.X = first.X; d2.Y = first.Y; d2.Mx = first.M; d2.My = gi.M; d2.g = first.g;
            sh_dbl.push_back(d2); sh_dbl_msg.push_back({pit->second.msg, (int)msgs.size()});
            sh_dbl_slices += (double)c.sd.n / 8192.0;
            mf.route = m.route = Route::Pair32Double;
            pend.erase(pit);
        } else {
            pend[key] = Pend{(int)msgs.size(), jo, r};
            m.route = Route::Pair32Single;
        }
        return true;
    }
    // any site: a chain of mode products (continuing from this level's shared product or from a remembered one), then a Gram
    void route_generic(Msg& m, Chain& c) {
        const int src = m.src, jo = m.jo, t = m.t;
        const int fr = fused_leg(s, c.sd, jo);
        std::vector<char> done(c.sd.z, 0);                   // legs already absorbed in the shared partial product
        {
            auto pf = prefix.find(src);
            if (pf != prefix.end() && pf->second.prod && (!pf->second.has_bra || pf->second.bra) && pf->second.site == s->site[src]) {
                bool same = true;
                for (auto& lm : pf->second.legs) { if (lm.first == jo) { same = false; break; } const Buf& mb = u.incoming(src, lm.first, t); if (!mb || mb->p != lm.second) { same = false; break; } }
                if (same) { c.y = pf->second.has_bra ? pf->second.bra->p : c.src; c.src = pf->second.prod->p; for (auto& lm : pf->second.legs) done[lm.first] = 1; }
            }
        }
        LegBufs want, base;
        for (int j = 0; j < c.sd.z; ++j) {
            if (j == jo || done[j]) continue;
            const Buf& mb = u.incoming(src, j, t);
            if (!mb) continue;                               // unset message = identity: nothing to absorb
            want.push_back({j, mb});
        }
        const bool from_prefix = c.y != nullptr;             // continues from this level's shared product: that product is remembered, not what follows
        if (u.cache_on && !from_prefix) {
            u.by_stability(want, src, t); c.ordered = true;
            const void* psi = c.src;
            if (continue_from_remembered(c, want, base)) c.y = psi;
        }
        for (auto& w : want) {
            if (w.first == fr) m.fused = w.second->p;        // absorbed inside the Gram kernel
            else c.steps.push_back({w.first, w.second->p});
        }
        if (u.cache_on && !from_prefix) continued[msgs.size()] = Continued{std::move(base), std::move(want)};
        m.route = m.fused ? Route::GenericFused : Route::GenericPlain;
    }

    // ---- 16-dimensional planes ----------------------------------------------------------------------------------------------------------------
    void pair_up_planes16() {
        if (!(std::is_same<T, float>::value && use_mfma() && use_pair())) return;
        // the two messages a site sends in this level, both continuing from the same shared product and each absorbing exactly the other's outgoing
        // leg, come from ONE pass over (T, psi) (mfma_pair_gram2x16_kernel)
        std::unordered_map<int, std::vector<int>> by_src;
        for (size_t ci = 0; ci < chains.size(); ++ci)
            if (chains[ci].y && chains[ci].steps.size() == 1 && !msgs[ci].fused && chains[ci].sd.n >= (size_t)(1u << 14)) by_src[chains[ci].v].push_back((int)ci);
        for (auto& kv : by_src) {
            if (kv.second.size() != 2) continue;
            const int ci = kv.second[0], cj = kv.second[1];
            Chain& a = chains[ci]; Chain& b = chains[cj];
            const int ly = msgs[ci].jo, lx = msgs[cj].jo;
            if (a.src != b.src || a.y != b.y || a.steps[0].first != lx || b.steps[0].first != ly) continue;
            PairGram2x16Item it{};
            if (!plane_geometry(a.sd.d, a.sd.z, a.sd.chi.data(), lx, ly, 16, it.g)) continue;
            it.X = a.src; it.Y = a.y; it.Mx = a.steps[0].second; it.My = b.steps[0].second;
            g16.push_back(it); g16_msg.push_back({ci, cj});
            a.steps.clear(); b.steps.clear();
            msgs[ci].route = msgs[cj].route = Route::Plane16Double;
        }
        // a site that sends ONE message in this level (no shared product): its last absorption is fused with the Gram too -- the chain
        // stops one leg early and the same kernel computes (T x_lx M) conj(psi) for that single message (My = null)
        for (size_t ci = 0; ci < chains.size(); ++ci) {
            Chain& c = chains[ci];
            if (!generic(msgs[ci].route)) continue;
            auto ct = continued.find(ci);
            if ((c.y && (ct == continued.end() || ct->second.base.empty())) || msgs[ci].fused || c.steps.empty() || (c.steps.size() & 1) == 0 || c.sd.n < (size_t)(1u << 14)) continue;
            const int ly = msgs[ci].jo, lx = c.steps.back().first;
            PairGram2x16Item it{};
            if (!plane_geometry(c.sd.d, c.sd.z, c.sd.chi.data(), lx, ly, 16, it.g)) continue;
            bool all16 = true; for (auto& st : c.steps) all16 = all16 && c.sd.chi[st.first] == 16;
            if (!all16) continue;
            it.Y = c.y ? c.y : c.src; it.Mx = c.steps.back().second; it.My = nullptr; it.X = nullptr;      // X = the chain's result, known after run_chains
            c.steps.pop_back();
            g16_single.push_back((int)g16.size());
            g16.push_back(it); g16_msg.push_back({(int)ci, -1});
            msgs[ci].route = Route::Plane16Single;
        }
    }

    // ---- launches.  Two independent launch chains make up a level: the bulk sites' plane kernels (pair product -> both-messages pair-Gram) and the other
    // sites' single-leg products -> Grams (boundary sites of a lattice: 24 of the 49 sites of a 7 x 7 one, small launches of 10-50 us each).
    // They meet in msg_finalize.  The second chain goes to the side stream, under the plane kernels (the chi = 16
    // pair-Gram items that continue from a chain's result keep everything on one stream); nothing released inside the region is handed out
    // again before the join (Pool::set_defer).
    struct SplitGuard { State* s; hipStream_t m; bool on; ~SplitGuard() { s->stream = m; if (on) s->pool->set_defer(false); } };
    void on_side(bool side) { if (split_level) { s->stream = side ? side_stream : main_stream; s->prof->chain = false; } }
    void fork() {
        main_stream = s->stream;
        bool has_other = false;              // (a chi = 16 single item counts as well, but then g16 is not empty and the level is not split anyway)
        for (const Msg& m : msgs) has_other = has_other || m.route == Route::Small || generic(m.route);
        split_level = (!sh_pair.empty() || !sh_dbl.empty()) && has_other && g16.empty();
        if (!split_level) return;
        side_stream = aux_stream_of(s);
        HIPCHK(hipEventRecord(s->ev_fork, main_stream)); HIPCHK(hipStreamWaitEvent(side_stream, s->ev_fork, 0));
        s->pool->set_defer(true);
    }
    void join() { if (split_level) { HIPCHK(hipEventRecord(s->ev_join, side_stream)); HIPCHK(hipStreamWaitEvent(main_stream, s->ev_join, 0)); } }

    // the bulk sites' pair products on the main stream, every chain next to them; then what the chains wrote is remembered and every message gets its Gram job
    void launch_products() {
        if (!sh_pair.empty()) {
            const int wgs = plan_pair(sh_pair.data(), (int)sh_pair.size());
            const PairItem* d = upload(s, sh_pair);
            ProfScope ps(s, TNQS_PROF_BP_PAIR, 2.0 * sh_pair_slices * 16384.0 * esz, 2 * 8.0 * sh_pair_slices * 16384.0 * 32);
            launch_mfma_pair(s->stream, d, (int)sh_pair.size(), wgs);
        }
        on_side(true);
        run_chains<T>(s, chains, TNQS_PROF_BP_MODEPROD, TNQS_PROF_BP_PAIR);
        on_side(false);
        if (u.cache_on) for (auto& kv : continued) if (!chains[kv.first].trail.empty()) u.remember(chains[kv.first], s->site[chains[kv.first].v], kv.second.base, kv.second.absorbed);
        for (size_t i = 0; i < chains.size(); ++i) {
            GramJob j{}; j.X = chains[i].result; j.Y = chains[i].y ? chains[i].y : chains[i].src; j.sd = chains[i].sd; j.leg = msgs[i].jo; j.keep_site = false;
            j.M = msgs[i].fused;
            jobs.push_back(j);
        }
    }
    void launch_small_sites() {
        if (small_items.empty()) return;
        size_t slab_bytes = 0;                   // one allocation for the raw messages of the level (views into it: a pool round trip per message otherwise)
        for (size_t q = 0; q < small_items.size(); ++q) { const int co = small_items[q].chi[small_items[q].jo]; slab_bytes += round256((size_t)co * co * esz); }
        Buf slab = dalloc(s, slab_bytes); size_t off = 0;
        for (size_t q = 0; q < small_items.size(); ++q) {
            GramJob& j = jobs[small_msg[q]];
            const int co = small_items[q].chi[small_items[q].jo];
            j.nchunks = 1; j.KK = co; j.partial = sub_buffer(slab, off, (size_t)co * co * esz); off += round256((size_t)co * co * esz);
            small_items[q].out = j.partial->p;
        }
        // matrix-core form on an unsharded handle: the kernel holds the whole message and finishes it (normalisation, message_diff) -- one launch less on
        // the critical path of the level
        if (!s->sharded() && !plan.in_place) {
            size_t nb_bytes = 0;
            for (size_t q = 0; q < small_items.size(); ++q) if (small_items[q].mfma) nb_bytes += round256((size_t)256 * esz);
            if (nb_bytes) {
                Buf nslab = dalloc(s, nb_bytes); size_t noff = 0;
                for (size_t q = 0; q < small_items.size(); ++q) {
                    SmallMsgItem& si = small_items[q]; if (!si.mfma) continue;
                    GramJob& j = jobs[small_msg[q]];
                    const int t = msgs[small_msg[q]].t; const int de = plan.seq[t];
                    j.final_msg = sub_buffer(nslab, noff, (size_t)256 * esz); noff += round256((size_t)256 * esz);
                    si.new_msg = j.final_msg->p; si.old_msg = u.cur[de] ? u.cur[de]->p : nullptr;
                    si.diff_out = reinterpret_cast<double*>(u.d_diffs->p) + t; si.normalize = u.normalize;
                }
            }
        }
        on_side(true);          // (with a split level: next to the bulk sites' plane kernels, like the other boundary-site work; the descriptor copy
                                //  travels on the same stream as the kernel that reads it)
        const SmallMsgItem* d = upload_small(s, small_items);          // (one workgroup per item reads its own descriptor: straight from the pinned arena)
        { ProfScope ps(s, TNQS_PROF_BP_FUSED, 0, 0); launch_bp_small_site(s->stream, d, (int)small_items.size(), small_max); }
        on_side(false);
    }
    // the one-message chi = 32 pair-Gram launch, in either form of its kernel: one partial per workgroup
    template <class Item, class PlanFn, class LaunchFn>
    void launch_pair32_singles(std::vector<Item>& items, void* Item::*partial, const std::vector<int>& of_msg, double slices, PlanFn plan_fn, LaunchFn launch_fn) {
        std::vector<int> nwg(items.size()); const int wgs = plan_fn(items.data(), (int)items.size(), nwg.data(), 0);
        for (size_t q = 0; q < items.size(); ++q) {
            GramJob& j = jobs[of_msg[q]];
            j.nchunks = nwg[q]; j.KK = 32; j.partial = dalloc(s, (size_t)j.nchunks * 1024 * esz);
            items[q].*partial = j.partial->p;
        }
        const Item* d = upload(s, items);
        ProfScope ps(s, TNQS_PROF_BP_PAIRGRAM, 2.0 * slices * 16384.0 * esz, 2 * 8.0 * slices * 16384.0 * 32);
        launch_fn(s->stream, d, (int)items.size(), wgs);
    }
    // the plane kernels' Grams: chi = 32 doubles, chi = 16 items, chi = 32 singles
    void launch_plane_grams() {
        if (!sh_dbl.empty()) {
            std::vector<int> nwg(sh_dbl.size()); const int wgs = plan_pair_gram2(sh_dbl.data(), (int)sh_dbl.size(), nwg.data());
            for (size_t q = 0; q < sh_dbl.size(); ++q) {
                PairGram2Item& it = sh_dbl[q]; GramJob& jy = jobs[sh_dbl_msg[q].first]; GramJob& jx = jobs[sh_dbl_msg[q].second];
                jy.nchunks = jx.nchunks = nwg[q]; jy.KK = jx.KK = 32;
                jy.partial = dalloc(s, (size_t)jy.nchunks * 1024 * esz); jx.partial = dalloc(s, (size_t)jx.nchunks * 1024 * esz);
                it.partial_y = jy.partial->p; it.partial_x = jx.partial->p;
            }
            const PairGram2Item* d = upload(s, sh_dbl);
            ProfScope ps(s, TNQS_PROF_BP_PAIRGRAM, 2.0 * sh_dbl_slices * 8192.0 * esz, 4 * 8.0 * sh_dbl_slices * 8192.0 * 32);
            launch_mfma_pair_gram2(s->stream, d, (int)sh_dbl.size(), wgs);
        }
        for (int q : g16_single) g16[q].X = chains[g16_msg[q].first].result;
        if (!g16.empty()) {
            std::vector<int> nwgs(g16.size()); const int wgs = plan_pair_gram2x16(g16.data(), (int)g16.size(), nwgs.data()); double by = 0, fl = 0;
            for (size_t q = 0; q < g16.size(); ++q) {
                PairGram2x16Item& it = g16[q]; GramJob& jy = jobs[g16_msg[q].first]; const int nwg = nwgs[q];
                jy.nchunks = nwg; jy.KK = 16; jy.partial = dalloc(s, (size_t)nwg * 256 * esz); it.partial_y = jy.partial->p;
                if (g16_msg[q].second >= 0) {
                    GramJob& jx = jobs[g16_msg[q].second];
                    jx.nchunks = nwg; jx.KK = 16; jx.partial = dalloc(s, (size_t)nwg * 256 * esz); it.partial_x = jx.partial->p;
                } else it.partial_x = nullptr;
                by += 2.0 * jy.sd.n * esz; fl += (g16_msg[q].second >= 0 ? 4 : 2) * 8.0 * jy.sd.n * 16;
            }
            const PairGram2x16Item* d = upload(s, g16);
            ProfScope ps(s, TNQS_PROF_BP_PAIRGRAM, by, fl);
            launch_mfma_pair_gram2x16(s->stream, d, (int)g16.size(), wgs);
        }
        // singles: the messages that were not merged into a double item.  (Slices: every term is a multiple of 1/16384 well inside the exact range of a
        // double, so the survivors' sum is what adding every message and taking the merged ones out again gave)
        std::vector<PairGramItem> singles; std::vector<int> single_msg; double slices = 0;
        for (size_t i = 0; i < msgs.size(); ++i) if (msgs[i].route == Route::Pair32Single) {
            singles.push_back(pair32_items[msgs[i].item]); single_msg.push_back((int)i); slices += (double)chains[i].sd.n / 16384.0;
        }
        if (singles.empty()) return;
        if (mfma_use_x3()) {
            // the bf16 kernel in its one-message form (round 5): half-slice workgroups in groups of 16.  These launches are what a
            // sweep in the reference's forest-cover order consists of (a handful of messages per dependency level)
            std::vector<PairGram2Item> one(singles.size());
            for (size_t q = 0; q < singles.size(); ++q) { const PairGramItem& a = singles[q]; one[q].X = a.X; one[q].Y = a.Y; one[q].Mx = a.M; one[q].g = a.g; }
            launch_pair32_singles(one, &PairGram2Item::partial_y, single_msg, slices, plan_x3_pair_gram1, launch_x3_pair_gram1);
        } else launch_pair32_singles(singles, &PairGramItem::partial, single_msg, slices, plan_pair_gram, launch_mfma_pair_gram);
    }
    // the fused and the plain Gram are different kernels: run them as two batches, keep the job order
    void launch_generic_grams() {
        std::vector<GramJob> jf, jp; std::vector<size_t> idf, idp;
        for (size_t i = 0; i < jobs.size(); ++i) {
            if (msgs[i].route == Route::GenericFused) { jf.push_back(jobs[i]); idf.push_back(i); }
            else if (msgs[i].route == Route::GenericPlain) { jp.push_back(jobs[i]); idp.push_back(i); }
        }
        on_side(true);
        run_grams<T, T>(s, jf, TNQS_PROF_BP_FUSED);
        run_grams<T, T>(s, jp, TNQS_PROF_BP_GRAM);
        join();
        on_side(false);
        for (size_t q = 0; q < jf.size(); ++q) jobs[idf[q]] = jf[q];
        for (size_t q = 0; q < jp.size(); ++q) jobs[idp[q]] = jp[q];
    }

    // ---- epilogue: m /= sum(m), message_diff against the previous value, for every message of the sub-batch in one launch --------------------
    MsgFinalItem final_item(int t, const void* partial, int nchunks) {
        const int de = plan.seq[t], c = s->chi[de / 2];
        Buf nb = dalloc(s, (size_t)c * c * esz);
        MsgFinalItem f{}; f.partial = partial; f.nchunks = nchunks; f.chi = c;
        const Buf& oldb = plan.in_place && u.fresh[de] ? u.fresh[de] : u.cur[de];
        f.old_msg = oldb ? oldb->p : nullptr; f.new_msg = nb->p;
        f.diff_out = reinterpret_cast<double*>(u.d_diffs->p) + t; f.normalize = u.normalize;
        u.fresh[de] = nb;
        return f;
    }
    void finalize() {
        std::vector<MsgFinalItem> fin;
        if (!s->sharded()) {
            for (size_t i = 0; i < jobs.size(); ++i) {
                if (jobs[i].final_msg) u.fresh[plan.seq[msgs[i].t]] = jobs[i].final_msg;         // (the small-site kernel finished it)
                else fin.push_back(final_item(msgs[i].t, jobs[i].partial->p, jobs[i].nchunks));
            }
        } else {
            const size_t stride = exchange_raw_messages();
            const char* base = reinterpret_cast<const char*>(s->exch);
            for (size_t q = start; q < end; ++q) fin.push_back(final_item(lev[q], base + (size_t)s->owner[g.src_of(plan.seq[lev[q]])] * stride + slot[q - start], 1));
        }
        if (!fin.empty()) {
            const MsgFinalItem* d = upload_small(s, fin);
            ProfScope ps(s, TNQS_PROF_SMALL, 0, 0);
            launch_msg_finalize<T>(s->stream, d, (int)fin.size());
        }
        // (sharded) the next sub-batch writes the exchange buffer again: ordered after this finalize by the stream; the host-side
        // all-gather callback is always preceded by a stream synchronisation inside exchange()
    }
    // sharded: owners reduce their raw messages into the exchange buffer, all-gather; then EVERY rank normalises / diffs every message of the
    // sub-batch (messages are replicated).  Returns the stride of a rank's block
    size_t exchange_raw_messages() {
        slot.assign(end - start, 0); std::vector<size_t> rank_bytes(s->nranks, 0);
        for (size_t q = start; q < end; ++q) {
            const int de = plan.seq[lev[q]], r = s->owner[g.src_of(de)];
            slot[q - start] = rank_bytes[r];
            rank_bytes[r] += round256((size_t)s->chi[de / 2] * s->chi[de / 2] * esz);
        }
        size_t stride = 0; for (size_t b : rank_bytes) stride = std::max(stride, b);
        check_exchange(s, stride);
        char* base = reinterpret_cast<char*>(s->exch);
        std::vector<ReduceItem> ri; int elems = 0; size_t oi = 0;
        for (size_t q = start; q < end; ++q) {
            const int de = plan.seq[lev[q]];
            if (!s->owns(g.src_of(de))) continue;
            const int n2 = s->chi[de / 2] * s->chi[de / 2];
            ri.push_back(ReduceItem{jobs[oi].partial->p, base + (size_t)s->rank * stride + slot[q - start], n2, jobs[oi].nchunks, 0, elems});
            elems += n2; ++oi;
        }
        if (!ri.empty()) { const ReduceItem* dr = upload(s, ri); launch_reduce<T, T>(s->stream, dr, (int)ri.size(), elems); }
        exchange(s, stride);
        return stride;
    }

    void run() {
        HostTimer ht_prep(0);
        take();
        shared_prefixes();
        route_messages();
        pair_up_planes16();
        ht_prep.stop();
        HostTimer ht_launch(1);
        fork();
        SplitGuard split_guard{s, main_stream, split_level};      // until the end of the sub-batch, finalize included: an exception still restores s->stream and ends the pool's defer mode
        launch_products();
        launch_small_sites();
        launch_plane_grams();
        launch_generic_grams();
        ht_launch.stop();
        HostTimer ht_fin(2);
        finalize();
    }
};

template <class T> void BpUpdate<T>::sweep(int iter) {
    fresh.assign(2 * (size_t)g.ne, nullptr);
    at.iter = iter; at.level = -1;
    for (auto& lev : plan.levels) {
        ++at.level;
        for (size_t start = 0; start < lev.size();) {          // sub-batches bounded by workspace bytes
            BpLevelBatch<T> b(*this, lev, start);
            b.run();
            start = b.end;
        }
    }
    for (size_t t = 0; t < nseq; ++t) if (fresh[plan.seq[t]]) cur[plan.seq[t]] = fresh[plan.seq[t]];
    s->stats.n_bp_sweeps += 1;
}

// optimistic: (apply_gates, a tolerance given) return after ENQUEUING the first sweep with its verdict left as a Check; iters_before: sweeps this update has already run
template <class T> void bp_update_t(State* s, const tnqs_bp_opts* o, int* niter_out, double* diff_out, bool optimistic, int iters_before) {
    HIPCHK(hipSetDevice(s->device));
    const std::shared_ptr<const BPPlan> plan = plan_for(*s->g, o);
    if (!(o ? o->normalize : 1)) materialize_scale_all(s);      // un-normalised messages carry the absolute scale of the site tensors
    if (plan->seq.empty()) { if (niter_out) *niter_out = 0; if (diff_out) *diff_out = 0; return; }
    PhaseScope phase_scope(s, TNQS_PROF_PHASE_BP_UPDATE); phase_scope.count = 0;       // launches = sweeps enqueued
    BpUpdate<T> u(s, *plan, o, optimistic, iters_before);
    for (int iter = 1 + iters_before; iter <= u.at.maxiter; ++iter) {
        phase_scope.count += 1;
        u.sweep(iter);
        const BpVerdict v = u.verdict(iter);
        if (v == BpVerdict::Deferred) return;             // committed already; the Check decides whether the caller comes back for more sweeps
        if (v == BpVerdict::Converged) break;
    }
    u.commit(niter_out, diff_out);
}

void bp_update(State* s, const tnqs_bp_opts* o, int* niter, double* diff) {
    if (s->dtype == TNQS_C64) bp_update_t<float>(s, o, niter, diff); else bp_update_t<double>(s, o, niter, diff);
}

template void bp_update_t<float>(State*, const tnqs_bp_opts*, int*, double*, bool, int);
template void bp_update_t<double>(State*, const tnqs_bp_opts*, int*, double*, bool, int);

}  // namespace tnqs
