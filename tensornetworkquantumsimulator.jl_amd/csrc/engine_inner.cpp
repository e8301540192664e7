// engine_inner.cpp -- inner(psi, phi; alg = "bp") (src/inner.jl:65-69): belief propagation on BilinearForm(ket, bra) (src/Forms/bilinearform.jl:16-25), two handles
// on the same graph with the same site dimensions and free bond dimensions.  The form network has two tensors per vertex and general chi_ket(e) x chi_bra(e)
// messages m[a, b] (a on the ket's leg, b on the bra's; the rectangular delta to begin with -- null here, as State::msg is null for the identity):
//   m_{u -> v}[a, b] = sum_{s, rest} (ket_u x_{k != v} m_{k -> u})[s, a, rest] conj(bra_u[s, b, rest]),   then m / sum(m)      (abstractbeliefpropagationcache.jl:162-190)
// Every message is absorbed on the ket's side.  Nothing here is shared with engine_bp.cpp, whose products assume bra = conj(ket); the sweep order (bp_schedule.cpp),
// the Gauss-Seidel position rule and tnqs_bp_opts are the same.  Per level and workspace-bounded batch, one launch per stage:
//   1. mode products whose steps CHANGE the leg's dimension (chi_ket -> chi_bra): fiber GEMMs with No != K, one FiberPass per step over all messages of the batch;
//   2. the rectangular Gram with the bra tensor (kernels_inner.hip), chunked;  3. the epilogue (chunk sum in f64, normalisation, message_diff, raw element sum).
// log z = sum_v log(vertex_scalar) - sum_e log(edge_scalar) (abstract...:289-304): the vertex scalar is sum_ab raw_{v -> w}[a, b] m_{w -> v}[a, b] for the first
// neighbour w, formed from the NORMALISED raw message and its raw element sum; the last sweep's is used when no message it absorbed changed after it, otherwise
// one more pass computes it (nothing is committed by that pass).  All scalars in one f64 launch; the call ends with one read-back (one more per sweep when a
// tolerance is given).  The messages live in buffers of the call: neither handle's messages are read or written.  Booked under TNQS_PROF_SMALL.
#include "engine_internal.hpp"

namespace tnqs {

namespace {

constexpr int kReadCommitted = INT_MAX;      // position of a job that reads the committed messages only (the pass after the last sweep)

struct InnerJob {
    int u = -1, jo = -1;       // source vertex and outgoing leg (-1: a vertex without neighbours -- the plain site overlap, a 1 x 1 "message")
    int t = kReadCommitted;    // position in the sequence
    Buf out; const void* old_msg = nullptr; double* diff = nullptr; double* sum = nullptr;
};

template <class T> struct InnerBp {
    State* const k; State* const b; const Graph& g; const BPPlan& plan;
    const size_t esz; const int normalize; const size_t budget;
    std::vector<Buf> cur, fresh;                              // per directed edge: the committed message, this sweep's (null = rectangular delta)
    std::map<std::pair<int, int>, Buf> deltas;                // rectangular deltas that had to be written out, by shape
    int nbatches = 0;

    InnerBp(State* ket, State* bra, const BPPlan& p, int norm, size_t ws) : k(ket), b(bra), g(*ket->g), plan(p), esz(ket->esz()), normalize(norm), budget(ws),
                                                                           cur(2 * (size_t)ket->g->ne), fresh(2 * (size_t)ket->g->ne) {}
    int rows(int de) const { return k->chi[de / 2]; }
    int cols(int de) const { return b->chi[de / 2]; }
    // delta(virtualinds(form, e)) as a matrix, for a leg whose two bond dimensions differ (with equal dimensions an unset message is skipped, as the identity is)
    const void* delta(int r, int c) {
        Buf& d = deltas[{r, c}];
        if (!d) {
            std::vector<T> h(2 * (size_t)r * c, (T)0);
            for (int i = 0; i < std::min(r, c); ++i) h[2 * ((size_t)i + (size_t)r * i)] = (T)1;
            upload(k, h); d = k->keepalive.back();            // ours from here on: a synchronisation between sweeps empties the keep-alive list
        }
        return d->p;
    }
    // THE Gauss-Seidel rule of bp_update: this sweep's value when the message was computed at an earlier position (in place: whenever there is one)
    const Buf& incoming(int src, int j, int t) const {
        const int din = g.dedge(g.nbr[src][j], src), pp = plan.pos_of[din];
        return (t != kReadCommitted && (plan.in_place || (pp >= 0 && pp < t)) && fresh[din]) ? fresh[din] : cur[din];
    }
    struct Work { SD sd; const void* res = nullptr; Buf buf[2]; std::vector<std::pair<int, const void*>> steps; std::vector<int> no; const void* Y = nullptr; int Kb = 1; };
    void set_up(const InnerJob& j, Work& w, size_t* ws_bytes) {
        w.sd = site_dims(k, j.u); w.res = k->site[j.u]->p; w.Y = b->site[j.u]->p;
        const SD sb = site_dims(b, j.u);
        size_t n = w.sd.n, nmax = n;
        for (int q = 0; q < w.sd.z; ++q) {
            if (q == j.jo) { w.Kb = sb.chi[q]; continue; }
            const Buf& m = incoming(j.u, q, j.t);
            if (!m && w.sd.chi[q] == sb.chi[q]) continue;
            w.steps.push_back({q, m ? m->p : nullptr}); w.no.push_back(sb.chi[q]);
            n = n / w.sd.chi[q] * sb.chi[q]; nmax = std::max(nmax, n);
        }
        if (ws_bytes) *ws_bytes = 2 * nmax * esz + 4096 * esz;
    }
    void run_batch(const InnerJob* jobs, size_t nj) {
        ++nbatches;
        std::vector<Work> ws(nj);
        size_t maxsteps = 0;
        for (size_t i = 0; i < nj; ++i) {
            set_up(jobs[i], ws[i], nullptr);
            for (auto& st : ws[i].steps) if (!st.second) st.second = delta(ws[i].sd.chi[st.first], ws[i].no[&st - ws[i].steps.data()]);
            maxsteps = std::max(maxsteps, ws[i].steps.size());
        }
        // 1. the mode products, step o of every chain of the batch in one pass; the tensor's dimensions follow the steps
        const FiberRules rules = fiber_rules_of(k, FiberUse::Chain);
        std::vector<FiberItem> items;
        for (size_t o = 0; o < maxsteps; ++o) {
            items.clear();
            for (Work& w : ws) {
                if (w.steps.size() <= o) continue;
                const int q = w.steps[o].first, No = w.no[o];
                FiberItem it = site_fiber_item(w.sd, q, false, No, false);
                const size_t nnew = w.sd.n / w.sd.chi[q] * No;
                Buf dst = dalloc(k, nnew * esz);
                it.in = w.res; it.out = dst->p; it.X = w.steps[o].second;
                items.push_back(it);
                w.sd.chi[q] = No; w.sd.n = nnew; w.res = dst->p; w.buf[o & 1] = dst;      // (the pass before last's buffer goes back: reuse is stream-ordered)
            }
            FiberPass(items, rules, esz).run<T>(k, TNQS_PROF_SMALL, /*norms=*/false);
        }
        // 2. the rectangular Gram with the bra's tensor
        std::vector<InnerGramItem> gi(nj); std::vector<int> npart(nj); double bytes = 0, flops = 0;
        for (size_t i = 0; i < nj; ++i) {
            const Work& w = ws[i]; InnerGramItem& it = gi[i]; it = InnerGramItem{};
            it.X = w.res; it.Y = w.Y;
            if (jobs[i].jo >= 0) { it.PA = (int)w.sd.pre(jobs[i].jo); it.Ka = w.sd.chi[jobs[i].jo]; it.Kb = w.Kb; it.PB = (int)w.sd.post(jobs[i].jo); }
            else { it.PA = w.sd.d; it.Ka = it.Kb = it.PB = 1; }
            bytes += (double)it.PA * it.PB * (it.Ka + it.Kb) * esz; flops += 8.0 * it.PA * it.PB * it.Ka * it.Kb;
        }
        const int chunks = plan_inner_gram(gi.data(), (int)nj, esz, 0, npart.data());
        std::vector<Buf> partial(nj);
        for (size_t i = 0; i < nj; ++i) { partial[i] = dalloc(k, (size_t)npart[i] * gi[i].Ka * gi[i].Kb * esz); gi[i].partial = partial[i]->p; }
        {
            const InnerGramItem* d = upload(k, gi);
            ProfScope ps(k, TNQS_PROF_SMALL, bytes, flops);
            launch_inner_gram<T>(k->stream, d, (int)nj, chunks);
        }
        // 3. the epilogue
        std::vector<InnerFinalItem> fi(nj);
        for (size_t i = 0; i < nj; ++i)
            fi[i] = InnerFinalItem{gi[i].partial, npart[i], gi[i].Ka, gi[i].Kb, jobs[i].old_msg, jobs[i].out->p, jobs[i].diff, jobs[i].sum, jobs[i].jo >= 0 ? normalize : 1};
        const InnerFinalItem* d = upload(k, fi);
        ProfScope ps(k, TNQS_PROF_SMALL, 0, 0);
        launch_inner_finalize<T>(k->stream, d, (int)nj);
    }
    // jobs that do not depend on each other, in batches whose chain temporaries stay within the budget (a job that needs more runs alone)
    void run(const std::vector<InnerJob>& jobs) {
        for (size_t j0 = 0; j0 < jobs.size();) {
            size_t j1 = j0, bytes = 0;
            while (j1 < jobs.size()) {
                Work w; size_t need = 0; set_up(jobs[j1], w, &need);
                if (j1 > j0 && bytes + need > budget) break;
                bytes += need; ++j1;
            }
            run_batch(jobs.data() + j0, j1 - j0);
            j0 = j1;
        }
    }
    InnerJob message_job(int de, int t, double* diff, double* sum) {
        InnerJob j; j.u = g.src_of(de); j.jo = g.leg(j.u, g.dst_of(de)); j.t = t;
        j.out = dalloc(k, (size_t)rows(de) * cols(de) * esz);
        const Buf& old = (t != kReadCommitted && plan.in_place && fresh[de]) ? fresh[de] : cur[de];
        j.old_msg = (t != kReadCommitted && old) ? old->p : nullptr; j.diff = diff; j.sum = sum;
        return j;
    }
    void sweep(double* d_diffs, double* d_sums) {
        std::fill(fresh.begin(), fresh.end(), Buf());
        std::vector<InnerJob> jobs;
        for (const std::vector<int>& lev : plan.levels) {
            jobs.clear();
            for (int t : lev) jobs.push_back(message_job(plan.seq[t], t, d_diffs + t, d_sums + 2 * (size_t)plan.seq[t]));
            run(jobs);
            for (size_t i = 0; i < lev.size(); ++i) fresh[plan.seq[lev[i]]] = jobs[i].out;
        }
        for (int de : plan.seq) if (fresh[de]) cur[de] = fresh[de];
    }
};

void check_same_network(const State* k, const State* b) {
    const Graph& gk = *k->g; const Graph& gb = *b->g;
    if (k->sharded() || b->sharded()) throw Err(TNQS_ERR_UNSUPPORTED, "inner_bp: sharded handles are not supported");
    if (gk.nv != gb.nv || gk.ne != gb.ne || gk.esrc != gb.esrc || gk.edst != gb.edst) throw Err(TNQS_ERR_INVALID, "inner_bp: the two states live on different graphs (vertex / edge lists differ)");
    if (k->d != b->d) throw Err(TNQS_ERR_INVALID, "inner_bp: the two states have different site dimensions");
    if (k->scalartype() != b->scalartype()) throw Err(TNQS_ERR_INVALID, "inner_bp: the two states have different element types");
    if (k->device != b->device) throw Err(TNQS_ERR_INVALID, "inner_bp: the two states live on different devices");
    for (int e = 0; e < gk.ne; ++e)
        if (!inner_gram_covers(k->chi[e], b->chi[e])) throw Err(TNQS_ERR_UNSUPPORTED, "inner_bp: bond dimensions beyond 64 are not supported (rectangular Gram kernel)");
}

template <class T> void inner_bp_t(State* k, State* b, const tnqs_bp_opts* o, double* out_log, int* niter_out, double* diff_out, size_t budget, int* nbatches) {
    const Graph& g = *k->g;
    const std::shared_ptr<const BPPlan> plan = plan_for(g, o);
    const int normalize = o ? o->normalize : 1;
    const int maxiter = (o && o->maxiter > 0) ? o->maxiter : (g.is_tree ? 1 : 25);
    double tol = -1.0;                                        // a bare update of the form cache has no tolerance (beliefpropagationcache.jl:62-67)
    if (o) tol = std::isnan(o->tolerance) ? (g.is_tree ? -1.0 : (k->dtype == TNQS_C64 ? 1e-5 : 1e-8)) : o->tolerance;
    const size_t nseq = plan->seq.size(), nde = 2 * (size_t)g.ne, nsc = (size_t)g.nv + g.ne;
    InnerBp<T> u(k, b, *plan, normalize, budget);
    // device doubles: [message_diff per position][raw element sums: per directed edge, then per vertex (the pass after the last sweep)][scalars: vertices, edges][sum of the diffs]
    Buf d_all = dalloc(k, (nseq + 2 * (nde + g.nv) + 2 * nsc + 1) * sizeof(double));
    double* const d_diffs = reinterpret_cast<double*>(d_all->p); double* const d_sums = d_diffs + nseq;
    double* const d_scal = d_sums + 2 * (nde + g.nv); double* const d_dsum = d_scal + 2 * nsc;
    HIPCHK(hipMemsetAsync(d_all->p, 0, d_all->bytes, k->stream));
    int niter = 0; double avg = 0;
    for (int iter = 1; iter <= maxiter && nseq > 0; ++iter) {
        u.sweep(d_diffs, d_sums);
        niter = iter;
        launch_sum_doubles(k->stream, d_diffs, (int)nseq, d_dsum);
        if (tol >= 0) {                                       // the one read-back of a sweep
            const double* st = readback<double>(k, d_dsum, 1);
            sync(k);
            avg = *st / (double)nseq;
            if (avg <= tol) break;
        }
    }
    // vertex scalars: the raw message towards the first neighbour -- the last sweep's where every message it absorbed is still the one it absorbed
    std::vector<InnerJob> extra; std::vector<const void*> vm(g.nv, nullptr); std::vector<const double*> vsum(g.nv, nullptr);
    for (int v = 0; v < g.nv; ++v) {
        if (g.nbr[v].empty()) { InnerJob j; j.u = v; j.out = dalloc(k, k->esz()); j.sum = d_sums + 2 * (nde + v); extra.push_back(j); vm[v] = j.out->p; vsum[v] = j.sum; continue; }
        const int de = g.dedge(v, g.nbr[v][0]), pv = plan->pos_of[de];
        bool stale = niter == 0 || pv < 0 || plan->in_place;
        for (size_t q = 1; q < g.nbr[v].size() && !stale; ++q) stale = plan->pos_of[g.dedge(g.nbr[v][q], v)] > pv;
        if (stale) { InnerJob j = u.message_job(de, kReadCommitted, nullptr, d_sums + 2 * (nde + v)); extra.push_back(j); vm[v] = j.out->p; vsum[v] = j.sum; }
        else { vm[v] = u.cur[de]->p; vsum[v] = d_sums + 2 * (size_t)de; }
    }
    u.run(extra);
    std::vector<InnerScalarItem> si;
    for (int v = 0; v < g.nv; ++v) {
        const double* sa = k->sscale[v] ? reinterpret_cast<const double*>(k->sscale[v]->p) : nullptr;
        const double* sb = b->sscale[v] ? reinterpret_cast<const double*>(b->sscale[v]->p) : nullptr;
        if (g.nbr[v].empty()) { si.push_back(InnerScalarItem{vm[v], nullptr, 1, 1, vsum[v], 1, sa, sb, d_scal + 2 * (size_t)v}); continue; }
        const int de = g.dedge(v, g.nbr[v][0]), dr = de ^ 1;
        si.push_back(InnerScalarItem{vm[v], u.cur[dr] ? u.cur[dr]->p : nullptr, u.rows(de), u.cols(de), vsum[v], normalize, sa, sb, d_scal + 2 * (size_t)v});
    }
    for (int e = 0; e < g.ne; ++e)
        si.push_back(InnerScalarItem{u.cur[2 * e] ? u.cur[2 * e]->p : nullptr, u.cur[2 * e + 1] ? u.cur[2 * e + 1]->p : nullptr, u.rows(2 * e), u.cols(2 * e), nullptr, 0, nullptr, nullptr,
                                     d_scal + 2 * ((size_t)g.nv + e)});
    {
        const InnerScalarItem* d = upload(k, si);
        ProfScope ps(k, TNQS_PROF_SMALL, 0, 0);
        launch_inner_scalar<T>(k->stream, d, (int)si.size());
    }
    const double* h = readback<double>(k, d_scal, 2 * nsc + 1);      // the one read-back of the call: scalars and the last sweep's summed diffs
    sync(k);
    if (tol < 0 && nseq > 0) avg = h[2 * nsc] / (double)nseq;
    std::complex<double> lz(0, 0); bool zero = false;
    for (size_t i = 0; i < nsc; ++i) {
        const std::complex<double> z(h[2 * i], h[2 * i + 1]);
        if (!std::isfinite(z.real()) || !std::isfinite(z.imag())) throw Err(TNQS_ERR_NUMERIC, "inner_bp: a vertex or edge scalar is not finite");
        if (z == std::complex<double>(0, 0)) { zero = true; continue; }
        if (i < (size_t)g.nv) lz += std::log(z); else lz -= std::log(z);
    }
    if (zero) { out_log[0] = -std::numeric_limits<double>::infinity(); out_log[1] = 0; }      // the reference's freenergy is -Inf, the overlap 0
    else {
        const double pi = 3.14159265358979323846;
        double im = std::fmod(lz.imag(), 2 * pi);
        if (im > pi) im -= 2 * pi; else if (im <= -pi) im += 2 * pi;
        out_log[0] = lz.real(); out_log[1] = im;
    }
    if (niter_out) *niter_out = niter;
    if (diff_out) *diff_out = avg;
    if (nbatches) *nbatches = u.nbatches;
}

}  // namespace

void inner_bp(State* k, State* b, const tnqs_bp_opts* o, double* out_log_re_im, int* niter, double* final_diff, size_t budget, int* nbatches) {
    if (!out_log_re_im) throw Err(TNQS_ERR_INVALID, "inner_bp: null output");
    check_same_network(k, b);
    if (o && o->n_sequence > 0 && (!o->seq_src || !o->seq_dst)) throw Err(TNQS_ERR_INVALID, "inner_bp: null edge sequence");
    HIPCHK(hipSetDevice(k->device));
    // both handles as the reference holds them: deferred one-site gates applied (they act on the site index, which ket and bra share only when both carry them);
    // pending real scale factors multiply the vertex scalars -- unless the messages are left un-normalised, which carry the tensors' absolute scale themselves
    materialize_pending_all(k);
    if (b != k) materialize_pending_all(b);
    if (!(o ? o->normalize : 1)) { materialize_scale_all(k); if (b != k) materialize_scale_all(b); }
    if (b != k && b->stream != k->stream) {                  // the bra's tensors are read on the ket's stream: behind whatever the bra's own stream still holds
        hipEvent_t ev; HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        hipError_t e1 = hipEventRecord(ev, b->stream), e2 = e1 == hipSuccess ? hipStreamWaitEvent(k->stream, ev, 0) : e1;
        (void)hipEventDestroy(ev);
        HIPCHK(e1); HIPCHK(e2);
    }
    if (!budget) {
        size_t free_b = 0, total_b = 0;
        HIPCHK(hipMemGetInfo(&free_b, &total_b));
        budget = std::min<size_t>(size_t(2) << 30, free_b / 4);
    }
    if (k->dtype == TNQS_C64) inner_bp_t<float>(k, b, o, out_log_re_im, niter, final_diff, budget, nbatches);
    else inner_bp_t<double>(k, b, o, out_log_re_im, niter, final_diff, budget, nbatches);
}

}  // namespace tnqs
