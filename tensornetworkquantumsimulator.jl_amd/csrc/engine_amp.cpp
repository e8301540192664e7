// engine_amp.cpp -- amplitudes <x|psi> of a batch of bitstrings by belief propagation (tnqs_amplitudes_bp): the reference's single-layer path, contract(tn; alg = "bp")
// (src/contract.jl:7-9) over the network A_v = T_v[x_v, ...] with vector messages that start as all ones (src/TensorNetworks/tensornetwork.jl:62-64) -- what
// certify_sample contracts per sample (src/sampling.jl:258-285).  Per string x:
//   m_{u -> v}[j] = sum A_u[..., j, ...] prod_{k != v} m_{k -> u}[i_k],   then m / sum(m)                                          (abstractbeliefpropagationcache.jl:162-190)
//   log a(x) = sum_v log(vertex scalar) - sum_e log(edge scalar),  vertex scalar = sum_j raw_{v -> w}[j] m_{w -> v}[j] for the first neighbour w              (:289-304)
// The driver is InnerBp's (engine_inner.cpp): the same plan_for, level schedule, Gauss-Seidel position rule and staleness rule for the vertex scalars; per level the
// messages form batches of jobs whose chain temporaries stay within the workspace budget.  What differs is the batch of strings: a message is a [chi][nstrings] matrix in
// the state's type (column n = string n, null = all ones), and the strings are cut into chunks of Bc so that a job's intermediate (n_u / (d_u chi_first) elements per
// string) fits the budget as well.  Per batch and chunk, one launch per stage:
//   1. amp_leg_gemm: the first message of every job absorbed into the site-tensor slice -- per job and site value g the strings with x_u = g are one group (a GEMM of
//      the slice, read in place, with the group's message columns); the groups come from one index list per vertex, built on the host and uploaded once per call.  No
//      string gets a copy of a site tensor or of a slice.  (A site with the outgoing leg only takes the same kernel with K = 1 and no message.)
//   2. amp_absorb: step o of every chain of the batch, the legs from the last to the first;  3. amp_finalize: raw sum, normalisation, message_diff, done strings skipped.
// With a tolerance, string n is done after the first sweep whose average message_diff is <= tol (amp_sweep_end): from then on none of its messages, sums or diffs is
// stored, so its niter, final_diff and log a are those of a call with that string alone; one read-back of the done flags per sweep.  Without one, one read-back per call.
// Neither the handle's messages nor its tensors are written.  Booked under TNQS_PROF_SMALL.
#include "engine_internal.hpp"

namespace tnqs {

namespace {

constexpr int kReadCommitted = INT_MAX;      // position of a job that reads the committed messages only (the pass after the last sweep)

struct AmpJob {
    int u = -1, jo = -1;       // source vertex and outgoing leg
    int t = kReadCommitted;    // position in the sequence
    Buf out; const void* old_msg = nullptr; double* diff = nullptr; double* sum = nullptr; bool freeze = false;      // out, old_msg: [chi][nstrings]; diff: [nstrings]; sum: [2 nstrings]
};

template <class T> struct AmpBp {
    State* const s; const Graph& g; const BPPlan& plan;
    const size_t esz; const int normalize; const size_t budget; const int B;
    std::vector<Buf> cur, fresh;                              // per directed edge: the committed message, this sweep's (null = all ones)
    Buf idx_buf; const int* d_idx = nullptr;                  // per vertex u: the strings' chunk positions, ordered by (chunk, x_u)
    std::vector<int> grp_off;                                 // [(u nchunks + c)(dmax + 1) + g]: where group g of chunk c starts in row u of d_idx
    const int* d_done = nullptr;
    int Bc = 1, nchunks = 1, dmax = 1, nbatches = 0;

    AmpBp(State* st, const BPPlan& p, int norm, size_t ws, int nstrings) : s(st), g(*st->g), plan(p), esz(st->esz()), normalize(norm), budget(ws), B(nstrings),
                                                                        cur(2 * (size_t)st->g->ne), fresh(2 * (size_t)st->g->ne) {}
    // the leg a job absorbs on the matrix cores: the widest but the outgoing one (the smallest intermediate), the first of equals; -1: the outgoing leg is the only one
    static int first_leg(const SD& sd, int jo) { int q = -1; for (int i = 0; i < sd.z; ++i) if (i != jo && (q < 0 || sd.chi[i] > sd.chi[q])) q = i; return q; }
    size_t inter_elems(int u, int jo) const { const SD sd = site_dims(s, u); const int q = first_leg(sd, jo); return sd.n / sd.d / (q >= 0 ? sd.chi[q] : 1); }
    size_t job_bytes(int u, int jo) const { return 2 * inter_elems(u, jo) * (size_t)Bc * esz; }
    // chunks of strings: the largest job's two intermediates within the budget; the groups of every vertex and chunk
    void lay_out_strings(const int32_t* cfg) {
        size_t worst = 1;
        for (int u = 0; u < g.nv; ++u) for (int j = 0; j < (int)g.nbr[u].size(); ++j) worst = std::max(worst, inter_elems(u, j));
        const size_t fit = std::min<size_t>(budget / (2 * worst * esz), (size_t(1) << 30) / worst);
        Bc = (int)std::max<size_t>(1, std::min<size_t>(fit, (size_t)B));
        nchunks = (B + Bc - 1) / Bc;
        for (int v = 0; v < g.nv; ++v) dmax = std::max(dmax, s->d[v]);
        std::vector<int> idx((size_t)g.nv * B);
        grp_off.assign((size_t)g.nv * nchunks * (dmax + 1), 0);
        for (int u = 0; u < g.nv; ++u)
            for (int c = 0; c < nchunks; ++c) {
                const int c0 = c * Bc, nc = std::min(Bc, B - c0);
                int* off = grp_off.data() + ((size_t)u * nchunks + c) * (dmax + 1);
                for (int p = 0; p < nc; ++p) ++off[cfg[(size_t)(c0 + p) * g.nv + u] + 1];
                off[0] = c0;
                for (int q = 0; q < dmax; ++q) off[q + 1] += off[q];
                std::vector<int> at(off, off + dmax);
                for (int p = 0; p < nc; ++p) idx[(size_t)u * B + at[cfg[(size_t)(c0 + p) * g.nv + u]]++] = p;
            }
        d_idx = upload(s, idx); idx_buf = s->keepalive.back();      // ours from here on: a synchronisation between sweeps empties the keep-alive list
    }
    // THE Gauss-Seidel rule of bp_update: this sweep's value when the message was computed at an earlier position (in place: whenever there is one)
    const Buf& incoming(int src, int j, int t) const {
        const int din = g.dedge(g.nbr[src][j], src), pp = plan.pos_of[din];
        return (t != kReadCommitted && (plan.in_place || (pp >= 0 && pp < t)) && fresh[din]) ? fresh[din] : cur[din];
    }
    const char* msg_at(const Buf& m, int chi, int c0) const { return m ? reinterpret_cast<const char*>(m->p) + (size_t)chi * c0 * esz : nullptr; }
    struct Work { Buf buf[2]; const void* res = nullptr; std::vector<int> dims, legs; std::vector<int> order; };      // dims / legs: what is left of the site's bond legs
    void run_batch(const AmpJob* jobs, size_t nj, int c, bool book) {
        if (book) ++nbatches;
        const int c0 = c * Bc, nc = std::min(Bc, B - c0);
        std::vector<Work> ws(nj);
        // 1. the first leg of every job on the matrix cores, one item per non-empty group
        std::vector<AmpGemmItem> gi; double bytes = 0, flops = 0; size_t maxsteps = 0;
        for (size_t i = 0; i < nj; ++i) {
            const AmpJob& j = jobs[i]; Work& w = ws[i];
            const SD sd = site_dims(s, j.u);
            const int q = first_leg(sd, j.jo);
            AmpGemmItem it{};
            it.d = sd.d;
            if (q >= 0) { it.PA = (int)(sd.pre(q) / sd.d); it.K = sd.chi[q]; it.PB = (int)sd.post(q); it.M = msg_at(incoming(j.u, q, j.t), it.K, c0); }
            else { it.PA = (int)(sd.n / sd.d); it.K = 1; it.PB = 1; it.M = nullptr; }
            const size_t nr = (size_t)it.PA * it.PB;
            w.buf[0] = dalloc(s, nr * nc * esz); w.res = w.buf[0]->p; it.R = w.buf[0]->p;
            for (int i2 = 0; i2 < sd.z; ++i2) if (i2 != q) { w.dims.push_back(sd.chi[i2]); w.legs.push_back(i2); }
            for (int i2 = sd.z - 1; i2 >= 0; --i2) if (i2 != q && i2 != j.jo) w.order.push_back(i2);
            maxsteps = std::max(maxsteps, w.order.size());
            const int* off = grp_off.data() + ((size_t)j.u * nchunks + c) * (dmax + 1);
            for (int gv = 0; gv < sd.d; ++gv) {
                it.ncols = off[gv + 1] - off[gv];
                if (!it.ncols) continue;
                it.T = reinterpret_cast<const char*>(s->site[j.u]->p) + (size_t)gv * esz; it.idx = d_idx + (size_t)j.u * B + off[gv];
                gi.push_back(it);
                bytes += ((double)nr * it.K + (double)nr * it.ncols + (double)it.K * it.ncols) * esz; flops += 8.0 * nr * it.K * it.ncols;
            }
        }
        {
            const int tiles = plan_amp_gemm(gi.data(), (int)gi.size());
            const AmpGemmItem* d = upload(s, gi);
            ProfScope ps(s, TNQS_PROF_SMALL, bytes, flops);
            launch_amp_leg_gemm<T>(s->stream, d, (int)gi.size(), tiles);
        }
        // 2. the remaining legs but the outgoing one, step o of every chain of the batch in one launch
        std::vector<AmpAbsorbItem> ai;
        for (size_t o = 0; o < maxsteps; ++o) {
            ai.clear(); bytes = flops = 0;
            for (size_t i = 0; i < nj; ++i) {
                Work& w = ws[i];
                if (w.order.size() <= o) continue;
                const int leg = w.order[o], pos = (int)(std::find(w.legs.begin(), w.legs.end(), leg) - w.legs.begin());
                AmpAbsorbItem it{};
                it.PA = it.PB = 1; it.K = w.dims[pos]; it.nstr = nc;
                for (int i2 = 0; i2 < pos; ++i2) it.PA *= w.dims[i2];
                for (size_t i2 = pos + 1; i2 < w.dims.size(); ++i2) it.PB *= w.dims[i2];
                Buf dst = dalloc(s, (size_t)it.PA * it.PB * nc * esz);
                it.in = w.res; it.out = dst->p; it.m = msg_at(incoming(jobs[i].u, leg, jobs[i].t), it.K, c0);
                ai.push_back(it);
                bytes += (double)it.PA * it.PB * nc * (it.K + 1.0) * esz; flops += 8.0 * it.PA * it.PB * nc * it.K;
                w.dims.erase(w.dims.begin() + pos); w.legs.erase(w.legs.begin() + pos);
                w.res = dst->p; w.buf[(o + 1) & 1] = dst;      // (the step before last's buffer goes back: reuse is stream-ordered)
            }
            const int wgs = plan_amp_absorb(ai.data(), (int)ai.size());
            const AmpAbsorbItem* d = upload(s, ai);
            ProfScope ps(s, TNQS_PROF_SMALL, bytes, flops);
            launch_amp_absorb<T>(s->stream, d, (int)ai.size(), wgs);
        }
        // 3. the epilogue
        std::vector<AmpFinalItem> fi(nj);
        for (size_t i = 0; i < nj; ++i) {
            const AmpJob& j = jobs[i];
            const int chi = ws[i].dims[0];
            AmpFinalItem& it = fi[i]; it = AmpFinalItem{};
            it.raw = ws[i].res; it.chi = chi; it.nstr = nc; it.normalize = normalize;
            it.old_msg = j.old_msg ? reinterpret_cast<const char*>(j.old_msg) + (size_t)chi * c0 * esz : nullptr;
            it.new_msg = reinterpret_cast<char*>(j.out->p) + (size_t)chi * c0 * esz;
            it.done = (j.freeze && d_done) ? d_done + c0 : nullptr;
            it.diff_out = j.diff ? j.diff + c0 : nullptr; it.sum_out = j.sum ? j.sum + 2 * (size_t)c0 : nullptr;
        }
        const int wgs = plan_amp_finalize(fi.data(), (int)nj);
        const AmpFinalItem* d = upload(s, fi);
        ProfScope ps(s, TNQS_PROF_SMALL, 0, 0);
        launch_amp_finalize<T>(s->stream, d, (int)nj, wgs);
    }
    // jobs that do not depend on each other, in batches whose chain temporaries stay within the budget (a job that needs more runs alone), chunk by chunk
    void run(const std::vector<AmpJob>& jobs) {
        for (size_t j0 = 0; j0 < jobs.size();) {
            size_t j1 = j0, bytes = 0;
            while (j1 < jobs.size()) {
                const size_t need = job_bytes(jobs[j1].u, jobs[j1].jo);
                if (j1 > j0 && bytes + need > budget) break;
                bytes += need; ++j1;
            }
            for (int c = 0; c < nchunks; ++c) run_batch(jobs.data() + j0, j1 - j0, c, true);
            j0 = j1;
        }
    }
    int chi_of(int de) const { return s->chi[de / 2]; }
    AmpJob message_job(int de, int t, double* diff, double* sum, bool freeze) {
        AmpJob j; j.u = g.src_of(de); j.jo = g.leg(j.u, g.dst_of(de)); j.t = t; j.freeze = freeze;
        j.out = dalloc(s, (size_t)chi_of(de) * B * esz);
        const Buf& old = (t != kReadCommitted && plan.in_place && fresh[de]) ? fresh[de] : cur[de];
        j.old_msg = (t != kReadCommitted && old) ? old->p : nullptr; j.diff = diff; j.sum = sum;
        return j;
    }
    void sweep(double* d_diffs, double* d_sums) {
        std::fill(fresh.begin(), fresh.end(), Buf());
        std::vector<AmpJob> jobs;
        for (const std::vector<int>& lev : plan.levels) {
            jobs.clear();
            for (int t : lev) jobs.push_back(message_job(plan.seq[t], t, d_diffs + (size_t)t * B, d_sums + 2 * (size_t)plan.seq[t] * B, true));
            run(jobs);
            for (size_t i = 0; i < lev.size(); ++i) fresh[plan.seq[lev[i]]] = jobs[i].out;
        }
        for (int de : plan.seq) if (fresh[de]) cur[de] = fresh[de];
    }
};

template <class T> void amplitudes_bp_t(State* s, int B, const int32_t* configs, const tnqs_bp_opts* o, double* out, int32_t* niter_out, double* diff_out, int32_t* flags_out,
                                        size_t budget, int* nbatches) {
    const Graph& g = *s->g;
    const std::shared_ptr<const BPPlan> plan = plan_for(g, o);
    const int normalize = o ? o->normalize : 1;
    const int maxiter = (o && o->maxiter > 0) ? o->maxiter : (g.is_tree ? 1 : 25);
    double tol = -1.0;                                        // a bare update has no tolerance (beliefpropagationcache.jl:62-67)
    if (o) tol = std::isnan(o->tolerance) ? (g.is_tree ? -1.0 : (s->dtype == TNQS_C64 ? 1e-5 : 1e-8)) : o->tolerance;
    const size_t nseq = plan->seq.size(), nde = 2 * (size_t)g.ne, nb = (size_t)B;
    AmpBp<T> u(s, *plan, normalize, budget, B);
    u.lay_out_strings(configs);
    // device doubles: [message_diff per position and string][raw element sums per directed edge, then per vertex (the pass after the last sweep), and string]
    // [log a per string][final diff per string]; ints: [niter][flags][done] per string
    const size_t ndbl = (nseq + 2 * (nde + g.nv) + 3) * nb;
    Buf d_all = dalloc(s, ndbl * sizeof(double) + 3 * nb * sizeof(int));
    double* const d_diffs = reinterpret_cast<double*>(d_all->p); double* const d_sums = d_diffs + nseq * nb;
    double* const d_out = d_sums + 2 * (nde + g.nv) * nb; double* const d_fdiff = d_out + 2 * nb;
    int* const d_niter = reinterpret_cast<int*>(d_fdiff + nb); int* const d_flags = d_niter + nb; int* const d_done = d_flags + nb;
    HIPCHK(hipMemsetAsync(d_all->p, 0, d_all->bytes, s->stream));
    if (tol >= 0) u.d_done = d_done;
    int niter = 0;
    for (int iter = 1; iter <= maxiter && nseq > 0; ++iter) {
        u.sweep(d_diffs, d_sums);
        niter = iter;
        launch_amp_sweep_end(s->stream, d_diffs, (int)nseq, B, iter, tol, d_done, d_niter, d_fdiff);
        if (tol >= 0) {                                       // the one read-back of a sweep
            const int* st = readback<int>(s, d_done, nb);
            sync(s);
            if (std::all_of(st, st + nb, [](int f) { return f != 0; })) break;
        }
    }
    // vertex scalars: the raw message towards the first neighbour -- the last sweep's where every message it absorbed is still the one it absorbed
    std::vector<AmpJob> extra; std::vector<const void*> vm(g.nv, nullptr); std::vector<const double*> vsum(g.nv, nullptr);
    for (int v = 0; v < g.nv; ++v) {
        if (g.nbr[v].empty()) continue;
        const int de = g.dedge(v, g.nbr[v][0]), pv = plan->pos_of[de];
        bool stale = niter == 0 || pv < 0 || plan->in_place;
        for (size_t q = 1; q < g.nbr[v].size() && !stale; ++q) stale = plan->pos_of[g.dedge(g.nbr[v][q], v)] > pv;
        if (stale) { AmpJob j = u.message_job(de, kReadCommitted, nullptr, d_sums + 2 * (nde + v) * nb, false); extra.push_back(j); vm[v] = j.out->p; vsum[v] = j.sum; }
        else { vm[v] = u.cur[de]->p; vsum[v] = d_sums + 2 * (size_t)de * nb; }
    }
    u.run(extra);
    std::vector<AmpScalarItem> si;
    for (int v = 0; v < g.nv; ++v) {
        AmpScalarItem it{};
        it.scale = s->sscale[v] ? reinterpret_cast<const double*>(s->sscale[v]->p) : nullptr; it.vertex = v; it.normalize = normalize; it.chi = 1;
        if (g.nbr[v].empty()) it.site = s->site[v]->p;
        else {
            const int de = g.dedge(v, g.nbr[v][0]), dr = de ^ 1;
            it.m = vm[v]; it.mr = u.cur[dr] ? u.cur[dr]->p : nullptr; it.rawsum = vsum[v]; it.chi = u.chi_of(de);
        }
        si.push_back(it);
    }
    for (int e = 0; e < g.ne; ++e) {
        AmpScalarItem it{};
        it.m = u.cur[2 * e] ? u.cur[2 * e]->p : nullptr; it.mr = u.cur[2 * e + 1] ? u.cur[2 * e + 1]->p : nullptr; it.chi = u.chi_of(2 * e); it.vertex = -1;
        si.push_back(it);
    }
    {
        std::vector<int> cfg(configs, configs + nb * g.nv);
        const int* d_cfg = upload(s, cfg);
        const AmpScalarItem* d = upload(s, si);
        ProfScope ps(s, TNQS_PROF_SMALL, 0, 0);
        launch_amp_scalar<T>(s->stream, d, g.nv, g.ne, d_cfg, g.nv, B, d_out, d_flags);
    }
    const char* h = readback<char>(s, d_out, 3 * nb * sizeof(double) + 2 * nb * sizeof(int));      // the one read-back of the call: log a, final diffs, sweeps, flags
    sync(s);
    std::memcpy(out, h, 2 * nb * sizeof(double));
    if (diff_out) std::memcpy(diff_out, h + 2 * nb * sizeof(double), nb * sizeof(double));
    if (niter_out) std::memcpy(niter_out, h + 3 * nb * sizeof(double), nb * sizeof(int));
    if (flags_out) std::memcpy(flags_out, h + 3 * nb * sizeof(double) + nb * sizeof(int), nb * sizeof(int));
    if (nbatches) *nbatches = u.nbatches;
}

}  // namespace

void amplitudes_bp(State* s, int nstrings, const int32_t* configs, const tnqs_bp_opts* o, double* out_log_re_im, int32_t* niter, double* final_diff, int32_t* flags,
                   size_t budget, int* nbatches) {
    const Graph& g = *s->g;
    if (nstrings < 0) throw Err(TNQS_ERR_INVALID, "amplitudes_bp: negative number of strings");
    if (nbatches) *nbatches = 0;
    if (nstrings == 0) return;
    if (!out_log_re_im || (!configs && g.nv > 0)) throw Err(TNQS_ERR_INVALID, "amplitudes_bp: null argument");
    if (o && o->n_sequence > 0 && (!o->seq_src || !o->seq_dst)) throw Err(TNQS_ERR_INVALID, "amplitudes_bp: null edge sequence");
    for (size_t n = 0; n < (size_t)nstrings; ++n)
        for (int v = 0; v < g.nv; ++v) {
            const int x = configs[n * g.nv + v];
            if (x < 0 || x >= s->d[v]) throw Err(TNQS_ERR_INVALID, "amplitudes_bp: configuration " + std::to_string(x) + " of vertex " + std::to_string(v) + " in string " +
                                                                       std::to_string(n) + " is outside 0.." + std::to_string(s->d[v] - 1));
        }
    if (s->sharded()) throw Err(TNQS_ERR_UNSUPPORTED, "amplitudes_bp: sharded handles are not supported");
    for (int v = 0; v < g.nv; ++v) {
        if (g.nbr[v].size() > 7) throw Err(TNQS_ERR_UNSUPPORTED, "amplitudes_bp: a vertex of more than 7 neighbours is not supported");
        if (site_nelem(s, v) / (size_t)s->d[v] > (size_t(1) << 30)) throw Err(TNQS_ERR_UNSUPPORTED, "amplitudes_bp: a site tensor slice of more than 2^30 elements is not supported");
    }
    for (int e = 0; e < g.ne; ++e)
        if (!amp_covers(s->chi[e])) throw Err(TNQS_ERR_UNSUPPORTED, "amplitudes_bp: bond dimensions beyond 64 are not supported (amp_leg_gemm_kernel, amp_finalize_kernel)");
    HIPCHK(hipSetDevice(s->device));
    // the state as the reference holds it: deferred one-site gates applied (they act on the site index, which is fixed here); pending real scale factors multiply the
    // vertex scalars -- unless the messages are left un-normalised, which carry the tensors' absolute scale themselves
    materialize_pending_all(s);
    if (!(o ? o->normalize : 1)) materialize_scale_all(s);
    if (!budget) {
        size_t free_b = 0, total_b = 0;
        HIPCHK(hipMemGetInfo(&free_b, &total_b));
        budget = std::min<size_t>(size_t(2) << 30, free_b / 4);
    }
    if (s->dtype == TNQS_C64) amplitudes_bp_t<float>(s, nstrings, configs, o, out_log_re_im, niter, final_diff, flags, budget, nbatches);
    else amplitudes_bp_t<double>(s, nstrings, configs, o, out_log_re_im, niter, final_diff, flags, budget, nbatches);
}

}  // namespace tnqs
