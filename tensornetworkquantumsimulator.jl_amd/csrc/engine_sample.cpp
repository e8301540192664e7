// engine_sample.cpp -- sampling bitstrings from a BP cache: sample(psi, nsamples; alg = "bp"), src/sampling.jl:18-43.
// Per sample: copy the cache; at every vertex in vertex order contract psi_v, conj psi_v and the incoming messages to the diagonal of rho_v, draw a configuration
// with those weights, replace psi_v by its slice (site dimension 1; bond dimensions and messages stay, as setindex_preserve! leaves them; no rescaling, as in the BP
// branch of the reference) and, unless v is the last vertex, update the messages.  The draw stays on the device (kernels_sample.hip): the slice and the BP update that
// follows are enqueued behind it without a host round trip; configurations and probabilities are read back once per sample.
#include "engine_internal.hpp"

namespace tnqs {

static void check_vertex(const State* s, int v, const char* who) {
    if (v < 0 || v >= s->g->nv) throw Err(TNQS_ERR_INVALID, std::string(who) + ": bad vertex");
    if (!s->site[v]) throw Err(TNQS_ERR_INVALID, std::string(who) + ": vertex not owned by this rank");
}
static void check_site_buffer(const State* s, int v, const SD& sd, const char* who) {
    if (s->site[v]->bytes != sd.n * s->esz()) throw Err(TNQS_ERR_INVALID, std::string(who) + ": bond dimensions are inconsistent with the stored tensor (set all neighbours first)");
}
[[noreturn]] static void throw_status(int status, int v, const char* who) {
    if (status & 1) throw Err(TNQS_ERR_NUMERIC, std::string(who) + ": tr(rho) of vertex " + std::to_string(v) + " is zero, negative or not finite");
    throw Err(TNQS_ERR_NUMERIC, std::string(who) + ": the reduced density matrix of vertex " + std::to_string(v) + " has a negative diagonal entry beyond rounding");
}

// diag(rho_v) partials and the draw kernel behind them, enqueued on the handle's stream.  The pending one-site gate of v is applied first (the diagonal sees it); a
// pending scale factor is not: p = diag / tr does not depend on it.
template <class T> static void enqueue_site_draw(State* s, int v, const double* d_uniform, uint64_t seed, uint64_t sample, uint64_t step, bool draw,
                                                 double* d_p, int* d_x, double* d_px, int* d_status, const char* who) {
    const Graph& g = *s->g;
    materialize_pending(s, {v});
    std::vector<Chain> chains(1);
    Chain& c = chains[0]; c.v = v; c.src = s->site[v]->p; c.sd = site_dims(s, v);
    check_site_buffer(s, v, c.sd, who);
    for (int j = 0; j < c.sd.z; ++j) { const int de = g.dedge(g.nbr[v][j], v); if (s->msg[de]) c.steps.push_back({j, s->msg[de]->p}); }
    run_chains<T>(s, chains, TNQS_PROF_SMALL);
    const int nb = plan_site_prob(c.sd.n, c.sd.d);
    Buf part = dalloc(s, (size_t)nb * 16 * sizeof(double));
    ProfScope ps(s, TNQS_PROF_SMALL, 2.0 * c.sd.n * s->esz(), 4.0 * c.sd.n);
    launch_site_prob_partial<T>(s->stream, chains[0].result, c.src, c.sd.n, c.sd.d, nb, reinterpret_cast<double*>(part->p));
    const double neg_tol = 100.0 * (double)std::numeric_limits<T>::epsilon();
    launch_site_draw(s->stream, reinterpret_cast<const double*>(part->p), nb, c.sd.d, neg_tol, d_uniform, seed, sample, step, draw, d_p, d_x, d_px, d_status);
    s->keepalive.push_back(part); s->keepalive.push_back(chains[0].tmp[0]); s->keepalive.push_back(chains[0].tmp[1]);
}

// psi_v <- psi_v[x, ...] with x from device memory (d_x) or from the host.  The pending scale factor stays beside the slice (the map is linear); unit_norm is gone.
template <class T> static void enqueue_project(State* s, int v, const int* d_x, int x_host) {
    const SD sd = site_dims(s, v);
    check_site_buffer(s, v, sd, "project_site");
    const size_t nout = sd.n / (size_t)sd.d;
    Buf out = dalloc(s, nout * s->esz());
    { ProfScope ps(s, TNQS_PROF_SMALL, 2.0 * nout * s->esz(), 0); launch_site_project<T>(s->stream, s->site[v]->p, out->p, nout, sd.d, d_x, x_host); }
    s->keepalive.push_back(s->site[v]);
    s->site[v] = out; s->d[v] = 1; s->unit_norm[v] = 0; s->projected[v] = 1;
}

void site_dim(const State* s, int v, int* d) {
    if (v < 0 || v >= s->g->nv) throw Err(TNQS_ERR_INVALID, "site_dim: bad vertex");
    *d = s->d[v];
}

void project_site(State* s, int v, int config) {
    if (s->sharded()) throw Err(TNQS_ERR_UNSUPPORTED, "project_site: sharded handles are not supported (the configuration would have to be agreed between the ranks)");
    check_vertex(s, v, "project_site");
    if (config < 0 || config >= s->d[v]) throw Err(TNQS_ERR_INVALID, "project_site: config " + std::to_string(config) + " outside [0, " + std::to_string(s->d[v]) + ")");
    HIPCHK(hipSetDevice(s->device));
    materialize_pending(s, {v});
    if (s->dtype == TNQS_C64) enqueue_project<float>(s, v, nullptr, config); else enqueue_project<double>(s, v, nullptr, config);
    sync(s);
}

void site_probabilities(State* s, int v, double* out) {
    check_vertex(s, v, "site_probabilities");
    HIPCHK(hipSetDevice(s->device));
    const int d = s->d[v];
    Buf d_p = dalloc(s, 16 * sizeof(double)), d_status = dalloc(s, sizeof(int));
    HIPCHK(hipMemsetAsync(d_status->p, 0, sizeof(int), s->stream));
    if (s->dtype == TNQS_C64) enqueue_site_draw<float>(s, v, nullptr, 0, 0, 0, false, reinterpret_cast<double*>(d_p->p), nullptr, nullptr, reinterpret_cast<int*>(d_status->p), "site_probabilities");
    else enqueue_site_draw<double>(s, v, nullptr, 0, 0, 0, false, reinterpret_cast<double*>(d_p->p), nullptr, nullptr, reinterpret_cast<int*>(d_status->p), "site_probabilities");
    reserve_readback(s, 512);
    const double* hp = readback<double>(s, d_p->p, (size_t)d);
    const int* hs = readback<int>(s, d_status->p, 1);
    sync(s);
    if (*hs) throw_status(*hs, v, "site_probabilities");
    std::copy(hp, hp + d, out);
}

template <class T> static void sample_bp_t(State* s, int nsamples, const tnqs_bp_opts* bp, uint64_t seed, const double* uniforms, int32_t* out_config, double* out_prob,
                                           tnqs_apply_stats* stats) {
    const Graph& g = *s->g;
    const int nv = g.nv;
    HIPCHK(hipSetDevice(s->device));
    for (int v = 0; v < nv; ++v) check_vertex(s, v, "sample_bp");
    tnqs_apply_stats total{};
    Buf d_u;
    if (uniforms) {
        d_u = dalloc(s, (size_t)nsamples * nv * sizeof(double));
        HIPCHK(hipMemcpyAsync(d_u->p, uniforms, (size_t)nsamples * nv * sizeof(double), hipMemcpyHostToDevice, s->stream));
    }
    Buf d_cfg = dalloc(s, (size_t)nv * sizeof(int)), d_px = dalloc(s, (size_t)nv * sizeof(double)), d_status = dalloc(s, sizeof(int));
    HIPCHK(hipStreamSynchronize(s->stream));
    // the status word of the draws travels to four pinned bytes of this call's own: not in a State's staging arena (reset inside the BP updates) and not in its
    // check ring (owned by the deferred verification: settle() rewinds it)
    struct Pinned { int* p = nullptr; ~Pinned() { if (p) (void)hipHostFree(p); } } pinned;
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&pinned.p), sizeof(int), hipHostMallocDefault));
    int* const h_st = pinned.p;
    for (int j = 0; j < nsamples; ++j) {
        std::unique_ptr<State> c(state_copy(s));                       // copy(bp_cache), src/sampling.jl:20: O(V + E), buffers shared
        c->stats = tnqs_apply_stats{};
        int* d_st = reinterpret_cast<int*>(d_status->p);
        HIPCHK(hipMemsetAsync(d_st, 0, sizeof(int), c->stream));
        *h_st = 0;
        for (int v = 0; v < nv; ++v) {
            const double* du = d_u ? reinterpret_cast<const double*>(d_u->p) + (size_t)j * nv + v : nullptr;
            enqueue_site_draw<T>(c.get(), v, du, seed, (uint64_t)j, (uint64_t)v, true, nullptr, reinterpret_cast<int*>(d_cfg->p) + v, reinterpret_cast<double*>(d_px->p) + v, d_st, "sample_bp");
            enqueue_project<T>(c.get(), v, reinterpret_cast<const int*>(d_cfg->p) + v, 0);
            HIPCHK(hipMemcpyAsync(h_st, d_st, sizeof(int), hipMemcpyDeviceToHost, c->stream));
            if (v + 1 < nv) {
                bp_update_t<T>(c.get(), bp, nullptr, nullptr);          // returns with the stream drained: the status of this vertex has arrived
                if (*h_st) throw_status(*h_st, v, "sample_bp");
            }
        }
        reserve_readback(c.get(), round256((size_t)nv * sizeof(int)) + round256((size_t)nv * sizeof(double)));
        const int* hc = readback<int>(c.get(), d_cfg->p, (size_t)nv);
        const double* hp = readback<double>(c.get(), d_px->p, (size_t)nv);
        sync(c.get());
        if (*h_st) throw_status(*h_st, nv - 1, "sample_bp");
        std::copy(hc, hc + nv, out_config + (size_t)j * nv);
        if (out_prob) std::copy(hp, hp + nv, out_prob + (size_t)j * nv);
        total.n_bp_updates += c->stats.n_bp_updates; total.n_bp_sweeps += c->stats.n_bp_sweeps; total.bp_not_converged += c->stats.bp_not_converged;
        total.n_bp_products_reused += c->stats.n_bp_products_reused; total.n_bp_products_evicted += c->stats.n_bp_products_evicted;
        total.last_bp_diff = c->stats.last_bp_diff;
    }
    if (stats) *stats = total;
}

void sample_bp(State* s, int nsamples, const tnqs_bp_opts* bp, uint64_t seed, const double* uniforms, int32_t* out_config, double* out_prob, tnqs_apply_stats* stats) {
    if (s->sharded()) throw Err(TNQS_ERR_UNSUPPORTED, "sample_bp: sharded handles are not supported (the configuration would have to be agreed between the ranks)");
    if (nsamples < 0) throw Err(TNQS_ERR_INVALID, "sample_bp: nsamples must be >= 0");
    if (nsamples > 0 && !out_config) throw Err(TNQS_ERR_INVALID, "sample_bp: out_config is null");
    if (uniforms) for (size_t k = 0; k < (size_t)nsamples * s->g->nv; ++k)
        if (!(uniforms[k] >= 0.0 && uniforms[k] < 1.0)) throw Err(TNQS_ERR_INVALID, "sample_bp: uniforms must lie in [0, 1)");
    if (nsamples == 0) { if (stats) *stats = tnqs_apply_stats{}; return; }
    if (s->dtype == TNQS_C64) sample_bp_t<float>(s, nsamples, bp, seed, uniforms, out_config, out_prob, stats);
    else sample_bp_t<double>(s, nsamples, bp, seed, uniforms, out_config, out_prob, stats);
}

}  // namespace tnqs
