// api.cpp -- extern "C" boundary of libtnqs_hip.so (include/tnqs.h).  No C++ exception crosses the ABI.
#include <cmath>
#include <cstring>
#include <string>
#include "api_guard.hpp"

using namespace tnqs;

static thread_local std::string g_err;
void tnqs::set_last_error(const char* msg) { g_err = msg; }

extern "C" {

int tnqs_version(void) { return 102; }
const char* tnqs_last_error(void) { return g_err.c_str(); }
int tnqs_device_count(int* count) {
    return guard([&] { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) n = 0; if (count) *count = n; });
}

int tnqs_create(int nv, int ne, const int32_t* es, const int32_t* ed, const int32_t* sd, int dtype, int device, tnqs_handle* out) {
    return guard([&] {
        if (!out) throw Err(TNQS_ERR_INVALID, "tnqs_create: out is null");
        if (ne > 0 && (!es || !ed)) throw Err(TNQS_ERR_INVALID, "tnqs_create: edge arrays are null");
        State* s = state_create(nv, ne, es, ed, sd, dtype, device);
        *out = new tnqs_state_s{s};
    });
}
int tnqs_destroy(tnqs_handle h) {
    return guard([&] { if (!h) return; if (h->s) { (void)hipSetDevice(h->s->device); if (h->s->stream) (void)hipStreamSynchronize(h->s->stream); delete h->s; } delete h; });
}
int tnqs_copy(tnqs_handle h, tnqs_handle* out) {
    return guard([&] { if (!out) throw Err(TNQS_ERR_INVALID, "tnqs_copy: out is null"); *out = new tnqs_state_s{state_copy(S(h))}; });
}
int tnqs_scalartype(tnqs_handle h, int* dtype) { return guard([&] { if (!dtype) throw Err(TNQS_ERR_INVALID, "scalartype: null output"); *dtype = S(h)->scalartype(); }); }
int tnqs_set_stream(tnqs_handle h, void* stream) {
    return guard([&] {
        State* s = S(h);
        if (s->own_stream && s->stream) { (void)hipStreamSynchronize(s->stream); (void)hipStreamDestroy(s->stream); }
        s->stream = reinterpret_cast<hipStream_t>(stream); s->own_stream = false;
    });
}

int tnqs_set_site_tensor(tnqs_handle h, int v, const void* host, int ndim, const int64_t* dims, const int32_t* role) {
    return guard([&] { if (!dims || !role) throw Err(TNQS_ERR_INVALID, "set_site_tensor: null argument"); state_set_site(S(h), v, host, ndim, dims, role); });
}
int tnqs_set_site_random(tnqs_handle h, int v, int n_neighbours, const int64_t* bond_dims, uint64_t seed, double scale) {
    return guard([&] { if (!bond_dims && n_neighbours > 0) throw Err(TNQS_ERR_INVALID, "set_site_random: null bond_dims"); state_set_site_random(S(h), v, n_neighbours, bond_dims, seed, scale); });
}
int tnqs_get_site_tensor(tnqs_handle h, int v, void* host, int ndim, const int32_t* role) {
    return guard([&] { if (!host || !role) throw Err(TNQS_ERR_INVALID, "get_site_tensor: null argument"); state_get_site(S(h), v, host, ndim, role); });
}
int tnqs_site_tensor_size(tnqs_handle h, int v, int64_t* n) {
    return guard([&] { State* s = S(h); if (v < 0 || v >= s->g->nv) throw Err(TNQS_ERR_INVALID, "bad vertex"); *n = state_site_size(s, v); });
}
int tnqs_set_message(tnqs_handle h, int src, int dst, const void* host, int chi) {
    return guard([&] { if (!host) throw Err(TNQS_ERR_INVALID, "set_message: null"); state_set_message(S(h), src, dst, host, chi); });
}
int tnqs_get_message(tnqs_handle h, int src, int dst, void* host, int chi) {
    return guard([&] { if (!host) throw Err(TNQS_ERR_INVALID, "get_message: null"); state_get_message(S(h), src, dst, host, chi); });
}
int tnqs_bond_dim(tnqs_handle h, int u, int v, int* chi) {
    return guard([&] { State* s = S(h); int e = s->g->edge(u, v); if (e < 0) throw Err(TNQS_ERR_INVALID, "bond_dim: not an edge"); *chi = s->chi[e]; });
}
int tnqs_maxvirtualdim(tnqs_handle h, int* chi) {
    return guard([&] { State* s = S(h); int m = 1; for (int c : s->chi) m = c > m ? c : m; *chi = m; });
}

int tnqs_bp_update(tnqs_handle h, const tnqs_bp_opts* o, int* niter, double* diff) {
    return guard([&] { State* s = S(h); s->stats = tnqs_apply_stats{}; bp_update(s, o, niter, diff); });
}
int tnqs_apply_gates(tnqs_handle h, int ngates, const int32_t* nverts, const int32_t* verts, const double* mats,
                     const tnqs_apply_opts* opts, const tnqs_bp_opts* bp, double* errs, tnqs_apply_stats* stats) {
    return guard([&] {
        State* s = S(h);
        if (ngates < 0 || (ngates > 0 && (!nverts || !verts || !mats))) throw Err(TNQS_ERR_INVALID, "apply_gates: null argument");
        apply_gates(s, ngates, nverts, verts, mats, opts, bp, errs);
        if (stats) *stats = s->stats;
    });
}
int tnqs_truncate(tnqs_handle h, int maxdim, double cutoff, int normalize, int ngroups, const int32_t* offs,
                  const int32_t* eu, const int32_t* ev, const tnqs_bp_opts* bp, tnqs_apply_stats* stats) {
    return guard([&] { State* s = S(h); truncate_bp(s, maxdim, cutoff, normalize, ngroups, offs, eu, ev, bp); if (stats) *stats = s->stats; });
}
int tnqs_rdm_1site(tnqs_handle h, int v, double* out) {
    return guard([&] { if (!out) throw Err(TNQS_ERR_INVALID, "rdm_1site: null"); rdm_1site(S(h), v, out); });
}
int tnqs_expect_1site(tnqs_handle h, int v, const double* op, double* out) {
    return guard([&] {
        State* s = S(h);
        if (!op || !out) throw Err(TNQS_ERR_INVALID, "expect_1site: null");
        if (v < 0 || v >= s->g->nv) throw Err(TNQS_ERR_INVALID, "expect_1site: bad vertex");
        int d = s->d[v];
        std::vector<double> r(2 * (size_t)d * d);
        rdm_1site(s, v, r.data());
        double nre = 0, nim = 0, tre = 0, tim = 0;
        for (int sp = 0; sp < d; ++sp) for (int si = 0; si < d; ++si) {
            double ore = op[2 * (sp + d * si)], oim = op[2 * (sp + d * si) + 1];
            double rre = r[2 * (si + d * sp)], rim = r[2 * (si + d * sp) + 1];
            nre += ore * rre - oim * rim; nim += ore * rim + oim * rre;
        }
        for (int si = 0; si < d; ++si) { tre += r[2 * (si + d * si)]; tim += r[2 * (si + d * si) + 1]; }
        double den = tre * tre + tim * tim;
        out[0] = (nre * tre + nim * tim) / den; out[1] = (nim * tre - nre * tim) / den;
    });
}
int tnqs_expect_region(tnqs_handle h, int nr, const int32_t* rv, const int32_t* parent, const double* ops, double* out4) {
    return guard([&] { expect_region(S(h), nr, rv, parent, ops, out4); });
}
int tnqs_vertex_scalars(tnqs_handle h, double* out) { return guard([&] { if (!out) throw Err(TNQS_ERR_INVALID, "vertex_scalars: null"); vertex_scalars(S(h), out); }); }
int tnqs_edge_scalars(tnqs_handle h, double* out) { return guard([&] { if (!out) throw Err(TNQS_ERR_INVALID, "edge_scalars: null"); edge_scalars(S(h), out); }); }
int tnqs_rescale(tnqs_handle h) { return guard([&] { rescale(S(h)); }); }
int tnqs_rescale_messages(tnqs_handle h, int n_edges, const int32_t* eu, const int32_t* ev) {
    return guard([&] { if (n_edges < 0) throw Err(TNQS_ERR_INVALID, "rescale_messages: negative count"); rescale_messages(S(h), n_edges, eu, ev); });
}
int tnqs_rescale_vertices(tnqs_handle h, int n_vertices, const int32_t* verts) {
    return guard([&] { if (n_vertices < 0) throw Err(TNQS_ERR_INVALID, "rescale_vertices: negative count"); rescale_vertices(S(h), n_vertices, verts); });
}
int tnqs_symmetric_gauge(tnqs_handle h, double regularization) { return guard([&] { symmetric_gauge(S(h), regularization); }); }
int tnqs_project_site(tnqs_handle h, int v, int config) { return guard([&] { project_site(S(h), v, config); }); }
int tnqs_site_dim(tnqs_handle h, int v, int* d) { return guard([&] { if (!d) throw Err(TNQS_ERR_INVALID, "site_dim: null output"); site_dim(S(h), v, d); }); }
int tnqs_site_probabilities(tnqs_handle h, int v, double* out_p) { return guard([&] { if (!out_p) throw Err(TNQS_ERR_INVALID, "site_probabilities: null output"); site_probabilities(S(h), v, out_p); }); }
int tnqs_sample_bp(tnqs_handle h, int nsamples, const tnqs_bp_opts* bp_opts, uint64_t seed, const double* uniforms, int32_t* out_config, double* out_prob, tnqs_apply_stats* stats) {
    return guard([&] { sample_bp(S(h), nsamples, bp_opts, seed, uniforms, out_config, out_prob, stats); });
}
int tnqs_loop_weights(tnqs_handle h, int ncycles, const int32_t* cycle_len, const int32_t* cycle_verts, double* out_re_im) {
    return guard([&] { loop_weights(S(h), ncycles, cycle_len, cycle_verts, out_re_im); });
}
int tnqs_config_weights(tnqs_handle h, int nconfigs, const int32_t* config_nedges, const int32_t* edge_u, const int32_t* edge_v, double* out_re_im) {
    return guard([&] { config_weights(S(h), nconfigs, config_nedges, edge_u, edge_v, out_re_im); });
}
int tnqs_rdm_edges(tnqs_handle h, int n_edges, const int32_t* edge_u, const int32_t* edge_v, double* out_rho) {
    return guard([&] { rdm_edges(S(h), n_edges, edge_u, edge_v, out_rho); });
}
int tnqs_bond_spectra(tnqs_handle h, int n_edges, const int32_t* edge_u, const int32_t* edge_v, double* out_spectra) {
    return guard([&] { bond_spectra(S(h), n_edges, edge_u, edge_v, out_spectra); });
}
int tnqs_rdm_paths(tnqs_handle h, int npaths, const int32_t* path_len, const int32_t* path_verts, double* out_rho) {
    return guard([&] { rdm_paths(S(h), npaths, path_len, path_verts, out_rho); });
}
int tnqs_inner_bp(tnqs_handle ket, tnqs_handle bra, const tnqs_bp_opts* opts, double* out_log_re_im, int* niter, double* final_diff) {
    return guard([&] { inner_bp(S(ket), S(bra), opts, out_log_re_im, niter, final_diff); });
}
int tnqs_expect_bmps(tnqs_handle h, const tnqs_bmps_opts* opts, const int32_t* vertex_row, const int32_t* vertex_col, int nobs, const int32_t* obs_nverts,
                     const int32_t* obs_verts, const double* obs_ops, double* out_numer_denom, double* out_log_norm_sqr, int32_t* out_fit_sweeps, double* out_fit_eps) {
    return guard([&] { expect_bmps(S(h), opts, vertex_row, vertex_col, nobs, obs_nverts, obs_verts, obs_ops, out_numer_denom, out_log_norm_sqr, out_fit_sweeps, out_fit_eps); });
}
int tnqs_amplitudes_bp(tnqs_handle h, int nstrings, const int32_t* configs, const tnqs_bp_opts* opts, double* out_log_re_im, int32_t* niter, double* final_diff, int32_t* flags) {
    return guard([&] { amplitudes_bp(S(h), nstrings, configs, opts, out_log_re_im, niter, final_diff, flags); });
}
int tnqs_expect_all(tnqs_handle h, const double* ops, double* out) {
    return guard([&] { if (!ops || !out) throw Err(TNQS_ERR_INVALID, "expect_all: null"); expect_all(S(h), ops, out); });
}

int tnqs_set_sharding(tnqs_handle h, int rank, int nranks, const int32_t* owner, tnqs_allgather_fn fn, void* ctx,
                      void* exch_dev, int64_t exch_bytes) {
    return guard([&] {
        State* s = S(h);
        if (nranks < 1 || rank < 0 || rank >= nranks) throw Err(TNQS_ERR_INVALID, "set_sharding: bad rank");
        if (nranks > 1) {
            if (!owner || !fn || !exch_dev || exch_bytes <= 0) throw Err(TNQS_ERR_INVALID, "set_sharding: owner, callback and exchange buffer are required for nranks > 1");
            for (int v = 0; v < s->g->nv; ++v) if (owner[v] < 0 || owner[v] >= nranks) throw Err(TNQS_ERR_INVALID, "set_sharding: owner out of range");
            s->owner.assign(owner, owner + s->g->nv);
        } else s->owner.clear();
        // one-site gates deferred while the handle was unsharded are applied NOW, while every tensor is still here: afterwards an accessor only
        // touches the vertices its rank owns, and a pending set that differs between ranks would give the two ranks of a gate different thetas
        materialize_pending_all(s);
        s->comm.reset();       // callback transport from here on: a communicator of an earlier tnqs_set_sharding_rccl must not keep serving exchange()
        s->rank = rank; s->nranks = nranks; s->ag_fn = fn; s->ag_ctx = ctx; s->exch = exch_dev; s->exch_bytes = (size_t)exch_bytes;
        if (nranks > 1) for (int v = 0; v < s->g->nv; ++v) if (!s->owns(v)) { s->site[v] = nullptr; s->sscale[v] = nullptr; }   // only owners hold site tensors
    });
}

int tnqs_rccl_unique_id(void* out128) { return guard([&] { if (!out128) throw Err(TNQS_ERR_INVALID, "rccl_unique_id: null output"); rccl_unique_id(out128); }); }
int tnqs_set_sharding_rccl(tnqs_handle h, int rank, int nranks, const int32_t* owner, const void* unique_id128, int64_t exch_bytes) {
    return guard([&] { set_sharding_rccl(S(h), rank, nranks, owner, unique_id128, exch_bytes); });
}
int tnqs_sharding_stats(tnqs_handle h, int64_t* n_exchanges, int64_t* bytes_exchanged) {
    return guard([&] { State* s = S(h); if (n_exchanges) *n_exchanges = s->comm ? s->comm->n_exchanges : 0; if (bytes_exchanged) *bytes_exchanged = s->comm ? s->comm->bytes_exchanged : 0; });
}
int tnqs_rccl_selftest(int device, int64_t bytes) { return guard([&] { rccl_selftest(device, bytes); }); }
int tnqs_rccl_preflight(void) { return guard([&] { rccl_preflight(); }); }

int tnqs_profile_enable(tnqs_handle h, int on) { return guard([&] { S(h)->prof->on = on != 0; }); }
int tnqs_profile_get(tnqs_handle h, int cls, int64_t* launches, double* ms, double* bytes, double* flops) {
    return guard([&] {
        State* s = S(h);
        if (cls < 0 || cls >= TNQS_PROF_NCLASSES) throw Err(TNQS_ERR_INVALID, "profile_get: bad class");
        prof_collect(s);
        const ProfClass& pc = s->prof->cls[cls];
        if (launches) *launches = pc.launches;
        if (ms) *ms = pc.ms;
        if (bytes) *bytes = pc.bytes;
        if (flops) *flops = pc.flops;
    });
}
int tnqs_profile_reset(tnqs_handle h) {
    return guard([&] { State* s = S(h); prof_collect(s); for (auto& p : s->prof->cls) p = ProfClass{}; });
}

}  // extern "C"
