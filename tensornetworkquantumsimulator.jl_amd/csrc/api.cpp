// api.cpp -- extern "C" boundary of libtnqs_hip.so (include/tnqs.h).  No C++ exception crosses the ABI.
#include <cmath>
#include <cstring>
#include <string>
#include "engine.hpp"

using namespace tnqs;

struct tnqs_state_s { State* s; };

static thread_local std::string g_err;

template <class F> static int guard(F&& f) {
    try { f(); return TNQS_OK; }
    catch (const Err& e) { g_err = e.what(); return e.code; }
    catch (const std::bad_alloc&) { g_err = "out of host memory"; return TNQS_ERR_HIP; }
    catch (const std::exception& e) { g_err = e.what(); return TNQS_ERR_INVALID; }
    catch (...) { g_err = "unknown error"; return TNQS_ERR_INVALID; }
}
static State* S(tnqs_handle h) { if (!h || !h->s) throw Err(TNQS_ERR_INVALID, "null handle"); return h->s; }

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

// ---- kernel-level debug entry points (include/tnqs_debug.h) ---------------------------------------------------
#include "../../include/tnqs_debug.h"
#include "kernels.hpp"
namespace tnqs { void dbg_default_sequence(const Graph& g, std::vector<int>& src, std::vector<int>& dst);
                 std::shared_ptr<Graph> dbg_make_graph(int nv, int ne, const int32_t* es, const int32_t* ed);
                 void dbg_default_sequence_graph(const Graph& g, std::vector<int>& src, std::vector<int>& dst, std::vector<int>& level);
                 void dbg_pair(int C0, int NMID, int NHI, const void* in, const void* Mx, const void* My, void* out);
                 void dbg_gram_fused(int PA, int K, int PB, const void* X, const void* Y, const void* M, void* out);
                 void dbg_gauge_gram(int z, const int* chi, int bleg, const void* X, const void* M, void* out);
                 void dbg_jacobi(int dtype, int m, int n, void* A, void* V, int* sweeps);
                 void dbg_chol(int n, const void* G, void* L, void* W, int* fail, double tau);
                 void dbg_theta_svd_pre(int m, int n, int nq, void* A, const void* Q, void* V, int* sweeps, int copies, int reps, double* ms, double* phase_us, int cap);
                 void dbg_time_jacobi_f32(int m, int n, const void* A, int copies, int reps, double* ms, int* sweeps);
                 void dbg_pair_legs(int d, int z, const int* chi, int lx, int ly, const void* in, const void* Mx, const void* My, void* out);
                 void dbg_pair_gram2(int d, int z, const int* chi, int lx, int ly, const void* X, const void* Y, const void* Mx, const void* My, void* out_y, void* out_x);
                 void dbg_bench_plane(int which, int nsites, int lx, int ly, int reps, double* ms);
                 void dbg_pair_gram(int d, int z, const int* chi, int lx, int ly, const void* X, const void* Y, const void* M, void* out);
                 void dbg_fiber_gemm(int dtype, int D, int PA, int K, int PB, int Do, int No, const void* in, const void* X, void* out, double* norm2, int use_mfma);
                 void dbg_gram(int dtype, int D, int PA, int K, int PB, const void* X, const void* Y, void* out, int acc64, int use_mfma);
                 void dbg_rowgemm(int D, int K, int nitems, const int* PA, const int* PB, const int* No, const void* in, const void* X, void* out, double* norm2, int tpw, int* route);
                 void dbg_gram_mfma(int nitems, const int* shape, const void* X, const void* Y, void* out, int nchunks, int* route);
                 void dbg_pair16(int d, int nitems, const int* z, const int* chi, const int* lx, const int* ly, const void* in, const void* M, void* out, int spw, int* route);
                 void dbg_pair_gram2x16(int d, int nitems, const int* z, const int* chi, const int* lx, const int* ly, const int* both, const void* X, const void* Y, const void* M,
                                        void* out_y, void* out_x, int spw);
                 void dbg_svd_tall(int nitems, const int* m, const int* n, void* A, int* chol_fail, int* polished, int* sweeps);
                 void dbg_small_site(int nitems, const int* d, const int* z, const int* chi, const int* jo, const void* psi, const void* M, const int* present, int form,
                                     const void* old_msg, const int* has_old, int normalize, void* out, void* new_msg, double* diff, int* route);
                 void dbg_msg_finalize(int dtype, int nitems, const int* chi, const int* nchunks, const void* partials, const void* old_msg, const int* has_old, int normalize,
                                       void* new_msg, double* diff);
                 void dbg_loop_cgemm(int dtype, int opB, int nitems, const int* m, const int* n, const int* k, const void* A, const void* B, void* C, int guard);
                 void dbg_loop_antiproject(int dtype, int nitems, const int* nr, const int* nc, void* T, const void* f, const void* b);
                 void dbg_loop_trace(int dtype, int nitems, const int* p, const int* q, const void* X, const void* Y, double* out);
                 void dbg_msg_rescale(int dtype, int nitems, const int* chi, const void* me, const void* mer, const int* present, void* me_out, void* mer_out, int guard);
                 void dbg_edge_scalar(int dtype, int nitems, const int* chi, const void* me, const void* mer, const int* present, double* out);
                 void dbg_env_prepare(int dtype, int nitems, const int* n, const void* msg, const int* present, void* H_out, void* V_out, int guard);
                 void dbg_env_finish(int dtype, int nitems, const int* n, const void* A, const void* V, const double* cutoff, void* msqrt_out, void* proj_out, int* flags_out, int guard);
                 void dbg_symg_build(int dtype, int nitems, const int* n, const void* AX, const void* VX, const void* AY, const void* VY, double reg, void* rx, void* ry, void* irx, void* iry,
                                     void* Ce, void* Ce0, int* flag_out, int guard);
                 void dbg_symg_finish(int dtype, int nitems, const int* n, const void* USigma, const void* Vsvd, const void* irx, const void* iry, void* Xs, void* Xd, double* S, int guard);
                 void dbg_diag(int dtype, int nitems, const int* chi, const double* S, void* out, int guard);
                 void dbg_cscale(int dtype, int nitems, const int* len, const void* src, const double* re, const double* im, void* dst, int guard);
                 void dbg_edge_rdm(int ptype, int nitems, const int* du, const int* dv, const int* chi, const int* nchunks_u, const int* nchunks_v, const void* partial_u, const void* partial_v,
                                   const double* scale_u, const double* scale_v, void* out, int guard);
                 void dbg_edge_rdm_mixed(int ptype_u, int ptype_v, int nitems, const int* du, const int* dv, const int* chi, const int* nchunks_u, const int* nchunks_v, const void* partial_u,
                                         const void* partial_v, const double* scale_u, const double* scale_v, void* out, int guard);
                 void dbg_bond_spectrum(int dtype, int nitems, const int* chi, const void* m1, const void* m2, const int* present, double* out, int* flags_out, int guard);
                 void dbg_path_apply(int ptype_in, int dtype, int nitems, const int* d, const int* chi_a, const int* chi_b, const int* nchunks_in, const int* ksplit, const void* L_in, const void* T,
                                     const double* scale, void* L_out, int guard);
                 int dbg_operator_sum(const void* gate, int d1, int d2, void* fa_out, void* fb_out);
                 void dbg_gate_theta(int dtype, int nitems, const int* dims, const int* mode, const int* rk, const void* F1, const void* F2, const double* tau, const void* gate,
                                     const int* maxdim, int lowrank_on, int stop_after, int* low_sizes, int* info, double* lam1, double* lam2, int* idx1, int* idx2,
                                     void* theta, void* theta0, void* thetaV, void* lowA, void* lowB, void* lowG, void* lowL, void* lowQ, void* lowL2c, int* texp, int* lowfail, int guard);
                 void dbg_gate_finish(int dtype, int nitems, const int* dims, const int* info_in, const int* texp, const void* theta, const void* thetaV, const double* lam1, const double* lam2,
                                      const int* idx1, const int* idx2, const void* GW1, const void* GW2, const int* maxdim, const double* cutoff, const int* normalize, const int* chi_cap,
                                      double* S, int* info_out, double* truncerr, void* X1, void* X2, int guard);
                 void dbg_theta_svd_stage(int dtype, int dyn, int nitems, const int* dims, const int* info, const int* K, const int* has_q, const void* Q, const int* rank_bounds,
                                          const int* cap, int recover_form, void* theta, void* theta0, void* thetaV, int* sweeps_out, int* route_out, int guard);
                 void dbg_qr2(int stage, int nitems, const int* n, const void* GW, const void* GV, const double* lam, const int* idx, const int* r, const void* A2, const void* V2, const double* tau,
                              void* X1, void* GVout, void* GWout, int* rk, int guard);
                 void dbg_small_svd(int dtype, int nitems, const int* shape, const void* src, void* GA, void* GV, int guard);
                 void dbg_inner_gram(int dtype, int nitems, const int* shape, const void* X, const void* Y, void* out, int max_chunks, int* nchunks_out, int guard, int* route);
                 void dbg_inner_finalize(int dtype, int nitems, const int* rows, const int* cols, const int* nchunks, const void* partials, const void* old_msg, const int* has_old,
                                         const int* normalize, void* new_msg, double* diff, double* sum, int guard);
                 void dbg_inner_scalar(int dtype, int nitems, const int* rows, const int* cols, const void* m, const void* mr, const int* present, const double* rawsum, const int* has_rawsum,
                                       const int* normalize, const double* scale_a, const double* scale_b, const int* has_scale, double* out, int guard);
                 void dbg_site_prob(int dtype, int n, int d, const void* tabs, const void* psi, int nblocks, double* partial, int guard, int* nblocks_out);
                 void dbg_site_draw(int nitems, const int* nblocks, const int* d, const double* partials, const double* neg_tol, const double* uniform, const int* use_counter,
                                    const unsigned long long* counter, const int* draw, double* p_out, int* x_out, double* px_out, int* status_out, int guard);
                 void dbg_site_project(int dtype, int nout, int d, const void* psi, int x, int x_on_device, void* out, int guard);
                 void dbg_site1(int nitems, const int* npairs, const void* in, const double* gates, int nbx, int normalize, void* out, double* partials, double* factors, int guard);
                 void dbg_norm_factor(int nitems, const int* npart, const double* partials, double* factors, int guard);
                 void dbg_scale(int dtype, int nitems, const int* len, const void* src, const double* factor, void* dst, int guard);
                 double dbg_pending_scale(State* s, int v); }
extern "C" {
int tnqs_dbg_default_sequence(tnqs_handle h, int* src, int* dst, int cap, int* n_out) {
    return guard([&] { std::vector<int> a, b; dbg_default_sequence(*S(h)->g, a, b); *n_out = (int)a.size();
                       for (int i = 0; i < (int)a.size() && i < cap; ++i) { src[i] = a[i]; dst[i] = b[i]; } });
}
int tnqs_dbg_default_sequence_graph(int nv, int ne, const int32_t* esrc, const int32_t* edst, int* src, int* dst, int* level, int cap, int* n_out) {
    return guard([&] { if (nv < 0 || ne < 0 || (ne > 0 && (!esrc || !edst)) || !n_out) throw Err(TNQS_ERR_INVALID, "tnqs_dbg_default_sequence_graph: bad arguments");
                       auto g = dbg_make_graph(nv, ne, esrc, edst); std::vector<int> a, b, l; dbg_default_sequence_graph(*g, a, b, l); *n_out = (int)a.size();
                       for (int i = 0; i < (int)a.size() && i < cap; ++i) { if (src) src[i] = a[i]; if (dst) dst[i] = b[i]; if (level) level[i] = l[i]; } });
}
int tnqs_dbg_gate_schedule(int nv, int ne, const int32_t* esrc, const int32_t* edst, int ngates, const int32_t* nverts, const int32_t* verts, int update_cache,
                           int* step_of_gate, int* step_is_bp, int cap, int* nsteps_out) {
    return guard([&] { if (nv < 0 || ne < 0 || (ne > 0 && (!esrc || !edst)) || ngates < 0 || (ngates > 0 && (!nverts || !verts)) || !nsteps_out) throw Err(TNQS_ERR_INVALID, "tnqs_dbg_gate_schedule: bad arguments");
                       for (int i = 0, o = 0; i < ngates; o += nverts[i], ++i) { if (nverts[i] < 1 || nverts[i] > 2) throw Err(TNQS_ERR_INVALID, "tnqs_dbg_gate_schedule: only one- and two-site gates");
                                                                                 for (int k = 0; k < nverts[i]; ++k) if (verts[o + k] < 0 || verts[o + k] >= nv) throw Err(TNQS_ERR_INVALID, "tnqs_dbg_gate_schedule: vertex out of range"); }
                       auto g = dbg_make_graph(nv, ne, esrc, edst); const GateSchedule steps = build_gate_schedule(*g, ngates, nverts, verts, update_cache != 0); *nsteps_out = (int)steps.size();
                       for (int k = 0; k < (int)steps.size(); ++k) { if (step_is_bp && k < cap) step_is_bp[k] = steps[k].is_bp ? 1 : 0; if (step_of_gate) for (int i = steps[k].begin; i < steps[k].end; ++i) step_of_gate[i] = k; } });
}
int tnqs_dbg_fiber_plan(int use, int dtype, int use_mfma, int use_chi64, int nitems, const int* shape, int* launches, int cap, int* nlaunches_out, int* items_out) {
    return guard([&] { if (use < 0 || use > 2 || (dtype != TNQS_C64 && dtype != TNQS_C128) || nitems < 0 || (nitems > 0 && !shape) || !nlaunches_out) throw Err(TNQS_ERR_INVALID, "tnqs_dbg_fiber_plan: bad arguments");
                       std::vector<FiberItem> items(nitems);
                       for (int i = 0; i < nitems; ++i) { const int* q = shape + 6 * i; for (int k = 0; k < 6; ++k) if (q[k] < 1) throw Err(TNQS_ERR_INVALID, "tnqs_dbg_fiber_plan: bad shape");
                                                          FiberItem& it = items[i]; it.D = q[0]; it.PA = q[1]; it.K = q[2]; it.PB = q[3]; it.Do = q[4]; it.No = q[5]; }
                       const std::vector<FiberLaunch> plan = plan_fiber_pass(items.data(), nitems, fiber_rules(use == 0 ? FiberUse::Chain : use == 1 ? FiberUse::Epilogue : FiberUse::Plain, dtype == TNQS_C64, use_mfma != 0, use_chi64 != 0),
                                                                            dtype == TNQS_C64 ? 8 : 16);
                       *nlaunches_out = (int)plan.size();
                       for (int l = 0; l < (int)plan.size(); ++l) { const FiberLaunch& L = plan[l];
                           if (launches && l < cap) { const int v[10] = {(int)L.route, L.D, L.K, L.TR, L.tpw, L.KKmax, L.NNmax, L.wgs, (int)L.items.size(), L.general ? 1 : 0}; std::copy(v, v + 10, launches + 10 * l); }
                           if (items_out) for (size_t k = 0; k < L.items.size(); ++k) { const FiberItem& it = L.items[k]; const int v[7] = {l, it.tile_begin, L.nwg[k], it.TA, it.TB, it.nta, it.ntb}; std::copy(v, v + 7, items_out + 7 * L.index[k]); } } });
}
int tnqs_dbg_jacobi(int dtype, int m, int n, void* A, void* V, int* sweeps) { return guard([&] { dbg_jacobi(dtype, m, n, A, V, sweeps); }); }
int tnqs_dbg_theta_svd_pre(int m, int n, int nq, void* A, const void* Q, void* V, int* sweeps, int copies, int reps, double* ms, double* phase_us, int cap) { return guard([&] { dbg_theta_svd_pre(m, n, nq, A, Q, V, sweeps, copies, reps, ms, phase_us, cap); }); }
int tnqs_dbg_time_jacobi_f32(int m, int n, const void* A, int copies, int reps, double* ms, int* sweeps) { return guard([&] { dbg_time_jacobi_f32(m, n, A, copies, reps, ms, sweeps); }); }
int tnqs_dbg_chol(int n, const void* G, void* L, void* W, int* fail, double tau) { return guard([&] { dbg_chol(n, G, L, W, fail, tau); }); }
int tnqs_dbg_fiber_gemm(int dtype, int D, int PA, int K, int PB, int Do, int No, const void* in, const void* X, void* out, double* norm2, int use_mfma) {
    return guard([&] { dbg_fiber_gemm(dtype, D, PA, K, PB, Do, No, in, X, out, norm2, use_mfma); });
}
int tnqs_dbg_pair(int C0, int NMID, int NHI, const void* in, const void* Mx, const void* My, void* out) { return guard([&] { dbg_pair(C0, NMID, NHI, in, Mx, My, out); }); }
int tnqs_dbg_pair_legs(int d, int z, const int* chi, int lx, int ly, const void* in, const void* Mx, const void* My, void* out) { return guard([&] { dbg_pair_legs(d, z, chi, lx, ly, in, Mx, My, out); }); }
int tnqs_dbg_pair_gram2(int d, int z, const int* chi, int lx, int ly, const void* X, const void* Y, const void* Mx, const void* My, void* out_y, void* out_x) {
    return guard([&] { dbg_pair_gram2(d, z, chi, lx, ly, X, Y, Mx, My, out_y, out_x); });
}
int tnqs_dbg_bench_plane(int which, int nsites, int lx, int ly, int reps, double* ms) { return guard([&] { dbg_bench_plane(which, nsites, lx, ly, reps, ms); }); }
int tnqs_dbg_pair_gram(int d, int z, const int* chi, int lx, int ly, const void* X, const void* Y, const void* M, void* out) { return guard([&] { dbg_pair_gram(d, z, chi, lx, ly, X, Y, M, out); }); }
int tnqs_dbg_gram_fused(int PA, int K, int PB, const void* X, const void* Y, const void* M, void* out) { return guard([&] { dbg_gram_fused(PA, K, PB, X, Y, M, out); }); }
int tnqs_dbg_gauge_gram(int z, const int* chi, int bleg, const void* X, const void* M, void* out) { return guard([&] { dbg_gauge_gram(z, chi, bleg, X, M, out); }); }
int tnqs_dbg_gram(int dtype, int D, int PA, int K, int PB, const void* X, const void* Y, void* out, int acc64, int use_mfma) {
    return guard([&] { dbg_gram(dtype, D, PA, K, PB, X, Y, out, acc64, use_mfma); });
}
int tnqs_dbg_rowgemm(int D, int K, int nitems, const int* PA, const int* PB, const int* No, const void* in, const void* X, void* out, double* norm2_out, int tpw, int* route_out) {
    return guard([&] { dbg_rowgemm(D, K, nitems, PA, PB, No, in, X, out, norm2_out, tpw, route_out); });
}
int tnqs_dbg_gram_mfma(int nitems, const int* shape, const void* X, const void* Y, void* out, int nchunks, int* route_out) {
    return guard([&] { dbg_gram_mfma(nitems, shape, X, Y, out, nchunks, route_out); });
}
int tnqs_dbg_pair16(int d, int nitems, const int* z, const int* chi, const int* lx, const int* ly, const void* in, const void* M, void* out, int spw, int* route_out) {
    return guard([&] { dbg_pair16(d, nitems, z, chi, lx, ly, in, M, out, spw, route_out); });
}
int tnqs_dbg_pair_gram2x16(int d, int nitems, const int* z, const int* chi, const int* lx, const int* ly, const int* both, const void* X, const void* Y, const void* M,
                           void* out_y, void* out_x, int spw) {
    return guard([&] { dbg_pair_gram2x16(d, nitems, z, chi, lx, ly, both, X, Y, M, out_y, out_x, spw); });
}
int tnqs_dbg_svd_tall(int nitems, const int* m, const int* n, void* A, int* chol_fail, int* polished, int* sweeps) {
    return guard([&] { dbg_svd_tall(nitems, m, n, A, chol_fail, polished, sweeps); });
}
int tnqs_dbg_small_site(int nitems, const int* d, const int* z, const int* chi, const int* jo, const void* psi, const void* M, const int* present, int form,
                        const void* old_msg, const int* has_old, int normalize, void* out, void* new_msg, double* diff_out, int* route_out) {
    return guard([&] { dbg_small_site(nitems, d, z, chi, jo, psi, M, present, form, old_msg, has_old, normalize, out, new_msg, diff_out, route_out); });
}
int tnqs_dbg_msg_finalize(int dtype, int nitems, const int* chi, const int* nchunks, const void* partials, const void* old_msg, const int* has_old, int normalize,
                          void* new_msg, double* diff_out) {
    return guard([&] { dbg_msg_finalize(dtype, nitems, chi, nchunks, partials, old_msg, has_old, normalize, new_msg, diff_out); });
}
int tnqs_dbg_loop_cgemm(int dtype, int opB, int nitems, const int* m, const int* n, const int* k, const void* A, const void* B, void* C, int guard_elems) {
    return guard([&] { dbg_loop_cgemm(dtype, opB, nitems, m, n, k, A, B, C, guard_elems); });
}
int tnqs_dbg_loop_antiproject(int dtype, int nitems, const int* nr, const int* nc, void* T, const void* f, const void* b) { return guard([&] { dbg_loop_antiproject(dtype, nitems, nr, nc, T, f, b); }); }
int tnqs_dbg_loop_trace(int dtype, int nitems, const int* p, const int* q, const void* X, const void* Y, double* out) { return guard([&] { dbg_loop_trace(dtype, nitems, p, q, X, Y, out); }); }
int tnqs_dbg_msg_rescale(int dtype, int nitems, const int* chi, const void* me, const void* mer, const int* present, void* me_out, void* mer_out, int guard_elems) {
    return guard([&] { dbg_msg_rescale(dtype, nitems, chi, me, mer, present, me_out, mer_out, guard_elems); });
}
int tnqs_dbg_edge_scalar(int dtype, int nitems, const int* chi, const void* me, const void* mer, const int* present, double* out_re_im) {
    return guard([&] { dbg_edge_scalar(dtype, nitems, chi, me, mer, present, out_re_im); });
}
int tnqs_dbg_env_prepare(int dtype, int nitems, const int* n, const void* msg, const int* present, void* H_out, void* V_out, int guard_elems) {
    return guard([&] { dbg_env_prepare(dtype, nitems, n, msg, present, H_out, V_out, guard_elems); });
}
int tnqs_dbg_env_finish(int dtype, int nitems, const int* n, const void* A, const void* V, const double* cutoff, void* msqrt_out, void* proj_out, int* flags_out, int guard_elems) {
    return guard([&] { dbg_env_finish(dtype, nitems, n, A, V, cutoff, msqrt_out, proj_out, flags_out, guard_elems); });
}
int tnqs_dbg_symg_build(int dtype, int nitems, const int* n, const void* AX, const void* VX, const void* AY, const void* VY, double reg, void* rx, void* ry, void* irx, void* iry,
                        void* Ce, void* Ce0, int* flag_out, int guard_elems) {
    return guard([&] { dbg_symg_build(dtype, nitems, n, AX, VX, AY, VY, reg, rx, ry, irx, iry, Ce, Ce0, flag_out, guard_elems); });
}
int tnqs_dbg_symg_finish(int dtype, int nitems, const int* n, const void* USigma, const void* Vsvd, const void* irx, const void* iry, void* Xs, void* Xd, double* S, int guard_elems) {
    return guard([&] { dbg_symg_finish(dtype, nitems, n, USigma, Vsvd, irx, iry, Xs, Xd, S, guard_elems); });
}
int tnqs_dbg_diag(int dtype, int nitems, const int* chi, const double* S, void* out, int guard_elems) { return guard([&] { dbg_diag(dtype, nitems, chi, S, out, guard_elems); }); }
int tnqs_dbg_cscale(int dtype, int nitems, const int* len, const void* src, const double* re, const double* im, void* dst, int guard_elems) {
    return guard([&] { dbg_cscale(dtype, nitems, len, src, re, im, dst, guard_elems); });
}
int tnqs_dbg_edge_rdm(int ptype, int nitems, const int* du, const int* dv, const int* chi, const int* nchunks_u, const int* nchunks_v, const void* partial_u, const void* partial_v,
                      const double* scale_u, const double* scale_v, void* out, int guard_elems) {
    return guard([&] { dbg_edge_rdm(ptype, nitems, du, dv, chi, nchunks_u, nchunks_v, partial_u, partial_v, scale_u, scale_v, out, guard_elems); });
}
int tnqs_dbg_rdm_edges_ws(tnqs_handle h, int n_edges, const int32_t* eu, const int32_t* ev, double* out, int64_t workspace_bytes, int* nbatches_out) {
    return guard([&] { if (workspace_bytes < 1) throw Err(TNQS_ERR_INVALID, "dbg_rdm_edges_ws: the workspace bound must be positive");
                       rdm_edges(S(h), n_edges, eu, ev, out, (size_t)workspace_bytes, nbatches_out); });
}
int tnqs_dbg_edge_rdm_mixed(int ptype_u, int ptype_v, int nitems, const int* du, const int* dv, const int* chi, const int* nchunks_u, const int* nchunks_v, const void* partial_u,
                            const void* partial_v, const double* scale_u, const double* scale_v, void* out, int guard_elems) {
    return guard([&] { dbg_edge_rdm_mixed(ptype_u, ptype_v, nitems, du, dv, chi, nchunks_u, nchunks_v, partial_u, partial_v, scale_u, scale_v, out, guard_elems); });
}
int tnqs_dbg_bond_spectrum(int dtype, int nitems, const int* chi, const void* m1, const void* m2, const int* present, double* out, int* flags_out, int guard_elems) {
    return guard([&] { dbg_bond_spectrum(dtype, nitems, chi, m1, m2, present, out, flags_out, guard_elems); });
}
int tnqs_dbg_path_apply(int ptype_in, int dtype, int nitems, const int* d, const int* chi_a, const int* chi_b, const int* nchunks_in, const int* ksplit, const void* L_in, const void* T,
                        const double* scale, void* L_out, int guard_elems) {
    return guard([&] { dbg_path_apply(ptype_in, dtype, nitems, d, chi_a, chi_b, nchunks_in, ksplit, L_in, T, scale, L_out, guard_elems); });
}
int tnqs_dbg_path_apply_plan(int nitems, const int* chi_a, const int* chi_b, const int* ksplit, int* ksplit_out, int* nrb_out) {
    return guard([&] { if (nitems < 1 || !chi_a || !chi_b || !ksplit || !ksplit_out || !nrb_out) throw Err(TNQS_ERR_INVALID, "dbg_path_apply_plan: bad arguments");
                       std::vector<PathApplyItem> it(nitems);
                       for (int i = 0; i < nitems; ++i) { if (chi_a[i] < 1 || chi_b[i] < 1 || ksplit[i] < 0) throw Err(TNQS_ERR_INVALID, "dbg_path_apply_plan: bad item");
                                                          it[i] = PathApplyItem{nullptr, nullptr, nullptr, nullptr, 1, chi_a[i], chi_b[i], 1, ksplit[i], 0, 0}; }
                       plan_path_apply(it.data(), nitems);
                       for (int i = 0; i < nitems; ++i) { ksplit_out[i] = it[i].ksplit; nrb_out[i] = it[i].nrb; } });
}
int tnqs_dbg_rdm_paths_ws(tnqs_handle h, int npaths, const int32_t* path_len, const int32_t* path_verts, double* out, int64_t workspace_bytes, int* nbatches_out) {
    return guard([&] { if (workspace_bytes < 1) throw Err(TNQS_ERR_INVALID, "dbg_rdm_paths_ws: the workspace bound must be positive");
                       rdm_paths(S(h), npaths, path_len, path_verts, out, (size_t)workspace_bytes, nbatches_out); });
}
int tnqs_dbg_pending_scale(tnqs_handle h, int v, double* factor) { return guard([&] { if (!factor) throw Err(TNQS_ERR_INVALID, "dbg_pending_scale: null output"); *factor = dbg_pending_scale(S(h), v); }); }
int tnqs_dbg_operator_sum(const void* gate, int d1, int d2, int* kappa_out, void* fa_out, void* fb_out) {
    return guard([&] { if (!kappa_out) throw Err(TNQS_ERR_INVALID, "dbg_operator_sum: null output"); *kappa_out = dbg_operator_sum(gate, d1, d2, fa_out, fb_out); });
}
int tnqs_dbg_gate_theta(int dtype, int nitems, const int* dims, const int* mode, const int* rk, const void* F1, const void* F2, const double* tau, const void* gate,
                        const int* maxdim, int lowrank_on, int stop_after, int* low_sizes_out, int* info, double* lam1, double* lam2, int* idx1, int* idx2,
                        void* theta, void* theta0, void* thetaV, void* lowA, void* lowB, void* lowG, void* lowL, void* lowQ, void* lowL2c, int* texp, int* lowfail, int guard_elems) {
    return guard([&] { dbg_gate_theta(dtype, nitems, dims, mode, rk, F1, F2, tau, gate, maxdim, lowrank_on, stop_after, low_sizes_out, info, lam1, lam2, idx1, idx2, theta, theta0, thetaV,
                                      lowA, lowB, lowG, lowL, lowQ, lowL2c, texp, lowfail, guard_elems); });
}
int tnqs_dbg_gate_finish(int dtype, int nitems, const int* dims, const int* info_in, const int* texp, const void* theta, const void* thetaV, const double* lam1, const double* lam2,
                         const int* idx1, const int* idx2, const void* GW1, const void* GW2, const int* maxdim, const double* cutoff, const int* normalize, const int* chi_cap,
                         double* S, int* info_out, double* truncerr, void* X1, void* X2, int guard_elems) {
    return guard([&] { dbg_gate_finish(dtype, nitems, dims, info_in, texp, theta, thetaV, lam1, lam2, idx1, idx2, GW1, GW2, maxdim, cutoff, normalize, chi_cap, S, info_out, truncerr, X1, X2, guard_elems); });
}
int tnqs_dbg_theta_svd_stage(int dtype, int dyn, int nitems, const int* dims, const int* info, const int* K, const int* has_q, const void* Q, const int* rank_bounds, const int* cap,
                             int recover_form, void* theta, void* theta0, void* thetaV, int* sweeps_out, int* route_out, int guard_elems) {
    return guard([&] { dbg_theta_svd_stage(dtype, dyn, nitems, dims, info, K, has_q, Q, rank_bounds, cap, recover_form, theta, theta0, thetaV, sweeps_out, route_out, guard_elems); });
}
int tnqs_dbg_qr2(int stage, int nitems, const int* n, const void* GW, const void* GV, const double* lam, const int* idx, const int* r, const void* A2, const void* V2, const double* tau,
                 void* X1, void* GVout, void* GWout, int* rk, int guard_elems) {
    return guard([&] { dbg_qr2(stage, nitems, n, GW, GV, lam, idx, r, A2, V2, tau, X1, GVout, GWout, rk, guard_elems); });
}
int tnqs_dbg_small_svd(int dtype, int nitems, const int* shape, const void* src, void* GA, void* GV, int guard_elems) {
    return guard([&] { dbg_small_svd(dtype, nitems, shape, src, GA, GV, guard_elems); });
}
int tnqs_dbg_inner_gram(int dtype, int nitems, const int* shape, const void* X, const void* Y, void* out, int max_chunks, int* nchunks_out, int guard_elems, int* route_out) {
    return guard([&] { dbg_inner_gram(dtype, nitems, shape, X, Y, out, max_chunks, nchunks_out, guard_elems, route_out); });
}
int tnqs_dbg_inner_finalize(int dtype, int nitems, const int* rows, const int* cols, const int* nchunks, const void* partials, const void* old_msg, const int* has_old,
                            const int* normalize, void* new_msg, double* diff_out, double* sum_out, int guard_elems) {
    return guard([&] { dbg_inner_finalize(dtype, nitems, rows, cols, nchunks, partials, old_msg, has_old, normalize, new_msg, diff_out, sum_out, guard_elems); });
}
int tnqs_dbg_inner_scalar(int dtype, int nitems, const int* rows, const int* cols, const void* m, const void* mr, const int* present, const double* rawsum, const int* has_rawsum,
                          const int* normalize, const double* scale_a, const double* scale_b, const int* has_scale, double* out_re_im, int guard_elems) {
    return guard([&] { dbg_inner_scalar(dtype, nitems, rows, cols, m, mr, present, rawsum, has_rawsum, normalize, scale_a, scale_b, has_scale, out_re_im, guard_elems); });
}
int tnqs_dbg_site_prob(int dtype, int n, int d, const void* tabs, const void* psi, int nblocks, double* partial, int guard_elems, int* nblocks_out) {
    return guard([&] { dbg_site_prob(dtype, n, d, tabs, psi, nblocks, partial, guard_elems, nblocks_out); });
}
int tnqs_dbg_site_draw(int nitems, const int* nblocks, const int* d, const double* partials, const double* neg_tol, const double* uniform, const int* use_counter,
                       const uint64_t* counter, const int* draw, double* p_out, int* x_out, double* px_out, int* status_out, int guard_elems) {
    return guard([&] { dbg_site_draw(nitems, nblocks, d, partials, neg_tol, uniform, use_counter, reinterpret_cast<const unsigned long long*>(counter), draw, p_out, x_out, px_out, status_out, guard_elems); });
}
int tnqs_dbg_site_project(int dtype, int nout, int d, const void* psi, int x, int x_on_device, void* out, int guard_elems) {
    return guard([&] { dbg_site_project(dtype, nout, d, psi, x, x_on_device, out, guard_elems); });
}
int tnqs_dbg_site1(int nitems, const int* npairs, const void* in, const double* gates, int nbx, int normalize, void* out, double* partials, double* factors, int guard_elems) {
    return guard([&] { dbg_site1(nitems, npairs, in, gates, nbx, normalize, out, partials, factors, guard_elems); });
}
int tnqs_dbg_norm_factor(int nitems, const int* npart, const double* partials, double* factors, int guard_elems) { return guard([&] { dbg_norm_factor(nitems, npart, partials, factors, guard_elems); }); }
int tnqs_dbg_scale(int dtype, int nitems, const int* len, const void* src, const double* factor, void* dst, int guard_elems) {
    return guard([&] { dbg_scale(dtype, nitems, len, src, factor, dst, guard_elems); });
}
int tnqs_dbg_inner_bp_ws(tnqs_handle ket, tnqs_handle bra, const tnqs_bp_opts* opts, double* out_log_re_im, int* niter, double* final_diff, int64_t workspace_bytes, int* nbatches_out) {
    return guard([&] { if (workspace_bytes < 1) throw Err(TNQS_ERR_INVALID, "dbg_inner_bp_ws: the workspace bound must be positive");
                       inner_bp(S(ket), S(bra), opts, out_log_re_im, niter, final_diff, (size_t)workspace_bytes, nbatches_out); });
}
}
