// engine_paths.cpp -- two-site reduced density matrices of the two ENDS of paths in one call (tnqs_rdm_paths; the reference's reduced_density_matrix(cache, [u, w];
// alg = "bp"), src/rdm.jl:52-73, with the path p_0 = u, p_1, .., p_n = w as the Steiner tree).  With E as in engine_rdm.cpp:
//   L_0[s, s'; a, a']  = E_{p_0 -> p_1}[(s, a), (s', a')]                                                a: the bond p_0 - p_1
//   T_k[(b, b'), (a, a')]: the double-layer transfer matrix of p_k (engine_loops.cpp), a: the bond from p_{k-1}, b: the bond to p_{k+1}
//   L_k[s, s'; b, b']  = sum_{a, a'} L_{k-1}[s, s'; a, a'] T_k[(b, b'), (a, a')]                         k = 1 .. n - 1
//   rho_{p_0, p_k}     = sum_{a, a'} L_{k-1}[s_u, s_u'; a, a'] E_{p_k -> p_{k-1}}[(s_w, a), (s_w', a')]  k = 1 .. n
// so one path yields rho(p_0, p_k) for EVERY k: n backward environments, one forward environment, n - 1 transfer matrices, n - 1 thin products.  L keeps the
// Gram-partial layout of an environment, so L_0 IS the forward end's Gram partial and the bond contraction is edge_rdm_kernel on (L_{k-1}, E).  L is complex128
// from the first step on (path_apply_kernel, kernels_rdm.hip); it is not rescaled along the path.
// Paths are batched under a workspace bound; a batch issues one launch per stage over all its paths (ends and transfer matrices shared by several paths of the
// batch are built once), one apply launch per step of the sweep, the bond contractions at its end, and the call ends with ONE read-back.
#include "engine_internal.hpp"

namespace tnqs {

namespace {
struct PathPlan { const int32_t* v; int len; size_t off /* of (p_0, p_1) in the output, complex numbers */; size_t ws_bytes, part_unit; };
constexpr size_t kGramChunkFloor = 2048;      // plan_gram hands a launch of n jobs at most max(n, 2048) chunk groups

void check_path(const State* s, const int32_t* pv, int len) {
    const Graph& g = *s->g;
    if (len < 2) throw Err(TNQS_ERR_INVALID, "rdm_paths: a path has at least 2 vertices");
    for (int k = 0; k < len; ++k) {
        if (pv[k] < 0 || pv[k] >= g.nv) throw Err(TNQS_ERR_INVALID, "rdm_paths: bad vertex");
        for (int q = 0; q < k; ++q) if (pv[q] == pv[k]) throw Err(TNQS_ERR_INVALID, "rdm_paths: repeated vertex in a path");
    }
    for (int k = 0; k + 1 < len; ++k) if (g.edge(pv[k], pv[k + 1]) < 0) throw Err(TNQS_ERR_INVALID, "rdm_paths: consecutive vertices of a path must be neighbours");
    for (int k = 0; k < len; ++k) for (int q = k + 2; q < len; ++q)
        if (g.edge(pv[k], pv[q]) >= 0) throw Err(TNQS_ERR_INVALID, "rdm_paths: the path has a chord (two non-consecutive vertices are neighbours): only induced paths are supported");
}

// what the kernels cannot take, and the workspace of the path on its own: chain temporaries and Gram partial of every end, chain temporaries, permuted copies and T of
// every inner vertex, the L's at the largest split
PathPlan describe_path(const State* s, const int32_t* pv, int len, size_t off) {
    const Graph& g = *s->g;
    const size_t esz = s->esz();
    PathPlan p{pv, len, off, 0, 0};
    const int d0 = s->d[pv[0]];
    if (d0 * d0 > 16) throw Err(TNQS_ERR_UNSUPPORTED, "rdm_paths: site dimension of the first vertex above 4");
    auto end = [&](int u, int toward) {
        const SD sd = site_dims(s, u);
        const size_t KK = (size_t)sd.d * sd.chi[g.leg(u, toward)];
        p.ws_bytes += 2 * sd.n * esz;
        p.part_unit = std::max(p.part_unit, KK * KK * 16 * 4);      // one chunk group of the end's Gram (at most 4 partials of at most complex128)
    };
    end(pv[0], pv[1]);
    for (int k = 1; k < len; ++k) {
        end(pv[k], pv[k - 1]);
        const int chi = s->chi[g.edge(pv[k - 1], pv[k])];
        if (edge_rdm_block(d0, s->d[pv[k]], chi) < 1) throw Err(TNQS_ERR_UNSUPPORTED, "rdm_paths: bond too large for the edge kernel ((d_u^2 + d_w^2) chi must stay below 4096)");
        if (k + 1 == len) break;
        const SD sd = site_dims(s, pv[k]);
        if (sd.z + 1 > 8) throw Err(TNQS_ERR_UNSUPPORTED, "rdm_paths: vertex degree > 7");
        const size_t ca = chi, cb = s->chi[g.edge(pv[k], pv[k + 1])], t = ca * ca * cb * cb;
        if (t > (size_t)INT_MAX / 4) throw Err(TNQS_ERR_UNSUPPORTED, "rdm_paths: bond dimension too large for the transfer-matrix route");
        p.ws_bytes += (4 * sd.n + t) * esz + (size_t)kPathApplyMaxSplit * d0 * cb * d0 * cb * 16;
    }
    return p;
}

struct Carried { const void* p; int nchunks; bool f64; };      // L_k of a path: where it is, its chunks, its partial type
}  // namespace

template <class T> static void rdm_paths_batch(State* s, const std::vector<PathPlan>& paths, Buf d_out) {
    const Graph& g = *s->g;
    constexpr bool f32 = std::is_same<T, float>::value;
    const size_t esz = s->esz();
    // the distinct ends (vertex, leg) and transfer matrices (vertex, in-leg, out-leg) of the batch
    std::vector<EnvEnd> ends; std::vector<TransferVertex> tvs;
    std::map<std::pair<int, int>, int> end_of; std::map<std::array<int, 3>, int> tv_of;
    auto end_id = [&](int u, int toward) {
        const int leg = g.leg(u, toward);
        auto f = end_of.find({u, leg});
        if (f != end_of.end()) return f->second;
        EnvEnd x; x.u = u; x.leg = leg; x.sd = site_dims(s, u); x.KK = x.sd.d * x.sd.chi[leg]; x.cls = f32 ? env_f32_class(x.KK) : 0;
        if (!s->site[u]) throw Err(TNQS_ERR_INVALID, "rdm_paths: vertex not owned by this rank");
        ends.push_back(x); return end_of[{u, leg}] = (int)ends.size() - 1;
    };
    auto tv_id = [&](int v, int from, int to) {
        const int ja = g.leg(v, from), jb = g.leg(v, to);
        auto f = tv_of.find({v, ja, jb});
        if (f != tv_of.end()) return f->second;
        TransferVertex x{}; x.v = v; x.ja = ja; x.jb = jb; x.sd = site_dims(s, v); x.ca = x.sd.chi[ja]; x.cb = x.sd.chi[jb];
        tvs.push_back(x); return tv_of[{v, ja, jb}] = (int)tvs.size() - 1;
    };
    std::vector<std::vector<int>> pend(paths.size()), ptv(paths.size());      // per path: end 0 forward, end k backward of p_k; transfer matrix of p_k at k - 1
    int maxlen = 0;
    for (size_t q = 0; q < paths.size(); ++q) {
        const PathPlan& p = paths[q]; maxlen = std::max(maxlen, p.len);
        pend[q].push_back(end_id(p.v[0], p.v[1]));
        for (int k = 1; k < p.len; ++k) pend[q].push_back(end_id(p.v[k], p.v[k - 1]));
        for (int k = 1; k + 1 < p.len; ++k) ptv[q].push_back(tv_id(p.v[k], p.v[k - 1], p.v[k + 1]));
    }
    // 2. environments; 3. transfer matrices
    run_env_ends<T>(s, ends, 0, ends.size());
    {
        std::vector<TransferVertex*> lvs; for (auto& x : tvs) lvs.push_back(&x);
        if (!lvs.empty()) build_transfer_matrices<T>(s, lvs, "rdm_paths");
        for (auto& x : tvs) { x.phi.reset(); x.psi.reset(); }      // stream-ordered reuse: the GEMM that reads them is enqueued
    }
    auto scale_of = [&](int v) { return s->sscale[v] ? reinterpret_cast<const double*>(s->sscale[v]->p) : nullptr; };
    // 4. the sweep: L[q][k] = L_k of path q; step k of every path that still has an inner vertex p_k in one launch per input partial type
    std::vector<std::vector<Carried>> L(paths.size()); std::vector<Buf> keep;
    for (size_t q = 0; q < paths.size(); ++q) { const EnvEnd& e = ends[pend[q][0]]; L[q].push_back(Carried{e.partial->p, e.nchunks, e.cls == 0}); }
    for (int k = 1; k + 1 < maxlen; ++k) {
        std::vector<PathApplyItem> items[2]; std::vector<size_t> who[2]; double bytes[2] = {0, 0}, flops[2] = {0, 0};
        for (size_t q = 0; q < paths.size(); ++q) {
            if (k + 1 >= paths[q].len) continue;
            const TransferVertex& x = tvs[ptv[q][k - 1]]; const Carried& in = L[q][k - 1];
            const int c = in.f64 ? 1 : 0;
            items[c].push_back(PathApplyItem{in.p, x.T->p, nullptr, scale_of(x.v), s->d[paths[q].v[0]], x.ca, x.cb, in.nchunks, 0, 0, 0}); who[c].push_back(q);
        }
        for (int c = 0; c < 2; ++c) {
            if (items[c].empty()) continue;
            const int wgs = plan_path_apply(items[c].data(), (int)items[c].size());
            for (size_t i = 0; i < items[c].size(); ++i) {
                PathApplyItem& it = items[c][i];
                const size_t R = (size_t)it.d * it.d, na = (size_t)it.chi_a * it.chi_a, nb = (size_t)it.chi_b * it.chi_b;
                Buf o = dalloc(s, (size_t)it.ksplit * R * nb * 16); keep.push_back(o);
                it.L_out = o->p; L[who[c][i]].push_back(Carried{o->p, it.ksplit, true});
                bytes[c] += na * nb * esz + (double)it.nrb * it.nchunks_in * R * na * (c ? 16.0 : 8.0) + (double)it.ksplit * R * nb * 16; flops[c] += 8.0 * R * na * nb;
            }
            const PathApplyItem* d = upload(s, items[c]);
            ProfScope ps(s, TNQS_PROF_PATH_RDM, bytes[c], flops[c]);
            if (c) launch_path_apply<double, T>(s->stream, d, (int)items[c].size(), wgs); else launch_path_apply<float, T>(s->stream, d, (int)items[c].size(), wgs);
        }
    }
    // the bond contractions of all (path, k): (L_{k-1}, E_{p_k -> p_{k-1}}) straight into the call's output, one launch per pair of partial types
    std::vector<EdgeRdmItem> items[4]; double pbytes = 0, flops = 0;
    for (size_t q = 0; q < paths.size(); ++q) {
        const PathPlan& p = paths[q]; const int u = p.v[0], du = s->d[u]; size_t off = p.off;
        for (int k = 1; k < p.len; ++k) {
            const Carried& l = L[q][k - 1]; const EnvEnd& e = ends[pend[q][k]];
            const int w = p.v[k], dw = e.sd.d, chi = e.sd.chi[e.leg]; const bool e64 = e.cls == 0;
            items[(l.f64 ? 2 : 0) + (e64 ? 1 : 0)].push_back(EdgeRdmItem{l.p, e.partial->p, l.nchunks, e.nchunks, du, dw, chi, scale_of(u), scale_of(w),
                                                                            reinterpret_cast<char*>(d_out->p) + off * 16});
            const double ku = (double)du * chi, kw = (double)dw * chi;
            pbytes += l.nchunks * ku * ku * (l.f64 ? 16.0 : 8.0) + e.nchunks * kw * kw * (e64 ? 16.0 : 8.0) + 16.0 * du * du * dw * dw; flops += 8.0 * chi * chi * du * du * dw * dw;
            off += (size_t)du * dw * du * dw;
        }
    }
    const EdgeRdmItem* d[4]; for (int c = 0; c < 4; ++c) d[c] = upload(s, items[c]);
    ProfScope ps(s, TNQS_PROF_PATH_RDM, pbytes, flops);
    launch_edge_rdm_mixed<float, float>(s->stream, d[0], (int)items[0].size());
    launch_edge_rdm_mixed<float, double>(s->stream, d[1], (int)items[1].size());
    launch_edge_rdm_mixed<double, float>(s->stream, d[2], (int)items[2].size());
    launch_edge_rdm_mixed<double, double>(s->stream, d[3], (int)items[3].size());
}

// out_rho: for path q = 0 .., for k = 1 .. path_len[q] - 1, the (d_p0 d_pk)^2 complex128 matrix of (p_0, p_k); budget == 0: min(2 GiB, a quarter of the free device memory)
void rdm_paths(State* s, int npaths, const int32_t* path_len, const int32_t* path_verts, double* out_rho, size_t budget, int* nbatches) {
    if (nbatches) *nbatches = 0;
    if (npaths < 0 || (npaths > 0 && (!path_len || !path_verts))) throw Err(TNQS_ERR_INVALID, "rdm_paths: bad arguments");
    if (npaths == 0) return;
    if (!out_rho) throw Err(TNQS_ERR_INVALID, "rdm_paths: null output");
    std::vector<size_t> first(npaths + 1, 0);
    for (int q = 0; q < npaths; ++q) {
        if (path_len[q] < 2) throw Err(TNQS_ERR_INVALID, "rdm_paths: a path has at least 2 vertices");
        first[q + 1] = first[q] + (size_t)path_len[q];
    }
    for (int q = 0; q < npaths; ++q) check_path(s, path_verts + first[q], path_len[q]);
    if (s->sharded()) throw Err(TNQS_ERR_UNSUPPORTED, "rdm_paths: sharded handles are not supported");
    std::vector<PathPlan> plans; std::vector<int> verts; size_t elems = 0;
    for (int q = 0; q < npaths; ++q) {
        const int32_t* pv = path_verts + first[q];
        plans.push_back(describe_path(s, pv, path_len[q], elems));
        for (int k = 0; k < path_len[q]; ++k) {
            if (k) { const size_t dd = (size_t)s->d[pv[0]] * s->d[pv[k]]; elems += dd * dd; }
            if (std::find(verts.begin(), verts.end(), pv[k]) == verts.end()) verts.push_back(pv[k]);
        }
    }
    HIPCHK(hipSetDevice(s->device));
    materialize_pending(s, verts);
    if (!budget) {
        size_t free_b = 0, total_b = 0;
        HIPCHK(hipMemGetInfo(&free_b, &total_b));
        budget = std::min<size_t>(size_t(2) << 30, free_b / 4);
    }
    Buf d_out = dalloc(s, elems * 16);
    for (size_t q = 0; q < plans.size();) {
        // paths in order while the batch's workspace -- the paths' own and the Gram partials of its ends' launches -- stays under the bound; one that needs more runs alone
        std::vector<PathPlan> batch; size_t bytes = 0, nends = 0, unit = 0;
        while (q < plans.size()) {
            const PathPlan& p = plans[q];
            const size_t b = bytes + p.ws_bytes, n = nends + (size_t)p.len, u = std::max(unit, p.part_unit);
            if (!batch.empty() && b + std::max(n, kGramChunkFloor) * u > budget) break;
            bytes = b; nends = n; unit = u; batch.push_back(p); ++q;
        }
        if (nbatches) ++*nbatches;
        if (s->dtype == TNQS_C64) rdm_paths_batch<float>(s, batch, d_out); else rdm_paths_batch<double>(s, batch, d_out);
    }
    HIPCHK(hipMemcpyAsync(out_rho, d_out->p, elems * 16, hipMemcpyDeviceToHost, s->stream));
    sync(s);
}

}  // namespace tnqs
