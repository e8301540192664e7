// engine_rdm.cpp -- two-site reduced density matrices of bonds in one call (tnqs_rdm_edges; the reference's reduced_density_matrix(cache, [u, v]; alg = "bp")
// for adjacent u, v: the Steiner tree is the bond itself).  For a bond (u, v) of dimension chi:
//   E_u[(s, a), (s', a')] = sum_rest (psi_u x_{k != v} m_{k -> u})[s, a, rest] conj(psi_u[s', a', rest])          (d_u chi) x (d_u chi)
//   rho_uv[s_u, s_v ; s_u', s_v'] = sum_{a, a'} E_u[(s_u, a), (s_u', a')] E_v[(s_v, a), (s_v', a')]
// E_u is the Gram of the gate path -- site index and one leg kept -- with the chain result on the ket side: one Chain and one GramJob per END (u -> v) of every
// distinct requested bond, all ends of a batch in one launch per stage.  The Gram partials of both ends go straight to edge_rdm_kernel (kernels_rdm.hip), which
// sums the chunks and contracts the bond.  Ends are batched under a workspace bound; the call ends with ONE read-back.
// No partial product is shared between the z chains of a vertex (each end absorbs its z - 1 messages on its own).
#include "engine_internal.hpp"

namespace tnqs {

using EdgeEnd = EnvEnd;

// the Gram route class of a ComplexF32 end: 1 / 2 = f32 accumulation on the matrix cores up to 32 x 32 / 64 x 64 (run_grams<float, float>, the BP message Gram's
// arithmetic), 0 = f64 accumulation on the generic kernel (run_grams<float, double>)
int env_f32_class(int KK) { return (use_mfma() && KK >= 8 && KK <= 32) ? 1 : (use_mfma() && use_chi64() && KK > 32 && KK <= 64) ? 2 : 0; }

// The environments E of ends [e0, e1) (shared with engine_paths.cpp): 1. the end's site tensor with the messages of every leg but its own absorbed on the ket side,
// 2. E = the Gram that keeps the site index and that leg, one launch per route class (EnvEnd::cls).  Leaves partial / nchunks; booked under TNQS_PROF_SMALL.
template <class T> void run_env_ends(State* s, std::vector<EnvEnd>& ends, size_t e0, size_t e1) {
    const Graph& g = *s->g;
    constexpr bool f32 = std::is_same<T, float>::value;
    std::vector<Chain> chains(e1 - e0);
    for (size_t i = e0; i < e1; ++i) {
        const EnvEnd& x = ends[i];
        Chain& c = chains[i - e0]; c.v = x.u; c.src = s->site[x.u]->p; c.sd = x.sd;
        for (int j = 0; j < x.sd.z; ++j) { if (j == x.leg) continue; const int de = g.dedge(g.nbr[x.u][j], x.u); if (s->msg[de]) c.steps.push_back({j, s->msg[de]->p}); }
    }
    run_chains<T>(s, chains, TNQS_PROF_SMALL);
    std::vector<GramJob> jobs[3];
    std::vector<size_t> who[3];
    for (size_t i = e0; i < e1; ++i) {
        GramJob j{}; j.X = chains[i - e0].result; j.Y = chains[i - e0].src; j.sd = ends[i].sd; j.leg = ends[i].leg; j.keep_site = true;
        jobs[ends[i].cls].push_back(j); who[ends[i].cls].push_back(i);
    }
    for (int cls = 0; cls < 3; ++cls) {
        if (jobs[cls].empty()) continue;
        if constexpr (f32) { if (cls) run_grams<float, float>(s, jobs[cls], TNQS_PROF_SMALL); else run_grams<float, double>(s, jobs[cls], TNQS_PROF_SMALL); }
        else run_grams<double, double>(s, jobs[cls], TNQS_PROF_SMALL);
        for (size_t q = 0; q < jobs[cls].size(); ++q) { EnvEnd& x = ends[who[cls][q]]; x.partial = jobs[cls][q].partial; x.nchunks = jobs[cls][q].nchunks; }
    }
}
template void run_env_ends<float>(State*, std::vector<EnvEnd>&, size_t, size_t);
template void run_env_ends<double>(State*, std::vector<EnvEnd>&, size_t, size_t);

template <class T> static void rdm_edges_t(State* s, const std::vector<int>& bonds /* distinct edge ids */, const std::vector<size_t>& off /* of bond k in d_out, complex numbers */,
                                           Buf d_out, size_t budget, int* nbatches) {
    const Graph& g = *s->g;
    const size_t esz = s->esz();
    constexpr bool f32 = std::is_same<T, float>::value;
    // ends 2 k, 2 k + 1: the source and the destination end of bond k
    std::vector<EdgeEnd> ends(2 * bonds.size());
    std::vector<char> acc32(bonds.size(), 0);          // both ends of the bond take the f32 matrix-core Gram: its partials are float (a bond's two ends share one partial type)
    for (size_t k = 0; k < bonds.size(); ++k) {
        const int e = bonds[k], uv[2] = {g.esrc[e], g.edst[e]};
        for (int q = 0; q < 2; ++q) {
            EdgeEnd& x = ends[2 * k + q];
            x.u = uv[q]; x.leg = g.leg(uv[q], uv[1 - q]); x.sd = site_dims(s, x.u); x.KK = x.sd.d * s->chi[e];
            x.ws_bytes = 2 * x.sd.n * esz;               // the two chain temporaries
            if (!s->site[x.u]) throw Err(TNQS_ERR_INVALID, "rdm_edges: vertex not owned by this rank");
        }
        if (edge_rdm_block(s->d[uv[0]], s->d[uv[1]], s->chi[e]) < 1) throw Err(TNQS_ERR_UNSUPPORTED, "rdm_edges: bond too large for the edge kernel ((d_u^2 + d_v^2) chi must stay below 4096)");
        acc32[k] = f32 && env_f32_class(ends[2 * k].KK) && env_f32_class(ends[2 * k + 1].KK);
        for (int q = 0; q < 2; ++q) ends[2 * k + q].cls = acc32[k] ? env_f32_class(ends[2 * k + q].KK) : 0;
    }
    size_t launched = 0;                                 // bonds [0, launched) have been handed to the edge kernel
    for (size_t e0 = 0; e0 < ends.size();) {
        size_t e1 = e0, bytes = 0;
        while (e1 < ends.size() && (e1 == e0 || bytes + ends[e1].ws_bytes <= budget)) bytes += ends[e1++].ws_bytes;
        if (nbatches) ++*nbatches;
        // 1. + 2. the environments of the batch's ends
        run_env_ends<T>(s, ends, e0, e1);
        // 3. every bond whose two ends are done: the chunks of both ends summed and the bond contracted, straight into the call's output
        std::vector<EdgeRdmItem> items[2]; double pbytes = 0, flops = 0;
        const size_t ready = e1 / 2;
        for (size_t k = launched; k < ready; ++k) {
            const EdgeEnd& a = ends[2 * k]; const EdgeEnd& b = ends[2 * k + 1];
            const int chi = s->chi[bonds[k]], du = a.sd.d, dv = b.sd.d;
            items[acc32[k] ? 0 : 1].push_back(EdgeRdmItem{a.partial->p, b.partial->p, a.nchunks, b.nchunks, du, dv, chi,
                                                          s->sscale[a.u] ? reinterpret_cast<const double*>(s->sscale[a.u]->p) : nullptr,
                                                          s->sscale[b.u] ? reinterpret_cast<const double*>(s->sscale[b.u]->p) : nullptr,
                                                          reinterpret_cast<char*>(d_out->p) + off[k] * 16});
            pbytes += ((double)a.nchunks * a.KK * a.KK + (double)b.nchunks * b.KK * b.KK) * (acc32[k] ? 8.0 : 16.0) + 16.0 * du * du * dv * dv;
            flops += 8.0 * chi * chi * du * du * dv * dv;
        }
        if (ready > launched) {
            const EdgeRdmItem* d0 = upload(s, items[0]); const EdgeRdmItem* d1 = upload(s, items[1]);
            ProfScope ps(s, TNQS_PROF_EDGE_RDM, pbytes, flops);
            launch_edge_rdm<float>(s->stream, d0, (int)items[0].size());
            launch_edge_rdm<double>(s->stream, d1, (int)items[1].size());
            for (size_t k = launched; k < ready; ++k) { ends[2 * k].partial.reset(); ends[2 * k + 1].partial.reset(); }     // stream-ordered reuse by the next batch
            launched = ready;
        }
        e0 = e1;
    }
}

// out_rho: the requests' (d_u d_v)^2 complex128 matrices one after the other; budget == 0: min(2 GiB, a quarter of the free device memory), as loop_weights
void rdm_edges(State* s, int n_edges, const int32_t* eu, const int32_t* ev, double* out_rho, size_t budget, int* nbatches) {
    const Graph& g = *s->g;
    if (nbatches) *nbatches = 0;
    if (n_edges < 0) throw Err(TNQS_ERR_INVALID, "rdm_edges: negative count");
    if (s->sharded()) throw Err(TNQS_ERR_UNSUPPORTED, "rdm_edges: sharded handles are not supported");
    // requests: (edge, listed from the destination end); null lists: every edge as (src, dst)
    std::vector<std::pair<int, bool>> req;
    if (!eu || !ev) for (int e = 0; e < g.ne; ++e) req.push_back({e, false});
    else for (int i = 0; i < n_edges; ++i) {
        if (eu[i] < 0 || eu[i] >= g.nv || ev[i] < 0 || ev[i] >= g.nv) throw Err(TNQS_ERR_INVALID, "rdm_edges: bad vertex");
        const int e = g.edge(eu[i], ev[i]);
        if (e < 0) throw Err(TNQS_ERR_INVALID, "rdm_edges: not an edge");
        req.push_back({e, eu[i] != g.esrc[e]});
    }
    if (req.empty()) return;
    if (!out_rho) throw Err(TNQS_ERR_INVALID, "rdm_edges: null output");
    HIPCHK(hipSetDevice(s->device));
    std::vector<int> bonds, slot(g.ne, -1), verts; std::vector<size_t> off; size_t elems = 0;
    for (auto& r : req) {
        if (slot[r.first] >= 0) continue;
        const int e = r.first;
        slot[e] = (int)bonds.size(); bonds.push_back(e); off.push_back(elems);
        const size_t dd = (size_t)s->d[g.esrc[e]] * s->d[g.edst[e]]; elems += dd * dd;
        for (int v : {g.esrc[e], g.edst[e]}) if (std::find(verts.begin(), verts.end(), v) == verts.end()) verts.push_back(v);
    }
    materialize_pending(s, verts);
    if (!budget) {
        size_t free_b = 0, total_b = 0;
        HIPCHK(hipMemGetInfo(&free_b, &total_b));
        budget = std::min<size_t>(size_t(2) << 30, free_b / 4);
    }
    Buf d_out = dalloc(s, elems * 16);
    if (s->dtype == TNQS_C64) rdm_edges_t<float>(s, bonds, off, d_out, budget, nbatches); else rdm_edges_t<double>(s, bonds, off, d_out, budget, nbatches);
    std::vector<double> rho(2 * elems);
    HIPCHK(hipMemcpyAsync(rho.data(), d_out->p, elems * 16, hipMemcpyDeviceToHost, s->stream));
    sync(s);
    // a request listed as (dst, src) gets the index-swapped matrix: rho_(v,u)[s_v, s_u ; s_v', s_u'] = rho_(u,v)[s_u, s_v ; s_u', s_v']
    double* o = out_rho;
    for (auto& r : req) {
        const int e = r.first, da = s->d[g.esrc[e]], db = s->d[g.edst[e]], dd = da * db;
        const double* m = rho.data() + 2 * off[slot[e]];
        if (!r.second) std::memcpy(o, m, sizeof(double) * 2 * (size_t)dd * dd);
        else for (int sa = 0; sa < da; ++sa) for (int sb = 0; sb < db; ++sb) for (int ta = 0; ta < da; ++ta) for (int tb = 0; tb < db; ++tb) {
            const size_t from = (size_t)(sb + db * sa) + (size_t)dd * (tb + db * ta), to = (size_t)(sa + da * sb) + (size_t)dd * (ta + da * tb);
            o[2 * to] = m[2 * from]; o[2 * to + 1] = m[2 * from + 1];
        }
        o += 2 * (size_t)dd * dd;
    }
}

}  // namespace tnqs
