// engine_loops.cpp -- loop corrections to the BP norm (src/MessagePassing/loopcorrection.jl:79-89 `weight`, specialised to a simple cycle).
// For a cycle v_0 .. v_{L-1} of a RESCALED cache (every vertex and edge scalar 1):
//   T_k[(b,b'),(a,a')] = sum psi_k[a,b,s,r] conj(psi_k[a',b',s,r']) prod_j m_{n_j -> v_k}[r_j, r'_j]      a: bond from v_{k-1}, b: bond to v_{k+1}
//   A_k = I - vec(m_{v_k -> v_{k+1}}) vec(m_{v_{k+1} -> v_k})^T                                            (bilinear, the antiprojector of the bond)
//   W = Tr prod_k (A_k T_k)
// Every T_k is built once as a (chi_b^2) x (chi_a^2) matrix -- a Gram that keeps two legs, written by the batched GEMM straight in this layout --
// and the ring is multiplied round: L - 2 products and the trace of the last pair.  Cycles are batched under a workspace budget; a batch issues
// one launch per stage over all its cycles (items of different shapes) and ends with ONE read-back.
#include "engine_internal.hpp"

namespace tnqs {

namespace {
using LoopVertex = TransferVertex;
struct LoopCycle { std::vector<LoopVertex> lv; std::vector<Buf> prod; size_t ws_bytes = 0; };

LoopCycle describe_cycle(const State* s, const int32_t* cv, int L) {
    const Graph& g = *s->g;
    LoopCycle c; c.lv.resize(L);
    size_t pmax = 0, elems = 0;
    for (int k = 0; k < L; ++k) {
        LoopVertex& x = c.lv[k];
        x.v = cv[k]; x.ja = g.leg(x.v, cv[(k + L - 1) % L]); x.jb = g.leg(x.v, cv[(k + 1) % L]); x.sd = site_dims(s, x.v);
        if (x.sd.z + 1 > 8) throw Err(TNQS_ERR_UNSUPPORTED, "loop_weights: vertex degree > 7");
        x.ca = x.sd.chi[x.ja]; x.cb = x.sd.chi[x.jb];
        const size_t t = (size_t)x.ca * x.ca * x.cb * x.cb;
        if (t > (size_t)INT_MAX / 4) throw Err(TNQS_ERR_UNSUPPORTED, "loop_weights: bond dimension too large for the transfer-matrix route");
        elems += 4 * x.sd.n + t; pmax = std::max(pmax, t);      // two chain temporaries, two permuted copies, T_k
    }
    elems += (size_t)(L - 2) * pmax;                            // the running products (an upper bound)
    c.ws_bytes = elems * s->esz();
    return c;
}
}  // namespace

// Steps 1-3 of a transfer-matrix batch (shared with engine_paths.cpp): for every listed vertex, T[(b, b'), (a, a')] with the messages of every leg but ja, jb absorbed
// on the ket side.  One chain launch set, the permuted copies, ONE batched GEMM; all booked under TNQS_PROF_LOOP.  Pending one-site gates must have been applied.
template <class T> void build_transfer_matrices(State* s, const std::vector<TransferVertex*>& lvs, const char* who) {
    const Graph& g = *s->g;
    const size_t esz = s->esz();
    // 1. phi = psi with the messages of every leg off the cycle / path absorbed on the ket side
    std::vector<Chain> chains(lvs.size());
    for (size_t i = 0; i < lvs.size(); ++i) {
        TransferVertex& x = *lvs[i];
        if (!s->site[x.v]) throw Err(TNQS_ERR_INVALID, std::string(who) + ": vertex not owned by this rank");
        Chain& c = chains[i]; c.v = x.v; c.src = s->site[x.v]->p; c.sd = x.sd;
        for (int j = 0; j < x.sd.z; ++j) { if (j == x.ja || j == x.jb) continue; const int de = g.dedge(g.nbr[x.v][j], x.v); if (s->msg[de]) c.steps.push_back({j, s->msg[de]->p}); }
    }
    run_chains<T>(s, chains, TNQS_PROF_LOOP);
    // 2. both to [(b, a), rest]; 3. T_k = phi psi^H through the output map (b + cb b') + cb^2 (a + ca a')
    std::vector<LoopGemmItem> build; double bflops = 0, bbytes = 0;
    {
        ProfScope ps(s, TNQS_PROF_LOOP, 0, 0);
        for (size_t i = 0; i < lvs.size(); ++i) {
            TransferVertex& x = *lvs[i];
            auto permuted = [&](const void* src) {
                Buf o = dalloc(s, x.sd.n * esz);
                PermItem it{}; it.in = src; it.out = o->p; it.ndim = x.sd.z + 1; it.n = x.sd.n;
                int q = 0;
                it.dims_out[q] = x.cb; it.stride_in[q++] = (long long)x.sd.pre(x.jb);
                it.dims_out[q] = x.ca; it.stride_in[q++] = (long long)x.sd.pre(x.ja);
                it.dims_out[q] = x.sd.d; it.stride_in[q++] = 1;
                for (int j = 0; j < x.sd.z; ++j) if (j != x.ja && j != x.jb) { it.dims_out[q] = x.sd.chi[j]; it.stride_in[q++] = (long long)x.sd.pre(j); }
                launch_permute<T>(s->stream, it);
                return o;
            };
            x.psi = permuted(chains[i].src);
            x.phi = chains[i].result == chains[i].src ? x.psi : permuted(chains[i].result);
            const int mn = x.ca * x.cb, kk = (int)(x.sd.n / (size_t)mn);
            x.T = dalloc(s, (size_t)mn * mn * esz);
            LoopGemmItem it{}; it.A = x.phi->p; it.B = x.psi->p; it.C = x.T->p; it.m = mn; it.n = mn; it.k = kk; it.opB = 1;
            it.I0 = x.cb; it.si0 = 1; it.si1 = (long long)x.cb * x.cb; it.J0 = x.cb; it.sj0 = x.cb; it.sj1 = (long long)x.cb * x.cb * x.ca;
            build.push_back(it); bflops += 8.0 * mn * mn * kk; bbytes += (2.0 * mn * kk + (double)mn * mn) * esz;
        }
    }
    chains.clear();
    {
        const int tiles = plan_loop_cgemm(build.data(), (int)build.size());
        const LoopGemmItem* d = upload(s, build);
        ProfScope ps(s, TNQS_PROF_LOOP, bbytes, bflops);
        launch_loop_cgemm<T>(s->stream, d, (int)build.size(), tiles);
    }
}
template void build_transfer_matrices<float>(State*, const std::vector<TransferVertex*>&, const char*);
template void build_transfer_matrices<double>(State*, const std::vector<TransferVertex*>&, const char*);

template <class T> static void loop_batch(State* s, std::vector<LoopCycle>& cyc, double* out /* 2 doubles per cycle */) {
    const Graph& g = *s->g;
    const size_t esz = s->esz();
    std::vector<LoopVertex*> lvs; std::vector<int> verts;
    for (auto& c : cyc) for (auto& x : c.lv) { lvs.push_back(&x); if (std::find(verts.begin(), verts.end(), x.v) == verts.end()) verts.push_back(x.v); }
    materialize_pending(s, verts);
    // 1-3. T_k of every vertex of every cycle
    build_transfer_matrices<T>(s, lvs, "loop_weights");
    // 4. A_k T_k in place: f = m_{v_k -> v_{k+1}}, b = m_{v_{k+1} -> v_k} (unset message = identity)
    {
        std::unordered_map<int, Buf> ident;
        auto msg_of = [&](int src, int dst, int chi) -> const void* {
            const int de = g.dedge(src, dst);
            if (s->msg[de]) return s->msg[de]->p;
            Buf& b = ident[chi];
            if (!b) { b = dalloc(s, (size_t)chi * chi * esz); launch_identity<T>(s->stream, b->p, chi); s->keepalive.push_back(b); }
            return b->p;
        };
        std::vector<LoopProjItem> pj; double bytes = 0;
        for (auto& c : cyc) { const int L = (int)c.lv.size();
            for (int k = 0; k < L; ++k) { LoopVertex& x = c.lv[k]; const int nx = c.lv[(k + 1) % L].v;
                pj.push_back(LoopProjItem{x.T->p, msg_of(x.v, nx, x.cb), msg_of(nx, x.v, x.cb), x.cb * x.cb, x.ca * x.ca, 0}); bytes += 3.0 * x.cb * x.cb * x.ca * x.ca * esz; } }
        const int wgs = plan_loop_antiproject(pj.data(), (int)pj.size());
        const LoopProjItem* d = upload(s, pj);
        ProfScope ps(s, TNQS_PROF_LOOP, bytes, 0);
        launch_loop_antiproject<T>(s->stream, d, (int)pj.size(), wgs);
    }
    // 5. P_t = (A_t T_t) P_{t-1}, P_0 = A_0 T_0, t = 1 .. L - 2: step t of every cycle that has one in one launch
    size_t maxL = 0; for (auto& c : cyc) maxL = std::max(maxL, c.lv.size());
    std::vector<const void*> P(cyc.size());
    for (size_t q = 0; q < cyc.size(); ++q) P[q] = cyc[q].lv[0].T->p;
    for (int t = 1; t + 2 <= (int)maxL; ++t) {
        std::vector<LoopGemmItem> items; double flops = 0, bytes = 0;
        for (size_t q = 0; q < cyc.size(); ++q) {
            LoopCycle& c = cyc[q];
            if (t > (int)c.lv.size() - 2) continue;
            LoopVertex& x = c.lv[t];
            const int m = x.cb * x.cb, k = x.ca * x.ca, n = c.lv[0].ca * c.lv[0].ca;
            Buf o = dalloc(s, (size_t)m * n * esz); c.prod.push_back(o);
            LoopGemmItem it{}; it.A = x.T->p; it.B = P[q]; it.C = o->p; it.m = m; it.n = n; it.k = k; it.opB = 0;
            it.I0 = m; it.si0 = 1; it.si1 = 0; it.J0 = n; it.sj0 = m; it.sj1 = 0;
            items.push_back(it); P[q] = o->p; flops += 8.0 * m * n * k; bytes += ((double)m * k + (double)k * n + (double)m * n) * esz;
        }
        const int tiles = plan_loop_cgemm(items.data(), (int)items.size());
        const LoopGemmItem* d = upload(s, items);
        ProfScope ps(s, TNQS_PROF_LOOP, bytes, flops);
        launch_loop_cgemm<T>(s->stream, d, (int)items.size(), tiles);
    }
    // 6. W = sum_ij (A_{L-1} T_{L-1})[i,j] P_{L-2}[j,i]
    Buf d_part = dalloc(s, cyc.size() * 128 * sizeof(double)), d_out = dalloc(s, cyc.size() * 2 * sizeof(double));
    {
        std::vector<LoopTraceItem> tr; double bytes = 0;
        for (size_t q = 0; q < cyc.size(); ++q) {
            LoopVertex& x = cyc[q].lv.back();
            tr.push_back(LoopTraceItem{x.T->p, P[q], x.cb * x.cb, x.ca * x.ca, reinterpret_cast<double*>(d_part->p) + 128 * q, reinterpret_cast<double*>(d_out->p) + 2 * q, 0, 0});
            bytes += 2.0 * x.cb * x.cb * x.ca * x.ca * esz;
        }
        const int wgs = plan_loop_trace(tr.data(), (int)tr.size());
        const LoopTraceItem* d = upload(s, tr);
        ProfScope ps(s, TNQS_PROF_LOOP, bytes, 0);
        launch_loop_trace<T>(s->stream, d, (int)tr.size(), wgs);
    }
    // 7. one read-back; a pending real scale of a site tensor enters T_k squared (as in rdm_batch)
    HIPCHK(hipMemcpyAsync(out, d_out->p, cyc.size() * 2 * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    std::vector<double> fac(verts.size(), 1.0);
    for (size_t i = 0; i < verts.size(); ++i) if (s->sscale[verts[i]]) HIPCHK(hipMemcpyAsync(&fac[i], s->sscale[verts[i]]->p, 8, hipMemcpyDeviceToHost, s->stream));
    sync(s);
    for (size_t q = 0; q < cyc.size(); ++q) {
        double f = 1.0;
        for (auto& x : cyc[q].lv) { const double a = fac[std::find(verts.begin(), verts.end(), x.v) - verts.begin()]; f *= a * a; }
        out[2 * q] *= f; out[2 * q + 1] *= f;
    }
}

void loop_weights(State* s, int ncycles, const int32_t* cycle_len, const int32_t* cycle_verts, double* out_re_im) {
    const Graph& g = *s->g;
    if (ncycles < 0 || (ncycles > 0 && (!cycle_len || !cycle_verts || !out_re_im))) throw Err(TNQS_ERR_INVALID, "loop_weights: bad arguments");
    if (s->sharded()) throw Err(TNQS_ERR_UNSUPPORTED, "loop_weights: sharded handles are not supported");
    std::vector<size_t> off(ncycles + 1, 0);
    for (int c = 0; c < ncycles; ++c) {
        const int L = cycle_len[c];
        if (L < 3) throw Err(TNQS_ERR_INVALID, "loop_weights: a cycle has at least 3 vertices");
        off[c + 1] = off[c] + (size_t)L;
        const int32_t* cv = cycle_verts + off[c];
        for (int k = 0; k < L; ++k) {
            if (cv[k] < 0 || cv[k] >= g.nv) throw Err(TNQS_ERR_INVALID, "loop_weights: bad vertex");
            for (int q = 0; q < k; ++q) if (cv[q] == cv[k]) throw Err(TNQS_ERR_INVALID, "loop_weights: repeated vertex in a cycle");
        }
        for (int k = 0; k < L; ++k) if (g.edge(cv[k], cv[(k + 1) % L]) < 0) throw Err(TNQS_ERR_INVALID, "loop_weights: consecutive vertices of a cycle must be neighbours");
    }
    if (ncycles == 0) return;
    HIPCHK(hipSetDevice(s->device));
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const size_t budget = std::min<size_t>(size_t(2) << 30, free_b / 4);
    for (int c = 0; c < ncycles;) {
        std::vector<LoopCycle> batch; size_t bytes = 0; const int c0 = c;
        while (c < ncycles) {
            LoopCycle lc = describe_cycle(s, cycle_verts + off[c], cycle_len[c]);
            if (!batch.empty() && bytes + lc.ws_bytes > budget) break;
            bytes += lc.ws_bytes; batch.push_back(std::move(lc)); ++c;
        }
        if (s->dtype == TNQS_C64) loop_batch<float>(s, batch, out_re_im + 2 * (size_t)c0); else loop_batch<double>(s, batch, out_re_im + 2 * (size_t)c0);
    }
}

}  // namespace tnqs
