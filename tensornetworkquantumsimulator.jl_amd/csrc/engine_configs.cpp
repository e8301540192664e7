// engine_configs.cpp -- loop corrections beyond simple cycles (src/MessagePassing/loopcorrection.jl:79-89 `weight`): connected leafless configurations with TWO
// independent loops, on the device.  Such a configuration has two branch vertices of internal degree 3 (theta: three chains between them; dumbbell: a closed chain
// on each and a bridge) or one of internal degree 4 (figure-eight: two closed chains).  A chain p_0 (branch), p_1 .. p_n, p_{n+1} (branch) carries
//   P = (A_n T_n) ... (A_1 T_1), chi_far^2 x chi_near^2, the transfer matrices and antiprojectors of engine_loops.cpp for the open chain,
// and the antiprojector A_0 of its first edge, which acts on the branch tensor's leg (a chain of one edge is A_0 alone).  For a closed chain (both ends on one
// vertex) L^T = (P A_0)^T = P^T - b_0 (f_0^T P^T) is formed once.
//   theta         B_u[(x0),(x1),(x2)] (loop_branch_gram_kernel) -> every leg through its chain: A_0 on the leading leg in place, then P as a GEMM whose output map
//                 moves the new leg to the back -> full contraction with B_w, written by the Gram kernel in the layout the legs ended up in (B_w IS materialised)
//   dumbbell      g_s[y] = sum L_s^T[x1,x2] B_s[x1,x2,y] (a GEMM with one row) on both sides, the bridge applied to g_u, W = g_w . (P A_0 g_u)
//   figure-eight  X = M phi with M[(a',b'),(a,b)] = L_0[(b,b'),(a,a')], Y = X psi^H over (a', b', site, outside legs), W = Y . L_1^T: the chi^8 tensor is never formed
// Simple cycles go to loop_weights in the ring order the decomposition fixes.  One launch per stage over the configurations of a batch -- the permutes excepted: one launch per permuted operand, as in build_transfer_matrices --, one read-back per batch.
#include "engine_internal.hpp"
#include <map>

namespace tnqs {

namespace {
enum CfgShape { kCycle = 0, kTheta = 1, kDumbbell = 2, kEight = 3 };

struct CfgChain {
    std::vector<int> path;                        // p_0, p_1 .. p_n, p_{n+1}
    int cn = 0, cf = 0;                           // bond dimensions of the first and the last edge
    std::vector<TransferVertex> tv;               // the inner vertices
    std::vector<Buf> prod; const void* P = nullptr;
    Buf Lt;                                       // closed chains: L^T, cn^2 x cf^2
    int n() const { return (int)path.size() - 2; }
    bool closed() const { return path.front() == path.back(); }
};
struct CfgBranch { int v = -1; SD sd; int nslots = 0; int nbv[4]; int leg[4]; int c[4]; int K = 1; Buf phi, psi, psi2; };
struct Config {
    int shape = kCycle; std::vector<int> ring; std::vector<CfgBranch> br; std::vector<CfgChain> ch; std::vector<int> verts;
    size_t ws_bytes = 0; int slot = 0;            // slot: position in the caller's list
    // device state of the batch
    Buf cur, Bw, gw, M, X; int lay[3]; long long dq[3];      // cur: the tensor / vector the rounds carry; lay: its legs (chains) in memory order, dq: their dimensions
};

// ---- decomposition (host only) -------------------------------------------------------------------------------------------------------------------------------
Config decompose(const Graph& g, int ne, const int32_t* eu, const int32_t* ev) {
    if (ne < 1) throw Err(TNQS_ERR_INVALID, "config_weights: a configuration has at least one edge");
    std::vector<std::pair<int, int>> es(ne);
    for (int i = 0; i < ne; ++i) {
        const int a = eu[i], b = ev[i];
        if (a < 0 || b < 0 || a >= g.nv || b >= g.nv || a == b || g.edge(a, b) < 0) throw Err(TNQS_ERR_INVALID, "config_weights: an edge of a configuration is not in the graph");
        es[i] = {std::min(a, b), std::max(a, b)};
    }
    std::sort(es.begin(), es.end());              // canonical: orientation and order of the caller's list do not matter from here on
    if (std::adjacent_find(es.begin(), es.end()) != es.end()) throw Err(TNQS_ERR_INVALID, "config_weights: repeated edge in a configuration");
    std::map<int, std::vector<int>> nb;           // internal neighbours, ascending
    for (auto& e : es) { nb[e.first].push_back(e.second); nb[e.second].push_back(e.first); }
    for (auto& kv : nb) std::sort(kv.second.begin(), kv.second.end());
    {   // connected
        std::set<int> seen{nb.begin()->first}; std::vector<int> todo{nb.begin()->first};
        while (!todo.empty()) { const int v = todo.back(); todo.pop_back(); for (int w : nb[v]) if (seen.insert(w).second) todo.push_back(w); }
        if (seen.size() != nb.size()) throw Err(TNQS_ERR_INVALID, "config_weights: a configuration must be connected");
    }
    for (auto& kv : nb) if (kv.second.size() < 2) throw Err(TNQS_ERR_INVALID, "config_weights: a configuration has a vertex of internal degree 1");
    const int loops = ne - (int)nb.size() + 1;
    if (loops > 2) throw Err(TNQS_ERR_UNSUPPORTED, "config_weights: configurations with more than two independent loops are not supported (" + std::to_string(loops) + ")");
    Config c;
    for (auto& kv : nb) { c.verts.push_back(kv.first); if ((int)g.nbr[kv.first].size() + 1 > 8) throw Err(TNQS_ERR_UNSUPPORTED, "config_weights: vertex degree > 7"); }
    if (loops == 1) {                             // a simple cycle: from the lowest vertex towards its lower ring neighbour
        c.shape = kCycle;
        int prev = c.verts[0], cur = nb[prev][0];
        c.ring.push_back(prev);
        while (cur != c.verts[0]) { c.ring.push_back(cur); const int nx = nb[cur][0] != prev ? nb[cur][0] : nb[cur][1]; prev = cur; cur = nx; }
        return c;
    }
    std::set<std::pair<int, int>> used;
    for (auto& kv : nb) {
        if (kv.second.size() < 3) continue;
        for (int w : kv.second) {
            if (used.count({std::min(kv.first, w), std::max(kv.first, w)})) continue;
            CfgChain ch; ch.path = {kv.first, w};
            used.insert({std::min(kv.first, w), std::max(kv.first, w)});
            while (nb[ch.path.back()].size() == 2) {
                const int cur = ch.path.back(), prev = ch.path[ch.path.size() - 2];
                const int nx = nb[cur][0] != prev ? nb[cur][0] : nb[cur][1];
                used.insert({std::min(cur, nx), std::max(cur, nx)}); ch.path.push_back(nx);
            }
            c.ch.push_back(std::move(ch));
        }
    }
    // order the chains by role: theta u -> w three times; dumbbell closed(u), closed(w), bridge; figure-eight closed, closed
    std::vector<int> branch; for (auto& kv : nb) if (kv.second.size() >= 3) branch.push_back(kv.first);
    auto slot = [&](CfgBranch& b, int nbv) { b.nbv[b.nslots++] = nbv; };
    if (branch.size() == 1) {
        c.shape = kEight; c.br.resize(1); c.br[0].v = branch[0];
        for (auto& ch : c.ch) { slot(c.br[0], ch.path[1]); slot(c.br[0], ch.path[ch.path.size() - 2]); }
    } else {
        c.br.resize(2); c.br[0].v = branch[0]; c.br[1].v = branch[1];
        if (!c.ch[0].closed() && !c.ch[1].closed() && !c.ch[2].closed()) {
            c.shape = kTheta;
            for (auto& ch : c.ch) { slot(c.br[0], ch.path[1]); slot(c.br[1], ch.path[ch.path.size() - 2]); }
        } else {
            c.shape = kDumbbell;
            std::stable_sort(c.ch.begin(), c.ch.end(), [&](const CfgChain& a, const CfgChain& b) {
                auto rank = [&](const CfgChain& x) { return !x.closed() ? 2 : (x.path[0] == branch[0] ? 0 : 1); };
                return rank(a) < rank(b); });
            for (int q = 0; q < 2; ++q) { slot(c.br[q], c.ch[q].path[1]); slot(c.br[q], c.ch[q].path[c.ch[q].path.size() - 2]); }
            slot(c.br[0], c.ch[2].path[1]); slot(c.br[1], c.ch[2].path[c.ch[2].path.size() - 2]);
        }
    }
    return c;
}

// bond dimensions, legs and the workspace need of a configuration (host only; nothing is allocated)
void describe(const State* s, Config& c) {
    const Graph& g = *s->g;
    if (c.shape == kCycle) return;
    size_t elems = 0;
    const size_t lim = (size_t)INT_MAX / 4;
    for (auto& b : c.br) {
        b.sd = site_dims(s, b.v); size_t in = 1;
        for (int q = 0; q < b.nslots; ++q) { b.leg[q] = g.leg(b.v, b.nbv[q]); b.c[q] = b.sd.chi[b.leg[q]]; in *= (size_t)b.c[q]; }
        b.K = (int)(b.sd.n / in);
        elems += 5 * b.sd.n;
    }
    for (auto& ch : c.ch) {
        const int n = ch.n(); ch.tv.resize(n); size_t pmax = 0;
        ch.cn = s->chi[g.edge(ch.path[0], ch.path[1])]; ch.cf = s->chi[g.edge(ch.path[n], ch.path[n + 1])];
        for (int k = 1; k <= n; ++k) {
            TransferVertex& x = ch.tv[k - 1];
            x.v = ch.path[k]; x.ja = g.leg(x.v, ch.path[k - 1]); x.jb = g.leg(x.v, ch.path[k + 1]); x.sd = site_dims(s, x.v);
            x.ca = x.sd.chi[x.ja]; x.cb = x.sd.chi[x.jb];
            const size_t t = (size_t)x.ca * x.ca * x.cb * x.cb;
            if (t > lim || (size_t)x.cb * x.cb * ch.cn * ch.cn > lim) throw Err(TNQS_ERR_UNSUPPORTED, "config_weights: bond dimension too large for the transfer-matrix route");
            elems += 4 * x.sd.n + t; pmax = std::max(pmax, (size_t)x.cb * x.cb * ch.cn * ch.cn);
        }
        elems += (size_t)std::max(0, n - 1) * pmax + (ch.closed() ? 2 * (size_t)ch.cn * ch.cn * ch.cf * ch.cf : 0);
    }
    auto sq = [](int x) { return (size_t)x * x; };
    if (c.shape == kTheta) {
        // the tensor the rounds carry: chains of one edge leave its size alone, the others (in this order) swap chi_near^2 for chi_far^2
        size_t cur = sq(c.ch[0].cn) * sq(c.ch[1].cn) * sq(c.ch[2].cn), bw = sq(c.ch[0].cf) * sq(c.ch[1].cf) * sq(c.ch[2].cf), peak = cur, big = cur, leg = SIZE_MAX;
        for (auto& ch : c.ch) {
            leg = std::min(leg, std::min(sq(ch.cn), sq(ch.cf)));
            if (!ch.n()) continue;
            const size_t nx = cur / sq(ch.cn) * sq(ch.cf); peak = std::max(peak, cur + nx); big = std::max(big, nx); cur = nx;
        }
        for (auto& b : c.br) if ((size_t)b.c[0] * b.c[1] * b.c[2] > lim || big / leg > lim)      // rows of the Gram; columns of a round's GEMM and antiprojector
            throw Err(TNQS_ERR_UNSUPPORTED, "config_weights: bond dimension too large for the branch route");
        elems += peak + bw;
    } else if (c.shape == kDumbbell) {
        for (auto& b : c.br) {
            if (sq(b.c[0]) * sq(b.c[1]) > lim || (size_t)b.c[0] * b.c[1] * b.c[2] > lim) throw Err(TNQS_ERR_UNSUPPORTED, "config_weights: bond dimension too large for the branch route");
            elems += sq(b.c[0]) * sq(b.c[1]) * sq(b.c[2]) + 2 * sq(b.c[2]);
        }
    } else {
        const CfgBranch& b = c.br[0];
        const size_t ab = (size_t)b.c[0] * b.c[1], ce = (size_t)b.c[2] * b.c[3];
        if (ce * b.K > lim || ab * b.K > lim) throw Err(TNQS_ERR_UNSUPPORTED, "config_weights: bond dimension too large for the branch route");
        elems += ab * ab + ab * ce * b.K + ce * ce;
    }
    c.ws_bytes = elems * s->esz() + 2 * kLoopDotMaxWgs * sizeof(double);
}

template <class T> void config_batch(State* s, std::vector<Config*>& cfg, double* out /* indexed by Config::slot */) {
    const Graph& g = *s->g;
    const size_t esz = s->esz();
    std::vector<int> verts;
    for (Config* c : cfg) for (int v : c->verts) if (std::find(verts.begin(), verts.end(), v) == verts.end()) verts.push_back(v);
    materialize_pending(s, verts);
    std::unordered_map<int, Buf> ident;
    auto msg_of = [&](int src, int dst, int chi) -> const void* {      // unset message = identity
        const int de = g.dedge(src, dst);
        if (s->msg[de]) return s->msg[de]->p;
        Buf& b = ident[chi];
        if (!b) { b = dalloc(s, (size_t)chi * chi * esz); launch_identity<T>(s->stream, b->p, chi); s->keepalive.push_back(b); }
        return b->p;
    };
    auto run_proj = [&](std::vector<LoopProjItem>& pj) {
        if (pj.empty()) return;
        double bytes = 0; for (auto& p : pj) bytes += 3.0 * p.nr * p.nc * esz;
        const int wgs = plan_loop_antiproject(pj.data(), (int)pj.size());
        const LoopProjItem* d = upload(s, pj);
        ProfScope ps(s, TNQS_PROF_LOOP, bytes, 0);
        launch_loop_antiproject<T>(s->stream, d, (int)pj.size(), wgs);
    };
    auto run_gemm = [&](std::vector<LoopGemmItem>& items) {
        if (items.empty()) return;
        double flops = 0, bytes = 0;
        for (auto& it : items) { flops += 8.0 * it.m * it.n * it.k; bytes += ((double)it.m * it.k + (double)it.k * it.n + (double)it.m * it.n) * esz; }
        const int tiles = plan_loop_cgemm(items.data(), (int)items.size());
        const LoopGemmItem* d = upload(s, items);
        ProfScope ps(s, TNQS_PROF_LOOP, bytes, flops);
        launch_loop_cgemm<T>(s->stream, d, (int)items.size(), tiles);
    };
    auto plain_gemm = [&](const void* A, const void* B, void* C, int m, int n, int k) {
        LoopGemmItem it{}; it.A = A; it.B = B; it.C = C; it.m = m; it.n = n; it.k = k; it.opB = 0; it.I0 = m; it.si0 = 1; it.si1 = 0; it.J0 = n; it.sj0 = m; it.sj1 = 0; return it;
    };

    // 1. the transfer matrices of every inner vertex of every chain, 2. A_k T_k in place
    {
        std::vector<TransferVertex*> lvs; std::vector<LoopProjItem> pj;
        for (Config* c : cfg) for (auto& ch : c->ch) for (auto& x : ch.tv) lvs.push_back(&x);
        if (!lvs.empty()) build_transfer_matrices<T>(s, lvs, "config_weights");
        for (Config* c : cfg) for (auto& ch : c->ch) for (int k = 1; k <= ch.n(); ++k) {
            TransferVertex& x = ch.tv[k - 1]; const int nx = ch.path[k + 1];
            pj.push_back(LoopProjItem{x.T->p, msg_of(x.v, nx, x.cb), msg_of(nx, x.v, x.cb), x.cb * x.cb, x.ca * x.ca, 0});
        }
        run_proj(pj);
    }
    // 3. P_t = (A_t T_t) P_{t-1}: step t of every chain that has one in one launch
    {
        int maxn = 0;
        for (Config* c : cfg) for (auto& ch : c->ch) { maxn = std::max(maxn, ch.n()); ch.P = ch.n() ? ch.tv[0].T->p : nullptr; }
        for (int t = 1; t < maxn; ++t) {
            std::vector<LoopGemmItem> items;
            for (Config* c : cfg) for (auto& ch : c->ch) {
                if (t >= ch.n()) continue;
                TransferVertex& x = ch.tv[t];
                const int m = x.cb * x.cb, k = x.ca * x.ca, n = ch.cn * ch.cn;
                Buf o = dalloc(s, (size_t)m * n * esz); ch.prod.push_back(o);
                items.push_back(plain_gemm(x.T->p, ch.P, o->p, m, n, k)); ch.P = o->p;
            }
            run_gemm(items);
        }
    }
    // 4. closed chains: L^T = P^T - b_0 (f_0^T P^T)
    {
        std::vector<LoopProjItem> pj;
        bool any = false; for (Config* c : cfg) for (auto& ch : c->ch) any = any || ch.closed();
        std::unique_ptr<ProfScope> ps; if (any) ps.reset(new ProfScope(s, TNQS_PROF_LOOP, 0, 0));      // the transposes: one permute launch per closed chain
        for (Config* c : cfg) for (auto& ch : c->ch) {
            if (!ch.closed()) continue;
            const int nn = ch.cn * ch.cn, nf = ch.cf * ch.cf;
            ch.Lt = dalloc(s, (size_t)nn * nf * esz);
            PermItem it{}; it.in = ch.P; it.out = ch.Lt->p; it.ndim = 2; it.n = (size_t)nn * nf;
            it.dims_out[0] = nn; it.stride_in[0] = nf; it.dims_out[1] = nf; it.stride_in[1] = 1;
            launch_permute<T>(s->stream, it);
            pj.push_back(LoopProjItem{ch.Lt->p, msg_of(ch.path[1], ch.path[0], ch.cn), msg_of(ch.path[0], ch.path[1], ch.cn), nn, nf, 0});
        }
        if (!pj.empty()) { const int wgs = plan_loop_antiproject(pj.data(), (int)pj.size()); const LoopProjItem* d = upload(s, pj); launch_loop_antiproject<T>(s->stream, d, (int)pj.size(), wgs); }
    }
    // 5. the branch vertices: phi (outside messages absorbed on the ket side) and psi as [slot legs .., site, outside legs ..]
    {
        std::vector<CfgBranch*> brs; for (Config* c : cfg) for (auto& b : c->br) brs.push_back(&b);
        std::vector<Chain> chains(brs.size());
        for (size_t i = 0; i < brs.size(); ++i) {
            CfgBranch& b = *brs[i];
            if (!s->site[b.v]) throw Err(TNQS_ERR_INVALID, "config_weights: vertex not owned by this rank");
            Chain& c = chains[i]; c.v = b.v; c.src = s->site[b.v]->p; c.sd = b.sd;
            for (int j = 0; j < b.sd.z; ++j) {
                if (std::find(b.leg, b.leg + b.nslots, j) != b.leg + b.nslots) continue;
                const int de = g.dedge(g.nbr[b.v][j], b.v); if (s->msg[de]) c.steps.push_back({j, s->msg[de]->p});
            }
        }
        run_chains<T>(s, chains, TNQS_PROF_LOOP);
        ProfScope ps(s, TNQS_PROF_LOOP, 0, 0);
        for (size_t i = 0; i < brs.size(); ++i) {
            CfgBranch& b = *brs[i];
            auto permuted = [&](const void* src, const int* order) {
                Buf o = dalloc(s, b.sd.n * esz);
                PermItem it{}; it.in = src; it.out = o->p; it.ndim = b.sd.z + 1; it.n = b.sd.n;
                int q = 0;
                for (int t = 0; t < b.nslots; ++t) { it.dims_out[q] = b.c[order[t]]; it.stride_in[q++] = (long long)b.sd.pre(b.leg[order[t]]); }
                it.dims_out[q] = b.sd.d; it.stride_in[q++] = 1;
                for (int j = 0; j < b.sd.z; ++j) if (std::find(b.leg, b.leg + b.nslots, j) == b.leg + b.nslots) { it.dims_out[q] = b.sd.chi[j]; it.stride_in[q++] = (long long)b.sd.pre(j); }
                launch_permute<T>(s->stream, it);
                return o;
            };
            const int id[4] = {0, 1, 2, 3}, swapped[4] = {2, 3, 0, 1};
            b.psi = permuted(chains[i].src, id);
            b.phi = chains[i].result == chains[i].src ? b.psi : permuted(chains[i].result, id);
            if (b.nslots == 4) b.psi2 = permuted(chains[i].src, swapped);
        }
    }
    // 6. the three-leg Grams of theta and dumbbell branch vertices in one launch; the figure-eight's M
    {
        std::vector<BranchGramItem> gi; double flops = 0, bytes = 0;
        std::unique_ptr<ProfScope> mscope;      // the figure-eights' M: one permute launch each
        for (Config* c : cfg) {
            if (c->shape == kTheta) {
                // chains of one edge go last: their antiprojector acts in place and does not move the leg
                int o[3], q = 0; bool all = true;
                for (int i = 0; i < 3; ++i) if (c->ch[i].n()) o[q++] = i;
                for (int i = 0; i < 3; ++i) if (!c->ch[i].n()) { o[q++] = i; all = false; }
                const int fin[3] = {all ? o[0] : o[2], all ? o[1] : o[0], all ? o[2] : o[1]};
                for (int p = 0; p < 3; ++p) { c->lay[p] = o[p]; c->dq[p] = (long long)c->ch[p].cn * c->ch[p].cn; }
                const int xu[3] = {c->br[0].c[0], c->br[0].c[1], c->br[0].c[2]}, xw[3] = {c->br[1].c[0], c->br[1].c[1], c->br[1].c[2]};
                c->cur = dalloc(s, (size_t)(c->dq[0] * c->dq[1] * c->dq[2]) * esz);
                c->Bw = dalloc(s, (size_t)xw[0] * xw[0] * xw[1] * xw[1] * xw[2] * xw[2] * esz);
                BranchGramItem a = branch_gram_item(xu, o, c->br[0].K); a.A = c->br[0].phi->p; a.B = c->br[0].psi->p; a.C = c->cur->p; gi.push_back(a);
                BranchGramItem b = branch_gram_item(xw, fin, c->br[1].K); b.A = c->br[1].phi->p; b.B = c->br[1].psi->p; b.C = c->Bw->p; gi.push_back(b);
            } else if (c->shape == kDumbbell) {
                const int id[3] = {0, 1, 2};
                for (int q = 0; q < 2; ++q) {
                    CfgBranch& b = c->br[q]; const int x[3] = {b.c[0], b.c[1], b.c[2]};
                    Buf& dst = q ? c->Bw : c->cur;
                    dst = dalloc(s, (size_t)x[0] * x[0] * x[1] * x[1] * x[2] * x[2] * esz);
                    BranchGramItem a = branch_gram_item(x, id, b.K); a.A = b.phi->p; a.B = b.psi->p; a.C = dst->p; gi.push_back(a);
                }
            } else {
                CfgBranch& b = c->br[0]; const int ca = b.c[0], cb = b.c[1];
                c->M = dalloc(s, (size_t)ca * ca * cb * cb * esz);
                PermItem it{}; it.in = c->ch[0].Lt->p; it.out = c->M->p; it.ndim = 4; it.n = (size_t)ca * ca * cb * cb;
                it.dims_out[0] = ca; it.stride_in[0] = ca; it.dims_out[1] = cb; it.stride_in[1] = (long long)ca * ca * cb;
                it.dims_out[2] = ca; it.stride_in[2] = 1; it.dims_out[3] = cb; it.stride_in[3] = (long long)ca * ca;
                if (!mscope) mscope.reset(new ProfScope(s, TNQS_PROF_LOOP, 0, 0));
                launch_permute<T>(s->stream, it);
            }
        }
        mscope.reset();
        for (auto& it : gi) { flops += 8.0 * it.m * it.n * it.k; bytes += (2.0 * it.m * it.k + (double)it.m * it.n) * esz; }
        if (!gi.empty()) {
            const int tiles = plan_loop_branch_gram(gi.data(), (int)gi.size());
            const BranchGramItem* d = upload(s, gi);
            ProfScope ps(s, TNQS_PROF_LOOP, bytes, flops);
            launch_loop_branch_gram<T>(s->stream, d, (int)gi.size(), tiles);
        }
    }
    // 7. three rounds: per round one antiprojector launch and one GEMM launch over all configurations
    for (int r = 0; r < 3; ++r) {
        std::vector<LoopProjItem> pj; std::vector<LoopGemmItem> gm;
        std::vector<std::pair<Config*, Buf>> next;
        for (Config* c : cfg) {
            if (c->shape == kTheta) {
                CfgChain& ch = c->ch[c->lay[0]];                      // the chain of the leading leg
                const long long X = c->dq[c->lay[0]], rest = c->dq[c->lay[1]] * c->dq[c->lay[2]];
                pj.push_back(LoopProjItem{c->cur->p, msg_of(ch.path[0], ch.path[1], ch.cn), msg_of(ch.path[1], ch.path[0], ch.cn), (int)X, (int)rest, 0});
                if (!ch.n()) continue;                                 // (only ever the last round: nothing left to rotate)
                const long long Y = (long long)ch.cf * ch.cf;
                Buf o = dalloc(s, (size_t)(Y * rest) * esz);
                LoopGemmItem it{}; it.A = ch.P; it.B = c->cur->p; it.C = o->p; it.m = (int)Y; it.n = (int)rest; it.k = (int)X; it.opB = 0;
                it.I0 = it.m; it.si0 = rest; it.si1 = 0; it.J0 = it.n; it.sj0 = 1; it.sj1 = 0;
                gm.push_back(it); next.push_back({c, o});
                c->dq[c->lay[0]] = Y; std::rotate(c->lay, c->lay + 1, c->lay + 3);
            } else if (c->shape == kDumbbell) {
                if (r == 0) {                                          // g_s = L_s^T . B_s on both sides
                    for (int q = 0; q < 2; ++q) {
                        CfgBranch& b = c->br[q]; const int k = b.c[0] * b.c[0] * b.c[1] * b.c[1], n = b.c[2] * b.c[2];
                        Buf o = dalloc(s, (size_t)n * esz);
                        gm.push_back(plain_gemm(c->ch[q].Lt->p, (q ? c->Bw : c->cur)->p, o->p, 1, n, k));
                        if (q) c->gw = o; else next.push_back({c, o});
                    }
                } else if (r == 1) {                                   // the bridge on g_u
                    CfgChain& ch = c->ch[2];
                    pj.push_back(LoopProjItem{c->cur->p, msg_of(ch.path[0], ch.path[1], ch.cn), msg_of(ch.path[1], ch.path[0], ch.cn), ch.cn * ch.cn, 1, 0});
                    if (ch.n()) {
                        Buf o = dalloc(s, (size_t)ch.cf * ch.cf * esz);
                        gm.push_back(plain_gemm(ch.P, c->cur->p, o->p, ch.cf * ch.cf, 1, ch.cn * ch.cn)); next.push_back({c, o});
                    }
                }
            } else {
                CfgBranch& b = c->br[0]; const int ab = b.c[0] * b.c[1], ce = b.c[2] * b.c[3];
                if (r == 0) {                                          // X[(c,e),(a',b'),rest] = M phi
                    c->X = dalloc(s, (size_t)ab * ce * b.K * esz);
                    LoopGemmItem it{}; it.A = c->M->p; it.B = b.phi->p; it.C = c->X->p; it.m = ab; it.n = ce * b.K; it.k = ab; it.opB = 0;
                    it.I0 = ab; it.si0 = ce; it.si1 = 0; it.J0 = ce; it.sj0 = 1; it.sj1 = (long long)ce * ab;
                    gm.push_back(it);
                } else if (r == 1) {                                   // Y[(c,c'),(e,e')] = X psi^H
                    c->cur = dalloc(s, (size_t)ce * ce * esz);
                    LoopGemmItem it{}; it.A = c->X->p; it.B = b.psi2->p; it.C = c->cur->p; it.m = ce; it.n = ce; it.k = ab * b.K; it.opB = 1;
                    it.I0 = b.c[2]; it.si0 = 1; it.si1 = (long long)b.c[2] * b.c[2]; it.J0 = b.c[2]; it.sj0 = b.c[2]; it.sj1 = (long long)b.c[2] * b.c[2] * b.c[3];
                    gm.push_back(it);
                }
            }
        }
        run_proj(pj);
        run_gemm(gm);
        for (auto& nx : next) nx.first->cur = nx.second;      // the round's input goes back to the pool behind the launch that read it
    }
    // 8. the full contractions in f64, one read-back; a pending real scale of a site tensor enters squared
    const size_t nc = cfg.size();
    Buf d_part = dalloc(s, nc * 2 * kLoopDotMaxWgs * sizeof(double)), d_out = dalloc(s, nc * 2 * sizeof(double));
    {
        std::vector<LoopDotItem> di; double bytes = 0;
        for (size_t q = 0; q < nc; ++q) {
            Config* c = cfg[q];
            LoopDotItem it{}; it.X = c->cur->p;
            if (c->shape == kTheta) { it.Y = c->Bw->p; it.n = c->dq[0] * c->dq[1] * c->dq[2]; }
            else if (c->shape == kDumbbell) { it.Y = c->gw->p; it.n = (long long)c->ch[2].cf * c->ch[2].cf; }
            else { it.Y = c->ch[1].Lt->p; it.n = (long long)c->ch[1].cn * c->ch[1].cn * c->ch[1].cf * c->ch[1].cf; }
            it.partial = reinterpret_cast<double*>(d_part->p) + 2 * kLoopDotMaxWgs * q; it.out = reinterpret_cast<double*>(d_out->p) + 2 * q;
            di.push_back(it); bytes += 2.0 * it.n * esz;
        }
        const int wgs = plan_loop_dot(di.data(), (int)di.size());
        const LoopDotItem* d = upload(s, di);
        ProfScope ps(s, TNQS_PROF_LOOP, bytes, 0);
        launch_loop_dot<T>(s->stream, d, (int)di.size(), wgs);
    }
    std::vector<double> res(2 * nc), fac(verts.size(), 1.0);
    HIPCHK(hipMemcpyAsync(res.data(), d_out->p, nc * 2 * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    for (size_t i = 0; i < verts.size(); ++i) if (s->sscale[verts[i]]) HIPCHK(hipMemcpyAsync(&fac[i], s->sscale[verts[i]]->p, 8, hipMemcpyDeviceToHost, s->stream));
    sync(s);
    for (size_t q = 0; q < nc; ++q) {
        double f = 1.0;
        for (int v : cfg[q]->verts) { const double a = fac[std::find(verts.begin(), verts.end(), v) - verts.begin()]; f *= a * a; }
        out[2 * (size_t)cfg[q]->slot] = res[2 * q] * f; out[2 * (size_t)cfg[q]->slot + 1] = res[2 * q + 1] * f;
    }
}
}  // namespace

void config_weights(State* s, int nconfigs, const int32_t* config_nedges, const int32_t* edge_u, const int32_t* edge_v, double* out_re_im) {
    if (nconfigs < 0 || (nconfigs > 0 && (!config_nedges || !edge_u || !edge_v || !out_re_im))) throw Err(TNQS_ERR_INVALID, "config_weights: bad arguments");
    if (s->sharded()) throw Err(TNQS_ERR_UNSUPPORTED, "config_weights: sharded handles are not supported");
    if (nconfigs == 0) return;
    // everything the host can decide first: decomposition, shapes, workspace
    std::vector<Config> cfg; cfg.reserve(nconfigs);
    size_t off = 0;
    for (int c = 0; c < nconfigs; ++c) {
        if (config_nedges[c] < 1) throw Err(TNQS_ERR_INVALID, "config_weights: a configuration has at least one edge");
        cfg.push_back(decompose(*s->g, config_nedges[c], edge_u + off, edge_v + off));
        cfg.back().slot = c; describe(s, cfg.back()); off += (size_t)config_nedges[c];
    }
    HIPCHK(hipSetDevice(s->device));
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    free_b += s->pool->bytes_cached();      // what the handle's pool holds from earlier calls is handed out again (or given back when an allocation fails)
    for (auto& c : cfg) if (c.ws_bytes > free_b)
        throw Err(TNQS_ERR_UNSUPPORTED, "config_weights: configuration " + std::to_string(c.slot) + " needs " + std::to_string(c.ws_bytes) + " bytes of workspace, " + std::to_string(free_b) + " bytes are free");
    // simple cycles: the cycle code, in the ring order of the decomposition
    {
        std::vector<int32_t> len, vs; std::vector<int> slots;
        for (auto& c : cfg) if (c.shape == kCycle) { len.push_back((int32_t)c.ring.size()); vs.insert(vs.end(), c.ring.begin(), c.ring.end()); slots.push_back(c.slot); }
        if (!len.empty()) {
            std::vector<double> w(2 * len.size());
            loop_weights(s, (int)len.size(), len.data(), vs.data(), w.data());
            for (size_t i = 0; i < slots.size(); ++i) { out_re_im[2 * (size_t)slots[i]] = w[2 * i]; out_re_im[2 * (size_t)slots[i] + 1] = w[2 * i + 1]; }
        }
    }
    const size_t budget = std::min<size_t>(size_t(2) << 30, free_b / 4);
    std::vector<Config*> rest; for (auto& c : cfg) if (c.shape != kCycle) rest.push_back(&c);
    for (size_t c = 0; c < rest.size();) {
        std::vector<Config*> batch; size_t bytes = 0;
        while (c < rest.size()) {
            if (!batch.empty() && bytes + rest[c]->ws_bytes > budget) break;
            bytes += rest[c]->ws_bytes; batch.push_back(rest[c]); ++c;
        }
        if (s->dtype == TNQS_C64) config_batch<float>(s, batch, out_re_im); else config_batch<double>(s, batch, out_re_im);
        for (Config* b : batch) *b = Config{};      // the batch's device buffers go back to the pool
    }
}

}  // namespace tnqs
