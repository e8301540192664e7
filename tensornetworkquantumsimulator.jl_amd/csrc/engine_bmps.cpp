// engine_bmps.cpp -- expect(psi, obs; alg = "boundarymps") and norm_sqr(psi; alg = "boundarymps") (src/expect.jl:84-156, src/norm_sqr.jl:86-91) on an open rectangular
// grid: the partition plan, the fitting driver and the measurement of src/MessagePassing/boundarympscache.jl in one call.
//   Plan (host, before any device work): partitions = the values of the grouping coordinate, a partition's vertices ordered by the other one (BoundaryMPSCache, :145-175,
//   sorted_edges, :604-614); is_correct_format (:69-81) and the absence of pseudo-edges (:560-576) are checked on the handle's graph, and every cross edge has to join equal
//   positions of neighbouring partitions (a full grid).  Link dimensions: virtual_index_dimension (:119-143).
//   Messages: per directed quotient edge p -> q one tensor M_l[link_l, a, a', link_{l+1}] per position l, dense, first index fastest.  They are fitted once, down the line and
//   up the line (maxiter = 1 on a line, :30; p -> p + 1 needs only p - 1 -> p), by update_message!(alg "fitting", :330-369).  What the reference keeps on the reverse edges
//   while it fits -- the daggered guess -- is Bt here; the environments inside the partition (update_partition!, :228-244) are Lenv[l] / Renv[l] = everything left / right of
//   position l with legs [incoming link, h, h', fitted link].  A local update (extracter, :311-319) is four contractions -- U L over the incoming link, A over (in, left),
//   conj(A) over (s, in', left'), R over (link, right, right') -- so the double-layer site tensor is never formed; an environment step replaces the last by Bt.  Every
//   contraction is one launch of bmps_contract_kernel over strided views (no permuted copy), every gauge step (:270-285) one launch of bmps_qr_kernel and one contraction.
//   The down and the up chain are NOT run as two items of the same launches: one contraction per launch, one chain after the other.
//   Host round trips: with a tolerance one read-back of cf per sweep; without, none until the call's one read-back (every sweep's cf is kept on the device).
//   Measurement (path_contract, :616-667): the left and right environments of a partition between its two incoming MPS are built once and shared by its observables (the
//   reference walks from leaf to leaf per observable: the same numbers up to rounding); numer = Lenv . sites with the operators . Renv, denom = the same at the first
//   support position with identities.  Norm (:504-519): log Z = sum_p log(vertex scalar) - sum_(p, p + 1) log(edge scalar), scalars complex128 whatever the element type.
// The handle's site tensors and messages are read only.  Booked under TNQS_PROF_SMALL.
#include "engine_internal.hpp"

namespace tnqs {

namespace {

enum : int { S = 0, KI, KO, KL, KR, BI, BO, BL, BR, UL, UR, DL, DR, S2, E1, E2 };      // leg labels: site, ket / bra legs towards in / out / left / right, links of the two MPS

struct Ten {
    Buf buf; const void* p = nullptr; int nd = 0; int lab[8]; int dim[8]; long long str[8];
    int find(int l) const { for (int i = 0; i < nd; ++i) if (lab[i] == l) return i; return -1; }
    long long size() const { long long n = 1; for (int i = 0; i < nd; ++i) n *= dim[i]; return n; }
    void add(int l, int d, long long st) { if (nd >= 8) throw Err(TNQS_ERR_UNSUPPORTED, "bmps: tensor with more than 8 legs"); lab[nd] = l; dim[nd] = d; str[nd] = st; ++nd; }
    Ten relabel(std::initializer_list<std::pair<int, int>> m) const { Ten t = *this; for (int i = 0; i < nd; ++i) for (auto& q : m) if (lab[i] == q.first) t.lab[i] = q.second; return t; }
};

struct GridPlan {
    int P = 0, L = 0;
    std::vector<int> vert;                  // vert[p * L + l]
    std::vector<int> part, pos;             // per vertex
    int at(int p, int l) const { return vert[(size_t)p * L + l]; }
};

// the partitioned graph of BoundaryMPSCache(...) (:145-175) for a handle whose vertices carry the coordinates (row, col); throws what is_correct_format (:69-81) would
GridPlan plan_grid(const Graph& g, const int32_t* vrow, const int32_t* vcol, int by) {
    GridPlan gp; const int nv = g.nv;
    std::vector<int> key(nv), ord(nv);
    for (int v = 0; v < nv; ++v) { key[v] = by == 0 ? vrow[v] : vcol[v]; ord[v] = by == 0 ? vcol[v] : vrow[v]; }
    std::vector<int> keys(key.begin(), key.end()); std::sort(keys.begin(), keys.end()); keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    gp.P = (int)keys.size(); gp.part.assign(nv, 0); gp.pos.assign(nv, 0);
    std::vector<std::vector<int>> groups(gp.P);
    for (int v = 0; v < nv; ++v) { gp.part[v] = (int)(std::lower_bound(keys.begin(), keys.end(), key[v]) - keys.begin()); groups[gp.part[v]].push_back(v); }
    for (auto& gr : groups) {
        std::sort(gr.begin(), gr.end(), [&](int a, int b) { return ord[a] < ord[b]; });
        for (size_t i = 0; i + 1 < gr.size(); ++i) {
            if (ord[gr[i]] == ord[gr[i + 1]]) throw Err(TNQS_ERR_INVALID, "boundarymps: two vertices carry the same coordinates");
            if (g.edge(gr[i], gr[i + 1]) < 0) throw Err(TNQS_ERR_INVALID, "boundarymps: consecutive vertices of a partition are not neighbours: the graph would need pseudo-edges, which are not supported");
        }
        for (size_t i = 0; i < gr.size(); ++i) gp.pos[gr[i]] = (int)i;
    }
    for (int e = 0; e < g.ne; ++e) {                      // the quotient graph first, then the partitions, as is_correct_format does
        const int dp = std::abs(gp.part[g.esrc[e]] - gp.part[g.edst[e]]);
        if (dp > 1) {
            if (dp == gp.P - 1) throw Err(TNQS_ERR_INVALID, "boundarymps: upon partitioning the graph forms a ring (periodic boundaries), which is not supported");
            throw Err(TNQS_ERR_INVALID, "Upon partitioning, graph does not form a line or ring: can't run boundary MPS");
        }
    }
    for (int e = 0; e < g.ne; ++e) {
        const int u = g.esrc[e], w = g.edst[e];
        if (gp.part[u] == gp.part[w] && std::abs(gp.pos[u] - gp.pos[w]) != 1) throw Err(TNQS_ERR_INVALID, "There's a partition that does not form a line: can't run boundary MPS");
    }
    if (gp.P < 2) throw Err(TNQS_ERR_INVALID, "boundarymps: fewer than two partitions");
    gp.L = (int)groups[0].size();
    if (gp.L < 2) throw Err(TNQS_ERR_INVALID, "boundarymps: fewer than two vertices in a partition");
    for (auto& gr : groups) if ((int)gr.size() != gp.L) throw Err(TNQS_ERR_UNSUPPORTED, "boundarymps: partitions of different lengths (only rectangular grids are supported)");
    gp.vert.resize((size_t)gp.P * gp.L);
    for (int p = 0; p < gp.P; ++p) for (int l = 0; l < gp.L; ++l) gp.vert[(size_t)p * gp.L + l] = groups[p][l];
    for (int e = 0; e < g.ne; ++e) {
        const int u = g.esrc[e], w = g.edst[e];
        if (gp.part[u] != gp.part[w] && gp.pos[u] != gp.pos[w]) throw Err(TNQS_ERR_UNSUPPORTED, "boundarymps: an edge between partitions joins different positions (only rectangular grids are supported)");
    }
    for (int p = 0; p + 1 < gp.P; ++p) for (int l = 0; l < gp.L; ++l)
        if (g.edge(gp.at(p, l), gp.at(p + 1, l)) < 0) throw Err(TNQS_ERR_UNSUPPORTED, "boundarymps: a missing edge between neighbouring partitions (only rectangular grids are supported)");
    return gp;
}

// virtual_index_dimension (:119-143): link l sits between positions l - 1 and l of the cross edges with bond dimensions chi[0 .. L - 1]; links 0 and L are 1
std::vector<int> link_dims(const std::vector<int>& chi, int R) {
    const int L = (int)chi.size(); std::vector<int> link(L + 1, 1);
    for (int l = 1; l < L; ++l) {
        double below = 1, above = 1;
        for (int k = 0; k < l; ++k) below *= chi[k];
        for (int k = l; k < L; ++k) above *= chi[k];
        link[l] = (int)std::min(std::min(above * above, below * below), (double)R);
    }
    return link;
}

struct Obs { int part, lmin, lmax; std::vector<int> pos; std::vector<const double*> op; };

template <class T> struct Bmps {
    State* const s; const Graph& g; const GridPlan& gp; const size_t esz;
    const int R, niters, normalize; const double tol;
    Buf one_b, ones_b; std::map<int, Buf> eyes;
    int nlaunches = 0;
    Bmps(State* st, const GridPlan& p, int r, int ni, int nz, double tl) : s(st), g(*st->g), gp(p), esz(st->esz()), R(r), niters(ni), normalize(nz), tol(tl) {
        std::vector<T> h(2 * 64, (T)0); for (int i = 0; i < 64; ++i) h[2 * i] = (T)1;
        upload(s, h); ones_b = s->keepalive.back(); one_b = ones_b;      // ours from here on: a synchronisation between sweeps empties the keep-alive list
    }
    Ten dense(std::initializer_list<std::pair<int, int>> legs) {
        Ten t; long long st = 1; for (auto& q : legs) { t.add(q.first, q.second, st); st *= q.second; }
        t.buf = dalloc(s, (size_t)st * esz); t.p = t.buf->p; return t;
    }
    Ten trivial(std::initializer_list<int> labs) { Ten t; for (int l : labs) t.add(l, 1, 0); t.buf = one_b; t.p = one_b->p; return t; }
    const Buf& eye(int d) {
        Buf& b = eyes[d];
        if (!b) { std::vector<T> h(2 * (size_t)d * d, (T)0); for (int i = 0; i < d; ++i) h[2 * ((size_t)i + (size_t)d * i)] = (T)1; upload(s, h); b = s->keepalive.back(); }
        return b;
    }
    // C = A B (B conjugated on request) over the legs the two share; the output's legs: A's own in A's order, then B's own in B's order, dense, first fastest.
    // scalar != null: every leg is shared and the complex128 result goes there
    Ten contract(const Ten& A, const Ten& B, bool conjB, double* scalar = nullptr) {
        BmpsContractItem it{}; Ten C; long long cst = 1;
        it.A = A.p; it.B = B.p; it.conjB = conjB ? 1 : 0;
        auto push = [&](int& n, int* d, long long* s1, long long* s2, int dim, long long a, long long b) {
            if (dim == 1) return;
            if (n >= kBmpsMaxLegs) throw Err(TNQS_ERR_UNSUPPORTED, "bmps: more than four legs in a group of a contraction");
            d[n] = dim; s1[n] = a; s2[n] = b; ++n;
        };
        for (int i = 0; i < A.nd; ++i) {
            const int j = B.find(A.lab[i]);
            if (j >= 0) {
                if (A.dim[i] != B.dim[j]) throw Err(TNQS_ERR_INVALID, "bmps: a shared leg has two dimensions");
                push(it.nk, it.kd, it.ka, it.kb, A.dim[i], A.str[i], B.str[j]);
            } else { push(it.nm, it.md, it.ma, it.mc, A.dim[i], A.str[i], cst); C.add(A.lab[i], A.dim[i], cst); cst *= A.dim[i]; }
        }
        for (int j = 0; j < B.nd; ++j) if (A.find(B.lab[j]) < 0) { push(it.nn, it.nd, it.nb, it.nc, B.dim[j], B.str[j], cst); C.add(B.lab[j], B.dim[j], cst); cst *= B.dim[j]; }
        if (scalar) { if (C.nd) throw Err(TNQS_ERR_INVALID, "bmps: a scalar contraction with an open leg"); it.C = scalar; it.out_f64 = 1; }
        else { C.buf = dalloc(s, (size_t)cst * esz); C.p = C.buf->p; it.C = C.buf->p; }
        size_t npart = 0; int wgs[2];
        plan_bmps_contract(&it, 1, esz, 0, &npart, wgs);
        Buf part; if (npart) { part = dalloc(s, npart * esz); it.partial = part->p; }
        const BmpsContractItem* d = upload(s, std::vector<BmpsContractItem>(1, it));
        ProfScope ps(s, TNQS_PROF_SMALL, (double)(it.M * it.K + it.K * it.N + it.M * it.N) * esz, 8.0 * it.M * it.N * it.K);
        launch_bmps_contract<T>(s->stream, d, 1, wgs[0]);
        if (wgs[1]) launch_bmps_reduce<T>(s->stream, d, 1, wgs[1]);
        nlaunches += 1 + (wgs[1] ? 1 : 0);
        return C;      // (a partial buffer goes back to the pool here: reuse is stream-ordered)
    }
    // the site tensor of vertex v as a strided view: every leg towards the partitions `pin` / `pout` and the positions left / right, dimension 1 where there is none
    Ten site_view(int v, int pin, int pout, bool bra) const {
        Ten t; t.p = s->site[v]->p; t.buf = s->site[v];
        t.add(S, s->d[v], 1);
        long long st = s->d[v]; bool have[4] = {false, false, false, false};
        const int labs[4] = {bra ? BI : KI, bra ? BO : KO, bra ? BL : KL, bra ? BR : KR};
        for (size_t j = 0; j < g.nbr[v].size(); ++j) {
            const int w = g.nbr[v][j], c = s->chi[g.nbr_e[v][j]];
            int r;
            if (gp.part[w] == gp.part[v]) r = gp.pos[w] < gp.pos[v] ? 2 : 3;
            else r = gp.part[w] == pin ? 0 : (gp.part[w] == pout ? 1 : -1);
            if (r < 0 || have[r]) throw Err(TNQS_ERR_INVALID, "bmps: a vertex with an unexpected neighbour");
            have[r] = true; t.add(labs[r], c, st); st *= c;
        }
        for (int r = 0; r < 4; ++r) if (!have[r]) t.add(labs[r], 1, 0);
        return t;
    }
    // everything left of position l + 1 from everything left of l: [UL, KL, BL, DL] -> [UR, KR, BR, DR] of site l, relabelled for the next site
    Ten three(const Ten& U, const Ten& env, const Ten& ket, const Ten& bra) { const Ten t1 = contract(U, env, false), t2 = contract(t1, ket, false); return contract(t2, bra, true); }
    Ten left_step(const Ten& U, const Ten& Lenv, const Ten& ket, const Ten& bra, const Ten& V) {
        return contract(three(U, Lenv, ket, bra), V, false).relabel({{UR, UL}, {KR, KL}, {BR, BL}, {DR, DL}});
    }
    Ten right_step(const Ten& U, const Ten& Renv, const Ten& ket, const Ten& bra, const Ten& V) {
        return contract(three(U, Renv, ket, bra), V, false).relabel({{UL, UR}, {KL, KR}, {BL, BR}, {DL, DR}});
    }
    void qr(const Ten& A, bool cols_are_first_leg, Ten& Q, Ten& Y) {
        const int n = cols_are_first_leg ? A.dim[0] : A.dim[3]; const long long m = A.size() / n;
        if (m < n || n > kBmpsQrMaxCols) throw Err(TNQS_ERR_UNSUPPORTED, "bmps: a gauge step with fewer rows than columns or more than 64 columns");
        Q = dense({{A.lab[0], A.dim[0]}, {A.lab[1], A.dim[1]}, {A.lab[2], A.dim[2]}, {A.lab[3], A.dim[3]}});
        Y = dense({{E1, n}, {E2, n}});
        Buf W = dalloc(s, 2 * (size_t)m * n * esz);
        BmpsQrItem it{}; it.A = A.p; it.Q = Q.buf->p; it.Y = Y.buf->p; it.W = W->p; it.W2 = reinterpret_cast<char*>(W->p) + (size_t)m * n * esz; it.m = (int)m; it.n = n;
        if (cols_are_first_leg) { it.ars = it.qrs = n; it.acs = it.qcs = 1; } else { it.ars = it.qrs = 1; it.acs = it.qcs = m; }
        const BmpsQrItem* d = upload_small(s, std::vector<BmpsQrItem>(1, it));      // one workgroup per item: read from the pinned arena, launched at once
        ProfScope ps(s, TNQS_PROF_SMALL, 2.0 * m * n * esz, 16.0 * m * n * n);
        launch_bmps_qr<T>(s->stream, d, 1); ++nlaunches;
    }
    // gauge_step! (:270-285): the orthogonality centre moves from Bt[from] to its neighbour Bt[to]
    void gauge_step(std::vector<Ten>& Bt, int from, int to) {
        Ten Q, Y;
        if (to > from) {
            qr(Bt[from], false, Q, Y);
            Bt[to] = contract(Y, Bt[to].relabel({{DL, E2}}), false).relabel({{E1, DL}});
        } else {
            qr(Bt[from], true, Q, Y);
            Bt[to] = contract(Bt[to].relabel({{DR, E2}}), Y, false).relabel({{E1, DR}});
        }
        Bt[from] = Q;
    }
    struct Fit { std::vector<Ten> msg; int sweeps = 0; double eps = std::numeric_limits<double>::quiet_NaN(); Buf cfs; };
    // update_message!(alg "fitting", :330-369) for the message p -> p + dir; U: the message into p from the other side (null at the end of the line)
    Fit fit(int p, int dir, const std::vector<Ten>* Uin) {
        const int L = gp.L, q = p + dir;
        std::vector<int> chi(L);
        for (int l = 0; l < L; ++l) chi[l] = s->chi[g.edge(gp.at(p, l), gp.at(q, l))];
        const std::vector<int> link = link_dims(chi, R);
        std::vector<Ten> U(L), ket(L), bra(L), Bt(L), Lenv(L), Renv(L);
        for (int l = 0; l < L; ++l) {
            U[l] = Uin ? (*Uin)[l].relabel({{DL, UL}, {KO, KI}, {BO, BI}, {DR, UR}}) : trivial({UL, KI, BI, UR});
            ket[l] = site_view(gp.at(p, l), p - dir, q, false); bra[l] = site_view(gp.at(p, l), p - dir, q, true);
            // the guess (:180-202): default_message = delta(a, a') (tensornetworkstate.jl:72-75) times all-ones links; dag() of a real tensor is itself
            Ten a; a.buf = ones_b; a.p = ones_b->p; a.add(DL, link[l], 1);
            Ten e; e.buf = eye(chi[l]); e.p = e.buf->p; e.add(KO, chi[l], 1); e.add(BO, chi[l], chi[l]);
            Ten b; b.buf = ones_b; b.p = ones_b->p; b.add(DR, link[l + 1], 1);
            Bt[l] = contract(contract(a, e, false), b, false);
        }
        for (int i = L - 1; i >= 1; --i) gauge_step(Bt, i, i - 1);                       // init_gauge_seq (:339-341)
        Lenv[0] = trivial({UL, KL, BL, DL}); Renv[L - 1] = trivial({UR, KR, BR, DR});
        for (int l = L - 1; l >= 1; --l) Renv[l - 1] = right_step(U[l], Renv[l], ket[l], bra[l], Bt[l]);      // init_update_seq (:340-342)
        std::vector<int> seq;
        for (int l = 0; l < L; ++l) seq.push_back(l);
        for (int l = L - 2; l >= 1; --l) seq.push_back(l);
        Fit f; f.cfs = dalloc(s, ((size_t)niters + 2 * L + 2) * sizeof(double));
        double* const d_cf = reinterpret_cast<double*>(f.cfs->p); double* const d_norms = d_cf + niters;
        int prev = -1; double prev_cf = 0;
        for (int iter = 1; iter <= niters; ++iter) {
            if (iter == niters) seq.push_back(0);
            for (size_t k = 0; k < seq.size(); ++k) {
                const int l = seq[k];
                if (prev >= 0) {                                                          // updater! (:321-328)
                    gauge_step(Bt, prev, l);
                    if (l > prev) Lenv[l] = left_step(U[prev], Lenv[prev], ket[prev], bra[prev], Bt[prev]);
                    else Renv[l] = right_step(U[prev], Renv[prev], ket[prev], bra[prev], Bt[prev]);
                }
                const Ten m = contract(three(U[l], Lenv[l], ket[l], bra[l]), Renv[l], false);      // extracter (:311-319): [DL, KO, BO, DR]
                Ten nb = dense({{DL, m.dim[0]}, {KO, m.dim[1]}, {BO, m.dim[2]}, {DR, m.dim[3]}});
                if (m.lab[0] != DL || m.lab[1] != KO || m.lab[2] != BO || m.lab[3] != DR) throw Err(TNQS_ERR_INVALID, "bmps: unexpected leg order of a local tensor");
                const BmpsNormItem ni{m.p, nb.buf->p, m.size(), d_norms + k, normalize, 1};       // norm, normalize, inserter! (:352-358)
                const BmpsNormItem* d = upload_small(s, std::vector<BmpsNormItem>(1, ni));
                { ProfScope ps(s, TNQS_PROF_SMALL, 2.0 * m.size() * esz, 0); launch_bmps_norm<T>(s->stream, d, 1); ++nlaunches; }
                Bt[l] = nb; prev = l;
            }
            { ProfScope ps(s, TNQS_PROF_SMALL, 0, 0); launch_sum_doubles(s->stream, d_norms, (int)seq.size(), d_cf + (iter - 1)); ++nlaunches; }
            f.sweeps = iter;
            if (tol >= 0) {                                                               // the one read-back of a sweep
                const double* h = readback<double>(s, d_cf + (iter - 1), 1);
                sync(s);
                const double cf = *h / (double)seq.size();
                f.eps = std::fabs(cf - prev_cf); prev_cf = cf;
                if (f.eps < tol) break;
            }
        }
        f.msg.resize(L);
        for (int l = 0; l < L; ++l) {                                                     // switch_messages! (:204-218): the message is the dagger of what was fitted
            f.msg[l] = dense({{DL, Bt[l].dim[0]}, {KO, Bt[l].dim[1]}, {BO, Bt[l].dim[2]}, {DR, Bt[l].dim[3]}});
            const BmpsNormItem ni{Bt[l].p, f.msg[l].buf->p, Bt[l].size(), nullptr, 0, 1};
            const BmpsNormItem* d = upload_small(s, std::vector<BmpsNormItem>(1, ni));
            ProfScope ps(s, TNQS_PROF_SMALL, 2.0 * Bt[l].size() * esz, 0); launch_bmps_norm<T>(s->stream, d, 1); ++nlaunches;
        }
        return f;
    }
};

double default_tol(int dtype) { return dtype == TNQS_C64 ? 1e-5 : 1e-8; }      // default_tolerance (beliefpropagationcache.jl:104-108)

template <class T> void expect_bmps_t(State* s, const GridPlan& gp, int R, int niters, int normalize, double tol, const std::vector<Obs>& obs, double* out_nd, double* out_log,
                                      int32_t* out_sweeps, double* out_eps) {
    const int P = gp.P, L = gp.L; const size_t nobs = obs.size();
    Bmps<T> b(s, gp, R, niters, normalize, tol);
    // which messages the request needs: down[p] = p -> p + 1 for p < the last partition measured, up[p] = p + 1 -> p for p >= the first
    int need_down = 0, need_up = P - 1;
    if (out_log) { need_down = P - 1; need_up = 0; }
    for (const Obs& o : obs) { need_down = std::max(need_down, o.part); need_up = std::min(need_up, o.part); }
    std::vector<typename Bmps<T>::Fit> down(P - 1), up(P - 1);
    for (int p = 0; p < need_down; ++p) down[p] = b.fit(p, +1, p > 0 ? &down[p - 1].msg : nullptr);
    for (int p = P - 2; p >= need_up; --p) up[p] = b.fit(p + 1, -1, p + 1 < P - 1 ? &up[p + 1].msg : nullptr);
    // scalars of the call, complex128: numerators, denominators, vertex scalars, edge scalars
    const size_t nsc = 2 * nobs + (out_log ? (size_t)(2 * P - 1) : 0);
    Buf d_sc = dalloc(s, std::max<size_t>(nsc, 1) * 2 * sizeof(double));
    HIPCHK(hipMemsetAsync(d_sc->p, 0, d_sc->bytes, s->stream));
    double* const sc = reinterpret_cast<double*>(d_sc->p);
    std::vector<Buf> opbufs;
    for (int p = 0; p < P; ++p) {
        std::vector<const Obs*> mine; std::vector<size_t> idx;
        for (size_t i = 0; i < nobs; ++i) if (obs[i].part == p) { mine.push_back(&obs[i]); idx.push_back(i); }
        if (mine.empty() && !out_log) continue;
        std::vector<Ten> U(L), V(L), ket(L), bra(L), Lenv(L), Renv(L);
        for (int l = 0; l < L; ++l) {
            U[l] = p > 0 ? down[p - 1].msg[l].relabel({{DL, UL}, {KO, KI}, {BO, BI}, {DR, UR}}) : b.trivial({UL, KI, BI, UR});
            V[l] = p < P - 1 ? up[p].msg[l] : b.trivial({DL, KO, BO, DR});
            ket[l] = b.site_view(gp.at(p, l), p - 1, p + 1, false); bra[l] = b.site_view(gp.at(p, l), p - 1, p + 1, true);
        }
        int lhi = 0, llo = out_log ? 0 : L - 1;      // environments up to the outermost support positions (the vertex scalar is taken at position 0)
        for (const Obs* o : mine) { lhi = std::max(lhi, o->lmin); llo = std::min(llo, o->lmin); }
        Lenv[0] = b.trivial({UL, KL, BL, DL}); Renv[L - 1] = b.trivial({UR, KR, BR, DR});
        for (int l = 0; l < lhi; ++l) Lenv[l + 1] = b.left_step(U[l], Lenv[l], ket[l], bra[l], V[l]);
        for (int l = L - 1; l > llo; --l) Renv[l - 1] = b.right_step(U[l], Renv[l], ket[l], bra[l], V[l]);
        auto close = [&](const Ten& X, int l, double* out) { b.contract(X.relabel({{UL, UR}, {KL, KR}, {BL, BR}, {DL, DR}}), Renv[l], false, out); };
        std::map<int, double*> denoms;
        for (size_t k = 0; k < mine.size(); ++k) {
            const Obs& o = *mine[k];
            Ten X = Lenv[o.lmin];
            for (int l = o.lmin; l <= o.lmax; ++l) {
                Ten kt = ket[l];
                for (size_t q = 0; q < o.pos.size(); ++q) if (o.pos[q] == l) {
                    const int d = s->d[gp.at(p, l)];
                    std::vector<T> h(2 * (size_t)d * d);
                    for (size_t e = 0; e < h.size(); ++e) h[e] = (T)o.op[q][e];
                    upload(s, h); opbufs.push_back(s->keepalive.back());
                    Ten O; O.buf = opbufs.back(); O.p = O.buf->p; O.add(S2, d, 1); O.add(S, d, d);
                    kt = b.contract(O, kt, false).relabel({{S2, S}});
                }
                X = b.left_step(U[l], X, kt, bra[l], V[l]);
            }
            close(X, o.lmax, sc + 4 * idx[k]);
            // the denominator: vertex_scalar at the first support vertex (:630), shared by the observables that start there
            double* const den = sc + 4 * idx[k] + 2;
            auto it = denoms.find(o.lmin);
            if (it == denoms.end()) {
                close(b.left_step(U[o.lmin], Lenv[o.lmin], ket[o.lmin], bra[o.lmin], V[o.lmin]), o.lmin, den);
                denoms[o.lmin] = den;
            } else HIPCHK(hipMemcpyAsync(den, it->second, 2 * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
        }
        if (out_log) {
            close(b.left_step(U[0], Lenv[0], ket[0], bra[0], V[0]), 0, sc + 4 * nobs + 2 * (size_t)p);                 // vertex_scalar (:504-510)
            if (p < P - 1) {                                                                                           // edge_scalar (:512-519)
                Ten E = b.trivial({E1, E2});
                for (int l = 0; l < L; ++l) {
                    const Ten t = b.contract(E, down[p].msg[l].relabel({{DL, E1}, {DR, UR}}), false);
                    E = b.contract(t, up[p].msg[l].relabel({{DL, E2}}), false).relabel({{UR, E1}, {DR, E2}});
                }
                b.contract(E, b.trivial({E1, E2}), false, sc + 4 * nobs + 2 * (size_t)(P + p));
            }
        }
    }
    // the call's read-back: scalars, and every sweep's cf of the fits that ran without a tolerance
    const double* h = readback<double>(s, sc, 2 * std::max<size_t>(nsc, 1));
    std::vector<const double*> hcf(2 * (size_t)(P - 1), nullptr);
    if (tol < 0) for (int k = 0; k < 2 * (P - 1); ++k) {
        auto& f = k < P - 1 ? down[k] : up[k - (P - 1)];
        if (f.sweeps) hcf[k] = readback<double>(s, f.cfs->p, (size_t)niters);
    }
    sync(s);
    for (size_t i = 0; i < 4 * nobs; ++i) {
        if (!std::isfinite(h[i])) throw Err(TNQS_ERR_NUMERIC, "boundarymps: a numerator or denominator is not finite");
        out_nd[i] = h[i];
    }
    if (out_log) {
        std::complex<double> lz(0, 0); bool zero = false;
        for (int i = 0; i < 2 * P - 1; ++i) {
            const std::complex<double> z(h[4 * nobs + 2 * i], h[4 * nobs + 2 * i + 1]);
            if (!std::isfinite(z.real()) || !std::isfinite(z.imag())) throw Err(TNQS_ERR_NUMERIC, "boundarymps: a vertex or edge scalar is not finite");
            if (z == std::complex<double>(0, 0)) { zero = true; continue; }
            if (i < P) lz += std::log(z); else lz -= std::log(z);
        }
        if (zero) { out_log[0] = -std::numeric_limits<double>::infinity(); out_log[1] = 0; }
        else {
            const double pi = 3.14159265358979323846;
            double im = std::fmod(lz.imag(), 2 * pi);
            if (im > pi) im -= 2 * pi; else if (im <= -pi) im += 2 * pi;
            out_log[0] = lz.real(); out_log[1] = im;
        }
    }
    for (int k = 0; k < 2 * (P - 1); ++k) {
        auto& f = k < P - 1 ? down[k] : up[k - (P - 1)];
        if (hcf[k]) {                                      // no tolerance: the last |cf - previous cf| from the cfs the device kept
            const double len = 2.0 * L - 2, last_len = len + 1;
            const double cf = hcf[k][niters - 1] / last_len, pcf = niters > 1 ? hcf[k][niters - 2] / len : 0.0;
            f.eps = std::fabs(cf - pcf);
        }
        if (out_sweeps) out_sweeps[k] = f.sweeps;
        if (out_eps) out_eps[k] = f.eps;
    }
}

}  // namespace

void expect_bmps(State* s, const tnqs_bmps_opts* o, const int32_t* vrow, const int32_t* vcol, int nobs, const int32_t* obs_nverts, const int32_t* obs_verts,
                 const double* obs_ops, double* out_nd, double* out_log, int32_t* out_sweeps, double* out_eps) {
    if (!o || !vrow || !vcol) throw Err(TNQS_ERR_INVALID, "boundarymps: null options or coordinates");
    if (nobs < 0 || (nobs > 0 && (!obs_nverts || !obs_verts || !obs_ops || !out_nd))) throw Err(TNQS_ERR_INVALID, "boundarymps: null observable arrays");
    if (nobs == 0 && !out_log) throw Err(TNQS_ERR_INVALID, "boundarymps: nothing to compute (no observable and no norm output)");
    if (s->sharded()) throw Err(TNQS_ERR_UNSUPPORTED, "boundarymps: sharded handles are not supported");
    if (o->partition_by != 0 && o->partition_by != 1) throw Err(TNQS_ERR_INVALID, "boundarymps: partition_by must be 0 (row) or 1 (col)");
    if (o->mps_bond_dimension < 1) throw Err(TNQS_ERR_INVALID, "boundarymps: mps_bond_dimension must be at least 1");
    const Graph& g = *s->g;
    const GridPlan gp = plan_grid(g, vrow, vcol, o->partition_by);
    const int R = o->mps_bond_dimension;
    int chimax = 1, dmax = 1;
    for (int c : s->chi) chimax = std::max(chimax, c);
    for (int d : s->d) dmax = std::max(dmax, d);
    int Reff = 1;                                         // the largest link any message of this network has at this R: min(x1^2, x2^2, R) (:119-143)
    for (int p = 0; p + 1 < gp.P; ++p) {
        std::vector<int> chi(gp.L);
        for (int l = 0; l < gp.L; ++l) chi[l] = s->chi[g.edge(gp.at(p, l), gp.at(p + 1, l))];
        for (int d : link_dims(chi, R)) Reff = std::max(Reff, d);
    }
    if (!((chimax <= 8 && Reff <= 64) || (chimax <= 16 && Reff <= 16)))
        throw Err(TNQS_ERR_UNSUPPORTED, "boundarymps: bond dimension " + std::to_string(chimax) + " with mps_bond_dimension " + std::to_string(R) + " (largest link " + std::to_string(Reff) +
                                            ") is beyond the supported envelope (chi <= 8 with links <= 64, or chi <= 16 with links <= 16; a link is min(x1^2, x2^2, mps_bond_dimension))");
    if (dmax > 16) throw Err(TNQS_ERR_UNSUPPORTED, "boundarymps: site dimension " + std::to_string(dmax) + " is beyond the supported envelope (d <= 16)");
    std::vector<Obs> obs((size_t)nobs);
    size_t voff = 0, ooff = 0;
    for (int i = 0; i < nobs; ++i) {
        Obs& ob = obs[i];
        if (obs_nverts[i] < 1) throw Err(TNQS_ERR_INVALID, "boundarymps: an observable without support");
        for (int k = 0; k < obs_nverts[i]; ++k) {
            const int v = obs_verts[voff + k];
            if (v < 0 || v >= g.nv) throw Err(TNQS_ERR_INVALID, "boundarymps: bad vertex in an observable");
            if (k == 0) ob.part = gp.part[v];
            else if (gp.part[v] != ob.part) throw Err(TNQS_ERR_INVALID, "Observable support must be within a single partition (row/ column) of the graph for now.");
            for (int q : ob.pos) if (q == gp.pos[v]) throw Err(TNQS_ERR_INVALID, "boundarymps: a vertex appears twice in an observable");
            ob.pos.push_back(gp.pos[v]); ob.op.push_back(obs_ops + ooff);
            ooff += 2 * (size_t)s->d[v] * s->d[v];
        }
        voff += obs_nverts[i];
        ob.lmin = *std::min_element(ob.pos.begin(), ob.pos.end()); ob.lmax = *std::max_element(ob.pos.begin(), ob.pos.end());
    }
    const int niters = o->niters > 0 ? o->niters : 50;                                   // _default_boundarymps_update_niters (:43)
    const double tol = std::isnan(o->tolerance) ? default_tol(s->dtype) : o->tolerance;
    HIPCHK(hipSetDevice(s->device));
    materialize_pending_all(s);
    materialize_scale_all(s);
    if (s->dtype == TNQS_C64) expect_bmps_t<float>(s, gp, R, niters, o->normalize, tol, obs, out_nd, out_log, out_sweeps, out_eps);
    else expect_bmps_t<double>(s, gp, R, niters, o->normalize, tol, obs, out_nd, out_log, out_sweeps, out_eps);
}

}  // namespace tnqs
