// engine_batch.cpp -- batched building blocks of the engine: mode-product chains, Gram jobs, the SVD batch.  Host orchestration only; every
// flop runs in the HIP kernels of kernels*.hip.
#include "engine_internal.hpp"

namespace tnqs {

// ---------------------------------------------------------------------------------------------------------------
// batched building blocks
// ---------------------------------------------------------------------------------------------------------------
void FiberPass::prepare(State* s, size_t k, bool norms) {
    if (norms) np[k] = dalloc(s, (size_t)std::max(1, plan[k].wgs) * sizeof(double));
    d_items[k] = upload(s, plan[k].items);
}
template <class T> void FiberPass::launch(State* s, size_t k, int cls, bool book) const {
    const FiberLaunch& L = plan[k];
    if (L.items.empty()) return;
    double* const partials = np[k] ? reinterpret_cast<double*>(np[k]->p) : nullptr;
    if (cls < 0) { launch_fiber_route<T>(s->stream, L, d_items[k], partials); return; }
    double bytes = 0, flops = 0;
    const bool rg = L.route == FiberRoute::RowGemm;
    if (book && !(rg && k > 0))      // RowGemm launches come first in a plan: launch 0 books them all
        for (size_t q = k; q < plan.size() && (q == k || (rg && plan[q].route == FiberRoute::RowGemm)); ++q)
            for (const FiberItem& it : plan[q].items) {
                const double fibers = (double)it.PA * it.PB, nin = fibers * it.D * it.K;
                bytes += (nin + fibers * it.Do * it.No) * s->esz(); flops += 8.0 * nin * it.Do * it.No;
            }
    ProfScope ps(s, cls, bytes, flops);
    launch_fiber_route<T>(s->stream, L, d_items[k], partials);
}
template void FiberPass::launch<float>(State*, size_t, int, bool) const;
template void FiberPass::launch<double>(State*, size_t, int, bool) const;

template <class T> void run_chains(State* s, std::vector<Chain>& chains, int cls, int cls_pair) {
    if (cls_pair < 0) cls_pair = cls;
    const size_t esz = s->esz();
    std::vector<int> nt(chains.size(), 0);          // temporaries written so far (ping-pong index)
    for (auto& c : chains) c.result = c.src;
    // ---- stage 0: two legs per pass over the tensor -- 32-dimensional legs: mfma_pair_kernel (once), 16-dimensional legs:
    // mfma_pair16_kernel, repeated while a chain still has two of them (a degree-6 site absorbs its legs in 3 passes instead of 5) ---
    if (std::is_same<T, float>::value && use_mfma() && use_pair()) {
        std::vector<PairItem> items; double bytes = 0, flops = 0;
        std::vector<std::pair<size_t, std::pair<int, int>>> sel;     // chain index, (position of x, position of y) in c.steps
        for (size_t ci = 0; ci < chains.size(); ++ci) {
            Chain& c = chains[ci];
            if (c.steps.size() < 2) continue;
            // the two highest eligible legs (steps are in ascending leg order)
            int py = -1, px = -1;
            for (int q = (int)c.steps.size() - 1; q >= 0 && px < 0; --q) {
                int leg = c.steps[q].first;
                bool ok = c.sd.chi[leg] == 32 && leg >= 1 && (c.sd.pre(leg) % 16 == 0);
                if (!ok) continue;
                if (py < 0) py = q; else px = q;
            }
            if (px < 0) continue;
            sel.push_back({ci, {px, py}});
        }
        if (!sel.empty()) {
            for (auto& se : sel) {
                Chain& c = chains[se.first];
                int x = c.steps[se.second.first].first, y = c.steps[se.second.second].first;
                PairItem it{};
                Buf& dst = c.tmp[nt[se.first] & 1];
                if (!dst) dst = dalloc(s, c.sd.n * esz);
                it.in = c.result; it.out = dst->p; it.Mx = c.steps[se.second.first].second; it.My = c.steps[se.second.second].second;
                if (!pair_geometry(c.sd.d, c.sd.z, c.sd.chi.data(), x, y, it.g)) throw Err(TNQS_ERR_HIP, "internal: pair geometry");
                items.push_back(it);
                c.result = dst->p; nt[se.first]++; c.trail.push_back({x, y});
                // drop the two consumed steps
                c.steps.erase(c.steps.begin() + se.second.second); c.steps.erase(c.steps.begin() + se.second.first);
                bytes += 2.0 * c.sd.n * esz; flops += 2 * 8.0 * c.sd.n * 32;
            }
            const int wgs = plan_pair(items.data(), (int)items.size());
            const PairItem* d = upload(s, items);
            ProfScope ps(s, cls_pair, bytes, flops);
            launch_mfma_pair(s->stream, d, (int)items.size(), wgs);
        }
        for (;;) {                                                  // 16-dimensional legs, two per round
            std::vector<Pair16Item> it16; std::vector<std::pair<size_t, std::pair<int, int>>> sel16; double by16 = 0, fl16 = 0;
            for (size_t ci = 0; ci < chains.size(); ++ci) {
                Chain& c = chains[ci];
                if (c.steps.size() < 2 || c.sd.n < (size_t)(1u << 14)) continue;     // small tensors stay on the single-leg kernel (launch bound)
                bool found = false;
                if (c.ordered) {                                                     // the caller's first two legs, when they form a plane
                    Pair16Item it{};
                    if (plane_geometry(c.sd.d, c.sd.z, c.sd.chi.data(), c.steps[0].first, c.steps[1].first, 16, it.g)) {
                        it.Mx = c.steps[0].second; it.My = c.steps[1].second;
                        it16.push_back(it); sel16.push_back({ci, {0, 1}}); found = true;
                    }
                }
                // the LOWEST remaining leg with the HIGHEST one (round 5): a plane that contains leg 0 streams at 4.4 - 4.55 TB/s, every other one at 3.7 - 3.9 and
                // (3,5) at 3.0 (profiles/plane16_bench.py, 12 sites, random data) -- "the two highest legs first" gave the y-lines of the cubic lattice (cross legs
                // 0, 2, 3, 5) the passes (3,5) + (0,2) = 3.57 ms per 12 sites, this rule (0,5) + (2,3) = 3.16; x-lines 3.17 -> 3.14, z-lines 3.33 -> 3.38
                for (int qx = 0; qx + 1 < (int)c.steps.size() && !found; ++qx)
                    for (int qy = (int)c.steps.size() - 1; qy > qx && !found; --qy) {
                        Pair16Item it{};
                        if (!plane_geometry(c.sd.d, c.sd.z, c.sd.chi.data(), c.steps[qx].first, c.steps[qy].first, 16, it.g)) continue;
                        it.Mx = c.steps[qx].second; it.My = c.steps[qy].second;
                        it16.push_back(it); sel16.push_back({ci, {qx, qy}}); found = true;
                    }
            }
            if (it16.empty()) break;
            std::vector<Pair16Item> kind[2]; int wgs16[2];           // [1]: whole 128-byte lines per wave (pair16_whole_lines)
            plan_pair16(it16.data(), (int)it16.size(), wgs16);
            for (size_t q = 0; q < it16.size(); ++q) {
                Chain& c = chains[sel16[q].first]; Pair16Item& it = it16[q];
                Buf& dst = c.tmp[nt[sel16[q].first] & 1];
                if (!dst) dst = dalloc(s, c.sd.n * esz);
                it.in = c.result; it.out = dst->p;
                kind[pair16_whole_lines(it.g) ? 1 : 0].push_back(it);
                c.result = dst->p; nt[sel16[q].first]++;
                c.trail.push_back({c.steps[sel16[q].second.first].first, c.steps[sel16[q].second.second].first});
                c.steps.erase(c.steps.begin() + sel16[q].second.second); c.steps.erase(c.steps.begin() + sel16[q].second.first);
                by16 += 2.0 * c.sd.n * esz; fl16 += 2 * 8.0 * c.sd.n * 16;
            }
            ProfScope ps(s, cls_pair, by16, fl16);
            for (int wl = 0; wl < 2; ++wl) {
                if (kind[wl].empty()) continue;
                const Pair16Item* d = upload(s, kind[wl]);
                launch_mfma_pair16(s->stream, d, (int)kind[wl].size(), wgs16[wl], wl == 1);
            }
        }
    }
    size_t maxsteps = 0;
    for (auto& c : chains) maxsteps = std::max(maxsteps, c.steps.size());
    const FiberRules rules = fiber_rules_of(s, FiberUse::Chain);
    std::vector<FiberItem> items;
    for (size_t o = 0; o < maxsteps; ++o) {
        items.clear();
        for (size_t ci = 0; ci < chains.size(); ++ci) {
            Chain& c = chains[ci];
            if (c.steps.size() <= o) continue;
            const int j = c.steps[o].first;
            c.trail.push_back({j});
            Buf& dst = c.tmp[nt[ci] & 1];
            if (!dst) dst = dalloc(s, c.sd.n * esz);
            FiberItem it = site_fiber_item(c.sd, j, false, c.sd.chi[j], false);
            it.in = c.result; it.out = dst->p; it.X = c.steps[o].second;
            items.push_back(it);
            c.result = dst->p; nt[ci]++;
        }
        FiberPass(items, rules, esz).run<T>(s, cls, /*norms=*/false);
    }
}

// the tall route of svd_batch (ComplexF32, no V): Cholesky-QR preprocessing, Jacobi on R, A <- A J, polishing sweeps where the pivot collapsed.
// d_fail (nt ints, may be null): the per-item Cholesky failure flags; d_polish_sweeps (nt ints, may be null): the sweeps of the polishing pass
// (written only by the items it ran on)
void svd_tall(State* s, const std::vector<JacobiItem>& tall, int* d_fail_out, int* d_polish_sweeps) {
    const size_t esz = sizeof(float) * 2;
    const size_t nt = tall.size();
    size_t off = 0; std::vector<size_t> oG(nt), oL(nt), oW(nt), oR0(nt), oRr(nt), oJ(nt), oT(nt);
    for (size_t i = 0; i < nt; ++i) {
        const size_t nn = (size_t)tall[i].n * tall[i].n, mn = (size_t)tall[i].m * tall[i].n;
        oG[i] = off; off += round256(nn * 16); oL[i] = off; off += round256(nn * 16); oW[i] = off; off += round256(nn * 16);
        oR0[i] = off; off += round256(nn * 8); oRr[i] = off; off += round256(nn * 8); oJ[i] = off; off += round256(nn * 16); oT[i] = off; off += round256(mn * 8);
    }
    Buf arena = dalloc(s, off); s->keepalive.push_back(arena);
    Buf fail_buf; if (!d_fail_out) { fail_buf = dalloc(s, nt * sizeof(int)); s->keepalive.push_back(fail_buf); }
    int* const d_fail = d_fail_out ? d_fail_out : reinterpret_cast<int*>(fail_buf->p);
    HIPCHK(hipMemsetAsync(d_fail, 0, nt * sizeof(int), s->stream));
    char* ap = reinterpret_cast<char*>(arena->p);
    std::vector<TallSvdItem> ti, wi; std::vector<CholItem> ci; std::vector<JacobiItem> rj; std::vector<SmallGemmItem> gi; std::vector<CopyItem> cp;
    int nmax = 1, mmax = 1;
    for (size_t i = 0; i < nt; ++i) {
        const int m = tall[i].m, n = tall[i].n; nmax = std::max(nmax, n); mmax = std::max(mmax, m);
        ti.push_back(TallSvdItem{tall[i].A, ap + oG[i], ap + oL[i], ap + oR0[i], ap + oRr[i], m, n});
        // delta = 1e-14 of the largest diagonal entry: singular directions below 1e-7 sigma_max are f32 noise of the data anyway, and R keeps
        // a condition number <= 1e7 whatever the rank of A (no failure branch: a rank-deficient theta is the normal case early in an evolution)
        ci.push_back(CholItem{ap + oG[i], ap + oL[i], ap + oW[i], n, d_fail + i, 0.0, 1e-14});      // Winv = (L^-1)^dagger = R^-1
        rj.push_back(JacobiItem{ap + oRr[i], nullptr, n, n, tall[i].sweeps_out});
        wi.push_back(TallSvdItem{nullptr, d_fail + i, ap + oW[i], ap + oJ[i], ap + oRr[i], n, n});   // J = R^-1 (R J), f64; G slot: the item's Cholesky failure flag (J := I then)
        gi.push_back(SmallGemmItem{tall[i].A, ap + oJ[i], ap + oT[i], m, n, n});
        cp.push_back(CopyItem{ap + oT[i], tall[i].A, (size_t)m * n / 2, (m * n) & 1});      // ComplexF32 elements in pairs; an odd count leaves one
    }
    const TallSvdItem* dt = upload(s, ti); const CholItem* dc = upload(s, ci); const JacobiItem* dj = upload(s, rj);
    const TallSvdItem* dw = upload(s, wi); const SmallGemmItem* dg = upload(s, gi); const CopyItem* dcp = upload(s, cp);
    launch_tall_gram(s->stream, dt, (int)nt, nmax);
    launch_chol_packed(s->stream, dc, (int)nt, nmax);
    launch_tall_rt(s->stream, dt, (int)nt);
    size_t lds = 0; for (auto& j : rj) lds = std::max(lds, jacobi_lds_bytes(j.m, j.n, false, esz));
    launch_jacobi<float>(s->stream, dj, (int)nt, 60, lds, nmax);
    launch_tall_w(s->stream, dw, (int)nt, nmax);
    launch_tall_mj(s->stream, dg, (int)nt);                        // A J in f64 (J is complex128): column-relative accuracy, no polishing needed
    launch_copy_items(s->stream, dcp, (int)nt);
    // Polishing sweeps on A J itself are only needed where the preprocessing gave nothing to build on: an item whose Cholesky pivot
    // collapsed in spite of the shift (J := I above) is factorised from scratch here; every other item is skipped on the device
    // (JacobiItem::only_if).  Round 2 polished every item (2.6 ms per chi = 64 colour batch): its A J was an f32 product with an f32 J,
    // which leaves eps32 sigma_max of residue in every column -- the f64 product does not.
    std::vector<JacobiItem> pol;
    for (size_t i = 0; i < nt; ++i) { JacobiItem j{tall[i].A, nullptr, tall[i].m, tall[i].n, d_polish_sweeps ? d_polish_sweeps + i : nullptr}; j.only_if = d_fail + i; pol.push_back(j); }
    const JacobiItem* dp = upload(s, pol);
    launch_jacobi<float>(s->stream, dp, (int)nt, 60, 0, mmax);
    s->stats.n_tall_svd += (int)nt;
}

// One-sided Jacobi SVD of a batch of matrices (A <- U Sigma in place; V accumulated only when the items carry one).  Three routes:
//   * the matrix fits the LDS (jacobi_lds_kernel);
//   * ComplexF32, no V wanted, too tall for the LDS but its n x n triangle fits (256 x 128 at chi = 64): Cholesky-QR preprocessing --
//     G = A^dagger A (f64) -> R = chol(G + delta I)^dagger -> Jacobi on R in LDS -> J = R^-1 (U_R S_R) (f64) -> A <- A J
//     (kernels_chi64.hip; the rotations that orthogonalise R's columns orthogonalise A's, delta only conditions R), followed by
//     polishing sweeps of the global-memory kernel on A J (relative orthogonality of the small columns);
//   * anything else: the global-memory kernel.
template <class T> SvdList svd_batch_list(const JacobiItem& j, bool with_v, size_t esz) {
    const size_t cap = 160 * 1024 - 2048;
    static const bool force_global = [] { const char* e = std::getenv("TNQS_JACOBI_GLOBAL"); return e && e[0] == '1'; }();
    if (j.n < 1 || j.m < 1) return SvdList::none;
    if (!force_global && jacobi_lds_bytes(j.m, j.n, with_v, esz) <= cap && std::max(j.m, j.n) <= 256) return SvdList::fit;
    // (the tall_* kernels of kernels_chi64.hip walk the rows in blocks: any m up to the 512 rows of a theta -- 260 x 12 is tested)
    if (!force_global && std::is_same<T, float>::value && !with_v && !j.V && use_mfma() && use_chi64() && j.m >= j.n && j.n <= 128 && j.n >= 2 &&
        jacobi_lds_bytes(j.n, j.n, false, esz) <= cap) return SvdList::tall;
    return SvdList::rest;
}
template <class T> void svd_batch(State* s, const std::vector<JacobiItem>& all, bool with_v) {
    const size_t esz = s->esz();
    std::vector<JacobiItem> fit, tall, rest, pre;
    for (auto& j : all) {
        const SvdList l = svd_batch_list<T>(j, with_v, esz);
        if (l == SvdList::none) continue;
        // a low-rank theta the caller offers to the preconditioned kernel (JacobiItem::pre): that kernel takes it when the dimensions found on the device
        // fit; the item stays in the lists below as well, whose kernels skip it in that case
        if (j.pre) pre.push_back(j);
        (l == SvdList::fit ? fit : l == SvdList::tall ? tall : rest).push_back(j);
    }
    if (!pre.empty()) {
        const JacobiItem* d = upload_small(s, pre);
        // LDS for the largest matrix the device may find: the low-rank factor (nhint columns) OR, when that route is withdrawn on the device, theta itself (j.n)
        int mm = 1, nn = 1; for (auto& j : pre) { mm = std::max(mm, std::min(j.m, 128)); nn = std::max(nn, std::min(j.n, 64)); }
        launch_theta_svd_pre(s->stream, d, (int)pre.size(), 60, mm, nn);
    }
    if (!fit.empty()) {
        size_t lds = 0; for (auto& j : fit) lds = std::max(lds, jacobi_lds_bytes(j.m, j.n, with_v, esz));
        const JacobiItem* d = upload_small(s, fit);
        int ncols = 1; for (auto& j : fit) ncols = std::max(ncols, j.nhint > 0 ? j.nhint : j.n);
        launch_jacobi<T>(s->stream, d, (int)fit.size(), 60, lds, mmax_of(fit), ncols);
    }
    if (!rest.empty()) {
        const JacobiItem* d = upload(s, rest);
        launch_jacobi<T>(s->stream, d, (int)rest.size(), 60, 0, mmax_of(rest));
    }
    if (!tall.empty()) svd_tall(s, tall);
}

template <class T, class Acc> void run_grams(State* s, std::vector<GramJob>& jobs, int cls) {
    if (jobs.empty()) return;
    const size_t esz = s->esz();
    size_t KKmax = 1;
    for (auto& j : jobs) { j.KK = (j.keep_site ? j.sd.d : 1) * (j.leg >= 0 ? j.sd.chi[j.leg] : 1); KKmax = std::max<size_t>(KKmax, j.KK); }
    constexpr bool f32 = std::is_same<T, float>::value, acc64 = std::is_same<Acc, double>::value, f32_acc64 = f32 && acc64;
    bool same = true, f64in = true;
    for (auto& j : jobs) { same = same && j.X == j.Y; f64in = f64in && j.M == nullptr && gram_f64in_covers(j.keep_site ? j.sd.d : 1, j.leg >= 0 ? j.sd.chi[j.leg] : 1); }
    const GramRoute r = gram_route(f32, acc64, jobs[0].M != nullptr, same, f64in, KKmax, use_mfma(), use_chi64());      // (kernels.hip, next to gram_tile_rows)
    const bool gauge = r == GramRoute::Gauge32 || r == GramRoute::Gauge64;
    const int TR = gram_tile_rows(r, KKmax, esz);
    std::vector<GramItem> items; double bytes = 0, flops = 0; bool all_full = true;
    for (auto& j : jobs) {
        GramItem it{};
        it.X = j.X; it.Y = j.Y; it.M = j.M;
        if (j.leg >= 0) {
            size_t pre = j.sd.pre(j.leg);
            if (j.keep_site) { it.D = j.sd.d; it.PA = (int)(pre / j.sd.d); } else { it.D = 1; it.PA = (int)pre; }
            it.K = j.sd.chi[j.leg]; it.PB = (int)j.sd.post(j.leg);
        } else { it.D = j.sd.d; it.PA = (int)(j.sd.n / j.sd.d); it.K = 1; it.PB = 1; }
        tile_params(it.PA, it.PB, TR, it.TA, it.TB, it.nta, it.ntb);
        if (r == GramRoute::Gauge32) { it.nta = gauge_gram32_units(j.sd.z, j.sd.chi.data(), j.leg); it.ntb = 1; }      // units of one fiber of r
        items.push_back(it);
        all_full = all_full && j.KK == (r == GramRoute::F64x128 ? 128 : 64);
        bytes += (j.X == j.Y ? 1.0 : 2.0) * j.sd.n * esz; flops += gauge ? 8.0 * j.sd.n * (j.KK + (r == GramRoute::Gauge32 ? 16.0 : 32.0)) : 8.0 * j.sd.n * j.KK * (j.M ? 2.0 : 1.0);
    }
    std::vector<int> npart(jobs.size());
    const int chunks = plan_gram(items.data(), (int)items.size(), r, f32_acc64, 0, npart.data());
    for (size_t q = 0; q < jobs.size(); ++q) {
        GramJob& j = jobs[q];
        j.nchunks = npart[q];
        j.partial = dalloc(s, (size_t)j.nchunks * j.KK * j.KK * 2 * sizeof(Acc));
        items[q].partial = j.partial->p;
    }
    const GramItem* d = upload(s, items);
    ProfScope ps(s, cls, bytes, flops);
    launch_gram_route<T, Acc>(s->stream, r, d, (int)items.size(), chunks, TR, (int)KKmax, all_full);
}

template void run_chains<float>(State*, std::vector<Chain>&, int, int);
template void run_chains<double>(State*, std::vector<Chain>&, int, int);
template SvdList svd_batch_list<float>(const JacobiItem&, bool, size_t);
template SvdList svd_batch_list<double>(const JacobiItem&, bool, size_t);
template void svd_batch<float>(State*, const std::vector<JacobiItem>&, bool);
template void svd_batch<double>(State*, const std::vector<JacobiItem>&, bool);
template void run_grams<float, float>(State*, std::vector<GramJob>&, int);
template void run_grams<float, double>(State*, std::vector<GramJob>&, int);
template void run_grams<double, double>(State*, std::vector<GramJob>&, int);

}  // namespace tnqs
