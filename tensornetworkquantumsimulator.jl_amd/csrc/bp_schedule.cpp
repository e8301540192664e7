// bp_schedule.cpp -- the order of a BP sweep and its level schedule (host graph code, no device call): the default sequence of a graph, the reference's
// forest-cover sequence, the dependency levels of a sequence, and the BPPlan the update (engine_bp.cpp) walks.
#include "engine.hpp"
#include <algorithm>
#include <climits>
#include <functional>
#include <numeric>

namespace tnqs {

// Default sweep order (the reference's default is NamedGraphs' forest-cover sequence, not available here; any sequence gives the
// same fixed point, abstractbeliefpropagationcache.jl:204-218).  The edges are decomposed into LINEAR FORESTS (disjoint simple paths);
// inside a forest the messages are ordered so that every message is computed from the OLD values of the other messages of the same
// forest: along a path v0..vk the hops v_i -> v_{i+1} are listed last hop first, the hops v_{i+1} -> v_i first hop first (a message
// u -> w depends on the message entering u through its other path edge, which therefore must come LATER in the sequence).  Level
// scheduling then puts a whole forest into one level: 2 levels per sweep on a square lattice (rows, columns), and both outgoing
// messages of a site inside a forest share one pair product.  It is an ordinary sequential Gauss-Seidel order.
// On periodic lattices the paths close: there the edge sets may contain cycles (path_cycle_sequence, default_sequence below) -- still a sequential order.
struct DSU { std::vector<int> p; explicit DSU(int n) : p(n) { std::iota(p.begin(), p.end(), 0); } int f(int x) { while (p[x] != x) x = p[x] = p[p[x]]; return x; }
             bool join(int a, int b) { a = f(a); b = f(b); if (a == b) return false; p[a] = b; return true; } };
// Forests: the reference's own default order (NamedGraphs forest_cover_edge_sequence: per component, post-order DFS edges towards the
// root, then their reverses in reverse order).  With it ONE sweep is exact on a tree -- which is what the reference's tree defaults
// (maxiter = 1, no tolerance; beliefpropagationcache.jl:39,110-113) rely on.  The linear-forest order below lists every message BEFORE
// the one it depends on (so that a forest is one level), i.e. information moves one hop per sweep: right for loopy graphs, where the
// fixed point is iterated anyway, wrong for the single sweep of a tree.
static std::vector<int> tree_sequence(const Graph& g) {
    std::vector<int> seq; std::vector<char> seen(g.nv, 0);
    for (int root = 0; root < g.nv; ++root) {
        if (seen[root] || g.nbr[root].empty()) continue;
        std::vector<std::pair<int, int>> post;                          // (child, parent)
        std::vector<std::pair<int, size_t>> stack{{root, 0}}; std::vector<int> par(1, -1);
        seen[root] = 1;
        while (!stack.empty()) {
            auto& top = stack.back(); const int x = top.first;
            bool pushed = false;
            while (top.second < g.nbr[x].size()) {
                const int y = g.nbr[x][top.second++];
                if (seen[y]) continue;
                seen[y] = 1; stack.push_back({y, 0}); par.push_back(x); pushed = true; break;
            }
            if (pushed) continue;
            if (par.back() >= 0) post.push_back({x, par.back()});
            stack.pop_back(); par.pop_back();
        }
        for (auto& e : post) seq.push_back(g.dedge(e.first, e.second));
        for (auto it = post.rbegin(); it != post.rend(); ++it) seq.push_back(g.dedge(it->second, it->first));
    }
    return seq;
}
// The reference's default order on ANY graph (beliefpropagationcache.jl:28: NamedGraphs forest_cover_edge_sequence, restated -- NamedGraphs is not part of
// the reference package; julia/replay_golden.jl checks the restatement against NamedGraphs' own): the edges are covered greedily by spanning forests
// (breadth-first from the first vertex that still has an uncovered edge, neighbours in ascending vertex id); per tree the edges towards the root in
// depth-first post-order, then their reverses in reverse order.  Selected with tnqs_bp_opts.n_sequence = -1; the same sequence as the host's
// graphs.py forest_cover_edge_sequence passed explicitly.
static std::vector<int> forest_cover_sequence(const Graph& g) {
    std::vector<char> remaining(g.ne, 1); int left = g.ne;
    std::vector<int> seq;
    while (left > 0) {
        std::vector<char> visited(g.nv, 0), used(g.ne, 0);
        for (int root = 0; root < g.nv; ++root) {
            if (visited[root]) continue;
            bool any = false; for (int e : g.nbr_e[root]) any = any || remaining[e];
            if (!any) continue;
            std::vector<std::vector<int>> children(g.nv);
            std::vector<int> queue{root}; visited[root] = 1;
            for (size_t qi = 0; qi < queue.size(); ++qi) {
                const int x = queue[qi];
                for (size_t j = 0; j < g.nbr[x].size(); ++j) {
                    const int y = g.nbr[x][j], e = g.nbr_e[x][j];
                    if (visited[y] || !remaining[e]) continue;
                    visited[y] = 1; children[x].push_back(y); used[e] = 1; queue.push_back(y);
                }
            }
            std::vector<std::pair<int, int>> post;                      // (child, parent)
            std::vector<std::pair<int, size_t>> stack{{root, 0}};
            while (!stack.empty()) {
                auto& top = stack.back();
                if (top.second < children[top.first].size()) { const int c = children[top.first][top.second++]; stack.push_back({c, 0}); }
                else { const int x = top.first; stack.pop_back(); if (!stack.empty()) post.push_back({x, stack.back().first}); }
            }
            for (auto& e : post) seq.push_back(g.dedge(e.first, e.second));
            for (auto it = post.rbegin(); it != post.rend(); ++it) seq.push_back(g.dedge(it->second, it->first));
        }
        for (int e = 0; e < g.ne; ++e) if (used[e]) { remaining[e] = 0; --left; }
    }
    return seq;
}
// dependency level of every position of a sequence: one more than the highest level among the EARLIER positions whose message enters the source
// (a later position is read in its old value); a level's messages are independent of each other
// `starts` (optional, ascending positions): the levels of the positions from a start on lie above everything before it (later is always allowed: which
// value a message reads is decided by the positions, not by the levels) -- a site then never meets messages of two sets in one level
static std::vector<int> sequence_levels(const Graph& g, const std::vector<int>& seq, const std::vector<int>& pos_of, const std::vector<int>* starts = nullptr) {
    std::vector<int> level(seq.size(), 0);
    int floor_lv = 0, top = -1; size_t ks = 0;
    for (size_t t = 0; t < seq.size(); ++t) {
        if (starts) while (ks < starts->size() && (*starts)[ks] == (int)t) { floor_lv = top + 1; ++ks; }
        const int src = g.src_of(seq[t]), dst = g.dst_of(seq[t]);
        int lv = 0;
        for (size_t j = 0; j < g.nbr[src].size(); ++j) {
            int k = g.nbr[src][j]; if (k == dst) continue;
            int pp = pos_of[g.dedge(k, src)];
            if (pp >= 0 && pp < (int)t) lv = std::max(lv, level[pp] + 1);
        }
        lv = std::max(lv, floor_lv);
        level[t] = lv; top = std::max(top, lv);
    }
    return level;
}
// The messages of edge sets of maximum degree 2 (`part[e]` = set of edge e), set after set.  Along a path v0..vk the hops v_i -> v_{i+1} are listed
// last hop first and the hops v_{i+1} -> v_i first hop first: every message is computed from the OLD values of its own set, the whole path is one
// level and an inner site sends both its messages in it.  Round a cycle v0..v_{n-1} the same holds for all hops but the two that leave v0, which
// come last (one of the messages a cycle carries must see a new value in any sequential order): v1..v_{n-1} send both their messages in one level,
// v0 both of its own in the next -- n two-message passes per cycle, where a path plus its closing edge in another forest takes n + 2 passes.
static std::vector<int> path_cycle_sequence(const Graph& g, const std::vector<int>& part, int np, std::vector<int>& starts) {
    std::vector<int> seq; starts.clear();
    for (int f = 0; f < np; ++f) {
        starts.push_back((int)seq.size());
        std::vector<std::vector<int>> adj(g.nv);
        for (int e = 0; e < g.ne; ++e) if (part[e] == f) { adj[g.esrc[e]].push_back(g.edst[e]); adj[g.edst[e]].push_back(g.esrc[e]); }
        std::vector<char> seen(g.nv, 0);
        for (int v = 0; v < g.nv; ++v) {
            if (adj[v].size() != 1 || seen[v]) continue;                   // start at a path end
            std::vector<int> path{v}; seen[v] = 1; int prev = -1, cur = v;
            for (;;) { int nxt = -1; for (int w : adj[cur]) if (w != prev) nxt = w; if (nxt < 0) break; prev = cur; cur = nxt; path.push_back(cur); seen[cur] = 1; }
            const int k = (int)path.size() - 1;
            for (int i = k - 1; i >= 0; --i) seq.push_back(g.dedge(path[i], path[i + 1]));
            for (int i = 0; i < k; ++i) seq.push_back(g.dedge(path[i + 1], path[i]));
        }
        for (int v = 0; v < g.nv; ++v) {
            if (adj[v].size() != 2 || seen[v]) continue;                   // what is left has no end: cycles
            std::vector<int> cyc{v}; seen[v] = 1; int prev = -1, cur = v;
            for (;;) { int nxt = (adj[cur][0] != prev) ? adj[cur][0] : adj[cur][1]; if (nxt == v) break; prev = cur; cur = nxt; cyc.push_back(cur); seen[cur] = 1; }
            const int n = (int)cyc.size();
            for (int i = n - 1; i >= 1; --i) seq.push_back(g.dedge(cyc[i], cyc[(i + 1) % n]));
            for (int i = 0; i + 1 < n; ++i) seq.push_back(g.dedge(cyc[i + 1], cyc[i]));
            seq.push_back(g.dedge(cyc[0], cyc[1])); seq.push_back(g.dedge(cyc[0], cyc[n - 1]));
        }
    }
    return seq;
}
// edge sets of maximum degree 2; with_cycles = false: linear forests (no cycle closes inside a set)
static void degree2_sets(const Graph& g, bool with_cycles, std::vector<int>& part, int& np) {
    part.assign(g.ne, -1); np = 0;
    // 1. unions of two colour classes (straight lines on lattices): pair the colours up; a union is a set of paths and even cycles
    std::vector<std::vector<char>> ok(g.ncolors, std::vector<char>(g.ncolors, 0));
    for (int a = 0; a < g.ncolors; ++a) for (int b = a + 1; b < g.ncolors; ++b) {
        bool acyclic = true;
        if (!with_cycles) { DSU d(g.nv); for (int e = 0; e < g.ne && acyclic; ++e) if (g.ecolor[e] == a || g.ecolor[e] == b) acyclic = d.join(g.esrc[e], g.edst[e]); }
        ok[a][b] = ok[b][a] = acyclic ? 1 : 0;
    }
    std::vector<int> mate(g.ncolors, -1), best;
    int best_pairs = -1;
    std::function<void(int, int)> rec = [&](int c, int pairs) {          // maximum matching of the colours (few colours: brute force)
        while (c < g.ncolors && mate[c] >= 0) ++c;
        if (c >= g.ncolors) { if (pairs > best_pairs) { best_pairs = pairs; best = mate; } return; }
        mate[c] = c; rec(c + 1, pairs); mate[c] = -1;                     // leave c single
        for (int b = c + 1; b < g.ncolors; ++b) if (mate[b] < 0 && ok[c][b]) { mate[c] = b; mate[b] = c; rec(c + 1, pairs + 1); mate[c] = mate[b] = -1; }
    };
    if (g.ncolors <= 10) rec(0, 0);
    // 2. greedy: an edge joins the first set where both ends still have degree < 2 (and, for forests, no cycle closes)
    std::vector<int> gpart(g.ne, -1); int gnp = 0;
    {
        std::vector<std::vector<int>> deg; std::vector<DSU> comp;
        for (int e = 0; e < g.ne; ++e) {
            int a = g.esrc[e], b = g.edst[e], f = 0;
            for (;; ++f) {
                if (f == gnp) { deg.emplace_back(g.nv, 0); comp.emplace_back(g.nv); ++gnp; }
                if (deg[f][a] < 2 && deg[f][b] < 2 && (with_cycles || comp[f].f(a) != comp[f].f(b))) break;
            }
            comp[f].join(a, b); ++deg[f][a]; ++deg[f][b]; gpart[e] = f;
        }
    }
    // the decomposition with fewer sets wins; ties go to the colour pairs
    if (best_pairs > 0 && g.ncolors - best_pairs <= gnp) {
        std::vector<int> fof(g.ncolors, -1);
        for (int c = 0; c < g.ncolors; ++c) if (fof[c] < 0) { fof[c] = np; if (best[c] != c && best[c] >= 0) fof[best[c]] = np; ++np; }
        for (int e = 0; e < g.ne; ++e) part[e] = fof[g.ecolor[e]];
    } else { part = gpart; np = gnp; }
}
static std::vector<int> default_sequence(const Graph& g, std::vector<int>& set_starts) {
    set_starts.clear();
    if (g.is_tree) {
        std::vector<int> seq = tree_sequence(g);
        if ((int)seq.size() != 2 * g.ne) throw Err(TNQS_ERR_HIP, "internal: tree sequence does not cover every message");
        return seq;
    }
    // linear forests (a forest is one level), or -- where it saves at least a twentieth of the (site, level) passes over the site tensors, i.e. on periodic
    // lattices -- sets that may close cycles (two levels per set, see path_cycle_sequence).  A pass is what a sweep costs on big tensors; the levels are
    // what it costs on small ones, and there the forests have fewer
    std::vector<int> best_seq; long best_passes = -1;
    const int nvariants = 2;
    for (int with_cycles = 0; with_cycles < nvariants; ++with_cycles) {
        std::vector<int> part; int np = 0;
        degree2_sets(g, with_cycles != 0, part, np);
        std::vector<int> starts;
        std::vector<int> seq = path_cycle_sequence(g, part, np, starts);
        if ((int)seq.size() != 2 * g.ne) throw Err(TNQS_ERR_HIP, "internal: default sequence does not cover every message");
        std::vector<int> pos_of(2 * (size_t)g.ne, -1);
        for (size_t t = 0; t < seq.size(); ++t) pos_of[seq[t]] = (int)t;
        if (!with_cycles) starts.clear();                                 // forests: plain dependency levels, as ever
        const std::vector<int> level = sequence_levels(g, seq, pos_of, starts.empty() ? nullptr : &starts);
        std::vector<std::pair<int, int>> sl;
        for (size_t t = 0; t < seq.size(); ++t) sl.push_back({g.src_of(seq[t]), level[t]});
        std::sort(sl.begin(), sl.end()); sl.erase(std::unique(sl.begin(), sl.end()), sl.end());
        const long passes = (long)sl.size();
        if (best_passes < 0 || passes * 20 <= best_passes * 19) { best_seq = std::move(seq); best_passes = passes; set_starts = starts; }
    }
    return best_seq;
}
static const std::vector<int>& default_seq_of(const Graph& g) {           // built on first use, kept with the graph
    if (g.default_seq.empty() && g.ne > 0) g.default_seq = default_sequence(g, g.default_set_starts);
    return g.default_seq;
}

static BPPlan make_plan(const Graph& g, const tnqs_bp_opts* o) {
    BPPlan p;
    if (o && o->n_sequence > 0) {
        for (int i = 0; i < o->n_sequence; ++i) {
            int de = g.dedge(o->seq_src[i], o->seq_dst[i]);
            if (de < 0) throw Err(TNQS_ERR_INVALID, "bp_update: edge_sequence contains a pair of non-adjacent vertices");
            p.seq.push_back(de);
        }
    } else if (o && o->n_sequence < 0) p.seq = forest_cover_sequence(g);      // the reference's own default order
    else p.seq = default_seq_of(g);
    p.pos_of.assign(2 * (size_t)g.ne, -1);
    for (size_t t = 0; t < p.seq.size(); ++t) { if (p.pos_of[p.seq[t]] >= 0) p.in_place = true; p.pos_of[p.seq[t]] = (int)t; }
    if (p.in_place) { for (size_t t = 0; t < p.seq.size(); ++t) { p.levels.push_back({(int)t}); p.level_of.push_back((int)t); } }
    else {
        const bool is_default = !(o && o->n_sequence != 0);
        p.level_of = sequence_levels(g, p.seq, p.pos_of, is_default && !g.default_set_starts.empty() ? &g.default_set_starts : nullptr);
        int nlev = 0;
        for (int lv : p.level_of) nlev = std::max(nlev, lv + 1);
        p.levels.resize(nlev);
        for (size_t t = 0; t < p.seq.size(); ++t) p.levels[p.level_of[t]].push_back((int)t);
        // the messages of a level are independent of each other: list them by source vertex, so that a workspace-bounded sub-batch (engine_bp.cpp BpLevelBatch)
        // holds all messages of the sites it touches (they share the pair product and the double pair-Gram pass)
        for (auto& lev : p.levels) std::stable_sort(lev.begin(), lev.end(), [&](int a, int b) { return g.src_of(p.seq[a]) < g.src_of(p.seq[b]); });
    }
    p.nlev = (int)p.levels.size();
    p.out_level.resize(g.nv); p.in_level.resize(g.nv);
    for (int v = 0; v < g.nv; ++v) for (size_t j = 0; j < g.nbr[v].size(); ++j) {
        const int po = p.pos_of[g.dedge(v, g.nbr[v][j])], pi = p.pos_of[g.dedge(g.nbr[v][j], v)];
        p.out_level[v].push_back(po >= 0 ? p.level_of[po] : -1); p.in_level[v].push_back(pi >= 0 ? p.level_of[pi] : -1);
    }
    return p;
}

// The level schedule depends on the graph and the sequence only: the ones of the default order and of the reference's forest-cover order (n_sequence = -1) are
// kept with the graph, the one of an explicit sequence is built per call.
std::shared_ptr<const BPPlan> plan_for(const Graph& g, const tnqs_bp_opts* o) {
    if (o && o->n_sequence > 0) return std::make_shared<const BPPlan>(make_plan(g, o));
    std::shared_ptr<const BPPlan>& kept = (o && o->n_sequence < 0) ? g.forest_plan : g.default_plan;
    if (!kept) kept = std::make_shared<const BPPlan>(make_plan(g, o));
    return kept;
}

// the default order as (src, dst) vertex pairs, for tests that replay it on the oracle (include/tnqs_debug.h)
void dbg_default_sequence(const Graph& g, std::vector<int>& src, std::vector<int>& dst) {
    for (int de : default_seq_of(g)) { src.push_back(g.src_of(de)); dst.push_back(g.dst_of(de)); }
}

// the same with the dependency levels bp_update schedules the order in (host only, no device: tests/test_bp_schedule.py)
void dbg_default_sequence_graph(const Graph& g, std::vector<int>& src, std::vector<int>& dst, std::vector<int>& level) {
    dbg_default_sequence(g, src, dst);
    level = plan_for(g, nullptr)->level_of;
}

}  // namespace tnqs
