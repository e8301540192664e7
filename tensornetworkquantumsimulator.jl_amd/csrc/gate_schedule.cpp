// gate_schedule.cpp -- the walk over the gate list of apply_gates (src/Apply/apply_gates.jl:46-98; host code, no device call): validation of the list and
// the GateSchedule the run-ahead driver (engine_runahead.cpp) executes.
#include "engine.hpp"

namespace tnqs {

// validation first (apply_gates.jl:109-120): nothing is mutated when an argument is bad.  voff / moff: where the vertices / the matrix of gate i start
void validate_gates(const State& s, int ngates, const int32_t* nverts, const int32_t* verts, std::vector<int>& voff, std::vector<size_t>& moff) {
    const Graph& g = *s.g;
    voff.assign(ngates + 1, 0); moff.assign(ngates + 1, 0);
    for (int i = 0; i < ngates; ++i) {
        int nv = nverts[i];
        if (nv < 1 || nv > 2) throw Err(TNQS_ERR_INVALID, "apply_gate!: only one- and two-site gates are supported; received a gate acting on " + std::to_string(nv) + " vertices.");
        voff[i + 1] = voff[i] + nv;
        size_t dd = 1;
        for (int k = 0; k < nv; ++k) { int v = verts[voff[i] + k]; if (v < 0 || v >= g.nv) throw Err(TNQS_ERR_INVALID, "apply_gates: vertex out of range");
                                       if (s.projected[v]) throw Err(TNQS_ERR_INVALID, "apply_gates: vertex " + std::to_string(v) + " was projected onto a configuration (tnqs_project_site: its site dimension is 1); gates cannot act on it");
                                       dd *= s.d[v]; }
        moff[i + 1] = moff[i] + 2 * dd * dd;
        if (nv == 2) {
            int a = verts[voff[i]], b = verts[voff[i] + 1];
            if (a == b || g.edge(a, b) < 0)
                throw Err(TNQS_ERR_INVALID, "apply_gate!: cannot apply a two-site gate on the non-adjacent vertices " + std::to_string(a) + " and " + std::to_string(b) +
                                                ". Simple update requires the two sites to share an edge of the tensor-network graph.");
        }
    }
}

// a vertex set as flags instead of std::set: this walk sits in front of the first kernel of a call
struct VSet { std::vector<char> f; std::vector<int> l; explicit VSet(int n) : f(n, 0) {} bool count(int v) const { return f[v] != 0; }
              void insert(int v) { if (!f[v]) { f[v] = 1; l.push_back(v); } } void clear() { for (int v : l) f[v] = 0; l.clear(); } };

// The walk -- which gates form a batch, where a BP update is due -- depends on the vertex lists alone (apply_gates.jl:64-90: vertex sets), not on any number
// computed on the way.  So the SCHEDULE is built first: steps = maximal runs of pairwise-disjoint gates ("batch") and the cache updates between them ("bp"), in
// the reference's order.  A batch is a run of the list, so a step names its gates as the range [begin, end) of the caller's list.
GateSchedule build_gate_schedule(const Graph& g, int ngates, const int32_t* nverts, const int32_t* verts, bool update_cache) {
    GateSchedule steps;
    VSet affected(g.nv), batch_verts(g.nv);
    int begin = 0;
    auto flush = [&](int end) { if (end > begin) steps.push_back(GateStep{false, begin, end}); begin = end; batch_verts.clear(); };
    const int32_t* vs = verts;
    for (int i = 0; i < ngates; vs += nverts[i], ++i) {
        const int nv = nverts[i];
        bool need = false;
        if (nv >= 2) for (int k = 0; k < nv; ++k) need = need || affected.count(vs[k]);            // apply_gates.jl:68
        if (update_cache && need) {
            flush(i);
            steps.push_back(GateStep{true, i, i});                                                 // :76
            affected.clear();                                                                      // :78
        }
        bool overlap = false;
        for (int k = 0; k < nv; ++k) overlap = overlap || batch_verts.count(vs[k]);
        if (overlap) flush(i);
        for (int k = 0; k < nv; ++k) { batch_verts.insert(vs[k]); affected.insert(vs[k]); }         // :88-90
    }
    flush(ngates);
    if (update_cache) steps.push_back(GateStep{true, ngates, ngates});                             // :93-95
    return steps;
}

}  // namespace tnqs
