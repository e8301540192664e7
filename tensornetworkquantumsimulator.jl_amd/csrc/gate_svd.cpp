// gate_svd.cpp -- the SVD stage of a two-site gate batch (simple_update.jl:53-59): the JacobiItem of every gate, svd_batch, and the recovery of V from the unrotated
// theta.  engine_gates.cpp (TwoSiteBatch::svd_and_finish) and the kernel-level entry point of debug_gate.cpp (tnqs_dbg_theta_svd_stage) both run THIS code.
#include "engine_internal.hpp"

namespace tnqs {

// the item svd_batch gets for one gate, and the column count of its full theta (the rows of the recovered V)
static JacobiItem theta_svd_item(bool F32, const ThetaSvdGate& g, const int* dims, int& ncfull) {
    JacobiItem j{};
    if (dims) {
        int Mr, Nc, ncolJ; theta_dims(dims, g.d1, g.d2, Mr, Nc, ncolJ);
        j = JacobiItem{g.theta, g.thetaV, Mr, ncolJ, g.info + 4};
        ncfull = Nc;
    } else {
        const int Mr = std::max(g.n1 * g.d1, g.n2 * g.d2), Nc = std::min(g.n1 * g.d1, g.n2 * g.d2);
        j = JacobiItem{g.theta, g.thetaV, Mr, Nc, g.info + 4, g.info, g.d1, g.d2, g.K};      // low-rank route expected: K columns
        // offered to theta_svd_pre_kernel, which decides on the device: the low-rank factor with its Q (2), or theta as it stands when the ranks the
        // sites CAN have (a site with fewer fibers than columns: a corner) keep it within 128 x 64 (1) -- those gates took 12-13 plain sweeps on 128 rows
        // and were what a colour batch of a small lattice waited for
        if (F32 && use_precond_svd()) {
            if (g.lowQ) { j.QB = g.lowQ; j.Vout = g.thetaV; j.pre = 2; }
            else if (theta_svd_pre_covers(std::max(g.a1, g.a2), std::min(g.a1, g.a2))) { j.Vout = g.thetaV; j.pre = 1; }
            j.cap = g.cap;
        }
        ncfull = Nc;
    }
    j.V = nullptr;          // V is never accumulated from the rotations: recovered below
    return j;
}

template <class T> void launch_theta_svd_stage(State* s, const std::vector<ThetaSvdGate>& gates, const int* dims, bool recover_mfma) {
    constexpr bool F32 = std::is_same<T, float>::value;
    const int npg = (int)gates.size();
    std::vector<JacobiItem> ji; std::vector<int> ncfull;
    for (int q = 0; q < npg; ++q) { int nc = 0; ji.push_back(theta_svd_item(F32, gates[q], dims ? dims + 8 * q : nullptr, nc)); ncfull.push_back(nc); }
    { ProfScope ps(s, TNQS_PROF_JACOBI, 0, 0); svd_batch<T>(s, ji, false); }
    std::vector<RecoverItem> rv;
    for (int q = 0; q < npg; ++q) rv.push_back(RecoverItem{gates[q].theta0, gates[q].theta, gates[q].thetaV, ji[q].m, ncfull[q], ji[q].n, ji[q].dyn, ji[q].dm, ji[q].dn, ji[q].pre});
    const RecoverItem* dr = upload_small(s, rv);
    { ProfScope ps(s, TNQS_PROF_JACOBI, 0, 0); { int nmax = 1; for (int nc : ncfull) nmax = std::max(nmax, nc); if (recover_mfma) launch_recover_v_mfma(s->stream, dr, npg, nmax); else launch_recover_v<T>(s->stream, dr, npg, nmax); } }
}
template void launch_theta_svd_stage<float>(State*, const std::vector<ThetaSvdGate>&, const int*, bool);
template void launch_theta_svd_stage<double>(State*, const std::vector<ThetaSvdGate>&, const int*, bool);

int theta_svd_route(bool F32, const ThetaSvdGate& g, const int* dims, const int* info) {
    int nc = 0; const JacobiItem j = theta_svd_item(F32, g, dims, nc);
    if (j.pre && theta_pre_takes(info, g.d1, g.d2, j.QB != nullptr)) return info[7] > 0 ? ThetaSvdPreLow : ThetaSvdPreTheta;
    const SvdList l = F32 ? svd_batch_list<float>(j, false, 8) : svd_batch_list<double>(j, false, 16);
    return l == SvdList::fit ? ThetaSvdLds : l == SvdList::tall ? ThetaSvdTall : l == SvdList::rest ? ThetaSvdGlobal : ThetaSvdNone;
}

}  // namespace tnqs
