// engine_runahead.cpp -- deferred verification (engine_internal.hpp): the pending checks of a State and the driver that runs the step schedule of an
// apply_gates call ahead of the device.  All of it runs once or twice per step, never per launch.
#include "engine_internal.hpp"

namespace tnqs {

void settle(State* s, bool block) {
    while (!s->checks.empty()) {
        Check& c = s->checks.front();
        if (block) HIPCHK(hipEventSynchronize(c.ev));
        else { const hipError_t q = hipEventQuery(c.ev); if (q == hipErrorNotReady) return; HIPCHK(q); }
        const bool ok = c.eval(s);
        const SpecFailed f{c.kind, c.step, c.iters_done};
        s->checks.pop_front();
        if (s->checks.empty()) s->arena.ring_off = 0;
        if (!ok) throw f;
    }
}
char* ring_alloc(State* s, size_t bytes) {
    HostArena& ar = s->arena;
    if (!ar.base) ar = acquire_arena();
    const size_t b = round256(std::max<size_t>(bytes, 1));
    if (b > ar.ring_cap) return nullptr;
    if (ar.ring_off + b > ar.ring_cap) { settle(s, true); ar.ring_off = 0; }
    char* p = ar.ring + ar.ring_off; ar.ring_off += b; return p;
}
// the event a new check records behind its staged copy
static hipEvent_t check_event(State* s) {
    HostArena& ar = s->arena;
    if (!ar.base) ar = acquire_arena();
    hipEvent_t& e = ar.cev[ar.cevn++ % kCheckEvents];
    if (!e) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return e;
}
void post_check(State* s, char* stage, const void* dsrc, size_t bytes, int kind, int cur_step, int iters_done, std::function<bool(State*)> eval) {
    HIPCHK(hipMemcpyAsync(stage, dsrc, bytes, hipMemcpyDeviceToHost, s->stream));
    Check c; c.kind = kind; c.step = cur_step; c.iters_done = iters_done; c.ev = check_event(s);
    HIPCHK(hipEventRecord(c.ev, s->stream));
    c.eval = std::move(eval);
    s->checks.push_back(std::move(c));
}
void drop_checks(State* s) { s->checks.clear(); s->arena.ring_off = 0; }

// ---------------------------------------------------------------------------------------------------------------
// the driver
// ---------------------------------------------------------------------------------------------------------------
static size_t site_bytes(const State* s) { size_t n = 0; for (auto& b : s->site) if (b) n += b->bytes; return n; }

// how far ahead?  A sharded handle, one with more than kRunAheadMaxSiteBytes of site tensors and every handle under TNQS_NO_SPECULATION=1 stay one step deep --
// the round-5 flow: a batch reads its results back, an update leaves its verdict pending until the next batch has prepared itself --, and so does, for
// kPenaltySteps steps, a handle on which a verification failed a moment ago (Graph::spec_penalty, shared by the copies of a handle: an evolution whose updates
// need several sweeps would throw away a batch per update otherwise)
RunAhead::RunAhead(State* st, const GateSchedule& sched, BatchFn b, UpdateFn u)
    : s(st), g(*st->g), steps(sched), batch(std::move(b)), update(std::move(u)), in_apply(st),
      deep(speculation_on() && !st->sharded() && site_bytes(st) <= kRunAheadMaxSiteBytes), snaps(sched.size() + 1) {}

void RunAhead::run() {
    try {
        while (k < steps.size() || !s->checks.empty()) {
            try { step(); }
            catch (const SpecFailed& f) { recover(f); }
        }
    } catch (...) { unwind(); throw; }
}

void RunAhead::step() {
    if (k >= steps.size()) { settle(s, true); return; }
    const GateStep& st = steps[k];
    s->cur_step = (int)k;
    const bool was_ahead = ahead();
    snapshot_in_front();
    if (st.is_bp) update(0); else batch(st, was_ahead);
    careful = false; ++k;
    settle_behind(was_ahead);
    drop_old_snaps();
}
void RunAhead::snapshot_in_front() { if (deep || !s->checks.empty()) snaps[k] = std::make_unique<Snapshot>(*s); }
void RunAhead::settle_behind(bool was_ahead) {
    if (g.spec_penalty > 0 && s->checks.empty()) g.spec_penalty -= 1;
    if (!was_ahead && s->checks.size() > 1) settle(s, true);        // one step deep: at most the verdict of the update just enqueued stays pending
    else if (s->checks.size() >= kMaxPendingChecks) settle(s, true);
    else settle(s, false);
}
// only the snapshots from the oldest pending check's step on can still be asked for
void RunAhead::drop_old_snaps() {
    const size_t keep_from = s->checks.empty() ? k : (size_t)std::max(0, s->checks.front().step);
    for (size_t q = 0; q < keep_from && q < snaps.size(); ++q) snaps[q].reset();
}
// the state a failed check goes back to: a gate batch (kind 0) the one in front of its step, a BP update (kind 1) the one right behind its first sweep, which
// is the one in front of the next step.  Null: none was taken (an update that was the last thing enqueued: the state as it stands is the one behind its sweep)
const Snapshot* RunAhead::snapshot_for(const SpecFailed& f) const {
    const size_t at = (size_t)f.step + (f.kind ? 1 : 0);
    return (f.step >= 0 && at < snaps.size()) ? snaps[at].get() : nullptr;
}
// after SpecFailed: nothing enqueued behind the failed step may leave a trace -- drain, drop the younger checks, put the state back
void RunAhead::recover(const SpecFailed& f) {
    HIPCHK(hipStreamSynchronize(s->stream)); if (s->aux_stream) HIPCHK(hipStreamSynchronize(s->aux_stream));
    drained(s); drop_checks(s);
    const auto redone = s->stats.n_spec_redone;      // (the snapshot carries the statistics of its moment)
    g.spec_penalty = kPenaltySteps;
    const Snapshot* snap = snapshot_for(f);
    if (f.kind == 0) {                          // a gate batch: back to the state in front of it, run it the careful way
        if (!snap) throw std::logic_error("apply_gates: no snapshot in front of a batch whose deferred verification failed");
        snap->restore(*s);
        k = (size_t)f.step; careful = true;
    } else {                                    // a BP update whose first sweep missed the tolerance: the state right behind that sweep, then the remaining sweeps
        if (snap) snap->restore(*s);
        s->cur_step = f.step;
        update(f.iters_done);
        k = (size_t)f.step + 1; careful = false;
    }
    s->stats.n_spec_redone = redone + 1;
    for (size_t q = k + 1; q < snaps.size(); ++q) snaps[q].reset();
}
// an error of a step: what is still unverified is settled -- or rolled back to the last verified state -- before the handle is handed back; the first error wins
void RunAhead::unwind() {
    try { settle(s, true); }
    catch (const SpecFailed& f) { (void)hipStreamSynchronize(s->stream); drop_checks(s); if (const Snapshot* snap = snapshot_for(f)) snap->restore(*s); }
    catch (...) { drop_checks(s); }
}

}  // namespace tnqs
