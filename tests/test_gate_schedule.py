"""Host-side logic of apply_gates (no GPU): the walk over the gate list -- which gates form a batch, where a BP update is due -- read through the host-only
entry point tnqs_dbg_gate_schedule (include/tnqs_debug.h; csrc/gate_schedule.cpp build_gate_schedule).  Where the updates fall is the reference's rule
(apply_gates.jl:64-95), restated here after the oracle's walk (oracle/tnqs_oracle.py apply_gates); the batches are the maximal runs of pairwise vertex-disjoint
gates between them, in list order."""
import ctypes as C

import numpy as np
import pytest

import tnqs_amd as tn

I32P = C.POINTER(C.c_int32)
IP = C.POINTER(C.c_int)


def gate_schedule(g, circuit, update_cache=True):
    """circuit: one list of vertices per gate.  Returns the steps in order: "bp" for an update, the list of gate indices for a batch."""
    lib = C.CDLL(tn.LIB_PATH)
    fn = lib.tnqs_dbg_gate_schedule
    fn.argtypes = [C.c_int, C.c_int, I32P, I32P, C.c_int, I32P, I32P, C.c_int, IP, IP, C.c_int, IP]
    fn.restype = C.c_int
    idx = {v: i for i, v in enumerate(g.vertices)}
    es = np.array([idx[a] for (a, b) in g.edges], dtype=np.int32); ed = np.array([idx[b] for (a, b) in g.edges], dtype=np.int32)
    nverts = np.array([len(vs) for vs in circuit], dtype=np.int32)
    verts = np.array([idx[v] for vs in circuit for v in vs], dtype=np.int32)
    n = len(circuit); cap = 2 * n + 2
    step_of_gate = (C.c_int * max(1, n))(); is_bp = (C.c_int * cap)(); nsteps = C.c_int(-1)
    rc = fn(g.nv(), g.ne(), es.ctypes.data_as(I32P), ed.ctypes.data_as(I32P), n, nverts.ctypes.data_as(I32P), verts.ctypes.data_as(I32P),
            1 if update_cache else 0, step_of_gate, is_bp, cap, C.byref(nsteps))
    assert rc == 0 and 0 <= nsteps.value <= cap
    steps = ["bp" if is_bp[k] else [] for k in range(nsteps.value)]
    for i in range(n):
        assert 0 <= step_of_gate[i] < nsteps.value and not is_bp[step_of_gate[i]], (i, step_of_gate[i])     # every gate in exactly one batch step
        steps[step_of_gate[i]].append(i)
    return steps


def update_positions(circuit, update_cache):
    """the oracle's walk: the gate indices in front of which an update falls (len(circuit): the one at the end)"""
    at = []; affected = set()
    for i, verts in enumerate(circuit):
        need = len(verts) >= 2 and any(v in affected for v in verts)               # apply_gates.jl:68
        if update_cache and need:
            at.append(i)                                                           # :76
            affected.clear()                                                       # :78
        affected.update(verts)                                                     # :88-90
    if update_cache:
        at.append(len(circuit))                                                    # :93-95
    return at


def restated(circuit, update_cache):
    """updates where the oracle's walk has them, maximal runs of pairwise-disjoint gates between them"""
    ups = update_positions(circuit, update_cache)
    steps = []; run = []; used = set()
    for i, verts in enumerate(circuit):
        if i in ups or any(v in used for v in verts):
            if run:
                steps.append(run)
            run = []; used = set()
        if i in ups:
            steps.append("bp")
        run.append(i); used.update(verts)
    if run:
        steps.append(run)
    return steps + (["bp"] if len(circuit) in ups else [])


def check(g, circuit, update_cache=True):
    steps = gate_schedule(g, circuit, update_cache)
    batches = [s for s in steps if s != "bp"]
    assert all(len(b) > 0 for b in batches)
    assert [i for b in batches for i in b] == list(range(len(circuit)))            # order preserved, nothing twice, nothing missing
    for b in batches:                                                               # the gates of a step are pairwise vertex-disjoint
        seen = [v for i in b for v in circuit[i]]
        assert len(seen) == len(set(seen)), b
    for prev, cur in zip(steps, steps[1:]):                                         # maximality: a batch directly behind a batch starts with a gate that overlaps it
        if prev != "bp" and cur != "bp":
            assert set(circuit[cur[0]]) & {v for i in prev for v in circuit[i]}, (prev, cur)
    gates_in_front = [sum(len(s) for s in steps[:k] if s != "bp") for k, s in enumerate(steps) if s == "bp"]
    assert gates_in_front == update_positions(circuit, update_cache)              # BP positions
    assert steps == restated(circuit, update_cache)
    return steps


def counts(steps):
    return sum(s == "bp" for s in steps), sum(s != "bp" for s in steps)


def tfim_layer(g):
    layer = [[v] for v in g.vertices]
    for grp in tn.edge_color(g, 4):
        layer += [[a, b] for (a, b) in grp]
    return layer


def test_the_circuits_of_the_scheduling_rule_counts():
    """tests/test_gpu_parity.py::test_scheduling_rule_counts asserts these (updates, batches) on the device"""
    g = tn.named_grid((3, 3))
    assert counts(check(g, [[(1, 1), (2, 1)], [(1, 2), (2, 2)]])) == (1, 1)
    assert counts(check(g, [[(1, 1), (2, 1)], [(2, 1), (3, 1)]])) == (2, 2)
    assert counts(check(g, [[(1, 1)], [(1, 1)], [(1, 1), (2, 1)]])) == (2, 3)
    assert counts(check(g, [[(1, 1)]], update_cache=False)) == (0, 1)


def test_tfim_layer_on_3x3():
    g = tn.named_grid((3, 3))
    layer = tfim_layer(g)
    steps = check(g, layer)
    # the one-site gates poison every vertex: one batch, then an update in front of the first two-site gate
    assert steps[0] == list(range(9)) and steps[1] == "bp" and steps[2][0] == 9 and steps[-1] == "bp"
    off = check(g, layer, update_cache=False)
    assert "bp" not in off and off[0] == list(range(9))                            # no BP step at all


def test_empty_list():
    g = tn.named_grid((3, 3))
    assert check(g, []) == ["bp"]
    assert check(g, [], update_cache=False) == []


def test_one_site_gates_only():
    g = tn.named_grid((3, 3))
    vs = list(g.vertices)
    circuit = [[v] for v in vs] + [[vs[0]], [vs[1]], [vs[0]]]
    steps = check(g, circuit)
    assert steps == [list(range(9)), [9, 10], [11], "bp"]                           # a batch per overlap run, no update in front of any, one at the end


def test_one_site_gate_on_an_affected_vertex_then_a_disjoint_two_site_gate():
    g = tn.named_grid((3, 3))
    steps = check(g, [[(1, 1)], [(1, 1)], [(2, 2), (2, 3)]])
    assert steps == [[0], [1, 2], "bp"]                                             # no update: only the one at the end


@pytest.mark.parametrize("name", ["grid4x4", "ring7"])
def test_random_circuits(name):
    g = tn.named_grid((4, 4)) if name == "grid4x4" else tn.named_grid((7,), periodic=True)
    vs = list(g.vertices); es = list(g.edges)
    rng = np.random.default_rng(20240 + len(vs))
    for _ in range(50):
        circuit = []
        for _ in range(int(rng.integers(180, 221))):
            if rng.random() < 0.4:
                circuit.append([vs[int(rng.integers(len(vs)))]])
            else:
                a, b = es[int(rng.integers(len(es)))]
                circuit.append([a, b] if rng.random() < 0.5 else [b, a])
        steps = check(g, circuit, update_cache=bool(rng.random() < 0.8))
        assert len(steps) > 2
