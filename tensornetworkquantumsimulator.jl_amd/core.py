"""Host-side mirror of the reference's operator interface for the BP-gauged gate-application path.

Same names, argument meaning and error behaviour as TensorNetworkQuantumSimulator.jl (paths relative to the
reference repo):
  TensorNetworkState / tensornetworkstate / random_tensornetworkstate   src/TensorNetworks/tensornetworkstate.jl:12-15,93-103,141-161
  BeliefPropagationCache, copy, message, network                         src/MessagePassing/beliefpropagationcache.jl:9-37
  update(bpc; maxiter, tolerance, edge_sequence, ...)                     src/MessagePassing/abstractbeliefpropagationcache.jl:223-259
  apply_gates / apply_circuit                                            src/Apply/apply_gates.jl:17-98,145
  truncate(bpc; maxdim, cutoff, edge_color, normalize_tensors)           src/truncate.jl:12-38
  expect(bpc, (op, [v]))                                                  src/expect.jl:54-82,114-121
  rdm(bpc, [u, v]) / rdm_edges / expect_edges (adjacent u, v)             src/rdm.jl:52-73 (reduced_density_matrix, alg = "bp")
  rdm_paths / rdm_pairs / expect_pairs / correlation_function (any u, w)  src/rdm.jl:52-73 with the path from u to w as the Steiner tree
  maxvirtualdim                                                           src/TensorNetworks/abstracttensornetwork.jl:27-29
  sample(psi, nsamples; alg = "bp")                                       src/sampling.jl:3-46
  norm_sqr / norm (alg = "bp", "loopcorrections"), loopcorrected_partitionfunction   src/norm_sqr.jl:10-18,62-78, src/MessagePassing/loopcorrection.jl:3-14
  inner / log_inner (alg = "bp")                                          src/inner.jl:65-69, src/Forms/bilinearform.jl:16-25
  log_amplitudes / amplitudes / log_probabilities (alg = "bp")            src/contract.jl:7-9 on the network certify_sample builds, src/sampling.jl:258-285
  bond_spectra / bond_entropies / renyi_entropy / von_neumann_... / second_renyi_entanglement_entropy   src/entanglement.jl:21-29,73-159 (alg = "bp")
Every flop runs in libtnqs_hip.so; this file only marshals arguments through the C ABI (include/tnqs.h)."""
from __future__ import annotations

import ctypes as C
import math
import warnings
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L
from .gates import gate_matrix, resolve_gate, resolve_gate_flat
from .graphs import NamedGraph, edge_color as _edge_color, leafless_edge_induced_subgraphs, connected_edge_components

_DT = {np.dtype(np.complex64): L.TNQS_C64, np.dtype(np.complex128): L.TNQS_C128, np.dtype(np.float32): L.TNQS_F32, np.dtype(np.float64): L.TNQS_F64}
_DT_INV = {v: k for k, v in _DT.items()}
_STATES = {"↑": (1, 0), "Up": (1, 0), "0": (1, 0), "Z+": (1, 0), "↓": (0, 1), "Dn": (0, 1), "1": (0, 1), "Z-": (0, 1),
           "+": (1 / math.sqrt(2), 1 / math.sqrt(2)), "X+": (1 / math.sqrt(2), 1 / math.sqrt(2)),
           "-": (1 / math.sqrt(2), -1 / math.sqrt(2)), "X-": (1 / math.sqrt(2), -1 / math.sqrt(2))}


class TensorNetworkState:
    """graph + one host tensor per vertex; axes (site, leg to each neighbour in ascending vertex position)"""

    def __init__(self, graph: NamedGraph, tensors: Dict):
        self.graph = graph
        self.tensors = {v: np.asarray(tensors[v]) for v in graph.vertices}
        dts = {t.dtype for t in self.tensors.values()}
        if len(dts) != 1:
            raise ValueError("all site tensors must share one dtype")
        for v in graph.vertices:
            if self.tensors[v].ndim != 1 + graph.degree(v):
                raise ValueError(f"tensor at {v} must have 1 + degree axes")
        for (a, b) in graph.edges:
            if self.bond_dim(a, b) != self.tensors[b].shape[1 + graph.neighbors(b).index(a)]:
                raise ValueError(f"bond dimension mismatch on edge {(a, b)}")

    @property
    def dtype(self):
        return next(iter(self.tensors.values())).dtype

    def bond_dim(self, a, b) -> int:
        return self.tensors[a].shape[1 + self.graph.neighbors(a).index(b)]

    def __getitem__(self, v):
        return self.tensors[v]

    def copy(self):
        return TensorNetworkState(self.graph, dict(self.tensors))


def scalartype(x):
    return x.dtype


def tensornetworkstate(eltype, f: Callable, g: NamedGraph, sitetype: str = "S=1/2", d: int = 2) -> TensorNetworkState:
    tensors = {}
    for v in g.vertices:
        s = f(v)
        if isinstance(s, str):
            if s not in _STATES:
                raise ValueError(f"unknown local state {s!r}")
            vec = np.zeros(d, dtype=eltype)
            vec[:2] = _STATES[s]
        elif isinstance(s, (list, tuple, np.ndarray)):
            vec = np.asarray(s, dtype=eltype)
        else:
            raise RuntimeError("Unrecognized local state constructor. Currently supported: Strings and Vectors.")
        tensors[v] = vec.reshape((len(vec),) + (1,) * g.degree(v))
    return TensorNetworkState(g, tensors)


def random_tensornetworkstate(eltype, g: NamedGraph, bond_dimension: int = 1, d: int = 2, seed: Optional[int] = None) -> TensorNetworkState:
    rng = np.random.default_rng(seed)
    tensors = {}
    for v in g.vertices:
        shp = (d,) + (bond_dimension,) * g.degree(v)
        t = rng.standard_normal(shp)
        if np.issubdtype(np.dtype(eltype), np.complexfloating):
            t = (t + 1j * rng.standard_normal(shp)) / math.sqrt(2)
        tensors[v] = t.astype(eltype)
    return TensorNetworkState(g, tensors)


def default_tolerance(dtype) -> Optional[float]:
    dt = np.dtype(dtype)
    if dt in (np.dtype(np.float32), np.dtype(np.complex64)):
        return 1.0e-5
    if dt in (np.dtype(np.float64), np.dtype(np.complex128)):
        return 1.0e-8
    return None


class BeliefPropagationCache:
    """Device-resident {network, messages} (beliefpropagationcache.jl:9-15) behind an opaque C handle."""

    def __init__(self, network, device: int = 0, _handle=None):
        self._shard = None
        if _handle is not None:
            self.graph, self._h, self.device = network, _handle, device[1]
            return
        if not isinstance(network, TensorNetworkState):
            raise TypeError("BeliefPropagationCache(network): expected a TensorNetworkState")
        g = network.graph
        if network.dtype not in _DT:
            raise TypeError(f"unsupported element type {network.dtype}; supported: float32, float64, complex64, complex128")
        self.graph, self.device = g, device
        es, esp = L.i32([g.index[a] for (a, b) in g.edges])
        ed, edp = L.i32([g.index[b] for (a, b) in g.edges])
        sd, sdp = L.i32([network.tensors[v].shape[0] for v in g.vertices])
        h = L.H()
        L.check(L.lib.tnqs_create(g.nv(), g.ne(), esp, edp, sdp, _DT[network.dtype], device, C.byref(h)))
        self._h = h
        self._shard_pending = None
        dt = self.dtype
        for v in g.vertices:
            self._set_tensor(v, network.tensors[v], dt)

    @property
    def dtype(self):
        """scalartype(bpc): the element type the handle speaks at the boundary.  A cache created from a real network stays real until a
        complex gate is applied to it (adapt_gate keeps a complex gate complex, apply_gates.jl:41-44) -- then it is the complex type of
        the same precision, like the reference's promoted network."""
        c = C.c_int()
        L.check(L.lib.tnqs_scalartype(self._h, C.byref(c)))
        return _DT_INV[c.value]

    # -- marshalling ---------------------------------------------------------------------------------------
    def _roles(self, v):
        # numpy C-order axes (s, n0, n1, ...) == column-major axes (..., n1, n0, s)
        nb = [self.graph.index[w] for w in self.graph.neighbors(v)]
        return list(reversed([-1] + nb))

    def _set_tensor(self, v, t, dt=None):
        dt = self.dtype if dt is None else dt          # (one FFI call; loops over the vertices read it once and pass it in)
        if np.iscomplexobj(t) and not np.issubdtype(dt, np.complexfloating):
            raise TypeError("cannot store a complex tensor in a cache whose element type is real (create it from a complex network)")
        t = np.ascontiguousarray(t, dtype=dt)
        dims = np.array(list(reversed(t.shape)), dtype=np.int64)
        roles, rp = L.i32(self._roles(v))
        L.check(L.lib.tnqs_set_site_tensor(self._h, self.graph.index[v], t.ctypes.data_as(C.c_void_p), t.ndim,
                                           dims.ctypes.data_as(C.POINTER(C.c_int64)), rp))

    def tensor(self, v, dt=None) -> np.ndarray:
        g = self.graph
        shape = [self._site_dim(v)] + [self.bond_dim(v, w) for w in g.neighbors(v)]
        out = np.empty(shape, dtype=self.dtype if dt is None else dt)
        roles, rp = L.i32(self._roles(v))
        L.check(L.lib.tnqs_get_site_tensor(self._h, g.index[v], out.ctypes.data_as(C.c_void_p), out.ndim, rp))
        return out

    def _site_dim(self, v) -> int:
        """the live site dimension (1 after `project`)"""
        d = C.c_int()
        L.check(L.lib.tnqs_site_dim(self._h, self.graph.index[v], C.byref(d)))
        return d.value

    def project(self, v, config: int) -> "BeliefPropagationCache":
        """a copy with psi_v replaced by its slice psi_v[config, ...] (site dimension 1; bond dimensions and messages kept, no rescaling):
        setindex_preserve!(cache, psi_v * onehot(s => config), v) of src/sampling.jl:35-36"""
        out = self.copy()
        L.check(L.lib.tnqs_project_site(out._h, self.graph.index[v], int(config)))
        return out

    def bond_dim(self, a, b) -> int:
        c = C.c_int()
        L.check(L.lib.tnqs_bond_dim(self._h, self.graph.index[a], self.graph.index[b], C.byref(c)))
        return c.value

    def message(self, e) -> np.ndarray:
        """message(bpc, src => dst): chi x chi, axes (ket, bra); identity when unset"""
        a, b = e
        chi = self.bond_dim(a, b)
        out = np.empty((chi, chi), dtype=self.dtype, order="F")
        L.check(L.lib.tnqs_get_message(self._h, self.graph.index[a], self.graph.index[b], out.ctypes.data_as(C.c_void_p), chi))
        return np.ascontiguousarray(out)

    def setmessage(self, e, m):
        a, b = e
        dt = self.dtype
        if np.iscomplexobj(m) and not np.issubdtype(dt, np.complexfloating):
            # same rule as _set_tensor: a real cache does not silently drop imaginary parts
            raise TypeError("cannot store a complex message in a cache whose element type is real (create it from a complex network)")
        m = np.asfortranarray(m, dtype=dt)
        L.check(L.lib.tnqs_set_message(self._h, self.graph.index[a], self.graph.index[b], m.ctypes.data_as(C.c_void_p), m.shape[0]))
        return self

    def network(self) -> TensorNetworkState:
        dt = self.dtype
        return TensorNetworkState(self.graph, {v: self.tensor(v, dt) for v in self.graph.vertices})

    def copy(self) -> "BeliefPropagationCache":
        h = L.H()
        L.check(L.lib.tnqs_copy(self._h, C.byref(h)))
        out = BeliefPropagationCache(self.graph, (None, self.device), _handle=h)
        out._shard = self._shard          # copies share the sharding state (and keep its callback alive)
        if hasattr(self._shard, "attach"):
            self._shard.attach(out)
        return out

    def owns(self, v) -> bool:
        return self._shard is None or self._shard.owner[self.graph.index[v]] == self._shard.rank

    def _set_random(self, v, bond_dims, seed: int, scale: float = 1.0):
        """synthetic site tensor generated on the device (tnqs_set_site_random): iid normal entries, bond_dims[j] = dimension of the leg to the
        j-th neighbour in ascending vertex order; on a sharded handle a vertex of another rank only records the dimensions"""
        dims = np.array(list(bond_dims), dtype=np.int64)
        L.check(L.lib.tnqs_set_site_random(self._h, self.graph.index[v], len(dims), dims.ctypes.data_as(C.POINTER(C.c_int64)),
                                           C.c_uint64(seed), C.c_double(scale)))

    def _declare_dims(self, v, shape):
        """sharded mode: record the bond dimensions of a vertex owned by another rank (no data is uploaded)"""
        dims = np.array(list(reversed(shape)), dtype=np.int64)
        roles, rp = L.i32(self._roles(v))
        L.check(L.lib.tnqs_set_site_tensor(self._h, self.graph.index[v], None, len(shape),
                                           dims.ctypes.data_as(C.POINTER(C.c_int64)), rp))

    def maxvirtualdim(self) -> int:
        c = C.c_int()
        L.check(L.lib.tnqs_maxvirtualdim(self._h, C.byref(c)))
        return c.value

    def default_bp_update_kwargs(self) -> dict:
        if self.graph.is_tree():
            return dict(maxiter=1, tolerance=None)
        return dict(maxiter=25, tolerance=default_tolerance(self.dtype))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and L is not None:
            try:
                L.lib.tnqs_destroy(h)
            except Exception:
                pass
            self._h = None


def network(bpc: BeliefPropagationCache) -> TensorNetworkState:
    return bpc.network()


def maxvirtualdim(x) -> int:
    if isinstance(x, BeliefPropagationCache):
        return x.maxvirtualdim()
    return max([x.bond_dim(a, b) for (a, b) in x.graph.edges], default=1)


def default_bp_update_kwargs(x) -> dict:
    if isinstance(x, BeliefPropagationCache):
        return x.default_bp_update_kwargs()
    if x.graph.is_tree():
        return dict(maxiter=1, tolerance=None)
    return dict(maxiter=25, tolerance=default_tolerance(x.dtype))


def _bp_opts(g: NamedGraph, kw: Optional[dict], defaults: Optional[dict] = None):
    """kwargs of `update` -> tnqs_bp_opts (+ the arrays that must stay alive during the call).
    `kw is None` means the caller omitted `bp_update_kwargs` altogether: `defaults` (= default_bp_update_kwargs, the only
    place where the reference carries a tolerance, beliefpropagationcache.jl:110-117) applies.  An explicit kwargs set
    without `tolerance` means NO convergence check, exactly like `update(bpc; maxiter = 10)` in the reference
    (`default_tolerance(::Algorithm"bp") = nothing`, beliefpropagationcache.jl:62-67)."""
    kw = dict(defaults or {}) if kw is None else dict(kw)
    o = L.BpOpts()
    keep = []
    unknown = set(kw) - {"maxiter", "tolerance", "edge_sequence", "normalize", "verbose"}
    if unknown:
        raise TypeError(f"update: unknown keyword(s) {sorted(unknown)}")
    mi = kw.get("maxiter")
    o.maxiter = int(mi) if mi is not None else 0
    tol = kw.get("tolerance")
    o.tolerance = -1.0 if tol is None else float(tol)
    o.normalize = 1 if kw.get("normalize", True) else 0
    seq = kw.get("edge_sequence")
    if isinstance(seq, str):
        if seq != "forest_cover":
            raise ValueError('edge_sequence: a list of (src, dst) pairs, or "forest_cover" for the reference\'s default order')
        o.n_sequence = -1          # forest_cover_edge_sequence(graph), built inside the library (include/tnqs.h)
        return o, keep
    if seq is not None:
        for (a, b) in seq:
            if a not in g.index or b not in g.index or not g.has_edge(a, b):
                raise RuntimeError(f"update: edge_sequence entry {(a, b)} is not an edge of the graph")
        s, sp = L.i32([g.index[a] for (a, b) in seq])
        d, dp = L.i32([g.index[b] for (a, b) in seq])
        keep += [s, d]
        o.n_sequence, o.seq_src, o.seq_dst = len(seq), sp, dp
    else:
        o.n_sequence = 0
    return o, keep


def update(bpc: BeliefPropagationCache, info: Optional[dict] = None, **kwargs) -> BeliefPropagationCache:
    """update(bpc; maxiter, tolerance, edge_sequence, normalize, verbose): returns a NEW cache (:228)."""
    verbose = kwargs.get("verbose", False)
    o, keep = _bp_opts(bpc.graph, kwargs)
    out = bpc.copy()
    niter, diff = C.c_int(), C.c_double()
    L.check(L.lib.tnqs_bp_update(out._h, C.byref(o), C.byref(niter), C.byref(diff)))
    tol = o.tolerance
    if tol >= 0:
        if diff.value <= tol:
            if verbose:
                print(f"BP converged to desired precision after {niter.value} iterations.")
        else:
            msg = (f"BP did not converge to tolerance {tol} after {niter.value} iterations "
                   f"(final average message change: {diff.value}).")
            print(msg) if verbose else warnings.warn(msg)
    if info is not None:
        info.update(niter=niter.value, diff=diff.value if diff.value >= 0 else None)
    return out


def _apply_opts(kw: Optional[dict], update_cache: bool) -> L.ApplyOpts:
    kw = dict(kw or {})
    unknown = set(kw) - {"maxdim", "cutoff", "normalize_tensors", "sqrt_cutoff"}
    if unknown:
        raise TypeError(f"apply_kwargs: unknown keyword(s) {sorted(unknown)}")
    a = L.ApplyOpts()
    md = kw.get("maxdim")
    a.maxdim = int(md) if md is not None else 0
    co = kw.get("cutoff")
    a.cutoff = float(co) if co is not None else -1.0
    a.normalize_tensors = 1 if kw.get("normalize_tensors", True) else 0
    sc = kw.get("sqrt_cutoff")
    a.sqrt_cutoff = float(sc) if sc is not None else -1.0
    a.update_cache = 1 if update_cache else 0
    return a


def _gate_spec_of(name: str):
    """the registry entry a gate name resolves to right now (None: a Pauli string or an unknown name)"""
    from .gates import _resolve
    return _resolve(name)


def _frozen_probe(gt):
    """None: not cacheable; (): nothing mutable; tuple(vs): the snapshot of a vertex list"""
    if not (isinstance(gt, tuple) and len(gt) >= 2 and isinstance(gt[0], str)):
        return None
    if not all(isinstance(x, (int, float, complex, np.integer, np.floating, np.complexfloating, bool)) for x in gt[2:]):
        return None
    vs = gt[1]
    if isinstance(vs, np.ndarray):
        return None
    if isinstance(vs, (list, tuple)) and any(isinstance(x, (list, np.ndarray, dict, set)) for x in vs):
        return None
    return tuple(vs) if isinstance(vs, list) else ()


_MARSHALLED: list = []      # (graph, ids of the gate tuples, gate tuples, arrays): the last few circuits, most recent first


def _marshal_circuit(circuit: Sequence, g: NamedGraph):
    """circuit tuples -> the flat arrays of tnqs_apply_gates (vertex counts, vertex ids, complex128 matrices).  A Trotter loop applies the same
    layer object over and over (examples/2dIsing_dynamics.jl:56-57); resolving 1160 gate tuples costs 2.5 ms of Python per 20x20 layer and 0.75 ms of
    a 5 ms heavy-hex layer, so the arrays of the last few circuits are kept -- keyed by the IDENTITY of every gate tuple (tuples are immutable: the same
    objects in the same order on the same graph are the same circuit), which costs ~30 ns per gate to check."""
    ids = tuple(map(id, circuit))
    for k, (g0, ids0, _gates, specs, snaps, arrs) in enumerate(_MARSHALLED):
        if (g0 is g and ids0 == ids and all(_gate_spec_of(nm) is sp for nm, sp in specs)      # (the registry still maps every name to the same definition)
                and (snaps is None or all(sn is None or (type(gt[1]) is list and tuple(gt[1]) == sn) for gt, sn in zip(circuit, snaps)))):
            if k:
                _MARSHALLED.insert(0, _MARSHALLED.pop(k))
            return arrs
    nverts, verts, mats = [], [], []
    index = g.index
    for gate in circuit:
        m, vs = resolve_gate_flat(gate, g)
        nverts.append(len(vs))
        for v in vs:
            verts.append(index[v])
        mats.append(m)
    ng = len(nverts)
    nv_a, nv_p = L.i32(nverts if ng else [0])
    vs_a, vs_p = L.i32(verts if verts else [0])
    mat_a = np.ascontiguousarray(np.concatenate(mats) if mats else np.zeros(1, dtype=np.complex128))
    arrs = (ng, nv_a, nv_p, vs_a, vs_p, mat_a)
    # cached only when nothing of a gate can be edited in place behind the identity key without being noticed (round-4 advisor finding): the gate is a
    # tuple, its name a string, its parameters plain numbers, its vertices a tuple / one hashable vertex -- or a LIST of hashable vertices, the form the
    # reference's API, the README and most callers use (("Rzz", [a, b], theta)): a list can be edited in place, so a frozen snapshot of it is kept next to
    # the identity key and compared on every lookup (~100 ns per gate; round-5 advisor finding: only tuple-form circuits were cached).  Anything else --
    # array parameters, nested lists -- is resolved again on every call.
    fz = [_frozen_probe(gt) for gt in circuit]
    if all(f is not None for f in fz):
        names = {gt[0] for gt in circuit}
        snaps = [f if f != () or isinstance(gt[1], list) else None for gt, f in zip(circuit, fz)]
        if all(sn is None for sn in snaps):
            snaps = None
        _MARSHALLED.insert(0, (g, ids, tuple(circuit), [(nm, _gate_spec_of(nm)) for nm in names], snaps, arrs))   # the tuple keeps the gate objects (and their ids) alive
        del _MARSHALLED[4:]
    return arrs


def apply_gates(circuit: Sequence, psi, apply_kwargs: Optional[dict] = None, bp_update_kwargs: Optional[dict] = None,
                update_cache: bool = True, verbose: bool = False, info: Optional[dict] = None):
    """apply_gates(circuit, psi; apply_kwargs, bp_update_kwargs, update_cache) -> (psi', truncation_errors).
    psi may be a TensorNetworkState (wrapped, BP-updated first, network returned; apply_gates.jl:17-27) or a
    BeliefPropagationCache (returned as a new cache; the input is untouched, :55)."""
    if isinstance(psi, TensorNetworkState):
        b0 = BeliefPropagationCache(psi)
        bpc = update(b0, **(b0.default_bp_update_kwargs() if bp_update_kwargs is None else bp_update_kwargs))
        out, errs = apply_gates(circuit, bpc, apply_kwargs=apply_kwargs, bp_update_kwargs=bp_update_kwargs,
                                update_cache=update_cache, verbose=verbose, info=info)
        return out.network(), errs
    if not isinstance(psi, BeliefPropagationCache):
        raise TypeError("apply_gates: expected a TensorNetworkState or a BeliefPropagationCache")
    g = psi.graph
    ng, nv_a, nv_p, vs_a, vs_p, mat_a = _marshal_circuit(circuit, g)
    errs = np.zeros(max(ng, 1), dtype=np.float64)
    ao = _apply_opts(apply_kwargs, update_cache)
    bo, keep = _bp_opts(g, bp_update_kwargs, psi.default_bp_update_kwargs())
    st = L.ApplyStats()
    out = psi.copy()
    L.check(L.lib.tnqs_apply_gates(out._h, ng, nv_p, vs_p, mat_a.ctypes.data_as(C.POINTER(C.c_double)), C.byref(ao),
                                   C.byref(bo), errs.ctypes.data_as(C.POINTER(C.c_double)), C.byref(st)))
    if st.bp_not_converged and not verbose:
        warnings.warn(f"BP did not converge in {st.bp_not_converged} of {st.n_bp_updates} cache updates "
                      f"(final average message change: {st.last_bp_diff}).")
    if info is not None:
        info.update(n_chol_fallbacks=st.n_chol_fallbacks, n_qr2_sites=st.n_qr2_sites, n_lowrank_svd=st.n_lowrank_svd, n_tall_svd=st.n_tall_svd, n_deferred_1site=st.n_deferred_1site, n_lowrank_fallbacks=st.n_lowrank_fallbacks, n_bp_products_reused=st.n_bp_products_reused, n_bp_products_evicted=st.n_bp_products_evicted, n_svd_sweeps=st.n_svd_sweeps, n_svd_sweeps_max=st.n_svd_sweeps_max, n_updates=st.n_bp_updates, n_sweeps=st.n_bp_sweeps, n_batches=st.n_batches,
                    n_two_site=st.n_two_site, bp_not_converged=st.bp_not_converged, n_spec_batches=st.n_spec_batches, n_spec_redone=st.n_spec_redone)
    return out, errs[:ng]


apply_circuit = apply_gates


def truncate(bpc, maxdim: int, cutoff: Optional[float] = None, edge_color=True,
             normalize_tensors: bool = True, bp_update_kwargs: Optional[dict] = None, info: Optional[dict] = None, alg: str = "bp",
             device: int = 0):
    """truncate(bpc; maxdim, cutoff, edge_color, normalize_tensors) (src/truncate.jl:12-38).  `edge_color` may be
    True (compute a colouring), False (update after every edge) or an explicit list of edge groups.
    Given a TensorNetworkState instead of a cache (src/truncate.jl:74-79, alg"bp"): a cache is built and updated with the defaults, truncated,
    and its network returned."""
    if alg != "bp":
        raise ValueError(f'truncate: only alg = "bp" is part of this path (received {alg!r}; boundary MPS truncation is out of scope)')
    if isinstance(bpc, TensorNetworkState):
        cache = update(BeliefPropagationCache(bpc, device=device))
        return network(truncate(cache, maxdim, cutoff=cutoff, edge_color=edge_color, normalize_tensors=normalize_tensors,
                                bp_update_kwargs=bp_update_kwargs, info=info))
    g = bpc.graph
    if edge_color is True:
        groups = _edge_color(g)
    elif edge_color is False:
        groups = []
    else:
        groups = [list(grp) for grp in edge_color]
    offs, eu, ev = [0], [], []
    for grp in groups:
        for (a, b) in grp:
            eu.append(g.index[a]); ev.append(g.index[b])
        offs.append(len(eu))
    o_a, o_p = L.i32(offs)
    u_a, u_p = L.i32(eu if eu else [0])
    v_a, v_p = L.i32(ev if ev else [0])
    bo, keep = _bp_opts(g, bp_update_kwargs, bpc.default_bp_update_kwargs())
    st = L.ApplyStats()
    out = bpc.copy()
    L.check(L.lib.tnqs_truncate(out._h, int(maxdim), -1.0 if cutoff is None else float(cutoff), 1 if normalize_tensors else 0,
                                len(groups), o_p, u_p, v_p, C.byref(bo), C.byref(st)))
    if info is not None:
        info.update(n_chol_fallbacks=st.n_chol_fallbacks, n_qr2_sites=st.n_qr2_sites, n_lowrank_svd=st.n_lowrank_svd, n_tall_svd=st.n_tall_svd, n_updates=st.n_bp_updates, n_sweeps=st.n_bp_sweeps, n_two_site=st.n_two_site)
    return out


def _rdm_edges_raw(bpc: BeliefPropagationCache, edges) -> Tuple[list, List[np.ndarray]]:
    """tnqs_rdm_edges: the un-normalised (d_u d_v) x (d_u d_v) matrices of `edges` (None: every edge of the graph) in request order, one device call"""
    g = bpc.graph
    req = list(g.edges) if edges is None else [tuple(e) for e in edges]
    for e in req:
        if len(e) != 2 or e[0] not in g.index or e[1] not in g.index or e[1] not in g.neighbors(e[0]):
            raise L.TnqsArgumentError(f"{e!r} is not an edge of the graph: only single vertices and bonds are supported")
    dim: Dict = {}
    for e in req:
        for v in e:
            if v not in dim:
                dim[v] = bpc._site_dim(v)
    sizes = [(dim[a] * dim[b]) ** 2 for (a, b) in req]
    out = np.zeros(sum(sizes), dtype=np.complex128)
    if edges is None:
        up, vp = None, None
    else:
        _u, up = L.i32([g.index[a] for (a, b) in req] or [0])
        _v, vp = L.i32([g.index[b] for (a, b) in req] or [0])
    L.check(L.lib.tnqs_rdm_edges(bpc._h, len(req), up, vp, out.ctypes.data_as(C.POINTER(C.c_double))))
    mats, off = [], 0
    for (a, b), n in zip(req, sizes):
        dd = dim[a] * dim[b]
        mats.append(np.ascontiguousarray(out[off:off + n].reshape(dd, dd, order="F")))
        off += n
    return req, mats


def rdm_edges(bpc: BeliefPropagationCache, edges=None, normalize: bool = True) -> Dict:
    """two-site reduced density matrices of bonds from the BP environment, all in one device call (reduced_density_matrix(cache, [u, v]; alg = "bp") of the
    reference for adjacent u, v): {(u, v): rho} with rho[s_v + d_v s_u, s_v' + d_v s_u'] -- the first vertex most significant, so that
    tr(np.kron(O_u, O_v) @ rho) is <O_u O_v> of a normalised rho.  edges = None: every edge of the graph; (v, u) gives the index-swapped matrix of (u, v)"""
    req, mats = _rdm_edges_raw(bpc, edges)
    return {e: (m / np.trace(m) if normalize else m) for e, m in zip(req, mats)}


def _two_site_operator(op, who: str) -> np.ndarray:
    """the (d_u d_v) x (d_u d_v) complex128 matrix of a two-site observable, first vertex most significant: a two-character Pauli string ("ZZ"), a pair of one-site
    matrices (O_u, O_v), or the full matrix itself"""
    if isinstance(op, str):
        if len(op) != 2:
            raise L.TnqsArgumentError(f"{who}: a string observable names one operator per vertex of the bond (two characters)")
        full = np.kron(gate_matrix(op[0]), gate_matrix(op[1]))
    elif isinstance(op, (tuple, list)) or (isinstance(op, np.ndarray) and op.ndim == 3):
        if len(op) != 2:
            raise L.TnqsArgumentError(f"{who}: a pair of one-site operators is expected")
        full = np.kron(np.asarray(op[0]), np.asarray(op[1]))
    else:
        full = np.asarray(op)
    return np.asarray(full, dtype=np.complex128)


def expect_edges(bpc: BeliefPropagationCache, op, edges=None) -> np.ndarray:
    """<O_u O_v> = tr(op rho_uv) / tr(rho_uv) for every listed bond (None: every edge of the graph, in its order) from ONE device call; `op`: a two-character
    Pauli string ("ZZ"), a pair of d x d matrices (O_u, O_v), or one (d_u d_v) x (d_u d_v) matrix with the first vertex most significant.  The operator is
    applied on the host"""
    full = _two_site_operator(op, "expect_edges")
    req, mats = _rdm_edges_raw(bpc, edges)
    out = np.zeros(len(req), dtype=np.complex128)
    for i, (e, m) in enumerate(zip(req, mats)):
        if full.shape != m.shape:
            raise L.TnqsArgumentError(f"expect_edges: operator of shape {full.shape} on bond {e!r} of dimension {m.shape[0]}")
        out[i] = np.sum(full * m.T) / np.trace(m)
    return out


# ---- two-site density matrices of distant vertices: the two ENDS of a path (tnqs_rdm_paths) ----------------------------------------------------
def _check_path(g, path) -> list:
    """an induced path of the graph as a list of vertices, or TnqsArgumentError: the reference contracts the INDUCED region of the path's vertices, so a chord would be
    summed over -- a different quantity, refused rather than answered"""
    path = list(path)
    if len(path) < 2:
        raise L.TnqsArgumentError(f"rdm_paths: a path has at least two vertices, got {path!r}")
    for v in path:
        if v not in g.index:
            raise L.TnqsArgumentError(f"rdm_paths: {v!r} is not a vertex of the graph")
    if len(set(path)) != len(path):
        raise L.TnqsArgumentError(f"rdm_paths: repeated vertex in the path {path!r}")
    nb = [set(g.neighbors(v)) for v in path]
    for k in range(len(path) - 1):
        if path[k + 1] not in nb[k]:
            raise L.TnqsArgumentError(f"rdm_paths: not a path: {path[k]!r} and {path[k + 1]!r} are not adjacent")
    for k in range(len(path)):
        for q in range(k + 2, len(path)):
            if path[q] in nb[k]:
                raise L.TnqsArgumentError(f"rdm_paths: the path has a chord ({path[k]!r} and {path[q]!r} are adjacent): only induced paths are supported "
                                          "(a shortest path is always induced)")
    return path


def _rdm_paths_raw(bpc: BeliefPropagationCache, paths) -> List[List[np.ndarray]]:
    """tnqs_rdm_paths: for every path, the un-normalised (d_p0 d_pk) x (d_p0 d_pk) matrices of (p_0, p_k), k = 1 .. len - 1; one device call"""
    g = bpc.graph
    paths = [_check_path(g, p) for p in paths]
    if not paths:
        return []
    dim: Dict = {}
    for p in paths:
        for v in p:
            if v not in dim:
                dim[v] = bpc._site_dim(v)
    sizes = [[(dim[p[0]] * dim[w]) ** 2 for w in p[1:]] for p in paths]
    out = np.zeros(sum(sum(sz) for sz in sizes), dtype=np.complex128)
    _l, lp = L.i32([len(p) for p in paths])
    _v, vp = L.i32([g.index[v] for p in paths for v in p])
    L.check(L.lib.tnqs_rdm_paths(bpc._h, len(paths), lp, vp, out.ctypes.data_as(C.POINTER(C.c_double))))
    res, off = [], 0
    for p, sz in zip(paths, sizes):
        mats = []
        for w, n in zip(p[1:], sz):
            dd = dim[p[0]] * dim[w]
            mats.append(np.ascontiguousarray(out[off:off + n].reshape(dd, dd, order="F")))
            off += n
        res.append(mats)
    return res


def _checked_trace(m: np.ndarray, pair) -> complex:
    t = np.trace(m)
    if t == 0 or not np.isfinite(t):
        raise L.TnqsDomainError(f"rdm_paths: the density matrix of {pair!r} has trace {t!r}: the environment carried along the path left the range of float64 "
                                "(it is not rescaled along the path)")
    return t


def rdm_paths(bpc: BeliefPropagationCache, paths, normalize: bool = True) -> List[Dict]:
    """two-site reduced density matrices of the two ENDS of paths from the BP environment, all in one device call (reduced_density_matrix(cache, [u, w]; alg = "bp") of
    the reference with the path as the Steiner tree): for every path p_0 .. p_n one dict {(p_0, p_k): rho, k = 1 .. n} -- a path yields the matrix of its first vertex
    with EVERY later one -- in the layout of rdm_edges (first vertex most significant).  Paths must be induced (no two non-consecutive vertices adjacent; a shortest path
    always is): TnqsArgumentError otherwise, before any device work.  The environment of p_0 is carried along the path in complex128 whatever the state's type, but it is
    NOT rescaled on the way: float64's range is what it has, and a trace that comes back zero or non-finite raises TnqsDomainError naming the pair"""
    paths = [list(p) for p in paths]
    res = []
    for p, mats in zip(paths, _rdm_paths_raw(bpc, paths)):
        dct = {}
        for w, m in zip(p[1:], mats):
            t = _checked_trace(m, (p[0], w))
            dct[(p[0], w)] = m / t if normalize else m
        res.append(dct)
    return res


def _merge_pair_paths(paths) -> Tuple[list, list]:
    """(merged, where): a path that is a prefix of another one of the list (same source, same first steps) rides on it -- merged holds the paths that are no such prefix,
    where[i] = (index into merged, k) says that paths[i] ends at vertex k of that merged path.  Pure host logic"""
    order = sorted(range(len(paths)), key=lambda i: -len(paths[i]))
    merged, prefix_of, where = [], {}, [None] * len(paths)
    for i in order:
        key = tuple(paths[i])
        if key not in prefix_of:
            merged.append(list(paths[i]))
            for k in range(1, len(key)):
                prefix_of.setdefault(key[:k + 1], (len(merged) - 1, k))
        where[i] = prefix_of[key]
    return merged, where


def _pair_path(g, u, w) -> list:
    """the tree path from u to w of steiner_region(g, [u, w]): the path expect(bpc, (op, [u, w])) contracts"""
    from .graphs import steiner_region
    for v in (u, w):
        if v not in g.index:
            raise L.TnqsArgumentError(f"rdm_pairs: {v!r} is not a vertex of the graph")
    if u == w:
        raise L.TnqsArgumentError(f"rdm_pairs: a pair names two different vertices, got {(u, w)!r}")
    try:
        region, parent = steiner_region(g, [u, w])
    except ValueError as e:
        raise L.TnqsArgumentError(str(e))
    path, i = [], region.index(w)
    while i >= 0:
        path.append(region[i]); i = parent[i]
    return path[::-1]


def _rdm_pairs_raw(bpc: BeliefPropagationCache, pairs) -> Tuple[list, List[np.ndarray]]:
    g = bpc.graph
    pairs = [tuple(p) for p in pairs]
    for p in pairs:
        if len(p) != 2:
            raise L.TnqsArgumentError(f"rdm_pairs: a pair names two vertices, got {p!r}")
    need, seen = [], set()                       # pairs that get a path: (w, u) listed after (u, w) is the index swap of it
    for (u, w) in pairs:
        if (u, w) not in seen and (w, u) not in seen:
            need.append((u, w))
        seen.add((u, w))
    merged, where = _merge_pair_paths([_pair_path(g, u, w) for (u, w) in need])
    raw = _rdm_paths_raw(bpc, merged)
    have = {pr: raw[j][k - 1] for pr, (j, k) in zip(need, where)}
    mats = []
    for (u, w) in pairs:
        if (u, w) in have:
            mats.append(have[(u, w)])
        else:
            m = have[(w, u)]; dw, du = bpc._site_dim(w), bpc._site_dim(u)
            mats.append(np.ascontiguousarray(m.reshape(dw, du, dw, du).transpose(1, 0, 3, 2).reshape(du * dw, du * dw)))
    return pairs, mats


def rdm_pairs(bpc: BeliefPropagationCache, pairs, normalize: bool = True) -> Dict:
    """{(u, w): rho} for arbitrary pairs of vertices from ONE device call (rdm_paths): the path of a pair is the tree path from u to w of steiner_region(g, [u, w]) -- the
    one expect(bpc, (op, [u, w])) contracts, so the two agree.  A pair whose path is a prefix of another requested pair's path from the same source rides on it; adjacent
    pairs are allowed; (w, u) listed after (u, w) is the index swap, done on the host"""
    req, mats = _rdm_pairs_raw(bpc, pairs)
    return {pr: (m / _checked_trace(m, pr) if normalize else m) for pr, m in zip(req, mats)}


def expect_pairs(bpc: BeliefPropagationCache, op, pairs) -> np.ndarray:
    """<O_u O_w> = tr(op rho_uw) / tr(rho_uw) for every listed pair of vertices (adjacent or not) from ONE device call; `op` as in expect_edges, applied on the host"""
    full = _two_site_operator(op, "expect_pairs")
    req, mats = _rdm_pairs_raw(bpc, pairs)
    out = np.zeros(len(req), dtype=np.complex128)
    for i, (pr, m) in enumerate(zip(req, mats)):
        if full.shape != m.shape:
            raise L.TnqsArgumentError(f"expect_pairs: operator of shape {full.shape} on the pair {pr!r} of dimension {m.shape[0]}")
        out[i] = np.sum(full * m.T) / _checked_trace(m, pr)
    return out


def correlation_function(bpc: BeliefPropagationCache, op, path, connected: bool = False) -> np.ndarray:
    """<O_{p0} O_{pk}>, k = 1 .. n - 1, along an induced path p_0 .. p_{n-1} from ONE device call; `op`: a pair of one-site operators (O_first, O_other) or a
    two-character Pauli string.  connected = True subtracts <O_{p0}> <O_{pk}> taken from the partial traces of the SAME two-site matrix: no further device call, and
    consistent by construction.  The environment is not rescaled along the path (see rdm_paths)"""
    if isinstance(op, str):
        if len(op) != 2:
            raise L.TnqsArgumentError("correlation_function: a string observable names one operator per end (two characters)")
        a, b = gate_matrix(op[0]), gate_matrix(op[1])
    else:
        if len(op) != 2:
            raise L.TnqsArgumentError("correlation_function: a pair of one-site operators is expected")
        a, b = np.asarray(op[0]), np.asarray(op[1])
    a = np.asarray(a, dtype=np.complex128); b = np.asarray(b, dtype=np.complex128)
    path = list(path)
    (mats,) = _rdm_paths_raw(bpc, [path])
    out = np.zeros(len(mats), dtype=np.complex128)
    for k, m in enumerate(mats):
        du, dw = a.shape[0], b.shape[0]
        if m.shape[0] != du * dw:
            raise L.TnqsArgumentError(f"correlation_function: operators of dimensions {du}, {dw} on the pair {(path[0], path[k + 1])!r} of dimension {m.shape[0]}")
        r4 = (m / _checked_trace(m, (path[0], path[k + 1]))).reshape(du, dw, du, dw)
        out[k] = np.einsum("as,bt,stab->", a, b, r4)
        if connected:
            out[k] -= np.einsum("as,sbab->", a, r4) * np.einsum("bt,atab->", b, r4)
    return out


def rdm(bpc: BeliefPropagationCache, v) -> np.ndarray:
    """normalised reduced density matrix from the BP environment: rho[s, s'] of a vertex, or -- for a list [u, v] of two adjacent vertices -- the two-site
    matrix of that bond (rdm_edges)"""
    if isinstance(v, list):
        if len(v) != 2 or v[0] not in bpc.graph.index or v[1] not in bpc.graph.index or v[1] not in bpc.graph.neighbors(v[0]):
            raise L.TnqsArgumentError(f"rdm: only single vertices and bonds (two adjacent vertices) are supported, got {v!r}")
        return rdm_edges(bpc, [tuple(v)])[tuple(v)]
    d = bpc._site_dim(v)
    out = np.zeros((d, d), dtype=np.complex128, order="F")
    L.check(L.lib.tnqs_rdm_1site(bpc._h, bpc.graph.index[v], out.ctypes.data_as(C.POINTER(C.c_double))))
    out = np.ascontiguousarray(out)
    return out / np.trace(out)


def _entropy_threshold(dtype) -> float:
    """10 eps of the real type of `dtype`: the reference's filter on the eigenvalues of a density matrix (entanglement.jl:26)"""
    dt = np.dtype(dtype)
    real = np.float32 if dt in (np.dtype(np.float32), np.dtype(np.complex64)) else np.float64
    return 10.0 * float(np.finfo(real).eps)


def _check_alpha(alpha) -> float:
    if isinstance(alpha, (bool, complex, np.complexfloating)) or not isinstance(alpha, (int, float, np.integer, np.floating)) or not alpha >= 0:
        raise L.TnqsArgumentError(f"renyi_entropy: the Renyi index must be real and >= 0 (received {alpha!r})")
    return float(alpha)


def _renyi_from_spectrum(lam, alpha: float, threshold: float) -> float:
    """renyi_entropy on eigenvalues (entanglement.jl:26-28): those with |lambda| <= threshold are dropped; alpha = 1: -sum lambda log lambda, otherwise
    log(sum lambda^alpha) / (1 - alpha).  A kept negative eigenvalue under a logarithm or a non-integer power is Julia's DomainError"""
    lam = np.asarray(lam, dtype=np.float64)
    lam = lam[np.abs(lam) > threshold]
    if alpha == 1.0:
        if np.any(lam < 0):
            raise L.TnqsDomainError("renyi_entropy: log of a negative eigenvalue of the density matrix")
        return float(-np.sum(lam * np.log(lam)))
    if alpha != int(alpha) and np.any(lam < 0):
        raise L.TnqsDomainError("renyi_entropy: non-integer power of a negative eigenvalue of the density matrix")
    s = float(np.sum(lam ** (int(alpha) if alpha == int(alpha) else alpha)))
    if s < 0:
        raise L.TnqsDomainError("renyi_entropy: log of a negative sum of eigenvalue powers")
    with np.errstate(divide="ignore"):
        return float(np.log(s) / (1.0 - alpha))


def _bond_spectra_raw(bpc: BeliefPropagationCache, edges) -> Tuple[list, List[np.ndarray]]:
    """tnqs_bond_spectra: the spectra of `edges` (None: every edge of the graph) in request order, one device call"""
    g = bpc.graph
    req = list(g.edges) if edges is None else [tuple(e) for e in edges]
    for e in req:
        if len(e) != 2 or e[0] not in g.index or e[1] not in g.index or e[1] not in g.neighbors(e[0]):
            raise L.TnqsArgumentError(f"{e!r} is not an edge of the graph: a bond spectrum belongs to two adjacent vertices")
    if not req:
        return [], []
    chis = [bpc.bond_dim(a, b) for (a, b) in req]
    out = np.zeros(sum(chis), dtype=np.float64)
    if edges is None:
        up, vp = None, None
    else:
        _u, up = L.i32([g.index[a] for (a, b) in req])
        _v, vp = L.i32([g.index[b] for (a, b) in req])
    L.check(L.lib.tnqs_bond_spectra(bpc._h, len(req), up, vp, out.ctypes.data_as(C.POINTER(C.c_double))))
    offs = np.concatenate([[0], np.cumsum(chis)])
    return req, [out[offs[i]:offs[i + 1]].copy() for i in range(len(req))]


def bond_spectra(bpc: BeliefPropagationCache, edges=None) -> Dict:
    """entanglement spectra of bonds from the BP messages, all in one device call: {(u, v): lambda} with lambda the eigenvalues of rho / tr rho,
    rho = sqrt(m_vu) m_uv^T sqrt(m_vu) (entanglement.jl:73-86), as a float64 array of chi entries -- descending, summing to 1, UNFILTERED.  edges = None: every edge of the
    graph; (v, u) and repeats are computed as listed (a repeated key keeps its last answer; bond_entropies keeps all).  Exact on trees (the Schmidt spectrum squared)"""
    req, spec = _bond_spectra_raw(bpc, edges)
    return dict(zip(req, spec))


def bond_entropies(bpc: BeliefPropagationCache, alpha=1, edges=None) -> np.ndarray:
    """Renyi entropies of order alpha (1: von Neumann) of the listed bonds (None: every edge of the graph, in its order), in request order, from ONE device call;
    the eigenvalues with |lambda| <= 10 eps(real type of the state) are dropped on the host as the reference drops them"""
    a = _check_alpha(alpha)
    _req, spec = _bond_spectra_raw(bpc, edges)
    if not spec:
        return np.zeros(0, dtype=np.float64)
    thr = _entropy_threshold(bpc.dtype)
    return np.array([_renyi_from_spectrum(lam, a, thr) for lam in spec], dtype=np.float64)


def renyi_entropy(x, where=None, alpha=None, alg: str = "bp", normalize: bool = True, cache_update_kwargs: Optional[dict] = None, device: int = 0) -> float:
    """renyi_entropy of the reference (src/entanglement.jl):
      renyi_entropy(rho, alpha, normalize=True)     rho a square numpy matrix (:21-29), on the host: eigenvalues of the Hermitian matrix rho (/ tr rho), those with
                                                    |lambda| <= 10 eps(real dtype of rho) dropped
      renyi_entropy(bpc, (u, v), alpha)             the bond formula from the two messages of the edge (:73-86), on the device (bond_spectra)
      renyi_entropy(bpc, [v] | [u, w], alpha)       entropy of the reduced density matrix of one vertex or of a pair of vertices, adjacent or not (:135-138; rdm,
                                                    rdm_edges, rdm_pairs); longer lists are not supported
      renyi_entropy(psi, ..., alpha)                a TensorNetworkState: a cache is built on `device` and updated with cache_update_kwargs (default
                                                    default_bp_update_kwargs) first (:110-114)
    alpha real and >= 0 (1: von Neumann).  Only alg = "bp"."""
    if isinstance(x, np.ndarray):
        if alpha is None:                              # renyi_entropy(rho, alpha)
            where, alpha = None, where
        a = _check_alpha(alpha)
        if x.ndim != 2 or x.shape[0] != x.shape[1]:
            raise L.TnqsArgumentError(f"renyi_entropy: a density matrix is square (received shape {x.shape})")
        rho = x if np.issubdtype(x.dtype, np.inexact) else x.astype(np.float64)
        thr = _entropy_threshold(rho.dtype)
        if normalize:
            rho = rho / np.trace(rho)
        lam = np.linalg.eigvalsh(rho, UPLO="U")                                    # Hermitian(rho): the upper triangle
        return _renyi_from_spectrum(lam, a, thr)
    if alg != "bp":
        raise L.TnqsError(f'renyi_entropy: algorithm choice not supported; supported on the HIP path: "bp" (received {alg!r})')
    a = _check_alpha(alpha)
    if not isinstance(x, (TensorNetworkState, BeliefPropagationCache)):
        raise TypeError("renyi_entropy: expected a matrix, a TensorNetworkState or a BeliefPropagationCache")
    g = x.graph
    if isinstance(where, tuple):
        if len(where) != 2 or where[0] not in g.index or where[1] not in g.index or where[1] not in g.neighbors(where[0]):
            raise L.TnqsArgumentError(f"renyi_entropy: {where!r} is not an edge of the graph")
    elif isinstance(where, list):
        if len(where) not in (1, 2) or any(v not in g.index for v in where) or len(set(where)) != len(where):
            raise L.TnqsArgumentError(f"renyi_entropy: only single vertices and pairs of vertices are supported, got {where!r}")
    else:
        raise L.TnqsArgumentError("renyi_entropy: `where` is an edge (a 2-tuple of adjacent vertices) or a list of one or two vertices")
    if isinstance(x, TensorNetworkState):
        bpc = BeliefPropagationCache(x, device=device)
        bpc = update(bpc, **(bpc.default_bp_update_kwargs() if cache_update_kwargs is None else cache_update_kwargs))
    else:
        bpc = x
    thr = _entropy_threshold(bpc.dtype)
    if isinstance(where, tuple):
        return _renyi_from_spectrum(_bond_spectra_raw(bpc, [where])[1][0], a, thr)
    if len(where) == 1:
        rho = rdm(bpc, where[0])
    elif where[1] in g.neighbors(where[0]):
        rho = rdm_edges(bpc, [tuple(where)])[tuple(where)]
    else:
        rho = rdm_pairs(bpc, [tuple(where)])[tuple(where)]
    # reduced_density_matrix(...; normalize = false) then renyi_entropy(...; normalize = true): the filter sees the state's real type
    return _renyi_from_spectrum(np.linalg.eigvalsh(rho, UPLO="U"), a, thr)


def von_neumann_entanglement_entropy(*args, **kwargs) -> float:
    """renyi_entropy with alpha = 1 (entanglement.jl:159)"""
    return renyi_entropy(*args, **kwargs, alpha=1)


def second_renyi_entanglement_entropy(*args, **kwargs) -> float:
    """renyi_entropy with alpha = 2 (entanglement.jl:149)"""
    return renyi_entropy(*args, **kwargs, alpha=2)


def _collect_observable(obs, g):
    """collectobservable (src/expect.jl:159-175): ("Z", [v]) / ("Z", v) / ("Z", [v], coeff)"""
    op = obs[0]
    verts = obs[1] if isinstance(obs[1], list) else ([obs[1]] if obs[1] in g.index else list(obs[1]))
    coeff = obs[2] if len(obs) > 2 else 1.0
    return op, verts, coeff


def _observable_ops(op, verts) -> list:
    ops = [c for c in op] if isinstance(op, str) else list(op)      # one Pauli character per vertex (collectobservable, expect.jl:159-175)
    if len(ops) != len(verts):
        raise L.TnqsError("Invalid observable: need as many operators as vertices passed.")
    return ops


def boundarymps_partitioning(observable, g) -> str:
    """boundarymps_partitioning (src/expect.jl:186-200): "row" when every observable's support shares its first coordinate, else "col" when it shares the last"""
    partitioning = None
    for o in (observable if isinstance(observable, list) else [observable]):
        vs = _collect_observable(o, g)[1]
        if len({v[0] for v in vs}) == 1 and partitioning in ("row", None):
            partitioning = "row"
        elif len({v[-1] for v in vs}) == 1 and partitioning in ("col", None):
            partitioning = "col"
        else:
            raise L.TnqsArgumentError("Observables must all be aligned in either the same column or the same row to do BoundaryMPS measurements.")
    return "row" if partitioning is None else partitioning


def _bmps_check_format(g, partition_by: str):
    """what BoundaryMPSCache(...) would need of the graph (src/MessagePassing/boundarympscache.jl:145-175, is_correct_format, :69-81), checked before any device work"""
    if partition_by not in ("row", "col"):
        raise L.TnqsArgumentError(f'boundarymps: partition_by must be "row" or "col" (received {partition_by!r})')
    if not all(isinstance(v, tuple) and len(v) == 2 for v in g.vertices):
        raise L.TnqsArgumentError("boundarymps: vertices must be 2-tuples (row, column)")
    key = (lambda v: v[0]) if partition_by == "row" else (lambda v: v[1])
    order = (lambda v: v[1]) if partition_by == "row" else (lambda v: v[0])
    keys = sorted({key(v) for v in g.vertices})
    part = {v: keys.index(key(v)) for v in g.vertices}
    groups = [sorted([v for v in g.vertices if part[v] == p], key=order) for p in range(len(keys))]
    for gr in groups:
        for a, b in zip(gr, gr[1:]):
            if b not in g.neighbors(a):
                raise L.TnqsArgumentError("boundarymps: consecutive vertices of a partition are not neighbours: the graph would need pseudo-edges, which are not supported")
    for (a, b) in g.edges:                            # the quotient graph first, then the partitions, as is_correct_format does
        dp = abs(part[a] - part[b])
        if dp > 1:
            if dp == len(keys) - 1:
                raise L.TnqsArgumentError("boundarymps: upon partitioning the graph forms a ring (periodic boundaries), which is not supported")
            raise L.TnqsArgumentError("Upon partitioning, graph does not form a line or ring: can't run boundary MPS")
    for (a, b) in g.edges:
        if part[a] == part[b] and abs(groups[part[a]].index(a) - groups[part[a]].index(b)) != 1:
            raise L.TnqsArgumentError("There's a partition that does not form a line: can't run boundary MPS")
    return part


def _bmps_handle(x, gauge_state: bool, device: int, who: str) -> BeliefPropagationCache:
    if isinstance(x, BeliefPropagationCache):
        return x                                      # the network as it stands; its messages are neither read nor changed
    if not isinstance(x, TensorNetworkState):
        raise TypeError(f"{who}: expected a TensorNetworkState or a BeliefPropagationCache")
    bpc = BeliefPropagationCache(x, device=device)
    if gauge_state:                                   # gauge_and_scale (src/symmetric_gauge.jl:76-83): BP with maxiter = 40, rescale, symmetric gauge
        bpc = symmetrize_and_normalize(update(bpc, maxiter=40))
    return bpc


def _bmps_call(bpc: BeliefPropagationCache, partition_by: str, mps_bond_dimension: int, message_update_kwargs, obs, want_norm: bool, info):
    """one tnqs_expect_bmps call; obs: [(verts, matrices)]; returns (numer / denom pairs as an (n, 2) complex array, log norm^2 or None)"""
    g = bpc.graph
    kw = dict(message_update_kwargs or {})
    unknown = set(kw) - {"niters", "tolerance", "normalize"}
    if unknown:
        raise L.TnqsArgumentError(f"boundarymps: unknown message_update_kwargs {sorted(unknown)}")
    tol = kw.get("tolerance", float("nan"))           # absent: default_tolerance of the element type; None: no tolerance
    o = L.BmpsOpts(0 if partition_by == "row" else 1, int(mps_bond_dimension), int(kw.get("niters", 50)), -1.0 if tol is None else float(tol), 1 if kw.get("normalize", True) else 0)
    _, rp = L.i32([v[0] for v in g.vertices]); _, cp = L.i32([v[1] for v in g.vertices])
    nv_, nvp = L.i32([len(vs) for vs, _ in obs] or [0]); ov, ovp = L.i32([g.index[v] for vs, _ in obs for v in vs] or [0])
    mats = [np.asarray(m, dtype=np.complex128).ravel(order="F") for _, ms in obs for m in ms]
    flat = np.ascontiguousarray(np.concatenate(mats)) if mats else np.zeros(1, dtype=np.complex128)
    out = np.zeros((max(len(obs), 1), 2), dtype=np.complex128)
    lg = np.zeros(2, dtype=np.float64)
    nq = 2 * (len({(v[0] if partition_by == "row" else v[1]) for v in g.vertices}) - 1)
    sweeps = np.zeros(max(nq, 1), dtype=np.int32); eps = np.zeros(max(nq, 1), dtype=np.float64)
    DP = C.POINTER(C.c_double)
    L.check(L.lib.tnqs_expect_bmps(bpc._h, C.byref(o), rp, cp, len(obs), nvp, ovp, flat.ctypes.data_as(DP), out.ctypes.data_as(DP),
                                   lg.ctypes.data_as(DP) if want_norm else None, sweeps.ctypes.data_as(C.POINTER(C.c_int32)), eps.ctypes.data_as(DP)))
    if info is not None:
        info.update(partition_by=partition_by, fit_sweeps=sweeps[:nq].copy(), fit_eps=eps[:nq].copy())
        if want_norm:
            info.update(log_norm_sqr=complex(lg[0], lg[1]))
    return out[:len(obs)], (complex(lg[0], lg[1]) if want_norm else None)


def _expect_bmps(x, observable, mps_bond_dimension, partition_by, gauge_state, message_update_kwargs, device, info):
    """expect(alg"boundarymps", psi, obs; mps_bond_dimension, partition_by, gauge_state) (src/expect.jl:84-156): every observable of the call in one device call"""
    if not isinstance(x, (TensorNetworkState, BeliefPropagationCache)):
        raise TypeError("expect: expected a TensorNetworkState or a BeliefPropagationCache")
    if mps_bond_dimension is None:
        raise L.TnqsArgumentError('expect: alg = "boundarymps" needs mps_bond_dimension')
    g = x.graph
    many = isinstance(observable, list)
    collected = [_collect_observable(o, g) for o in (observable if many else [observable])]
    by = boundarymps_partitioning(observable, g) if partition_by is None else partition_by
    part = _bmps_check_format(g, by)
    dims = dict(zip(g.vertices, _site_dims_of(x)))
    obs, slot = [], []
    for op, verts, coeff in collected:
        for v in verts:
            if v not in g.index:
                raise L.TnqsArgumentError(f"expect: {v!r} is not a vertex of the graph")
        ops = _observable_ops(op, verts)
        if len({part[v] for v in verts}) != 1:
            raise L.TnqsArgumentError("Observable support must be within a single partition (row/ column) of the graph for now.")
        if len(set(verts)) != len(verts):
            raise L.TnqsArgumentError("expect: a vertex appears twice in an observable")
        if coeff == 0:
            slot.append(None)                          # iszero(coeff) && return zero(coeff) (expect.jl:91)
            continue
        mats = []
        for v, o_ in zip(verts, ops):
            m = np.asarray(gate_matrix(o_) if isinstance(o_, str) else o_, dtype=np.complex128)
            if m.shape != (dims[v], dims[v]):
                raise L.TnqsArgumentError(f"expect: the operator on {v!r} is not a {dims[v]} x {dims[v]} matrix")
            mats.append(m)
        slot.append(len(obs)); obs.append((verts, mats))
    bpc = _bmps_handle(x, gauge_state, device, "expect")
    nd = _bmps_call(bpc, by, mps_bond_dimension, message_update_kwargs, obs, False, info)[0] if obs else None
    res = [0.0 * c if k is None else c * nd[k, 0] / nd[k, 1] for (_, _, c), k in zip(collected, slot)]
    return res if many else res[0]


def expect(x, observable, alg: str = "bp", mps_bond_dimension: Optional[int] = None, partition_by: Optional[str] = None, gauge_state: bool = True,
           message_update_kwargs: Optional[dict] = None, device: int = 0, info: Optional[dict] = None):
    """expect(alg"bp", cache, obs) for single-site observables (src/expect.jl:59-82); a list of observables returns
    a list (:114-121).
    alg = "boundarymps" (src/expect.jl:84-156): x is a TensorNetworkState on an open rectangular grid (vertices (row, column)), uploaded to a temporary handle on `device`
    and, with gauge_state, first taken through gauge_and_scale (BP with maxiter = 40, rescale, symmetric gauge); or a BeliefPropagationCache, whose network is used as it
    stands (its messages are neither read nor changed, gauge_state does not apply).  mps_bond_dimension is required; partition_by ("row" / "col") is inferred from the
    observables when omitted (row preferred); message_update_kwargs: niters (50), tolerance (default_tolerance of the element type; None: none), normalize (True).  All
    observables of the call are measured in ONE device call; info (optional dict) receives partition_by, fit_sweeps and fit_eps (one entry per directed pair of
    neighbouring partitions: p -> p + 1 first, then p + 1 -> p)."""
    if alg == "boundarymps":
        return _expect_bmps(x, observable, mps_bond_dimension, partition_by, gauge_state, message_update_kwargs, device, info)
    if alg != "bp":
        raise L.TnqsError(f'expect: algorithm choice not supported; supported on the HIP path: "bp" and "boundarymps" (received {alg!r})')
    bpc = x
    if isinstance(observable, list):
        return [expect(bpc, o) for o in observable]
    op, verts, coeff = _collect_observable(observable, bpc.graph)
    if coeff == 0:
        return 0.0 * coeff
    if len(verts) != 1:
        return coeff * _expect_region(bpc, op, verts)
    m = np.asfortranarray(gate_matrix(op) if isinstance(op, str) else np.asarray(op), dtype=np.complex128)
    out = (C.c_double * 2)()
    L.check(L.lib.tnqs_expect_1site(bpc._h, bpc.graph.index[verts[0]], m.ctypes.data_as(C.POINTER(C.c_double)), out))
    return coeff * complex(out[0], out[1])


def _expect_region(bpc: BeliefPropagationCache, op, verts) -> complex:
    """multi-site observable (src/expect.jl:59-82): operators on `verts`, identities on the rest of their Steiner tree, the
    cache's messages on the region's boundary; numerator / denominator"""
    from .graphs import steiner_region
    g = bpc.graph
    if isinstance(op, str):
        ops = [c for c in op]                       # one Pauli character per vertex (collectobservable, expect.jl:159-175)
    else:
        ops = list(op)
    if len(ops) != len(verts):
        raise L.TnqsError("Invalid observable: need as many operators as vertices passed.")
    try:
        region, parent = steiner_region(g, verts)
    except ValueError as e:
        raise L.TnqsError(str(e))
    opmap = {v: o for v, o in zip(verts, ops)}
    mats = []
    for v in region:
        d = bpc._site_dim(v)
        o = opmap.get(v)
        m = np.eye(d) if o is None else (gate_matrix(o) if isinstance(o, str) else np.asarray(o))
        mats.append(np.asarray(m, dtype=np.complex128).ravel(order="F"))
    flat = np.ascontiguousarray(np.concatenate(mats))
    rv, rvp = L.i32([g.index[v] for v in region]); pa, pap = L.i32(parent)
    out = (C.c_double * 4)()
    L.check(L.lib.tnqs_expect_region(bpc._h, len(region), rvp, pap, flat.ctypes.data_as(C.POINTER(C.c_double)), out))
    return complex(out[0], out[1]) / complex(out[2], out[3])


def expect_all(bpc: BeliefPropagationCache, op) -> np.ndarray:
    """<op_v> for every vertex in one batched launch (the per-layer probe of examples/2dIsing_dynamics.jl:60)"""
    g = bpc.graph
    mats = []
    for v in g.vertices:
        m = gate_matrix(op) if isinstance(op, str) else np.asarray(op)
        mats.append(np.asarray(m, dtype=np.complex128).ravel(order="F"))
    ops = np.ascontiguousarray(np.concatenate(mats))
    out = np.zeros(g.nv(), dtype=np.complex128)
    L.check(L.lib.tnqs_expect_all(bpc._h, ops.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


# ---- BP scalars and normalisation ------------------------------------------------------------
def vertex_scalars(bpc: BeliefPropagationCache) -> np.ndarray:
    """vertex_scalars (abstractbeliefpropagationcache.jl:22-28,134-138): tr(rho_v) for every vertex (NaN for other ranks' vertices)"""
    out = np.zeros(bpc.graph.nv(), dtype=np.complex128)
    L.check(L.lib.tnqs_vertex_scalars(bpc._h, out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def edge_scalars(bpc: BeliefPropagationCache) -> np.ndarray:
    """edge_scalars (beliefpropagationcache.jl:47-49, abstract...:140-144), in the order of `bpc.graph.edges`"""
    out = np.zeros(bpc.graph.ne(), dtype=np.complex128)
    L.check(L.lib.tnqs_edge_scalars(bpc._h, out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def freenergy(bpc: BeliefPropagationCache) -> complex:
    """freenergy (abstract...:289-300): sum log(vertex scalars) - sum log(edge scalars); -inf when an edge scalar is zero"""
    num, den = vertex_scalars(bpc), edge_scalars(bpc)
    if np.any(den == 0):
        return -np.inf
    f = np.sum(np.log(num.astype(np.complex128))) - np.sum(np.log(den.astype(np.complex128)))
    return complex(f)


def partitionfunction(bpc: BeliefPropagationCache) -> complex:
    """partitionfunction (abstract...:302-304) = exp(freenergy): the BP estimate of <psi|psi>"""
    return complex(np.exp(freenergy(bpc)))


def rescale(bpc: BeliefPropagationCache) -> BeliefPropagationCache:
    """rescale (abstract...:324-328): copy, rescale_messages! then rescale_vertices! -- every vertex / edge scalar becomes 1"""
    out = bpc.copy()
    L.check(L.lib.tnqs_rescale(out._h))
    return out


def rescale_messages(bpc: BeliefPropagationCache, edges=None) -> BeliefPropagationCache:
    """rescale_messages!(bpc, edges) on a copy (beliefpropagationcache.jl:127-140): each listed edge's two messages are normalised and
    divided by sqrt of their overlap, so that the edge scalar becomes 1; edges = None: every edge (abstract...:310-312)"""
    out = bpc.copy()
    if edges is None:
        L.check(L.lib.tnqs_rescale_messages(out._h, 0, None, None))
    else:
        g = bpc.graph
        (_, eup), (_, evp) = L.i32([g.index[a] for (a, b) in edges]), L.i32([g.index[b] for (a, b) in edges])
        L.check(L.lib.tnqs_rescale_messages(out._h, len(edges), eup, evp))
    return out


def rescale_vertices(bpc: BeliefPropagationCache, vertices=None) -> BeliefPropagationCache:
    """rescale_vertices!(bpc, vertices) on a copy (beliefpropagationcache.jl:82-101): psi_v *= sign(vn) / sqrt(vn) with vn the vertex
    scalar under the cache's current messages; vertices = None: every vertex (abstract...:314-316)"""
    out = bpc.copy()
    if vertices is None:
        L.check(L.lib.tnqs_rescale_vertices(out._h, 0, None))
    else:
        _, vp = L.i32([bpc.graph.index[v] for v in vertices])
        L.check(L.lib.tnqs_rescale_vertices(out._h, len(vertices), vp))
    return out


def normalize(tns: TensorNetworkState, alg: str = "bp", cache_update_kwargs=None, device: int = 0) -> TensorNetworkState:
    """normalize(tns; alg = "bp") (src/normalize.jl:1-6): BP-converge, rescale!, return the network (norm_sqr(bp) = 1)"""
    if alg != "bp":
        raise L.TnqsError(f"normalize: only alg = \"bp\" is implemented on the HIP path; received {alg!r}")
    bpc = BeliefPropagationCache(tns, device=device)
    bpc = update(bpc, **(bpc.default_bp_update_kwargs() if cache_update_kwargs is None else cache_update_kwargs))
    return rescale(bpc).network()


def symmetric_gauge(x, regularization: Optional[float] = None, cache_update_kwargs=None, device: int = 0):
    """symmetric_gauge (src/symmetric_gauge.jl:58-68): for a cache, a gauged COPY (messages become diag(S) on every edge); for a
    TensorNetworkState, BP-update first (default maxiter = 40) and return the gauged network"""
    reg = -1.0 if regularization is None else float(regularization)
    if isinstance(x, TensorNetworkState):
        bpc = update(BeliefPropagationCache(x, device=device), **(cache_update_kwargs if cache_update_kwargs is not None else dict(maxiter=40)))
        L.check(L.lib.tnqs_symmetric_gauge(bpc._h, reg))
        return bpc.network()
    out = x.copy()
    L.check(L.lib.tnqs_symmetric_gauge(out._h, reg))
    return out


def symmetrize_and_normalize(bpc: BeliefPropagationCache, regularization: Optional[float] = None) -> BeliefPropagationCache:
    """symmetrize_and_normalize (symmetric_gauge.jl:70-74): rescale, then symmetric gauge"""
    return symmetric_gauge(rescale(bpc), regularization=regularization)


# ---- loop corrections (src/MessagePassing/loopcorrection.jl, src/norm_sqr.jl) -------------------------------------
HOST_CONTRACTION_LIMIT = 2 ** 24      # a configuration is contracted on the host only while every intermediate stays BELOW this many elements


def loop_weights(bpc: BeliefPropagationCache, cycles) -> np.ndarray:
    """W(c) = Tr prod_k (A_k T_k) of simple cycles (vertex lists, consecutive vertices and the closing pair neighbours) on the device, in one
    call (tnqs_loop_weights); `bpc` must be rescaled for these to be the weights of the loop series"""
    g = bpc.graph
    out = np.zeros(len(cycles), dtype=np.complex128)
    ln, lnp = L.i32([len(c) for c in cycles] or [0])
    vs, vsp = L.i32([g.index[v] for c in cycles for v in c] or [0])
    L.check(L.lib.tnqs_loop_weights(bpc._h, len(cycles), lnp, vsp, out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def configuration_weights(bpc: BeliefPropagationCache, configurations) -> np.ndarray:
    """W(c) of connected leafless configurations (lists of edges) with at most two independent loops -- simple cycles, thetas, dumbbells, figure-eights -- on the
    device, in one call (tnqs_config_weights); `bpc` must be rescaled for these to be the weights of the loop series.  Order and orientation of a
    configuration's edges do not matter.  Three or more independent loops: TnqsError (unsupported)."""
    g = bpc.graph
    configurations = [list(c) for c in configurations]
    out = np.zeros(len(configurations), dtype=np.complex128)
    try:
        eu = [g.index[a] for c in configurations for (a, b) in c]
        ev = [g.index[b] for c in configurations for (a, b) in c]
    except KeyError as e:
        raise L.TnqsArgumentError(f"configuration_weights: {e.args[0]!r} is not a vertex of the graph") from None
    ln, lnp = L.i32([len(c) for c in configurations] or [0])
    us, usp = L.i32(eu or [0])
    vs, vsp = L.i32(ev or [0])
    L.check(L.lib.tnqs_config_weights(bpc._h, len(configurations), lnp, usp, vsp, out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def _independent_loops(edges) -> int:
    return len(edges) - len({v for e in edges for v in e}) + 1


def _check_branched(branched, who: str):
    if branched not in ("host", "device"):
        raise L.TnqsArgumentError(f'{who}: branched must be "host" or "device" (received {branched!r})')


def _cycle_order(edges):
    """the vertices of a simple cycle, given as its edge set, in ring order (None: some vertex has another degree than 2)"""
    nb: Dict = {}
    for (a, b) in edges:
        nb.setdefault(a, []).append(b); nb.setdefault(b, []).append(a)
    if any(len(x) != 2 for x in nb.values()):
        return None
    start = edges[0][0]
    ring, prev, cur = [start], None, start
    while True:
        nxt = nb[cur][0] if nb[cur][0] != prev else nb[cur][1]
        if nxt == start:
            return ring
        ring.append(nxt); prev, cur = cur, nxt


def _host_plan(bpc: BeliefPropagationCache, edges):
    """einsum operands (as shapes) and index lists of the configuration `edges`: per vertex the ket and the bra, per leg outside the configuration
    the incoming message, per edge of the configuration its antiprojector (loopcorrection.jl:79-89)"""
    g = bpc.graph
    inside = {frozenset(e) for e in edges}
    verts = sorted({v for e in edges for v in e}, key=g.index.__getitem__)
    label: Dict = {}

    def ix(*key):
        return label.setdefault(key, len(label))
    ops = []          # (kind, payload, shape, indices)
    for v in verts:
        nbs = g.neighbors(v)
        shape = (bpc._site_dim(v),) + tuple(bpc.bond_dim(v, w) for w in nbs)
        ops.append(("ket", v, shape, [ix("s", v)] + [ix("k", v, w) for w in nbs]))
        ops.append(("bra", v, shape, [ix("s", v)] + [ix("b", v, w) for w in nbs]))
        for w in nbs:
            if frozenset((v, w)) not in inside:
                chi = bpc.bond_dim(v, w)
                ops.append(("msg", (w, v), (chi, chi), [ix("k", v, w), ix("b", v, w)]))
    for (u, v) in edges:
        chi = bpc.bond_dim(u, v)
        ops.append(("anti", (u, v), (chi,) * 4, [ix("k", u, v), ix("b", u, v), ix("k", v, u), ix("b", v, u)]))
    return ops, len(label)


def _largest_intermediate(ops, path) -> int:
    """largest intermediate (elements) of a pairwise contraction path as np.einsum_path returns it"""
    dims: Dict[int, int] = {}
    for (_, _, shape, idx) in ops:
        dims.update(zip(idx, shape))
    cur = [frozenset(idx) for (_, _, _, idx) in ops]
    worst = 1
    for step in path:
        taken = [cur[q] for q in step]
        cur = [c for q, c in enumerate(cur) if q not in step]
        rest = frozenset().union(*cur) if cur else frozenset()
        res = frozenset(i for t in taken for i in t if i in rest)
        worst = max(worst, int(np.prod([dims[i] for i in res], dtype=np.float64)) if res else 1)
        cur.append(res)
    return worst


def _host_weight(bpc: BeliefPropagationCache, edges) -> complex:
    """weight of a connected configuration that is not a simple cycle (a vertex of internal degree >= 3), contracted in complex128 on the host"""
    ops, nlabels = _host_plan(bpc, edges)
    if nlabels > 52:
        raise L.TnqsError(f"loopcorrected_partitionfunction: configuration {tuple(edges)} has {nlabels} indices; the host contraction takes at most 52")
    # the path and its largest intermediate from the shapes alone (zero-stride stand-ins: nothing is read back or allocated before the check)
    fake = [np.lib.stride_tricks.as_strided(np.zeros(1), shape=sh, strides=(0,) * len(sh)) for (_, _, sh, _) in ops]
    args = [x for f, (_, _, _, idx) in zip(fake, ops) for x in (f, idx)]
    # numpy's greedy search only takes pairwise steps within the element limit it is given; what it cannot place is left as ONE step over all remaining
    # operands (a naive nested loop): such a step means the limit cannot be kept
    path = np.einsum_path(*args, [], optimize=("greedy", HOST_CONTRACTION_LIMIT - 1))[0][1:]
    big = _largest_intermediate(ops, path)
    if big >= HOST_CONTRACTION_LIMIT or any(len(step) > 2 for step in path):
        big = max(big, HOST_CONTRACTION_LIMIT)
        raise L.TnqsError(f"loopcorrected_partitionfunction: configuration {tuple(edges)} is not a simple cycle and its host contraction needs an intermediate "
                          f"of at least {big} elements; intermediates must stay below {HOST_CONTRACTION_LIMIT} (2^24)")
    real = []
    for (kind, what, sh, idx) in ops:
        if kind == "ket":
            t = bpc.tensor(what).astype(np.complex128)
        elif kind == "bra":
            t = np.conj(bpc.tensor(what).astype(np.complex128))
        elif kind == "msg":
            t = bpc.message(what).astype(np.complex128)
        else:
            u, v = what
            chi = sh[0]
            eye = np.eye(chi)
            # u's side pairs with the message INTO u, v's side with the message into v (bilinear)
            t = np.einsum("ac,bd->abcd", eye, eye) - np.einsum("ab,cd->abcd", bpc.message((v, u)).astype(np.complex128), bpc.message((u, v)).astype(np.complex128))
        real += [t, idx]
    return complex(np.einsum(*real, [], optimize=["einsum_path"] + list(path)))


def loopcorrected_partitionfunction(bpc: BeliefPropagationCache, max_configuration_size: int, connected_only: bool = False, branched: str = "host") -> complex:
    """loopcorrected_partitionfunction (loopcorrection.jl:3-14): Z_bp (1 + sum_c W(c)) over the leafless edge-induced subgraphs c of at most
    `max_configuration_size` edges, on a rescaled copy of the cache.  A disconnected configuration weighs the product of its components' weights
    (`connected_only` leaves those out: DESIGN.md section 5 on what the reference's enumeration is not pinned to).  Simple cycles are weighed on the
    device in one call; a connected configuration with a vertex of internal degree >= 3 is contracted on the host (_host_weight) -- or, with
    branched = "device", on the device together with the cycles (configuration_weights) when it has two independent loops; components with three or more
    independent loops stay on the host path with its limit."""
    _check_branched(branched, "loopcorrected_partitionfunction")
    zbp = partitionfunction(bpc)
    configs = leafless_edge_induced_subgraphs(bpc.graph, max_configuration_size, connected_only=connected_only)
    if not configs:
        return zbp
    r = rescale(bpc)
    parts = [connected_edge_components(c) for c in configs]
    weight: Dict = {}
    cycles, keys = [], []
    comps = list(dict.fromkeys(c for p in parts for c in p))
    if branched == "device":
        on_device = [c for c in comps if _independent_loops(c) <= 2]
        for k, w in zip(on_device, configuration_weights(r, on_device) if on_device else []):
            weight[k] = complex(w)
        comps = [c for c in comps if c not in weight]
    for comp in comps:
        ring = _cycle_order(comp)
        if ring is None:
            weight[comp] = _host_weight(r, comp)
        else:
            cycles.append(ring); keys.append(comp)
    if cycles:
        for k, w in zip(keys, loop_weights(r, cycles)):
            weight[k] = complex(w)
    total = sum(complex(np.prod([weight[c] for c in p])) for p in parts)
    return zbp * (1 + total)


def norm_sqr(x, alg: str, max_configuration_size: Optional[int] = None, cache_update_kwargs: Optional[dict] = None, device: int = 0,
             branched: str = "host", mps_bond_dimension: Optional[int] = None, partition_by: str = "row", message_update_kwargs: Optional[dict] = None,
             info: Optional[dict] = None) -> complex:
    """norm_sqr(psi; alg) (src/norm_sqr.jl:10-18,62-91) for alg = "bp", "loopcorrections" and "boundarymps".  x: a TensorNetworkState (a cache is built and
    updated with cache_update_kwargs, default default_bp_update_kwargs, on `device`) or an updated BeliefPropagationCache (which stays on its own device: `device` is not used).
    branched ("host" / "device"): where loopcorrected_partitionfunction weighs configurations with two independent loops.
    alg = "boundarymps" (:86-91): mps_bond_dimension is required, partition_by defaults to "row", message_update_kwargs as `expect` takes them; the state is not gauged and a
    cache's messages are neither read nor changed; one device call; info (optional dict) receives log_norm_sqr (the complex logarithm the result is the exp of), fit_sweeps, fit_eps."""
    _check_branched(branched, "norm_sqr")
    if alg == "boundarymps":
        if not isinstance(x, (TensorNetworkState, BeliefPropagationCache)):
            raise TypeError("norm_sqr: expected a TensorNetworkState or a BeliefPropagationCache")
        if mps_bond_dimension is None:
            raise L.TnqsArgumentError('norm_sqr: alg = "boundarymps" needs mps_bond_dimension')
        _bmps_check_format(x.graph, partition_by)
        bpc = _bmps_handle(x, False, device, "norm_sqr")
        return complex(np.exp(_bmps_call(bpc, partition_by, mps_bond_dimension, message_update_kwargs, [], True, info)[1]))
    if alg not in ("bp", "loopcorrections"):
        raise L.TnqsError(f'norm_sqr: algorithm choice not supported; supported on the HIP path: "bp" and "loopcorrections", and "boundarymps" on open rectangular grids (received {alg!r})')
    if alg == "loopcorrections" and max_configuration_size is None:
        raise L.TnqsArgumentError('norm_sqr: alg = "loopcorrections" needs max_configuration_size')
    if isinstance(x, TensorNetworkState):
        bpc = BeliefPropagationCache(x, device=device)
        bpc = update(bpc, **(bpc.default_bp_update_kwargs() if cache_update_kwargs is None else cache_update_kwargs))
    elif isinstance(x, BeliefPropagationCache):
        bpc = x
    else:
        raise TypeError("norm_sqr: expected a TensorNetworkState or a BeliefPropagationCache")
    if alg == "bp":
        return partitionfunction(bpc)
    return loopcorrected_partitionfunction(bpc, int(max_configuration_size), branched=branched)


def norm(x, alg: str, **kwargs) -> complex:
    """norm = sqrt(norm_sqr) (src/norm_sqr.jl:80-81); every keyword of norm_sqr, `branched` included"""
    return complex(np.sqrt(complex(norm_sqr(x, alg, **kwargs))))


def _site_dims_of(x) -> list:
    if isinstance(x, TensorNetworkState):
        return [x.tensors[v].shape[0] for v in x.graph.vertices]
    return [x._site_dim(v) for v in x.graph.vertices]


def log_inner(psi, phi, alg: str = "bp", cache_update_kwargs: Optional[dict] = None, device: int = 0, info: Optional[dict] = None) -> complex:
    """log of inner(psi, phi; alg = "bp") (src/inner.jl:65-69): belief propagation on BilinearForm(psi, phi), the reference's freenergy of the form cache -- a complex
    number whose imaginary part lies in (-pi, pi]; the overlap of two un-normalised states on a large lattice overflows a double, its log does not.  The conjugate is on
    the SECOND argument, sum psi conj(phi): the reference's docstring says <psi|phi>, its code builds bra = dag(prime(phi)), and the code is what this follows.
    psi, phi: a TensorNetworkState (uploaded to a temporary handle on `device`) or a BeliefPropagationCache, whose network is used as it stands on its handle -- nothing
    is uploaded, its own messages are neither read nor changed, and `device` is not used for it.  Same graph and site dimensions; bond dimensions are free per state.
    cache_update_kwargs: maxiter, tolerance, edge_sequence (and normalize) as `update` takes them; omitted: the reference's defaults for a bare `update` of the form
    cache -- maxiter 25 (1 on a tree), no tolerance, the default sequence.  info (optional dict) receives niter, diff and converged.  (-inf + 0j: the overlap is 0.)"""
    if alg != "bp":
        raise L.TnqsError(f'inner: algorithm choice not supported; supported on the HIP path: "bp" (received {alg!r})')
    for x in (psi, phi):
        if not isinstance(x, (TensorNetworkState, BeliefPropagationCache)):
            raise TypeError("inner: expected a TensorNetworkState or a BeliefPropagationCache")
    ga, gb = psi.graph, phi.graph
    if list(ga.vertices) != list(gb.vertices) or [tuple(e) for e in ga.edges] != [tuple(e) for e in gb.edges]:
        raise L.TnqsArgumentError("inner: the two states must live on the same graph (same vertices and edges in the same order)")
    if _site_dims_of(psi) != _site_dims_of(phi):
        raise L.TnqsArgumentError("inner: the two states must have the same site dimensions")
    if np.dtype(psi.dtype) != np.dtype(phi.dtype):
        raise L.TnqsArgumentError(f"inner: the two states must have the same element type (received {np.dtype(psi.dtype)} and {np.dtype(phi.dtype)})")
    o, keep = _bp_opts(ga, {} if cache_update_kwargs is None else cache_update_kwargs)
    ket = psi if isinstance(psi, BeliefPropagationCache) else BeliefPropagationCache(psi, device=device)
    bra = ket if phi is psi else (phi if isinstance(phi, BeliefPropagationCache) else BeliefPropagationCache(phi, device=device))
    out = np.zeros(2, dtype=np.float64)
    niter, diff = C.c_int(), C.c_double()
    L.check(L.lib.tnqs_inner_bp(ket._h, bra._h, C.byref(o), out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(niter), C.byref(diff)))
    if info is not None:
        info.update(niter=niter.value, diff=diff.value, converged=bool(o.tolerance >= 0 and diff.value <= o.tolerance))
    return complex(out[0], out[1])


def inner(psi, phi, alg: str = "bp", cache_update_kwargs: Optional[dict] = None, device: int = 0, info: Optional[dict] = None) -> complex:
    """inner(psi, phi; alg = "bp") = exp(log_inner(...)) = sum psi conj(phi) in the BP approximation (exact on trees); see log_inner for the arguments"""
    return complex(np.exp(log_inner(psi, phi, alg=alg, cache_update_kwargs=cache_update_kwargs, device=device, info=info)))


def _configs_of(graph, dims, bitstrings, who: str):
    """bitstrings -> ((B, nv) int32 array in graph.vertices order, single): a sequence of {vertex: int} dicts (what `sample` returns) or an integer array (B, nv);
    one dict or one row is a single string.  TnqsArgumentError for a missing vertex, a wrong width, a value that is no integer or lies outside 0 .. d_v - 1"""
    verts = list(graph.vertices)
    nv = len(verts)
    single = isinstance(bitstrings, dict)
    rows = [bitstrings] if single else bitstrings
    if single or (isinstance(rows, (list, tuple)) and len(rows) > 0 and all(isinstance(r, dict) for r in rows)):
        cfg = np.zeros((len(rows), nv), dtype=np.int64)
        for j, r in enumerate(rows):
            for i, v in enumerate(verts):
                if v not in r:
                    raise L.TnqsArgumentError(f"{who}: bitstring {j} has no value for vertex {v!r}")
                if int(r[v]) != r[v]:
                    raise L.TnqsArgumentError(f"{who}: the value of vertex {v!r} in bitstring {j} is not an integer ({r[v]!r})")
                cfg[j, i] = int(r[v])
    else:
        a = np.asarray(rows)
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise L.TnqsArgumentError(f"{who}: bitstrings are dicts {{vertex: int}} or an integer array (received dtype {a.dtype})")
        if a.ndim == 1 and a.size == nv and nv > 0:
            a, single = a.reshape(1, nv), True
        if a.ndim == 1 and a.size == 0:
            a = a.reshape(0, nv)
        if a.ndim != 2 or a.shape[1] != nv:
            raise L.TnqsArgumentError(f"{who}: an array of bitstrings has shape (B, number of vertices) = (B, {nv}); received {a.shape}")
        cfg = a.astype(np.int64)
    d = np.asarray(dims, dtype=np.int64).reshape(1, nv)
    bad = np.argwhere((cfg < 0) | (cfg >= d))
    if len(bad):
        j, i = (int(t) for t in bad[0])
        raise L.TnqsArgumentError(f"{who}: the value {int(cfg[j, i])} of vertex {verts[i]!r} in bitstring {j} is outside 0..{int(d[0, i]) - 1}")
    return np.ascontiguousarray(cfg, dtype=np.int32), single


def log_amplitudes(x, bitstrings, alg: str = "bp", cache_update_kwargs: Optional[dict] = None, device: int = 0, info: Optional[dict] = None):
    """log <x|psi> of a batch of bitstrings in one device call (tnqs_amplitudes_bp): belief propagation on the single-layer network T_v[x_v, ...] -- the reference's
    contract(tn; alg = "bp") (src/contract.jl:7-9) with vector messages that start as all ones, what certify_sample contracts per sample (src/sampling.jl:258-285); exact
    on trees.  Returns a complex128 array, one entry per string (imaginary parts in (-pi, pi]; -inf + 0j: the amplitude is exactly 0), or one complex number for a single
    string.  x: a TensorNetworkState (uploaded to a temporary handle on `device`) or a BeliefPropagationCache, whose network is used as it stands on its handle,
    un-normalised -- its own messages are neither read nor changed.  bitstrings: a sequence of {vertex: int} dicts, exactly what `sample` returns, or an integer array
    (B, nv) in graph.vertices order; one dict or one row gives a scalar.  cache_update_kwargs: maxiter, tolerance, edge_sequence (and normalize) as `inner` takes them;
    omitted: maxiter 25 (1 on a tree), no tolerance, the default sequence.  With a tolerance every string stops on its own, as if it had been the only one.  info
    (optional dict) receives the arrays niter, diff, converged and flags (bit 0: a vertex or edge scalar exactly zero, bit 1: a scalar not finite, the result then nan)."""
    if alg != "bp":
        raise L.TnqsError(f'amplitudes: algorithm choice not supported; supported on the HIP path: "bp" (received {alg!r})')
    if not isinstance(x, (TensorNetworkState, BeliefPropagationCache)):
        raise TypeError("amplitudes: expected a TensorNetworkState or a BeliefPropagationCache")
    g = x.graph
    cfg, single = _configs_of(g, _site_dims_of(x), bitstrings, "amplitudes")
    o, keep = _bp_opts(g, {} if cache_update_kwargs is None else cache_update_kwargs)
    bpc = x if isinstance(x, BeliefPropagationCache) else BeliefPropagationCache(x, device=device)
    nb = cfg.shape[0]
    out = np.zeros(2 * max(nb, 1), dtype=np.float64)
    niter, flags, diff = np.zeros(max(nb, 1), dtype=np.int32), np.zeros(max(nb, 1), dtype=np.int32), np.zeros(max(nb, 1), dtype=np.float64)
    L.check(L.lib.tnqs_amplitudes_bp(bpc._h, nb, cfg.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(o), out.ctypes.data_as(C.POINTER(C.c_double)),
                                     niter.ctypes.data_as(C.POINTER(C.c_int32)), diff.ctypes.data_as(C.POINTER(C.c_double)), flags.ctypes.data_as(C.POINTER(C.c_int32))))
    if info is not None:
        info.update(niter=niter[:nb].copy(), diff=diff[:nb].copy(), converged=(diff[:nb] <= o.tolerance) if o.tolerance >= 0 else np.zeros(nb, dtype=bool), flags=flags[:nb].copy())
    res = out[:2 * nb:2] + 1j * out[1:2 * nb:2]
    return complex(res[0]) if single else res


def amplitudes(x, bitstrings, alg: str = "bp", cache_update_kwargs: Optional[dict] = None, device: int = 0, info: Optional[dict] = None):
    """<x|psi> = exp(log_amplitudes(...)) in the BP approximation (exact on trees); see log_amplitudes for the arguments"""
    la = log_amplitudes(x, bitstrings, alg=alg, cache_update_kwargs=cache_update_kwargs, device=device, info=info)
    return complex(np.exp(la)) if isinstance(la, complex) else np.exp(la)


def log_probabilities(bpc, bitstrings, alg: str = "bp", cache_update_kwargs: Optional[dict] = None, device: int = 0, info: Optional[dict] = None):
    """log p(x) = 2 Re log <x|psi> - log norm_sqr(psi; alg = "bp"): the normalised BP probability of each string, the p that goes with the log q of
    sample_with_probabilities (p / q re-weighting, src/sampling.jl:258-285).  bpc: an updated BeliefPropagationCache (its messages give the norm) or a TensorNetworkState
    (a cache is built and updated with its defaults on `device`)."""
    if alg != "bp":
        raise L.TnqsError(f'amplitudes: algorithm choice not supported; supported on the HIP path: "bp" (received {alg!r})')
    if isinstance(bpc, TensorNetworkState):
        bpc = BeliefPropagationCache(bpc, device=device)
        bpc = update(bpc, **bpc.default_bp_update_kwargs())
    la = log_amplitudes(bpc, bitstrings, alg=alg, cache_update_kwargs=cache_update_kwargs, device=device, info=info)
    with np.errstate(divide="ignore"):
        ln = float(np.log(complex(norm_sqr(bpc, alg="bp"))).real)
    return 2 * la.real - ln


def site_probabilities(bpc: BeliefPropagationCache, v) -> np.ndarray:
    """p[s] = real(diag rho_v)[s] / tr rho_v under the cache's messages: the weights `sample` draws the configuration of v from"""
    out = np.zeros(bpc._site_dim(v), dtype=np.float64)
    L.check(L.lib.tnqs_site_probabilities(bpc._h, bpc.graph.index[v], out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def _check_sample_args(graph, nsamples, alg, uniforms):
    """the argument checks of `sample` that need no device"""
    if alg != "bp":
        raise L.TnqsError(f"sample: only alg = \"bp\" is implemented on the HIP path; received {alg!r}")
    if int(nsamples) != nsamples or nsamples < 0:
        raise L.TnqsArgumentError(f"sample: nsamples must be a non-negative integer; received {nsamples!r}")
    if uniforms is None:
        return None
    u = np.ascontiguousarray(uniforms, dtype=np.float64)
    if u.shape != (int(nsamples), graph.nv()):
        raise L.TnqsArgumentError(f"sample: uniforms must have shape (nsamples, number of vertices) = {(int(nsamples), graph.nv())}; received {u.shape}")
    if not np.all((u >= 0.0) & (u < 1.0)):
        raise L.TnqsArgumentError("sample: uniforms must lie in [0, 1)")
    return u


def sample_with_probabilities(x, nsamples: int, alg: str = "bp", bp_update_kwargs: Optional[dict] = None, gauge_state: bool = True,
                              seed: Optional[int] = None, uniforms=None, device: int = 0):
    """sample(alg"bp", psi, nsamples; bp_update_kwargs, gauge_state) (src/sampling.jl:3-46) -> (bitstrings, logq): a list of {vertex: int}
    dicts and, per sample, the log of the probability with which the sampler drew it (the sum of the logs of its step probabilities).
    x: a TensorNetworkState or a BeliefPropagationCache; either is updated first and, with gauge_state, put into the symmetric gauge
    (:11-14); then, per sample and vertex in vertex order: weights from rho_v, a draw, projection, BP update -- all on the device.
    bp_update_kwargs = None: default_bp_update_kwargs of the cache.  uniforms: (nsamples, nv) numbers in [0, 1) to draw with instead of
    the library's counter-based generator (seed; None: a fresh one from numpy)."""
    if not isinstance(x, (TensorNetworkState, BeliefPropagationCache)):
        raise TypeError("sample: expected a TensorNetworkState or a BeliefPropagationCache")
    u = _check_sample_args(x.graph, nsamples, alg, uniforms)
    nsamples = int(nsamples)
    bpc = BeliefPropagationCache(x, device=device) if isinstance(x, TensorNetworkState) else x
    g = bpc.graph
    kw = bpc.default_bp_update_kwargs() if bp_update_kwargs is None else bp_update_kwargs
    bpc = update(bpc, **kw)
    if gauge_state:
        bpc = symmetrize_and_normalize(bpc)
    bo, keep = _bp_opts(g, kw)
    nv = g.nv()
    cfg = np.zeros((max(nsamples, 1), nv), dtype=np.int32)
    prob = np.ones((max(nsamples, 1), nv), dtype=np.float64)
    st = L.ApplyStats()
    if seed is None:
        seed = int(np.random.default_rng().integers(0, 2 ** 63))
    L.check(L.lib.tnqs_sample_bp(bpc._h, nsamples, C.byref(bo), C.c_uint64(int(seed) & (2 ** 64 - 1)),
                                 None if u is None else u.ctypes.data_as(C.POINTER(C.c_double)), cfg.ctypes.data_as(C.POINTER(C.c_int32)),
                                 prob.ctypes.data_as(C.POINTER(C.c_double)), C.byref(st)))
    bitstrings = [{v: int(cfg[j, i]) for i, v in enumerate(g.vertices)} for j in range(nsamples)]
    with np.errstate(divide="ignore"):
        logq = np.log(prob[:nsamples]).sum(axis=1)
    return bitstrings, logq


def sample(x, nsamples: int, alg: str = "bp", bp_update_kwargs: Optional[dict] = None, gauge_state: bool = True, seed: Optional[int] = None,
           uniforms=None, device: int = 0):
    """sample(psi, nsamples; alg = "bp") (src/sampling.jl:3-46): a list of {vertex: int} dicts (see sample_with_probabilities)"""
    return sample_with_probabilities(x, nsamples, alg=alg, bp_update_kwargs=bp_update_kwargs, gauge_state=gauge_state, seed=seed,
                                     uniforms=uniforms, device=device)[0]


def profile_enable(bpc: BeliefPropagationCache, on: bool = True):
    L.check(L.lib.tnqs_profile_enable(bpc._h, 1 if on else 0))


PROF_CLASSES = ("bp_modeprod", "bp_gram", "gate_modeprod", "gate_gram", "gate_apply", "jacobi", "small", "bp_fused", "bp_pair", "bp_pairgram",
                # whole phases on the handle's stream (critical path; the kernel classes above overlap where a phase uses two streams): launches = sweeps / batches
                "phase_bp_update", "phase_gate_batch",
                # every launch of tnqs_loop_weights and tnqs_config_weights (loopcorrected_partitionfunction); flops = 8 m n k per complex product of the batched GEMM
                "loop",
                # the bond-contraction kernel of tnqs_rdm_edges (rdm_edges / expect_edges); its chains and Grams are booked under "small"
                "edge_rdm",
                # the apply kernel and the bond contractions of tnqs_rdm_paths (rdm_paths / rdm_pairs / expect_pairs / correlation_function); its transfer matrices
                # are booked under "loop", its chains and Grams under "small"
                "path_rdm")


def profile_get(bpc: BeliefPropagationCache) -> dict:
    out = {}
    for i, name in enumerate(PROF_CLASSES):
        n, ms, by, fl = C.c_int64(), C.c_double(), C.c_double(), C.c_double()
        L.check(L.lib.tnqs_profile_get(bpc._h, i, C.byref(n), C.byref(ms), C.byref(by), C.byref(fl)))
        out[name] = dict(launches=n.value, ms=ms.value, bytes=by.value, flops=fl.value)
    return out


def profile_reset(bpc: BeliefPropagationCache):
    L.check(L.lib.tnqs_profile_reset(bpc._h))
