"""GPU tests of boundary MPS (tnqs_expect_bmps, tn.expect / tn.norm_sqr with alg = "boundarymps"): the two kernels of csrc/kernels_bmps.hip through their debug entry
points, and the call end to end against the dense simulator on the cases tests/test_bmps_ref_cpu.py pins tests/bmps_ref.py on.

Tolerances (none of them measured on the kernels):
  contraction   per entry 8 u (K + nchunks) sum|a||b|, u = 2^-24 (f32 accumulation) / 2^-53, K the contracted length: the bound tests/test_gpu_inner.py derives for its Gram
  QR            ||Q^dagger Q - I||_max and ||Q Y - A||_max / ||A||_max at most 8 x what numpy.linalg.qr leaves at the same precision on the same input, floor 8 u m: the
                margin is for a different reduction order, not for a different algorithm
  end to end    every link at its full dimension, so the answer is the dense simulator's.  ComplexF32: 1e-5 on expectation values and on log norm^2 / (nv + ne), the bound
                the GPU suite holds everywhere.  ComplexF64: tests/bmps_ref.py itself sits at most 3.9e-16 from the dense simulator on these cases (measured by
                tests/test_bmps_ref_cpu.py, complex128 numpy); ten times that is below the floor of 1e-12, so the bound is 1e-12."""
import ctypes as C

import numpy as np
import pytest

import tnqs_amd as tn
import bmps_cases as cases

pytestmark = pytest.mark.gpu
lib = C.CDLL(tn.LIB_PATH)
L = tn.core.L
ERR_INVALID, ERR_UNSUPPORTED = -1, -2                    # include/tnqs.h
DT = {0: np.complex64, 1: np.complex128}
U = {0: 2.0 ** -24, 1: 2.0 ** -53}
GUARD = 7
SENTINEL = 777.0 - 555.0j
E2E_BOUND = {np.complex64: 1e-5, np.complex128: 1e-12}


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


# ---- the contraction kernel ------------------------------------------------------------------------------------------
# (dimension of every label, A's labels, B's labels, C's labels in the output's memory order, conj, pad: A's / B's fastest leg strided by 2)
CONTRACTIONS = [
    (dict(k=33, a=5, b=17, x=3), "kab", "xk", "axb", False, (True, False)),                       # permuted output, strided operand, two M tiles
    (dict(a=2, p=2, b=1, q=5, c=3, r=13, x=16, y=5), "apbqcr", "rxqpy", "xabcy", True, (False, True)),   # K = 130 over three legs, a leg of dimension 1, N = 80
    (dict(a=17, x=16), "a", "x", "ax", False, (False, False)),                                      # no contracted leg at all
    (dict(a=17, k=1, x=3), "ak", "kx", "xa", True, (False, False)),                                 # K = 1
    (dict(k=2, a=3, x=2), "ka", "xk", "ax", True, (False, False)),                                  # K = 2
    (dict(k=130), "k", "k", "", False, (False, False)),                                             # a scalar
    (dict(a=16, b=17, k=33, x=17, y=5), "abk", "kxy", "abxy", False, (False, False)),               # M = 272, N = 85: a grid of tiles with ragged edges
    (dict(a=3, b=2, c=5, d=2, k=2, l=3, m=2, n=3, w=2, x=3, y=2, z=2), "akblcmdn", "nwmxlykz", "wxyzabcd", True, (False, False)),      # four legs in every group
]


def _operand(rng, dims, labels, dt, pad):
    shape = tuple(dims[c] for c in labels)
    base = np.zeros(((2,) if pad else ()) + shape, dtype=dt, order="F")
    base[...] = (rng.standard_normal(base.shape) + 1j * rng.standard_normal(base.shape)).astype(dt)
    view = base[0] if pad else base
    strides = {c: view.strides[i] // view.itemsize for i, c in enumerate(labels)}
    return base, view, strides


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("force_chunks", [0, 3])
def test_contraction_kernel_mixed_shapes_in_one_launch(dtype, force_chunks):
    rng = np.random.default_rng(100 + dtype)
    dt = DT[dtype]
    ngroup, dimsv, stridesv, conjv, sizes, As, Bs, refs, bounds_in, cshapes = [], [], [], [], [], [], [], [], [], []
    for dims, la, lb, lc, conj, (pa, pb) in CONTRACTIONS:
        Abase, A, sa = _operand(rng, dims, la, dt, pa)
        Bbase, B, sb = _operand(rng, dims, lb, dt, pb)
        cshape = tuple(dims[c] for c in lc)
        cstr, acc = {}, 1
        for c in lc:
            cstr[c] = acc; acc *= dims[c]
        M = [c for c in la if c not in lb]; N = [c for c in lb if c not in la]; K = [c for c in la if c in lb]
        assert sorted(M + N) == sorted(lc)
        ngroup += [len(M), len(N), len(K)]
        d12 = [1] * 12; s24 = [0] * 24
        for q, c in enumerate(M):
            d12[q] = dims[c]; s24[q] = sa[c]; s24[4 + q] = cstr[c]
        for q, c in enumerate(N):
            d12[4 + q] = dims[c]; s24[8 + q] = sb[c]; s24[12 + q] = cstr[c]
        for q, c in enumerate(K):
            d12[8 + q] = dims[c]; s24[16 + q] = sa[c]; s24[20 + q] = sb[c]
        dimsv += d12; stridesv += s24; conjv.append(int(conj)); sizes += [Abase.size, Bbase.size, max(acc, 1)]
        As.append(Abase.ravel(order="F")); Bs.append(Bbase.ravel(order="F")); cshapes.append(cshape)
        Bx = B.conj() if conj else B
        spec = f"{la},{lb}->{lc}"
        refs.append(np.einsum(spec, A.astype(np.clongdouble), Bx.astype(np.clongdouble)))
        bounds_in.append((np.einsum(spec, np.abs(A).astype(np.float64), np.abs(B).astype(np.float64)), int(np.prod([dims[c] for c in K], dtype=np.int64))))
    out = np.full(GUARD + sum(int(np.prod(s, dtype=np.int64)) + GUARD for s in cshapes), SENTINEL, dtype=dt)
    nch = np.zeros(len(CONTRACTIONS), dtype=np.int32)
    rc = lib.tnqs_dbg_bmps_contract(dtype, len(CONTRACTIONS), _p(np.asarray(ngroup, dtype=np.int32)), _p(np.asarray(dimsv, dtype=np.int32)),
                                    _p(np.asarray(stridesv, dtype=np.int64)), _p(np.asarray(conjv, dtype=np.int32)), _p(np.asarray(sizes, dtype=np.int64)),
                                    _p(np.concatenate(As)), _p(np.concatenate(Bs)), _p(out), GUARD, force_chunks, _p(nch))
    assert rc == 0, L.lib.tnqs_last_error()
    if force_chunks:
        assert nch[1] == 3 and nch[5] == 3 and nch[2] == 1       # as many chunks as asked for where the range has the blocks
    off, worst = 0, 0.0
    for i, cshape in enumerate(cshapes):
        assert np.all(out[off:off + GUARD] == dt(SENTINEL)), f"guard in front of item {i}"
        off += GUARD
        n = int(np.prod(cshape, dtype=np.int64))
        got = out[off:off + n].reshape(cshape, order="F")
        off += n
        sab, K = bounds_in[i]
        bound = 8 * U[dtype] * (K + int(nch[i])) * sab
        err = np.abs(got.astype(np.clongdouble) - refs[i])
        worst = max(worst, float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny))))
        assert np.all(err <= bound), (i, float(err.max()), float(np.max(bound)))
    assert np.all(out[off:off + GUARD] == dt(SENTINEL))
    print(f"MEASURED bmps contraction dtype={dtype} force_chunks={force_chunks}: worst error / bound = {worst:.3f}, chunks = {nch.tolist()}")


def test_contraction_refuses_an_index_outside_its_array():
    one = np.ones(4, dtype=np.complex64); out = np.zeros(2 * GUARD + 4, dtype=np.complex64)
    args = (np.asarray([1, 1, 0], dtype=np.int32), np.asarray([2, 1, 1, 1, 2, 1, 1, 1, 1, 1, 1, 1], dtype=np.int32), np.zeros(24, dtype=np.int64),
            np.zeros(1, dtype=np.int32), np.asarray([2, 2, 4], dtype=np.int64))
    args[2][0] = 1; args[2][4] = 1; args[2][8] = 1; args[2][12] = 4      # the N leg's stride in C walks out of C
    rc = lib.tnqs_dbg_bmps_contract(0, 1, *[_p(a) for a in args], _p(one), _p(one), _p(out), GUARD, 0, None)
    assert rc == ERR_INVALID and not out.any()


# ---- the QR kernel ---------------------------------------------------------------------------------------------------
QR_SHAPES = [(1, 1), (4, 1), (8, 4), (36, 9), (64, 16), (256, 16), (1024, 32), (4096, 64)]
QR_DEFICIENT = [(8, 4), (64, 16), (256, 16)]


def _qr_inputs(dt):
    rng = np.random.default_rng(7)
    mats = [(rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(dt) for s in QR_SHAPES]
    for (m, n) in QR_DEFICIENT:
        mats.append(np.ones((m, n), dtype=dt))                       # the initial guess of a message: rank 1
        a = (rng.standard_normal((m, n)) + 1j * rng.standard_normal((m, n))).astype(dt)
        a[:, n - 1] = a[:, 0]                                        # two equal columns
        mats.append(a)
    return mats


def _qr_figures(Q, Y, A):
    Q, Y, A = Q.astype(np.clongdouble), Y.astype(np.clongdouble), A.astype(np.clongdouble)
    return float(np.abs(Q.conj().T @ Q - np.eye(Q.shape[1])).max()), float(np.abs(Q @ Y - A).max() / np.abs(A).max())


@pytest.mark.parametrize("dtype", [0, 1])
def test_qr_kernel_is_orthonormal_also_for_rank_deficient_input(dtype):
    dt = DT[dtype]
    mats = _qr_inputs(dt)
    m = np.asarray([a.shape[0] for a in mats], dtype=np.int32); n = np.asarray([a.shape[1] for a in mats], dtype=np.int32)
    rowmajor = np.asarray([i % 2 for i in range(len(mats))], dtype=np.int32)
    A = np.concatenate([a.ravel(order="C" if r else "F") for a, r in zip(mats, rowmajor)])
    Q = np.full(GUARD + sum(a.size + GUARD for a in mats), SENTINEL, dtype=dt)
    Y = np.full(GUARD + sum(a.shape[1] ** 2 + GUARD for a in mats), SENTINEL, dtype=dt)
    rc = lib.tnqs_dbg_bmps_qr(dtype, len(mats), _p(m), _p(n), _p(rowmajor), _p(A), _p(Q), _p(Y), GUARD)
    assert rc == 0, L.lib.tnqs_last_error()
    oq, oy = 0, 0
    for i, a in enumerate(mats):
        mi, ni = a.shape
        assert np.all(Q[oq:oq + GUARD] == dt(SENTINEL)) and np.all(Y[oy:oy + GUARD] == dt(SENTINEL))
        oq += GUARD; oy += GUARD
        q = Q[oq:oq + mi * ni].reshape((mi, ni), order="C" if rowmajor[i] else "F"); oq += mi * ni
        y = Y[oy:oy + ni * ni].reshape((ni, ni), order="F"); oy += ni * ni
        assert np.all(np.tril(y, -1) == 0)
        qn, yn = np.linalg.qr(a, mode="reduced")
        assert qn.dtype == dt
        (orth, res), (orth_np, res_np) = _qr_figures(q, y, a), _qr_figures(qn, yn, a)
        floor = 8 * U[dtype] * mi
        print(f"MEASURED bmps qr dtype={dtype} item {i} {mi}x{ni}: |Q^H Q - I| = {orth:.3e} (numpy {orth_np:.3e}), |QY - A| / |A| = {res:.3e} (numpy {res_np:.3e}), floor {floor:.3e}")
        assert orth <= max(8 * orth_np, floor) and res <= max(8 * res_np, floor), (i, a.shape)
    assert np.all(Q[oq:] == dt(SENTINEL)) and np.all(Y[oy:] == dt(SENTINEL))


def test_qr_refuses_shapes_outside_its_envelope():
    a = np.ones(65 * 65, dtype=np.complex64); q = np.zeros(65 * 65 + 2 * GUARD, dtype=np.complex64); y = q.copy()
    for (m, n) in [(65, 65), (3, 4)]:
        rc = lib.tnqs_dbg_bmps_qr(0, 1, _p(np.asarray([m], dtype=np.int32)), _p(np.asarray([n], dtype=np.int32)), _p(np.zeros(1, dtype=np.int32)), _p(a), _p(q), _p(y), GUARD)
        assert rc == ERR_UNSUPPORTED and not q.any() and not y.any()


# ---- end to end, every link at its full dimension --------------------------------------------------------------------
def _observables(obs):
    return [(list(ops), list(vs)) for vs, ops in obs]


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
@pytest.mark.parametrize("name", sorted(cases.EXACT_CASES))
def test_exact_regime_matches_the_dense_simulator(name, dt):
    g, tensors, R, by, obs, dense, log_n2 = cases.exact_case(name)
    psi = tn.TensorNetworkState(g, {v: t.astype(dt) for v, t in tensors.items()})
    info = {}
    got = tn.expect(psi, _observables(obs), alg="boundarymps", mps_bond_dimension=R, partition_by=by, gauge_state=False, info=info)
    bound = E2E_BOUND[dt]
    for (vs, _), a, b in zip(obs, got, dense):
        print(f"MEASURED bmps expect {name} {np.dtype(dt).name} {vs}: |device - dense| = {abs(a - b):.3e}")
        assert abs(a - b) <= bound
    assert info["partition_by"] == by
    P = len({(v[0] if by == "row" else v[1]) for v in g.vertices})
    assert len(info["fit_sweeps"]) == 2 * (P - 1) and info["fit_sweeps"].max() >= 2      # the fit runs more than one sweep: a tolerance cannot stop the first
    assert tn.expect(psi, _observables(obs)[0], alg="boundarymps", mps_bond_dimension=R, gauge_state=False) == pytest.approx(dense[0], abs=bound)      # partition_by inferred
    ninfo = {}
    n2 = tn.norm_sqr(psi, alg="boundarymps", mps_bond_dimension=R, partition_by=by, info=ninfo)
    nv, ne = len(g.vertices), len(g.edges)
    err = abs(ninfo["log_norm_sqr"] - log_n2) / (nv + ne)
    print(f"MEASURED bmps norm_sqr {name} {np.dtype(dt).name}: |log device - log dense| / (nv + ne) = {err:.3e}")
    assert err <= bound and n2 == pytest.approx(np.exp(ninfo["log_norm_sqr"]))
    assert tn.norm(psi, alg="boundarymps", mps_bond_dimension=R, partition_by=by) == pytest.approx(np.sqrt(n2))


def test_gauge_state_is_gauge_and_scale_on_the_device():
    """gauge_state = True takes a TensorNetworkState through BP with maxiter = 40, rescale and the symmetric gauge (src/symmetric_gauge.jl:76-83) by the existing device
    calls: the same launches on the same numbers as doing so by hand and handing the cache over, so the same bits; a cache is used as it stands"""
    g, tensors, R, by, obs, dense, _ = cases.exact_case("3x3_chi2_R4")
    psi = tn.TensorNetworkState(g, {v: t.astype(np.complex64) for v, t in tensors.items()})
    kw = dict(alg="boundarymps", mps_bond_dimension=R, partition_by=by)
    gauged = tn.symmetrize_and_normalize(tn.update(tn.BeliefPropagationCache(psi), maxiter=40))
    a = tn.expect(psi, _observables(obs), **kw)
    assert a == tn.expect(gauged, _observables(obs), **kw) == tn.expect(gauged, _observables(obs), gauge_state=False, **kw)
    for x, want in zip(a, dense):
        assert abs(x - want) <= 1e-5      # the gauge does not change the state


@pytest.mark.parametrize("dtype", [0, 1])
def test_the_entry_point_directly_without_a_tolerance(dtype):
    """tnqs_expect_bmps on a cache's handle: one sweep and no tolerance (no read-back before the last), numerators and denominators, the norm in the same call; the
    handle's tensors and messages are what they were"""
    g, tensors, R, by, obs, dense, log_n2 = cases.exact_case("3x4_chi2_R16_col")
    dt = DT[dtype]
    bpc = tn.update(tn.BeliefPropagationCache(tn.TensorNetworkState(g, {v: t.astype(dt) for v, t in tensors.items()})), maxiter=2)
    before = {v: bpc.tensor(v).copy() for v in g.vertices}; msg_before = bpc.message(((1, 1), (1, 2))).copy()
    o = L.BmpsOpts(1, R, 1, -1.0, 1)
    _, rp = L.i32([v[0] for v in g.vertices]); _, cp = L.i32([v[1] for v in g.vertices])
    _, nvp = L.i32([len(vs) for vs, _ in obs]); _, ovp = L.i32([g.index[v] for vs, _ in obs for v in vs])
    flat = np.concatenate([np.asarray(m, dtype=np.complex128).ravel(order="F") for _, ops in obs for m in ops])
    out = np.zeros((len(obs), 2), dtype=np.complex128); lg = np.zeros(2); sweeps = np.zeros(6, dtype=np.int32); eps = np.zeros(6)
    rc = lib.tnqs_expect_bmps(bpc._h, C.byref(o), rp, cp, len(obs), nvp, ovp, _p(flat), _p(out), _p(lg), _p(sweeps), _p(eps))
    assert rc == 0, L.lib.tnqs_last_error()
    bound = E2E_BOUND[dt]
    for k, want in enumerate(dense):
        assert abs(out[k, 0] / out[k, 1] - want) <= bound
    assert abs(complex(lg[0], lg[1]) - log_n2) / (len(g.vertices) + len(g.edges)) <= bound
    assert sweeps.tolist() == [1] * 6 and np.all(np.isfinite(eps)) and np.all(eps > 0)
    for v in g.vertices:
        assert np.array_equal(bpc.tensor(v), before[v])
    assert np.array_equal(bpc.message(((1, 1), (1, 2))), msg_before)


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_untouched():
    g = tn.named_grid((3, 3))
    psi = tn.random_tensornetworkstate(np.complex64, g, bond_dimension=2, seed=4)
    bpc = tn.BeliefPropagationCache(psi)
    before = {v: bpc.tensor(v).copy() for v in g.vertices}
    kw = dict(alg="boundarymps", mps_bond_dimension=4)
    with pytest.raises(tn.TnqsArgumentError, match="ring"):
        gp = tn.named_grid((4, 4), periodic=True)
        tn.expect(tn.random_tensornetworkstate(np.complex64, gp, bond_dimension=2, seed=1), ("Z", [(2, 2)]), **kw)
    with pytest.raises(tn.TnqsArgumentError, match="pseudo-edges"):
        gh = tn.heavy_hexagonal_lattice(2, 2)
        tn.norm_sqr(tn.random_tensornetworkstate(np.complex64, gh, bond_dimension=2, seed=1), **kw)
    with pytest.raises(tn.TnqsArgumentError, match="aligned in either the same column or the same row"):
        tn.expect(bpc, ("ZZ", [(1, 1), (2, 2)]), **kw)
    with pytest.raises(tn.TnqsArgumentError, match="single partition"):
        tn.expect(bpc, ("ZZ", [(1, 1), (2, 1)]), partition_by="row", **kw)
    with pytest.raises(tn.TnqsArgumentError, match="mps_bond_dimension"):
        tn.expect(bpc, ("Z", [(1, 1)]), alg="boundarymps")
    with pytest.raises(tn.TnqsArgumentError, match="mps_bond_dimension"):
        tn.norm_sqr(bpc, alg="boundarymps")
    with pytest.raises(tn.TnqsError, match="as many operators as vertices"):
        tn.expect(bpc, ("Z", [(1, 1), (1, 2)]), **kw)
    with pytest.raises(tn.TnqsError, match="algorithm choice not supported"):
        tn.expect(bpc, ("Z", [(1, 1)]), alg="exact")
    wide = tn.BeliefPropagationCache(tn.random_tensornetworkstate(np.complex64, tn.named_grid((2, 4)), bond_dimension=8, seed=2))
    with pytest.raises(tn.TnqsError, match="envelope"):      # the middle link of a row of four chi = 8 edges is min(64^2, 64^2, 65) = 65
        tn.expect(wide, ("Z", [(1, 1)]), alg="boundarymps", mps_bond_dimension=65)
    # ... while no link of the 3 x 3, chi = 2 network exceeds 4, whatever is asked for: taken, and the same fit as R = 4
    assert tn.expect(bpc, ("Z", [(1, 1)]), alg="boundarymps", mps_bond_dimension=65) == tn.expect(bpc, ("Z", [(1, 1)]), **kw)
    big = tn.BeliefPropagationCache(tn.random_tensornetworkstate(np.complex64, tn.named_grid((2, 2)), bond_dimension=9, seed=2))
    with pytest.raises(tn.TnqsError, match="envelope"):
        tn.norm_sqr(big, alg="boundarymps", mps_bond_dimension=17)
    for v in g.vertices:
        assert np.array_equal(bpc.tensor(v), before[v])
    assert tn.expect(bpc, ("Z", [(1, 1)])) == tn.expect(bpc, ("Z", [(1, 1)]), alg="bp")      # alg = "bp" is what it was


def test_error_codes_and_a_sharded_handle():
    """a two-rank handle on one GPU as tests/test_gpu_amplitudes.py sets it up: the callback is never reached"""
    g = tn.named_grid((2, 2))
    bpc = tn.BeliefPropagationCache(tn.random_tensornetworkstate(np.complex64, g, bond_dimension=2, seed=61))
    _, rp = L.i32([v[0] for v in g.vertices]); _, cp = L.i32([v[1] for v in g.vertices])
    lg = np.zeros(2)

    def call(opts, h=None):
        return lib.tnqs_expect_bmps((h or bpc)._h, C.byref(opts), rp, cp, 0, None, None, None, None, _p(lg), None, None)
    big = tn.BeliefPropagationCache(tn.random_tensornetworkstate(np.complex64, g, bond_dimension=9, seed=2))
    assert call(L.BmpsOpts(0, 17, 0, float("nan"), 1), big) == ERR_UNSUPPORTED and b"envelope" in L.lib.tnqs_last_error() and not lg.any()      # chi = 9: links up to 16, this one is 17
    assert call(L.BmpsOpts(0, 0, 0, float("nan"), 1)) == ERR_INVALID and not lg.any()
    assert call(L.BmpsOpts(2, 4, 0, float("nan"), 1)) == ERR_INVALID and not lg.any()
    assert call(L.BmpsOpts(0, 4, 0, float("nan"), 1)) == 0 and lg.any()
    lg[:] = 0
    buf = C.c_void_p()
    lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]; lib.hipFree.argtypes = [C.c_void_p]
    assert lib.hipMalloc(C.byref(buf), 1 << 16) == 0 and buf.value
    try:
        cb = L.ALLGATHER_FN(lambda ctx, base, nbytes, nranks: -1)
        owner, op = L.i32([0, 0, 1, 1])
        L.check(L.lib.tnqs_set_sharding(bpc._h, 0, 2, op, cb, None, buf, 1 << 16))
        assert call(L.BmpsOpts(0, 4, 0, float("nan"), 1)) == ERR_UNSUPPORTED and b"sharded" in L.lib.tnqs_last_error() and not lg.any()
        del bpc
    finally:
        lib.hipFree(buf)


# ---- end to end, truncated -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
@pytest.mark.parametrize("name", sorted(cases.truncated_cases()))
def test_truncated_regime_matches_the_converged_reference(name, dt):
    """4 x 4, R in {2, 4, 8}, gauge_state = True, default niters, a tolerance the fit stops by.  After a few sweeps the truncated result depends on how a QR completes the
    null space of the rank-deficient guess, so only converged values are compared: tests/bmps_truncated_select.py kept these states because every fit of tests/bmps_ref.py
    stops by tolerance under five seeded null-space completions, and recorded the spread of the five results per observable; the device may sit ten times that spread
    from the reference, floored at the exact-regime bound of its element type.  Tolerances: 1e-5 (ComplexF32), 1e-6 (ComplexF64; at 1e-8 no chi = 3 seed of twenty stopped
    before 50 sweeps).  Kept: chi = 2 seed 40, chi = 3 seed 41 (seed 40 ran into niters).  Largest bound over the three observables, 10 x spread, per (element type, R)
    (tests/golden/meta/bmps_truncated.json holds them per observable; tests/test_bmps_ref_cpu.py::test_truncated_cases_are_conditioned prints the table):
        chi = 2   ComplexF32  R = 2: 1.2e-2   R = 4: 1e-5 (floor)   R = 8: 3.8e-5      ComplexF64  R = 2: 4.1e-3   R = 4: 5.7e-9   R = 8: 2.5e-5
        chi = 3   ComplexF32  R = 2: 2.5e-2   R = 4: 6.5e-3         R = 8: 4.1e-3      ComplexF64  R = 2: 9.3e-3   R = 4: 2.2e-3   R = 8: 1.4e-3
    <I> has no spread: it is held to the floor.  What these bounds can see: the values are of order 0.1 .. 0.3, so the rows at 4e-3 .. 2.5e-2 (chi = 3 at every R, R = 2 at both chi) catch
    gross errors only -- on random states the fit converges slowly and to completion-dependent values, which the rule measures faithfully; the discriminating rows are chi = 2 at R = 4 and
    R = 8, and the exact-regime tests above carry the tight bounds."""
    e = cases.truncated_cases()[name]
    g, tensors = cases.grid_state((4, 4), e["chi"], 2, e["seed"])
    psi = tn.TensorNetworkState(g, {v: t.astype(dt) for v, t in tensors.items()})
    obs = [([cases.TRUNCATED_OPS[c] for c in ops], [tuple(v) for v in vs]) for vs, ops in e["observables"]]
    dense = np.asarray(e["dense_re"]) + 1j * np.asarray(e["dense_im"])
    floor, err_dense = E2E_BOUND[dt], {}
    for R in (2, 4, 8):
        run = e["runs"][f"{np.dtype(dt).name}_R{R}"]
        want = np.asarray(run["re"]) + 1j * np.asarray(run["im"])
        info = {}
        got = np.asarray(tn.expect(psi, obs, alg="boundarymps", mps_bond_dimension=R, gauge_state=True, message_update_kwargs=dict(tolerance=run["tolerance"]), info=info))
        fitted = info["fit_sweeps"][info["fit_sweeps"] > 0]      # the request needs four of the six messages; the others report 0 sweeps
        print(f"MEASURED bmps truncated {name} {np.dtype(dt).name} R={R}: sweeps of the fitted messages {fitted.tolist()} (reference {run['sweeps']})")
        assert info["partition_by"] == "row" and len(fitted) == 4 and fitted.min() >= 2
        for k, ops in enumerate(o for _, o in e["observables"]):
            bound = max(10 * run["spread"][k], floor)
            print(f"MEASURED bmps truncated {name} {np.dtype(dt).name} R={R} {ops}: |device - reference| = {abs(got[k] - want[k]):.3e} (bound {bound:.1e}), |device - dense| = {abs(got[k] - dense[k]):.3e}")
            assert abs(got[k] - want[k]) <= bound
            if ops == "I":
                assert abs(got[k] - 1) <= floor
        err_dense[R] = float(np.max(np.abs(got - dense)))
    assert err_dense[8] <= err_dense[2]
