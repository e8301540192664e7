"""Kernel-level GPU tests of the two kernels that produce every BP message of a small lattice -- bp_small_site_kernel<1024> (scalar and matrix-core form) and
msg_finalize_kernel<T> -- through tnqs_dbg_small_site / tnqs_dbg_msg_finalize (include/tnqs_debug.h), against the float64 reference of tests/small_site_ref.py
(pinned to the oracle in tests/test_small_site_ref_cpu.py).  Inputs detect transpositions: complex random tensors, complex random non-Hermitian messages, a
distinct matrix per leg.

Tolerances (none of them measured on the kernels):
  raw message      max|got - ref| / max|ref| < ref.raw_bound() = 4 x the worst error of the complex64 numpy restatement over the same cases (3.9e-6)
  normalised       the same bound divided by the conditioning |sum(ref)| / sum|ref| of the case, which is >= 0.1 by the choice of inputs
  message_diff     1e-12 absolute against the float64 formula on the kernel's OWN new_msg: four double sums of <= 1024 products of f32 values, 1024 x 2^-53 on f <= 1
  msg_finalize     the summation bound nchunks x eps x sum|partials| per element (eps = 2^-23 / 2^-52), carried through the division for normalised messages"""
import ctypes as C

import numpy as np
import pytest

import tnqs_amd as tn
import small_site_ref as ref

pytestmark = pytest.mark.gpu
lib = C.CDLL(tn.LIB_PATH)
ERR_UNSUPPORTED = -2                                     # include/tnqs.h
ROUTE_SCALAR, ROUTE_MFMA16 = 7, 8                        # include/tnqs_debug.h
SENTINEL = np.complex64(-7.5 + 3.25j)


def _ints(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.int32))


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _measured(kernel, err):
    print(f"MEASURED {kernel}: {err:.3e}")


def _item(d, chis, jo, present=None, tag=0, psd_like=False, scale=None):
    psi, Ms = ref.inputs(d, chis, tag=tag, psd_like=psd_like)
    if scale is not None:
        psi = (psi.astype(np.complex128) * scale).astype(np.complex64)
    present = tuple(present) if present is not None else (1,) * len(chis)
    return dict(d=d, chis=tuple(chis), jo=jo, psi=psi, Ms=Ms, present=present)


def _ref_raw(it):
    return ref.message(it["psi"], ref.masked(it["Ms"], it["present"]), it["jo"])


def small_site(items, form, olds=None, normalize=1, epilogue=False, expect_rc=0):
    """one tnqs_dbg_small_site call.  Returns (out, new, diff, route) per item; out and new_msg are pre-filled with SENTINEL, so whatever the call must leave
    alone is seen to be left alone.  olds: None or an array per item (None entries = identity)"""
    n = len(items)
    co = [it["chis"][it["jo"]] if 0 <= it["jo"] < len(it["chis"]) else 1 for it in items]
    psi = np.concatenate([ref.flat(it["psi"]) for it in items]).astype(np.complex64)
    M = np.concatenate([ref.flat(m) for it in items for m in it["Ms"]]).astype(np.complex64)
    present = _ints([p for it in items for p in it["present"]])
    off = np.concatenate([[0], np.cumsum([c * c for c in co])])
    out = np.full(off[-1], SENTINEL, dtype=np.complex64)
    new = np.full(off[-1], SENTINEL, dtype=np.complex64) if epilogue else None
    diff = np.full(n, -5.0) if epilogue else None
    old, has_old = None, None
    if olds is not None:
        old = np.zeros(off[-1], dtype=np.complex64); has_old = _ints([o is not None for o in olds])
        for i, o in enumerate(olds):
            if o is not None:
                old[off[i]:off[i + 1]] = ref.flat(o)
    route = _ints([0] * n)
    rc = lib.tnqs_dbg_small_site(n, _p(_ints([it["d"] for it in items])), _p(_ints([len(it["chis"]) for it in items])), _p(_ints([c for it in items for c in it["chis"]])),
                                 _p(_ints([it["jo"] for it in items])), _p(psi), _p(M), _p(present), form, _p(old), _p(has_old), normalize,
                                 _p(out), _p(new), _p(diff), _p(route))
    assert rc == expect_rc, (rc, lib.tnqs_last_error())
    if rc != 0:                                          # a refusal writes nothing
        assert np.all(out == SENTINEL) and (new is None or np.all(new == SENTINEL)) and (diff is None or np.all(diff == -5.0))
        return None
    res = []
    for i in range(n):
        o = ref.unflat(out[off[i]:off[i + 1]], co[i])
        w = ref.unflat(new[off[i]:off[i + 1]], co[i]) if epilogue else None
        res.append((o, w, diff[i] if epilogue else None, int(route[i])))
    if epilogue:
        assert np.all(out == SENTINEL)                   # with the epilogue the raw message goes nowhere the caller sees
    return res


def _check_raw(name, items, res, want_route=None):
    worst = 0.0
    for it, (o, _, _, route) in zip(items, res):
        assert np.all(np.isfinite(o)) and not np.any(o == SENTINEL)
        if want_route is not None:
            assert route == want_route
        worst = max(worst, ref.rel_err(o, _ref_raw(it)))
    _measured(name, worst)
    return worst


# ---- raw message, scalar form --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,chis,jo", ref.SCALAR_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_scalar_form_shape_sweep(d, chis, jo):
    """every leg of every shape as the outgoing one; the matrix of the outgoing leg is handed to the kernel as well and has to be ignored"""
    items = [_item(d, chis, jo)]
    for form in (0, -1):                                 # (the engine's rule gives the scalar form for all of these shapes)
        res = small_site(items, form)
        err = _check_raw(f"small_site scalar d {d} chi {chis} jo {jo} form {form}", items, res, ROUTE_SCALAR)
        assert err < ref.raw_bound()                     # measured 6.4e-7 at worst (d 2, legs (32, 4, 32), jo 2: 8192 elements)


@pytest.mark.parametrize("d,chis,present", ref.NULL_CASES, ids=lambda v: "".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_scalar_form_null_messages(d, chis, present):
    """every subset of present legs, every outgoing leg (one launch): a null matrix is the identity, none present gives psi^dagger psi over the rest"""
    items = [_item(d, chis, jo, present) for jo in range(len(chis))]
    if not any(present):
        for it in items:
            other = [a for a in range(it["psi"].ndim) if a != it["jo"] + 1]
            p = ref.r32(it["psi"])
            assert ref.rel_err(np.tensordot(p, p.conj(), axes=(other, other)), _ref_raw(it)) < 1e-14
    err = _check_raw(f"small_site scalar d {d} chi {chis} present {present}", items, small_site(items, 0), ROUTE_SCALAR)
    assert err < ref.raw_bound()                         # measured 1.9e-7


# ---- raw message, matrix-core form and the scalar form on the same inputs --------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,chis,present", ref.MFMA_CASES, ids=lambda v: "".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_matrix_core_form_and_scalar_form_on_16_dimensional_legs(d, chis, present):
    items = [_item(d, chis, jo, present) for jo in range(len(chis))]
    rm = small_site(items, 1)
    ra = small_site(items, -1)                           # the engine's rule picks the matrix-core form here
    rs = small_site(items, 0)
    em = _check_raw(f"small_site mfma16 d {d} z {len(chis)} present {present}", items, rm, ROUTE_MFMA16)
    es = _check_raw(f"small_site scalar d {d} z {len(chis)} all-16 present {present}", items, rs, ROUTE_SCALAR)
    assert em < ref.raw_bound() and es < ref.raw_bound()         # measured 2.8e-7 (matrix-core form), 3.8e-7 (scalar form)
    cross = 0.0
    for it, a, b, c in zip(items, rm, rs, ra):
        assert c[3] == ROUTE_MFMA16 and np.array_equal(a[0], c[0])
        cross = max(cross, ref.rel_err(a[0], b[0].astype(np.complex128)))
    _measured(f"small_site mfma16 against scalar d {d} z {len(chis)} present {present}", cross)
    assert cross < 2 * ref.raw_bound()                   # both within the bound of the same reference; measured 4.1e-7


# ---- one launch of many items -----------------------------------------------------------------------------------------------------------------------------------
def test_multi_item_launch_of_both_forms():
    items = [_item(d, chis, jo, present, tag=1) for d, chis, jo, present in ref.MULTI_ITEMS]
    sizes = [it["psi"].size for it in items]
    assert min(sizes) == 64 and max(sizes) == 8192 and sizes[0] < 8192 and sizes[-1] < 8192
    res = small_site(items, -1)
    routes = [r[3] for r in res]
    assert routes == [ROUTE_MFMA16 if set(it["chis"]) == {16} else ROUTE_SCALAR for it in items] and len(set(routes)) == 2
    for i, (it, r) in enumerate(zip(items, res)):        # every item on its own
        err = _check_raw(f"small_site multi-item launch item {i} ({'mfma16' if r[3] == ROUTE_MFMA16 else 'scalar'}, {sizes[i]} elements)", [it], [r])
        assert err < ref.raw_bound()                     # measured 5.2e-7 (the 8192-element scalar item)
    # the same launch with the epilogue: new_msg per item, `out` untouched (small_site asserts the sentinel)
    olds = [None if i % 2 else ref.crandn(np.random.default_rng(i), (it["chis"][it["jo"]],) * 2) for i, it in enumerate(items)]
    rese = small_site(items, -1, olds=olds, normalize=0, epilogue=True)
    for i, (it, r, old) in enumerate(zip(items, rese, olds)):
        want, _ = ref.finalize(_ref_raw(it), old, False)
        err = ref.rel_err(r[1], want)
        _measured(f"small_site multi-item launch with epilogue item {i}", err)
        assert err < ref.raw_bound()
        assert abs(r[2] - ref.message_diff(r[1], np.eye(want.shape[0]) if old is None else old)) < 1e-12


# ---- fused epilogue ---------------------------------------------------------------------------------------------------------------------------------------------
def msg_finalize(dtype, chis, nchunks, partials, olds, normalize):
    """one tnqs_dbg_msg_finalize call; partials[i]: array (nchunks[i], chi, chi); returns (new, diff) per item"""
    dt = np.complex64 if dtype == 0 else np.complex128
    n = len(chis)
    off = np.concatenate([[0], np.cumsum([c * c for c in chis])])
    P = np.concatenate([ref.flat(p[c]) for p in partials for c in range(p.shape[0])]).astype(dt)
    new = np.full(off[-1], SENTINEL, dtype=dt); diff = np.full(n, -5.0)
    old, has_old = None, None
    if olds is not None:
        old = np.zeros(off[-1], dtype=dt); has_old = _ints([o is not None for o in olds])
        for i, o in enumerate(olds):
            if o is not None:
                old[off[i]:off[i + 1]] = ref.flat(o)
    rc = lib.tnqs_dbg_msg_finalize(dtype, n, _p(_ints(chis)), _p(_ints(nchunks)), _p(P), _p(old), _p(has_old), normalize, _p(new), _p(diff))
    assert rc == 0, lib.tnqs_last_error()
    return [(ref.unflat(new[off[i]:off[i + 1]], chis[i]), diff[i]) for i in range(n)]


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("d,chis", ref.EPILOGUE_SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_fused_epilogue_against_finalize(d, chis, normalize):
    """new_msg against finalize(message(..)) in float64, message_diff against the float64 formula on the kernel's own new_msg; old: identity (null), an unrelated
    matrix, the f32-rounded expected message itself.  All outgoing legs and all three choices in one launch, in every form the shape has"""
    mfma = set(chis) == {16}
    items, olds, wants, conds = [], [], [], []
    for jo in range(len(chis)):
        it = _item(d, chis, jo, tag=ref.EPILOGUE_TAG, psd_like=True)
        raw = _ref_raw(it)
        cond = ref.conditioning(raw)
        assert cond >= 0.1                               # (before the GPU is touched: tests/test_small_site_ref_cpu.py holds the same for every case)
        want, _ = ref.finalize(raw, None, normalize)
        for old in (None, ref.crandn(np.random.default_rng(jo + 50), raw.shape), want.astype(np.complex64)):
            items.append(it); olds.append(old); wants.append(want); conds.append(cond if normalize else 1.0)
    for form in ((1, 0) if mfma else (0,)):
        res = small_site(items, form, olds=olds, normalize=normalize, epilogue=True)
        e_new = e_diff = 0.0
        for it, old, want, cond, (_, new, diff, route) in zip(items, olds, wants, conds, res):
            assert route == (ROUTE_MFMA16 if form == 1 else ROUTE_SCALAR) and np.all(np.isfinite(new))
            err = ref.rel_err(new, want)
            assert err < ref.raw_bound() / cond, (it["jo"], err, cond)       # measured x conditioning: 1.8e-7 (matrix-core form), 2.3e-7 (scalar form)
            dd = abs(diff - ref.message_diff(new, np.eye(want.shape[0]) if old is None else old))
            assert dd < 1e-12, (it["jo"], diff)                              # measured 6.7e-16
            e_new = max(e_new, err * cond); e_diff = max(e_diff, dd)
        name = "mfma16" if form == 1 else "scalar + msg_finalize<float>"
        _measured(f"small_site epilogue {name} d {d} chi {chis} normalize {normalize} new_msg x conditioning", e_new)
        _measured(f"small_site epilogue {name} d {d} chi {chis} normalize {normalize} message_diff", e_diff)
        if normalize:
            assert all(abs(np.sum(r[1].astype(np.complex128)) - 1) < 1e-5 for r in res)
    if mfma:
        # the kernel's own epilogue against the raw message of the same form + msg_finalize_kernel<float>: the same arithmetic in the same order
        raws = small_site(items, 1)
        sep = msg_finalize(0, [16] * len(items), [1] * len(items), [r[0][None] for r in raws], olds, normalize)
        fused = small_site(items, 1, olds=olds, normalize=normalize, epilogue=True)
        same_msg = all(np.array_equal(f[1], s[0]) for f, s in zip(fused, sep)); same_diff = all(f[2] == s[1] for f, s in zip(fused, sep))
        print(f"FUSED small_site epilogue d {d} z {len(chis)} normalize {normalize}: bit-identical to raw + msg_finalize: new_msg {same_msg}, message_diff {same_diff}")
        for f, s in zip(fused, sep):
            ulp = np.spacing(np.float32(max(np.max(np.abs(s[0].real)), np.max(np.abs(s[0].imag)))))
            assert np.max(np.abs(f[1].real - s[0].real)) <= ulp and np.max(np.abs(f[1].imag - s[0].imag)) <= ulp
            assert abs(f[2] - s[1]) < 1e-12


# ---- msg_finalize on its own ------------------------------------------------------------------------------------------------------------------------------------
FIN_CHI = [1, 2, 3, 16, 31, 32]
FIN_NCHUNKS = [1, 7, 8, 9, 31, 32, 33, 40, 70, 300]      # the 32-, 8- and 1-wide loops of the reduction and their seams


def _fin_partials(rng, chi, nch, dt):
    """partials whose element sum does not cancel: a common positive-definite part plus noise that adds up to a tenth of it"""
    a = ref.crandn(rng, (chi, chi)).astype(np.complex128)
    base = a @ a.conj().T / chi + np.eye(chi)
    return np.stack([(base / nch + 0.1 / np.sqrt(nch) * ref.crandn(rng, (chi, chi))).astype(dt) for _ in range(nch)])


def _fin_check(dtype, chis, nchunks, partials, olds, normalize, res):
    eps = 2.0 ** -23 if dtype == 0 else 2.0 ** -52
    worst = worst_d = 0.0
    for chi, nch, p, old, (new, diff) in zip(chis, nchunks, partials, olds, res):
        p = p.astype(np.complex128)
        m = p.sum(axis=0)
        B = nch * eps * np.abs(p).sum(axis=0)            # summation bound of any order, per element
        s = m.sum()
        if normalize and s != 0:
            # got = fl(m~ / s~), |m~ - m| <= B, |s~ - s| <= sum(B): |got - m / s| <= B / |s~| + |m| sum(B) / (|s| |s~|) + 4 eps |m / s|, |s~| >= |s| - sum(B)
            # (4 eps: the reciprocal of s~ and the complex product in double, a handful of roundings, and the rounding to T)
            assert ref.conditioning(m) >= 0.1
            sl = abs(s) - B.sum()
            tol = B / sl + np.abs(m) * B.sum() / (abs(s) * sl) + 4 * eps * np.abs(m / s)
            m = m / s
        else:
            tol = B + eps * np.abs(m)
        assert np.all(np.abs(new - m) <= tol), (chi, nch, float(np.max(np.abs(new - m) / tol)))      # measured 3.1e-7 (ComplexF32), 8.0e-15 (ComplexF64) of the largest entry
        worst = max(worst, ref.rel_err(new, m))
        dd = abs(diff - ref.message_diff(new, np.eye(chi) if old is None else old))
        assert dd < 1e-12, (chi, nch, diff)
        worst_d = max(worst_d, dd)
    return worst, worst_d


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("dtype", [0, 1])
def test_msg_finalize_every_chi_and_chunk_count(dtype, normalize):
    """one launch per chi with every chunk count as an item, old given / null alternating"""
    dt = np.complex64 if dtype == 0 else np.complex128
    worst = worst_d = 0.0
    for chi in FIN_CHI:
        rng = np.random.default_rng([chi, dtype])
        partials = [_fin_partials(rng, chi, nch, dt) for nch in FIN_NCHUNKS]
        olds = [None if i % 2 else ref.crandn(rng, (chi, chi)).astype(dt) for i in range(len(FIN_NCHUNKS))]
        chis = [chi] * len(FIN_NCHUNKS)
        res = msg_finalize(dtype, chis, FIN_NCHUNKS, partials, olds, normalize)
        w, wd = _fin_check(dtype, chis, FIN_NCHUNKS, partials, olds, normalize, res)
        worst = max(worst, w); worst_d = max(worst_d, wd)
    _measured(f"msg_finalize dtype {dtype} normalize {normalize} new_msg", worst)
    _measured(f"msg_finalize dtype {dtype} normalize {normalize} message_diff", worst_d)


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("dtype", [0, 1])
def test_msg_finalize_items_of_different_sizes_in_one_launch(dtype, normalize):
    dt = np.complex64 if dtype == 0 else np.complex128
    rng = np.random.default_rng(77 + dtype)
    chis = [32, 1, 3, 31, 16, 2, 32, 5]
    nchunks = [33, 300, 9, 1, 70, 8, 7, 40]
    partials = [_fin_partials(rng, c, n, dt) for c, n in zip(chis, nchunks)]
    olds = [ref.crandn(rng, (c, c)).astype(dt) if i % 3 else None for i, c in enumerate(chis)]
    for use_olds in (olds, None):                        # (None: no old array at all)
        res = msg_finalize(dtype, chis, nchunks, partials, use_olds, normalize)
        w, wd = _fin_check(dtype, chis, nchunks, partials, use_olds or [None] * len(chis), normalize, res)
        _measured(f"msg_finalize dtype {dtype} normalize {normalize} mixed launch new_msg", w)
        _measured(f"msg_finalize dtype {dtype} normalize {normalize} mixed launch message_diff", wd)


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("chi,nch", [(2, 1), (3, 9), (16, 33), (32, 40)])
def test_msg_finalize_skips_the_normalisation_of_an_exactly_zero_sum(dtype, chi, nch):
    """small-integer partials whose elements come in (p, -p) pairs: every sum is exact in either precision, the message's element sum is exactly zero, so the
    normalisation has to be skipped and the output is the plain reduction, bit for bit"""
    dt = np.complex64 if dtype == 0 else np.complex128
    rng = np.random.default_rng(chi + nch)
    half = (chi * chi) // 2
    v = rng.integers(-8, 9, size=(nch, half)) + 1j * rng.integers(-8, 9, size=(nch, half))
    flatp = np.zeros((nch, chi * chi), dtype=np.complex128)
    flatp[:, 0:2 * half:2] = v; flatp[:, 1:2 * half:2] = -v
    partials = np.stack([ref.unflat(flatp[c], chi) for c in range(nch)]).astype(dt)
    m = partials.astype(np.complex128).sum(axis=0)
    assert m.sum() == 0 and np.max(np.abs(m)) > 0
    (new, diff), = msg_finalize(dtype, [chi], [nch], [partials], None, 1)
    assert np.array_equal(new.astype(np.complex128), m)
    assert abs(diff - ref.message_diff(m, np.eye(chi))) < 1e-12
    _measured(f"msg_finalize dtype {dtype} zero-sum chi {chi} nchunks {nch}", float(np.max(np.abs(new - m))))


# ---- scale sweep ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", ref.SCALES)
@pytest.mark.parametrize("d,chis", ref.SCALE_SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_raw_message_scale_sweep(d, chis, scale):
    """psi scaled by 1e-18 .. 1e6 (the message by its square): the relative bound is unchanged while |psi|^2 prod |M| stays inside the f32 range -- the
    complex64 restatement does stay within it on these inputs (tests/test_small_site_ref_cpu.py)"""
    items = [_item(d, chis, jo, tag=2, scale=scale) for jo in range(len(chis))]
    forms = (0, 1) if set(chis) == {16} else (0,)
    for form in forms:
        err = _check_raw(f"small_site {'mfma16' if form else 'scalar'} d {d} chi {chis} scale {scale:g}", items, small_site(items, form))
        assert err < ref.raw_bound()                     # measured 3.7e-7 (scalar form, 1e-18), 3.4e-7 (matrix-core form, 1e-9)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,chis,form", [(1, (2,) * 9, -1), (1, (2, 33), 0), (8193, (1,), -1), (3, (16, 16, 16), -1), (2, (16, 8), 1), (3, (4, 4), 1)],
                         ids=["z9", "leg33", "n8193", "n12288_all16", "form1_not_all_16", "form1_small"])
def test_refusals(d, chis, form):
    """z = 9, a leg of 33, 8193 elements, and form = 1 on a shape that is not all-16: TNQS_ERR_UNSUPPORTED, nothing written, no fall-back"""
    it = _item(d, chis, 0)
    for epilogue in (False, True):
        assert small_site([it], form, epilogue=epilogue, expect_rc=ERR_UNSUPPORTED) is None
    ok = _item(2, (2, 4, 4), 0)                          # a refused item refuses the whole launch
    assert small_site([ok, it], form, expect_rc=ERR_UNSUPPORTED) is None
