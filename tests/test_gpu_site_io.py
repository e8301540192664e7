"""Site tensors across the C boundary with free leg orders: raw calls of tnqs_set_site_tensor / tnqs_get_site_tensor (include/tnqs.h).  The Python layer always passes the
full axis reversal (core.py _roles); the C driver and the Julia extension pass other orders, so permute_kernel<T> is driven here the way they drive it: a star whose centre
has 1, 3 and 7 neighbours (ndim = 2, 4, 8) with prime bond dimensions, a seeded random leg order into the library and a different one out of it.  Pure data movement:
get equals the numpy transpose of what was set bit for bit, for both complex types and for the real handles (widened on the way in, narrowed on the way out).  The one
case with arithmetic, a pending scale factor, is held to 2 u_T |v|: the factor rounded to the element type, then one product."""
import ctypes as C

import numpy as np
import pytest

import tnqs_amd as tn

pytestmark = pytest.mark.gpu
lib = C.CDLL(tn.LIB_PATH)
L = tn.core.L
ERR_INVALID = -1                                         # include/tnqs.h
PRIMES = [3, 5, 7, 11, 13, 17, 2]
DTYPES = [np.complex64, np.complex128, np.float32, np.float64]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def star(z, dtype, seed):
    """(cache, centre index, neighbour indices ascending, canonical centre tensor [d][chi_0]..[chi_{z-1}]) of a star with the centre in the middle of the vertex
    order, so that neighbours lie on both sides of it; every tensor set through the Python layer first (placeholders), the centre then again by the raw call"""
    rng = np.random.default_rng([z, seed])
    c = z // 2
    verts = list(range(z + 1))
    nbrs = [v for v in verts if v != c]
    g = tn.NamedGraph(verts, [(c, w) for w in nbrs])
    chis = PRIMES[:z]

    def rnd(shape):
        t = rng.standard_normal(shape)
        if np.issubdtype(np.dtype(dtype), np.complexfloating):
            t = t + 1j * rng.standard_normal(shape)
        return t.astype(dtype)
    tensors = {w: rnd((2, chi)) for w, chi in zip(nbrs, chis)}
    tensors[c] = rnd((2,) + tuple(chis))
    return tn.BeliefPropagationCache(tn.TensorNetworkState(g, tensors)), c, nbrs, rnd((2,) + tuple(chis))


def order(z, rng):
    """a random order of the canonical axes (0 = site, 1 + j = leg to the j-th neighbour) that is neither the identity nor the reversal the Python layer uses"""
    ident = list(range(z + 1))
    while True:
        p = [int(x) for x in rng.permutation(z + 1)]
        if z == 1 or (p != ident and p != ident[::-1]):
            return p


def set_raw(h, v, t_canon, perm, nbrs, dims=None, roles=None, ndim=None):
    """hand the library transpose(t_canon, perm) in column-major order: caller axis k is canonical axis perm[k]"""
    flat = np.ascontiguousarray(np.transpose(t_canon, perm).ravel(order="F"))
    d = np.asarray([t_canon.shape[a] for a in perm] if dims is None else dims, dtype=np.int64)
    r = np.asarray([-1 if a == 0 else nbrs[a - 1] for a in perm] if roles is None else roles, dtype=np.int32)
    return L.lib.tnqs_set_site_tensor(h, v, _p(flat), len(perm) if ndim is None else ndim, d.ctypes.data_as(C.POINTER(C.c_int64)), r.ctypes.data_as(C.POINTER(C.c_int32)))


def get_raw(h, v, shape_canon, perm, nbrs, dtype, roles=None, ndim=None):
    out = np.full(int(np.prod(shape_canon)), -123.0, dtype=dtype)
    r = np.asarray([-1 if a == 0 else nbrs[a - 1] for a in perm] if roles is None else roles, dtype=np.int32)
    rc = L.lib.tnqs_get_site_tensor(h, v, _p(out), len(perm) if ndim is None else ndim, r.ctypes.data_as(C.POINTER(C.c_int32)))
    return rc, out


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("z", [1, 3, 7])
def test_set_and_get_in_free_leg_orders(z, dtype):
    bpc, c, nbrs, T = star(z, dtype, 1)
    rng = np.random.default_rng([z, 99])
    for rep in range(2 if z < 7 else 1):
        pset = order(z, rng)
        pget = order(z, rng)
        while z > 1 and pget == pset:
            pget = order(z, rng)
        assert set_raw(bpc._h, c, T, pset, nbrs) == 0, L.lib.tnqs_last_error()
        rc, got = get_raw(bpc._h, c, T.shape, pget, nbrs, dtype)
        assert rc == 0, L.lib.tnqs_last_error()
        assert _same_bits(got, np.transpose(T, pget).ravel(order="F")), (pset, pget)
        # and the canonical layout is what the Python layer reads (its own order is the full reversal)
        assert _same_bits(bpc.tensor(c), T)
    print(f"MEASURED site io z={z} {np.dtype(dtype).name}: {T.size} elements bit-exact in free leg orders")


@pytest.mark.parametrize("dtype", [np.complex64, np.float64])
def test_invalid_arguments_leave_the_stored_tensor(dtype):
    z = 3
    bpc, c, nbrs, T = star(z, dtype, 2)
    perm = [2, 0, 3, 1]
    assert set_raw(bpc._h, c, T, perm, nbrs) == 0
    good_roles = [-1 if a == 0 else nbrs[a - 1] for a in perm]
    dup = list(good_roles); dup[0] = dup[2]
    stranger = list(good_roles); stranger[0] = c                      # the centre is not its own neighbour
    bad_site = [T.shape[a] for a in perm]; bad_site[1] = 3            # caller axis 1 is the site leg
    other = np.zeros_like(T) + 5
    for kw in (dict(roles=dup), dict(roles=stranger), dict(dims=bad_site), dict(ndim=9, roles=good_roles + [0] * 5, dims=[T.shape[a] for a in perm] + [1] * 5)):
        assert set_raw(bpc._h, c, other, perm, nbrs, **kw) == ERR_INVALID, kw
        rc, got = get_raw(bpc._h, c, T.shape, perm, nbrs, dtype)
        assert rc == 0 and _same_bits(got, np.transpose(T, perm).ravel(order="F")), kw
    for kw in (dict(roles=dup), dict(roles=stranger), dict(ndim=9, roles=good_roles + [0] * 5), dict(ndim=3, roles=good_roles[:3])):
        rc, got = get_raw(bpc._h, c, T.shape, perm, nbrs, dtype, **kw)
        assert rc == ERR_INVALID and np.all(got == -123.0), kw


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_get_applies_a_pending_scale_factor(dtype):
    """a normalising one-site gate leaves the tensor as the gate made it and records 1 / norm; the gate here has entries 0, 2 and 1/2, so the stored tensor is known
    exactly: get in a free order = stored x factor, the factor rounded to the element type and one product -- 2 u_T |v|"""
    z = 3
    bpc, c, nbrs, T = star(z, dtype, 3)
    assert set_raw(bpc._h, c, T, [1, 3, 0, 2], nbrs) == 0
    G = np.array([[0.0, 2.0], [0.5, 0.0]])
    out, _ = tn.apply_gates([(G, [c])], bpc, apply_kwargs=dict(normalize_tensors=True), update_cache=False)
    f = C.c_double(1.0)
    assert lib.tnqs_dbg_pending_scale(out._h, c, C.byref(f)) == 0
    stored = np.stack([2.0 * T[1], 0.5 * T[0]])                      # exact in either type
    assert f.value != 1.0 and abs(f.value * np.linalg.norm(stored.astype(np.complex128)) - 1) < 1e-6
    perm = [3, 1, 0, 2]
    rc, got = get_raw(out._h, c, T.shape, perm, nbrs, dtype)
    assert rc == 0, L.lib.tnqs_last_error()
    want = np.transpose(stored, perm).ravel(order="F").astype(np.clongdouble) * np.longdouble(f.value)
    uT = 2.0 ** -24 if dtype == np.complex64 else 2.0 ** -53
    err = np.abs(got.astype(np.clongdouble) - want).astype(np.float64)
    bound = 2 * uT * np.abs(want).astype(np.float64)
    worst = float(np.max(err / bound))
    print(f"MEASURED site io pending scale {np.dtype(dtype).name}: factor {f.value:.6f}, worst error / bound = {worst:.3f}")
    assert np.all(err <= bound)
    assert lib.tnqs_dbg_pending_scale(out._h, c, C.byref(f)) == 0 and f.value == 1.0      # folded in by the read
