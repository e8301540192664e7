"""The checks of tests/theta_svd_ref.py, checked themselves (no GPU): an exact SVD stage -- LAPACK's SVD with shuffled columns and random phases, V formed the way the
route forms it, everything rounded to the element type -- must pass them on every launch of tests/test_gpu_site_svd_stage.py, and five broken stages must fail them.
Then the host-only form of tnqs_dbg_theta_svd_stage (theta = NULL: only route_out is filled) on the same item tables: every item gets the route named for it, every
TNQS_DBG_ROUTE_SVD_* occurs, and the two refusals are refusals."""
import ctypes as C

import numpy as np
import pytest

import theta_svd_ref as ref

LAUNCHES = {"dyn-c64": (ref.dyn_f32_items, 0, 1), "dyn-c128": (ref.dyn_f64_items, 1, 1),
            "static-c64": (lambda: ref.static_items(0), 0, 0), "static-c128": (lambda: ref.static_items(1), 1, 0)}


def launch(name, seed=1):
    items, dtype, dyn = LAUNCHES[name]
    return ref.Launch(items(), dtype, dyn, seed=seed)


def recover(th0, A):
    """V[:, u] = theta0^dagger a_u / |a_u|^2, zero for a zero column"""
    s2 = np.sum(np.abs(A) ** 2, axis=0)
    return th0.conj().T @ A / np.where(s2 > 0, s2, 1.0) * (s2 > 0)


def exact_outputs(it, dtype, inp, rng):
    M, Q, th0 = inp
    ct = ref.CT[dtype]
    u, s, vh = np.linalg.svd(M, full_matrices=False)
    ncol = M.shape[1]
    perm = rng.permutation(ncol); ph = np.exp(2j * np.pi * rng.random(ncol))
    A = ((u * s)[:, perm] * ph).astype(ct).astype(np.complex128)
    if s[0] == 0:
        return A.astype(ct), np.zeros((th0.shape[1], ncol), dtype=ct)
    if it.route in ref.PRE_ROUTES:
        V = vh.conj().T[:, perm] * ph
        if it.route == ref.ROUTE_PRE_LOWRANK:
            V = np.conj(Q) @ V
        if 0 < it.cap < ncol:                       # the kernel's rule: everything within 1e-4 of the cap-th singular value is formed, the others leave as sigma_j e_0
            sp = s[perm]
            thr = np.sort(sp)[::-1][it.cap - 1] * (1 - 1e-4)
            un = sp < thr
            A[:, un] = 0; A[0, un] = sp[un]; V[:, un] = 0
            A = A.astype(ct).astype(np.complex128)
        return A.astype(ct), V.astype(ct)
    return A.astype(ct), recover(th0, A).astype(ct)


def emulate(L, seed=5):
    rng = np.random.default_rng(seed)
    for i, it in enumerate(L.items):
        A, V = exact_outputs(it, L.dtype, L.inp[i], rng)
        L.set_outputs(i, A, V)
        L.routes[i] = it.route
        L.sweeps[i] = 0 if it.kind == "zero" else 5
    return L


def index(L, name):
    return [it.name for it in L.items].index(name)


@pytest.mark.parametrize("name", sorted(LAUNCHES))
def test_an_exact_stage_passes(name):
    L = emulate(launch(name))
    res = ref.check_launch(L)
    worst = max(max(r.values()) for r in res.values() if r)
    print(f"worst error / bound of an exact stage, {name}: {worst:.3f}")
    assert set(res) == {it.name for it in L.items} and worst < 1
    for it in L.items:                              # the lines every nonzero item is held to
        if it.kind != "zero":
            assert {"singular values", "orthogonality", "reconstruction", "V"} <= set(res[it.name]), (it.name, res[it.name])
    if name == "dyn-c64":                           # who ran: the capped items of the preconditioned kernel show it, those of the plain Jacobi do not
        for nm, sig in (("A", True), ("C", True), ("E", True), ("B", False), ("D", False), ("F", False)):
            A, V = L.outputs(index(L, nm))
            assert ref.has_pre_signature(A, V, L.items[index(L, nm)].cap) is sig, nm


@pytest.mark.parametrize("name,item", [("dyn-c64", "G"), ("dyn-c64", "A"), ("dyn-c128", "G"), ("static-c64", "260x12"), ("static-c128", "260x12")])
def test_broken_1_a_column_pair_left_unrotated(name, item):
    L = emulate(launch(name))
    i = index(L, item)
    A, V = (x.astype(np.complex128) for x in L.outputs(i))
    p, q = np.argsort(-np.linalg.norm(A, axis=0))[:2]
    A[:, p], A[:, q] = (A[:, p] + A[:, q]) / np.sqrt(2), (A[:, p] - A[:, q]) / np.sqrt(2)        # the pair as it was one rotation earlier
    if L.items[i].route in ref.PRE_ROUTES:
        V[:, p], V[:, q] = (V[:, p] + V[:, q]) / np.sqrt(2), (V[:, p] - V[:, q]) / np.sqrt(2)    # (the reconstruction still holds: only the orthogonality can tell)
    else:
        V = recover(L.inp[i][2], A)
    L.set_outputs(i, A, V)
    with pytest.raises(AssertionError, match=f"item {item}"):
        ref.check_launch(L)


@pytest.mark.parametrize("name", ["static-c64", "static-c128"])
def test_broken_2_v_of_another_item(name):
    L = emulate(launch(name))
    i, j = index(L, "24x24"), index(L, "rank3")
    (Ai, Vi), (Aj, Vj) = [tuple(x.copy() for x in L.outputs(k)) for k in (i, j)]
    L.set_outputs(i, Ai, Vj); L.set_outputs(j, Aj, Vi)
    with pytest.raises(AssertionError, match="reconstruction"):
        ref.check_launch(L)


@pytest.mark.parametrize("name", ["dyn-c64", "dyn-c128"])
def test_broken_3_the_bound_as_leading_dimension(name):
    """item F: 60 x 8 at the start of a slot sized for 80 x 20, read and written with leading dimension 80"""
    L = emulate(launch(name))
    i = index(L, "F"); it = L.items[i]
    assert (it.m, it.ncol, it.MrB) == (60, 8, 80)
    Mw = L.slot(L.theta_in, L.lens, i)[: 80 * 8].reshape((80, 8), order="F").astype(np.complex128)
    T0w = L.slot(L.theta0_in, L.lens, i)[: 80 * 8].reshape((80, 8), order="F").astype(np.complex128)
    u, s, _ = np.linalg.svd(Mw, full_matrices=False)
    Aw = u * s
    L.slot(L.theta, L.lens, i)[: 80 * 8] = ref.flat(Aw)
    L.slot(L.thetaV, L.vlens, i)[: 64] = ref.flat(recover(T0w, Aw))
    with pytest.raises(AssertionError, match="outside the items' dynamic extents"):
        ref.check_launch(L)
    with pytest.raises(AssertionError):               # and the numbers alone say so too
        ref.check_item(it, L.dtype, L.inp[i], *L.outputs(i), it.route)


@pytest.mark.parametrize("name,item", [("dyn-c64", "E"), ("dyn-c64", "F"), ("dyn-c128", "F")])
def test_broken_4_a_wide_item_not_adjointed(name, item):
    """the stored matrix is the adjoint, max(r1 d1, r2 d2) rows; a stage that takes (r1 d1) x (r2 d2) reads the same numbers as a wide matrix"""
    L = emulate(launch(name))
    i = index(L, item); it = L.items[i]
    Mr, Nc = it.r1 * it.d1, it.r2 * it.d2
    assert Mr < Nc
    Mw = L.slot(L.theta_in, L.lens, i)[: Mr * Nc].reshape((Mr, Nc), order="F").astype(np.complex128)
    _, _, vh = np.linalg.svd(Mw, full_matrices=True)
    Aw = Mw @ vh.conj().T                              # orthogonal columns (Nc of them, Nc - Mr zero) of Mr rows
    L.slot(L.theta, L.lens, i)[: Mr * Nc] = ref.flat(Aw)
    with pytest.raises(AssertionError, match=f"item {item}"):
        ref.check_launch(L)


@pytest.mark.parametrize("name", ["dyn-c64", "dyn-c128", "static-c64", "static-c128"])
def test_broken_5_nu_columns_recovered_as_if_nu_were_n(name):
    """the low-rank factor on the plain Jacobi: V is n x nu with nu < n.  A recovery that takes nu = n computes the same first nu columns and writes n - nu more, from
    whatever follows the factor in theta -- only the check of what lies outside the item can tell"""
    L = emulate(launch(name))
    i = index(L, "B" if L.dyn else "24x10"); it = L.items[i]
    assert it.ncol < it.nfull
    Aext = L.slot(L.theta, L.lens, i)[: it.m * it.nfull].reshape((it.m, it.nfull), order="F").astype(np.complex128)
    L.slot(L.thetaV, L.vlens, i)[: it.nfull * it.nfull] = ref.flat(recover(L.inp[i][2], Aext))
    ref.check_item(it, L.dtype, L.inp[i], *L.outputs(i), it.route)      # the item's own numbers are right
    with pytest.raises(AssertionError, match="thetaV: .* outside the items' dynamic extents"):
        ref.check_launch(L)


# ---- the host-only form of the entry point -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import tnqs_amd as tn
    lib = C.CDLL(tn.LIB_PATH)
    lib.tnqs_last_error.restype = C.c_char_p
    return lib


def test_host_only_routes_match_the_item_tables_and_cover_every_route(lib):
    seen = set()
    for name in sorted(LAUNCHES):
        L = launch(name)
        before = [a.copy() for a in (L.theta, L.theta0, L.thetaV)]
        rc = L.call(lib, host_only=True)
        assert rc == 0, lib.tnqs_last_error()
        for it, r in zip(L.items, L.routes):
            assert r == it.route, (name, it.name, ref.ROUTE_NAME.get(int(r), int(r)), ref.ROUTE_NAME[it.route])
        assert all(np.array_equal(a, b) for a, b in zip(before, (L.theta, L.theta0, L.thetaV))) and np.all(L.sweeps == -1)
        seen |= {int(r) for r in L.routes}
    assert seen == set(ref.ROUTE_NAME)


def test_host_only_recover_form_does_not_change_the_routes(lib):
    L = launch("static-c64")
    assert L.call(lib, recover_form=1, host_only=True) == 0
    assert [int(r) for r in L.routes] == [it.route for it in L.items]


@pytest.mark.parametrize("dtype", [0, 1])
def test_refusals(lib, dtype):
    """the run-ahead regime where a bound fails the engine's one_trip rule (more than 256 rows); d^2 chi beyond 512 in either regime"""
    L = ref.Launch([ref.Item("24x24", 12, 12), ref.Item("260x12", 130, 6)], dtype, dyn=1)
    assert L.call(lib, host_only=True) == ref.ERR_UNSUPPORTED and b"run-ahead" in lib.tnqs_last_error()
    L = ref.Launch([ref.Item("small ranks, bounds within the LDS but 260 rows", 4, 4, n1=130, n2=6)], dtype, dyn=1)
    assert L.call(lib, host_only=True) == ref.ERR_UNSUPPORTED
    for dyn in (0, 1):
        L = ref.Launch([ref.Item("516", 4, 4, n1=258, n2=4)], dtype, dyn=dyn)
        assert L.call(lib, host_only=True) == ref.ERR_UNSUPPORTED and b"512" in lib.tnqs_last_error()
    assert np.all(L.routes == 0)
