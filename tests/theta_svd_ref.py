"""Reference and checks for the SVD stage of a two-site gate (csrc/gate_svd.cpp launch_theta_svd_stage: the gates' JacobiItems, svd_batch, the recovery of V), reached
through tnqs_dbg_theta_svd_stage (include/tnqs_debug.h) -- for tests/test_gpu_site_svd_stage.py, and checked on LAPACK outputs and on broken outputs in
tests/test_theta_svd_ref_cpu.py.  The single-item kernel tests of tests/test_gpu_kernels.py (test_jacobi_svd, check_theta_svd_pre, test_svd_tall_route) take their checks
from here too, so a batched item is held to exactly what the single-item test of the kernel that factorised it asserts.

Everything is plain numpy in complex128 on the inputs AS ROUNDED TO THE ELEMENT TYPE.  For one gate with device info (r1, r2, ..., K) the SVD runs on the m x ncol matrix M,
m = max(r1 d1, r2 d2), nfull = min(r1 d1, r2 d2), ncol = K or nfull (theta_dims: a wide theta is stored as its adjoint); theta0 is the m x nfull theta, theta0 = M Q^T on the
low-rank route.  The stage leaves A = U Sigma (m x ncol, any column order and phase) and V (nfull x ncol) with theta0 = A V^dagger.  The checks are invariant to column order
and phase:

  singular values   sorted column norms of A against numpy.linalg.svd(M), every one of them
  orthogonality     off-diagonal entries of A^dagger A against eps sigma_max^2
  rotation          A A^dagger = M M^dagger (the columns of A are a rotation of M's)
  reconstruction    sum_u a_u v_u^dagger = theta0 -- with a cap, the best approximation of that rank over the formed columns
  V                 orthonormal on the columns above the noise floor

Tolerances, by the kernel that factorised the item (route_out):
  plain Jacobi (LDS or global memory), V recovered: test_jacobi_svd's forms with eps = EPS[dtype] max(m, ncol) -- singular values eps sigma_max, orthogonality eps sigma_max^2,
      reconstruction 4 eps sigma_max.  The rotation has no line in test_jacobi_svd: A A^dagger - M M^dagger is first order in the same backward error as the reconstruction,
      times one more factor of at most sigma_max, so 4 eps sigma_max^2.  A recovered V (v_u = theta0^dagger a_u / |a_u|^2) is orthonormal only as far as the columns of A are
      orthogonal RELATIVE to their own norms: |V^dagger V - I|_uv <= 4 EPS[dtype] max(m, nfull) sigma_max / min(sigma_u, sigma_v), test_jacobi_svd's "recovered V: eps*cond"
      with the condition number of the pair; asserted on the columns above the noise floor sigma_u > eps sigma_max (below it a singular value is not asserted to any digit).
  preconditioned kernel: check_theta_svd_pre's (singular values 4e-6 sigma_max, rank-k reconstruction 3e-6 sigma_max sqrt(n), V 3e-6, U 3e-6 sigma_max weighted, the
      sigma_j e_0 form of the unformed columns with the 1e-4 tie band at the cap); the rotation, where every column is formed: |A - M U_L| <= 3e-6 sigma_max per entry is what
      the U line asserts, so rows of the error have norm <= 3e-6 sigma_max sqrt(n) and A A^dagger - M M^dagger <= 2 * 3e-6 sqrt(n) sigma_max^2.
  tall route: test_svd_tall_route's (1e-5, 1.25e-6, 4.5e-6), then the recovered-V lines of the plain Jacobi."""
import ctypes as C

import numpy as np

CT = {0: np.complex64, 1: np.complex128}
EPS = {0: 2e-6, 1: 1e-14}                               # test_jacobi_svd's per-type constants
ROUTE_PRE_LOWRANK, ROUTE_PRE_THETA, ROUTE_LDS, ROUTE_GLOBAL, ROUTE_TALL = 10, 11, 12, 13, 14      # TNQS_DBG_ROUTE_SVD_* (include/tnqs_debug.h)
ROUTE_NAME = {ROUTE_PRE_LOWRANK: "pre_lowrank", ROUTE_PRE_THETA: "pre_theta", ROUTE_LDS: "jacobi_lds", ROUTE_GLOBAL: "jacobi_global", ROUTE_TALL: "tall"}
PRE_ROUTES = (ROUTE_PRE_LOWRANK, ROUTE_PRE_THETA)
TALL_BOUNDS = (1e-5, 1.25e-6, 4.5e-6)                   # test_svd_tall_route: singular values, orthogonality of the normalised columns, A A^dagger (relative)
SENT = -7.5 + 3.25j
ERR_INVALID, ERR_UNSUPPORTED = -1, -2                   # include/tnqs.h


def rnd(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def flat(m):
    return np.asarray(m).ravel(order="F")


def theta_dims(info, d1, d2):
    """kernels.hpp theta_dims: rows, columns of theta, columns the SVD runs on"""
    Mr, Nc = info[0] * d1, info[1] * d2
    if Mr < Nc:
        Mr, Nc = Nc, Mr
    return Mr, Nc, (info[7] if info[7] > 0 else Nc)


# ---- the single-item checks, shared with tests/test_gpu_kernels.py ----------------------------------------------------------------------------------------------
def jacobi_errors(a, A, V):
    """test_jacobi_svd's three matrix lines on a (m x n, complex128), A = U Sigma, V with a = A V^dagger: (singular values / sigma_max, reconstruction / sigma_max,
    orthogonality / sigma_max^2); the caller compares them with eps, 4 eps, eps"""
    A = np.asarray(A, dtype=np.complex128); V = np.asarray(V, dtype=np.complex128)
    s_ref = np.linalg.svd(a, compute_uv=False)
    s = np.sort(np.linalg.norm(A, axis=0))[::-1]
    G = A.conj().T @ A
    off = G - np.diag(np.diag(G))
    return (np.max(np.abs(s[:len(s_ref)] - s_ref)) / s_ref[0], np.max(np.abs(A @ V.conj().T - a)) / s_ref[0], np.max(np.abs(off)) / s_ref[0] ** 2)


def pre_unformed(nrm, cap):
    """check_theta_svd_pre's column sets: keep = the columns whose vectors must be formed, other = those that must leave as sigma_j e_0 -- all but the ones within 1e-4 of
    the cap-th singular value (ties at the cap are formed too: the consumer ranks again)"""
    n = len(nrm)
    order = np.argsort(-nrm, kind="stable")
    keep = order[: (cap if 0 < cap < n else n)]
    other = np.array([j for j in order[len(keep):] if nrm[j] < nrm[keep[-1]] * (1 - 2e-4)], dtype=int)
    return keep, other


def has_pre_signature(A, V, cap):
    """the preconditioned kernel's mark on an item with 0 < cap < ncol: the unformed columns are sigma_j e_0, their V columns zero.  None where no column has to be unformed"""
    A = np.asarray(A, dtype=np.complex128); V = np.asarray(V, dtype=np.complex128)
    nrm = np.linalg.norm(A, axis=0)
    _, other = pre_unformed(nrm, cap)
    if not len(other):
        return None
    return bool(np.all(A[1:, other] == 0) and np.allclose(A[0, other].real, nrm[other]) and np.all(A[0, other].imag == 0) and np.all(V[:, other] == 0))


def check_pre(M32, Q, theta, A, V, sw, sv_tol=4e-6, cap=0):
    """check_theta_svd_pre on the outputs (A, V, sw) of the preconditioned kernel for the factor M32 (complex128 values of the ComplexF32 input) of theta = M32 Q^T (Q None:
    theta itself).  Returns error / bound per line"""
    A = np.asarray(A, dtype=np.complex128); V = np.asarray(V, dtype=np.complex128)
    s_ref = np.linalg.svd(M32, compute_uv=False)
    nrm = np.linalg.norm(A, axis=0)
    out = {}
    assert 0 < sw < 30
    e = np.max(np.abs(np.sort(nrm)[::-1] - s_ref))
    assert e < sv_tol * s_ref[0], (np.sort(nrm)[::-1][:4], s_ref[:4])      # EVERY singular value (the truncation error needs them all)
    out["singular values"] = e / (sv_tol * s_ref[0])
    n = M32.shape[1]
    keep, other = pre_unformed(nrm, cap)
    if len(other):
        assert np.all(A[1:, other] == 0) and np.allclose(A[0, other].real, nrm[other]) and np.all(A[0, other].imag == 0)
        assert np.all(V[:, other] == 0)                                                       # never garbage
    full = M32 @ Q.T if Q is not None else M32                                                # theta
    u, sv, vh = np.linalg.svd(full, full_matrices=False)
    k = len(keep)
    best = (u[:, :k] * sv[:k]) @ vh[:k]                                                       # best rank-k approximation
    rec = A[:, keep] @ V[:, keep].conj().T                                                    # (U Sigma) V^dagger over the kept triplets
    b = 3e-6 * s_ref[0] * np.sqrt(n)
    assert np.max(np.abs(rec - best)) < b, float(np.max(np.abs(rec - best)) / s_ref[0])
    out["reconstruction"] = np.max(np.abs(rec - best)) / b
    if theta is not None and k == n:
        assert np.max(np.abs(rec - theta)) < b
        out["reconstruction"] = max(out["reconstruction"], np.max(np.abs(rec - theta)) / b)
    big = nrm[keep] > 1e-5 * s_ref[0]                                       # V: orthonormal to f32 rounding whatever the singular value (no division by Sigma^2)
    Vb = V[:, keep][:, big]
    e = np.max(np.abs(Vb.conj().T @ Vb - np.eye(Vb.shape[1])))
    assert e < 3e-6
    out["V"] = e / 3e-6
    nb = nrm[keep][big]
    U = A[:, keep][:, big] / nb                                             # U Sigma = M U_L: absolute accuracy eps * sigma_max per column (like LAPACK's)
    e = np.max(np.abs((U.conj().T @ U - np.eye(U.shape[1])) * np.minimum.outer(nb, nb)))
    assert e < 3e-6 * s_ref[0]
    out["orthogonality"] = e / (3e-6 * s_ref[0])
    return out


def tall_errors(b, A):
    """test_svd_tall_route's three figures for b (complex128 values of the ComplexF32 input, nonzero) and the output A of the tall route"""
    A = np.asarray(A, dtype=np.complex128)
    s_ref = np.linalg.svd(b, compute_uv=False)
    nrm = np.linalg.norm(A, axis=0)
    e_s = np.max(np.abs(np.sort(nrm)[::-1][:len(s_ref)] - s_ref)) / s_ref[0]
    big = nrm > 1e-4 * s_ref[0]
    U = A[:, big] / nrm[big]
    e_o = np.max(np.abs(U.conj().T @ U - np.eye(U.shape[1])))
    e_r = np.max(np.abs(A @ A.conj().T - b @ b.conj().T)) / s_ref[0] ** 2
    return e_s, e_o, e_r


# ---- the items of a launch ----------------------------------------------------------------------------------------------------------------------------------------
class Item:
    """one gate of a launch.  (r1, r2): the ranks the device holds; (n1, n2): the bounds (default: the ranks); K: the columns the host expects of the low-rank route, K_dev
    those alive on the device (default K); has_q: the gate has its Q; rub: the ranks the sites CAN have (default: the bounds); kind: "spread" (singular values over 3.5
    decades), "rank3", "zero"; route: the kernel named for the item"""

    def __init__(self, name, r1, r2, n1=None, n2=None, K=0, K_dev=None, has_q=False, rub=None, cap=0, kind="spread", route=None, d1=2, d2=2):
        self.name, self.r1, self.r2, self.d1, self.d2 = name, r1, r2, d1, d2
        self.n1, self.n2 = (r1 if n1 is None else n1), (r2 if n2 is None else n2)
        self.K, self.K_dev, self.has_q, self.cap, self.kind, self.route = K, (K if K_dev is None else K_dev), has_q, cap, kind, route
        self.rub = (self.n1, self.n2) if rub is None else rub
        self.info = [r1, r2, 0, 0, 0, int(r1 * d1 < r2 * d2), 0, self.K_dev]
        self.m, self.nfull, self.ncol = theta_dims(self.info, d1, d2)
        self.MrB, self.NcB = max(self.n1 * d1, self.n2 * d2), min(self.n1 * d1, self.n2 * d2)

    def inputs(self, rng, dtype):
        """(M, Q, theta0): M and theta0 hold the complex128 values of the numbers rounded to the element type"""
        m, nfull, ncol = self.m, self.nfull, self.ncol
        if self.kind == "zero":
            M = np.zeros((m, ncol), dtype=np.complex128)
        else:
            rank = 3 if self.kind == "rank3" else ncol
            dec = np.exp(-np.arange(rank) * (8.0 / rank))                     # test_theta_svd_pre_kernel's spectra: 3.5 decades
            q1, _ = np.linalg.qr(rnd(rng, (m, rank))); q2, _ = np.linalg.qr(rnd(rng, (ncol, rank)))
            M = (q1 * dec) @ q2.conj().T
        M = M.astype(CT[dtype]).astype(np.complex128)
        Q = np.linalg.qr(rnd(rng, (nfull, self.K)))[0] if self.has_q or self.K_dev > 0 else None
        theta0 = (M @ Q.T).astype(CT[dtype]).astype(np.complex128) if self.K_dev > 0 else M.copy()
        return M, Q, theta0


class Launch:
    """the arrays of one tnqs_dbg_theta_svd_stage call: theta, theta0, thetaV sized from the bounds, guard / item / guard / ..., every element the stage may not write
    (guard bands, and the part of a slot beyond the item's dynamic extent) holding a sentinel"""

    def __init__(self, items, dtype, dyn, seed=0, guard=3):
        self.items, self.dtype, self.dyn, self.guard = items, dtype, dyn, guard
        rng = np.random.default_rng(seed)
        self.inp = [it.inputs(rng, dtype) for it in items]
        self.lens = [it.MrB * it.NcB for it in items]
        self.vlens = [it.MrB * it.MrB for it in items]
        self.theta, self.theta0, self.thetaV = self._array(self.lens), self._array(self.lens), self._array(self.vlens)
        q = []
        for i, it in enumerate(items):
            M, Q, th0 = self.inp[i]
            self.slot(self.theta, self.lens, i)[: M.size] = flat(M)
            self.slot(self.theta0, self.lens, i)[: th0.size] = flat(th0)
            if it.has_q:
                slot = np.zeros(it.NcB * it.K, dtype=np.complex128)
                slot[: Q.size] = flat(Q)
                q.append(slot)
        self.Q = np.ascontiguousarray(np.concatenate(q)) if q else None
        self.theta_in, self.theta0_in, self.thetaV_in = self.theta.copy(), self.theta0.copy(), self.thetaV.copy()
        self.sweeps = np.full(len(items), -1, dtype=np.int32)
        self.routes = np.zeros(len(items), dtype=np.int32)

    def _array(self, lens):
        return np.full(self.guard + sum(l + self.guard for l in lens), SENT, dtype=CT[self.dtype])

    def slot(self, arr, lens, i):
        s = self.guard + sum(l + self.guard for l in lens[:i])
        return arr[s: s + lens[i]]

    def outputs(self, i):
        """(A, V) of item i as the stage left them"""
        it = self.items[i]
        A = self.slot(self.theta, self.lens, i)[: it.m * it.ncol].reshape((it.m, it.ncol), order="F")
        V = self.slot(self.thetaV, self.vlens, i)[: it.nfull * it.ncol].reshape((it.nfull, it.ncol), order="F")
        return A, V

    def set_outputs(self, i, A, V):
        it = self.items[i]
        self.slot(self.theta, self.lens, i)[: it.m * it.ncol] = flat(A)
        self.slot(self.thetaV, self.vlens, i)[: it.nfull * it.ncol] = flat(V)

    def call(self, lib, recover_form=0, host_only=False):
        """tnqs_dbg_theta_svd_stage on the launch's arrays (host_only: theta = NULL, only route_out is filled); returns the status"""
        def ints(v):
            return np.ascontiguousarray(np.asarray(v, dtype=np.int32).ravel())

        def p(a):
            return None if a is None else a.ctypes.data_as(C.c_void_p)
        its = self.items
        dims = ints([[it.d1, it.d2, it.n1, it.n2] for it in its]); info = ints([it.info for it in its]); K = ints([it.K for it in its])
        hq = ints([int(it.has_q) for it in its]); rub = ints([it.rub for it in its]); cap = ints([it.cap for it in its])
        th = (None, None, None) if host_only else (self.theta, self.theta0, self.thetaV)
        return lib.tnqs_dbg_theta_svd_stage(self.dtype, int(self.dyn), len(its), p(dims), p(info), p(K), p(hq), p(self.Q), p(rub), p(cap), int(recover_form),
                                            p(th[0]), p(th[1]), p(th[2]), p(self.sweeps), p(self.routes), self.guard)


# ---- the checks of a launch -----------------------------------------------------------------------------------------------------------------------------------------
def check_untouched(L):
    """guard bands intact, theta0 as it went up, and every element of theta / thetaV beyond the item's DYNAMIC extent, inside its bound-sized slot, unchanged"""
    assert np.array_equal(L.theta0.view(np.uint8), L.theta0_in.view(np.uint8)), "theta0 was written"
    for arr, arr_in, lens, what in ((L.theta, L.theta_in, L.lens, "theta"), (L.thetaV, L.thetaV_in, L.vlens, "thetaV")):
        own = np.zeros(arr.size, dtype=bool)
        for i, it in enumerate(L.items):
            s = L.guard + sum(l + L.guard for l in lens[:i])
            own[s: s + it.ncol * (it.m if what == "theta" else it.nfull)] = True
        bad = ~own & (arr.view(np.uint8).reshape(arr.size, -1) != arr_in.view(np.uint8).reshape(arr.size, -1)).any(axis=1)
        assert not bad.any(), f"{what}: {int(bad.sum())} elements outside the items' dynamic extents were written (first at {int(np.argmax(bad))})"


def check_item(it, dtype, inp, A, V, route, sw=None):
    """every check of the module docstring on one item, by the tolerances of the kernel `route` names.  Returns {line: error / bound}"""
    M, Q, th0 = inp
    A = np.asarray(A).astype(np.complex128); V = np.asarray(V).astype(np.complex128)
    assert np.all(np.isfinite(A)) and np.all(np.isfinite(V)), "a non-finite output"
    m, ncol = M.shape; nfull = th0.shape[1]
    s_ref = np.linalg.svd(M, compute_uv=False)
    s0 = s_ref[0]
    if s0 == 0:                                       # zero theta: U Sigma = 0, V = 0, on every route
        assert np.all(A == 0) and np.all(V == 0), "zero theta: U Sigma and V must be zero"
        if sw is not None and route in PRE_ROUTES:
            assert sw == 0
        return {}
    nrm = np.linalg.norm(A, axis=0)
    capped = 0 < it.cap < ncol
    if route in PRE_ROUTES:
        out = check_pre(M, Q if route == ROUTE_PRE_LOWRANK else None, th0, A, V, 1 if sw is None else sw, cap=it.cap)
        keep, other = pre_unformed(nrm, it.cap)
        if not len(other) and len(keep) == ncol:      # every column formed: the columns are a rotation of M's
            b = 2 * 3e-6 * np.sqrt(ncol) * s0 ** 2
            e = np.max(np.abs(A @ A.conj().T - M @ M.conj().T))
            assert e < b, ("rotation", e, b)
            out["rotation"] = e / b
        return out
    out = {}
    if sw is not None:
        assert 0 <= sw < 60
    if capped:                                        # an item the plain Jacobi took does not carry the preconditioned kernel's signature
        assert has_pre_signature(A, V, it.cap) is False, "the preconditioned kernel's unformed columns on an item the plain Jacobi should have taken"
    eps = EPS[dtype] * max(m, ncol)
    if route == ROUTE_TALL:
        for name, e, b in zip(("singular values", "orthogonality", "rotation"), tall_errors(M, A), TALL_BOUNDS):
            assert e < b, (name, e, b)
            out[name] = e / b
    else:
        G = A.conj().T @ A
        lines = (("singular values", np.max(np.abs(np.sort(nrm)[::-1] - s_ref)), eps * s0),
                 ("orthogonality", np.max(np.abs(G - np.diag(np.diag(G)))), eps * s0 ** 2),
                 ("rotation", np.max(np.abs(A @ A.conj().T - M @ M.conj().T)), 4 * eps * s0 ** 2))
        for name, e, b in lines:
            assert e < b, (name, e, b)
            out[name] = e / b
    e, b = np.max(np.abs(A @ V.conj().T - th0)), 4 * eps * s0
    assert e < b, ("reconstruction", e, b)
    out["reconstruction"] = e / b
    big = nrm > eps * s0                              # the columns above the noise floor
    Vb, nb = V[:, big], nrm[big]
    bound = 4 * EPS[dtype] * max(m, nfull) * s0 / np.minimum.outer(nb, nb)
    ratio = np.abs(Vb.conj().T @ Vb - np.eye(Vb.shape[1])) / bound
    assert np.max(ratio) < 1, ("V", float(np.max(ratio)))
    out["V"] = float(np.max(ratio))
    return out


def check_launch(L, expect_routes=True):
    """all of it on the arrays of a launch after the call (or after an emulation of it).  Returns {item name: {line: error / bound}}"""
    check_untouched(L)
    res = {}
    for i, it in enumerate(L.items):
        if expect_routes and it.route is not None:
            assert L.routes[i] == it.route, (it.name, ROUTE_NAME.get(int(L.routes[i]), int(L.routes[i])), ROUTE_NAME[it.route])
        A, V = L.outputs(i)
        try:
            res[it.name] = check_item(it, L.dtype, L.inp[i], A, V, int(L.routes[i]), None if L.sweeps[i] < 0 else int(L.sweeps[i]))
        except AssertionError as e:
            raise AssertionError(f"item {it.name} ({ROUTE_NAME.get(int(L.routes[i]))}): {e}") from e
    return res


# ---- the launches of tests/test_gpu_site_svd_stage.py (all d = 2: the smallest shapes that still reach each branch) -----------------------------------------------
def dyn_f32_items():
    return [Item("A", 12, 12, K=20, has_q=True, cap=10, route=ROUTE_PRE_LOWRANK),                                  # 24 x 20 factor at its bounds, V through Q
            Item("B", 8, 8, K=12, has_q=True, cap=6, route=ROUTE_LDS),                                             # K <= 16: declined; 16 x 12, recovery with nu = 12 < n = 16
            Item("C", 10, 10, n1=12, n2=12, K=20, K_dev=0, has_q=True, cap=8, route=ROUTE_PRE_THETA),              # low-rank route withdrawn on the device: theta itself, 20 x 20
            Item("D", 6, 6, n1=12, n2=12, K=20, K_dev=0, has_q=True, cap=5, route=ROUTE_LDS),                      # the same with 12 <= 16 columns: the pre = 2 offer declined
            Item("E", 10, 40, rub=(10, 40), cap=10, route=ROUTE_PRE_THETA),                                        # pre = 1 taken: wide, stored 80 x 20
            Item("F", 4, 30, n1=10, n2=40, rub=(10, 40), cap=4, route=ROUTE_LDS),                                  # pre = 1 declined: 60 x 8, leading dimension 60 in a slot for 80
            Item("G", 70, 8, route=ROUTE_LDS),                                                                     # 140 x 16: its rows pick the instantiation of the launch
            Item("H", 12, 12, cap=10, kind="rank3", route=ROUTE_PRE_THETA),
            Item("I", 12, 12, kind="zero", route=ROUTE_PRE_THETA),
            Item("I-lds", 6, 6, kind="zero", route=ROUTE_LDS),
            Item("I-low", 12, 12, K=20, has_q=True, kind="zero", route=ROUTE_PRE_LOWRANK)]


def dyn_f64_items():
    keep = {"B", "D", "F", "G", "H", "I", "I-lds"}      # no `pre` in double: every item on the LDS Jacobi, recover_v_kernel<double, 8> with nu < n and ranks below the bounds
    items = [it for it in dyn_f32_items() if it.name in keep]
    for it in items:
        it.route = ROUTE_LDS
    return items


def static_items(dtype):
    big = ROUTE_TALL if dtype == 0 else ROUTE_GLOBAL                                                               # 260 rows: the tall route / jacobi_kernel<double, 8>
    return [Item("24x24", 12, 12, route=ROUTE_LDS),
            Item("24x10", 12, 12, K=10, route=ROUTE_LDS),                                                          # the factor of a 24 x 24 theta: nu = 10 < n = 24
            Item("260x12", 130, 6, route=big),
            Item("rank3", 12, 12, kind="rank3", route=ROUTE_LDS),
            Item("zero", 12, 12, kind="zero", route=ROUTE_LDS),
            Item("zero260", 130, 6, kind="zero", route=big)]
