"""Kernel-level GPU tests through include/tnqs_debug.h: each HIP kernel against a float64 numpy evaluation of the
same contraction (transposition-detecting random inputs, odd dimensions, ragged tiles)."""
import ctypes as C
import os

import numpy as np
import pytest

import tnqs_amd as tn
import theta_svd_ref as svd_ref

pytestmark = pytest.mark.gpu
lib = C.CDLL(tn.LIB_PATH)
CDT = {0: np.complex64, 1: np.complex128}
EPS = {0: 2e-6, 1: 1e-14}


def rnd(rng, shape, dt):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dt)


def jacobi(a, dtype):
    m, n = a.shape
    A = np.asfortranarray(a.astype(CDT[dtype]))
    V = np.zeros((n, n), dtype=CDT[dtype], order="F")
    sw = C.c_int()
    rc = lib.tnqs_dbg_jacobi(dtype, m, n, A.ctypes.data_as(C.c_void_p), V.ctypes.data_as(C.c_void_p), C.byref(sw))
    assert rc == 0, lib.tnqs_last_error()
    return A, V, sw.value


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("shape", [(3, 3), (6, 6), (12, 12), (12, 6), (17, 9), (40, 40), (64, 64), (128, 128), (130, 70), (1, 1), (5, 2), (256, 256),
                                   (96, 96), (80, 48)])         # six rows per lane: full tiles (f64: V recovered) and the guarded path with V in LDS
def test_jacobi_svd(dtype, shape):
    rng = np.random.default_rng(sum(shape) + dtype)
    a = rnd(rng, shape, np.complex128)
    A, V, sw = jacobi(a, dtype)
    eps = EPS[dtype] * max(shape)
    e_s, e_rec, e_off = svd_ref.jacobi_errors(a, A, V)                                  # (shared with the batched SVD stage: tests/test_gpu_site_svd_stage.py)
    assert sw < 60      # rows >= columns is required (wide matrices are handled through their adjoint)
    assert e_s < eps
    assert np.max(np.abs(V.conj().T @ V - np.eye(shape[1]))) < 4 * eps                  # V unitary (recovered V: eps*cond)
    assert e_rec < 4 * eps                                                              # A_in = (U S) V^dagger (V may be recovered: eps*cond)
    assert e_off < eps                                                                  # columns orthogonal


@pytest.mark.parametrize("n,rank", [(6, 3), (12, 5), (64, 20), (8, 8)])
def test_jacobi_hermitian_psd_rank_deficient(n, rank):
    rng = np.random.default_rng(n)
    b = rnd(rng, (rank, n), np.complex128)
    g = b.conj().T @ b
    A, V, sw = jacobi(g, 1)
    lam = np.real(np.sum(V.conj() * A, axis=0))                                          # Rayleigh quotients
    ref = np.linalg.eigvalsh(g)
    assert np.max(np.abs(np.sort(lam) - ref)) < 1e-12 * ref[-1]
    keep = lam > 1e-12 * lam.max()
    assert keep.sum() == rank
    rec = (V[:, keep] * lam[keep]) @ V[:, keep].conj().T
    assert np.max(np.abs(rec - g)) < 1e-12 * ref[-1]


def fiber_ref(x, X, D, PA, K, PB, Do, No):
    t = x.reshape(PB, K, PA, D).transpose(3, 2, 1, 0)            # [s, a, k, b]
    Xm = X.reshape(No, Do, K, D).transpose(3, 2, 1, 0)           # [s, k, s', n]
    out = np.einsum("sakb,sktn->tanb", t.astype(np.complex128), Xm.astype(np.complex128))
    return out.transpose(3, 2, 1, 0).reshape(-1)                 # memory order: s' fastest, then a, n, b


def c128_routes(D, PA, K, PB, Do, No, same):
    """what a single ComplexF64 item runs on with the matrix cores on, from the HOST ONLY modes of tnqs_dbg_fiber_pass_c128 (the epilogue's rules with 12 tiles per
    workgroup, as tnqs_dbg_fiber_gemm plans) and tnqs_dbg_gram_c128 (gram_route, as tnqs_dbg_gram asks it): (fiber route, Gram route), TNQS_DBG_ROUTE_*"""
    IP = C.POINTER(C.c_int)
    fs = (C.c_int * 6)(D, PA, K, PB, Do, No); gs = (C.c_int * 4)(D, PA, K, PB); one = (C.c_int * 1)(1); sm = (C.c_int * 1)(int(same)); fr, gr = C.c_int(-1), C.c_int(-1)
    lib.tnqs_dbg_fiber_pass_c128.argtypes = [C.c_int, C.c_int, C.c_int, IP, IP, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, IP, IP, IP, IP]
    lib.tnqs_dbg_gram_c128.argtypes = [C.c_int, C.c_int, IP, IP, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, IP, C.c_int, IP]
    assert lib.tnqs_dbg_fiber_pass_c128(1, 1, 1, fs, one, None, None, None, None, 12, 0, C.byref(fr), None, None, None) == 0, lib.tnqs_last_error()
    assert lib.tnqs_dbg_gram_c128(1, 1, gs, sm, None, None, None, 0, None, 0, C.byref(gr)) == 0, lib.tnqs_last_error()
    return fr.value, gr.value


FIBER_GENERIC, FIBER_F64_GENERAL, GRAM_GENERIC, GRAM_F64IN = 15, 17, 18, 19      # TNQS_DBG_ROUTE_* (include/tnqs_debug.h)


# (1, 1): ComplexF64 with the matrix cores on -- mfma_fiber_gemm_f64_kernel<.., true> (kernels_f64.hip) where 4 <= D K <= 64 and Do No <= 64, else the vector kernel
# (the shapes with D K > 64 or D K < 4); which of the two is asserted below before the numbers
@pytest.mark.parametrize("dtype,mfma", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("D,PA,K,PB,Do,No", [(2, 64, 64, 8, 2, 64), (1, 128, 64, 16, 1, 64), (2, 4, 64, 70, 2, 40), (1, 64, 32, 64, 1, 32), (2, 32, 32, 32, 2, 32), (2, 128, 32, 4, 2, 17), (1, 2, 32, 200, 1, 32), (2, 16, 16, 70, 2, 5),
                                             (1, 2, 3, 5, 1, 3), (1, 100, 10, 7, 1, 10), (1, 1, 7, 130, 1, 7), (2, 9, 5, 4, 2, 3),
                                             (2, 1, 1, 1, 2, 1), (2, 300, 1, 1, 2, 1), (1, 64, 32, 33, 1, 32), (2, 16, 16, 16, 2, 16),
                                             (3, 5, 4, 6, 3, 2), (2, 70, 8, 3, 2, 11),
                                             # D K = 64 with fewer than 32 fibers below the leg: the shapes of the register-direct kernels' second addressing mode (rows_b),
                                             # here on mfma_fiber_gemm_w_kernel -- the register-direct kernels themselves: test_rowgemm_on_the_fiber_gemm_shapes
                                             (2, 1, 32, 64, 2, 32), (2, 8, 32, 16, 2, 32), (1, 16, 64, 8, 1, 64), (1, 4, 64, 32, 1, 40), (2, 2, 32, 48, 2, 9)])
def test_fiber_gemm(dtype, mfma, D, PA, K, PB, Do, No):
    rng = np.random.default_rng(D + PA + K + PB)
    dt = CDT[dtype]
    x = rnd(rng, D * PA * K * PB, dt)
    X = rnd(rng, D * K * Do * No, dt)
    out = np.zeros(Do * PA * No * PB, dtype=dt)
    n2 = C.c_double()
    if dtype == 1 and mfma == 1:
        assert c128_routes(D, PA, K, PB, Do, No, True)[0] == (FIBER_F64_GENERAL if 4 <= D * K <= 64 and Do * No <= 64 else FIBER_GENERIC)
    rc = lib.tnqs_dbg_fiber_gemm(dtype, D, PA, K, PB, Do, No, x.ctypes.data_as(C.c_void_p), X.ctypes.data_as(C.c_void_p),
                                 out.ctypes.data_as(C.c_void_p), C.byref(n2), mfma)
    assert rc == 0, lib.tnqs_last_error()
    ref = fiber_ref(x, X, D, PA, K, PB, Do, No)
    scale = np.max(np.abs(ref))
    assert np.max(np.abs(out - ref)) < EPS[dtype] * D * K * scale
    assert abs(n2.value - np.sum(np.abs(ref) ** 2)) < 1e-5 * np.sum(np.abs(ref) ** 2)


@pytest.mark.parametrize("dtype,acc64,mfma", [(0, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, 1), (0, 1, 1), (1, 1, 1)])       # (1, 1, 1): ComplexF64 operands with the matrix cores on (D K > 64 or < 4: the vector kernel; asserted below)
@pytest.mark.parametrize("D,PA,K,PB,same", [(2, 64, 64, 16, 1), (2, 2, 64, 300, 1), (1, 64, 64, 32, 0), (2, 1024, 32, 32, 1), (2, 32, 32, 1000, 1), (2, 1, 32, 1024, 1), (2, 77, 19, 11, 1), (1, 64, 32, 1024, 0), (1, 2048, 32, 32, 0), (1, 2, 32, 700, 1), (1, 70, 17, 9, 0),
                                           (1, 2, 3, 5, 0), (1, 100, 10, 7, 0), (1, 1, 7, 130, 1), (2, 9, 5, 40, 1), (2, 30, 1, 1, 0),
                                           (1, 64, 32, 33, 0), (2, 16, 16, 16, 1), (2, 512, 32, 8, 1), (3, 5, 5, 6, 0),
                                           # the element-wise tile fill of the matrix-core kernels (more k-slices per thread than the register prefetch holds;
                                           # tiles are TA = min(PA, 64), TB = min(PB, max(1, 64 / TA))):
                                           # KK = 30, D = 3: one-element units, TA = 5, TB = 12, U = 180 units, KP = 1 and K = 10 > 8 -- mfma_gram32_kernel with Y != X
                                           # (mfma = 1, f32 accumulation), a full tile and an edge tile of one b (PB = 13; with PB < 12 the tile is smaller and KP = 2)
                                           (3, 5, 10, 13, 0),
                                           # KK = 40, PA odd: one-element units, TA = 3, TB = 21, U = 63, KP = 4 and K / KP = 10 > 8 -- mfma_gram64_f64_kernel<false>
                                           # (mfma = 1, acc64 = 1), two full tiles and an edge tile
                                           (1, 3, 40, 50, 1)])
def test_gram(dtype, acc64, mfma, D, PA, K, PB, same):
    if mfma and not acc64 and D * K > 32:
        pytest.skip('f32 MFMA Gram covers D*K <= 32')
    if mfma and acc64 and dtype == 0 and not (same and 16 <= D * K <= 64):
        pytest.skip('f64 MFMA Gram covers X == Y, 16 <= D*K <= 64')
    rng = np.random.default_rng(D + PA + K + PB)
    dt = CDT[dtype]
    x = rnd(rng, D * PA * K * PB, dt)
    y = x if same else rnd(rng, D * PA * K * PB, dt)
    KK = D * K
    odt = np.complex128 if (acc64 or dtype == 1) else np.complex64
    out = np.zeros(KK * KK, dtype=odt)
    if dtype == 1 and mfma == 1:      # mfma_gram_f64in_kernel where 4 <= D K <= 64, else the vector kernel: asserted before the numbers
        assert c128_routes(D, PA, K, PB, D, K, same)[1] == (GRAM_F64IN if 4 <= KK <= 64 else GRAM_GENERIC)
    rc = lib.tnqs_dbg_gram(dtype, D, PA, K, PB, x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p),
                           out.ctypes.data_as(C.c_void_p), acc64, mfma)
    assert rc == 0, lib.tnqs_last_error()
    tx = x.reshape(PB, K, PA, D).transpose(3, 1, 2, 0).reshape(D, K, -1).astype(np.complex128)   # [s, k, (a,b)]
    ty = y.reshape(PB, K, PA, D).transpose(3, 1, 2, 0).reshape(D, K, -1).astype(np.complex128)
    mx = tx.transpose(1, 0, 2).reshape(KK, -1)        # row index s + D*k  -> reshape from [k, s]
    my = ty.transpose(1, 0, 2).reshape(KK, -1)
    ref = (mx @ my.conj().T).T.reshape(-1)            # out[i + KK*j]
    tol = (1e-13 if odt == np.complex128 and dtype == 1 else (1e-6 if acc64 else 3e-5)) * np.max(np.abs(ref))
    assert np.max(np.abs(out - ref)) < tol * max(1.0, np.sqrt(PA * PB / 64))


@pytest.mark.parametrize("chi,bleg", [((16, 16, 16, 16), 0), ((16, 16, 16, 16), 1), ((16, 16, 16, 16), 3), ((16, 16, 16), 2), ((16, 16, 8, 16, 4), 3),
                                      ((32, 32, 32, 32), 0), ((32, 32, 32, 32), 2), ((32, 32, 32, 32), 3), ((32, 32, 32), 1)])
def test_gauge_leg_inside_the_f64_gram(chi, bleg):
    """the gate path's fused kernels (kernels_gate.hip): the last gauge leg r (the lowest leg that is not the bond) absorbed inside the f64
    Gram over the (s, bond) columns -- mfma_gauge_gram64_kernel (chi = 32) and the wave-private mfma_gauge_gram32_kernel (chi = 16), bond leg 0
    (lanes along the bond index) and >= 1 -- against numpy in f64: G = X'^dagger X' of X' = X x_r M.  The kernels round X' to f32 and add
    the squares up in f64, so the difference to the all-f64 reference is the f32 rounding of X' (three-multiplication product: normwise)."""
    lib.tnqs_dbg_gauge_gram.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    rng = np.random.default_rng(sum(chi) + bleg)
    z = len(chi); K = chi[bleg]; KK = 2 * K; r = 1 if bleg == 0 else 0
    n = 2 * int(np.prod(chi))
    x = rnd(rng, n, np.complex64); m = rnd(rng, chi[r] * chi[r], np.complex64)
    out = np.zeros(KK * KK, dtype=np.complex128)
    rc = lib.tnqs_dbg_gauge_gram(z, (C.c_int * z)(*chi), bleg, x.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    assert rc == 0, lib.tnqs_last_error()
    X = x.reshape((2,) + tuple(chi), order="F").astype(np.complex128)              # [s, l0, l1, ...]
    mm = m.reshape(chi[r], chi[r], order="F").astype(np.complex128)                # M[r, r'] at r + chi r'
    Xp = np.moveaxis(np.tensordot(X, mm, axes=([1 + r], [0])), -1, 1 + r)          # X x_r M
    cols = np.moveaxis(Xp, 1 + bleg, 1).reshape(KK, -1, order="F")                 # rows i = s + 2 k
    ref = (cols @ cols.conj().T).reshape(-1, order="F")                            # out[i + KK j] = sum X'[i, .] conj(X'[j, .])
    err = np.max(np.abs(out - ref)) / np.max(np.abs(ref))
    print(f"chi {chi} bond leg {bleg}: fused gauge + Gram against f64 numpy, relative {err:.1e}")
    assert err < 1e-6            # measured 4e-9 ... 3e-8


@pytest.mark.parametrize("PA,K,PB", [(64, 32, 64), (2048, 32, 8), (2, 32, 32 * 33), (64, 17, 40), (2, 9, 64)])
def test_gram_fused_mode_product(PA, K, PB):
    """fused (X x_r M) + Gram: r = first row leg; rows of a 64-fiber tile are (s:2, i_r:32)"""
    rng = np.random.default_rng(PA + K + PB)
    dt = np.complex64
    x = rnd(rng, PA * K * PB, dt); y = rnd(rng, PA * K * PB, dt); m = rnd(rng, 32 * 32, dt)
    out = np.zeros(K * K, dtype=dt)
    rc = lib.tnqs_dbg_gram_fused(PA, K, PB, x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p),
                                 m.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    assert rc == 0, lib.tnqs_last_error()
    mm = m.reshape(32, 32).T.astype(np.complex128)                      # M[i, j] stored at i + 32 j
    if PA >= 64:        # element (a, k, b), a = s + 2*i + 64*a'
        tx = x.reshape(PB, K, PA // 64, 32, 2).astype(np.complex128)    # [b, k, a', i, s]
        ty = y.reshape(PB, K, PA // 64, 32, 2).astype(np.complex128)
        tx = np.einsum("bkais,ij->bkajs", tx, mm)
        ref = np.einsum("bkajs,bqajs->kq", tx, ty.conj())
    else:               # PA == 2 (a = s), first row leg = fastest part of b
        tx = x.reshape(PB // 32, 32, K, 2).astype(np.complex128)        # [b', i, k, s]
        ty = y.reshape(PB // 32, 32, K, 2).astype(np.complex128)
        tx = np.einsum("biks,ij->bjks", tx, mm)
        ref = np.einsum("bjks,bjqs->kq", tx, ty.conj())
    got = out.reshape(K, K).T                                            # out[i + K j]
    assert np.max(np.abs(got - ref)) < 2e-5 * np.max(np.abs(ref)) * max(1.0, np.sqrt(PA * PB / 64))


@pytest.mark.parametrize("C0,NMID,NHI", [(64, 1, 4), (16, 1, 1), (64, 32, 1), (2048, 1, 1), (32, 3, 2)])
def test_pair_mode_products(C0, NMID, NHI):
    """two slow 32-dimensional legs absorbed in one pass (16 companions per workgroup)"""
    rng = np.random.default_rng(C0 + NMID + NHI)
    dt = np.complex64
    n = C0 * 32 * NMID * 32 * NHI
    x = rnd(rng, n, dt); mx = rnd(rng, 1024, dt); my = rnd(rng, 1024, dt)
    out = np.zeros(n, dtype=dt)
    rc = lib.tnqs_dbg_pair(C0, NMID, NHI, x.ctypes.data_as(C.c_void_p), mx.ctypes.data_as(C.c_void_p), my.ctypes.data_as(C.c_void_p),
                           out.ctypes.data_as(C.c_void_p))
    assert rc == 0, lib.tnqs_last_error()
    t = x.reshape(NHI, 32, NMID, 32, C0).astype(np.complex128)             # [hi, iy, mid, ix, c]
    Mx = mx.reshape(32, 32).T.astype(np.complex128); My = my.reshape(32, 32).T.astype(np.complex128)     # M[i, j] at i + 32 j
    ref = np.einsum("hymxc,xa,yb->hbmac", t, Mx, My).reshape(-1)
    assert np.max(np.abs(out - ref)) < 3e-5 * np.max(np.abs(ref))


def _site(rng, d, chi):
    """site tensor [d][chi_0]..[chi_{z-1}] column-major as a numpy array indexed [s, i_0, ..., i_{z-1}]"""
    shp = (d,) + tuple(chi)
    flat = rnd(rng, int(np.prod(shp)), np.complex64)
    return flat, flat.reshape(shp[::-1]).transpose(*range(len(shp) - 1, -1, -1)).astype(np.complex128)


PAIR_SHAPES = [((32, 32, 32), 1, 2), ((32, 32, 32), 0, 1), ((32, 32, 32), 0, 2), ((32, 32, 32), 2, 0), ((8, 32, 32), 1, 2), ((32, 32, 8), 0, 1),
               ((32, 32, 8, 4), 0, 1), ((32, 16, 32, 2), 0, 2), ((32, 32, 4, 32), 1, 3), ((32, 8, 32, 32), 3, 0), ((32, 32, 32, 32), 0, 3), ((32, 32, 32, 32), 2, 1)]


@pytest.mark.parametrize("chi,lx,ly", PAIR_SHAPES)
def test_pair_mode_products_on_arbitrary_legs(chi, lx, ly):
    """pair kernel with the general companion geometry (leg 0 included: only the 2-dim site index is faster)"""
    rng = np.random.default_rng(sum(chi) + 7 * lx + ly)
    z = len(chi)
    flat, t = _site(rng, 2, chi)
    mx = rnd(rng, 1024, np.complex64); my = rnd(rng, 1024, np.complex64)
    out = np.zeros_like(flat)
    cchi = (C.c_int * z)(*chi)
    rc = lib.tnqs_dbg_pair_legs(2, z, cchi, lx, ly, flat.ctypes.data_as(C.c_void_p), mx.ctypes.data_as(C.c_void_p), my.ctypes.data_as(C.c_void_p),
                                out.ctypes.data_as(C.c_void_p))
    assert rc == 0
    Mx = mx.reshape(32, 32).T.astype(np.complex128); My = my.reshape(32, 32).T.astype(np.complex128)     # M[i, j] at i + 32 j
    ref = np.moveaxis(np.tensordot(t, Mx, axes=([1 + lx], [0])), -1, 1 + lx)
    ref = np.moveaxis(np.tensordot(ref, My, axes=([1 + ly], [0])), -1, 1 + ly)
    got = out.reshape((2,) + tuple(chi), order="F")
    assert np.max(np.abs(got - ref)) < 3e-5 * np.max(np.abs(ref))


@pytest.mark.parametrize("chi,lx,ly", PAIR_SHAPES)
def test_pair_gram_on_arbitrary_legs(chi, lx, ly):
    """last absorption (leg lx) + Gram keeping leg ly, X and Y different tensors"""
    rng = np.random.default_rng(sum(chi) + 5 * lx + ly)
    z = len(chi)
    fx, tx = _site(rng, 2, chi); fy, ty = _site(rng, 2, chi)
    m = rnd(rng, 1024, np.complex64)
    out = np.zeros(1024, dtype=np.complex64)
    cchi = (C.c_int * z)(*chi)
    rc = lib.tnqs_dbg_pair_gram(2, z, cchi, lx, ly, fx.ctypes.data_as(C.c_void_p), fy.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p),
                                out.ctypes.data_as(C.c_void_p))
    assert rc == 0
    M = m.reshape(32, 32).T.astype(np.complex128)
    xm = np.moveaxis(np.tensordot(tx, M, axes=([1 + lx], [0])), -1, 1 + lx)
    axes = [a for a in range(z + 1) if a != 1 + ly]
    ref = np.tensordot(xm, ty.conj(), axes=(axes, axes))               # [b, b']
    got = out.reshape(32, 32).T                                          # out[b + 32 b']
    assert np.max(np.abs(got - ref)) < 3e-5 * np.max(np.abs(ref)) * max(1.0, np.sqrt(tx.size / 65536))


@pytest.mark.parametrize("chi,lx,ly", PAIR_SHAPES)
def test_double_pair_gram(chi, lx, ly):
    """both messages of a plane from one pass over (X, Y): the second one reads the same LDS planes transposed"""
    rng = np.random.default_rng(sum(chi) + 3 * lx + ly)
    z = len(chi)
    fx, tx = _site(rng, 2, chi); fy, ty = _site(rng, 2, chi)
    mx = rnd(rng, 1024, np.complex64); my = rnd(rng, 1024, np.complex64)
    oy = np.zeros(1024, dtype=np.complex64); ox = np.zeros(1024, dtype=np.complex64)
    cchi = (C.c_int * z)(*chi)
    rc = lib.tnqs_dbg_pair_gram2(2, z, cchi, lx, ly, fx.ctypes.data_as(C.c_void_p), fy.ctypes.data_as(C.c_void_p), mx.ctypes.data_as(C.c_void_p),
                                 my.ctypes.data_as(C.c_void_p), oy.ctypes.data_as(C.c_void_p), ox.ctypes.data_as(C.c_void_p))
    assert rc == 0
    Mx = mx.reshape(32, 32).T.astype(np.complex128); My = my.reshape(32, 32).T.astype(np.complex128)
    scale = max(1.0, np.sqrt(tx.size / 65536))
    for (absorbed, kept, M, got) in ((lx, ly, Mx, oy), (ly, lx, My, ox)):
        xm = np.moveaxis(np.tensordot(tx, M, axes=([1 + absorbed], [0])), -1, 1 + absorbed)
        axes = [a for a in range(z + 1) if a != 1 + kept]
        ref = np.tensordot(xm, ty.conj(), axes=(axes, axes))
        assert np.max(np.abs(got.reshape(32, 32).T - ref)) < 3e-5 * np.max(np.abs(ref)) * scale


@pytest.mark.parametrize("D,PA,K,PB", [(2, 64, 32, 64), (1, 128, 64, 32), (2, 1, 32, 2048)])
def test_bf16x3_fiber_gemm_and_gram_are_f32_accurate(D, PA, K, PB):
    """the other kernels of the bf16 x 3 route (csrc/kernels_x3.hip: x3_rowgemm64_kernel -- chi = 32 epilogue with the site index folded in, chi = 64 mode
    product -- and x3_gram64_kernel, reached through tnqs_dbg_rowgemm / tnqs_dbg_gram_mfma, which report the kernel that ran) against f64 references, held to
    f32-class bounds: 1e-6 of the largest entry for the 64-term products, 3e-6 for the Gram's sums of PA PB terms (the generic tests above allow EPS D K = 4e-5
    resp. 3e-5)"""
    if NO_X3:
        pytest.skip("the bf16 x 3 kernels are switched off in this process")
    res, route = rowgemm(D, K, [(PA, PB, K)], seed=PA + PB)
    assert route == ROUTE_X3
    (out, ref, _), = res
    assert np.max(np.abs(out - ref)) < 1e-6 * np.max(np.abs(ref))
    if D * K == 64 and PA * PB >= 64:
        ((g, gref),), groute = gram_mfma([(D, PA, K, PB)], False)
        assert groute == ROUTE_X3
        assert np.max(np.abs(g - gref)) < 3e-6 * np.max(np.abs(gref))


@pytest.mark.parametrize("D,PA,K,PB", [(2, 64, 32, 64), (1, 128, 64, 32), (2, 1, 32, 2048)])
def test_mfma_fiber_gemm_and_vector_gram_are_f32_accurate(D, PA, K, PB):
    """the same shapes through tnqs_dbg_fiber_gemm (mfma_fiber_gemm_w_kernel) and tnqs_dbg_gram (KK = 64 without f64 accumulation: the vector Gram of
    kernels.hip), at the same bounds"""
    rng = np.random.default_rng(D + PA + K + PB)
    x = rnd(rng, D * PA * K * PB, np.complex64)
    X = rnd(rng, D * K * D * K, np.complex64)
    out = np.zeros(D * PA * K * PB, dtype=np.complex64)
    n2 = C.c_double()
    assert lib.tnqs_dbg_fiber_gemm(0, D, PA, K, PB, D, K, x.ctypes.data_as(C.c_void_p), X.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.byref(n2), 1) == 0
    ref = fiber_ref(x, X, D, PA, K, PB, D, K)
    assert np.max(np.abs(out - ref)) < 1e-6 * np.max(np.abs(ref))
    if D * K == 64 and PA * PB >= 64:
        y = rnd(rng, D * PA * K * PB, np.complex64)
        KK = D * K
        g = np.zeros(KK * KK, dtype=np.complex64)
        assert lib.tnqs_dbg_gram(0, D, PA, K, PB, x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p), 0, 1) == 0
        gref = gram_ref(x, y, D, PA, K, PB)
        assert np.max(np.abs(g - gref)) < 3e-6 * np.max(np.abs(gref))


@pytest.mark.parametrize("lx,ly", [(1, 2), (0, 3), (2, 0)])
@pytest.mark.parametrize("scale", [1e-36, 1e-12, 1e-3, 1e6])
def test_bf16x3_plane_kernels_are_f32_accurate(lx, ly, scale):
    """round 5: the chi = 32 plane kernels multiply on the bf16 matrix cores -- every f32 operand split EXACTLY into three bf16 pieces, six of the nine piece
    products kept (the dropped ones are below one f32 rounding of the product), f32 accumulation (csrc/kernels_x3.hip).  That is f32 arithmetic, not bf16
    arithmetic: against an f64 reference the error has to be what the f32 matrix instructions give (measured on the same inputs, profiles/x3_error.py:
    3.0-5.6e-7 of the largest entry for the split route, 2.6-6.2e-7 for v_mfma_f32_32x32x2_f32; a bf16-rounded operand alone would give 4e-3), at any
    scale of the data (bf16 has the exponent range of f32: no scaling anywhere).  Bound: 1e-6 of the largest entry, thirty times tighter than the generic
    kernel tests above."""
    rng = np.random.default_rng(11 * lx + ly)
    chi = (32, 32, 32, 32); z = 4
    cchi = (C.c_int * z)(*chi)
    fx, tx = _site(rng, 2, chi); fy, ty = _site(rng, 2, chi)
    fx *= np.float32(scale); tx = tx * float(np.float32(scale)); fy *= np.float32(scale); ty = ty * float(np.float32(scale))
    # data at 1e-36 (round-5 verdict: the untested corner): the LOW bf16 piece of an operand below ~2^-110 is a denormal and the matrix cores flush it -- the kernels
    # themselves lose 16-bit instead of 24-bit operands there (measured 1.5e-5; asserted as the documented bound, 1e-4).  Data of that size are outside the domain
    # of the ComplexF32 path on ANY route (test_gate_path_is_scale_invariant_where_f32_is below)
    tol = 1e-4 if scale < 1e-30 else 1e-6
    mx = rnd(rng, 1024, np.complex64); my = rnd(rng, 1024, np.complex64)
    Mx = mx.reshape(32, 32).T.astype(np.complex128); My = my.reshape(32, 32).T.astype(np.complex128)
    out = np.zeros_like(fx)
    assert lib.tnqs_dbg_pair_legs(2, z, cchi, lx, ly, fx.ctypes.data_as(C.c_void_p), mx.ctypes.data_as(C.c_void_p), my.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == 0
    ref = np.moveaxis(np.tensordot(tx, Mx, axes=([1 + lx], [0])), -1, 1 + lx)
    ref = np.moveaxis(np.tensordot(ref, My, axes=([1 + ly], [0])), -1, 1 + ly)
    assert np.max(np.abs(out.reshape((2,) + chi, order="F") - ref)) < tol * np.max(np.abs(ref))
    if scale < 1e-30:
        return          # (the Gram of two tensors at 1e-36 underflows in f32 on any route: 1e-72)
    oy = np.zeros(1024, dtype=np.complex64); ox = np.zeros(1024, dtype=np.complex64)
    assert lib.tnqs_dbg_pair_gram2(2, z, cchi, lx, ly, fx.ctypes.data_as(C.c_void_p), fy.ctypes.data_as(C.c_void_p), mx.ctypes.data_as(C.c_void_p),
                                   my.ctypes.data_as(C.c_void_p), oy.ctypes.data_as(C.c_void_p), ox.ctypes.data_as(C.c_void_p)) == 0
    for (absorbed, kept, M, got) in ((lx, ly, Mx, oy), (ly, lx, My, ox)):
        xm = np.moveaxis(np.tensordot(tx, M, axes=([1 + absorbed], [0])), -1, 1 + absorbed)
        axes = [a for a in range(z + 1) if a != 1 + kept]
        ref = np.tensordot(xm, ty.conj(), axes=(axes, axes))
        assert np.max(np.abs(got.reshape(32, 32).T - ref)) < 2 * tol * np.max(np.abs(ref))


@pytest.mark.parametrize("scale", [1e-7, 1e-3, 1e4])
def test_gate_path_is_scale_invariant_where_f32_is(scale):
    """where does the corner above begin to matter?  Nowhere the ComplexF32 path itself works.  theta = gate . R1 R2 carries the product of the two site tensors'
    norms and the truncation rule squares its singular values IN THE DATA'S PRECISION (NDTensors truncate! on P = S^2; gate_finish_kernel does the same on
    purpose): with tensor norms of 1e-12, P = 1e-48 is zero in f32 and every bond is cut to dimension 1 -- in the reference's ComplexF32 arithmetic as much as
    here (measured on this path: chi' = 1 and error 0 at 1e-12, NaN at 1e12) -- long before an entry reaches 2^-110 = 8e-34.  Inside that domain the bf16 split
    is exact: one colour group of Rzz gates with unset (identity) messages and normalize_tensors on tensors at 1e-7, 1e-3 and 1e4 against the same tensors at 1:
    the gauge-invariant results -- spectrum (the bond messages diag(S)), truncation errors, <Z> on the gate vertices -- agree to f32 rounding."""
    g = tn.named_grid((4, 4)); chi = 32
    rng = np.random.default_rng(5)
    tens = {v: rnd(rng, (2,) + (chi,) * g.degree(v), np.complex64) / np.float32(np.sqrt(2.0 * chi ** g.degree(v))) for v in g.vertices}
    grp = tn.edge_color(g, 4)[0]
    layer = [("Rzz", [a, b], 0.3) for (a, b) in grp]
    outs = []
    for sc in (1.0, scale):
        b = tn.BeliefPropagationCache(tn.tensornetworkstate(np.complex64, lambda v: "↑", g))
        for v in g.vertices:
            b._set_tensor(v, tens[v] * np.float32(sc))
        b, errs = tn.apply_gates(layer, b, apply_kwargs=dict(maxdim=chi, cutoff=1e-10, normalize_tensors=True), update_cache=False)
        outs.append(([np.diag(b.message(e)).real for e in grp], errs, tn.expect_all(b, "Z").real, [b.bond_dim(a, c) for (a, c) in grp]))
    (s1, e1, z1, d1), (s2, e2, z2, d2) = outs
    assert d1 == d2 == [chi] * len(grp)
    assert max(np.max(np.abs(a - b)) / np.max(a) for a, b in zip(s1, s2)) < 3e-6
    assert np.max(np.abs(e1 - e2)) < 2e-5 * float(np.max(e1))
    assert np.max(np.abs(z1 - z2)) < 1e-5


@pytest.mark.parametrize("shape,rank", [((64, 64), 64), ((128, 128), 64), ((144, 144), 72), ((200, 120), 120)])
@pytest.mark.parametrize("scale", [1e-18, 1e-10, 1e-5, 1.0, 1e12])
def test_jacobi_svd_is_scale_invariant(shape, rank, scale):
    """ComplexF32: the sweeps square inner products, which underflows for matrices of small magnitude (singular values of 1e-5 are
    enough: the rotation phases of the smaller columns lose their unit modulus).  Both kernels (LDS-resident up to 136 rows here, global
    memory beyond) scale the matrix by an exact power of two first.  Before that fix the global-memory kernel returned singular values
    off by 20-40 % for theta matrices of chi >= 36 whose tensors carried a small norm; the LDS kernel skipped rotations below 1e-36."""
    rng = np.random.default_rng(shape[0] + rank)
    m, n = shape
    b0 = (rnd(rng, (m, rank), np.complex128) @ rnd(rng, (rank, n), np.complex128)) / rank
    b = (b0 * scale).astype(np.complex64)
    s_ref = np.linalg.svd(b.astype(np.complex128), compute_uv=False)
    A, V, sw = jacobi(b, 0)
    s = np.sort(np.linalg.norm(A.astype(np.complex128), axis=0))[::-1]
    assert sw < 60
    assert np.max(np.abs(s[:len(s_ref)] - s_ref)) < 3e-5 * s_ref[0]
    assert np.all(np.isfinite(V))
    if scale >= 1e-15:                                   # V is recovered by an f32 GEMM of theta0 with U Sigma: its products underflow below ~1e-18;
        rec = (A.astype(np.complex128) @ V.conj().T.astype(np.complex128))      # inside the engine theta is scaled to O(1) first (theta_scale_kernel)
        assert np.max(np.abs(rec - b)) < 2e-5 * s_ref[0]


@pytest.mark.parametrize("shape,rank", [((128, 64), 64), ((128, 64), 20), ((128, 40), 40), ((64, 64), 64), ((100, 33), 33), ((256, 64), 48), ((72, 8), 8),
                                        ((130, 70), 70), ((40, 40), 3)])
@pytest.mark.parametrize("scale", [1e-9, 1.0, 1e6])
def test_theta_svd_kernel(shape, rank, scale, monkeypatch):
    """the engine's theta SVD route at the shapes a gate batch produces (one-sided f32 sweeps on A in LDS, V not accumulated but recovered from
    the unrotated copy): singular values against LAPACK relative to the largest one, the reconstruction A = (U Sigma) V^dagger, and -- what
    the V recovery depends on -- the orthogonality of the columns of U Sigma relative to their OWN norms, for full-rank, rank-deficient and
    badly scaled inputs with spectra spread over 3.5 decades"""
    monkeypatch.setenv("TNQS_DBG_THETA_SVD", "1")
    rng = np.random.default_rng(shape[0] + 7 * rank)
    m, n = shape
    dec = np.exp(-np.arange(rank) * (8.0 / max(rank, 1)))                    # singular values spread over 3.5 decades, as a truncating theta has them
    q1, _ = np.linalg.qr(rnd(rng, (m, rank), np.complex128)); q2, _ = np.linalg.qr(rnd(rng, (n, rank), np.complex128))
    b = ((q1 * dec) @ q2.conj().T * scale).astype(np.complex64)
    s_ref = np.linalg.svd(b.astype(np.complex128), compute_uv=False)
    A, V, sw = jacobi(b, 0)
    A = A.astype(np.complex128)
    nrm = np.linalg.norm(A, axis=0)
    s = np.sort(nrm)[::-1]
    assert sw < 60
    assert np.max(np.abs(s[:len(s_ref)] - s_ref)) < 1e-5 * s_ref[0], (s[:4], s_ref[:4])
    big = nrm > 1e-4 * s_ref[0]                                             # columns that carry signal: mutually orthogonal relative to their own norms
    U = A[:, big] / nrm[big]
    assert np.max(np.abs(U.conj().T @ U - np.eye(U.shape[1]))) < 5e-6
    rec = A @ V.conj().T.astype(np.complex128)
    assert np.max(np.abs(rec - b)) < 2e-5 * s_ref[0]


@pytest.mark.parametrize("n", [1, 2, 5, 16, 33, 64, 65, 96, 128])
@pytest.mark.parametrize("cond", [1e2, 1e10])
def test_cholesky_kernels(n, cond):
    """chol_kernel (n <= 96: one barrier per column, unscaled trailing updates, four lanes per column of the inverse) and the packed kernel
    (n <= 128): G = L L^dagger, W = (L^-1)^dagger, against numpy in f64, for well- and ill-conditioned Gram matrices; a numerically singular
    matrix raises the failure flag instead of producing NaNs"""
    rng = np.random.default_rng(n)
    q, _ = np.linalg.qr(rnd(rng, (n, n), np.complex128))
    lam = np.logspace(0, -np.log10(cond), n)
    g = np.asfortranarray((q * lam) @ q.conj().T)
    L = np.zeros((n, n), dtype=np.complex128, order="F"); W = np.zeros((n, n), dtype=np.complex128, order="F"); fail = C.c_int(-1)
    rc = lib.tnqs_dbg_chol(n, g.ctypes.data_as(C.c_void_p), L.ctypes.data_as(C.c_void_p), W.ctypes.data_as(C.c_void_p), C.byref(fail), C.c_double(1e-12))
    assert rc == 0, tn._lib.lib.tnqs_last_error()
    assert fail.value == 0
    assert np.max(np.abs(np.triu(L, 1))) == 0 and np.all(np.diag(L).real > 0) and np.max(np.abs(np.diag(L).imag)) == 0
    assert np.max(np.abs(L @ L.conj().T - g)) < 1e-13 * n
    ref = np.linalg.cholesky(g)
    assert np.max(np.abs(L - ref)) < 1e-11 * cond ** 0.5
    assert np.max(np.abs(W.conj().T @ L - np.eye(n))) < 1e-13 * n * cond ** 0.5            # W^dagger = L^-1
    # singular: rank n - 1 (n >= 2) -> flagged, finite output
    if n >= 2:
        lam2 = lam.copy(); lam2[-1] = 0.0
        g2 = np.asfortranarray((q * lam2) @ q.conj().T)
        rc = lib.tnqs_dbg_chol(n, g2.ctypes.data_as(C.c_void_p), L.ctypes.data_as(C.c_void_p), W.ctypes.data_as(C.c_void_p), C.byref(fail), C.c_double(1e-12))
        assert rc == 0 and (fail.value == 1 or cond > 1e9) and np.all(np.isfinite(L))


# ---- preconditioned theta SVD kernel (round 5) ----------------------------------------------------------------------------------------
def theta_svd_pre(a, q=None, copies=1, reps=0, cap=0):
    """q given: a is the low-rank factor of theta = a q^T, V (nq x n) = right singular vectors of theta; q None: a is theta itself, V is n x n"""
    m, n = a.shape; nq = q.shape[0] if q is not None else n
    A = np.asfortranarray(a.astype(np.complex64)); Q = np.asfortranarray(q.astype(np.complex128)) if q is not None else None
    V = np.zeros((nq, n), dtype=np.complex64, order="F")
    sw = C.c_int(); ms = C.c_double(0.0); ph = (C.c_double * 6)()
    rc = lib.tnqs_dbg_theta_svd_pre(m, n, nq, A.ctypes.data_as(C.c_void_p), Q.ctypes.data_as(C.c_void_p) if Q is not None else None, V.ctypes.data_as(C.c_void_p), C.byref(sw),
                                    copies, reps, C.byref(ms), ph, cap)
    assert rc == 0, lib.tnqs_last_error()
    theta_svd_pre.phases_us = [round(x, 1) for x in ph]          # load, Gram, Cholesky + conversion, sweeps, U Sigma, V (workgroup 0)
    return A, V, sw.value, ms.value


def low_rank_factors(r1, r2, gate):
    """the engine's low-rank route in numpy (f64): operator-sum factors of the gate by elimination with complete pivoting, theta = A B^T, B = Q L^dagger
    (Cholesky QR), M = A conj(L) -- returns (M, Q, theta)"""
    d1 = d2 = 2
    g4 = gate.reshape(d1, d2, d1, d2)
    O = np.transpose(g4, (0, 2, 1, 3)).reshape(d1 * d1, d2 * d2).astype(np.complex128).copy()
    fa, fb, amax = [], [], np.abs(O).max()
    for _ in range(min(O.shape)):
        i, j = np.unravel_index(np.argmax(np.abs(O)), O.shape)
        if not np.abs(O[i, j]) > 1e-13 * amax:
            break
        col, row = O[:, j].copy(), O[i, :] / O[i, j]
        O -= np.outer(col, row); fa.append(col.reshape(d1, d1)); fb.append(row.reshape(d2, d2))
    R1, R2 = r1.astype(np.complex128), r2.astype(np.complex128)
    A = np.concatenate([np.einsum("xs,rsb->rxb", a, R1).reshape(R1.shape[0] * d1, -1) for a in fa], axis=1)
    B = np.concatenate([np.einsum("ys,rsb->ryb", b, R2).reshape(R2.shape[0] * d2, -1) for b in fb], axis=1)
    L = np.linalg.cholesky(B.conj().T @ B)
    Q = B @ np.linalg.inv(L).conj().T
    return A @ np.conj(L), Q, A @ B.T


def check_theta_svd_pre(M, Q, theta, sv_tol=4e-6, cap=0):
    A, V, sw, _ = theta_svd_pre(M, Q, cap=cap)
    svd_ref.check_pre(M.astype(np.complex64).astype(np.complex128), Q, theta, A, V, sw, sv_tol=sv_tol, cap=cap)      # (shared with the batched SVD stage)
    return sw


@pytest.mark.parametrize("shape,rank", [((128, 64, 128), 64), ((128, 64, 128), 20), ((128, 40, 100), 40), ((64, 64, 64), 64), ((100, 33, 80), 33), ((72, 8, 40), 8),
                                        ((40, 40, 40), 3), ((128, 64, 64), 64), ((6, 2, 4), 2)])
@pytest.mark.parametrize("scale", [1e-9, 1.0, 1e6])
def test_theta_svd_pre_kernel(shape, rank, scale):
    """synthetic factors with spectra spread over 3.5 decades, full rank and rank deficient, badly scaled: singular values against LAPACK, the reconstruction
    theta = (U Sigma) V^dagger, V orthonormal, U Sigma orthogonal to eps sigma_max"""
    m, n, nq = shape
    rng = np.random.default_rng(m + 7 * rank + n)
    dec = np.exp(-np.arange(rank) * (8.0 / max(rank, 1)))
    q1, _ = np.linalg.qr(rnd(rng, (m, rank), np.complex128)); q2, _ = np.linalg.qr(rnd(rng, (n, rank), np.complex128))
    M = (q1 * dec) @ q2.conj().T * scale
    Q, _ = np.linalg.qr(rnd(rng, (nq, n), np.complex128))
    check_theta_svd_pre(M, Q, None)
    if rank == n and n >= 8:
        check_theta_svd_pre(M, Q, None, cap=n // 2)           # only the n/2 largest triplets are formed (the bond dimension cap of a gate)
    check_theta_svd_pre(M, None, None, cap=(n // 2 if n >= 8 else 0))      # theta itself (a corner gate: no low-rank route): V = its right singular vectors


@pytest.mark.parametrize("with_q", [False, True])
def test_theta_svd_pre_kernel_on_degenerate_input(with_q):
    """round-5 advisor finding: theta identically ZERO used to come back with sigma_j = 1 on the unformed columns (largest pivot 0 -> every pivot replaced by 1) --
    weight in S and in the truncation error that the matrix does not have; a NaN entry used to be sorted to the end as a zero column instead of being reported.
    Now: zero in, zero out (U Sigma = 0, V = 0, no sweeps); NaN in, NaN kept in A (gate_finish reports TNQS_ERR_NUMERIC, like the plain Jacobi route) and V = NaN."""
    m, n, nq = 128, 64, 128
    rng = np.random.default_rng(3)
    Q = np.linalg.qr(rnd(rng, (nq, n), np.complex128))[0] if with_q else None
    A, V, sw, _ = theta_svd_pre(np.zeros((m, n), dtype=np.complex64), Q)
    assert sw == 0 and np.all(A == 0) and np.all(V == 0)
    M = rnd(rng, (m, n), np.complex64); M[5, 7] = np.nan
    A, V, sw, _ = theta_svd_pre(M, Q)
    assert sw == 0 and np.isnan(A[5, 7]) and np.all(np.isnan(V.real))
    np.testing.assert_array_equal(np.delete(A.ravel(order="F"), 5 + m * 7), np.delete(np.asfortranarray(M).ravel(order="F"), 5 + m * 7))      # nothing else was touched


def test_theta_svd_pre_kernel_on_harvested_factors():
    """R factors of two-site gates harvested from oracle runs (tests/golden/make_theta_factors.py: a random chi = 32 state after three TFIM layers, a chi = 16
    state evolved from the product state): the engine's low-rank factor M and Q built in numpy, then the kernel against LAPACK.  Sweeps: the numpy model of
    the kernel (scratch notes in DESIGN.md 4.26) needs 3-7 where the plain Jacobi on M needs 7-9"""
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "theta_factors.npz"))
    keys = sorted({k.rsplit("_", 1)[0] for k in z.files})
    sweeps = {}
    for k in keys:
        r1, r2, gate = z[k + "_r1"], z[k + "_r2"], z[k + "_gate"]
        if r1.shape[0] * 2 < r2.shape[0] * 2:           # theta wider than tall: the engine stores its adjoint and runs no low-rank route
            continue
        M, Q, theta = low_rank_factors(r1, r2, gate)
        if not (M.shape[1] <= 64 and M.shape[0] <= 128):
            continue
        sweeps[k] = check_theta_svd_pre(M, Q, theta)
    print("sweeps of the preconditioned kernel:", sweeps)
    assert len(sweeps) >= 6 and max(sweeps.values()) <= 8



# ---- the kernels of single engine launches, reached through the multi-item entry points of include/tnqs_debug.h (items set up as the engine sets them
# up; a shape the named kernel does not take is refused, and the entry point reports which kernel ran) ------------------------------------------------
ROUTE_X3, ROUTE_F32, ROUTE_F64, ROUTE_F64_SHARED, ROUTE_HALF_LINES, ROUTE_WHOLE_LINES = 1, 2, 3, 4, 5, 6
ERR_UNSUPPORTED = -2                                     # include/tnqs.h
NO_X3 = os.environ.get("TNQS_NO_BF16X3") == "1"          # the library reads the switch once per process: the f32 leg runs in a child (test_f32_matrix_core_leg)


def _ints(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.int32))


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _measured(kernel, err):
    print(f"MEASURED {kernel}: {err:.3e}")


def rowgemm(D, K, items, scale=1.0, tpw=0, seed=0, zero=False):
    """items: (PA, PB, No) -> per item (out, ref, norm2) and the route"""
    rng = np.random.default_rng(seed + 31 * K + D)
    xs, Xs, refs = [], [], []
    for (PA, PB, No) in items:
        x = rnd(rng, D * PA * K * PB, np.complex64) * np.float32(scale)
        if zero:
            x[:] = 0
        X = rnd(rng, D * K * D * No, np.complex64)
        xs.append(x); Xs.append(X); refs.append(fiber_ref(x, X, D, PA, K, PB, D, No))
    out = np.zeros(sum(r.size for r in refs), dtype=np.complex64)
    n2 = np.zeros(len(items)); route = C.c_int(0)
    PA, PB, No = (_ints([it[q] for it in items]) for q in range(3))
    rc = lib.tnqs_dbg_rowgemm(D, K, len(items), _p(PA), _p(PB), _p(No), _p(np.concatenate(xs)), _p(np.concatenate(Xs)), _p(out),
                              n2.ctypes.data_as(C.c_void_p), tpw, C.byref(route))
    assert rc == 0, lib.tnqs_last_error()
    outs = np.split(out, np.cumsum([r.size for r in refs])[:-1])
    return [(o, r, n) for o, r, n in zip(outs, refs, n2)], route.value


def rowgemm_route(D, K):
    return ROUTE_X3 if D * K == 64 and not NO_X3 else ROUTE_F32


# bounds of the register-direct kernels, relative to the largest entry of the product (inputs are seeded: the measured maxima on the MI355X are deterministic).
# bf16 x 3 (D K = 64): the documented f32-class bound 1e-6 (measured 5.9e-7), 1e-4 for data at 1e-36 (the flushed low pieces; measured 5.8e-5).
# f32 matrix instructions, about five times the measured maximum (EPS D K of test_fiber_gemm would allow 6.4e-5 ... 2.6e-4): <1,1,1> 4.1e-7, <4,4,2> 8.7e-7,
# and under TNQS_NO_BF16X3=1 <2,2,1> 6.0e-7, <2,2,2> 5.7e-7
ROWGEMM_TOL = {(ROUTE_X3, 1, 64): 1e-6, (ROUTE_X3, 2, 32): 1e-6, (ROUTE_F32, 1, 32): 2e-6, (ROUTE_F32, 2, 64): 4.5e-6,
               (ROUTE_F32, 1, 64): 3e-6, (ROUTE_F32, 2, 32): 3e-6}
ROWGEMM_NORM_TOL = 1e-6             # the norm partials (f32 squares per lane and tile, f64 across): measured 1.4e-7 of sum |ref|^2


def rowgemm_tol(D, K, tiny=False):
    r = rowgemm_route(D, K)
    return 1e-4 if (tiny and r == ROUTE_X3) else ROWGEMM_TOL[(r, D, K)]


# rows of a tile = several b-indices (PA < 32: the kernels' second addressing mode, rows_b), 32 consecutive a-indices (PA = 32, 96); PB keeps PB % (32 / PA) == 0
ROWGEMM_ITEMS = [(1, 64), (2, 48), (8, 12), (16, 6), (32, 7), (96, 3)]


@pytest.mark.parametrize("K,D", [(32, 1), (32, 2), (64, 1), (64, 2)])
@pytest.mark.parametrize("No", ["1", "5", "K-1", "K"])
@pytest.mark.parametrize("tpw", [0, 1, 8])
def test_rowgemm_multi_item_launch(K, D, No, tpw):
    """launch_mfma_rowgemm as the engine launches it (the chi = 32 gate epilogue of the headline workload: D = 2, K = 32 on x3_rowgemm64_kernel; chi = 64 mode
    product D = 1, K = 64; mfma_rowgemm_kernel<1,1,1> and <4,4,2>): six items of different PA / PB in ONE launch (binary search on tile_begin), every
    addressing mode, tail columns No < K, the engine's tiles per workgroup and forced ones with ragged last groups (tpw = 1, 8), and each item's norm
    partials against sum |ref|^2"""
    no = {"1": 1, "5": 5, "K-1": K - 1, "K": K}[No]
    res, route = rowgemm(D, K, [(PA, PB, no) for (PA, PB) in ROWGEMM_ITEMS], tpw=tpw, seed=no)
    assert route == rowgemm_route(D, K)
    err = max(np.max(np.abs(o - r)) / np.max(np.abs(r)) for o, r, _ in res)
    nerr = max(abs(n - np.sum(np.abs(r) ** 2)) / np.sum(np.abs(r) ** 2) for _, r, n in res)
    _measured(f"rowgemm route {route} D {D} K {K} No {no} tpw {tpw} (norm {nerr:.1e})", err)
    assert all(np.all(np.isfinite(o)) for o, _, _ in res)          # every output element written
    assert err < rowgemm_tol(D, K)
    assert nerr < ROWGEMM_NORM_TOL


@pytest.mark.parametrize("K,D", [(32, 1), (32, 2), (64, 1), (64, 2)])
@pytest.mark.parametrize("scale", [0.0, 1e-36, 1e-12, 1e-3, 1e6])
def test_rowgemm_scale_sweep(K, D, scale):
    """the tensor operand at any scale (the bf16 split keeps the f32 exponent range: no scaling anywhere).  At 1e-36 the low bf16 piece of an operand is a
    denormal that the matrix cores flush: the documented bound 1e-4 (test_bf16x3_plane_kernels_are_f32_accurate).  Scale 0: exact zeros and norm^2 0."""
    items = [(2, 32, K), (32, 5, K - 1), (16, 4, 5)]
    res, route = rowgemm(D, K, items, scale=scale or 1.0, zero=scale == 0.0, seed=7)
    assert route == rowgemm_route(D, K)
    if scale == 0.0:
        for o, _, n in res:
            assert np.all(o == 0) and n == 0.0
        return
    err = max(np.max(np.abs(o - r)) / np.max(np.abs(r)) for o, r, _ in res)
    _measured(f"rowgemm route {route} D {D} K {K} scale {scale:g}", err)
    assert err < rowgemm_tol(D, K, tiny=scale < 1e-30)
    if scale > 1e-30:               # (|out|^2 of data at 1e-36 underflows in the f32 partial sums, on any route)
        assert max(abs(n - np.sum(np.abs(r) ** 2)) / np.sum(np.abs(r) ** 2) for _, r, n in res) < ROWGEMM_NORM_TOL


def test_rowgemm_refuses_what_it_does_not_cover():
    x = np.zeros(2 * 3 * 32 * 5, dtype=np.complex64); X = np.zeros(64 * 64, dtype=np.complex64); out = np.zeros(x.size, dtype=np.complex64)
    for (D, K, PA, PB, No) in [(2, 32, 3, 5, 32), (2, 32, 4, 5, 32), (2, 32, 32, 5, 33), (3, 32, 32, 1, 32), (2, 16, 32, 1, 16), (2, 32, 48, 1, 32)]:
        assert lib.tnqs_dbg_rowgemm(D, K, 1, _p(_ints([PA])), _p(_ints([PB])), _p(_ints([No])), _p(x), _p(X), _p(out), None, 0, None) == ERR_UNSUPPORTED


def gram_ref(x, y, D, PA, K, PB):
    KK = D * K
    tx = x.reshape(PB, K, PA, D).transpose(1, 3, 2, 0).reshape(KK, -1).astype(np.complex128)   # rows s + D k
    ty = y.reshape(PB, K, PA, D).transpose(1, 3, 2, 0).reshape(KK, -1).astype(np.complex128)
    return (tx @ ty.conj().T).T.reshape(-1)                                                       # out[i + KK j]


def gram_mfma(items, same, nchunks=0, seed=0):
    rng = np.random.default_rng(seed + len(items))
    xs = [rnd(rng, int(np.prod(s)), np.complex64) for s in items]
    ys = xs if same else [rnd(rng, int(np.prod(s)), np.complex64) for s in items]
    refs = [gram_ref(x, y, *s) for x, y, s in zip(xs, ys, items)]
    f64 = max(s[0] * s[2] for s in items) > 64
    out = np.zeros(sum(r.size for r in refs), dtype=np.complex128 if f64 else np.complex64)
    route = C.c_int(0)
    rc = lib.tnqs_dbg_gram_mfma(len(items), _p(_ints(items).ravel()), _p(np.concatenate(xs)), None if same else _p(np.concatenate(ys)), _p(out), nchunks, C.byref(route))
    assert rc == 0, lib.tnqs_last_error()
    return list(zip(np.split(out, np.cumsum([r.size for r in refs])[:-1]), refs)), route.value


# 32 < KK <= 64 (KK = 40, 48, 64), fiber counts PA PB that are not multiples of 64, every item in several chunks
GRAM64_LAUNCHES = {"kk40": [(1, 7, 40, 30)], "kk48": [(2, 5, 24, 37)], "kk64": [(2, 64, 32, 3)],
                   "mixed": [(1, 7, 40, 30), (2, 5, 24, 37), (2, 64, 32, 3), (1, 3, 64, 100), (2, 1, 32, 70)]}
GRAM64_TOL = {ROUTE_X3: 1.5e-6, ROUTE_F32: 2e-6}      # relative to the largest entry; measured x3_gram64_kernel 2.8e-7, mfma_gram64_kernel 3.8e-7


@pytest.mark.parametrize("launch", sorted(GRAM64_LAUNCHES))
@pytest.mark.parametrize("same", [0, 1])
@pytest.mark.parametrize("nchunks", [0, 3])
def test_gram_mfma64(launch, same, nchunks):
    """the BP message Gram for 32 < KK <= 64 (launch_mfma_gram64: x3_gram64_kernel, mfma_gram64_kernel under TNQS_NO_BF16X3=1), X != Y and X == Y, the engine's
    chunking (one tile per chunk here) and three chunks of several tiles, several items of different KK in one launch (chunk_begin), partials reduced as the
    engine reduces them"""
    res, route = gram_mfma(GRAM64_LAUNCHES[launch], same, nchunks)
    assert route == (ROUTE_F32 if NO_X3 else ROUTE_X3)
    err = max(np.max(np.abs(o - r)) / np.max(np.abs(r)) for o, r in res)
    _measured(f"gram64 route {route} {launch} same {same} nchunks {nchunks}", err)
    assert err < GRAM64_TOL[route]


GRAM128_LAUNCHES = {"kk72": ([(2, 5, 36, 41)], ROUTE_F64), "kk72b": ([(1, 3, 72, 50)], ROUTE_F64), "kk128": ([(2, 64, 64, 3), (1, 7, 128, 30)], ROUTE_F64_SHARED),
                    "kk128x3": ([(2, 64, 64, 3), (1, 7, 128, 30), (2, 5, 64, 13)], ROUTE_F64_SHARED),      # three items of different sizes on the shared-panel kernel
                    "mixed96_128": ([(2, 5, 48, 29), (2, 3, 64, 50), (1, 2, 96, 33)], ROUTE_F64)}


@pytest.mark.parametrize("launch", sorted(GRAM128_LAUNCHES))
@pytest.mark.parametrize("nchunks", [0, 2])
def test_gram_mfma128_f64(launch, nchunks):
    """the gate-path Gram at chi = 64 (launch_mfma_gram128_f64): f32 operands, products exact in f64, f64 accumulation -- 1e-12 of the largest entry.  Both
    instantiations: <true> when every item has D K = 128 (the engine's all_kk128), <false> otherwise (KK = 72, a 96 + 128 launch)"""
    items, want = GRAM128_LAUNCHES[launch]
    res, route = gram_mfma(items, True, nchunks)
    assert route == want
    err = max(np.max(np.abs(o - r)) / np.max(np.abs(r)) for o, r in res)
    _measured(f"gram128 route {route} {launch} nchunks {nchunks}", err)
    assert err < 5e-15             # (the f64 bound 1e-12 is 1000 times the measured 9.4e-16: held to five times that)


def test_gram_mfma_refuses_what_it_does_not_cover():
    x = np.zeros(2 * 64 * 64, dtype=np.complex64); out = np.zeros(128 * 128, dtype=np.complex128)
    for items, y in [([(1, 2, 32, 3)], None), ([(2, 1, 65, 1)], None), ([(2, 2, 64, 2)], x)]:
        assert lib.tnqs_dbg_gram_mfma(len(items), _p(_ints(items).ravel()), _p(x), _p(y), _p(out), 0, None) == ERR_UNSUPPORTED


def _plane_launch(items, rng):
    """items: (chi, lx, ly) -> flat tensors, numpy tensors, matrices (Mx, My) as numpy and flat"""
    flats, ts, ms, mflat = [], [], [], []
    for (chi, lx, ly) in items:
        f, t = _site(rng, 2, chi); flats.append(f); ts.append(t)
        m = rnd(rng, 512, np.complex64); mflat.append(m)
        ms.append((m[:256].reshape(16, 16).T.astype(np.complex128), m[256:].reshape(16, 16).T.astype(np.complex128)))     # M[i, j] at i + 16 j
    z = _ints([len(c) for c, _, _ in items]); chi = _ints([x for c, _, _ in items for x in c])
    lx = _ints([it[1] for it in items]); ly = _ints([it[2] for it in items])
    return flats, ts, ms, np.concatenate(mflat), (z, chi, lx, ly)


def _absorb(t, M, leg):
    return np.moveaxis(np.tensordot(t, M, axes=([1 + leg], [0])), -1, 1 + leg)


# heavy-hex (degree 3), degree 4 with mixed legs, degree 5 and 6; planes that contain leg 0 (leg-0 branch of plane_geometry: mfma_pair16_kernel) and planes that
# do not (16 contiguous companions: mfma_pair16w_kernel)
PLANE16_HALF = [((16, 16, 16), 0, 2), ((16, 8, 16, 4), 0, 2), ((16, 4, 16, 8), 2, 0), ((16, 8, 16, 4, 16), 0, 4), ((16, 4, 16, 2, 16, 4), 4, 0)]
PLANE16_WHOLE = [((16, 16, 16), 1, 2), ((8, 16, 16, 4), 1, 2), ((16, 8, 16, 4, 16), 2, 4), ((16, 4, 16, 2, 16, 4), 2, 4), ((16, 16, 16, 16), 3, 1)]


@pytest.mark.parametrize("kind", ["half", "whole"])
@pytest.mark.parametrize("spw", [0, 4, 12])
def test_pair16_multi_item_launch(kind, spw):
    """two 16-dimensional legs absorbed in one pass (launch_mfma_pair16), all geometries of one kind in ONE launch (wg_begin), the engine's slices per
    workgroup and forced ones with ragged last groups"""
    items = PLANE16_HALF if kind == "half" else PLANE16_WHOLE
    rng = np.random.default_rng(len(items) + spw)
    flats, ts, ms, m, (z, chi, lx, ly) = _plane_launch(items, rng)
    x = np.concatenate(flats); out = np.zeros_like(x); route = C.c_int(0)
    rc = lib.tnqs_dbg_pair16(2, len(items), _p(z), _p(chi), _p(lx), _p(ly), _p(x), _p(m), _p(out), spw, C.byref(route))
    assert rc == 0, lib.tnqs_last_error()
    assert route.value == (ROUTE_HALF_LINES if kind == "half" else ROUTE_WHOLE_LINES)
    err = 0.0
    for o, t, (Mx, My), (c, a, b) in zip(np.split(out, np.cumsum([f.size for f in flats])[:-1]), ts, ms, items):
        ref = _absorb(_absorb(t, Mx, a), My, b)
        err = max(err, np.max(np.abs(o.reshape((2,) + c, order="F") - ref)) / np.max(np.abs(ref)))
    _measured(f"pair16 {kind} spw {spw}", err)
    assert err < 2e-6              # two chained 16-term f32 products; measured 3.8e-7 (half lines), 3.1e-7 (whole lines)


def test_pair16_refuses_mixed_kinds_and_uncovered_planes():
    items = [PLANE16_HALF[0], PLANE16_WHOLE[0]]
    rng = np.random.default_rng(0)
    flats, _, _, m, (z, chi, lx, ly) = _plane_launch(items, rng)
    x = np.concatenate(flats); out = np.zeros_like(x)
    assert lib.tnqs_dbg_pair16(2, 2, _p(z), _p(chi), _p(lx), _p(ly), _p(x), _p(m), _p(out), 0, None) == ERR_UNSUPPORTED
    z1, chi1 = _ints([4]), _ints([4, 16, 8, 16])        # leg 1 above 8 elements: no companion geometry
    assert lib.tnqs_dbg_pair16(2, 1, _p(z1), _p(chi1), _p(_ints([1])), _p(_ints([3])), _p(x), _p(m), _p(out), 0, None) == ERR_UNSUPPORTED


@pytest.mark.parametrize("spw", [0, 8])
def test_pair_gram2x16_both_and_single_message_items(spw):
    """both messages of a 16 x 16 plane from one pass over (X, Y) (launch_mfma_pair_gram2x16) and the single-message form of the BP update (My = null,
    no partial_x), items of both forms and both geometries in ONE launch, partials summed per message"""
    items = [PLANE16_HALF[1], PLANE16_WHOLE[2], PLANE16_HALF[0], PLANE16_WHOLE[3], PLANE16_HALF[4], PLANE16_WHOLE[1]]
    both = _ints([1, 1, 0, 0, 1, 0])
    rng = np.random.default_rng(3 + spw)
    fx, tx, ms, m, (z, chi, lx, ly) = _plane_launch(items, rng)
    fy, ty = zip(*[_site(rng, 2, c) for c, _, _ in items])
    oy = np.zeros(256 * len(items), dtype=np.complex64); ox = np.full(256 * len(items), 7, dtype=np.complex64)
    rc = lib.tnqs_dbg_pair_gram2x16(2, len(items), _p(z), _p(chi), _p(lx), _p(ly), _p(both), _p(np.concatenate(fx)), _p(np.concatenate(fy)), _p(m), _p(oy), _p(ox), spw)
    assert rc == 0, lib.tnqs_last_error()
    err = 0.0
    for i, ((c, a, b), X, Y, (Mx, My)) in enumerate(zip(items, tx, ty, ms)):
        zz = len(c)
        for (absorbed, kept, M, got) in ((a, b, Mx, oy), (b, a, My, ox)):
            g = got[256 * i: 256 * (i + 1)]
            if M is My and not both[i]:
                assert np.all(g == 7)                       # single-message item: no second message written
                continue
            axes = [q for q in range(zz + 1) if q != 1 + kept]
            ref = np.tensordot(_absorb(X, M, absorbed), Y.conj(), axes=(axes, axes))
            err = max(err, np.max(np.abs(g.reshape(16, 16).T - ref)) / np.max(np.abs(ref)))
    _measured(f"pair_gram2x16 spw {spw}", err)
    assert err < 3e-6              # measured 5.6e-7


def tall_svd(mats):
    ms = _ints([a.shape[0] for a in mats]); ns = _ints([a.shape[1] for a in mats])
    A = np.concatenate([np.asfortranarray(a.astype(np.complex64)).ravel(order="F") for a in mats])
    fail, pol, sw = (np.zeros(len(mats), dtype=np.int32) for _ in range(3))
    rc = lib.tnqs_dbg_svd_tall(len(mats), _p(ms), _p(ns), _p(A), _p(fail), _p(pol), _p(sw))
    assert rc == 0, lib.tnqs_last_error()
    outs = np.split(A, np.cumsum([a.size for a in mats])[:-1])
    return [o.reshape(a.shape, order="F").astype(np.complex128) for o, a in zip(outs, mats)], fail, pol, sw


def check_tall(a, A):
    """what test_theta_svd_kernel asserts, with the reconstruction in the form the V-less route allows: A_out = A J with J unitary <=> A_out A_out^H = A A^H"""
    b = a.astype(np.complex64).astype(np.complex128)
    if not np.any(b):
        assert np.all(A == 0)
        return 0.0
    e_s, e_o, e_r = svd_ref.tall_errors(b, A)                                           # (shared with the batched SVD stage)
    _measured("svd_tall singular values", e_s); _measured("svd_tall orthogonality", e_o); _measured("svd_tall reconstruction", e_r)
    b_s, b_o, b_r = svd_ref.TALL_BOUNDS                                             # 1e-5, 1.25e-6, 4.5e-6
    assert e_s < b_s and e_o < b_o and e_r < b_r, (e_s, e_o, e_r)                  # measured 2.9e-6, 2.5e-7, 8.6e-7
    return max(e_s, e_o, e_r)


@pytest.mark.parametrize("scale", [1e-9, 1.0, 1e6])
def test_svd_tall_route(scale):
    """svd_batch's tall route (tall_gram -> chol_packed -> tall_rt -> Jacobi on R -> tall_w -> tall_mj -> copy_items, polish where the pivot collapsed) at the
    shapes the engine sends it (m <= 512, 2 <= n <= 128): full rank, rank deficient, spectra over 3.5 decades, badly scaled -- all in one launch with an all-zero
    item (every pivot refused: tau = 0 and a shift of 1e-14 * 0; J := I, the polishing sweeps factorise it) and an item with exact zero columns next to nonzero
    ones (the shift keeps its pivots: no failure, no polish)"""
    rng = np.random.default_rng(int(np.log10(scale)) + 20)
    mats = []
    for (m, n, rank) in [(256, 128, 128), (256, 128, 40), (200, 100, 100), (130, 70, 7), (256, 2, 2)]:
        dec = np.exp(-np.arange(rank) * (8.0 / max(rank, 1)))
        q1, _ = np.linalg.qr(rnd(rng, (m, rank), np.complex128)); q2, _ = np.linalg.qr(rnd(rng, (n, rank), np.complex128))
        mats.append((q1 * dec) @ q2.conj().T * scale)
    zc = rnd(rng, (256, 96), np.complex128) * scale; zc[:, [0, 17, 50, 95]] = 0
    mats += [np.zeros((256, 128)), zc]
    # more than 256 rows: where svd_batch sends a ComplexF32 260 x 12 theta (the LDS kernels stop at 256 rows); the polishing launch is jacobi_kernel<float, 8> then
    q1, _ = np.linalg.qr(rnd(rng, (260, 12), np.complex128)); q2, _ = np.linalg.qr(rnd(rng, (12, 12), np.complex128))
    mats.append((q1 * np.exp(-np.arange(12) * (8.0 / 12))) @ q2.conj().T * scale)
    outs, fail, pol, sw = tall_svd(mats)
    assert list(fail) == [0, 0, 0, 0, 0, 1, 0, 0]
    assert list(pol) == [0, 0, 0, 0, 0, 1, 0, 0]
    assert np.all(sw >= 0) and np.all(sw < 60)
    for a, A in zip(mats, outs):
        check_tall(a, A)


def test_svd_tall_route_odd_sizes():
    """the tall route where m n is odd (d = 3 sites with unequal odd ranks give such thetas, 165 x 123 for one): A J comes back through copy_items, which moves 16-byte
    words, i.e. PAIRS of ComplexF32 elements -- the last element of an odd count has to be moved on its own.  One launch with an even control.  The inputs are dense
    and generic (no column of A is a singular direction), so the last element of U Sigma = A J mixes a whole row of A: it is the input's last element only if it was
    left behind.  A left-behind element also breaks the bounds of check_tall by three orders of magnitude (one entry of relative size 1 / sqrt(m n) against 4.5e-6)"""
    rng = np.random.default_rng(77)
    mats = []
    for (m, n) in [(261, 13), (165, 123), (257, 3), (511, 127), (260, 12)]:
        q1, _ = np.linalg.qr(rnd(rng, (m, n), np.complex128)); q2, _ = np.linalg.qr(rnd(rng, (n, n), np.complex128))
        mats.append(((q1 * np.exp(-np.arange(n) * (4.0 / n))) @ q2.conj().T).astype(np.complex64).astype(np.complex128))
    outs, fail, pol, sw = tall_svd(mats)
    assert not fail.any() and not pol.any() and np.all(sw >= 0) and np.all(sw < 60)
    for a, A in zip(mats, outs):
        assert np.linalg.matrix_rank(a) == a.shape[1]
        assert A[-1, -1] != a[-1, -1], a.shape          # the last element was written
        check_tall(a, A)


def test_f32_matrix_core_leg():
    """the f32 matrix-instruction variants that only run under TNQS_NO_BF16X3=1 (mfma_rowgemm_kernel<2,2,1>, <2,2,2>, mfma_gram64_kernel): the library reads
    the switch once per process, so the rowgemm and Gram tests above run again in a child process with the switch set, asserting that route"""
    if NO_X3:
        pytest.skip("this is the child")
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-s", "-m", "gpu", os.path.abspath(__file__), "-k", "rowgemm or gram_mfma64", "-p", "no:cacheprovider"],
                       env=dict(os.environ, TNQS_NO_BF16X3="1", PYTHONPATH=os.pathsep.join(sys.path)), capture_output=True, text=True, timeout=600)
    print("\n".join(l[l.index("MEASURED"):] for l in r.stdout.splitlines() if "MEASURED" in l))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert " passed" in r.stdout and " failed" not in r.stdout


@pytest.mark.parametrize("D,PA,K,PB,No", [(2, 1, 32, 64, 32), (2, 8, 32, 16, 32), (1, 16, 64, 8, 64), (1, 4, 64, 32, 40), (2, 2, 32, 48, 9),
                                          (2, 64, 64, 8, 64), (1, 128, 64, 16, 64), (1, 64, 32, 64, 32), (2, 32, 32, 32, 32), (2, 128, 32, 4, 17)])
def test_rowgemm_on_the_fiber_gemm_shapes(D, PA, K, PB, No):
    """the register-direct kernels on the shapes test_fiber_gemm gives mfma_fiber_gemm_w_kernel that they cover, the rows_b ones (PA < 32) first"""
    res, route = rowgemm(D, K, [(PA, PB, No)], seed=PA + PB)
    assert route == rowgemm_route(D, K)
    (out, ref, n2), = res
    err = np.max(np.abs(out - ref)) / np.max(np.abs(ref))
    _measured(f"rowgemm route {route} fiber-gemm shape {(D, PA, K, PB, No)}", err)
    assert err < rowgemm_tol(D, K)
    assert abs(n2 - np.sum(np.abs(ref) ** 2)) < ROWGEMM_NORM_TOL * np.sum(np.abs(ref) ** 2)
