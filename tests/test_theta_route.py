"""Which theta route a two-site gate is offered and what it is given to work in (no GPU): the host rule of the gate path (csrc/gate_theta.cpp theta_route) read through the
host-only mode of tnqs_dbg_gate_theta (include/tnqs_debug.h: info == NULL fills low_sizes_out and returns) against a restatement of the rule written here from its description
in DESIGN.md 4.7 and next to the kernels.  Only shapes, gates and caps go in.

With Mr = d1^2 chi, Nc = d2^2 chi, kappa = the gate's operator-Schmidt rank, K = kappa chi and cap = min(Mr, Nc, maxdim if > 0):
  * operator-sum factors (lowA: Mr K, lowB: Nc K) whenever the low-rank switch is on;
  * the low-rank route (lowG, lowL: K K; ComplexF64: L2 and Lc, 2 K K) iff K < Nc, K <= 128, cap <= K, Mr >= Nc and -- ComplexF64 -- the Mr x K factor fits the LDS-resident Jacobi;
  * the preconditioned route (lowQ: Nc K) iff the low-rank route, ComplexF32, theta_svd_pre_covers(Mr, K) and K <= 96;
  * max(d1, d2)^2 chi > 512: TNQS_ERR_UNSUPPORTED, nothing written.
The ComplexF64 LDS term needs no device: jacobi_lds() compares jacobi_lds_bytes() with a constant (160 KiB - 2 KiB) unless TNQS_JACOBI_GLOBAL=1 sends every Jacobi to the
global-memory kernel, so every ComplexF64 case is decided here as well; the two environment switches the rule reads are read here too."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import tnqs_amd as tn

lib = C.CDLL(tn.LIB_PATH)
lib.tnqs_last_error.restype = C.c_char_p
ERR_UNSUPPORTED = -2                                     # include/tnqs.h
C64, C128 = 0, 1
DIMS = [(2, 2), (2, 3), (3, 2)]
CHIS = [1, 3, 8, 16, 24, 32, 33, 48, 64, 128]


def _on(name):
    return os.environ.get(name, "")[:1] == "1"


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- gates of a given operator-Schmidt rank ---------------------------------------------------------------------------------------------------------------
def _unitary(rng, n):
    q, r = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    return q * (np.diag(r) / np.abs(np.diag(r)))


def gate_of(name, d1, d2, rng):
    """g[(s1' s2'), (s1 s2)], first vertex most significant"""
    if name == "product":
        return np.kron(_unitary(rng, d1), _unitary(rng, d2))
    if name == "Rzz":
        z = lambda d: np.linspace(1.0, -1.0, d)
        return np.diag(np.exp(-0.5j * 0.37 * np.kron(z(d1), z(d2))))
    if name == "CNOT":
        return np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0]], dtype=complex)
    if name == "SWAP":
        return np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], dtype=complex)
    assert name == "random"
    return _unitary(rng, d1 * d2)


GATES = {"product": 1, "Rzz": 2, "CNOT": 2, "SWAP": 4, "random": 4}      # name -> operator-Schmidt rank


def schmidt_rank(g, d1, d2):
    O = np.asarray(g).reshape(d1, d2, d1, d2).transpose(0, 2, 1, 3).reshape(d1 * d1, d2 * d2)
    s = np.linalg.svd(O, compute_uv=False)
    return int(np.sum(s > 1e-10 * s[0]))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------------------
def refused(d1, d2, chi):
    return d1 * d1 * chi > 512 or d2 * d2 * chi > 512


def expected_sizes(f32, d1, d2, chi, kappa, maxdim, lowrank_on):
    Mr, Nc, K = d1 * d1 * chi, d2 * d2 * chi, kappa * chi
    cap = min(Mr, Nc, maxdim) if maxdim > 0 else min(Mr, Nc)
    if not lowrank_on or kappa == 0:
        return [0] * 6
    esz = 8 if f32 else 16
    lds_fits = f32 or (not _on("TNQS_JACOBI_GLOBAL") and (Mr + 2) * K * esz <= 160 * 1024 - 2048)
    low = K < Nc and K <= 128 and cap <= K and Mr >= Nc and lds_fits
    pre_covers = 2 <= K <= 64 and K <= Mr <= 128
    lowq = low and f32 and not _on("TNQS_NO_PRECOND_SVD") and pre_covers and K <= 96
    return [Mr * K, Nc * K, K * K if low else 0, K * K if low else 0, Nc * K if lowq else 0, 2 * K * K if (low and not f32) else 0]


# ---- the host-only call --------------------------------------------------------------------------------------------------------------------------------------
def low_sizes(dtype, items, lowrank_on):
    """items: (d1, d2, chi, gate, maxdim).  Returns (status, sizes[n][6]); sizes start at -1"""
    n = len(items)
    dims = np.ascontiguousarray(np.array([it[:3] for it in items], dtype=np.int32).ravel())
    mode = np.zeros(2 * n, dtype=np.int32); rk = np.zeros(2 * n, dtype=np.int32); tau = np.zeros(2 * n, dtype=np.float64)
    md = np.ascontiguousarray(np.array([it[4] for it in items], dtype=np.int32))
    g = np.ascontiguousarray(np.concatenate([np.asarray(it[3], dtype=np.complex128).ravel(order="F") for it in items]))
    F = np.zeros(1, dtype=np.complex128)                  # the site factors are not read by the host-only mode: only non-null
    sizes = np.full(6 * n, -1, dtype=np.int32)
    rc = lib.tnqs_dbg_gate_theta(dtype, n, _p(dims), _p(mode), _p(rk), _p(F), _p(F), _p(tau), _p(g), _p(md), int(lowrank_on), 0, _p(sizes), *([None] * 16), 3)
    return rc, sizes.reshape(n, 6)


def check(dtype, items, lowrank_on=1):
    """accepted items in one call, every refused item in a call of its own"""
    ok = [it for it in items if not refused(*it[:3])]
    if ok:
        rc, got = low_sizes(dtype, ok, lowrank_on)
        assert rc == 0, (rc, lib.tnqs_last_error())
        for it, z in zip(ok, got):
            d1, d2, chi, g, md = it
            want = expected_sizes(dtype == C64, d1, d2, chi, schmidt_rank(g, d1, d2), md, lowrank_on)
            assert list(z) == want, (dtype, d1, d2, chi, schmidt_rank(g, d1, d2), md, lowrank_on, list(z), want)
    for it in items:
        if refused(*it[:3]):
            rc, got = low_sizes(dtype, [it], lowrank_on)
            assert rc == ERR_UNSUPPORTED, (rc, it[:3])
            assert b"d^2*chi > 512" in lib.tnqs_last_error()
            assert np.all(got == -1), "a refused call wrote to low_sizes_out"
    return len(ok)


def maxdims(K):
    return sorted({0, max(K - 1, 0), K, K + 1})


@pytest.fixture(scope="module")
def gates():
    rng = np.random.default_rng(20240611)
    out = {}
    for (d1, d2) in DIMS:
        for name, rank in GATES.items():
            if name in ("CNOT", "SWAP") and (d1, d2) != (2, 2):
                continue
            g = gate_of(name, d1, d2, rng)
            assert schmidt_rank(g, d1, d2) == rank, (name, d1, d2)
            out[(name, d1, d2)] = g
    return out


@pytest.mark.parametrize("dtype", [C64, C128], ids=["c64", "c128"])
@pytest.mark.parametrize("d1,d2", DIMS, ids=["2x2", "2x3", "3x2"])
def test_low_sizes_follow_the_rule(gates, dtype, d1, d2):
    items = []
    for (name, a, b), g in gates.items():
        if (a, b) != (d1, d2):
            continue
        for chi in CHIS:
            for md in maxdims(GATES[name] * chi):
                items.append((d1, d2, chi, g, md))
    nok = check(dtype, items)
    assert nok >= len(items) // 2                         # most of the grid is inside the refusal limit
    # every branch of the rule is taken somewhere in the grid of this parameter set (d1 < d2 never offers the low-rank route: Mr < Nc)
    f32 = dtype == C64
    rows = [expected_sizes(f32, *it[:3], schmidt_rank(it[3], d1, d2), it[4], 1) for it in items if not refused(*it[:3])]
    assert any(r[2] == 0 for r in rows)
    if d1 >= d2:
        assert any(r[2] > 0 for r in rows)
        assert any(r[4] > 0 for r in rows) == (f32 and not _on("TNQS_NO_PRECOND_SVD"))
        assert any(r[5] > 0 for r in rows) == (not f32 and not _on("TNQS_JACOBI_GLOBAL"))


@pytest.mark.parametrize("dtype", [C64, C128], ids=["c64", "c128"])
def test_boundaries_of_K(gates, dtype):
    """K = 96 / 98 (Rzz at chi = 48 / 49: the K <= 96 term of the preconditioned route) and K = 128 / 130 (chi = 64 / 65: the K <= 128 term of the low-rank route), and
    the same K reached with a rank-4 gate, each with the four caps around K"""
    rzz, swap = gates[("Rzz", 2, 2)], gates[("SWAP", 2, 2)]
    items = [(2, 2, chi, rzz, md) for chi in (48, 49, 64, 65) for md in maxdims(2 * chi)]
    items += [(2, 2, chi, swap, md) for chi in (24, 25, 32, 33) for md in maxdims(4 * chi)]
    assert check(dtype, items) == len(items)
    f32 = dtype == C64
    assert expected_sizes(f32, 2, 2, 64, 2, 128, 1)[2] == (128 * 128 if f32 else 0)      # K = 128: offered (ComplexF64: the 256 x 128 factor is beyond the LDS)
    assert expected_sizes(f32, 2, 2, 65, 2, 130, 1)[2] == 0                              # K = 130: not offered
    assert expected_sizes(f32, 2, 2, 32, 2, 64, 1)[4] == (128 * 64 if f32 and not _on("TNQS_NO_PRECOND_SVD") else 0)
    assert expected_sizes(f32, 2, 2, 48, 2, 96, 1)[4] == 0                               # K = 96 passes K <= 96, but theta_svd_pre_covers stops at 64 columns


@pytest.mark.parametrize("dtype", [C64, C128], ids=["c64", "c128"])
def test_lowrank_switch_off(gates, dtype):
    items = [(d1, d2, chi, g, md) for (name, d1, d2), g in gates.items() for chi in (3, 32) for md in (0, 2 * chi)]
    assert check(dtype, items, lowrank_on=0) == len(items)
    rc, got = low_sizes(dtype, items, 0)
    assert rc == 0 and np.all(got == 0)


@pytest.mark.parametrize("dtype", [C64, C128], ids=["c64", "c128"])
def test_refusal_limit(gates, dtype):
    """d^2 chi = 512 is accepted, 516 refused, on either side of the gate"""
    for (d1, d2, chi, ok) in [(2, 2, 128, True), (2, 2, 129, False), (2, 3, 56, True), (2, 3, 57, False), (3, 2, 57, False), (3, 2, 56, True)]:
        for name in ("product", "Rzz", "random"):
            for md, on in itertools.product((0, 7), (0, 1)):
                assert check(dtype, [(d1, d2, chi, gates[(name, d1, d2)], md)], lowrank_on=on) == (1 if ok else 0)
