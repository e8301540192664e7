"""Which Gram kernel a batch launches (no GPU): the one route rule of the engine (csrc/kernels.hip gram_route -- run_grams, tnqs_dbg_gram and tnqs_dbg_gram_c128 ask it)
read through the host-only entry point tnqs_dbg_gram_route against a restatement written here from its description ("Gram routes"), tabulated over both element
types, both accumulator types, M on and off, `same` on and off, covered on and off, each switch off and the boundaries of KKmax.  Only values go in."""
import ctypes as C
import itertools

import pytest

import tnqs_amd as tn

GENERIC, MFMA32, MFMA64, FUSED32, F64X64, F64X128, F64IN, GAUGE64, GAUGE32 = range(9)      # the order of GramRoute (csrc/kernels.hpp)
C64, C128 = 0, 1
KKMAX = (1, 3, 4, 7, 8, 15, 16, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 256)


def gram_route(dtype, acc64, has_m, all_same, all_f64in, kkmax, use_mfma=1, use_chi64=1):
    lib = C.CDLL(tn.LIB_PATH)
    fn = lib.tnqs_dbg_gram_route
    fn.argtypes = [C.c_int] * 8 + [C.POINTER(C.c_int)]
    r = C.c_int(-1)
    assert fn(dtype, acc64, has_m, all_same, all_f64in, kkmax, use_mfma, use_chi64, C.byref(r)) == 0
    return r.value


def expected(dtype, acc64, has_m, all_same, all_f64in, kkmax, use_mfma, use_chi64):
    """a table, not a chain of else-ifs: each route with the whole condition it is taken under; exactly one holds"""
    f32 = dtype == C64
    gate_path = f32 and acc64                      # f32 data, f64 accumulation
    hit = {
        GAUGE32: has_m and gate_path and kkmax == 32,
        GAUGE64: has_m and gate_path and kkmax != 32,
        FUSED32: has_m and not gate_path,
        F64X64: not has_m and gate_path and use_mfma and all_same and 16 <= kkmax <= 64,
        F64X128: not has_m and gate_path and use_mfma and use_chi64 and all_same and 64 < kkmax <= 128,
        F64IN: not has_m and not f32 and use_mfma and all_f64in,
        MFMA32: not has_m and f32 and not acc64 and use_mfma and 8 <= kkmax <= 32,
        MFMA64: not has_m and f32 and not acc64 and use_mfma and use_chi64 and 32 < kkmax <= 64,
    }
    taken = [r for r, h in hit.items() if h]
    assert len(taken) <= 1
    return taken[0] if taken else GENERIC


def test_route_table():
    n = 0
    for dtype, acc64, has_m, same, cov, mf, c64 in itertools.product((C64, C128), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1)):
        if dtype == C128 and not acc64:
            continue                               # ComplexF64 is accumulated in double: run_grams<double, float> does not exist
        for kk in KKMAX:
            assert gram_route(dtype, acc64, has_m, same, cov, kk, mf, c64) == expected(dtype, acc64, has_m, same, cov, kk, mf, c64), (dtype, acc64, has_m, same, cov, kk, mf, c64)
            n += 1
    assert n == 3 * 32 * len(KKMAX)


@pytest.mark.parametrize("kk,route", [(3, GENERIC), (4, F64IN), (15, F64IN), (16, F64IN), (32, F64IN), (33, F64IN), (64, F64IN), (65, GENERIC), (128, GENERIC), (129, GENERIC)])
def test_complex128_boundaries(kk, route):
    """ComplexF64 operands: covered (every item 4 <= D K <= 64, no M) is what decides, with and without `same`; each switch off"""
    covered = int(4 <= kk <= 64)
    for same in (0, 1):
        assert gram_route(C128, 1, 0, same, covered, kk) == route
        assert gram_route(C128, 1, 0, same, covered, kk, use_mfma=0) == GENERIC
        assert gram_route(C128, 1, 0, same, covered, kk, use_chi64=0) == route
    assert gram_route(C128, 1, 0, 1, 0, 16) == GENERIC          # one item of the batch outside the kernel sends the whole batch to the vector kernel


@pytest.mark.parametrize("kk,acc32,acc64_same,acc64_other", [(3, GENERIC, GENERIC, GENERIC), (4, GENERIC, GENERIC, GENERIC), (15, MFMA32, GENERIC, GENERIC), (16, MFMA32, F64X64, GENERIC),
                                                             (32, MFMA32, F64X64, GENERIC), (33, MFMA64, F64X64, GENERIC), (64, MFMA64, F64X64, GENERIC),
                                                             (65, GENERIC, F64X128, GENERIC), (128, GENERIC, F64X128, GENERIC), (129, GENERIC, GENERIC, GENERIC)])
def test_complex64_boundaries(kk, acc32, acc64_same, acc64_other):
    for same in (0, 1):
        assert gram_route(C64, 0, 0, same, 0, kk) == acc32
        assert gram_route(C64, 0, 0, same, 0, kk, use_mfma=0) == GENERIC
        assert gram_route(C64, 0, 0, same, 0, kk, use_chi64=0) == (acc32 if acc32 != MFMA64 else GENERIC)
    assert gram_route(C64, 1, 0, 1, 0, kk) == acc64_same and gram_route(C64, 1, 0, 0, 0, kk) == acc64_other
    assert gram_route(C64, 1, 0, 1, 0, kk, use_chi64=0) == (acc64_same if acc64_same != F64X128 else GENERIC)
    assert gram_route(C64, 1, 0, 1, 0, kk, use_mfma=0) == GENERIC
    # M set: the switches and `same` do not matter
    for mf, c64, same in itertools.product((0, 1), (0, 1), (0, 1)):
        assert gram_route(C64, 0, 1, same, 0, kk, mf, c64) == FUSED32
        assert gram_route(C64, 1, 1, same, 0, kk, mf, c64) == (GAUGE32 if kk == 32 else GAUGE64)
