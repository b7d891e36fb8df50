"""CPU: the entry points with both operands or an offset per universe, and Halve
/ Skew, are exported and bound, and they validate their arguments before
touching any device (no compute calls here: every call below either fails
validation or has n == 0)."""
import ctypes
import os
import re

import numpy as np
import pytest

import test_pair_model as P

BASES = ("lifeapi_convolve_pair_batch", "lifeapi_intersecting_offsets_batch", "lifeapi_transform_offsets_batch",
         "lifeapi_symmetricize_offsets_batch", "lifeapi_halve_batch", "lifeapi_skew_batch")
NAMES = [base + tail for base in BASES for tail in ("_dev", "")]
# made-up, aligned, far apart: validation never reads through them
A, B, D, E = 1 << 20, 1 << 24, 1 << 28, 1 << 30
N = 4
SYMMETRICIZE_DEFINED = (0, 1, 3, 5, 6, 7, 11, 13, 17)


@pytest.fixture(scope="module")
def hip():
    import lifeapi_amd.hip as h
    return h


def err(hip):
    return hip.lib.lifeapi_last_error()


def test_symbols_exported_and_bound(hip):
    lib = ctypes.CDLL(hip.LIB_PATH)
    assert len(NAMES) == 12
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in hip.EXPORTS and getattr(hip.lib, name).restype is ctypes.c_int, name
    assert hip.abi_version() == 2
    for fn in ("convolve_pair", "intersecting_offsets", "transform_offsets", "symmetricize_offsets", "halve", "skew"):
        assert callable(getattr(hip, fn)) and callable(getattr(hip, fn + "_host")), fn
    assert {hip.SYMMETRIES[v]: hip.TRANSFORMS[P.M.T[t]] for v, t in
            ((P.IO_VALUES[s], P.IO_TRANSFORM[s]) for s in P.IO_SYMS)} == hip.INTERSECTING_TRANSFORMS
    assert hip.HALVE_MODES == P.HALVE_MODES


def test_header_declares_what_is_bound(hip):
    """each new entry point is declared once, with as many parameters and the
    same integer / pointer kinds as hip.py binds, and the header cites the
    reference's lines"""
    text = open(os.path.join(os.path.dirname(os.path.dirname(hip.LIB_PATH)), "include", "lifeapi_hip.h")).read()
    kinds = {ctypes.c_void_p: "pointer", ctypes.c_size_t: "size_t", ctypes.c_uint32: "uint32_t", ctypes.c_int: "int"}
    for name in NAMES:
        found = re.findall(r"\bint %s\(([^)]*)\);" % name, text)
        assert len(found) == 1, name
        params = [" ".join(p.split()) for p in found[0].split(",")]
        declared = ["pointer" if "*" in p else p.rsplit(" ", 1)[0] for p in params]
        assert declared == [kinds[a] for a in getattr(hip.lib, name).argtypes], (name, declared)
    for cite in ("Symmetry.hpp:729-768", "Symmetry.hpp:770-772", "Symmetry.hpp:681-709", "Symmetry.hpp:711-718",
                 "Symmetry.hpp:720-727", "Symmetry.hpp:540-563", "LifeAPI.hpp:1293-1370"):
        assert cite in text, cite
    assert "#define LIFEAPI_ABI_VERSION 2" in text


@pytest.mark.parametrize("dev", [True, False])
@pytest.mark.parametrize("base,codes,bad", [(BASES[0], range(16), (16, 2 ** 32 - 1)),
                                            (BASES[1], tuple(P.IO_VALUES.values()), P.IO_UNDEFINED + (2 ** 32 - 1,))])
def test_pair_validation(hip, dev, base, codes, bad):
    f = getattr(hip.lib, base + ("_dev" if dev else ""))
    last = None if dev else 0
    for code in codes:
        assert f(None, None, code, None, 0, last) == 0 and f(A + 1, B + 3, code, 5, 0, last) == 0, code   # n == 0
    for code in bad:    # checked first, n == 0 included
        for n in (0, N):
            assert f(A, B, code, D, n, last) == -1, (code, n)
            assert b"transform" in err(hip) or b"undefined" in err(hip)
    code = codes[1]
    for args in ((None, B, code, D), (A, None, code, D), (A, B, code, None)):
        assert f(*args, N, last) == -1 and b"null" in err(hip), args
    for args in ((A + 4, B, code, D), (A, B + 2, code, D), (A, B, code, D + 1)):
        assert f(*args, N, last) == -1 and b"aligned" in err(hip), args
    # the output over part of an operand (either, both ways), the operands over each other
    for args in ((A, B, code, A + 512), (A, B, code, B - 512 * N + 8), (A, B, code, B + 512 * N - 8),
                 (A, A + 512, code, D), (B + 8, B, code, D), (A, A + 512 * N - 8, code, A)):
        assert f(*args, N, last) == -1 and b"overlap" in err(hip), args
    # (what is allowed -- b == a, out == a, out == b -- launches: tests/test_gpu_pair.py)


@pytest.mark.parametrize("dev", [True, False])
@pytest.mark.parametrize("base,codes,bad", [(BASES[2], range(16), (16, 2 ** 32 - 1)),
                                            (BASES[3], SYMMETRICIZE_DEFINED, P.M.UNDEFINED_SYMMETRIES + (2 ** 32 - 1,))])
def test_offsets_validation(hip, dev, base, codes, bad):
    f = getattr(hip.lib, base + ("_dev" if dev else ""))
    last = None if dev else 0
    for code in codes:
        assert f(None, None, 0, code, None, last) == 0 and f(A + 1, B + 3, 0, code, 7, last) == 0, code     # n == 0
    for code in bad:
        for n in (0, N):
            assert f(A, B, n, code, D, last) == -1, (code, n)
            assert b"transform" in err(hip) or b"undefined" in err(hip)
    code = codes[1]
    for args in ((None, B, N, code, D), (A, None, N, code, D), (A, B, N, code, None)):
        assert f(*args, last) == -1 and b"null" in err(hip), args
    for args in ((A + 4, B, N, code, D), (A, B + 2, N, code, D), (A, B, N, code, D + 2)):
        assert f(*args, last) == -1 and b"aligned" in err(hip), args
    # the output over part of the input; the offsets over the output's first and last bytes (in place too)
    for args in ((A, A + 512, N, code, D), (A, B, N, code, B), (A, B, N, code, B + 512 * N - 4),
                 (A, B, N, code, B - 8 * N + 4), (A, A, N, code, A + 1024)):
        assert f(*args, last) == -1 and b"overlap" in err(hip), args
    # (offsets just clear of the output, and over the INPUT of an out-of-place call, are no error by
    # validation: such calls launch, tests/test_gpu_pair.py)


@pytest.mark.parametrize("dev", [True, False])
def test_halve_and_skew_validation(hip, dev):
    halve, skew = (getattr(hip.lib, b + ("_dev" if dev else "")) for b in BASES[4:])
    last = None if dev else 0
    for mode in range(3):
        assert halve(None, None, 0, mode, last) == 0 and halve(A + 1, 3, 0, mode, last) == 0
    for inverse in (0, 1, -5):
        assert skew(None, None, 0, inverse, last) == 0 and skew(A + 1, 3, 0, inverse, last) == 0
    for mode in (3, 2 ** 32 - 1):
        for n in (0, N):
            assert halve(A, B, n, mode, last) == -1 and b"mode" in err(hip), (mode, n)
    for f, arg in ((halve, 0), (halve, 2), (skew, 0), (skew, 1)):
        for args in ((None, B), (A, None)):
            assert f(*args, N, arg, last) == -1 and b"null" in err(hip), args
        for args in ((A + 4, B), (A, B + 1)):
            assert f(*args, N, arg, last) == -1 and b"aligned" in err(hip), args
        for args in ((A, A + 512), (A + 512 * N - 8, A)):
            assert f(*args, N, arg, last) == -1 and b"overlap" in err(hip), args


def test_python_wrappers_reject_bad_shapes(hip):
    two, three = np.zeros((2, 64), np.uint64), np.zeros((3, 64), np.uint64)
    with pytest.raises(ValueError):
        hip.convolve_pair_host(two, three)
    with pytest.raises(ValueError):
        hip.intersecting_offsets_host(two, "C2", three)
    with pytest.raises(ValueError):
        hip.transform_offsets_host(two, 0, np.zeros((3, 2), np.int32))
    with pytest.raises(ValueError):
        hip.symmetricize_offsets_host(two, "C4", np.zeros(3, np.int32))
    with pytest.raises(ValueError):
        hip.halve_host(two, "HalveZ")
    with pytest.raises(ValueError):
        hip.halve_host(np.zeros(65, np.uint64))
    empty = np.zeros((0, 64), np.uint64)
    assert hip.convolve_pair_host(empty).shape == (0, 64) and hip.skew_host(empty, True).shape == (0, 64)
    assert hip.intersecting_offsets_host(empty, "D2diagodd").shape == (0, 64)
    assert hip.symmetricize_offsets_host(empty, "D4diag", np.zeros((0, 2), np.int32)).shape == (0, 64)
    with pytest.raises(hip.LifeApiError):
        hip.intersecting_offsets_host(empty, "D4")
