"""CPU: the LifeStable lookahead entry points (strip passes, TestUnknowns,
PropagateAndTest) are exported and bound, and they validate their arguments
before touching any device (no compute calls here: every call below either
fails validation or has n == 0)."""
import ctypes
import os

import numpy as np
import pytest

BASES = ("lifeapi_stable_strip_pass_batch", "lifeapi_stable_test_unknowns_batch",
         "lifeapi_stable_propagate_and_test_batch")
NAMES = [base + tail for base in BASES for tail in ("_dev", "")]
# made-up, aligned, far apart: validation never reads through them
A, B, D = 1 << 20, 1 << 24, 1 << 28
N = 4


@pytest.fixture(scope="module")
def hip():
    import lifeapi_amd.hip as h
    return h


def err(hip):
    return hip.lib.lifeapi_last_error()


def test_symbols_exported_and_bound(hip):
    lib = ctypes.CDLL(hip.LIB_PATH)
    assert len(NAMES) == 6
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in hip.EXPORTS and getattr(hip.lib, name).restype is ctypes.c_int, name
    assert hip.abi_version() == 2
    for fn in ("stable_strip_pass", "stable_test_unknowns", "stable_propagate_and_test"):
        assert callable(getattr(hip, fn)) and callable(getattr(hip, fn + "_host")), fn


def test_header_declares_and_cites(hip):
    text = open(os.path.join(os.path.dirname(os.path.dirname(hip.LIB_PATH)), "include", "lifeapi_hip.h")).read()
    for name in NAMES:
        assert f"int {name}(" in text, name
    for cite in ("LifeStable.hpp:921-948, 995-1249", "LifeStable.hpp:1321-1338", "LifeStable.hpp:1251-1284",
                 "LifeStable.hpp:217-233", "LifeStable.hpp:163-184"):
        assert cite in text.split("#ifndef LIFEAPI_HIP_H")[0], cite
    body = text.split("#ifndef LIFEAPI_HIP_H")[1]
    for cite in ("LifeStable.hpp:921-948", ":1111-1195", ":995-1109", ":1215-1236", ":1238-1249", ":1197-1213",
                 "LifeStable.hpp:1321-1338", ":1251-1284", ":217-233", "LifeStable.hpp:163-184"):
        assert cite in body, cite


@pytest.mark.parametrize("dev", [True, False])
def test_strip_pass_validation(hip, dev):
    f = getattr(hip.lib, BASES[0] + ("_dev" if dev else ""))
    last = None if dev else 0
    for pass_ in range(6):
        assert f(None, None, None, 0, pass_, 0, last) == 0
    # the pass is checked first, n == 0 included
    for n in (0, N):
        for pass_ in (-1, 6):
            assert f(A, B, D, n, pass_, 0, last) == -1 and b"pass" in err(hip), (n, pass_)
    for args in ((None, B, D), (A, None, D), (A, B, None)):
        assert f(*args, N, 4, 0, last) == -1 and b"null" in err(hip), args
    assert f(A + 4, B, D, N, 4, 0, last) == -1 and b"misaligned" in err(hip)
    assert f(A, B + 1, D + 3, 0, 4, 0, last) == 0           # columns and flags are bytes
    # the columns over the planes' first and last byte, the flags over the planes
    for args in ((A, A, D), (A, A + 5120 * N - 1, D), (A, A - N + 1, D), (A, B, A + 5120)):
        assert f(*args, N, 4, 0, last) == -1 and b"overlap" in err(hip), args


@pytest.mark.parametrize("dev", [True, False])
def test_test_unknowns_validation(hip, dev):
    f = getattr(hip.lib, BASES[1] + ("_dev" if dev else ""))
    last = None if dev else 0
    assert f(None, None, 0, None, 0, 0, last) == 0 and f(None, None, 1, None, 0, 7, last) == 0
    for args in ((None, B, 0, D), (A, None, 0, D), (A, B, 1, None)):
        assert f(*args, N, 0, last) == -1 and b"null" in err(hip), args
    for args in ((A + 4, B, 0, D), (A, B + 4, 0, D), (A, B + 2, 1, D)):
        assert f(*args, N, 0, last) == -1 and b"misaligned" in err(hip), args
    # the one mask over the planes' end, N masks over their start, the mask inside, the flags over the planes
    for args in ((A, A + 5120 * N - 8, 0, D), (A, A - 512 * N + 8, 1, D), (A, A + 1024, 0, D), (A, B, 0, A + 7)):
        assert f(*args, N, 0, last) == -1 and b"overlap" in err(hip), args


@pytest.mark.parametrize("dev", [True, False])
def test_propagate_and_test_validation(hip, dev):
    f = getattr(hip.lib, BASES[2] + ("_dev" if dev else ""))
    last = None if dev else 0
    assert f(None, None, 0, 0, last) == 0 and f(None, None, 0, 1, last) == 0
    for args in ((None, D), (A, None)):
        assert f(*args, N, 0, last) == -1 and b"null" in err(hip), args
    assert f(A + 4, D, N, 0, last) == -1 and b"misaligned" in err(hip)
    for args in ((A, A), (A, A + 5120 * N - 1), (A, A - N + 1)):
        assert f(*args, N, 0, last) == -1 and b"overlap" in err(hip), args


def test_python_wrappers_reject_bad_shapes(hip):
    s = np.zeros((3, 640), np.uint64)
    with pytest.raises(ValueError):
        hip.stable_strip_pass_host(np.zeros(3 * 64, np.uint64), np.zeros(1, np.uint8), 4)
    with pytest.raises(ValueError):
        hip.stable_strip_pass_host(s, np.zeros(2, np.uint8), 4)
    with pytest.raises(ValueError):
        hip.stable_strip_pass_host(s, np.zeros(3, np.uint8), 6)
    with pytest.raises(ValueError):
        hip.stable_strip_pass_host(s, np.zeros(3, np.uint8), "propagate")
    with pytest.raises(ValueError):
        hip.stable_test_unknowns_host(s, np.zeros((2, 64), np.uint64))
    with pytest.raises(ValueError):
        hip.stable_test_unknowns_host(np.zeros(650, np.uint64), np.zeros(64, np.uint64))
    with pytest.raises(ValueError):
        hip.stable_propagate_and_test_host(np.zeros(641, np.uint64))
    for out, fl in (hip.stable_strip_pass_host(s[:0], np.zeros(0, np.uint8), "propagate_strip"),
                    hip.stable_test_unknowns_host(s[:0], np.zeros(64, np.uint64)),
                    hip.stable_propagate_and_test_host(s[:0])):
        assert out.shape == (0, 640) and fl.shape == (0,)
