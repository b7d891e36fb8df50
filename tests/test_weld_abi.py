"""CPU: the LifeWeld construction entry points are exported and bound, and they
validate their arguments before touching any device (no compute calls here:
every call below either fails validation or has n == 0)."""
import ctypes

import numpy as np
import pytest

BASES = ("lifeapi_weld_from_required_batch", "lifeapi_weld_to_target_batch", "lifeapi_weld_to_stable_batch",
         "lifeapi_weld_interaction_offsets_batch")
NAMES = [base + tail for base in BASES for tail in ("_dev", "")]
# made-up, aligned, far apart: validation never reads through them
A, B, D, E = 1 << 20, 1 << 24, 1 << 28, 1 << 30
N = 4


@pytest.fixture(scope="module")
def hip():
    import lifeapi_amd.hip as h
    return h


def err(hip):
    return hip.lib.lifeapi_last_error()


def test_symbols_exported_and_bound(hip):
    lib = ctypes.CDLL(hip.LIB_PATH)
    assert len(NAMES) == 8
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in hip.EXPORTS and getattr(hip.lib, name).restype is ctypes.c_int, name
    assert hip.abi_version() == 2
    for fn in ("weld_from_required", "weld_to_target", "weld_to_stable", "weld_interaction_offsets"):
        assert callable(getattr(hip, fn)) and callable(getattr(hip, fn + "_host")), fn


def test_header_declares_and_cites(hip):
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(hip.LIB_PATH)), "include", "lifeapi_hip.h")).read()
    for name in NAMES:
        assert f"int {name}(" in text, name
    for cite in ("LifeWeld.hpp:133-159", "LifeWeld.hpp:188-191", "LifeWeld.hpp:279-325", "LifeWeld.hpp:327-400",
                 "LifeWeld.hpp:206-245"):
        assert cite in text.split("#ifndef LIFEAPI_HIP_H")[0], cite


@pytest.mark.parametrize("dev", [True, False])
def test_from_required_validation(hip, dev):
    f = getattr(hip.lib, BASES[0] + ("_dev" if dev else ""))
    last = None if dev else 0
    assert f(None, None, 0, None, 0, last) == 0 and f(None, None, 1, None, 0, last) == 0
    for args in ((None, B, 0, D), (A, None, 0, D), (A, B, 0, None)):
        assert f(*args, N, last) == -1 and b"null" in err(hip), args
    for args in ((A + 4, B, 0, D), (A, B + 2, 1, D), (A, B, 0, D + 1)):
        assert f(*args, N, last) == -1 and b"misaligned" in err(hip), args
    # the welds over the states, over the one required state, over the last of N required states
    for args in ((A, B, 0, A + 512), (A, D + 2048 * N - 8, 0, D), (A, D - 512 * N + 8, 1, D), (D + 1024, B, 1, D)):
        assert f(*args, N, last) == -1 and b"overlap" in err(hip), args


@pytest.mark.parametrize("dev", [True, False])
def test_to_target_validation(hip, dev):
    f = getattr(hip.lib, BASES[1] + ("_dev" if dev else ""))
    last = None if dev else 0
    assert f(None, None, None, 0, last) == 0
    for args in ((None, B, D), (A, None, D), (A, B, None)):
        assert f(*args, N, last) == -1 and b"null" in err(hip), args
    for args in ((A + 4, B, D), (A, B + 4, D), (A, B, D + 4)):
        assert f(*args, N, last) == -1 and b"misaligned" in err(hip), args
    # wanted over the welds, unwanted over the welds, wanted over unwanted (both ways)
    for args in ((A, A + 2048 * N - 8, D), (A, B, A), (A, B, B + 512), (A, B + 512 * N - 8, B)):
        assert f(*args, N, last) == -1 and b"overlap" in err(hip), args


@pytest.mark.parametrize("dev", [True, False])
def test_to_stable_validation(hip, dev):
    f = getattr(hip.lib, BASES[2] + ("_dev" if dev else ""))
    last = None if dev else 0
    assert f(None, None, 0, None, 0, None, 0, last) == 0 and f(None, None, 1, None, 65536, None, 0, last) == 0
    # the duration is checked first, n == 0 included
    for n in (0, N):
        assert f(A, None, 0, None, 65537, D, n, last) == -1 and b"duration" in err(hip), n
    for args in ((None, None, 0, None, 8, D), (A, None, 0, None, 8, None)):
        assert f(*args, N, last) == -1 and b"null" in err(hip), args
    for args in ((A + 4, None, 0, None, 8, D), (A, B + 4, 0, None, 8, D), (A, B, 1, E + 2, 8, D), (A, None, 0, None, 8, D + 4)):
        assert f(*args, N, last) == -1 and b"misaligned" in err(hip), args
    # the stables over the welds, over the one active state, over N active states, over the mask
    for args in ((A, None, 0, None, 8, A + 2048), (A, D + 5120 * N - 8, 0, None, 8, D), (A, D - 512 * N + 8, 1, None, 8, D),
                 (A, B, 0, D + 512, 0, D)):
        assert f(*args, N, last) == -1 and b"overlap" in err(hip), args


@pytest.mark.parametrize("dev", [True, False])
def test_interaction_offsets_validation(hip, dev):
    f = getattr(hip.lib, BASES[3] + ("_dev" if dev else ""))
    last = None if dev else 0
    assert f(None, None, None, 0, last) == 0
    for args in ((None, B, D), (A, None, D), (A, B, None)):
        assert f(*args, N, last) == -1 and b"null" in err(hip), args
    for args in ((A + 4, B, D), (A, B + 4, D), (A, B, D + 4)):
        assert f(*args, N, last) == -1 and b"misaligned" in err(hip), args
    for args in ((A, B, A + 2048 * N - 8), (A, D + 512 * N - 8, D), (A, D - 2048 + 8, D)):
        assert f(*args, N, last) == -1 and b"overlap" in err(hip), args


def test_python_wrappers_reject_bad_shapes(hip):
    z = np.zeros(64, np.uint64)
    with pytest.raises(ValueError):
        hip.weld_to_target_host(np.zeros(3 * 64, np.uint64))
    with pytest.raises(ValueError):
        hip.weld_from_required_host(np.zeros((3, 64), np.uint64), np.zeros((2, 64), np.uint64))
    with pytest.raises(ValueError):
        hip.weld_to_stable_host(np.zeros((2, 256), np.uint64), mask=np.zeros((2, 64), np.uint64))
    with pytest.raises(ValueError):
        hip.weld_interaction_offsets_host(np.zeros((2, 256), np.uint64), z)
    assert hip.weld_to_target_host(np.zeros((0, 256), np.uint64))[0].shape == (0, 64)
