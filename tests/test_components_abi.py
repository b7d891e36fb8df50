"""CPU: the connected-component entry points are exported and bound, and they
validate their arguments before touching any device (no compute calls here:
every call below either fails validation or has n == 0)."""
import ctypes

import numpy as np
import pytest

import components_cases as C

NAMES = [base + tail for base in ("lifeapi_first_on_batch", "lifeapi_component_containing_batch",
                                  "lifeapi_components_batch") for tail in ("_dev", "")]
A, B, D = 1 << 20, 1 << 24, 1 << 28      # made-up, aligned, far apart: validation never reads through them


@pytest.fixture(scope="module")
def hip():
    import lifeapi_amd.hip as h
    return h


def ptr(a):
    return a.ctypes.data


def test_symbols_exported_and_bound(hip):
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in hip.EXPORTS and getattr(hip.lib, name).restype is ctypes.c_int, name
    assert hip.abi_version() == 2
    for fn in ("first_on", "component_containing", "components", "first_on_host", "component_containing_host",
               "components_host"):
        assert callable(getattr(hip, fn)), fn


def test_first_on_validation(hip):
    L = hip.lib
    assert L.lifeapi_first_on_batch_dev(None, None, 0, None) == 0
    assert L.lifeapi_first_on_batch_dev(A, None, 4, None) == -1 and b"null" in L.lifeapi_last_error()
    assert L.lifeapi_first_on_batch_dev(None, B, 4, None) == -1
    assert L.lifeapi_first_on_batch_dev(A + 4, B, 4, None) == -1
    assert L.lifeapi_first_on_batch_dev(A, B + 2, 4, None) == -1 and b"misaligned" in L.lifeapi_last_error()
    assert L.lifeapi_first_on_batch_dev(A, A + 1024, 4, None) == -1 and b"overlap" in L.lifeapi_last_error()
    assert L.lifeapi_first_on_batch(None, None, 0, 0) == 0
    assert L.lifeapi_first_on_batch(None, B, 4, 0) == -1


def test_component_containing_validation(hip):
    L = hip.lib
    cc = L.lifeapi_component_containing_batch_dev
    assert cc(None, None, 0, None, None, 0, None) == 0
    assert cc(None, B, 0, None, D, 4, None) == -1 and b"null" in L.lifeapi_last_error()
    assert cc(A, None, 0, None, D, 4, None) == -1 and b"seeds" in L.lifeapi_last_error()
    assert cc(A, B, 0, None, None, 4, None) == -1
    assert cc(A + 4, B, 0, None, D, 4, None) == -1
    assert cc(A, B + 4, 0, None, D, 4, None) == -1
    assert cc(A, B, 0, None, A + 512, 4, None) == -1 and b"overlap" in L.lifeapi_last_error()
    # one seed for the batch inside the output; per-universe seeds half over it
    assert cc(A, D + 512, 0, None, D, 4, None) == -1 and b"overlap" in L.lifeapi_last_error()
    assert cc(A, D + 512, 1, None, D, 4, None) == -1 and b"overlap" in L.lifeapi_last_error()
    # a corona without (0, 0), and the empty one, are ComponentContaining's to take
    for name in ("no_centre", "none", "7x7", "default"):
        assert cc(None, None, 0, ptr(C.CORONAS[name]), None, 0, None) == 0, name
        assert L.lifeapi_component_containing_batch(None, None, 0, ptr(C.CORONAS[name]), None, 0, 0) == 0, name
    assert L.lifeapi_component_containing_batch(A, None, 0, None, D, 4, 0) == -1
    assert L.lifeapi_component_containing_batch(A, B, 0, None, A + 512, 4, 0) == -1


def test_components_validation(hip):
    L = hip.lib
    comp = L.lifeapi_components_batch_dev
    assert comp(None, None, None, None, 0, 0, None) == 0
    assert comp(A, None, None, None, 8, 4, None) == -1 and b"both" in L.lifeapi_last_error()
    assert comp(A, None, None, D, 0, 4, None) == -1 and b"max_components" in L.lifeapi_last_error()
    assert comp(None, None, B, None, 0, 4, None) == -1 and b"null" in L.lifeapi_last_error()
    assert comp(A + 4, None, B, None, 0, 4, None) == -1
    assert comp(A, None, B + 2, None, 0, 4, None) == -1 and b"misaligned" in L.lifeapi_last_error()
    assert comp(A, None, B, D + 4, 2, 4, None) == -1 and b"misaligned" in L.lifeapi_last_error()
    assert comp(A, None, A + 8, None, 0, 4, None) == -1 and b"overlap" in L.lifeapi_last_error()
    assert comp(A, None, None, A + 512, 2, 4, None) == -1 and b"overlap" in L.lifeapi_last_error()
    assert comp(A, None, D + 64, D, 2, 4, None) == -1 and b"overlap" in L.lifeapi_last_error()
    # the corona must hold (0, 0), whatever else is asked, n == 0 included
    for name in ("no_centre", "none"):
        for n in (0, 4):
            assert comp(A, ptr(C.CORONAS[name]), B, D, 2, n, None) == -1, (name, n)
            assert b"corona" in L.lifeapi_last_error() and b"(0, 0)" in L.lifeapi_last_error()
            assert L.lifeapi_components_batch(A, ptr(C.CORONAS[name]), B, D, 2, n, 0) == -1, (name, n)
            assert b"corona" in L.lifeapi_last_error()
    for name in C.COMPONENTS_CORONAS:
        assert comp(None, ptr(C.CORONAS[name]), None, None, 0, 0, None) == 0, name
    assert L.lifeapi_components_batch(A, None, None, None, 8, 4, 0) == -1
    assert L.lifeapi_components_batch(A, None, None, D, 0, 4, 0) == -1


def test_python_wrappers_reject_bad_shapes(hip):
    with pytest.raises(ValueError):
        hip._corona(np.zeros(63, np.uint64))
    assert hip._corona(None) is None
    assert (hip._corona(C.CORONAS["plus"].view(np.int64)) == C.CORONAS["plus"]).all()
