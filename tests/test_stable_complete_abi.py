"""CPU: the CompleteStable entry points are exported and bound, and they
validate their arguments before touching any device (no compute calls here:
every call below either fails validation or has n == 0)."""
import ctypes
import os

import numpy as np
import pytest

BASE = "lifeapi_stable_complete_batch"
# made-up, aligned, far apart: validation never reads through them
P, S, B, R, C, W = 1 << 20, 1 << 24, 1 << 28, 1 << 30, 1 << 32, 1 << 34
N = 4
FRAME, HEADER = 5376, 256


@pytest.fixture(scope="module")
def hip():
    import lifeapi_amd.hip as h
    return h


def err(hip):
    return hip.lib.lifeapi_last_error()


def call(hip, dev, planes=P, seeds=S, per=0, flags=0, budget=0, depth=8, best=B, result=R, nodes=C, n=N, ws=W,
         ws_bytes=HEADER + 8 * FRAME):
    if dev:
        return hip.lib.lifeapi_stable_complete_batch_dev(planes, seeds, per, flags, budget, depth, best, result, nodes, n,
                                                         ws, ws_bytes, None)
    return hip.lib.lifeapi_stable_complete_batch(planes, seeds, per, flags, budget, depth, best, result, nodes, n, 0)


def test_symbols_exported_and_bound(hip):
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in (BASE + "_dev", BASE, "lifeapi_stable_complete_workspace_bytes"):
        assert hasattr(lib, name), name
        assert name in hip.EXPORTS, name
    assert hip.lib.lifeapi_stable_complete_workspace_bytes.restype is ctypes.c_size_t
    assert hip.abi_version() == 2
    for fn in ("stable_complete", "stable_complete_host", "stable_complete_workspace_bytes"):
        assert callable(getattr(hip, fn)), fn
    assert (hip.COMPLETE_MINIMISE, hip.COMPLETE_USE_SEED) == (1, 2)


def test_header_declares_and_states_the_semantics(hip):
    text = open(os.path.join(os.path.dirname(os.path.dirname(hip.LIB_PATH)), "include", "lifeapi_hip.h")).read()
    for decl in ("size_t lifeapi_stable_complete_workspace_bytes(", f"int {BASE}_dev(", f"int {BASE}(",
                 "#define LIFEAPI_COMPLETE_MINIMISE 1u", "#define LIFEAPI_COMPLETE_USE_SEED 2u",
                 "#define LIFEAPI_ABI_VERSION 2"):
        assert decl in text, decl
    # the budget's placement, the three defined cases, the quirks kept
    for words in ("LifeStable.hpp:\n * 1340-1458", "nodes >= node_budget", ":1343", ":1439", "state.ZOI()", "empty seed",
                  "max_depth frames", "a TIMEOUT with a\n * non-empty best is COMPLETED", "minimise pass is\n * ignored",
                  ":1415-1420", ":1378-1391", "currentPop >= maxPop"):
        assert words in text, words


@pytest.mark.parametrize("dev", [True, False])
def test_n_zero_succeeds_with_any_pointers(hip, dev):
    assert call(hip, dev, None, None, 0, 0, 0, 0, None, None, None, 0, None, 0) == 0
    assert call(hip, dev, P + 3, S + 1, 1, 255, 1 << 40, 9999, P, P, P, 0, P, 1) == 0


@pytest.mark.parametrize("dev", [True, False])
def test_validation(hip, dev):
    bad = lambda **kw: call(hip, dev, **kw)     # noqa: E731
    for kw in (dict(planes=None), dict(best=None), dict(result=None), dict(seeds=None, flags=2), dict(seeds=None, flags=3)):
        assert bad(**kw) == -1 and b"null" in err(hip), kw
    for kw in (dict(planes=P + 4), dict(best=B + 4), dict(nodes=C + 4), dict(seeds=S + 4, flags=2)):
        assert bad(**kw) == -1 and b"misaligned" in err(hip), kw
    for flags in (4, 8, 1 << 31, 7):
        assert bad(flags=flags) == -1 and b"flag" in err(hip), flags
    for depth in (0, 4097, 1 << 31):
        assert bad(depth=depth) == -1 and b"max_depth" in err(hip), depth
    for budget in ((1 << 24) + 1, 1 << 32, (1 << 64) - 1):
        assert bad(budget=budget) == -1 and b"node_budget" in err(hip), budget
    # outputs over the inputs' first and last byte, over the one seed and the N seeds, over each other
    for kw in (dict(best=P), dict(best=P + 5120 * N - 8), dict(result=P + 5120 * N - 1), dict(nodes=P - 8 * N + 8),
               dict(best=S, flags=2), dict(result=S + 511, flags=2), dict(result=S + 512 * N - 1, flags=2, per=1),
               dict(result=B), dict(nodes=B + 512 * N - 8), dict(result=C + 8 * N - 1)):
        assert bad(**kw) == -1 and b"overlap" in err(hip), kw


def test_workspace_validation(hip):
    bad = lambda **kw: call(hip, True, **kw)    # noqa: E731
    assert bad(ws=None) == -1 and b"d_workspace" in err(hip)
    for ws in (W + 8, W + 64):
        assert bad(ws=ws) == -1 and b"aligned" in err(hip), ws
    # one stack of max_depth frames behind the header is the least
    for depth in (1, 8, 4096):
        assert bad(depth=depth, ws_bytes=HEADER + depth * FRAME - 1) == -1 and b"below one" in err(hip), depth
    assert bad(ws_bytes=0) == -1 and b"below one" in err(hip)
    # over the planes' end, the best states, the result bytes, the node counts, the seed
    for kw in (dict(ws=P + 5120 * N - 128), dict(best=W + 128), dict(result=W + HEADER + 8 * FRAME - 1), dict(nodes=W),
               dict(seeds=W + 1024, flags=2)):
        assert bad(**kw) == -1 and b"overlap" in err(hip), kw


def test_workspace_bytes_rejects_bad_depths(hip):
    f = hip.lib.lifeapi_stable_complete_workspace_bytes
    for depth in (0, 4097):
        assert f(N, depth) == 0 and b"max_depth" in err(hip)
        with pytest.raises(hip.LifeApiError):
            hip.stable_complete_workspace_bytes(N, depth)
    # no objects: the least that is accepted, no device asked
    assert f(0, 8) == HEADER + 8 * FRAME and f(0, 4096) == HEADER + 4096 * FRAME


def test_python_wrappers_reject_bad_shapes(hip):
    s = np.zeros((3, 640), np.uint64)
    with pytest.raises(ValueError):
        hip.stable_complete_host(np.zeros(641, np.uint64))
    with pytest.raises(ValueError):
        hip.stable_complete_host(s, seed=np.zeros((2, 64), np.uint64))
    with pytest.raises(ValueError):
        hip.stable_complete_host(s, seed=np.zeros(65, np.uint64))
    result, best, nodes = hip.stable_complete_host(s[:0], minimise=True, seed=np.zeros(64, np.uint64))
    assert result.shape == (0,) and best.shape == (0, 64) and nodes.shape == (0,)
