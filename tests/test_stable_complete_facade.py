"""The C++ surface of CompleteStable (CompleteStableBatch, UnweldableMask of
lifeapi/batch.hpp) on the lifeapi:: structs: tests/cpp/
stable_complete_batch_test.cpp.  Without a GPU it compiles, links and runs the
checks that need no device; on one it replays a case file written here from
tests/golden/stable_complete.npz: the recorded searches in the four flag
combinations, and UnweldableMask against the masks the reference's own search
recorded for a few catalyst pairs (at most 64 placements each, at a budget that
some placements exhaust)."""
import os
import subprocess

import numpy as np
import pytest

import stable_complete_cases as C
import test_stable_complete_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "build")
NAME = "stable_complete_batch_test"


def build():
    """build/<NAME> from tests/cpp/<NAME>.cpp, rebuilt when a source is newer, linked as
    __graft_entry__.build_cpp_tests links it"""
    src, out = os.path.join(ROOT, "tests", "cpp", NAME + ".cpp"), os.path.join(BUILD, NAME)
    inc = os.path.join(ROOT, "include", "lifeapi")
    deps = [src, os.path.join(ROOT, "lifeapi_amd", "liblifeapi_hip.so")] + [os.path.join(inc, f) for f in os.listdir(inc)]
    if os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    os.makedirs(BUILD, exist_ok=True)
    subprocess.run(["g++", "-std=c++20", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), src,
                    "-o", out, "-L" + os.path.join(ROOT, "lifeapi_amd"), "-llifeapi_hip",
                    "-Wl,-rpath,$ORIGIN/../lifeapi_amd", "-Wl,-rpath,/opt/rocm/lib", "-pthread"], check=True)
    return out


def write_cases(path, rec, port, pick):
    """the case file of tests/cpp/stable_complete_batch_test.cpp for the objects `pick` and every weld case"""
    words = lambda a: np.ascontiguousarray(a, np.uint64).tobytes()   # noqa: E731
    welds = C.weld_inputs(port)
    with open(path, "wb") as f:
        f.write(words([len(pick), len(welds), C.WELD_BUDGET]))
        for u in pick:
            f.write(words(rec.planes[u]) + words(rec.seeds[u]))
            for fl in range(4):
                f.write(words([rec.result[u, fl], rec.nodes[u, fl]]) + words(rec.best[u, fl]))
        for c, w in enumerate(welds):
            f.write(b"".join(words(a) for a in (rec.weld["a"][c], rec.weld["b"][c], w[4], w[5], rec.weld["mask"][c])))


def test_weld_recording_is_not_vacuous():
    rec = M.recording()
    counts = rec.weld["counts"]
    assert len(counts) == len(C.WELD_CASES) >= 3
    tested = np.array([sum(M.pop(t) for t in [rec.weld["tested"][c]]) for c in range(len(counts))])
    assert (tested == counts.sum(axis=1)).all() and (tested <= 64).all() and (tested >= 16).all()
    # every case has placements with no completion and placements that exhaust the budget
    assert (counts[:, 1] > 0).all() and (counts[:, 2] > 0).all() and (counts[:, 0] > 0).all()
    for c in range(len(counts)):
        marked = rec.weld["mask"][c] & rec.weld["tested"][c]
        assert M.pop(marked) == counts[c, 1]


def test_batch_test_without_a_device():
    """compiles with -Werror, links, and its no-device checks pass: empty batches succeed,
    mismatched sizes and bad arguments throw LIFEAPI_E_INVALID"""
    r = subprocess.run([build()], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "ok (no device)" in r.stdout


def test_batch_test_under_host_sanitizers_without_a_device():
    """the same program with the library's host code (every csrc/*.hip, host side only) and the test
    under ASan + UBSan: the argument checks of the host form, no device touched"""
    exe = os.path.join(BUILD, NAME + "_asan")
    if not os.path.exists(exe):
        import __graft_entry__ as g
        g.build_asan_test()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:protect_shadow_gap=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout, r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "ok (no device)" in r.stdout


@pytest.mark.gpu
def test_batch_test_gpu(tmp_path, port, hip):
    rec = M.recording()
    pick = np.arange(0, len(rec.kept), 2)
    path = tmp_path / "cases.bin"
    write_cases(path, rec, port, pick)
    assert {0, 1} <= set(rec.result[pick].reshape(-1))
    r = subprocess.run([build(), str(path)], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "stable_complete_batch_test: ok\n" in r.stdout
