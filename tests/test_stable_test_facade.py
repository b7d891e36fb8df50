"""The C++ surface of the LifeStable lookahead family (PropagateStripBatch,
TestUnknownsBatch, PropagateAndTestBatch of lifeapi/batch.hpp) on the lifeapi::
structs: tests/cpp/stable_test_batch_test.cpp.  Without a GPU it compiles, links
and runs the checks that need no device; on one it replays a case file written
here from tests/golden/stable_test.npz."""
import os
import subprocess

import numpy as np
import pytest

import test_stable_test_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "build")
NAME = "stable_test_batch_test"


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
    """the case file of tests/cpp/stable_test_batch_test.cpp for the objects `pick`"""
    tested, _ = port.stable_pass(rec.planes[pick].reshape(-1, 640), 4)
    words = lambda a: np.ascontiguousarray(a, np.uint64).tobytes()   # noqa: E731
    with open(path, "wb") as f:
        f.write(words([len(pick)]))
        for u, t in zip(pick, tested):
            cells = M.vulnerable_zoi(port, t.reshape(10, 64))
            f.write(b"".join(words(a) for a in (
                rec.planes[u], [rec.columns[u]], rec.pat[u], [rec.pat_flags[u]], rec.strip(u, 0, 7, 4),
                [rec.strip_flags[u, 0, 7, 4]], t, cells, rec.tu[u], [rec.tu_flags[u]])))


def test_batch_test_without_a_device():
    """compiles with -Werror, links, and its no-device checks pass: empty batches succeed,
    mismatched sizes throw LIFEAPI_E_INVALID"""
    r = subprocess.run([build()], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "ok (no device)" in r.stdout


@pytest.mark.gpu
def test_batch_test_gpu(tmp_path, port, hip):
    rec = M.Recording()
    pick = np.arange(0, len(rec.kept), 3)
    path = tmp_path / "cases.bin"
    write_cases(path, rec, port, pick)
    assert {0, 1, 3} <= set(rec.pat_flags[pick]) and {0, 3} <= set(rec.tu_flags[pick])
    r = subprocess.run([build(), str(path)], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "stable_test_batch_test: ok\n" in r.stdout
