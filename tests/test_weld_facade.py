"""The C++ surfaces of the LifeWeld construction family against
tests/golden/weld_family.npz: the single-object members of lifeapi/LifeState.hpp on the
CPU (tests/cpp/weld_facade_test.cpp; compiles and runs without a GPU), and
helpers for the batched templates' GPU test
(tests/test_gpu_weld.py::test_weld_batch_cpp).  Both programs read one binary
case file written here from the npz (tests/cpp/weld_cases.hpp)."""
import os
import subprocess

import numpy as np

import test_weld_model as M
import weld_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "build")


def build(name, gpu=False):
    """build/<name> from tests/cpp/<name>.cpp, rebuilt when a source is newer;
    the GPU program links the library as __graft_entry__.build_cpp_tests does"""
    src, out = os.path.join(ROOT, "tests", "cpp", name + ".cpp"), os.path.join(BUILD, name)
    inc = os.path.join(ROOT, "include", "lifeapi")
    deps = [src, os.path.join(ROOT, "tests", "cpp", "weld_cases.hpp")] + [os.path.join(inc, f) for f in os.listdir(inc)]
    if os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    os.makedirs(BUILD, exist_ok=True)
    cmd = ["g++", "-std=c++20", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", out]
    if gpu:
        cmd += ["-L" + os.path.join(ROOT, "lifeapi_amd"), "-llifeapi_hip", "-Wl,-rpath,$ORIGIN/../lifeapi_amd",
                "-Wl,-rpath,/opt/rocm/lib", "-pthread"]
    subprocess.run(cmd, check=True)
    return out


def write_cases(path, rec):
    """the recording as the case file of tests/cpp/weld_cases.hpp; returns the four section sizes"""
    words = lambda a: np.ascontiguousarray(a, np.uint64).tobytes()   # noqa: E731
    required = [(s, r, w) for (s, r), w in zip(rec.pairs.values(), rec.from_required)]
    statics = list(zip(rec.welds.values(), rec.target, rec.stable0))
    replays = [(rec.welds[w], rec.actives[a], rec.masks[m], np.array([d], np.uint64), want)
               for (w, a, d, m), want in zip(C.STABLE_CASES, rec.stable)]
    offsets = [(rec.welds[n], rec.welds[o], rec.offsets[i, j]) for i, o in enumerate(C.OFFSET_OTHERS)
               for j, n in enumerate(C.OFFSET_WELDS)]
    with open(path, "wb") as f:
        f.write(np.array([len(required), len(statics), len(replays), len(offsets)], np.uint64).tobytes())
        for section in (required, statics, replays, offsets):
            for case in section:
                f.write(b"".join(words(a) for a in case))
    return len(required), len(statics), len(replays), len(offsets)


def test_facade_weld_members_cpu(tmp_path, port):
    """FromRequired, ToTarget, ToStable() and ToStable(active, duration, mask),
    InteractionOffsets, AllFrozen, operator| and Moved on every golden case"""
    exe = build("weld_facade_test")
    path = tmp_path / "cases.bin"
    sizes = write_cases(path, M.Recording(port))
    assert sizes == (18, 29, 59, 95)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "ok (18 pairs, 29 welds, 59 replays, 95 offsets)" in r.stdout


def test_batch_test_compiles_without_gpu():
    """the GPU program's source is self-contained C++20 (syntax only here)"""
    subprocess.run(["g++", "-std=c++20", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "tests", "cpp"),
                    os.path.join(ROOT, "tests", "cpp", "weld_batch_test.cpp")], check=True)
