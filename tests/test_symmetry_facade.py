"""The C++ surfaces of the symmetry layer against tests/golden/symmetry.npz:
the single-universe members of lifeapi/LifeState.hpp on the CPU
(tests/cpp/symmetry_facade_test.cpp; compiles and runs without a GPU), and
helpers for the batched templates' GPU test
(tests/test_gpu_symmetry.py::test_symmetry_batch_cpp).  Both programs read one
binary case file written here from the npz (tests/cpp/symmetry_cases.hpp)."""
import os
import subprocess

import numpy as np
import pytest

import test_symmetry_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "build")


def build(name, gpu=False):
    """build/<name> from tests/cpp/<name>.cpp, rebuilt when a source is newer;
    the GPU program links the library as __graft_entry__.build_cpp_tests does"""
    src, out = os.path.join(ROOT, "tests", "cpp", name + ".cpp"), os.path.join(BUILD, name)
    inc = os.path.join(ROOT, "include", "lifeapi")
    deps = [src, os.path.join(ROOT, "tests", "cpp", "symmetry_cases.hpp")] + [os.path.join(inc, f) for f in os.listdir(inc)]
    if os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    os.makedirs(BUILD, exist_ok=True)
    cmd = ["g++", "-std=c++20", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", out]
    if gpu:
        cmd += ["-L" + os.path.join(ROOT, "lifeapi_amd"), "-llifeapi_hip", "-Wl,-rpath,$ORIGIN/../lifeapi_amd",
                "-Wl,-rpath,/opt/rocm/lib", "-pthread"]
    subprocess.run(cmd, check=True)
    return out


def write_cases(path, port, gold):
    """every array of the golden as the case file of tests/cpp/symmetry_cases.hpp"""
    ts, ss = M.transform_states(port), M.symmetricize_states(port)
    tr = [(t, 0, 0, s, gold["transform"][t][k]) for t in range(16) for k, s in enumerate(ts)]
    tr += [(t, dx, dy, s, gold["transform_move"][t][m][k]) for t in range(16) for m, (dx, dy) in enumerate(M.MOVES)
           for k, s in enumerate(ts[:2])]
    sy = [(sym, dx, dy, s, gold["symmetricize"][j][i][o]) for j, sym in enumerate(M.SYMMETRIES.values())
          for i, s in enumerate(ss) for o, (dx, dy) in enumerate(M.OFFSETS)]
    orbit_states = gold["orbit_states"].reshape(-1, 64)
    with open(path, "wb") as f:
        f.write(np.array([len(tr), len(sy), len(orbit_states)], np.uint64).tobytes())
        for kind, dx, dy, a, b in tr + sy:
            f.write(np.array([kind, dx, dy], np.int64).tobytes())
            f.write(np.ascontiguousarray(a, np.uint64).tobytes() + np.ascontiguousarray(b, np.uint64).tobytes())
        for k, s in enumerate(orbit_states):
            f.write(np.ascontiguousarray(s, np.uint64).tobytes())
            f.write(gold["bounds"].reshape(-1, 4)[k].astype(np.int64).tobytes())
            f.write(np.ascontiguousarray(gold["orbit_images"].reshape(-1, 8, 64)[k], np.uint64).tobytes())
            f.write(np.array([gold["orbit_mask"].ravel()[k]], np.uint64).tobytes())


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(M.GOLDEN))


def test_facade_symmetry_members_cpu(tmp_path, port, gold):
    """Transform / Transformed / Transform(dx, dy, t), FlipX, FlipY, BitReverse,
    Transpose, TransformInverse, XYBounds, SymmetryOrbit[Representatives],
    PerpComponent, Symmetricize and LifeTarget::Transform[ed] on every golden case"""
    exe = build("symmetry_facade_test")
    path = tmp_path / "cases.bin"
    write_cases(path, port, gold)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "ok (480 transforms, 162 symmetries, 48 orbits)" in r.stdout


def test_batch_test_compiles_without_gpu():
    """the GPU program's source is self-contained C++20 (syntax only here)"""
    subprocess.run(["g++", "-std=c++20", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "symmetry_batch_test.cpp")], check=True)
