"""The C++ surfaces of the connected-component family against
tests/golden/components.npz: the single-universe members of
lifeapi/LifeState.hpp on the CPU (tests/cpp/components_facade_test.cpp; compiles
and runs without a GPU), and helpers for the batched templates' GPU test
(tests/test_gpu_components.py::test_components_batch_cpp).  Both programs read
one binary case file written here from the npz (tests/cpp/components_cases.hpp)."""
import os
import subprocess

import numpy as np
import pytest

import components_cases as C
import test_components_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "build")


def build(name, gpu=False):
    """build/<name> from tests/cpp/<name>.cpp, rebuilt when a source is newer;
    the GPU program links the library as __graft_entry__.build_cpp_tests does"""
    src, out = os.path.join(ROOT, "tests", "cpp", name + ".cpp"), os.path.join(BUILD, name)
    inc = os.path.join(ROOT, "include", "lifeapi")
    deps = [src, os.path.join(ROOT, "tests", "cpp", "components_cases.hpp")] + [os.path.join(inc, f) for f in os.listdir(inc)]
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
    """every array of the golden as the case file of tests/cpp/components_cases.hpp;
    returns the three section sizes"""
    states = C.states(port)
    seeds = M.cc_seeds(states)
    words = lambda a: np.ascontiguousarray(a, np.uint64).tobytes()   # noqa: E731
    cc = [(states[n], seeds[n][kind], C.CORONAS[corona], gold["cc"][c, i, k]) for c, corona in enumerate(C.CORONAS)
          for i, n in enumerate(C.CC_STATES) for k, kind in enumerate(C.SEED_KINDS)]
    parts = [(states[n], C.CORONAS[corona], p) for corona in C.COMPONENTS_CORONAS
             for n, p in M.recorded_parts(gold, states, corona).items()]
    with open(path, "wb") as f:
        f.write(np.array([len(states), len(cc), len(parts)], np.uint64).tobytes())
        for s, cell in zip(states.values(), gold["first_on"]):
            f.write(words(s) + cell.astype(np.int64).tobytes())
        for case in cc:
            f.write(b"".join(words(a) for a in case))
        for s, corona, p in parts:
            f.write(words(s) + words(corona) + np.array([len(p)], np.uint64).tobytes() + words(p))
    return len(states), len(cc), len(parts)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(M.GOLDEN))


def test_facade_component_members_cpu(tmp_path, port, gold):
    """FirstOn, FirstCell, ComponentContaining(seed[, corona]) and
    Components([corona]) on every golden case"""
    exe = build("components_facade_test")
    path = tmp_path / "cases.bin"
    sizes = write_cases(path, port, gold)
    assert sizes == (145, 288, 705)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "ok (145 cells, 288 seeds, 705 lists)" in r.stdout


def test_batch_test_compiles_without_gpu():
    """the GPU program's source is self-contained C++20 (syntax only here)"""
    subprocess.run(["g++", "-std=c++20", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "tests", "cpp"),
                    os.path.join(ROOT, "tests", "cpp", "components_batch_test.cpp")], check=True)
