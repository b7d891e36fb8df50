"""The C++ surfaces of IntersectingOffsets, Halve and Skew against
tests/golden/pair.npz: the single-universe members and free functions of
lifeapi/LifeState.hpp on the CPU (tests/cpp/pair_facade_test.cpp; compiles and
runs without a GPU), and helpers for the batched templates' GPU test
(tests/test_gpu_pair.py::test_pair_batch_cpp).  Both programs read one binary
case file written here from the npz (tests/cpp/pair_cases.hpp)."""
import os
import subprocess

import numpy as np
import pytest

import test_pair_model as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "build")


def build(name, gpu=False):
    """build/<name> from tests/cpp/<name>.cpp, rebuilt when a source is newer;
    the GPU program links the library as __graft_entry__.build_cpp_tests does"""
    src, out = os.path.join(ROOT, "tests", "cpp", name + ".cpp"), os.path.join(BUILD, name)
    inc = os.path.join(ROOT, "include", "lifeapi")
    deps = [src, os.path.join(ROOT, "tests", "cpp", "pair_cases.hpp")] + [os.path.join(inc, f) for f in os.listdir(inc)]
    if gpu:
        deps.append(os.path.join(ROOT, "lifeapi_amd", "liblifeapi_hip.so"))
    if os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    os.makedirs(BUILD, exist_ok=True)
    cmd = ["g++", "-std=c++20", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", out]
    if gpu:
        cmd += ["-L" + os.path.join(ROOT, "lifeapi_amd"), "-llifeapi_hip", "-Wl,-rpath,$ORIGIN/../lifeapi_amd",
                "-Wl,-rpath,/opt/rocm/lib", "-pthread"]
    subprocess.run(cmd, check=True)
    return out


def cases(port, gold):
    """every array of the golden as (kind, arg, a, b, out)"""
    p1, p2 = P.sparse_pairs()
    pat2, zero = P.M.cells([P.RESIDUE_PAT2]), np.zeros(64, np.uint64)
    out = []
    for k, sym in enumerate(P.IO_SYMS):
        y = P.IO_VALUES[sym]
        out += [(0, y, s, pat2, P.M.cell(*at.tolist())) for s, at in zip(P.residue_states(), gold["residue_landing"][k])]
        out += [(0, y, p1[i], p2[i], gold["sparse_pairs"][k, i]) for i in range(P.N_SPARSE)]
        out += [(0, y, p1[i], p1[i], gold["sparse_self"][k, i]) for i in range(P.N_SPARSE)]
        for i, (_, x, z) in enumerate(P.choice_cases(port)):
            out += [(0, y, x, z, gold["choice"][k, i, 0]), (0, y, z, x, gold["choice"][k, i, 1])]
    a, b = P.pair16()
    out += [(1, t, a[i], b[i], gold["convolve_pair"][t, i]) for t in range(16) for i in range(P.N_PAIR16)]
    hs = P.halve_states(port)
    out += [(2, m, s, zero, gold["halve"][m, i]) for m in range(3) for i, s in enumerate(hs)]
    out += [(3, v, s, zero, gold["skew"][v, i]) for v in range(2) for i, s in enumerate(hs)]
    return out


def write_cases(path, port, gold):
    """the case file of tests/cpp/pair_cases.hpp; returns the number of cases"""
    all_cases = cases(port, gold)
    with open(path, "wb") as f:
        f.write(np.array([len(all_cases)], np.uint64).tobytes())
        for kind, arg, a, b, out in all_cases:
            f.write(np.array([kind, arg], np.int64).tobytes())
            for s in (a, b, out):
                f.write(np.ascontiguousarray(s, np.uint64).tobytes())
    return len(all_cases)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(P.GOLDEN))


def test_facade_pair_members_cpu(tmp_path, port, gold):
    """IntersectingOffsets (both forms), Convolve of a transformed operand,
    Halve / HalveX / HalveY and Skew / InvSkew on every golden case"""
    exe = build("pair_facade_test")
    path = tmp_path / "cases.bin"
    write_cases(path, port, gold)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "ok (1752 offsets, 252 self, 96 convolutions, 408 halves, 272 skews)" in r.stdout


def test_batch_test_compiles_without_gpu():
    """the GPU program's source is self-contained C++20 (syntax only here)"""
    subprocess.run(["g++", "-std=c++20", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "pair_batch_test.cpp")], check=True)
