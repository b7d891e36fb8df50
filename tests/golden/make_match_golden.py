"""Records tests/golden/match.npz: the reference's own LifeState::Match(const
LifeTarget&), Convolve and InteractionOffsets (LifeTarget.hpp:53-55,
LifeAPI.hpp:432-435, 1293-1370, 1066-1095) on the inputs that
tests/test_match_model.py builds.  CPU only; run from the repository root
where the reference's headers are:

    python tests/golden/make_match_golden.py [--ref DIR] [--rate]

match_ref_shim.cpp is compiled against those headers where they lie, into a
temporary directory, with the flags of oracle/Makefile (the forced prelude,
the xxHash include directory).  Only data is stored: the special input
states, the targets / patterns / others and the reference's outputs; the
seeded random states are regenerated from Port.fill.  --rate instead prints
the reference's CPU rate for Match on every target (16 threads), for scale.
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_match_model as M  # noqa: E402
from oracle.oracle import Port  # noqa: E402

XXH_DIR = "/usr/local/lib/python3.10/dist-packages/pyarrow/include/arrow/vendored/xxhash"  # oracle/Makefile
CXX = "/opt/rocm/lib/llvm/bin/clang++"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--rate", action="store_true")
    args = ap.parse_args()
    port = Port()
    special = M.special_states(port)
    assert len(special) == M.N_SPECIAL
    states = M.all_states(port, special)
    targets, patterns, others = M.build_targets(port, states), M.build_patterns(port), M.build_others(port)
    t = np.stack([np.stack(v) for v in targets.values()])
    p, o = np.stack(list(patterns.values())), np.stack(list(others.values()))
    n = len(states)
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "inc", "xxHash"))
        os.symlink(os.path.join(XXH_DIR, "xxhash.h"), os.path.join(tmp, "inc", "xxHash", "xxhash.h"))
        exe = os.path.join(tmp, "match_ref_shim")
        lib = os.path.join(ROOT, "lifeapi_amd")
        # (the standard headers lifeapi/batch.hpp and the shim use come in
        # ahead of the prelude, which defines `constexpr` away after its own)
        pre = [x for h in ("span", "stdexcept", "type_traits", "chrono", "cstdio") for x in ("-include", h)]
        subprocess.run([CXX, "-std=c++20", "-O2", "-march=x86-64-v3", "-pthread", "-Wno-nonportable-include-path",
                        "-Wno-undefined-inline", *pre, "-include", os.path.join(ROOT, "oracle", "ref_prelude.hpp"),
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(tmp, "inc"), "-I" + args.ref,
                        os.path.join(HERE, "match_ref_shim.cpp"), "-o", exe, "-L" + lib, "-llifeapi_hip",
                        "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True)
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            f.write(np.array([n, len(t), len(p), len(o)], np.uint64).tobytes())
            for a in (states, t, p, o):
                f.write(np.ascontiguousarray(a, np.uint64).tobytes())
        if args.rate:
            subprocess.run([exe, fin, "--rate"], check=True)
            print("targets:", ", ".join(f"{k} {name}" for k, name in enumerate(targets)))
            return
        subprocess.run([exe, fin, fout], check=True)
        out = np.fromfile(fout, np.uint64)
    assert out.size == (len(t) + len(p) + len(o)) * n * 64
    out = out.reshape(-1, n, 64)
    match, conv, inter = out[:len(t)], out[len(t):len(t) + len(p)], out[len(t) + len(p):]
    # non-vacuity, on the reference's outputs alone
    ok = M.nonvacuity(states, t, match)
    assert ok == (True, True, True), ok
    path = os.path.join(HERE, "match.npz")
    np.savez_compressed(path, special_states=special, target_names=np.array(list(targets)), targets=t,
                        pattern_names=np.array(list(patterns)), patterns=p, other_names=np.array(list(others)),
                        others=o, match=match, convolve=conv, interaction=inter)
    print(f"{path}: {os.path.getsize(path)} bytes; {len(t)} targets, {len(p)} patterns, {len(o)} others x {n} states")


if __name__ == "__main__":
    main()
