"""Records tests/golden/match.npz: the reference's own LifeState::Match(const
LifeTarget&), Convolve and InteractionOffsets (LifeTarget.hpp:53-55,
LifeAPI.hpp:432-435, 1293-1370, 1066-1095) on the inputs that
tests/test_match_model.py builds.  CPU only; run from the repository root
where the reference's headers are:

    python tests/golden/make_match_golden.py [--ref DIR] [--rate | --sharp]

match_ref_shim.cpp is compiled against those headers where they lie, into a
temporary directory, with the flags of oracle/Makefile (the forced prelude,
the xxHash include directory).  Only data is stored: the special input
states, the targets / patterns / others and the reference's outputs; the
seeded random states are regenerated from Port.fill.  --rate instead prints
the reference's CPU rate for Match on every target (16 threads), for scale;
--sharp instead records tests/golden/match_sharp.npz, the same three functions
on the inputs of tests/match_sharp.py (near misses, impulses, sparse soups
with clusters), all of them regenerated from seeds but the impulse states.
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


def compile_shim(ref, tmp):
    os.makedirs(os.path.join(tmp, "inc", "xxHash"))
    os.symlink(os.path.join(XXH_DIR, "xxhash.h"), os.path.join(tmp, "inc", "xxHash", "xxhash.h"))
    exe = os.path.join(tmp, "match_ref_shim")
    lib = os.path.join(ROOT, "lifeapi_amd")
    # (the standard headers lifeapi/batch.hpp and the shim use come in
    # ahead of the prelude, which defines `constexpr` away after its own)
    pre = [x for h in ("span", "stdexcept", "type_traits", "chrono", "cstdio") for x in ("-include", h)]
    subprocess.run([CXX, "-std=c++20", "-O2", "-march=x86-64-v3", "-pthread", "-Wno-nonportable-include-path",
                    "-Wno-undefined-inline", *pre, "-include", os.path.join(ROOT, "oracle", "ref_prelude.hpp"),
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(tmp, "inc"), "-I" + ref,
                    os.path.join(HERE, "match_ref_shim.cpp"), "-o", exe, "-L" + lib, "-llifeapi_hip",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


Z = np.zeros((0, 64), np.uint64)


def write_input(path, states, t=Z.reshape(0, 2, 64), p=Z, o=Z):
    with open(path, "wb") as f:
        f.write(np.array([len(states), len(t), len(p), len(o)], np.uint64).tobytes())
        for a in (states, t, p, o):
            f.write(np.ascontiguousarray(a, np.uint64).tobytes())


def reference(exe, tmp, states, t=Z.reshape(0, 2, 64), p=Z, o=Z):
    """the reference's (match[target][state], convolve[pattern][state],
    interaction[other][state]): every target, pattern and other on every state"""
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    write_input(fin, states, t, p, o)
    subprocess.run([exe, fin, fout], check=True)
    out = np.fromfile(fout, np.uint64)
    n = len(states)
    assert out.size == (len(t) + len(p) + len(o)) * n * 64
    out = out.reshape(-1, n, 64)
    return out[:len(t)], out[len(t):len(t) + len(p)], out[len(t) + len(p):]


def record_sharp(port, exe, tmp, targets, patterns):
    """tests/golden/match_sharp.npz: the reference on the inputs of
    tests/match_sharp.py.  Every target on its own near misses (one run of the
    shim each), every pattern on the impulse states, every sharp other on the
    first N_RECORDED universes of interaction_batch."""
    import match_sharp as S
    cases = S.near_miss_cases(port, targets)
    masks = []
    for name, (states, (dx, dy)) in cases.items():
        m = reference(exe, tmp, states, np.stack(targets[name])[None])[0][0]
        assert (int(m[0][dx]) >> dy) & 1, name                     # the planted match is one
        assert not ((m[1:, dx] >> np.uint64(dy)) & np.uint64(1)).any(), name   # and no near miss matches there
        masks.append(m)
    impulses = S.impulse_states()
    conv = reference(exe, tmp, impulses, p=np.stack(list(patterns.values())))[1]
    others = S.sharp_others(port)
    o = np.stack(list(others.values()))
    inter = reference(exe, tmp, S.interaction_batch(port, S.N_RECORDED), o=o)[2]
    path = os.path.join(HERE, "match_sharp.npz")
    np.savez_compressed(path, near_miss_names=np.array(list(cases)), near_miss_match=np.concatenate(masks),
                        impulse_states=impulses, pattern_names=np.array(list(patterns)), convolve=conv,
                        other_names=np.array(list(others)), others=o, interaction=inter)
    print(f"{path}: {os.path.getsize(path)} bytes; {sum(map(len, masks))} near misses of {len(cases)} targets, "
          f"{len(patterns)} patterns x {len(impulses)} impulses, {len(o)} others x {S.N_RECORDED} universes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--rate", action="store_true")
    ap.add_argument("--sharp", action="store_true")
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
        exe = compile_shim(args.ref, tmp)
        if args.rate:
            fin = os.path.join(tmp, "in.bin")
            write_input(fin, states, t, p, o)
            subprocess.run([exe, fin, "--rate"], check=True)
            print("targets:", ", ".join(f"{k} {name}" for k, name in enumerate(targets)))
            return
        if args.sharp:
            record_sharp(port, exe, tmp, targets, patterns)
            return
        match, conv, inter = reference(exe, tmp, states, t, p, o)
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
