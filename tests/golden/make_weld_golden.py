"""Records tests/golden/weld_family.npz: the reference's own LifeWeld::FromRequired,
ToTarget, ToStable and InteractionOffsets (LifeWeld.hpp:133-400) on the inputs
that tests/weld_cases.py builds.  CPU only; run from the repository root where
the reference's headers are:

    python tests/golden/make_weld_golden.py [--ref DIR]

weld_ref_shim.cpp is compiled against those headers where they lie, into a
temporary directory, with the flags of make_components_golden.py.  Only data is
stored: the reference's outputs; the inputs are rebuilt by weld_cases.py.
Non-vacuity is asserted on the reference's outputs alone, before anything is
written.

  from_required  (pairs, 4, 64)    FromRequired of weld_cases.pairs, in order
  target         (welds, 2, 64)    ToTarget of weld_cases.welds, in order
  stable0        (welds, 10, 64)   ToStable()
  stable         (cases, 10, 64)   ToStable(active, duration, mask), STABLE_CASES
  offsets        (others, welds, 64)  InteractionOffsets, OFFSET_OTHERS x OFFSET_WELDS
  state_offsets  (welds, 64)       LifeState::InteractionOffsets of the states of
                                   OFFSET_WELDS with plain_eater's
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]

import weld_cases as C  # noqa: E402
from make_match_golden import CXX, XXH_DIR  # noqa: E402
from oracle.oracle import Port  # noqa: E402

FROM_REQUIRED, TO_TARGET, TO_STABLE0, TO_STABLE, TO_STABLE_DEFAULT_MASK, OFFSETS, STEPPED, STATE_OFFSETS, OWN_SIDE = range(9)
SIZE = {FROM_REQUIRED: 256, TO_TARGET: 128, TO_STABLE0: 640, TO_STABLE: 640, TO_STABLE_DEFAULT_MASK: 640, OFFSETS: 64,
        STEPPED: 256, STATE_OFFSETS: 64, OWN_SIDE: 64}
Z, ZW = np.zeros(64, np.uint64), np.zeros(256, np.uint64)


def compile_shim(ref, tmp):
    os.makedirs(os.path.join(tmp, "inc", "xxHash"))
    os.symlink(os.path.join(XXH_DIR, "xxhash.h"), os.path.join(tmp, "inc", "xxHash", "xxhash.h"))
    exe = os.path.join(tmp, "weld_ref_shim")
    lib = os.path.join(ROOT, "lifeapi_amd")
    pre = [x for h in ("span", "stdexcept", "type_traits", "array", "utility", "cstdio") for x in ("-include", h)]
    subprocess.run([CXX, "-std=c++20", "-O2", "-march=x86-64-v3", "-pthread", "-Wno-nonportable-include-path",
                    "-Wno-undefined-inline", *pre, "-include", os.path.join(ROOT, "oracle", "ref_prelude.hpp"),
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(tmp, "inc"), "-I" + ref,
                    os.path.join(HERE, "weld_ref_shim.cpp"), "-o", exe, "-L" + lib, "-llifeapi_hip",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def reference(exe, tmp, ops):
    """ops: (kind, duration, weld, other, x, y); the shim's output per op"""
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([len(ops)], np.uint64).tobytes())
        for kind, duration, weld, other, x, y in ops:
            f.write(np.array([kind, duration], np.int64).tobytes())
            for a, k in ((weld, 256), (other, 256), (x, 64), (y, 64)):
                a = np.ascontiguousarray(a, np.uint64).reshape(-1)
                assert a.size == k
                f.write(a.tobytes())
    subprocess.run([exe, fin, fout], check=True, timeout=600)
    out, res, at = np.fromfile(fout, np.uint64), [], 0
    for kind, *_ in ops:
        res.append(out[at:at + SIZE[kind]])
        at += SIZE[kind]
    assert at == out.size
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    port = Port()
    pairs = C.pairs(port)
    data = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = compile_shim(args.ref, tmp)
        run = lambda ops: np.stack(reference(exe, tmp, ops))   # noqa: E731
        data["from_required"] = run([(FROM_REQUIRED, 0, ZW, ZW, s, r) for s, r in pairs.values()]).reshape(-1, 4, 64)
        welds = C.welds(port, data["from_required"])
        names = list(welds)
        data["target"] = run([(TO_TARGET, 0, w, ZW, Z, Z) for w in welds.values()]).reshape(-1, 2, 64)
        data["stable0"] = run([(TO_STABLE0, 0, w, ZW, Z, Z) for w in welds.values()]).reshape(-1, 10, 64)
        act, msk = C.actives(port), C.masks(port)
        data["stable"] = run([(TO_STABLE, d, welds[w], ZW, act[a], msk[m]) for w, a, d, m in C.STABLE_CASES]).reshape(-1, 10, 64)
        data["offsets"] = run([(OFFSETS, 0, welds[n], welds[o], Z, Z) for o in C.OFFSET_OTHERS
                               for n in C.OFFSET_WELDS]).reshape(len(C.OFFSET_OTHERS), len(C.OFFSET_WELDS), 64)
        data["state_offsets"] = run([(STATE_OFFSETS, 0, welds[n], welds["plain_eater"], Z, Z) for n in C.OFFSET_WELDS])
        # ---- for the checks below only ----
        stepped = run([(STEPPED, 0, welds[n], ZW, Z, Z) for n in C.REFERENCE_PAIRS]).reshape(-1, 4, 64)
        own_side = run([(OWN_SIDE, 0, welds[n], welds[o], Z, Z) for o in C.OFFSET_OTHERS
                        for n in C.OFFSET_WELDS]).reshape(data["offsets"].shape)
        default_mask = run([(TO_STABLE_DEFAULT_MASK, d, welds[w], ZW, act[a], Z) for w, a, d, m in C.STABLE_CASES
                            if m == "all"]).reshape(-1, 10, 64)

    # ---- non-vacuity, on the reference's outputs alone ----
    for n, after in zip(C.REFERENCE_PAIRS, stepped):    # the reference's own RequiredTest, and something frozen
        assert (after == welds[n]).all() and welds[n][1:].any(), n
    cases = {c: s for c, s in zip(C.STABLE_CASES, data["stable"])}
    static = {n: s for n, s in zip(names, data["stable0"])}
    assert (cases[("eater", "glider", 40, "all")] != static["eater"]).any()
    assert (cases[("eater", "glider", 0, "all")] == static["eater"]).all()
    assert (cases[("eater", "glider", 40, "all")] != cases[("eater", "glider", 8, "all")]).any()
    assert (cases[("eater", "glider", 40, "half")] != cases[("eater", "glider", 40, "all")]).any()
    assert (default_mask == np.stack([s for c, s in cases.items() if c[3] == "all"])).all()
    differs = [(n, o) for i, o in enumerate(C.OFFSET_OTHERS) for j, n in enumerate(C.OFFSET_WELDS)
               if (own_side[i, j] != data["offsets"][i, j]).any()]
    assert differs, "no pair tells the reference's masks from the own-side formula"
    state_pops = [int(np.unpackbits(w[0].view(np.uint8)).sum()) for w in welds.values()]

    path = os.path.join(HERE, "weld_family.npz")
    np.savez_compressed(path, **data)
    size = os.path.getsize(path)
    assert size <= 512 << 10, size
    print(f"{path}: {size} bytes; {len(pairs)} pairs, {len(welds)} welds (states of {min(state_pops)}..{max(state_pops)} "
          f"cells), {len(C.STABLE_CASES)} ToStable cases, {data['offsets'].shape[0] * data['offsets'].shape[1]} "
          f"InteractionOffsets pairs of which {len(differs)} show the masking oddity")


if __name__ == "__main__":
    main()
