"""Records tests/golden/pair.npz: the reference's own IntersectingOffsets
(Symmetry.hpp:729-772), a.Convolve(b.Transformed(t)) (LifeAPI.hpp:1293-1370),
Halve / HalveX / HalveY and Skew / InvSkew (Symmetry.hpp:681-727) on the
inputs that tests/test_pair_model.py builds.  CPU only; run from the
repository root where the reference's headers are:

    python tests/golden/make_pair_golden.py [--ref DIR]

pair_ref_shim.cpp is compiled against those headers where they lie, into a
temporary directory, with the flags of make_match_golden.py.  Only data is
stored: the reference's outputs (the residue sweep as landing coordinates);
every input is regenerated from Port.fill seeds and the builders of the
model's file.  Non-vacuity is asserted on the reference's outputs alone,
before anything is written.
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

import test_pair_model as P  # noqa: E402
import test_symmetry_model as M  # noqa: E402
from make_match_golden import CXX, XXH_DIR  # noqa: E402
from oracle.oracle import Port  # noqa: E402

INTERSECTING, CONVOLVE, HALVE, SKEW = 0, 1, 2, 3


def compile_shim(ref, tmp):
    os.makedirs(os.path.join(tmp, "inc", "xxHash"))
    os.symlink(os.path.join(XXH_DIR, "xxhash.h"), os.path.join(tmp, "inc", "xxHash", "xxhash.h"))
    exe = os.path.join(tmp, "pair_ref_shim")
    lib = os.path.join(ROOT, "lifeapi_amd")
    pre = [x for h in ("span", "stdexcept", "type_traits", "array", "utility", "cstdio") for x in ("-include", h)]
    subprocess.run([CXX, "-std=c++20", "-O2", "-march=x86-64-v3", "-pthread", "-Wno-nonportable-include-path",
                    "-Wno-undefined-inline", *pre, "-include", os.path.join(ROOT, "oracle", "ref_prelude.hpp"),
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(tmp, "inc"), "-I" + ref,
                    os.path.join(HERE, "pair_ref_shim.cpp"), "-o", exe, "-L" + lib, "-llifeapi_hip",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def reference(exe, tmp, ops):
    """ops: (kind, arg, a, b); the shim's 64 words per op"""
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    zero = np.zeros(64, np.uint64)
    with open(fin, "wb") as f:
        f.write(np.array([len(ops)], np.uint64).tobytes())
        for kind, arg, a, b in ops:
            f.write(np.array([kind, arg], np.int64).tobytes())
            f.write(np.ascontiguousarray(a, np.uint64).tobytes())
            f.write(np.ascontiguousarray(zero if b is None else b, np.uint64).tobytes())
    subprocess.run([exe, fin, fout], check=True)
    out = np.fromfile(fout, np.uint64).reshape(-1, 64)
    assert len(out) == len(ops)
    return out


def pops(states):
    return np.unpackbits(np.ascontiguousarray(states, np.uint64).view(np.uint8).reshape(len(states), -1), axis=1).sum(axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    port = Port()
    syms = [P.IO_VALUES[s] for s in P.IO_SYMS]
    p1, p2 = P.sparse_pairs()
    cases, hs, (qa, qb) = P.choice_cases(port), P.halve_states(port), P.pair16()
    pat2 = M.cells([P.RESIDUE_PAT2])
    with tempfile.TemporaryDirectory() as tmp:
        exe = compile_shim(args.ref, tmp)
        res = reference(exe, tmp, [(INTERSECTING, y, s, pat2) for y in syms for s in P.residue_states()])
        pairs = reference(exe, tmp, [(INTERSECTING, y, a, b) for y in syms for a, b in zip(p1, p2)])
        selfs = reference(exe, tmp, [(INTERSECTING, y, a, a) for y in syms for a in p1])
        swapped = reference(exe, tmp, [(INTERSECTING, P.IO_VALUES["C4"], b, a) for a, b in zip(p1, p2)])
        # pat2.Convolve(pat1.Transformed(wrong)), for the non-vacuity checks alone
        wrong = {(s, w): reference(exe, tmp, [(CONVOLVE, M.T[w], b, a) for a, b in zip(p1, p2)])
                 for s, ws in P.IO_WRONG.items() for w in ws}
        choice = reference(exe, tmp, [(INTERSECTING, y, *ab) for y in syms for _, x, z in cases
                                      for ab in ((x, z), (z, x))])
        halve = reference(exe, tmp, [(HALVE, m, s, None) for m in range(3) for s in hs])
        skew = reference(exe, tmp, [(SKEW, i, s, None) for i in range(2) for s in hs])
        conv = reference(exe, tmp, [(CONVOLVE, t, a, b) for t in range(16) for a, b in zip(qa, qb)])
    res, pairs, selfs = (v.reshape(len(syms), -1, 64) for v in (res, pairs, selfs))
    choice = choice.reshape(len(syms), len(cases), 2, 64)
    halve, skew, conv = halve.reshape(3, -1, 64), skew.reshape(2, -1, 64), conv.reshape(16, -1, 64)

    # ---- non-vacuity, on the reference's outputs alone ----
    assert (pops(res.reshape(-1, 64)) == 1).all()                      # one cell against one cell: one cell
    landing = np.array([M.where(s) for s in res.reshape(-1, 64)], np.uint8).reshape(len(syms), 192, 2)
    for k, s in enumerate(P.IO_SYMS):
        for line in range(3):                                             # every residue lands somewhere else
            assert len({tuple(c) for c in landing[k, 64 * line:64 * line + 64].tolist()}) == 64, (s, line)
    for v in (pairs, selfs):
        n = pops(v.reshape(-1, 64))
        assert n.min() >= 1 and n.max() <= 576, (n.min(), n.max())       # k x k cells: at most k^2 sums
    k4 = P.IO_SYMS.index("C4")
    assert (swapped != pairs[k4]).any(axis=1).sum() >= 30
    for (s, w), v in wrong.items():
        differ = (v != pairs[P.IO_SYMS.index(s)]).any(axis=1).sum()
        assert differ >= 30, (s, w, differ)
    names = [c[0] for c in cases]
    for i, name in enumerate(names):
        n = pops(choice[:, i].reshape(-1, 64))
        assert (n == 0).all() if "empty" in name else (n > 0).all(), name
    assert (pops(choice[:, names.index("full column")].reshape(-1, 64)) >= 64 * 3).all()
    for t in range(16):
        for u in range(t):
            assert (conv[t] != conv[u]).any(), (t, u)
    assert (halve[:, :8] != halve[:, :8][[1, 2, 0]]).any(axis=(1, 2)).all()
    assert (skew[0] != skew[1]).any(axis=1).sum() >= 130

    path = os.path.join(HERE, "pair.npz")
    np.savez_compressed(path, residue_landing=landing, sparse_pairs=pairs, sparse_self=selfs, choice=choice,
                        halve=halve, skew=skew, convolve_pair=conv)
    size = os.path.getsize(path)
    assert size <= 256 << 10, size
    print(f"{path}: {size} bytes; {len(syms)} symmetries x (192 residues, {len(p1)} pairs and self-pairs, "
          f"{len(cases)} x 2 operand-choice cases), {len(hs)} states x 5, 16 transforms x {len(qa)} pairs")


if __name__ == "__main__":
    main()
