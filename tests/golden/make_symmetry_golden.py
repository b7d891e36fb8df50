"""Records tests/golden/symmetry.npz: the reference's own Transform / Moved,
Symmetricize, XYBounds, SymmetryOrbit and SymmetryOrbitRepresentatives
(Symmetry.hpp:105-173, 565-654, 798-830, LifeAPI.hpp:446-484, 682-735) on the
inputs that tests/test_symmetry_model.py builds.  CPU only; run from the
repository root where the reference's headers are:

    python tests/golden/make_symmetry_golden.py [--ref DIR] [--only-sweeps]

--only-sweeps records tests/golden/symmetry_sweeps.npz alone (the shift,
offset, bounding-box and stabiliser sweeps) and leaves symmetry.npz as it is.
symmetry_ref_shim.cpp is compiled against those headers where they lie, into a
temporary directory, with the flags of make_match_golden.py.  Only data is
stored: the reference's outputs and the moved orbit inputs; the seeded random
states are regenerated from Port.fill.  Non-vacuity is asserted on the
reference's outputs alone, before anything is written.
"""
import argparse
import itertools
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_symmetry_model as M  # noqa: E402
from make_match_golden import CXX, XXH_DIR  # noqa: E402
from oracle.oracle import Port  # noqa: E402

TRANSFORM, SYMMETRICIZE, ORBIT = 0, 1, 2
ORBIT_WORDS = 64 + 4 + 8 * 64 + 1


def compile_shim(ref, tmp):
    os.makedirs(os.path.join(tmp, "inc", "xxHash"))
    os.symlink(os.path.join(XXH_DIR, "xxhash.h"), os.path.join(tmp, "inc", "xxHash", "xxhash.h"))
    exe = os.path.join(tmp, "symmetry_ref_shim")
    lib = os.path.join(ROOT, "lifeapi_amd")
    pre = [x for h in ("span", "stdexcept", "type_traits", "array", "utility", "cstdio") for x in ("-include", h)]
    subprocess.run([CXX, "-std=c++20", "-O2", "-march=x86-64-v3", "-pthread", "-Wno-nonportable-include-path",
                    "-Wno-undefined-inline", *pre, "-include", os.path.join(ROOT, "oracle", "ref_prelude.hpp"),
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(tmp, "inc"), "-I" + ref,
                    os.path.join(HERE, "symmetry_ref_shim.cpp"), "-o", exe, "-L" + lib, "-llifeapi_hip",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def reference(exe, tmp, ops):
    """ops: (kind, a, b, c, state); the shim's output per op, as uint64 words"""
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([len(ops)], np.uint64).tobytes())
        for kind, a, b, c, state in ops:
            f.write(np.array([kind, a, b, c], np.int64).tobytes())
            f.write(np.ascontiguousarray(state, np.uint64).tobytes())
    subprocess.run([exe, fin, fout], check=True)
    out, res, at = np.fromfile(fout, np.uint64), [], 0
    for kind, *_ in ops:
        k = ORBIT_WORDS if kind == ORBIT else 64
        res.append(out[at:at + k])
        at += k
    assert at == out.size
    return res


def distinct(arrays):
    return all((a != b).any() for a, b in itertools.combinations(arrays, 2))


def record_sweeps(ref, port):
    """tests/golden/symmetry_sweeps.npz: the reference on the sweeps of
    tests/test_symmetry_model.py.  Landing coordinates, bounds, masks and
    images of a few cells: all of it compresses to little."""
    syms = list(M.SYMMETRIES.values())
    r5, pairs, states = M.symmetricize_states(port)[0], M.pair_states(), M.orbit_sweep_states()
    with tempfile.TemporaryDirectory() as tmp:
        exe = compile_shim(ref, tmp)
        moved = reference(exe, tmp, [(TRANSFORM, t, dx, dy, M.cell(*M.SWEEP_CELL)) for t in range(16)
                                     for dx, dy in M.SHIFTS])
        landing = np.array([M.where(s) for s in moved], np.uint8).reshape(16, len(M.SHIFTS), 2)
        sy = np.stack(reference(exe, tmp, [(SYMMETRICIZE, y, dx, dy, r5) for y in syms for dx, dy in M.SYM_SWEEP]))
        sy = sy.reshape(len(syms), len(M.SYM_SWEEP), 64)
        po = np.stack(reference(exe, tmp, [(ORBIT, 0, 0, 0, s) for s in pairs]))
        so = np.stack(reference(exe, tmp, [(ORBIT, 0, 0, 0, s) for s in states]))
    assert (po[:, :64] == pairs).all() and (so[:, :64] == states).all()
    pair_bounds, pair_mask = po[:, 64:68].view(np.int64).astype(np.int8), po[:, -1].astype(np.uint8)
    orbit_bounds, orbit_mask = so[:, 64:68].view(np.int64).astype(np.int8), so[:, -1].astype(np.uint8)
    orbit_images = so[:, 68:68 + 512].reshape(len(states), 8, 64)

    # ---- non-vacuity, on the reference's outputs alone ----
    at = 0
    for name, sweep in M.SHIFT_SWEEPS.items():   # every residue of a sweep lands the cell somewhere else
        for t in range(16):
            assert len({tuple(c) for c in landing[t, at:at + 64].tolist()}) == 64, (name, M.TRANSFORMS[t])
        at += 64
    c1 = syms.index(M.SYMMETRIES["C1"])
    for k in range(len(syms)):
        for part in (sy[k, :141], sy[k, 141:]):   # a line's offsets matter (D4diag halves them: 32 results)
            assert k == c1 or len({p.tobytes() for p in part}) >= 32, syms[k]
    stab = orbit_mask[:3 * len(M.SUBGROUPS) + len(syms)]
    assert set(M.STABILISER_MASKS) <= set(stab.tolist()), sorted(set(stab.tolist()))
    assert len({tuple(b) for b in pair_bounds.tolist()}) >= 4000
    assert (orbit_mask[-2:] == 0xFF).all() and (orbit_bounds[-2:] == (-20, -20, 19, 19)).all()

    path = os.path.join(HERE, "symmetry_sweeps.npz")
    np.savez_compressed(path, shift_landing=landing, symmetricize_sweep=sy, pair_bounds=pair_bounds,
                        pair_mask=pair_mask, orbit_bounds=orbit_bounds, orbit_mask=orbit_mask,
                        orbit_images=orbit_images)
    size = os.path.getsize(path)
    assert size <= 512 << 10, size
    print(f"{path}: {size} bytes; 16 transforms x {len(M.SHIFTS)} shifts, {len(syms)} symmetries x "
          f"{len(M.SYM_SWEEP)} offsets, {len(pairs)} pairs, {len(states)} orbits; pair masks "
          f"{sorted(set(pair_mask.tolist()))}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--only-sweeps", action="store_true", help="record symmetry_sweeps.npz alone")
    args = ap.parse_args()
    port = Port()
    record_sweeps(args.ref, port)
    if args.only_sweeps:
        return
    ts, ss, bases = M.transform_states(port), M.symmetricize_states(port), M.orbit_bases(port)
    syms = list(M.SYMMETRIES.values())
    with tempfile.TemporaryDirectory() as tmp:
        exe = compile_shim(args.ref, tmp)
        tr = np.stack(reference(exe, tmp, [(TRANSFORM, t, 0, 0, s) for t in range(16) for s in ts]))
        tr = tr.reshape(16, len(ts), 64)
        tm = np.stack(reference(exe, tmp, [(TRANSFORM, t, dx, dy, s) for t in range(16) for dx, dy in M.MOVES
                                           for s in ts[:2]])).reshape(16, len(M.MOVES), 2, 64)

        def symm(offsets):
            r = reference(exe, tmp, [(SYMMETRICIZE, y, dx, dy, s) for y in syms for s in ss for dx, dy in offsets])
            return np.stack(r).reshape(len(syms), len(ss), len(offsets), 64)
        sy = symm(M.OFFSETS)
        sy_x, sy_y = symm([(dx + 1, dy) for dx, dy in M.OFFSETS]), symm([(dx, dy + 1) for dx, dy in M.OFFSETS])
        ob = np.stack(reference(exe, tmp, [(ORBIT, 0, dx, dy, s) for s in bases for dx, dy in M.ORBIT_MOVES]))
    ob = ob.reshape(len(bases), len(M.ORBIT_MOVES), ORBIT_WORDS)
    orbit_states, bounds = ob[..., :64], ob[..., 64:68].view(np.int64).astype(np.int32)
    images, masks = ob[..., 68:68 + 512].reshape(len(bases), len(M.ORBIT_MOVES), 8, 64), ob[..., -1].astype(np.uint8)

    # ---- non-vacuity, on the reference's outputs alone ----
    for k in range(M.N_RANDOM):
        assert distinct(tr[:, k]), f"transforms of random state {k} coincide"
    assert distinct(tr[:, M.N_RANDOM + M.CELLS.index((17, 42))])
    # every listed move changes the result, but the whole turn (64, -64), which the reference wraps away
    for t in range(16):
        for m, (dx, dy) in enumerate(M.MOVES):
            whole = dx % 64 == 0 and dy % 64 == 0
            assert ((tm[t, m] != tr[t, :2]).any(axis=1) != whole).all(), (t, dx, dy)
    c1 = syms.index(M.SYMMETRIES["C1"])
    for i in range(len(ss)):
        for o in range(len(M.OFFSETS)):
            assert distinct([sy[k, i, o] for k in range(len(syms))]), (i, M.OFFSETS[o])
            for k in range(len(syms)):
                changed = (sy_x[k, i, o] != sy[k, i, o]).any(), (sy_y[k, i, o] != sy[k, i, o]).any()
                assert changed == ((False, False) if k == c1 else (True, True)), (syms[k], i, M.OFFSETS[o], changed)
    for k in range(len(syms)):   # and every listed offset gives another result
        for i in range(len(ss)):
            assert k == c1 or distinct(list(sy[k, i])), (syms[k], i)
    mset = set(masks.ravel().tolist())
    assert len(mset) >= 8 and {0x01, 0xFF, 0x07, 0x7F} <= mset, sorted(mset)
    assert any(k & (k >> 1) != k >> 1 for k in mset)
    assert (bounds[M.ORBIT_NAMES.index("empty")] == -1).all()
    # a seam case: the pattern straddles the window's edge, where the reference reports the whole window
    # (top -32, bottom 31, never top > bottom) although few rows are populated
    rows = np.bitwise_or.reduce(orbit_states, axis=-1)
    assert any(b[1] == -32 and b[3] == 31 and bin(int(r)).count("1") < 8
               for b, r in zip(bounds.reshape(-1, 4), rows.ravel())), "no seam case"
    p, m = M.ORBIT_NAMES.index("block"), M.ORBIT_MOVES.index((30, 31))
    assert tuple(bounds[p, m]) == (30, -32, 31, 31) and bin(masks[p, m]).count("1") == 3
    assert bin(masks[M.ORBIT_NAMES.index("L3"), m]).count("1") == 7

    path = os.path.join(HERE, "symmetry.npz")
    np.savez_compressed(path, transform=tr, transform_move=tm, symmetricize=sy, orbit_states=orbit_states,
                        bounds=bounds, orbit_images=images, orbit_mask=masks)
    size = os.path.getsize(path)
    assert size <= 512 << 10, size
    print(f"{path}: {size} bytes; 16 transforms x {len(ts)} states, x {len(M.MOVES)} moves x 2, {len(syms)} symmetries "
          f"x {len(ss)} x {len(M.OFFSETS)} offsets, {len(bases)} x {len(M.ORBIT_MOVES)} orbits; masks {sorted(mset)}")


if __name__ == "__main__":
    main()
