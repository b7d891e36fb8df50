"""Records tests/golden/components.npz: the reference's own FirstOn,
ComponentContaining and Components (LifeAPI.hpp:301-323, 655-676, 1184-1193) on
the inputs that tests/components_cases.py builds.  CPU only; run from the
repository root where the reference's headers are:

    python tests/golden/make_components_golden.py [--ref DIR]

components_ref_shim.cpp is compiled against those headers where they lie, into
a temporary directory, with the flags of make_symmetry_golden.py.  Only data is
stored: the reference's outputs; the inputs are rebuilt by components_cases.py.
Non-vacuity is asserted on the reference's outputs alone, before anything is
written.

  first_on        (states, 2) int32, every state in components_cases.states' order
  count_<corona>  int32 per state: all states for "default", other_corona_names
                  for the other coronas holding (0, 0)
  comp_<corona>   the components of those states one after the other, (sum, 64)
  cc              (corona, state, seed kind, 64): ComponentContaining on
                  CC_STATES x SEED_KINDS with every corona of CORONAS
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

import components_cases as C  # noqa: E402
from make_match_golden import CXX, XXH_DIR  # noqa: E402
from oracle.oracle import Port  # noqa: E402

FIRST_ON, CONTAINING, CONTAINING_DEFAULT, COMPONENTS = range(4)
ZERO = np.zeros(64, np.uint64)


def compile_shim(ref, tmp):
    os.makedirs(os.path.join(tmp, "inc", "xxHash"))
    os.symlink(os.path.join(XXH_DIR, "xxhash.h"), os.path.join(tmp, "inc", "xxHash", "xxhash.h"))
    exe = os.path.join(tmp, "components_ref_shim")
    lib = os.path.join(ROOT, "lifeapi_amd")
    pre = [x for h in ("span", "stdexcept", "type_traits", "array", "utility", "cstdio") for x in ("-include", h)]
    subprocess.run([CXX, "-std=c++20", "-O2", "-march=x86-64-v3", "-pthread", "-Wno-nonportable-include-path",
                    "-Wno-undefined-inline", *pre, "-include", os.path.join(ROOT, "oracle", "ref_prelude.hpp"),
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(tmp, "inc"), "-I" + ref,
                    os.path.join(HERE, "components_ref_shim.cpp"), "-o", exe, "-L" + lib, "-llifeapi_hip",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def reference(exe, tmp, ops):
    """ops: (kind, state, seed, corona); the shim's output per op, as uint64 words"""
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([len(ops)], np.uint64).tobytes())
        for kind, state, seed, corona in ops:
            f.write(np.array([kind], np.int64).tobytes())
            for a in (state, seed, corona):
                f.write(np.ascontiguousarray(a, np.uint64).tobytes())
    subprocess.run([exe, fin, fout], check=True, timeout=600)
    out, res, at = np.fromfile(fout, np.uint64), [], 0
    for kind, *_ in ops:
        k = 2 if kind == FIRST_ON else 64 if kind in (CONTAINING, CONTAINING_DEFAULT) else 1 + 64 * int(out[at])
        res.append(out[at:at + k])
        at += k
    assert at == out.size
    return res


def cells_of(component):
    return C.to_cells(component)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    states = C.states(Port())
    names = list(states)
    others = C.other_corona_names(states)
    data = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = compile_shim(args.ref, tmp)
        fo = reference(exe, tmp, [(FIRST_ON, s, ZERO, ZERO) for s in states.values()])
        data["first_on"] = np.stack(fo).view(np.int64).astype(np.int32)
        parts = {}
        for corona in C.COMPONENTS_CORONAS:
            use = names if corona == "default" else others
            r = reference(exe, tmp, [(COMPONENTS, states[n], ZERO, C.CORONAS[corona]) for n in use])
            data["count_" + corona] = np.array([int(x[0]) for x in r], np.int32)
            data["comp_" + corona] = np.concatenate([x[1:] for x in r]).reshape(-1, 64)
            parts[corona] = {n: x[1:].reshape(-1, 64) for n, x in zip(use, r)}
        seeds = {n: C.seeds_for(states[n]) for n in C.CC_STATES}
        ops = [(CONTAINING, states[n], seeds[n][k], C.CORONAS[corona])
               for corona in C.CORONAS for n in C.CC_STATES for k in C.SEED_KINDS]
        cc = np.stack(reference(exe, tmp, ops)).reshape(len(C.CORONAS), len(C.CC_STATES), len(C.SEED_KINDS), 64)
        data["cc"] = cc
        singles = np.stack(reference(exe, tmp, [(CONTAINING, states[n], one, C.CORONAS["default"]) for n in C.CC_STATES
                                                for one in C.two_cells(states[n])])).reshape(len(C.CC_STATES), 2, 64)
        # The snapshot's ConstantParse (LifeAPI.hpp:1147-1148) does not advance on a
        # "$" without a count, so its default-argument overloads (LifeAPI.hpp:1184-1193)
        # see the five cells (-2..2, -2) in place of the 21 the RLE spells: this
        # pins that, which is why every "default" above is passed explicitly (and
        # why Components() is never called: without (0, 0) it does not terminate).
        row5 = C.from_cells([(a, -2) for a in range(-2, 3)])
        for n in C.CC_STATES:
            quirk = reference(exe, tmp, [(CONTAINING_DEFAULT, states[n], states[n], ZERO),
                                         (CONTAINING, states[n], states[n], row5)])
            assert (quirk[0] == quirk[1]).all(), n

    # ---- non-vacuity, on the reference's outputs alone ----
    count = {c: dict(zip(names if c == "default" else others, data["count_" + c].tolist())) for c in C.COMPONENTS_CORONAS}
    d = count["default"]
    for p in C.PAIR_BASES:
        for a, b in C.PAIR_OFFSETS:   # every offset counts: one piece exactly on the corona's 21 cells
            n = f"pair_{p[0]}_{a}_{b}"
            assert d[n] == (1 if (a, b) in C.DEFAULT_CELLS else 2), (n, d[n])
            if max(abs(a), abs(b)) == 3:   # the 7 x 7 solid joins what the default leaves apart
                assert count["7x7"][n] == 1 and d[n] == 2, n
    lattice = parts["default"]["lattice512"]
    assert d["lattice512"] == 512 and [cells_of(c) for c in lattice[:3]] == [[(60, 0)], [(60, 4)], [(60, 8)]]
    assert [cells_of(c)[0] for c in parts["default"]["six_cells"]] == [(60, 3), (62, 0), (33, 33), (1, 9)]
    assert tuple(data["first_on"][names.index("quad0")]) == (1, 40) and tuple(data["first_on"][names.index("empty")]) == (-1, -1)
    assert d["empty"] == 0 and d["spiral"] == 1 and d["spiral_cut"] == 2 and d["staircase"] == 2
    assert d["full_row"] == d["full_col"] == 1 and d["row_and_col"] == 2 and d["comb"] == 1
    soup = [d[n] for n in names if n.startswith("soup")]
    assert min(soup) <= 3 and max(soup) >= 100, (min(soup), max(soup))
    # the asymmetric coronas tell the axes and the directions apart
    # (FirstOn starts at (20, 30) for a = +-1, the later group of four for a = -1, and at the lower row for b = +-1)
    for corona, joined in (("right", {(1, 0)}), ("down", {(0, 1), (0, -1)})):
        for a, b in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            assert count[corona][f"pair_20_{a}_{b}"] == (1 if (a, b) in joined else 2), (corona, a, b)
    ck, cs = {k: i for i, k in enumerate(C.SEED_KINDS)}, list(C.CORONAS)
    dflt = cc[cs.index("default")]
    for i, n in enumerate(C.CC_STATES):
        assert not dflt[i, ck["far"]].any() and not dflt[i, ck["empty"]].any(), n
        assert (dflt[i, ck["state"]] == states[n]).all(), n
        for k in ("inside", "adjacent"):   # one whole component of the list
            assert any((dflt[i, ck[k]] == c).all() for c in parts["default"][n]), (n, k)
        assert (dflt[i, ck["two"]] == (singles[i, 0] | singles[i, 1])).all() and (singles[i, 0] != singles[i, 1]).any(), n
        assert not (dflt[i, ck["adjacent"]] & seeds[n]["adjacent"]).any(), n   # a seed outside the state stays outside
    assert not cc[cs.index("none")].any()
    lone = C.CC_STATES.index("pair_63_3_3")   # without its centre the corona drops a lone seed
    assert not cc[cs.index("no_centre"), lone, ck["inside"]].any() and dflt[lone, ck["inside"]].any()
    assert any((cc[cs.index(c)] != dflt).any() for c in ("3x3", "plus", "right", "down", "7x7", "no_centre"))

    path = os.path.join(HERE, "components.npz")
    np.savez_compressed(path, **data)
    size = os.path.getsize(path)
    assert size <= 512 << 10, size
    print(f"{path}: {size} bytes; {len(names)} states, soups {min(soup)}..{max(soup)} components, "
          + ", ".join(f"{c}: {int(data['count_' + c].sum())} components" for c in C.COMPONENTS_CORONAS))


if __name__ == "__main__":
    main()
