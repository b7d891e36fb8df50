"""Records tests/golden/stable_complete.npz: the reference's own
LifeStable::CompleteStable (LifeStable.hpp:1340-1458) and LifeWeld::UnweldableMask
(LifeWeld.hpp:247-277) on the inputs that tests/stable_complete_cases.py builds.
CPU only; run from the repository root where the reference's headers are:

    python tests/golden/make_stable_complete_golden.py [--ref DIR]

stable_complete_ref_shim.cpp is compiled against those headers where they lie,
into a temporary directory, with the flags of make_stable_test_golden.py.  Only
data is stored.  The shim runs CompleteStable(1e9f, ...) and, beside it, the same
search spelled out over the reference's own members with a node counter and a
node budget; without a budget the two must agree or the shim fails, so the node
counts, stack depths and budget-limited results below are the reference's own
search's, and the reference's clock is never read.

The family is drawn (stable_complete_cases.DRAWN objects), run in the four flag
combinations (index f = minimise | use_seed << 1), classified on those outputs
alone, and PER_CLASS objects of each class are kept, the cheapest first (four of
the classes `long`, at least 128 nodes in some combination, and `deep`, at least 16 frames).  Caps,
which are conditions and not measurements: every kept object runs at most 4096
nodes and 32 frames in all four combinations; the recorder fails if a class
cannot be filled within them.

  kept       (K,)          indices into the family
  head       (K, 4, 8)     per combination: result (0 COMPLETED, 1 INCONSISTENT, 2 TIMEOUT),
                           nodes, deepest stack, search-area rounds, population the rounds
                           found (before the minimise pass), 1 if the reference defines the
                           call (0: unknown within state.ZOI(), where the spelled-out search
                           runs one step: not compared with CompleteStable), frames popped,
                           most ZOI growths of the seed at one node
  best       (K, 4, 64)    the completion ^ the input's state plane where COMPLETED, else 0
  budgets    (K, 4, 4)     the budgets run: 1, nodes - 1 (1 where that is 0), nodes, nodes + 1
  bhead      (K, 4, 4, 2)  per budget: result, nodes
  bbest      (K, 4, 4, 64) per budget: the completion ^ state where COMPLETED, else 0
  classes    (K,)          bit c set: object in class CLASSES[c]
  weld_a, weld_b (P, 4, 64)   the catalyst pairs of stable_complete_cases.WELD_CASES as
                           LifeWeld::FromRequired made them
  weld_mask, weld_tested (P, 64)   UnweldableMask at WELD_BUDGET nodes per placement, and the
                           placements searched
  weld_counts (P, 3)       placements COMPLETED / INCONSISTENT / TIMEOUT
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

import stable_complete_cases as C  # noqa: E402
from make_match_golden import CXX, XXH_DIR  # noqa: E402

MAX_NODES, MAX_FRAMES, PER_CLASS, NEED = 4096, 32, 10, 8
CLASSES = ("depth0", "backtracked", "bad_root", "bad_tree", "rounds2", "minimise_improves", "seed3",
           "column_seam", "row_seam", "within_zoi", "long", "deep")
FEWER = {"long": 4, "deep": 4}      # (their searches are what the tests' time goes to)


def compile_shim(ref, tmp):
    os.makedirs(os.path.join(tmp, "inc", "xxHash"))
    os.symlink(os.path.join(XXH_DIR, "xxhash.h"), os.path.join(tmp, "inc", "xxHash", "xxhash.h"))
    exe = os.path.join(tmp, "stable_complete_ref_shim")
    lib = os.path.join(ROOT, "lifeapi_amd")
    pre = [x for h in ("span", "stdexcept", "type_traits", "array", "utility", "cstdio") for x in ("-include", h)]
    subprocess.run([CXX, "-std=c++20", "-O2", "-march=x86-64-v3", "-pthread", "-Wno-nonportable-include-path",
                    "-Wno-undefined-inline", *pre, "-include", os.path.join(ROOT, "oracle", "ref_prelude.hpp"),
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(tmp, "inc"), "-I" + ref,
                    os.path.join(HERE, "stable_complete_ref_shim.cpp"), "-o", exe, "-L" + lib, "-llifeapi_hip",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def shim(exe, tmp, mode, rec):
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([len(rec)], np.uint64).tobytes())
        f.write(np.ascontiguousarray(rec, np.uint64).tobytes())
    subprocess.run([exe, str(mode), fin, fout], check=True, timeout=3000)
    return np.fromfile(fout, np.uint64).reshape(len(rec), -1)


def search(exe, tmp, planes, seeds, flags, budgets, cap):
    """the spelled-out search of every object: (head (n, 8), best (n, 64))"""
    n = len(planes)
    extra = np.stack([np.full(n, flags, np.uint64), np.asarray(budgets, np.uint64), np.full(n, cap, np.uint64)], axis=1)
    out = shim(exe, tmp, 0, np.concatenate([planes.reshape(n, 640), seeds, extra], axis=1))
    return out[:, :8].astype(np.int64), out[:, 8:]


def pop(w):
    return np.unpackbits(np.ascontiguousarray(w, "<u8").view(np.uint8), axis=-1).sum(axis=-1)


def classify(head, best, infos):
    h0, h1, h2 = head[:, 0], head[:, 1], head[:, 2]
    return np.stack([
        (h0[:, 0] == 0) & (h0[:, 2] == 0),
        (h0[:, 0] == 0) & (h0[:, 6] > 0),
        (h0[:, 0] == 1) & (h0[:, 2] == 0),
        (h0[:, 0] == 1) & (h0[:, 2] > 0),
        h0[:, 3] > 1,
        (h1[:, 0] == 0) & (h1[:, 4] > 0) & (pop(best[:, 1]) < h1[:, 4]),
        h2[:, 7] >= 3,
        np.array([i["column_seam"] for i in infos]),
        np.array([i["row_seam"] for i in infos]),
        h0[:, 5] == 0,
        head[:, :, 1].max(axis=1) >= 128,
        h0[:, 2] >= 16,
    ], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    planes, seeds, infos = C.build(range(C.DRAWN))
    from oracle.oracle import Port
    welds_in = C.weld_inputs(Port())
    with tempfile.TemporaryDirectory() as tmp:
        exe = compile_shim(args.ref, tmp)
        runs = [search(exe, tmp, planes, seeds, f, np.zeros(C.DRAWN), MAX_NODES + 1) for f in range(4)]
        head, best = np.stack([r[0] for r in runs], axis=1), np.stack([r[1] for r in runs], axis=1)
        ok = ((head[:, :, 0] != 5) & (head[:, :, 1] <= MAX_NODES) & (head[:, :, 2] <= MAX_FRAMES)).all(axis=1)
        cls = classify(head, best, infos) & ok[:, None]
        cost = head[:, :, 1].sum(axis=1)
        print("drawn", C.DRAWN, "within the caps", int(ok.sum()), {n: int(cls[:, c].sum()) for c, n in enumerate(CLASSES)})
        kept = []
        for c, name in enumerate(CLASSES):
            members = np.flatnonzero(cls[:, c])
            assert len(members) >= FEWER.get(name, NEED), f"class {name}: {len(members)} objects within the caps; widen the family"
            kept += [int(i) for i in members[np.argsort(cost[members], kind="stable")][:FEWER.get(name, PER_CLASS)]]
        kept = np.array(sorted(set(kept)), np.int32)
        k = len(kept)
        nodes = head[kept][:, :, 1]
        budgets = np.stack([np.ones_like(nodes), np.maximum(nodes - 1, 1), nodes, nodes + 1], axis=2)     # (k, 4, 4)
        bhead, bbest = np.zeros((k, 4, 4, 2), np.int64), np.zeros((k, 4, 4, 64), np.uint64)
        for f in range(4):
            for b in range(4):
                h, w = search(exe, tmp, planes[kept], seeds[kept], f, budgets[:, f, b], 1 << 40)
                bhead[:, f, b], bbest[:, f, b] = h[:, :2], w
        wrec = np.stack([np.concatenate(list(w) + [np.array([C.WELD_BUDGET], np.uint64)]) for w in welds_in])
        wout = shim(exe, tmp, 1, wrec)
    state = planes[kept][:, 0]
    done = head[kept][:, :, 0] == 0
    bdone = bhead[:, :, :, 0] == 0
    data = {"kept": kept, "head": head[kept].astype(np.int32),
            "best": np.where(done[:, :, None], best[kept] ^ state[:, None], 0).astype(np.uint64),
            "budgets": budgets.astype(np.int32), "bhead": bhead.astype(np.int32),
            "bbest": np.where(bdone[..., None], bbest ^ state[:, None, None], 0).astype(np.uint64),
            "classes": (cls[kept] << np.arange(len(CLASSES))).sum(axis=1).astype(np.int32),
            "weld_a": wout[:, :256].reshape(-1, 4, 64), "weld_b": wout[:, 256:512].reshape(-1, 4, 64),
            "weld_mask": wout[:, 512:576], "weld_tested": wout[:, 576:640], "weld_counts": wout[:, 640:643].astype(np.int32)}

    # ---- non-vacuity, on the reference's outputs alone, on the kept set ----
    assert not np.where(~done[:, :, None], best[kept], 0).any() and not np.where(~bdone[..., None], bbest, 0).any()
    for c, name in enumerate(CLASSES):
        assert int(cls[kept][:, c].sum()) >= FEWER.get(name, NEED), name
    assert (head[kept][:, :, 1] <= MAX_NODES).all() and (head[kept][:, :, 2] <= MAX_FRAMES).all()
    # the budgets bite: at nodes - 1 some runs time out and some still complete on an earlier find
    at = bhead[:, :, 1, 0][nodes > 1]
    assert (at == 2).sum() >= 8 and (at == 0).sum() >= 8, np.bincount(at)
    assert (bhead[:, :, 2:, 0] == head[kept][:, :, None, 0]).all() and (bhead[:, :, 2:, 1] == nodes[:, :, None]).all()
    wc = data["weld_counts"]
    assert (pop(data["weld_tested"]) <= 64).all() and (wc.sum(axis=1) >= 16).all(), wc
    assert (wc[:, 1] > 0).all() and (wc[:, 2] > 0).all() and (wc[:, 0] > 0).sum() >= 2, wc

    path = os.path.join(HERE, "stable_complete.npz")
    np.savez_compressed(path, **data)
    size = os.path.getsize(path)
    assert size <= os.path.getsize(os.path.join(HERE, "stable.npz")), size
    print(f"{path}: {size} bytes; kept {k}: " + ", ".join(f"{n} {int(cls[kept][:, c].sum())}" for c, n in enumerate(CLASSES))
          + f"; nodes up to {nodes.max()}, frames up to {head[kept][:, :, 2].max()}; welds {wc.tolist()}")


if __name__ == "__main__":
    main()
