"""Records tests/golden/stable_test.npz: the reference's own LifeStable strip
passes (LifeStable.hpp:921-948, 995-1249), TestUnknowns (:1321-1338) and
PropagateAndTest (:163-184) on the inputs that tests/stable_test_cases.py
builds.  CPU only; run from the repository root where the reference's headers
are:

    python tests/golden/make_stable_test_golden.py [--ref DIR]

stable_test_ref_shim.cpp is compiled against those headers where they lie, into
a temporary directory, with the flags of make_weld_golden.py.  Only data is
stored: the reference's outputs, as XOR against the inputs, which
stable_test_cases.py rebuilds.  The family is drawn (stable_test_cases.DRAWN
objects), classified on the reference's outputs alone, at most 256 objects are
kept, and non-vacuity is asserted on the kept set before anything is written.

  kept         (K,)              indices into the family
  counts       (K, 8)            PropagateAndTest's flags, cells tested, forced on,
                                 forced off, changing Joins, inconsistent in
                                 TestUnknowns, inconsistent in Propagate, outer rounds
  pat, pat_flags   (K, 10, 64), (K,)   PropagateAndTest: planes ^ input, result
  tu, tu_flags     (K, 10, 64), (K,)   Propagate, then TestUnknowns(Vulnerable().ZOI())
  fresh        (K, 10, 64)       the object after PropagateStep(), UpdateOptions(), SignalNeighbours(),
                                 its state and unknown then PropagateAndTest's (options and
                                 cells nothing has synchronised yet), ^ input
  strip, strip_flags (K, 2, 8, 6, 10, 6), (K, 2, 8, 6)
                                 from the object as given and from the fresh one, the six
                                 strip passes at columns {0, 1, 2, 31, 61, 62, 63, the
                                 pattern's own}: columns x-2 .. x+3 of planes ^ start
                                 (nothing else changes: asserted here), result
  drawn_mean_tested  ()          mean cells tested per object over the whole family
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

import stable_test_cases as C  # noqa: E402
from make_match_golden import CXX, XXH_DIR  # noqa: E402

KEEP, PER_CLASS = 256, 20
NEED = {"forced_on": 8, "forced_off": 8, "joins": 8, "bad_test": 4, "bad_propagate": 4, "rounds3": 4, "straddles": 16}


def compile_shim(ref, tmp):
    os.makedirs(os.path.join(tmp, "inc", "xxHash"))
    os.symlink(os.path.join(XXH_DIR, "xxhash.h"), os.path.join(tmp, "inc", "xxHash", "xxhash.h"))
    exe = os.path.join(tmp, "stable_test_ref_shim")
    lib = os.path.join(ROOT, "lifeapi_amd")
    pre = [x for h in ("span", "stdexcept", "type_traits", "array", "utility", "cstdio") for x in ("-include", h)]
    subprocess.run([CXX, "-std=c++20", "-O2", "-march=x86-64-v3", "-pthread", "-Wno-nonportable-include-path",
                    "-Wno-undefined-inline", *pre, "-include", os.path.join(ROOT, "oracle", "ref_prelude.hpp"),
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(tmp, "inc"), "-I" + ref,
                    os.path.join(HERE, "stable_test_ref_shim.cpp"), "-o", exe, "-L" + lib, "-llifeapi_hip",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def reference(exe, tmp, mode, planes, columns):
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    rec = np.concatenate([planes.reshape(len(planes), 640), columns.astype(np.uint64)[:, None]], axis=1)
    with open(fin, "wb") as f:
        f.write(np.array([len(planes)], np.uint64).tobytes())
        f.write(np.ascontiguousarray(rec, np.uint64).tobytes())
    subprocess.run([exe, str(mode), fin, fout], check=True, timeout=600)
    return np.fromfile(fout, np.uint64).reshape(len(planes), -1)


def classes(counts, infos):
    c = counts.astype(np.int64)
    return {"forced_on": c[:, 2] > 0, "forced_off": c[:, 3] > 0, "joins": c[:, 4] > 0, "bad_test": c[:, 5] > 0,
            "bad_propagate": c[:, 6] > 0, "rounds3": c[:, 7] >= 3, "straddles": np.array([i["straddles"] for i in infos])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    assert C.DRAWN >= 2000
    planes, columns, infos = C.build(range(C.DRAWN))
    with tempfile.TemporaryDirectory() as tmp:
        exe = compile_shim(args.ref, tmp)
        counts = reference(exe, tmp, 0, planes, columns)
        assert counts.shape == (C.DRAWN, 8)
        cls = classes(counts, infos)
        kept = []
        for name in NEED:
            kept += [int(i) for i in np.flatnonzero(cls[name])[:PER_CLASS] if i not in kept]
        kept += [i for i in range(C.DRAWN) if i not in kept][:KEEP - len(kept)]
        kept = np.array(sorted(kept[:KEEP]), np.int32)
        rec = reference(exe, tmp, 1, planes[kept], columns[kept])
    k = len(kept)
    assert k <= KEEP and rec.shape == (k, 641 * 99)
    rec = rec.reshape(k, 99, 641)
    src = planes[kept].reshape(k, 640)
    data = {"kept": kept, "counts": counts[kept].astype(np.uint32),
            "pat": (rec[:, 0, :640] ^ src).reshape(k, 10, 64), "pat_flags": rec[:, 0, 640].astype(np.uint8),
            "tu": (rec[:, 1, :640] ^ src).reshape(k, 10, 64), "tu_flags": rec[:, 1, 640].astype(np.uint8),
            "drawn_mean_tested": np.float64(counts[:, 1].mean())}
    data["fresh"] = (rec[:, 2, :640] ^ src).reshape(k, 10, 64)
    start = np.stack([src, rec[:, 2, :640]], axis=1)                      # (k, 2, 640): as given, fresh
    diff = (rec[:, 3:, :640].reshape(k, 2, 48, 640) ^ start[:, :, None]).reshape(k, 2, 8, 6, 10, 64)
    xs = np.concatenate([np.tile(np.array(C.STRIP_COLUMNS), (k, 1)), columns[kept][:, None]], axis=1).astype(np.int64)
    cols = (xs[:, :, None] - 2 + np.arange(6)) % 64                       # (k, 8, 6)
    at = np.broadcast_to(cols[:, None, :, None, None, :], (k, 2, 8, 6, 10, 6))
    strip = np.take_along_axis(diff, at, axis=5)
    outside = diff.copy()
    np.put_along_axis(outside, at, 0, axis=5)
    assert not outside.any(), "a strip pass changed a column outside x-2 .. x+3"
    data["strip"], data["strip_flags"] = strip, rec[:, 3:, 640].reshape(k, 2, 8, 6).astype(np.uint8)
    for which in range(6):
        assert strip[:, :, :, which].any(), which

    # ---- non-vacuity, on the reference's outputs alone, on the kept set ----
    kc = classes(counts[kept], [infos[i] for i in kept])
    for name, need in NEED.items():
        assert int(kc[name].sum()) >= need, (name, int(kc[name].sum()), need)
    assert data["strip"].any() and (data["strip_flags"] == 0).any() and (data["strip_flags"] == 3).any()
    assert (data["pat_flags"] == 0).sum() >= 8 and (data["pat_flags"] == 3).any() and (data["tu_flags"] == 0).any()

    path = os.path.join(HERE, "stable_test.npz")
    np.savez_compressed(path, **data)
    size = os.path.getsize(path)
    assert size <= os.path.getsize(os.path.join(HERE, "stable.npz")), size
    tot = counts.astype(np.int64)
    print(f"{path}: {size} bytes; drawn {C.DRAWN}: cells tested {tot[:, 1].sum()} (mean {tot[:, 1].mean():.2f}), forced on "
          f"{tot[:, 2].sum()}, forced off {tot[:, 3].sum()}, changing Joins {tot[:, 4].sum()}, inconsistent in TestUnknowns "
          f"{tot[:, 5].sum()}, in Propagate {tot[:, 6].sum()}, most rounds {tot[:, 7].max()}; kept {k}: "
          + ", ".join(f"{n} {int(v.sum())}" for n, v in kc.items())
          + f"; strip flags {np.bincount(data['strip_flags'].reshape(-1), minlength=4).tolist()}")


if __name__ == "__main__":
    main()
