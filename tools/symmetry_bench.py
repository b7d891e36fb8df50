"""Times the symmetry kernels (symmetry_kernels.hpp) against the streaming step
of the same run, in one process on one GPU:

    python tools/symmetry_bench.py [--n 1048576] [--rounds 7] [--out FILE]

Transform, Symmetricize, Halve and Skew move what the step moves (512 B in,
512 B out per universe), the per-universe-offset forms 8 B more;
IntersectingOffsets reads one batch in the self form and two otherwise; XYBounds reads 512 B and writes 16, the mask-only orbit reads 512 B
and writes 1, the orbit with images writes 8 x 512 B.  Every case is timed two
ways with device events, warmed up, over `rounds` alternating rounds (each
round runs every case once, in turn): alone, each launch after the 768 MiB
read scrub bench.py uses, and back to back (5 launches between one pair of
events).  Reported per case: median and min-max ms, the ratio to the step of
the same run and the algorithmic bytes over the median as a share of 8 TB/s.
One JSON line per case; needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import lifeapi_amd.hip as hip  # noqa: E402

SCRUB_MIB = 768
HBM_TBPS = 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "symmetry_bench needs a GPU"
    n = args.n
    x = hip.fill_random(n, seed=11)
    y = hip.empty_universes(n)
    bounds = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    first = torch.empty(n, dtype=torch.uint8, device="cuda")
    images = torch.empty((n, 8, 64), dtype=torch.int64, device="cuda")
    scrub_buf = torch.ones(SCRUB_MIB << 17, dtype=torch.int64, device="cuda")
    sink = torch.empty((), dtype=torch.int64, device="cuda")
    stream = hip._stream(None)

    def scrub():
        torch.sum(scrub_buf, 0, out=sink)

    # one 16-cell region (a 4 x 4 block) and one 3-cell region per universe, placed by the universe's index;
    # the shared pattern of the yardstick is universe 0's block; offsets in [-200, 200]
    u = torch.arange(n, device="cuda")
    col, row = u % 55, (u * 7) % 58
    blocks, threes = torch.zeros_like(x), torch.zeros_like(x)
    for j in range(4):
        blocks[u, col + j] = torch.bitwise_left_shift(torch.full_like(u, 15), row)
    for j, (dc, dr) in enumerate(((0, 0), (5, 2), (9, 1))):
        threes[u, col + dc] = torch.bitwise_left_shift(torch.ones_like(u), row + dr)
    shared = blocks[:1].clone()
    offsets = torch.randint(-200, 201, (n, 2), dtype=torch.int32, device="cuda")

    def orbit(img):
        hip._check(hip.lib.lifeapi_symmetry_orbit_batch_dev(x.data_ptr(), images.data_ptr() if img else None,
                                                            first.data_ptr(), n, stream))

    io = 1024  # algorithmic bytes per universe of the batch-to-batch kernels
    cases = [
        ("step_1gen", lambda: hip.step(x, out=y, generations=1), io),
        ("transform_identity_move", lambda: hip.transform(x, "Identity", 13, -27, out=y), io),
        ("transform_flipx", lambda: hip.transform(x, "ReflectAcrossXEven", out=y), io),
        ("transform_transpose", lambda: hip.transform(x, "ReflectAcrossYeqX", out=y), io),
        ("transform_rotate90_move", lambda: hip.transform(x, "Rotate90", 13, -27, out=y), io),
        ("symmetricize_c2", lambda: hip.symmetricize(x, "C2", 7, -3, out=y), io),
        ("symmetricize_c4", lambda: hip.symmetricize(x, "C4", 7, -3, out=y), io),
        ("symmetricize_d4diag", lambda: hip.symmetricize(x, "D4diag", 7, -3, out=y), io),
        ("transform_offsets_identity", lambda: hip.transform_offsets(x, "Identity", offsets, out=y), io + 8),
        ("transform_offsets_rotate90", lambda: hip.transform_offsets(x, "Rotate90", offsets, out=y), io + 8),
        ("symmetricize_offsets_c2", lambda: hip.symmetricize_offsets(x, "C2", offsets, out=y), io + 8),
        ("symmetricize_offsets_c4", lambda: hip.symmetricize_offsets(x, "C4", offsets, out=y), io + 8),
        ("symmetricize_offsets_d4diag", lambda: hip.symmetricize_offsets(x, "D4diag", offsets, out=y), io + 8),
        ("halve", lambda: hip.halve(x, "Halve", out=y), io),
        ("halve_y", lambda: hip.halve(x, "HalveY", out=y), io),
        ("skew", lambda: hip.skew(x, out=y), io),
        # IntersectingOffsets(active, sym) of one 16-cell region per universe, next to Convolve of the same
        # batch with one shared 16-cell pattern; then a half-density batch against 3-cell regions, both orders
        ("convolve_shared_16", lambda: hip.convolve(blocks, shared, out=y), io),
        ("intersecting_self_c2", lambda: hip.intersecting_offsets(blocks, "C2", out=y), io),
        ("intersecting_self_d2acrossx", lambda: hip.intersecting_offsets(blocks, "D2AcrossX", out=y), io),
        ("intersecting_self_d2diagodd", lambda: hip.intersecting_offsets(blocks, "D2diagodd", out=y), io),
        ("pair_dense_x_3cells", lambda: hip.convolve_pair(x, threes, out=y), io + 512),
        ("pair_3cells_x_dense", lambda: hip.convolve_pair(threes, x, out=y), io + 512),
        ("bounds", lambda: hip._check(hip.lib.lifeapi_bounds_batch_dev(x.data_ptr(), bounds.data_ptr(), n, stream)),
         528),
        ("orbit_mask_only", lambda: orbit(False), 513),
        ("orbit_with_images", lambda: orbit(True), 512 + 8 * 512 + 1),
    ]
    alone = {c[0]: [] for c in cases}
    b2b = {c[0]: [] for c in cases}
    reps = 5
    for r in range(2 + args.rounds):  # two warm-up rounds
        for name, fn, _ in cases:
            scrub()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= 2:
                alone[name].append(e0.elapsed_time(e1))
        for name, fn, _ in cases:
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            if r >= 2:
                b2b[name].append(e0.elapsed_time(e1) / reps)
    lines = []
    step = {k: float(np.median(v["step_1gen"])) for k, v in (("alone", alone), ("b2b", b2b))}
    for name, _, nbytes in cases:
        rec = {"case": name, "n": n, "rounds": args.rounds, "bytes_per_universe": nbytes}
        for how, ms in (("alone", alone[name]), ("b2b", b2b[name])):
            med = float(np.median(ms))
            rec[how] = {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                        "ratio_to_step": round(med / step[how], 3),
                        "share_of_8TBps": round(n * nbytes / (med * 1e-3) / (HBM_TBPS * 1e12), 3)}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
