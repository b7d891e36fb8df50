"""Times Match, Convolve and InteractionOffsets (match_kernels.hpp) against the
streaming step of the same run, which moves the same bytes (512 B in, 512 B
out per universe), in one process on one GPU:

    python tools/match_bench.py [--n 1048576] [--rounds 7] [--out FILE]

Every case is timed two ways with device events, warmed up, over `rounds`
alternating rounds (each round runs every case once, in turn): alone, each
launch after the 768 MiB read scrub bench.py uses, and back to back (5
launches between one pair of events).  Reported per case: median and min-max
ms, the ratio to the step of the same run, the algorithmic bytes over the
median as a share of 8 TB/s, and the VALU instructions per universe the
pattern costs in the kernels' loops (counted from the ISA, build/asm: per
half-column of r care rows, 6 per pair of rows -- 4 v_alignbit_b32 + 2
v_bitop3_b32 -- and 4 for an odd one; the cross-lane fetches are 2
ds_bpermute_b32 per populated column and universe, on the LDS pipe).
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


def pattern(cells):
    p = np.zeros(64, np.uint64)
    for a, b in cells:
        p[a % 64] |= np.uint64(1) << np.uint64(b % 64)
    return p


def loop_valu(*planes):
    """VALU instructions per universe of the fold loops for these pattern
    planes (each plane's rows of a column fold separately, low and high half)"""
    total = 0
    for p in planes:
        for w in p:
            for half in (int(w) & 0xFFFFFFFF, int(w) >> 32):
                r = bin(half).count("1")
                total += 6 * (r // 2) + 4 * (r % 2)
    return total


def dev(p):
    return torch.from_numpy(p.view(np.int64).reshape(1, 64).copy()).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "match_bench needs a GPU"
    n = args.n
    x = hip.fill_random(n, seed=11)
    y = hip.empty_universes(n)
    scrub_buf = torch.ones(SCRUB_MIB << 17, dtype=torch.int64, device="cuda")
    sink = torch.empty((), dtype=torch.int64, device="cuda")

    def scrub():
        torch.sum(scrub_buf, 0, out=sink)

    blk = pattern([(20 + i, 30 + j) for i in (0, 1) for j in (0, 1)])
    ring = pattern([(19 + i, 29 + j) for i in range(4) for j in range(4)]) & ~blk
    rng = np.random.default_rng(77)
    bits = rng.integers(0, 2, size=(5, 5))
    w5 = pattern([(30 + i, 12 + j) for i in range(5) for j in range(5) if bits[i, j]])
    u5 = pattern([(30 + i, 12 + j) for i in range(5) for j in range(5) if not bits[i, j]])
    p3 = pattern([(i, j) for i in (-1, 0, 1) for j in (-1, 0, 1)])
    p7 = pattern([(i, j) for i in range(7) for j in range(7)])
    eater = pattern([(30, 30), (31, 30), (30, 31), (32, 31), (32, 32), (32, 33), (33, 33)])
    d = {k: dev(v) for k, v in dict(blk=blk, ring=ring, w5=w5, u5=u5, p3=p3, p7=p7, eater=eater).items()}
    io, cnt = 1024, 516  # algorithmic bytes per universe: mask out / count only
    cases = [
        ("step_1gen", lambda: hip.step(x, out=y, generations=1), io, None),
        ("match_block_ring_mask", lambda: hip.match(x, d["blk"], d["ring"], out=y), io, loop_valu(blk, ring)),
        ("match_block_ring_count", lambda: hip.match(x, d["blk"], d["ring"], count="only"), cnt, loop_valu(blk, ring)),
        ("match_5x5_mask", lambda: hip.match(x, d["w5"], d["u5"], out=y), io, loop_valu(w5, u5)),
        ("match_5x5_count", lambda: hip.match(x, d["w5"], d["u5"], count="only"), cnt, loop_valu(w5, u5)),
        ("convolve_3x3", lambda: hip.convolve(x, d["p3"], out=y), io, loop_valu(p3)),
        ("convolve_7x7", lambda: hip.convolve(x, d["p7"], out=y), io, loop_valu(p7)),
        ("interaction_offsets_eater", lambda: hip.interaction_offsets(x, d["eater"], out=y), io, None),
    ]
    alone = {c[0]: [] for c in cases}
    b2b = {c[0]: [] for c in cases}
    reps = 5
    for r in range(2 + args.rounds):  # two warm-up rounds
        for name, fn, _, _ in cases:
            scrub()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= 2:
                alone[name].append(e0.elapsed_time(e1))
        for name, fn, _, _ in cases:
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
    for name, _, nbytes, valu in cases:
        rec = {"case": name, "n": n, "rounds": args.rounds, "loop_valu_per_universe": valu,
               "bytes_per_universe": nbytes}
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
