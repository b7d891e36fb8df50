"""Instruction counts of IntersectingOffsets' self form next to Convolve with a
shared pattern, per universe, from hardware counters:

    rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU --kernel-include-regex "k_convolve" \\
        -d DIR -o pmc --output-format csv -- python tools/pair_pmc.py run [--n 1048576]
    python tools/pair_pmc.py sum DIR [--n 1048576]

run: on n universes holding one 16-cell region each (the batch of
tools/symmetry_bench.py), three launches each of Convolve with universe 0's
region as the shared pattern (k_convolve) and of IntersectingOffsets(active,
sym) for C2, D2AcrossX and D2diagodd (k_convolve_pair, in that order), and
nothing else under the counters.  sum: the counter CSV as one JSON line per
launch group: wave-level instructions per universe.  Counters are collected in
a run of their own, never together with a trace."""
import argparse
import csv
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GROUPS = ("convolve_shared_16", "intersecting_self_c2", "intersecting_self_d2acrossx", "intersecting_self_d2diagodd")
REPS = 3


def run(n):
    import torch

    import lifeapi_amd.hip as hip
    u = torch.arange(n, device="cuda")
    col, row = u % 55, (u * 7) % 58
    blocks = torch.zeros((n, 64), dtype=torch.int64, device="cuda")
    for j in range(4):
        blocks[u, col + j] = torch.bitwise_left_shift(torch.full_like(u, 15), row)
    shared, y = blocks[:1].clone(), torch.empty_like(blocks)
    for _ in range(REPS):
        hip.convolve(blocks, shared, out=y)
    for sym in ("C2", "D2AcrossX", "D2diagodd"):
        for _ in range(REPS):
            hip.intersecting_offsets(blocks, sym, out=y)
    torch.cuda.synchronize()


def summarize(d, n):
    paths = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
    if not paths:
        raise SystemExit(f"no counter_collection.csv under {d}")
    by_disp = {}
    for path in paths:
        with open(path) as f:
            for r in csv.DictReader(f):
                e = by_disp.setdefault(int(r["Dispatch_Id"]), {"name": r["Kernel_Name"], "ctr": {}})
                e["ctr"][r["Counter_Name"]] = e["ctr"].get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
    disp = [by_disp[k] for k in sorted(by_disp) if "k_convolve" in by_disp[k]["name"]]
    if len(disp) != REPS * len(GROUPS):
        raise SystemExit(f"{len(disp)} k_convolve* dispatches, expected {REPS * len(GROUPS)}")
    for g, name in enumerate(GROUPS):
        rows = disp[REPS * g:REPS * g + REPS]
        assert ("k_convolve_pair" in rows[0]["name"]) == (g > 0), rows[0]["name"]
        rec = {"case": name, "n": n, "kernel": re.search(r"k_\w+", rows[0]["name"]).group(0)}
        for c in ("SQ_INSTS_VALU", "SQ_INSTS_SALU"):
            vals = [r["ctr"].get(c, float("nan")) / n for r in rows]
            rec[c + "_per_universe"] = round(sorted(vals)[len(vals) // 2], 2)
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("run", "sum"))
    ap.add_argument("dir", nargs="?")
    ap.add_argument("--n", type=int, default=1 << 20)
    args = ap.parse_args()
    if args.mode == "run":
        run(args.n)
    else:
        summarize(args.dir, args.n)


if __name__ == "__main__":
    main()
