"""Times k_stable_complete (stable_complete_kernels.hpp) against Propagate on the
same batch, in one process on one GPU:

    python tools/stable_complete_bench.py [--n 1048576] [--rounds 5] [--depth 24] [--out FILE]

Inputs: the kept objects of tests/golden/stable_complete.npz (the known part of
a still life, tests/stable_complete_cases.py), replicated to n LifeStables (5 KiB
each).  Cases, warmed up, device events, median of `rounds`:

  propagate            Propagate (lifeapi_stable_pass_batch_dev, pass 4) on a fresh
                       copy of the batch (in place; the copy is outside the events)
  complete             CompleteStable(minimise = false), a full workspace
  complete_minimise    CompleteStable(minimise = true)
  complete_seeded      CompleteStable(minimise = false, useSeed), a seed per object
  complete_one_in_8    `complete` with an eighth of the full workspace

each with time per object and, from the node counts the kernel returns, per
node, and the node / Propagate ratio (a node is one Propagate plus Vulnerable, two
neighbour counts and at most one 5376-byte frame each way).  One JSON line per
case; needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_stable_complete_model as M  # noqa: E402
import lifeapi_amd.hip as hip  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64).copy()).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "stable_complete_bench needs a GPU"
    n = args.n
    rec = M.recording()
    k = len(rec.kept)
    assert rec.depth.max() <= args.depth
    pick = torch.arange(n, device="cuda") % k
    given = up(rec.planes.reshape(k, 640))[pick]
    seeds = up(rec.seeds)[pick]
    work = torch.empty_like(given)
    full = hip.stable_complete_workspace_bytes(n, args.depth)
    ws = torch.empty(full, dtype=torch.uint8, device="cuda")
    small = ws[:256 + (full - 256) // 8 // (args.depth * 5376) * (args.depth * 5376)]

    def complete(f, workspace):
        minimise, use_seed = ((False, False), (True, False), (False, True))[f]
        return lambda: hip.stable_complete(given, minimise=minimise, seed=seeds if use_seed else None,
                                           max_depth=args.depth, workspace=workspace)

    cases = [("propagate", None, lambda: hip.stable_pass(work, "propagate")),
             ("complete", 0, complete(0, ws)), ("complete_minimise", 1, complete(1, ws)),
             ("complete_seeded", 2, complete(2, ws)), ("complete_one_in_8", 0, complete(0, small))]
    ms, nodes = {name: [] for name, *_ in cases}, {}
    for r in range(1 + args.rounds):  # one warm-up round
        for name, f, fn in cases:
            if f is None:
                work.copy_(given)
            t, out = timed(fn)
            if r >= 1:
                ms[name].append(t)
            if f is not None and r == 0:
                # the timed work is the recorded one
                result, best, count = (x[:k].cpu().numpy() for x in out)
                assert (result == rec.result[:, f]).all() and (count == rec.nodes[:, f]).all()
                assert (best.view(np.uint64) == rec.best[:, f]).all()
                nodes[name] = int(out[2].sum().item())
    med = {name: float(np.median(v)) for name, v in ms.items()}
    lines = []
    for name, f, _ in cases:
        line = {"case": name, "n": n, "rounds": args.rounds, "median_ms": round(med[name], 4),
                "min_ms": round(min(ms[name]), 4), "max_ms": round(max(ms[name]), 4),
                "ns_per_object": round(med[name] * 1e6 / n, 2)}
        if f is not None:
            line.update({"nodes": nodes[name], "nodes_per_object": round(nodes[name] / n, 2),
                         "ns_per_node": round(med[name] * 1e6 / nodes[name], 2),
                         "node_to_propagate": round(med[name] / nodes[name] / (med["propagate"] / n), 2),
                         "workspace_bytes": int((small if name == "complete_one_in_8" else ws).numel())})
        lines.append(json.dumps(line))
    for line in lines:
        print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
