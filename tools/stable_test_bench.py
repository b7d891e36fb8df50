"""Times the LifeStable lookahead kernels (stable_test_kernels.hpp) against
Propagate and the streaming 1-generation step of the same run, in one process on
one GPU:

    python tools/stable_test_bench.py [--n 1048576] [--rounds 5] [--out FILE]

Inputs: the kept objects of tests/golden/stable_test.npz (partly known still
lifes, tests/stable_test_cases.py), replicated to n LifeStables (5 KiB each).
Cases, each on a fresh copy of its input (the kernels work in place; the copy is
outside the timed events), warmed up, median of `rounds`:

  step_1gen            Step() on n universes (1 KiB each)
  propagate            Propagate (lifeapi_stable_pass_batch_dev, pass 4)
  propagate_strip      PropagateStrip at the pattern's own column, from the pool's
                       unsynchronised start
  test_unknowns        TestUnknowns(Vulnerable().ZOI()) on the objects after Propagate
  propagate_and_test   PropagateAndTest

each with its ratio to propagate and to step_1gen.  One JSON line per case, and
one with the recorder's mean cells tested per object; needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_stable_test_model as M  # noqa: E402
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "stable_test_bench needs a GPU"
    n = args.n
    rec = M.Recording()
    k = len(rec.kept)
    pick = torch.arange(n, device="cuda") % k
    given = up(rec.planes.reshape(k, 640))[pick]
    fresh = up(rec.start[:, 1].reshape(k, 640))[pick]
    columns = torch.from_numpy(rec.columns).cuda()[pick].contiguous()
    block = np.zeros(64, np.uint64)
    block[[63, 0, 1]] = np.uint64(0x8000000000000003)
    after = given.clone()
    hip.stable_pass(after, "propagate")
    cells = hip.convolve(hip.stable_vulnerable(after), up(block)[None])       # Vulnerable().ZOI()
    work = torch.empty_like(given)
    states = hip.fill_random(n, seed=1500) & hip.fill_random(n, seed=1501)
    y = hip.empty_universes(n)

    cases = [("step_1gen", None, lambda: hip.step(states, out=y, generations=1)),
             ("propagate", given, lambda: hip.stable_pass(work, "propagate")),
             ("propagate_strip", fresh, lambda: hip.stable_strip_pass(work, columns, "propagate_strip")),
             ("test_unknowns", after, lambda: hip.stable_test_unknowns(work, cells)),
             ("propagate_and_test", given, lambda: hip.stable_propagate_and_test(work))]
    ms = {name: [] for name, *_ in cases}
    for r in range(1 + args.rounds):  # one warm-up round
        for name, src, fn in cases:
            if src is not None:
                work.copy_(src)
            t, _ = timed(fn)
            if r >= 1:
                ms[name].append(t)
    # the timed work is the recorded one
    work.copy_(given)
    flags = hip.stable_propagate_and_test(work)
    torch.cuda.synchronize()
    assert (flags[:k].cpu().numpy() == rec.pat_flags).all()
    assert (work[:k].cpu().numpy().view(np.uint64).reshape(k, 10, 64) == rec.pat).all()

    med = {name: float(np.median(v)) for name, v in ms.items()}
    lines = []
    for name, *_ in cases:
        lines.append(json.dumps({"case": name, "n": n, "rounds": args.rounds, "median_ms": round(med[name], 4),
                                 "min_ms": round(min(ms[name]), 4), "max_ms": round(max(ms[name]), 4),
                                 "ns_per_object": round(med[name] * 1e6 / n, 2),
                                 "ratio_to_propagate": round(med[name] / med["propagate"], 2),
                                 "ratio_to_step": round(med[name] / med["step_1gen"], 2)}))
    kept_tested = float(rec.counts[:, 1].mean())
    lines.append(json.dumps({"pool_objects": k, "mean_cells_tested_per_object_pool": round(kept_tested, 2),
                             "mean_cells_tested_per_object_drawn_family": round(rec.mean_tested, 2)}))
    for line in lines:
        print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
