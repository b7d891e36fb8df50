"""Times the connected-component kernels (components_kernels.hpp) against the
streaming step of the same run and against the composition the library allowed
before them, in one process on one GPU:

    python tools/components_bench.py [--n 1048576] [--rounds 5] [--compose-n 65536] [--out FILE]

Inputs: soups of density 2^-1, 2^-3 and 2^-4, a batch of pitch-3 spirals (612
rounds of the reference's loop), and a 2^-4 soup with a glider planted whose
one cell seeds ComponentContaining.  On each soup and the spirals:
ComponentContaining from the universe's FirstCell, Components count-only and
Components with a cap of 8.  Every kernel case is timed two ways with device
events, warmed up, over `rounds` alternating rounds: alone, each launch after
the 768 MiB read scrub bench.py uses, and back to back (3 launches between one
pair of events); reported with the ratio to the 1-generation step of the same
run.

The yardstick ("compose"): ComponentContaining as lifeapi_convolve_batch_dev
with the corona, torch & / & ~ / |, and one any() sync per round until no
universe grows, on the same input, timed once with device events, with its
round count (the longest flood of the batch).  Components composed the same way
(first_on for the seed, the composed flood, one any() per component) is timed
on the first `compose-n` universes, the kernel on the same slice beside it.
One JSON line per case; needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import components_cases as C  # noqa: E402
import lifeapi_amd.hip as hip  # noqa: E402

SCRUB_MIB = 768
CAP = 8
REPS = 3


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def first_cells(x):
    """FirstCell of every universe as a batch of seeds"""
    cells = hip.first_on(x).to(torch.int64)
    seeds = torch.zeros_like(x)
    on = torch.nonzero(cells[:, 0] >= 0).squeeze(1)
    seeds[on, cells[on, 0]] = torch.ones((), dtype=torch.int64, device="cuda") << cells[on, 1]
    return seeds


def compose_flood(x, seeds, corona):
    """the reference's loop over the batch with the parent's entry points; (result, rounds)"""
    res, front, rounds = torch.zeros_like(x), seeds.clone(), 0
    nb = torch.empty_like(x)
    while bool(front.any()):
        hip.convolve(front, corona, out=nb)
        nb &= x
        front = nb & ~res
        res |= nb
        rounds += 1
    return res, rounds


def compose_count(x, corona):
    rem, counts, rounds = x.clone(), torch.zeros(len(x), dtype=torch.int32, device="cuda"), 0
    while bool(rem.any()):
        counts += rem.any(dim=1)
        comp, r = compose_flood(rem, first_cells(rem), corona)
        rem &= ~comp
        rounds += r
    return counts, rounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--compose-n", type=int, default=1 << 16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "components_bench needs a GPU"
    n, m = args.n, min(args.compose_n, args.n)
    corona = torch.from_numpy(C.CORONAS["default"].view(np.int64).copy()).cuda()[None]

    def soup(k):
        s = hip.fill_random(n, seed=100 * k)
        for j in range(1, k):
            s &= hip.fill_random(n, seed=100 * k + j)
        return s
    inputs = {"soup_2^-1": soup(1), "soup_2^-3": soup(3), "soup_2^-4": soup(4)}
    spiral = torch.from_numpy(C.from_cells(C.spiral_path()).view(np.int64).copy()).cuda()
    inputs["spirals"] = spiral[None].repeat(n, 1).contiguous()
    glider = C.from_cells([(31, 30), (32, 31), (30, 32), (31, 32), (32, 32)])
    clear = C.from_cells([(x, y) for x in range(25, 38) for y in range(25, 38)])
    g = (inputs["soup_2^-4"] & ~torch.from_numpy(clear.view(np.int64).copy()).cuda()) | \
        torch.from_numpy(glider.view(np.int64).copy()).cuda()
    glider_seed = torch.from_numpy(C.from_cells([(32, 31)]).view(np.int64).copy()).cuda()[None]

    y = hip.empty_universes(n)
    counts = torch.empty(n, dtype=torch.int32, device="cuda")
    comps = torch.empty((n, CAP, 64), dtype=torch.int64, device="cuda")
    scrub_buf = torch.ones(SCRUB_MIB << 17, dtype=torch.int64, device="cuda")
    sink = torch.empty((), dtype=torch.int64, device="cuda")
    stream = hip._stream(None)

    def count_only(x, k=None):
        k = len(x) if k is None else k
        hip._check(hip.lib.lifeapi_components_batch_dev(x.data_ptr(), None, counts.data_ptr(), None, 0, k, stream))

    cases = [("step_1gen", lambda: hip.step(inputs["soup_2^-1"], out=y, generations=1), None)]
    compose = {}
    for name, x in inputs.items():
        seeds = first_cells(x)
        cases.append((f"containing_first_cell/{name}", lambda x=x, s=seeds: hip.component_containing(x, s, out=y),
                      lambda x=x, s=seeds: compose_flood(x, s, corona)))
        cases.append((f"components_count/{name}", lambda x=x: count_only(x), None))
        cases.append((f"components_cap8/{name}",
                      lambda x=x: hip.components(x, max_components=CAP, count=False, components_out=comps), None))
        cases.append((f"components_count_first_{m}/{name}", lambda x=x: count_only(x, m),
                      lambda x=x: compose_count(x[:m], corona)))
    cases.append(("containing_glider_cell/soup_2^-4", lambda: hip.component_containing(g, glider_seed, out=y),
                  lambda: compose_flood(g, glider_seed.expand(n, 64).contiguous(), corona)))

    alone = {c[0]: [] for c in cases}
    b2b = {c[0]: [] for c in cases}
    for r in range(1 + args.rounds):  # one warm-up round
        for name, fn, _ in cases:
            torch.sum(scrub_buf, 0, out=sink)
            ms, _ = timed(fn)
            if r >= 1:
                alone[name].append(ms)
        for name, fn, _ in cases:
            fn()
            ms, _ = timed(lambda: [fn() for _ in range(REPS)])
            if r >= 1:
                b2b[name].append(ms / REPS)
    for name, fn, comp in cases:
        if comp is None:
            continue
        fn()
        torch.cuda.synchronize()
        want = y.clone() if name.startswith("containing") else counts[:m].clone()
        ms, (got, rounds) = timed(comp)
        assert torch.equal(got, want), f"{name}: the composition and the kernel disagree"
        compose[name] = {"ms": round(ms, 3), "rounds": rounds}

    lines = []
    step = {k: float(np.median(v["step_1gen"])) for k, v in (("alone", alone), ("b2b", b2b))}
    for name, _, _ in cases:
        rec = {"case": name, "n": n, "rounds": args.rounds}
        for how, ms in (("alone", alone[name]), ("b2b", b2b[name])):
            med = float(np.median(ms))
            rec[how] = {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                        "ratio_to_step": round(med / step[how], 3)}
        if name in compose:
            rec["compose"] = dict(compose[name], over_kernel_alone=round(compose[name]["ms"] / rec["alone"]["median_ms"], 1))
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
