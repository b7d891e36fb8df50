"""A/B: the streaming step's two ways above the plain streaming rate, together.
Up to 4M universes the product alternates the group order between launches
and stores the last min(256 MiB, half) of each launch plain (Infinity Cache
reuse); above, each XCD streams a contiguous eighth of the batch (kXcdChunk),
one order, all nontemporal.  Since step_kernels.hpp step_body decides the
plain tail by dispatch position (step_order.hpp), a chunked launch can keep
the end of every XCD's run in the cache, so the two compose.  This tool
measures the product of both at every size, same process, same buffers,
ping-pong as bench.py's timed region (tools/step_store_ab.py's method).

Baseline: the shipped policy of the size as step_order keywords ("shipped",
tuning build kernel k_step_ab: the product's code under another name), and
the product's own launch next to it ("product", hip.step).  Variants: XCD
chunks {off, on} x order {alternating, fixed} x plain tail {0, 128 MiB,
min(256 MiB, half)} x resident blocks per CU {all 8, 7, 6} x universes per
wave {4, 8}.

Timing as bench.back_to_back_ms: 20 launches between one pair of events,
median of 3 runs = one round of one variant; the variants interleaved round
by round (--rounds, at least 7).  The rule (round 7's): faster only if the
median gain exceeds 3 x the baseline's p10-p90 spread over its rounds and the
two sets of rounds do not overlap.  Every variant's result is checked word for
word against the product's first, in both orders.

Output, kept short (a sweep is 73 variants x 6 sizes): per size one object
for "shipped" (its policy, rounds_us in microseconds, median, p10, p90, and
whether every variant was exact), then one array per variant: [universes,
variant, rounds_us, median_us, gain over "shipped" / its p10-p90 spread,
"faster" / "slower" / "" by the rule], with "NOT EXACT" appended where a
variant's result differed.  A variant's name
spells its policy: mapping (xcd chunks / flat) _ order _ plain tail in MiB _
resident blocks per CU (0 = all 8) _ universes per wave."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools", "tune"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
import lifeapi_amd.hip as hip  # noqa: E402
import tune_hip  # noqa: E402
from step_store_ab import MIB, RT, launcher, stats, verdict  # noqa: E402

SIZES = [1 << 19, 1 << 20, 1 << 21, 1 << 22, 1 << 23, 1 << 24]


def parent_policy(n):
    """step.hip shipped_step for gens <= 2 before this round, as step_order
    keywords: what every variant is compared against."""
    resident = 0 if n < (1 << 20) else 7 if n < (1 << 21) else 6
    if n > (1 << 22):
        return dict(upw=4, resident=resident, alternate=False, plain_bytes=0, xcd_chunk=True)
    return dict(upw=4, resident=resident, alternate=n >= (3 << 16), plain_bytes=min(256 * MIB, n * 512 // 2),
                xcd_chunk=False)


def variants(n):
    out = {"shipped": parent_policy(n)}
    for chunk in (False, True):
        for alt in (True, False):
            for plain in (0, 128 * MIB, 256 * MIB):
                for resident in (0, 7, 6):
                    for upw in (4, 8):
                        p = dict(upw=upw, resident=resident, alternate=alt, plain_bytes=min(plain, n * 512 // 2),
                                 xcd_chunk=chunk)
                        if p not in out.values():
                            out[f"{'xcd' if chunk else 'flat'}_{'alt' if alt else 'fixed'}_plain"
                                f"{p['plain_bytes'] // MIB}_res{resident}_u{upw}"] = p
    return out


def report(n, shipped, rounds, exact):
    """the lines of one size (see above) from {variant: rounds in ms}"""
    def us(v):
        return round(v * 1e3, 2)

    base = stats(rounds["shipped"])
    yield {"universes": n, "variant": "shipped", **shipped, "rounds_us": [us(v) for v in rounds["shipped"]],
           "median_us": us(base["median_ms"]), "p10_us": us(base["p10_ms"]), "p90_us": us(base["p90_ms"]),
           "all_exact": all(exact.values())}
    for name, r in rounds.items():
        if name == "shipped":
            continue
        v = verdict(rounds["shipped"], r)
        line = [n, name, [us(x) for x in r], us(v["median_ms"]),
                None if v["gain_over_spread"] is None else round(v["gain_over_spread"], 1),
                "faster" if v["faster"] else "slower" if v["slower"] else ""]
        if not exact[name]:
            line.append("NOT EXACT")
        yield line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="+", default=SIZES)
    ap.add_argument("--only", nargs="+", default=None, help="these variants (and the two baselines) only")
    args = ap.parse_args()
    if args.rounds < 7:
        ap.error("at least 7 rounds")
    rt = RT()
    for n in args.sizes:
        a0 = hip.fill_random(n, seed=4)
        a, b = a0.clone(), torch.empty_like(a0)
        want = hip.step(a0)
        vs = variants(n)
        if args.only:
            vs = {k: v for k, v in vs.items() if k == "shipped" or k in args.only}
        fns = {name: launcher("r7", p) for name, p in vs.items()}
        fns["product"] = lambda x, y: hip.step(x, out=y, generations=1)
        exact, got = {}, torch.empty_like(a0)
        for name, fn in fns.items():
            exact[name] = True
            for _ in range(2):  # (both orders of an alternating launch)
                got.zero_()
                fn(a0, got)
                torch.cuda.synchronize()
                exact[name] = exact[name] and bool(torch.equal(got, want))
        del got
        rounds = {name: [] for name in fns}
        for _ in range(args.rounds):
            for name, fn in fns.items():
                a.copy_(a0)
                rounds[name].append(bench.back_to_back_ms(rt, fn, a, b, reps=20, warm=5, repeats=3))
        for line in report(n, vs["shipped"], rounds, exact):
            print(json.dumps(line, separators=(",", ":")), flush=True)
        del a, a0, b, want
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
