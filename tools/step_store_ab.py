"""A/B: the streaming step's body with a wave's stores issued back to back
(the product's step_body: full groups load and store unconditionally, one
group per wave, nothing waited for behind the stores; tuning build body "r7")
against round 6's (body "r6", tools/tune/step_r6.hpp: every store behind a
vmcnt(0) of its own and one more before the wave ends), same process, same
buffers, ping-pong as bench.py's timed region.

Timing as bench.back_to_back_ms: 20 launches between one pair of events,
median of 3 runs = one round of one variant; the variants are interleaved
round by round (--rounds, at least 7), so drift of the box lands on all of
them alike.  Sizes: 1M universes (the bench's config 2: 4 per wave, every
block slot, alternating order, the last min(256 MiB, half) stored plain) and
16M (config 4: 8 per wave, 7 blocks per CU, one order, nontemporal, XCD
chunks) -- both bodies under round 6's policy of the size, then the retune
sweep on the new body: universes per wave {4, 8} x resident blocks per CU
{all that fit, 7, 6}, at 1M x plain tail {0, 128, 256 MiB} x {alternating,
fixed} order, at 16M x {XCD chunks, plain block mapping}.  At 1M also the
fused 1-generation step with final states (k_step_contains<8>) in both forms
(tuning build step_contains_nat, 8 per wave against 256 + 8: the same
treatment), one order, nontemporal.

One JSON line per (size, variant): the rounds, their median and p10 / p90;
then per size one "verdict" line for r7 against r6 and one per sweep variant
against round 6's policy on r7.  The rule (both): faster only if the median
improves by more than 3 x the baseline's own p10-p90 spread over its rounds
and the two sets of rounds do not overlap.  Every variant's result is checked
word for word against the product's launch first."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools", "tune"))
import bench  # noqa: E402
import lifeapi_amd.hip as hip  # noqa: E402
import tune_hip  # noqa: E402

MIB = 1 << 20


class RT:
    kind = "hip"
    device = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()

    @staticmethod
    def event():
        return torch.cuda.Event(enable_timing=True)


def shipped_policy(n):
    """Round 6's launch policy for gens <= 2 as step_order keywords: the policy
    both bodies are compared under and the sweep's baseline ("_shipped" in the
    variant names; what the sweep then moved is in step.hip shipped_step)."""
    if n > (1 << 22):
        return dict(upw=8, resident=7, alternate=False, plain_bytes=0, xcd_chunk=True)
    return dict(upw=4, resident=0, alternate=True, plain_bytes=min(256 * MIB, n * 512 // 2), xcd_chunk=False)


def variants(n):
    """name -> (body, policy); the first two are the A/B, the rest the sweep."""
    ship = shipped_policy(n)
    out = {"r6_shipped": ("r6", ship), "r7_shipped": ("r7", ship)}
    for upw in (4, 8):
        for resident in (0, 7, 6):
            if n > (1 << 22):
                for chunk in (True, False):
                    p = dict(upw=upw, resident=resident, alternate=False, plain_bytes=0, xcd_chunk=chunk)
                    if p != ship:
                        out[f"r7_u{upw}_res{resident}_{'xcd' if chunk else 'flat'}"] = ("r7", p)
            else:
                for plain in (0, 128 * MIB, 256 * MIB):
                    for alt in (True, False):
                        p = dict(upw=upw, resident=resident, alternate=alt, plain_bytes=min(plain, n * 512 // 2),
                                 xcd_chunk=False)
                        if p != ship:
                            out[f"r7_u{upw}_res{resident}_plain{plain // MIB}_{'alt' if alt else 'fixed'}"] = ("r7", p)
    return out


def launcher(body, p):
    flip = [False]

    def fn(x, y):
        rev = p["alternate"] and flip[0]
        flip[0] = not flip[0]
        tune_hip.step_order(x, y, 1, reverse=rev, nts=True, resident=p["resident"], upw=p["upw"],
                            plain_bytes=p["plain_bytes"], xcd_chunk=p["xcd_chunk"], body=body)
    return fn


def contains_launcher(upw, w, u):
    def fn(x, y):
        tune_hip.step_contains_nat(x, w, u, 1, upw, 0, final=y)
    return fn


def stats(rounds):
    r = np.asarray(rounds)
    return {"median_ms": float(np.median(r)), "p10_ms": float(np.percentile(r, 10)),
            "p90_ms": float(np.percentile(r, 90)), "min_ms": float(r.min()), "max_ms": float(r.max())}


def verdict(base, cand):
    """cand faster than base: median gain > 3 x base's p10-p90 spread, rounds disjoint."""
    b, c = stats(base), stats(cand)
    spread = b["p90_ms"] - b["p10_ms"]
    gain = b["median_ms"] - c["median_ms"]
    return {"base_median_ms": b["median_ms"], "median_ms": c["median_ms"], "ratio": c["median_ms"] / b["median_ms"],
            "base_spread_p10_p90_ms": spread, "gain_ms": gain, "gain_over_spread": gain / spread if spread else None,
            "rounds_disjoint": bool(max(cand) < min(base)), "faster": bool(gain > 3 * spread and max(cand) < min(base)),
            "slower": bool(-gain > 3 * spread and min(cand) > max(base))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1 << 20, 1 << 24])
    ap.add_argument("--no-sweep", action="store_true", help="the two bodies under round 6's policy only")
    args = ap.parse_args()
    if args.rounds < 7:
        ap.error("at least 7 rounds")
    rt = RT()
    for n in args.sizes:
        a0 = hip.fill_random(n, seed=4)
        a, b = a0.clone(), torch.empty_like(a0)
        want = hip.step(a0)
        vs = variants(n)
        if args.no_sweep:
            vs = {k: v for k, v in vs.items() if k.endswith("_shipped")}
        fns, exact = {}, {}
        for name, (body, p) in vs.items():
            fns[name] = launcher(body, p)
            got = torch.empty_like(a0)
            for _ in range(2):  # (both orders of an alternating launch)
                got.zero_()
                fns[name](a0, got)
                torch.cuda.synchronize()
                exact[name] = exact.get(name, True) and bool(torch.equal(got, want))
            del got
        if n <= (1 << 22):
            # a block in a ring of dead cells: few universes hold it, as in a search
            w, u = torch.zeros((1, 64), dtype=torch.int64, device="cuda"), torch.zeros((1, 64), dtype=torch.int64,
                                                                                       device="cuda")
            w[0, 10:12] = 3 << 40
            u[0, 9:13] = 15 << 39
            u ^= w
            want_first, want_fin = hip.step_contains(a0, w, u, 1, final=torch.empty_like(a0))
            for name, upw in (("contains_r6", 8), ("contains_r7", 256 + 8)):
                vs[name] = ("r6" if upw == 8 else "r7", dict(upw=upw, resident=0, alternate=False, plain_bytes=0,
                                                             xcd_chunk=False))
                fns[name] = contains_launcher(upw, w, u)
                got = torch.empty_like(a0)
                first = tune_hip.step_contains_nat(a0, w, u, 1, upw, 0, final=got)
                torch.cuda.synchronize()
                exact[name] = bool(torch.equal(got, want_fin)) and bool(torch.equal(first, want_first))
                del got
        rounds = {name: [] for name in vs}
        for _ in range(args.rounds):
            for name in vs:
                a.copy_(a0)
                rounds[name].append(bench.back_to_back_ms(rt, fns[name], a, b, reps=20, warm=5, repeats=3))
        for name, (body, p) in vs.items():
            s = stats(rounds[name])
            print(json.dumps({"universes": n, "variant": name, "body": body, **p, "exact": exact[name],
                              "rounds_ms": rounds[name], **s,
                              "tb_per_s": n * 1024 / (s["median_ms"] / 1e3) / 1e12}), flush=True)
        print(json.dumps({"universes": n, "verdict": "r7_shipped against r6_shipped",
                          **verdict(rounds["r6_shipped"], rounds["r7_shipped"])}), flush=True)
        if "contains_r7" in vs:
            print(json.dumps({"universes": n, "verdict": "contains_r7 against contains_r6",
                              **verdict(rounds["contains_r6"], rounds["contains_r7"])}), flush=True)
        for name in vs:
            if not name.endswith("_shipped") and not name.startswith("contains_"):
                print(json.dumps({"universes": n, "verdict": f"{name} against r7_shipped",
                                  **verdict(rounds["r7_shipped"], rounds[name])}), flush=True)
        del a, a0, b, want
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
