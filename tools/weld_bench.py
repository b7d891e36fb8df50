"""Times the LifeWeld construction kernels (weld_kernels.hpp) against the
streaming step of the same run and against the composition the library allowed
before them, in one process on one GPU:

    python tools/weld_bench.py [--n 1048576] [--rounds 5] [--compose-n 262144] [--offsets-compose-n 4096] [--out FILE]

Inputs: states and `required` are soups of density 2^-2 and 2^-1; the welds are
FromRequired of those; `active` is a soup of density 2^-4 per weld; the mask is
a half plane; `other` is the eater's weld of tests/weld_cases.py.  Every kernel
case is timed two ways with device events, warmed up, over `rounds` alternating
rounds: alone, each launch after the 768 MiB read scrub bench.py uses, and back
to back (3 launches between one pair of events); reported with the ratio to the
1-generation step of the same run, and for the bytes-bound calls with the bytes
moved per second beside the step's.

The yardstick ("compose"): the same result from the entry points of the parent
commit -- convolve with the 3 x 3 block for ZOI, step, neighbour_count,
weld_step, and torch elementwise operations -- on the first `compose-n` objects,
timed once with device events, asserted equal bit for bit, the kernel timed on
the same slice beside it.  InteractionOffsets: six of its seven convolutions
have one pattern for the batch and compose as convolve launches; the first birth
term's pattern differs per weld (weld_kernels.hpp), which the parent can only do
one weld per launch, so it is composed on `offsets-compose-n` welds.
One JSON line per case; needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_weld_model as M  # noqa: E402
import weld_cases as C  # noqa: E402
import lifeapi_amd.hip as hip  # noqa: E402
from oracle.oracle import Port  # noqa: E402

SCRUB_MIB = 768
REPS = 3
DURATIONS = (0, 8, 40)
KIB_MOVED = {"step_1gen": 1, "from_required": 3, "to_target": 3, "to_stable/0": 7}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64).copy()).cuda()


# ---- the composition: the parent's entry points and torch elementwise ----------------

class Compose:
    def __init__(self, other_weld):
        block = np.zeros(64, np.uint64)
        block[[63, 0, 1]] = np.uint64(0x8000000000000003)
        self.block = up(block)[None]
        b = M.cells(other_weld)
        self.bkeep = M.mirrored(M.zoi(b[0] & ~(b[1] | b[2] | b[3])))
        self.bplanes = M.side_planes(M.mirrored(b[0]))
        self.bk = up(M.words(self.bkeep))[None]
        self.b_masked = {k: up(M.words(v & self.bkeep))[None] for k, v in self.bplanes.items()}
        self.b_cells = up(M.words(self.bplanes["cells"]))[None]
        self.b_dead2 = self.bplanes["dead2"]

    def zoi(self, x):
        return hip.convolve(x, self.block)

    @staticmethod
    def exactly(c, n):
        """cells whose 4-plane count (k, 4, 64) = bit3..bit0 is n"""
        r = None
        for plane, bit in enumerate((8, 4, 2, 1)):
            t = c[:, plane] if n & bit else ~c[:, plane]
            r = t if r is None else r & t
        return r

    def from_required(self, s, r):
        za = self.zoi(self.zoi(s) & ~r)
        kept = s & za
        frozen = (za & r) | (hip.step(kept) & ~kept)
        c = hip.neighbour_count(s & ~za)
        return torch.stack([kept, c[:, 1] & frozen, c[:, 2] & frozen, c[:, 3] & frozen], 1).reshape(len(s), 256)

    def to_target(self, welds):
        w = welds.view(-1, 4, 64)
        return w[:, 0].clone(), self.zoi(w[:, 0] & ~(w[:, 1] | w[:, 2] | w[:, 3])) & ~w[:, 0]

    def to_stable(self, welds, active, duration, mask):
        w = welds.view(-1, 4, 64)
        s, f2, f1, f0 = (w[:, i].contiguous() for i in range(4))
        frozen = f2 | f1 | f0
        mine = hip.neighbour_count(s)
        k0 = mine[:, 3] & f0
        k1 = (mine[:, 2] & f1) | (mine[:, 2] & k0) | (f1 & k0)
        k2 = (mine[:, 1] & f2) | (mine[:, 1] & k1) | (f2 & k1)
        total = torch.stack([mine[:, 0] ^ k2, mine[:, 1] ^ f2 ^ k1, mine[:, 2] ^ f1 ^ k0, mine[:, 3] ^ f0], 1)
        off = ~s & self.zoi(s & ~frozen)
        live, dead = frozen & s, frozen & ~s
        opt = {"live2": off.clone(), "live3": off.clone()}
        for name in M.OPTIONS[2:]:
            opt[name] = s.clone()
        for who, n, keep in M.STATIC_LINES:
            cells = (live if who == "live" else dead) & self.exactly(total, n)
            for name in M.OPTIONS:
                if name != keep:
                    opt[name] |= cells
        ever = torch.zeros_like(s)
        if duration:
            cw = welds.clone()
            cur = cw.view(-1, 4, 64)[:, 0]
            cur |= active
            for _ in range(duration):
                ever |= s ^ cur
                now = hip.neighbour_count(cur.contiguous())
                before = cur.clone()
                hip.weld_step(cw, 1)
                deadnow = mask & ~s & ~before
                fate = {"born": deadnow & cur, "stay": deadnow & ~cur}
                for f, a, b, name in M.REPLAY_LINES:
                    cells = fate[f] & self.exactly(now, a) & self.exactly(mine, b)
                    for o in M.OPTIONS:
                        if (o != name) if f == "born" else (o == name):
                            opt[o] |= cells
        was = mask & ~s & ever
        opt["live2"] |= was
        opt["live3"] |= was
        planes = [s, ~(s | off | was)] + [opt[name] for name in M.OPTIONS]
        return torch.stack(planes, 1).reshape(len(s), 640)

    def side_planes(self, s):
        c = hip.neighbour_count(s)
        b3, b2, b1, b0 = c[:, 0], c[:, 1], c[:, 2], c[:, 3]
        high = b3 | b2
        return {"cells": s, "dead1": ~high & ~b1 & b0 & ~s, "dead2": ~high & b1 & ~b0 & ~s, "live3": ~high & b1 & b0 & s,
                "live4up": high & s, "dead2up": (high | b1) & ~s, "dead1up": (high | b1 | b0) & ~s}

    def offsets_uniform(self, welds):
        """the six convolutions whose pattern is one for the batch; also a's dead1 plane under its mask"""
        w = welds.view(-1, 4, 64)
        s = w[:, 0].contiguous()
        ak = self.zoi(s & ~(w[:, 1] | w[:, 2] | w[:, 3]))
        a = self.side_planes(s)
        out = hip.convolve(s, self.b_cells)
        out |= hip.convolve((a["dead2"] & self.bk).contiguous(), self.b_masked["dead1"])     # a's plane under b's mask
        for mine, theirs in (("live3", "dead2up"), ("live4up", "dead1up"), ("dead2up", "live3"), ("dead1up", "live4up")):
            out |= hip.convolve((a[mine] & ak).contiguous(), self.b_masked[theirs])
        return out, (a["dead1"] & ak).contiguous(), ak

    def offsets(self, welds):
        out, first, ak = self.offsets_uniform(welds)
        b_dead2 = up(M.words(self.b_dead2))[None]
        patterns = (b_dead2 & ak).contiguous()                 # b's plane under a's mask: one pattern per weld
        for u in range(len(out)):
            out[u:u + 1] |= hip.convolve(first[u:u + 1], patterns[u:u + 1])
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--compose-n", type=int, default=1 << 18)
    ap.add_argument("--offsets-compose-n", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "weld_bench needs a GPU"
    n, m, mo = args.n, min(args.compose_n, args.n), min(args.offsets_compose_n, args.n)
    port = Port()

    def soup(k, seed):
        s = hip.fill_random(n, seed=seed)
        for j in range(1, k):
            s &= hip.fill_random(n, seed=seed + j)
        return s
    states, required, active = soup(2, 1400), soup(1, 1410), soup(4, 1420)
    mask = up(C.masks(port)["half"])[None]
    eater = np.asarray(dict(np.load(C.FIXTURE))["from_required"][0], np.uint64).reshape(4, 64)
    other = up(eater).reshape(1, 256)
    comp = Compose(eater)

    welds = hip.weld_from_required(states, required)
    y = hip.empty_universes(n)
    wanted, unwanted = hip.empty_universes(n), hip.empty_universes(n)
    stables = torch.empty((n, 640), dtype=torch.int64, device="cuda")
    welds_out = torch.empty((n, 256), dtype=torch.int64, device="cuda")
    scrub_buf = torch.ones(SCRUB_MIB << 17, dtype=torch.int64, device="cuda")
    sink = torch.empty((), dtype=torch.int64, device="cuda")

    # (name, kernel on the first k objects, where its answer then lies, composition on the first k objects,
    #  objects composed)
    cases = [("step_1gen", lambda k: hip.step(states[:k], out=y[:k], generations=1), None, None, 0),
             ("from_required", lambda k: hip.weld_from_required(states[:k], required[:k], out=welds_out[:k]),
              lambda k: welds_out[:k], lambda k: comp.from_required(states[:k], required[:k]), m),
             ("to_target", lambda k: hip.weld_to_target(welds[:k], wanted=wanted[:k], unwanted=unwanted[:k]),
              lambda k: torch.cat([wanted[:k], unwanted[:k]], 1), lambda k: torch.cat(comp.to_target(welds[:k]), 1), m)]
    for d in DURATIONS:
        cases.append((f"to_stable/{d}", lambda k, d=d: hip.weld_to_stable(welds[:k], active[:k], d, mask, out=stables[:k]),
                      lambda k: stables[:k], lambda k, d=d: comp.to_stable(welds[:k], active[:k], d, mask), m))
    cases.append(("interaction_offsets", lambda k: hip.weld_interaction_offsets(welds[:k], other, out=y[:k]),
                  lambda k: y[:k], lambda k: comp.offsets(welds[:k]), mo))
    cases.append(("interaction_offsets/six_uniform_terms_only", None, None,
                  lambda k: comp.offsets_uniform(welds[:k])[0], m))

    kernels = [c for c in cases if c[1] is not None]
    alone = {c[0]: [] for c in kernels}
    b2b = {c[0]: [] for c in kernels}
    for r in range(1 + args.rounds):  # one warm-up round
        for name, fn, *_ in kernels:
            torch.sum(scrub_buf, 0, out=sink)
            ms, _ = timed(lambda: fn(n))
            if r >= 1:
                alone[name].append(ms)
        for name, fn, *_ in kernels:
            fn(n)
            ms, _ = timed(lambda: [fn(n) for _ in range(REPS)])
            if r >= 1:
                b2b[name].append(ms / REPS)

    compose = {}
    for name, fn, where, cfn, k in cases:
        if cfn is None:
            continue
        rec = {"n": k}
        if fn is not None:
            fn(k)
            ms, _ = timed(lambda: fn(k))
            want = where(k).clone()
            rec["kernel_ms"] = round(ms, 4)
        cfn(min(k, 64))     # warm the composition's own launches and allocations
        ms, got = timed(lambda: cfn(k))
        if fn is not None:
            assert torch.equal(got.reshape(want.shape), want), f"{name}: the composition and the kernel disagree"
            rec["over_kernel"] = round(ms / rec["kernel_ms"], 1)
        rec["ms"] = round(ms, 3)
        compose[name] = rec
        del got
        torch.cuda.empty_cache()

    lines = []
    step = {k: float(np.median(v["step_1gen"])) for k, v in (("alone", alone), ("b2b", b2b))}
    for name, fn, *_ in cases:
        rec = {"case": name, "n": n, "rounds": args.rounds}
        if fn is not None:
            for how, ms in (("alone", alone[name]), ("b2b", b2b[name])):
                med = float(np.median(ms))
                rec[how] = {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                            "ratio_to_step": round(med / step[how], 3)}
                if name in KIB_MOVED:
                    rec[how]["GB_per_s"] = round(KIB_MOVED[name] * 1024 * n / med / 1e6, 1)
        if name in compose:
            rec["compose"] = compose[name]
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
