#!/usr/bin/env python3
"""Host-pointer path (lifeapi_step_batch on pageable numpy arrays, the C++
facade's StepBatch; the host Contains and Step+Contains calls) against the
PCIe copy rates torch gets for the same bytes (pageable and pinned, each
direction).  One JSON line per case.  LIFEAPI_HIP_LIB=<another build of the
library> measures that build instead (an A/B runs the two alternately).
`host_bench.py enqueue` measures the host cost per *_dev call instead
(enqueue, below)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lifeapi_amd.hip as hip  # noqa: E402


def wall(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2]


def enqueue(n=64, calls=20000):
    """The host cost of one *_dev call: `calls` calls on a batch of n back to
    back on the current stream, a host clock around the loop, one synchronise
    after it and none inside.  At 64 universes the kernels take a few
    microseconds, so the loop measures what the library does on the host to
    enqueue a launch (through ctypes: the same for every build)."""
    L, st = hip.lib, hip._stream(None)
    zeros = lambda words: torch.zeros(words, dtype=torch.int64, device="cuda")  # noqa: E731
    x, y, w, u = hip.fill_random(n, seed=5), zeros(n * 64), zeros(64), zeros(64)
    first, pop, flags = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3))
    planes, welds = zeros(n * 640), zeros(n * 256)
    p = lambda t: t.data_ptr()  # noqa: E731
    contains = lambda final, gens: lambda: L.lifeapi_step_contains_batch_dev(  # noqa: E731
        p(x), final, p(w), p(u), p(first), n, gens, st)
    cases = [("step_1gen", lambda: L.lifeapi_step_batch_dev(p(x), p(y), n, 1, st)),
             ("step_8gen", lambda: L.lifeapi_step_batch_dev(p(x), p(y), n, 8, st)),
             ("filter_cone_2gen", contains(None, 2)), ("filter_iterated_8gen", contains(None, 8)),
             ("final_split_pair_8gen", contains(p(y), 8)), ("final_stream_2gen", contains(p(y), 2)),
             ("stable_pass_0", lambda: L.lifeapi_stable_pass_batch_dev(p(planes), p(flags), n, 0, 0, st)),
             ("stable_pass_4", lambda: L.lifeapi_stable_pass_batch_dev(p(planes), p(flags), n, 4, 0, st)),
             ("weld_1gen", lambda: L.lifeapi_weld_step_batch_dev(p(welds), n, 1, st)),
             ("pop", lambda: L.lifeapi_pop_batch_dev(p(x), p(pop), n, st))]
    for case, fn in cases:
        hip._check(fn())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bad = 0
        for _ in range(calls):
            bad |= fn()
        t = time.perf_counter() - t0
        torch.cuda.synchronize()
        t_done = time.perf_counter() - t0  # (with the queue drained: the larger of the host's and the GPU's time)
        hip._check(bad)
        print(json.dumps({"case": "enqueue_" + case, "universes": n, "calls": calls, "us_per_call": 1e6 * t / calls,
                          "us_per_call_drained": 1e6 * t_done / calls}), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "enqueue":  # host_bench.py enqueue [universes [calls]]
        return enqueue(*(int(a) for a in sys.argv[2:4]))
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
    rng = np.random.default_rng(5)
    x = rng.integers(0, 2**63, size=(n, 64), dtype=np.uint64)
    nbytes = x.nbytes
    dev = torch.empty(n * 64, dtype=torch.int64, device="cuda")
    out = np.zeros_like(x)  # touched: no page faults inside the timed calls
    reps = 3 if n > (1 << 16) else 101  # a small n measures the call's latency: more repeats
    # the host search calls, whose target is staged with each chunk: Contains,
    # and Step + Contains over 2 generations without final states.
    w, u = np.zeros(64, np.uint64), np.zeros(64, np.uint64)
    w[20] = w[21] = np.uint64(0b11 << 30)
    u[19] = u[22] = np.uint64(0b1111 << 29)
    hit = np.zeros(n, np.uint8)

    def contains_host():
        hip._check(hip.lib.lifeapi_contains_batch(x.ctypes.data, w.ctypes.data, u.ctypes.data,
                                                  hit.ctypes.data, n, 0))
    for case, gens, fn in (("contains_host", 0, contains_host),
                           ("step_contains_host", 2, lambda: hip.step_contains_host(x, w, u, 2))):
        t = wall(fn, reps)
        print(json.dumps({"case": case, "universes": n, "gens": gens, "s": t, "universes_per_s": n / t}),
              flush=True)
    for gens in (1, 1024):
        if gens == 1024 and n > (1 << 16):
            continue
        for case, kw in (("step_host", {"out": out}), ("step_host_inplace", {"out": x}),
                         ("step_host_fresh_out", {})):
            t = wall(lambda: hip.step_host(x, generations=gens, **kw), reps)
            print(json.dumps({"case": case, "universes": n, "gens": gens, "s": t,
                              "universe_gen_per_s": n * gens / t,
                              "GBps_round_trip": 2 * nbytes / t / 1e9}), flush=True)
        def pin_each_call():  # registration inside the timed call, as a library-side pin would
            with hip.host_pinned(x, out):
                hip.step_host(x, generations=gens, out=out)
        t = wall(pin_each_call, reps)
        print(json.dumps({"case": "step_host_register_per_call", "universes": n, "gens": gens, "s": t,
                          "universe_gen_per_s": n * gens / t}), flush=True)
        with hip.host_pinned(x, out):  # page-locked once (lifeapi_host_register)
            for case, o in (("step_host_pinned", out), ("step_host_pinned_inplace", x)):
                t = wall(lambda: hip.step_host(x, generations=gens, out=o), reps)
                print(json.dumps({"case": case, "universes": n, "gens": gens, "s": t,
                                  "universe_gen_per_s": n * gens / t,
                                  "GBps_round_trip": 2 * nbytes / t / 1e9}), flush=True)
    xt = torch.from_numpy(x.view(np.int64).reshape(-1))
    pin = xt.pin_memory()
    for name, src, dst in (("h2d_pageable", xt, dev), ("h2d_pinned", pin, dev),
                           ("d2h_pageable", dev, xt), ("d2h_pinned", dev, pin)):
        t = wall(lambda: dst.copy_(src, non_blocking=True))
        print(json.dumps({"case": name, "bytes": nbytes, "s": t, "GBps": nbytes / t / 1e9}), flush=True)
    # both directions at once on two streams: is the link full duplex?
    dev2 = torch.empty_like(dev)
    pin2 = torch.empty_like(pin).pin_memory()
    xt2 = xt.clone()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    cases = [("duplex_pinned", pin, pin2), ("duplex_pageable", xt, xt2)]
    for name, a, b in cases:
        def both():
            with torch.cuda.stream(s1):
                dev.copy_(a, non_blocking=True)
            with torch.cuda.stream(s2):
                b.copy_(dev2, non_blocking=True)
        t = wall(both)
        print(json.dumps({"case": name, "bytes_each_way": nbytes, "s": t,
                          "GBps_total": 2 * nbytes / t / 1e9}), flush=True)


    # the same duplex copy on hipHostRegister-ed (not hipHostMalloc-ed) memory
    with hip.host_pinned(xt.numpy(), xt2.numpy()):
        t = wall(both_fn(dev, dev2, xt, xt2, s1, s2))
        print(json.dumps({"case": "duplex_registered", "bytes_each_way": nbytes, "s": t,
                          "GBps_total": 2 * nbytes / t / 1e9}), flush=True)
    # step_host on hipHostMalloc-ed arrays (torch pinned tensors)
    pa, pb = pin.numpy().view(np.uint64), pin2.numpy().view(np.uint64)
    t = wall(lambda: hip.step_host(pa, generations=1, out=pb))
    print(json.dumps({"case": "step_host_hostmalloc", "universes": n, "s": t,
                      "universe_gen_per_s": n / t, "GBps_round_trip": 2 * nbytes / t / 1e9}), flush=True)


def both_fn(dev, dev2, a, b, s1, s2):
    def both():
        with torch.cuda.stream(s1):
            dev.copy_(a, non_blocking=True)
        with torch.cuda.stream(s2):
            b.copy_(dev2, non_blocking=True)
    return both


if __name__ == "__main__":
    main()
