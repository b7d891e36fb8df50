"""CPU: numpy definitions of the six LifeStable strip passes (LifeStable.hpp:
921-948, 995-1249), Join (:217-233), TestUnknown (:1251-1284), TestUnknowns
(:1321-1338) and PropagateAndTest (:163-184), pinned to every answer the
reference recorded in tests/golden/stable_test.npz.

They work on cell arrays and integer neighbour counts of the six gathered strip
columns, not on bit planes or lane masks, so they share nothing with the kernels
but the definitions (and the three espresso fragments' recorded truth tables,
tests/golden/stable_*_tt.npz).  The full Propagate and Vulnerable inside
PropagateAndTest are the existing oracle's; where strip and full passes meet
(SynchroniseStateKnown on the strip's six columns, UpdateOptions on its inner
four, on objects both find consistent) they must agree.

`max_iters` bounds Propagate, PropagateStrip and the outer loop as the entry
points do: flag 4, the object unchanged.  The bound is this project's own, so
the reference recorded nothing about it: the bounded strip loops are pinned to
k explicit applications of the steps that the recording does pin
(test_bounded_strip_loop_is_k_steps), and the bounded lookaheads to the
recording wherever the bound is not reached.  bounded_strips,
bounded_unknowns and bounded_propagate_and_test compute, once per process,
what the GPU tests compare against, and test_bounded_*_cover_* proves here,
without a GPU, that those sets reach every place a bounded run can stop.

Where a bounded PropagateAndTest can stop, and what reaches it:
  * a Propagate in round 1; a PropagateStrip in round 1, at TestUnknowns' first
    cell and at a later one; a PropagateStrip in round 2 or later: many of the
    recorded objects at max_iters 2, 3, 4 and 6;
  * a Propagate in round 2 or later: of the recorded objects only number 249
    (object 3821 of the family), at max_iters = 8, in round 2.  An unbounded
    run of all 5981 objects of stable_test_cases.DRAWN with region < 3, noting
    every loop's iterations, finds no other at any max_iters: the first
    Propagate is nearly always the deepest;
  * the outer loop running out (propagate_and_test's final `return 4`): no
    object of that family at any max_iters -- an inner loop always needs more
    iterations than the outer loop needs rounds.  The second family,
    stable_test_cases.dense (more cells known, so short lookaheads and many
    rounds), has two among its first 4290: DENSE_OUTER, 7 and 10 rounds.
"""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stable_test_cases as C  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ST, UN, L2, L3, D0, D6 = 0, 1, 2, 3, 4, 9
BOUND = 1 << 20


def cells(words):
    w = np.ascontiguousarray(words, np.uint64)
    return ((w[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool)


def words(c):
    return (c.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(axis=-1, dtype=np.uint64)


_TT = {}


def table(name):
    if name not in _TT:
        _TT[name] = np.load(os.path.join(GOLDEN, f"stable_{name}_tt.npz"))["tt"].astype(bool)
    return _TT[name]


def lookup(name, inputs):
    """the fragment's outputs for bool input arrays (input i = bit i of the row)"""
    row = np.zeros(inputs[0].shape, np.int64)
    for i, a in enumerate(inputs):
        row |= a.astype(np.int64) << i
    return table(name)[:, row]


def bits(n, k):
    return [((n >> i) & 1).astype(bool) for i in k]


def inner_count(a):
    """(6, 64) strip -> the 3 x 3 counts (centre included) of its inner four columns"""
    v = a.astype(np.int64)
    v = v + np.roll(v, 1, 1) + np.roll(v, -1, 1)
    return v[0:4] + v[1:5] + v[2:6]


def strip_columns(x):
    return (x - 2 + np.arange(6)) % 64


# ---- the strip passes, in place on p = (10, 64, 64) bool [plane, x, y] ------------
# each returns (consistent, changed)

def sync_strip(p, x):
    i = strip_columns(x)
    s = p[:, i]
    known_on, known_off = ~s[UN] & s[ST], ~s[UN] & ~s[ST]
    maybe_dead, maybe_live = ~s[D0:].all(0), ~(s[L2] & s[L3])
    changes = (maybe_dead & known_on) | (maybe_live & known_off)
    s[D0:] |= known_on
    s[L2:D0] |= known_off
    changes |= ~s[ST] & maybe_live & ~maybe_dead
    s[ST] |= maybe_live & ~maybe_dead
    changes |= ~s[UN] & maybe_live & maybe_dead
    s[UN] &= maybe_live & maybe_dead
    p[:, i] = s            # every column is finished before the abort is reported
    return not (~maybe_live & ~maybe_dead).any(), bool(changes.any())


def options_strip(p, x):
    i = strip_columns(x)
    st, un = p[ST][i], p[UN][i]
    off = ~un & ~st
    r = lookup("count", bits(inner_count(st), (2, 1, 0)) + bits(inner_count(off), (3, 2, 1, 0)) + [st[1:5], off[1:5]])
    j = i[1:5]
    changes = (r[:8] & ~p[L2:, j]).any()
    p[L2:, j] |= r[:8]
    return not r[8].any(), bool(changes)


def signal_strip(p, x):
    i = strip_columns(x)
    st, un = p[ST][i], p[UN][i]
    j = i[1:5]
    r = lookup("signal", list(p[L2:, j]) + bits(inner_count(st), (2, 1, 0)) + bits(inner_count(st | un), (3, 2, 1, 0))
               + [st[1:5], un[1:5]])
    sig = np.zeros((2, 6, 64), bool)
    for k in (0, 1):                      # off, on: the signal to the eight neighbours, the centre's own
        s = r[k]
        tall = s | np.roll(s, 1, 1) | np.roll(s, -1, 1)
        sig[k, 0:4] |= tall
        sig[k, 2:6] |= tall
        sig[k, 1:5] |= np.roll(s, 1, 1) | np.roll(s, -1, 1) | r[2 + k]
    if (sig[0] & sig[1] & un).any():
        return False, False               # before anything is written
    off, on = sig[0] & un, sig[1] & un
    p[ST][i] = (st & ~off) | on
    p[UN][i] = un & ~(off | on)
    p[L2:D0, i] |= off
    p[D0:, i] |= on
    return True, bool((off | on).any())


def step_strip(p, x):
    changed = False
    for f in (sync_strip, options_strip, signal_strip):
        ok, ch = f(p, x)
        if not ok:
            return False, False
        changed |= ch
    return True, changed


def stabilise_step(p, x):
    changed = False
    for f in (sync_strip, options_strip):
        ok, ch = f(p, x)
        if not ok:
            return False, False
        changed |= ch
    return True, changed


def loop(step, p, x, max_iters=0, trace=None):
    """PropagateStrip / StabiliseOptionsStrip: flags 0, 1 | changed << 1, | 4 when the bound stopped it
    (`trace`, a list, then takes a stop: see propagate_and_test)"""
    ever = 0
    for _ in range(max_iters or BOUND):
        ok, ch = step(p, x)
        if not ok:
            return 0
        if not ch:
            return 1 | ever
        ever = 2
    if trace is not None:
        trace.append({"site": "strip", "round": 0, "cells": 0})
    return 1 | ever | 4


def strip_pass(planes, x, which, max_iters=0):
    """pass `which` (0..5) at column x of (10, 64) words: (planes, flags)"""
    p = cells(planes)
    if which < 4:
        ok, ch = (sync_strip, options_strip, signal_strip, step_strip)[which](p, int(x))
        fl = int(ok) | int(ch) << 1
    else:
        fl = loop(step_strip if which == 4 else stabilise_step, p, int(x), max_iters)
    return words(p), fl


# ---- the lookahead -------------------------------------------------------------

def set_cell(p, x, y, on):
    p[ST, x, y], p[UN, x, y] = on, False
    if on:
        p[D0:, x, y] = True
    else:
        p[L2:D0, x, y] = True


def join(a, b):
    out = a & b                                   # an option stays ruled out where both rule it out
    out[UN] = a[UN] | b[UN] | (a[ST] ^ b[ST])
    out[ST] = a[ST] & ~out[UN]
    return out


def first_on(c):
    """FirstOn (LifeAPI.hpp:301-323): the LAST populated group of four columns, its first
    populated column, that column's lowest row"""
    cols = np.flatnonzero(c.any(1))
    quad = cols[-1] & ~3
    x = cols[cols >= quad][0]
    return int(x), int(np.flatnonzero(c[x])[0])


def lookahead_cell(p, x, y, max_iters=0, trace=None):
    """in place; flags 0, 1 | changed << 1, or 4 (bounded: p is then meaningless).  A stop is
    traced once, with `trials` = (the on-trial was stopped, the off-trial was stopped)."""
    on, off = p.copy(), p.copy()
    set_cell(on, x, y, True)
    set_cell(off, x, y, False)
    stops = []
    ron, roff = loop(step_strip, on, x, max_iters, stops), loop(step_strip, off, x, max_iters, stops)
    if ron & 4 or (roff & 4):
        if trace is not None:
            trace.append(dict(stops[0], trials=(bool(ron & 4), bool(roff & 4))))
        return 4
    if not ron & 1:                    # forced off: inside the object itself, consistent or not
        p[:] = off
        return 3 if roff & 1 else 0
    if not roff & 1:                   # forced on
        p[:] = on
        return 3
    if ron & roff & 2:
        j = join(on, off)
        changed = bool((j != p).any())
        p[:] = j
        return 1 | changed << 1
    return 1


def lookahead_cells(p, c, max_iters=0, trace=None):
    remaining = c & p[UN]
    any_changes = 0
    tested = 0
    while remaining.any():
        x, y = first_on(remaining)
        remaining[x, y] = False
        r = lookahead_cell(p, x, y, max_iters, trace)
        if r == 4 or not r & 1:
            if r == 4 and trace is not None:
                trace[-1]["cells"] = tested
            return r & 4
        tested += 1
        any_changes |= r & 2
        remaining &= p[UN]
    return 1 | any_changes


def lookahead(planes, cell_words, max_iters=0, trace=None):
    """TestUnknowns(cells) of (10, 64) words: (planes, flags); flags 4 leaves the planes as given"""
    p = cells(planes)
    fl = lookahead_cells(p, cells(cell_words), max_iters, trace)
    return (np.array(planes, np.uint64) if fl == 4 else words(p)), fl


def zoi(c):
    out = np.zeros_like(c)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            out |= np.roll(c, (dx, dy), (0, 1))
    return out


def vulnerable_zoi(port, planes):
    return words(zoi(cells(port.stable_vulnerable(planes.reshape(1, 640))[0])))


def propagate_and_test(port, planes, max_iters=0, trace=None):
    """PropagateAndTest of (10, 64) words: (planes, flags).

    `trace`, a list, takes one entry per call, a dict of
      site    where the run ended: "propagate" (the bound stopped a Propagate), "strip" (a
              PropagateStrip of a TestUnknown; `trials` = which of its two), "outer" (the outer
              loop ran out), or "finished" (flags other than 4);
      round   the outer round it ended in, from 1;
      cells   the cells TestUnknowns had finished in that round before a "strip" stop."""
    def note(site, rnd):
        if trace is not None:
            trace.append({"site": site, "round": rnd, "cells": 0})

    given = np.array(planes, np.uint64)
    cur, ever = given.copy(), 0
    for rnd in range(1, (max_iters or BOUND) + 1):
        out, fl = port.stable_pass_bounded(cur.reshape(1, 640), 4, max_iters)
        cur, r = out[0].reshape(10, 64), int(fl[0])
        if r & 4:
            note("propagate", rnd)
            return given, 4
        if not r & 1:
            note("finished", rnd)
            return cur, 0
        cur, t = lookahead(cur, vulnerable_zoi(port, cur), max_iters, trace)
        if t & 4:
            if trace is not None:
                trace[-1]["round"] = rnd
            return given, 4
        if not t & 1:
            note("finished", rnd)
            return cur, 0
        if not (r | t) & 2:
            note("finished", rnd)
            return cur, 1 | ever
        ever = 2
    note("outer", max_iters)
    return given, 4


# ---- pinned to the recording ------------------------------------------------------

class Recording:
    def __init__(self):
        z = np.load(os.path.join(GOLDEN, "stable_test.npz"))
        self.kept = z["kept"]
        self.planes, self.columns, self.infos = C.build(self.kept)
        self.counts = z["counts"]
        self.pat, self.pat_flags = z["pat"] ^ self.planes, z["pat_flags"]
        self.tu, self.tu_flags = z["tu"] ^ self.planes, z["tu_flags"]
        # the strip passes start from the object as given (0) and from the "fresh" one (1):
        # after PropagateStep, UpdateOptions and SignalNeighbours, with the state and unknown
        # planes PropagateAndTest ends on: nothing synchronised yet
        self.start = np.stack([self.planes, z["fresh"] ^ self.planes], axis=1)
        self.strip_diff, self.strip_flags = z["strip"], z["strip_flags"]
        self.mean_tested = float(z["drawn_mean_tested"])

    def strip_column(self, u, c):
        return int(self.columns[u]) if c == 7 else C.STRIP_COLUMNS[c]

    def strip(self, u, v, c, which):
        """the recorded planes of pass `which` at the c-th column of object u, start v"""
        out = self.start[u, v].copy()
        out[:, strip_columns(self.strip_column(u, c))] ^= self.strip_diff[u, v, c, which]
        return out


@pytest.fixture(scope="module")
def rec():
    return recording()


def test_recording_is_not_vacuous(rec):
    c = rec.counts.astype(np.int64)
    assert len(rec.kept) <= 256 and rec.planes.shape == (len(rec.kept), 10, 64)
    assert (c[:, 2] > 0).sum() >= 8 and (c[:, 3] > 0).sum() >= 8 and (c[:, 4] > 0).sum() >= 8
    assert (c[:, 5] > 0).sum() >= 4 and (c[:, 6] > 0).sum() >= 4 and (c[:, 7] >= 3).sum() >= 4
    assert sum(i["straddles"] for i in rec.infos) >= 16
    assert (rec.pat_flags == c[:, 0]).all()


@pytest.mark.parametrize("which", range(6))
def test_strip_passes_match_the_recording(rec, which):
    assert rec.strip_diff[:, :, :, which].any()
    for u in range(0, len(rec.kept), 2):
        for v in (0, 1):
            for c in range(8):
                got, fl = strip_pass(rec.start[u, v], rec.strip_column(u, c), which)
                assert fl == rec.strip_flags[u, v, c, which], (u, v, c)
                assert (got == rec.strip(u, v, c, which)).all(), (u, v, c)


def test_fresh_start_is_the_oracles(rec, port):
    out = rec.planes.reshape(-1, 640)
    for which in (3, 1, 2):
        out, _ = port.stable_pass(out, which)
    out = out.reshape(-1, 10, 64)
    out[:, :2] = rec.pat[:, :2]
    assert (out.reshape(-1, 10, 64) == rec.start[:, 1]).all()


def test_test_unknowns_matches_the_recording(rec, port):
    after, _ = port.stable_pass(rec.planes.reshape(-1, 640), 4)
    for u in range(len(rec.kept)):
        cur = after[u].reshape(10, 64)
        got, fl = lookahead(cur, vulnerable_zoi(port, cur))
        assert fl == rec.tu_flags[u], u
        assert (got == rec.tu[u]).all(), u


def test_propagate_and_test_matches_the_recording(rec, port):
    for u in range(len(rec.kept)):
        got, fl = propagate_and_test(port, rec.planes[u])
        assert fl == rec.pat_flags[u], u
        assert (got == rec.pat[u]).all(), u


def test_strip_meets_the_full_passes(rec, port):
    """SynchroniseStateKnown on the strip's six columns and UpdateOptions on its inner four
    are the oracle's full passes there, wherever both are consistent"""
    met = 0
    for which, inner in ((0, slice(0, 6)), (1, slice(1, 5))):
        for v in (0, 1):
            full, ffl = port.stable_pass(rec.start[:, v].reshape(-1, 640), which)
            for u in range(len(rec.kept)):
                for c in (0, 7):
                    cols = strip_columns(rec.strip_column(u, c))[inner]
                    if rec.strip_flags[u, v, c, which] & 1 and ffl[u] & 1:
                        want = full[u].reshape(10, 64)[:, cols]
                        assert (rec.strip(u, v, c, which)[:, cols] == want).all(), (which, u, v, c)
                        met += 1
    assert met > 400


def test_bound_leaves_the_object(rec, port):
    """max_iters = 1: every object whose first Propagate step changes something is flagged 4 and
    left as given; with the bound lifted the same objects match the recording"""
    hit = 0
    for u in range(0, len(rec.kept), 4):
        got, fl = propagate_and_test(port, rec.planes[u], max_iters=1)
        if fl == 4:
            assert (got == rec.planes[u]).all()
            hit += 1
        else:
            assert fl == rec.pat_flags[u] and (got == rec.pat[u]).all()
    assert hit >= 8


# ---- the bound: what the GPU tests compare against, computed once per process -------

BOUNDS = (1, 2, 3, 4)
PAT_BOUNDS = (2, 3, 4, 6, 8, 9, 10)     # 10: the first at which nothing below is stopped
DENSE = tuple(sorted({i for i, _ in C.DENSE_OUTER}))


@functools.lru_cache(maxsize=None)
def recording():
    return Recording()


@functools.lru_cache(maxsize=None)
def own_strips():
    """every recorded object and start, row 2u + v, at the object's own column: (starts (2n, 10,
    64), columns (2n,), the recorded (planes, flags) of each of the six passes)"""
    rec = recording()
    want = [(np.stack([rec.strip(u, v, 7, which) for u in range(len(rec.kept)) for v in (0, 1)]),
             rec.strip_flags[:, :, 7, which].reshape(-1)) for which in range(6)]
    return rec.start.reshape(-1, 10, 64), np.repeat(rec.columns, 2), want


@functools.lru_cache(maxsize=None)
def bounded_strips():
    """[which, k] = (planes (2n, 10, 64), flags (2n,)) of pass `which` (4, 5) under max_iters = k
    (BOUNDS) on own_strips()' starts and columns; ["columns"] = (planes
    (2n, 7, 10, 64), flags (2n, 7)) of pass 4 under max_iters = 2 at the seven STRIP_COLUMNS"""
    starts, columns, _ = own_strips()
    out = {}
    for which in (4, 5):
        for k in BOUNDS:
            got = [strip_pass(s, x, which, k) for s, x in zip(starts, columns)]
            out[which, k] = np.stack([g[0] for g in got]), np.array([g[1] for g in got], np.uint8)
    got = [strip_pass(s, x, 4, 2) for s in starts for x in C.STRIP_COLUMNS]
    out["columns"] = (np.stack([g[0] for g in got]).reshape(len(starts), 7, 10, 64),
                      np.array([g[1] for g in got], np.uint8).reshape(len(starts), 7))
    return out


@functools.lru_cache(maxsize=None)
def bounded_unknowns(port):
    """TestUnknowns under max_iters = k (BOUNDS) after a Propagate, on every third recorded
    object that is not a whole torus: want["per", k] with each object's own Vulnerable().ZOI()
    (the recording's call), want["one", k] with every cell of the torus, the same for all; each
    (planes, flags, stops), stops[j] the trace's entry of a stopped object, else None"""
    rec = recording()
    pick = np.array([u for u, info in enumerate(rec.infos) if info["region"] < 3][::3])
    after, _ = port.stable_pass(rec.planes[pick].reshape(-1, 640), 4)
    after = after.reshape(-1, 10, 64)
    b = SimpleNamespace(pick=pick, after=after, per=np.stack([vulnerable_zoi(port, p) for p in after]),
                        one=np.full(64, ~np.uint64(0), np.uint64), want={})
    for k in BOUNDS:
        for form in ("per", "one"):
            planes, flags, stops = [], [], []
            for j in range(len(pick)):
                trace = []
                pl, fl = lookahead(after[j], b.per[j] if form == "per" else b.one, k, trace)
                planes.append(pl)
                flags.append(fl)
                stops.append(trace[0] if trace else None)
            b.want[form, k] = np.stack(planes), np.array(flags, np.uint8), stops
    return b


@functools.lru_cache(maxsize=None)
def bounded_propagate_and_test(port):
    """PropagateAndTest under max_iters = k (PAT_BOUNDS) on every recorded object that is not a
    whole torus (`pick`) and then the objects DENSE of the second family: `given`, and per k
    want[k] = (planes, flags, ends), ends[j] the trace's entry.  A run that a bound did not stop
    is the same run under every larger bound, so only the objects that the bound before stopped
    are run again.  `free` = (planes, flags) with no bound: the recording, and the model for
    DENSE."""
    rec = recording()
    pick = np.array([u for u, info in enumerate(rec.infos) if info["region"] < 3])
    dense = np.stack([C.dense(i)[0] for i in DENSE])
    free = [propagate_and_test(port, p) for p in dense]
    b = SimpleNamespace(pick=pick, given=np.concatenate([rec.planes[pick], dense]), want={},
                        free=(np.concatenate([rec.pat[pick], np.stack([f[0] for f in free])]),
                              np.concatenate([rec.pat_flags[pick], np.array([f[1] for f in free], np.uint8)])))
    last = None
    for k in PAT_BOUNDS:
        planes, flags, ends = [], [], []
        for j, p in enumerate(b.given):
            if last is not None and last[1][j] != 4:
                pl, fl, end = last[0][j], last[1][j], last[2][j]
            else:
                trace = []
                pl, fl = propagate_and_test(port, p, k, trace)
                end, = trace
            planes.append(pl)
            flags.append(fl)
            ends.append(end)
        last = b.want[k] = np.stack(planes), np.array(flags, np.uint8), ends
    return b


@pytest.mark.parametrize("which", (4, 5))
def test_bounded_strip_loop_is_k_steps(rec, which):
    """strip_pass(.., 4 | 5, max_iters = k) is k applications of the step that pass 3 (and 0, 1)
    pin to the recording, by the flag rules of lifeapi_stable_pass_batch_dev: 7 while every
    iteration so far changed something, the confirming iteration included in the count; 0 from
    the inconsistent iteration on; from the last iteration on, the recorded pass"""
    step = step_strip if which == 4 else stabilise_step
    depths = set()
    for u in range(len(rec.kept)):
        for v in (0, 1):
            x = int(rec.columns[u])
            p, after = cells(rec.start[u, v]), []
            while not after or after[-1][1:] == (True, True):
                ok, ch = step(p, x)
                after.append((words(p), ok, ch))
            m = len(after)
            depths.add(m)
            assert rec.strip_flags[u, v, 7, which] == (after[-1][1] and 1 | 2 * (m > 1)), (u, v)
            assert (rec.strip(u, v, 7, which) == after[-1][0]).all(), (u, v)
            for k in range(1, m + 2):
                got, fl = strip_pass(rec.start[u, v], x, which, k)
                assert fl == (7 if k < m else rec.strip_flags[u, v, 7, which]), (u, v, k)
                assert (got == after[min(k, m) - 1][0]).all(), (u, v, k)
    assert {1, 2, 3, 4} <= depths


@pytest.mark.parametrize("which", (4, 5))
def test_bounded_strips_cover_every_flag(rec, which):
    """what the GPU tests of the bounded strip passes rely on: stopped, finished and
    inconsistent objects at every max_iters below 4, none stopped at 4"""
    want = bounded_strips()
    recorded = rec.strip_flags[:, :, 7, which].reshape(-1)
    for k in (1, 2, 3):
        fl = want[which, k][1]
        assert (fl == 7).any() and ((fl == 3) | (fl == 1)).any() and (fl == 0).any(), (k, np.bincount(fl))
        assert ((fl == 7) | (fl == recorded)).all()
    planes, fl = want[which, 4]
    assert (fl == recorded).all() and (planes == own_strips()[2][which][0]).all()
    if which == 4:
        fl = want["columns"][1]
        assert all((fl == f).sum() >= 8 for f in (0, 1, 3, 7)), np.bincount(fl.reshape(-1))


def stop_cells(stops):
    """(stopped at TestUnknowns' first cell, at a later one): the rows"""
    return ([j for j, s in enumerate(stops) if s and s["cells"] == 0],
            [j for j, s in enumerate(stops) if s and s["cells"] > 0])


def test_bounded_unknowns_cover_both_cells(rec, port):
    """what the GPU test of the bounded TestUnknowns relies on: stops at the first cell and at a
    later one, in the on-trial alone and in the off-trial alone, next to objects that are not
    stopped; those equal the recording"""
    b = bounded_unknowns(port)
    trials = {(late, t): 0 for late in (False, True) for t in ((True, False), (False, True))}
    for (form, k), (planes, flags, stops) in b.want.items():
        first, later = stop_cells(stops)
        assert len(first) >= 2, (form, k)
        assert len(later) >= 2 or k == 1, (form, k)     # (at 1 the first cell stops all that any stops)
        assert ((flags == 4) == np.array([s is not None for s in stops])).all()
        assert (planes[flags == 4] == b.after[flags == 4]).all()
        assert (flags != 4).sum() >= 2, (form, k)
        for s in stops:
            if s and s["trials"] in ((True, False), (False, True)):
                trials[s["cells"] > 0, s["trials"]] += 1
        if form == "per":
            free = flags != 4
            assert (flags[free] == rec.tu_flags[b.pick][free]).all() and (planes[free] == rec.tu[b.pick][free]).all()
    assert min(trials.values()) >= 2, trials
    assert len(b.pick) >= 60 and {3, 1, 0} <= set(b.want["per", 4][1])


def pat_sites(b):
    """{site: the rows of b.given that end there under some bound of PAT_BOUNDS}"""
    sites = {}
    for k, (_, _, ends) in b.want.items():
        for j, e in enumerate(ends):
            if e["site"] == "strip":
                key = ("strip", min(e["round"], 2), "first" if e["cells"] == 0 else "later")
                key = key[:2] if key[1] == 2 else key
            else:
                key = (e["site"], e["round"] if e["site"] == "finished" else min(e["round"], 2))
            key = ("outer",) if e["site"] == "outer" else key
            sites.setdefault(key, set()).add(j)
    return sites


def test_bounded_propagate_and_test_covers_every_stop(rec, port):
    """what the GPU test of the bounded PropagateAndTest relies on: every place a bounded run can
    stop, each in at least two objects (a Propagate past round 1: the one object there is), and
    runs that finish in 2, 3 and 4 rounds; a stopped object is as given, a finished one the
    unbounded one, whatever the bound; max_iters = 10 stops nothing and 9 still does"""
    b = bounded_propagate_and_test(port)
    sites = pat_sites(b)
    for key in (("propagate", 1), ("strip", 1, "first"), ("strip", 1, "later"), ("strip", 2), ("outer",),
                ("finished", 2), ("finished", 3), ("finished", 4)):
        assert len(sites.get(key, ())) >= 2, (key, sites.get(key))
    assert len(sites[("propagate", 2)]) >= 1
    assert sites[("outer",)] == {len(b.pick) + j for j in range(len(DENSE))}
    for k, (planes, flags, ends) in b.want.items():
        stopped = flags == 4
        assert (stopped == np.array([e["site"] != "finished" for e in ends])).all()
        assert (planes[stopped] == b.given[stopped]).all()
        assert (flags[~stopped] == b.free[1][~stopped]).all() and (planes[~stopped] == b.free[0][~stopped]).all()
        for i, at in C.DENSE_OUTER:
            if at == k:
                assert ends[len(b.pick) + DENSE.index(i)] == {"site": "outer", "round": k, "cells": 0}
    assert not (b.want[10][1] == 4).any() and (b.want[9][1] == 4).any()
    assert max(e["round"] for e in b.want[10][2]) >= 10
