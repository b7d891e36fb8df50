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
points do: flag 4, the object unchanged.
"""
import os
import sys

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


def loop(step, p, x, max_iters=0):
    """PropagateStrip / StabiliseOptionsStrip: flags 0, 1 | changed << 1, | 4 when the bound stopped it"""
    ever = 0
    for _ in range(max_iters or BOUND):
        ok, ch = step(p, x)
        if not ok:
            return 0
        if not ch:
            return 1 | ever
        ever = 2
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


def lookahead_cell(p, x, y, max_iters=0):
    """in place; flags 0, 1 | changed << 1, or 4 (bounded: p is then meaningless)"""
    on, off = p.copy(), p.copy()
    set_cell(on, x, y, True)
    set_cell(off, x, y, False)
    ron, roff = loop(step_strip, on, x, max_iters), loop(step_strip, off, x, max_iters)
    if ron & 4 or (roff & 4):
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


def lookahead_cells(p, c, max_iters=0):
    remaining = c & p[UN]
    any_changes = 0
    while remaining.any():
        x, y = first_on(remaining)
        remaining[x, y] = False
        r = lookahead_cell(p, x, y, max_iters)
        if r == 4 or not r & 1:
            return r & 4
        any_changes |= r & 2
        remaining &= p[UN]
    return 1 | any_changes


def lookahead(planes, cell_words, max_iters=0):
    """TestUnknowns(cells) of (10, 64) words: (planes, flags); flags 4 leaves the planes as given"""
    p = cells(planes)
    fl = lookahead_cells(p, cells(cell_words), max_iters)
    return (np.array(planes, np.uint64) if fl == 4 else words(p)), fl


def zoi(c):
    out = np.zeros_like(c)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            out |= np.roll(c, (dx, dy), (0, 1))
    return out


def vulnerable_zoi(port, planes):
    return words(zoi(cells(port.stable_vulnerable(planes.reshape(1, 640))[0])))


def propagate_and_test(port, planes, max_iters=0):
    """PropagateAndTest of (10, 64) words: (planes, flags)"""
    given = np.array(planes, np.uint64)
    cur, ever = given.copy(), 0
    for _ in range(max_iters or BOUND):
        out, fl = port.stable_pass_bounded(cur.reshape(1, 640), 4, max_iters)
        cur, r = out[0].reshape(10, 64), int(fl[0])
        if r & 4:
            return given, 4
        if not r & 1:
            return cur, 0
        cur, t = lookahead(cur, vulnerable_zoi(port, cur), max_iters)
        if t & 4:
            return given, 4
        if not t & 1:
            return cur, 0
        if not (r | t) & 2:
            return cur, 1 | ever
        ever = 2
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
    return Recording()


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
