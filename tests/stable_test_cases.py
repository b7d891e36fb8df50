"""Deterministic inputs of the LifeStable lookahead tests (strip passes,
TestUnknowns, PropagateAndTest): partly known still lifes on the torus.

Object i of the family (numpy's frozen RandomState stream, seeded by i):
  * a small still life moved anywhere on the 64 x 64 torus, one in four pushed
    over the column 63 / 0 seam;
  * a random subset (density 1/4 or 1/8) of the cells within three ZOIs of it
    known, on or off as the pattern has them;
  * `unknown` = one of four regions -- the pattern's ZOI, two ZOIs, three ZOIs,
    the whole torus -- minus the known cells; everything outside is SetOff;
  * in one object of five, one cell of the pattern's boundary wrongly SetOn.
tests/golden/make_stable_test_golden.py draws the family, classifies it on the
reference's outputs and keeps the indices in tests/golden/stable_test.npz
(`kept`); the tests rebuild those objects here.  `dense` draws a second family
that is not recorded; the numpy model alone judges it.

A LifeStable is (10, 64) uint64: {state, unknown, live2, live3, dead0, dead1,
dead2, dead4, dead5, dead6}, word x = column x, bit y = row y, option planes
1 = ruled out (LifeStable.hpp:41-53)."""
import numpy as np

STILL_LIFES = {
    "block": "2o$2o!",
    "beehive": "b2o$o2bo$b2o!",
    "boat": "2o$obo$bo!",
    "long_boat": "2o$obo$bobo$2bo!",
    "snake": "2obo$ob2o!",
    "eater": "2o$obo$2bo$2b2o!",
    "loaf": "b2o$o2bo$bobo$2bo!",
    "tub": "bo$obo$bo!",
    "ship": "2o$obo$b2o!",
    "pond": "b2o$o2bo$o2bo$b2o!",
    "carrier": "2o2b$o2bo$2b2o!",
    "barge": "bo$obo$bobo$2bo!",
}
NAMES = tuple(STILL_LIFES)
STRIP_COLUMNS = (0, 1, 2, 31, 61, 62, 63)   # and the pattern's own column
STRIP_PASSES = ("sync_strip", "options_strip", "signal_strip", "step_strip", "propagate_strip", "stabilise_strip")
DRAWN = 8000        # the family the recorder draws from


def cells(rle):
    """the (x, y) cells of an RLE"""
    out, x, y, run = [], 0, 0, 0
    for ch in rle:
        if ch.isdigit():
            run = run * 10 + int(ch)
            continue
        k = run or 1
        run = 0
        if ch == "o":
            out += [(x + j, y) for j in range(k)]
            x += k
        elif ch == "b":
            x += k
        elif ch == "$":
            y += k
            x = 0
        elif ch == "!":
            break
    return out


def pack(a):
    """(64, 64) bool [x, y] -> (64,) uint64"""
    return np.packbits(np.asarray(a, bool), axis=1, bitorder="little").view("<u8").reshape(64).astype(np.uint64)


def unpack(w):
    """(64,) uint64 -> (64, 64) bool [x, y]"""
    return np.unpackbits(np.ascontiguousarray(w, "<u8").view(np.uint8).reshape(64, 8), axis=1, bitorder="little").astype(bool)


def zoi(a):
    out = np.zeros_like(a)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            out |= np.roll(np.roll(a, dx, 0), dy, 1)
    return out


def one(i):
    """object i: (planes (10, 64) uint64, column, info)"""
    rs = np.random.RandomState(977 * i + 13)
    name = NAMES[i % len(NAMES)]
    pat = cells(STILL_LIFES[name])
    width = 1 + max(x for x, _ in pat)
    dx = (64 - 1 - rs.randint(width - 1)) if rs.randint(4) == 0 else rs.randint(64)
    dy = rs.randint(64)
    p = np.zeros((64, 64), bool)
    for x, y in pat:
        p[(x + dx) % 64, (y + dy) % 64] = True
    density = (0.25, 0.125)[rs.randint(2)]
    z1 = zoi(p)
    z2 = zoi(z1)
    z3 = zoi(z2)
    known = (rs.random_sample((64, 64)) < density) & z3
    which = rs.randint(4)
    region = (z1, z2, z3, np.ones((64, 64), bool))[which]
    on = known & p
    off = ~region | (known & ~p)
    state, unknown = on.copy(), region & ~known
    live, dead = off.copy(), on.copy()
    wrong = None
    if rs.randint(5) == 0:
        boundary = np.argwhere(z1 & ~p)
        x, y = boundary[rs.randint(len(boundary))]
        wrong = (int(x), int(y))
        state[x, y], unknown[x, y], dead[x, y] = True, False, True
    planes = np.stack([pack(state), pack(unknown), pack(live), pack(live)] + [pack(dead)] * 6)
    info = {"name": name, "dx": int(dx), "dy": int(dy), "region": int(which), "wrong": wrong,
            "straddles": bool(p[63].any() and p[0].any())}
    return planes, int(dx % 64), info


def dense(i):
    """object i (< DENSE_DRAWN) of a second family, not recorded: more of the neighbourhood
    known (density 0.4 .. 0.85), never the whole torus unknown, no wrong cell.  Its lookaheads
    are short and its PropagateAndTest takes many rounds, so a `max_iters` can run out in the
    outer loop before any inner loop reaches it (DENSE_OUTER): no object of the first family
    does that.  (planes (10, 64) uint64, column, info)"""
    rs = np.random.RandomState(1000003 * (i + 1) + 7)
    name = NAMES[i % len(NAMES)]
    dx, dy = rs.randint(64), rs.randint(64)
    p = np.zeros((64, 64), bool)
    for x, y in cells(STILL_LIFES[name]):
        p[(x + dx) % 64, (y + dy) % 64] = True
    density = (0.4, 0.55, 0.7, 0.85)[rs.randint(4)]
    z1 = zoi(p)
    z2 = zoi(z1)
    z3 = zoi(z2)
    known = (rs.random_sample((64, 64)) < density) & z3
    which = rs.randint(3)
    region = (z1, z2, z3)[which]
    on = known & p
    off = ~region | (known & ~p)
    unknown = region & ~known
    planes = np.stack([pack(on), pack(unknown), pack(off), pack(off)] + [pack(on)] * 6)
    return planes, int(dx), {"name": name, "dx": int(dx), "dy": int(dy), "region": int(which)}


DENSE_DRAWN = 4000
# (object, max_iters) of the second family at which PropagateAndTest's outer loop runs out: that
# many rounds each change something and no Propagate or PropagateStrip in them needs more
# iterations (found by running the model unbounded over the whole family and comparing each
# object's rounds with the iterations of its deepest inner loop so far)
DENSE_OUTER = ((1918, 6), (1881, 7), (1881, 8), (1881, 9))


def build(indices):
    """(planes (n, 10, 64), columns (n,) uint8, infos) of the objects `indices`"""
    got = [one(int(i)) for i in indices]
    return (np.stack([g[0] for g in got]), np.array([g[1] for g in got], np.uint8), [g[2] for g in got])
