"""Deterministic inputs of the CompleteStable tests: the known part of a still
life on the torus, the rest to be found.

Object i of the family (numpy's frozen RandomState stream, seeded by i), one of
three kinds (i % 3):
  0  as tests/stable_test_cases.py: a small still life anywhere on the torus,
     a random subset of the cells within three ZOIs of it known, `unknown` =
     the pattern's ZOI, two ZOIs, three ZOIs or the whole torus minus the known
     cells, everything outside SetOff; one object in four carries one cell of
     the pattern's boundary wrongly SetOn;
  1  the same with half or three quarters of the neighbourhood known (short
     searches, and many that are inconsistent at the root when a cell is wrong);
  2  only a few cells of the pattern known (two to five of its ON cells and as
     many OFF cells next to it), all the rest of a window of three to five
     ZOIs around them unknown: the searches that need several search-area
     rounds and that find more than one completion.
The last IMPROVERS objects of the family are purpose-made for the minimise
pass: two sparse objects (`sparse`: one to three ON cells of a pattern known and a
random tenth to half of the OFF cells within three ZOIs of it, found by a search
over 6000 such draws) whose cheapest completion inside the search area of the
rounds has 7 cells while one with 6 reaches outside it, each moved to twelve
places on the torus, the seams among them.
One object in four sits over the column 63 / 0 seam, one in four over the row
seam.  Every object comes with a seed for the seeded search: a single cell two
to nine cells away from the pattern's corner.

tests/golden/make_stable_complete_golden.py draws the family, classifies it on
the reference's outputs alone and keeps the indices in
tests/golden/stable_complete.npz (`kept`); the tests rebuild those objects here.

A LifeStable is (10, 64) uint64: {state, unknown, live2, live3, dead0, dead1,
dead2, dead4, dead5, dead6}, word x = column x, bit y = row y, option planes
1 = ruled out (LifeStable.hpp:41-53)."""
import numpy as np

from stable_test_cases import NAMES, STILL_LIFES, cells, pack, unpack, zoi  # noqa: F401

RANDOM, IMPROVERS = 3600, 24
DRAWN = RANDOM + IMPROVERS        # the family the recorder draws from
IMPROVER_BASES = (3210, 5632)     # indices into `sparse`
FLAGS = ((False, False), (True, False), (False, True), (True, True))    # (minimise, use_seed), index = flags word


def sparse(i):
    """sparse object i (not part of the family by itself): (state, unknown, known off) as (64, 64) bool"""
    rs = np.random.RandomState(104729 * i + 5)
    pat = cells(STILL_LIFES[NAMES[i % len(NAMES)]])
    dx, dy = rs.randint(64), rs.randint(64)
    p = np.zeros((64, 64), bool)
    for x, y in pat:
        p[(x + dx) % 64, (y + dy) % 64] = True
    z = [p]
    for _ in range(6):
        z.append(zoi(z[-1]))
    on_cells = np.argwhere(p)
    k = 1 + rs.randint(3)
    known = np.zeros((64, 64), bool)
    for x, y in on_cells[rs.permutation(len(on_cells))[:k]]:
        known[x, y] = True
    density = (0.1, 0.2, 0.3, 0.45)[rs.randint(4)]
    known |= (rs.random_sample((64, 64)) < density) & z[3] & ~p
    region = z[4 + rs.randint(3)]
    return known & p, region & ~known, ~region | (known & ~p)


def improver(j):
    """purpose-made object j (< IMPROVERS) for the minimise pass"""
    rs = np.random.RandomState(48611 * j + 3)
    state, unknown, off = sparse(IMPROVER_BASES[j % 2])
    xs, ys = np.nonzero(state)
    tx = (63 - xs.min()) if j % 4 >= 2 else rs.randint(64)        # a known ON cell in column 63 / row 63: the
    ty = (63 - ys.min()) if j % 8 >= 4 else rs.randint(64)        # unknown region around it crosses the seam
    state, unknown, off = (np.roll(a, (tx, ty), (0, 1)) for a in (state, unknown, off))
    planes = np.stack([pack(state), pack(unknown), pack(off), pack(off)] + [pack(state)] * 6)
    s = np.zeros((64, 64), bool)
    s[(xs.min() + tx + 5) % 64, (ys.min() + ty - 4) % 64] = True
    zs = zoi(zoi(state))
    info = {"name": "improver", "kind": 3, "region": 0, "wrong": None,
            "column_seam": bool(zs[63].any() and zs[0].any()), "row_seam": bool(zs[:, 63].any() and zs[:, 0].any())}
    return planes, pack(s), info


def one(i):
    """object i: (planes (10, 64) uint64, seed (64,) uint64, info)"""
    if i >= RANDOM:
        return improver(i - RANDOM)
    rs = np.random.RandomState(7919 * i + 31)
    kind = i % 3
    name = NAMES[(i // 3) % len(NAMES)]
    pat = cells(STILL_LIFES[name])
    width, height = 1 + max(x for x, _ in pat), 1 + max(y for _, y in pat)
    dx = (64 - 1 - rs.randint(width - 1)) if rs.randint(4) == 0 else rs.randint(64)
    dy = (64 - 1 - rs.randint(height - 1)) if rs.randint(4) == 0 else rs.randint(64)
    p = np.zeros((64, 64), bool)
    for x, y in pat:
        p[(x + dx) % 64, (y + dy) % 64] = True
    z = [p]
    for _ in range(5):
        z.append(zoi(z[-1]))
    wrong = None
    if kind < 2:
        density = ((0.25, 0.125), (0.5, 0.75))[kind][rs.randint(2)]
        known = (rs.random_sample((64, 64)) < density) & z[3]
        which = rs.randint(4)
        region = (z[1], z[2], z[3], np.ones((64, 64), bool))[which]
    else:
        on_cells, ring = np.argwhere(p), np.argwhere(z[1] & ~p)
        k = 2 + rs.randint(4)
        known = np.zeros((64, 64), bool)
        for x, y in on_cells[rs.permutation(len(on_cells))[:k]]:
            known[x, y] = True
        for x, y in ring[rs.permutation(len(ring))[:k]]:
            known[x, y] = True
        which = 3 + rs.randint(3)
        region = z[which]
    on = known & p
    off = ~region | (known & ~p)
    state, unknown = on.copy(), region & ~known
    live, dead = off.copy(), on.copy()
    if kind < 2 and rs.randint(4) == 0:
        boundary = np.argwhere(z[1] & ~p)
        x, y = boundary[rs.randint(len(boundary))]
        wrong = (int(x), int(y))
        state[x, y], unknown[x, y], dead[x, y], live[x, y] = True, False, True, False
    planes = np.stack([pack(state), pack(unknown), pack(live), pack(live)] + [pack(dead)] * 6)
    s = np.zeros((64, 64), bool)
    sx, sy = (2 + rs.randint(8)) * (1, -1)[rs.randint(2)], (2 + rs.randint(8)) * (1, -1)[rs.randint(2)]
    s[(dx + sx) % 64, (dy + sy) % 64] = True
    info = {"name": name, "kind": kind, "region": int(which), "wrong": wrong,
            "column_seam": bool(p[63].any() and p[0].any()), "row_seam": bool(p[:, 63].any() and p[:, 0].any())}
    return planes, pack(s), info


def build(indices):
    """(planes (n, 10, 64), seeds (n, 64), infos) of the objects `indices`"""
    got = [one(int(i)) for i in indices]
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got]), [g[2] for g in got]


# ---- UnweldableMask: catalyst pairs (state, required as LifeWeld::FromRequired takes them) ----
# the (state, required) RLEs are those of tests/weld_cases.py; `at`: where the weld sits; the
# placements tested are the offsets of `window` = (x0, y0, w, h) that do not interact
WELD_CASES = (
    ("eater", "eater", (20, 30), (12, 22, 8, 8)),
    ("eater", "block", (20, 30), (15, 25, 8, 8)),
    ("block", "eater", (61, 62), (55, 57, 8, 8)),
    ("eater", "eater", (20, 30), (22, 24, 8, 8)),
)
WELD_BUDGET = 64     # nodes per placement: some placements of every case exhaust it


def weld_inputs(port):
    """per case (state_a, required_a, state_b, required_b, good, bad), each (64,) uint64"""
    import weld_cases as WC
    base = {n: (port.parse(s), WC.moved(port.parse(r), -1, -1)) for n, (s, r) in WC.REFERENCE_PAIRS.items()}
    base["block"] = (port.parse("2o$2o!"), WC.moved(port.parse("2o$2o$2o$2o!"), -1, -1))
    out = []
    for a, b, at, (x0, y0, w, h) in WELD_CASES:
        window = np.zeros((64, 64), bool)
        for x in range(w):
            window[(x0 + x) % 64, [(y0 + y) % 64 for y in range(h)]] = True
        out.append((WC.moved(base[a][0], *at), WC.moved(base[a][1], *at), base[b][0], base[b][1],
                    pack(~window), np.zeros(64, np.uint64)))
    return out
