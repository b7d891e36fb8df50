"""Inputs of the LifeWeld construction family (FromRequired, ToTarget, ToStable,
InteractionOffsets): seeded, deterministic, CPU only, data alone (no model of the
operations).  tests/golden/make_weld_golden.py records the reference's answers
on them (tests/golden/weld_family.npz), tests/test_weld_model.py pins the numpy
definitions to that recording, the facade and GPU tests run on the same inputs.

  pairs(port)            name -> (state, required), the FromRequired inputs:
                           eater, cat2, cat3   the three pairs of the reference's
                                               tests/LifeWeldTest.cpp
                           block, empty
                           <name>_seam         the same moved across column 63/0
                                               and row 63/0
                           soup<k>_<j>         state of density 2^-k, required of
                                               density 2^-j
  welds(port, recorded)  name -> (4, 64) weld: FromRequired of every pair (the
                         recorded answers, in pairs' order), then
                           plain_<name>        a state with no frozen count
                           plain_lattice       ... whose ZOI is the whole torus
                           soupweld<k>_<j>     state of density 2^-k, frozen
                                               planes of density 2^-j
  STABLE_CASES           (weld, active, duration, mask) names of the ToStable cases
  actives(port), masks(port)
  OFFSET_OTHERS, OFFSET_WELDS   the InteractionOffsets cases: every weld of
                         OFFSET_WELDS against every `other`
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "weld_family.npz")
U1 = np.uint64(1)
DURATIONS = (0, 1, 2, 8, 40)


def moved(s, dx, dy):
    """(x, y) -> (x + dx, y + dy) on the torus; s may be (..., 64)"""
    s = np.roll(np.asarray(s, np.uint64), dx, axis=-1)
    dy %= 64
    return s if dy == 0 else (s << np.uint64(dy)) | (s >> np.uint64(64 - dy))


def soup(port, seed, k):
    """one universe of density 2^-k"""
    a = port.fill(k, seed=seed)
    return np.bitwise_and.reduce(a, axis=0)


# the (state, required) pairs of tests/LifeWeldTest.cpp (required is Moved(-1, -1) there)
REFERENCE_PAIRS = {
    "eater": ("2b2o$bobo$bo$2o!", "2b2o$b3o$b4o$5o$4o$4o!"),
    "cat2": ("2o$o2bob2o$b3obobo$5bobo$b5ob3o$bo4bo3bo$4bobo2b2o$4b2o!",
             "4o$5o2bo$4o$5o4bo$b5ob5o$b12o$b12o$b12o$4b9o$4b4o!"),
    "cat3": ("4b2ob2o$3bobobobo$b3o3bobo$o4bobob3o$b3ob2obo3bo$3bo4bo2b2o$5b3o$4b2o!",
             "4b2o$3b2o2bo2b2o$b4o6bo$6obob5o$15o$15o$b14o$3b12o$4b6o$4b4o!"),
}
AT = (20, 30)            # where the interior copies sit
SEAM = (61, 62)          # ... and the ones across both seams
SOUP_PAIRS = ((1, 1), (1, 3), (2, 1), (2, 2), (2, 4), (3, 2), (3, 3), (4, 1))
SOUP_WELDS = ((1, 2), (2, 1), (2, 3), (3, 1), (3, 2), (4, 3))


def pairs(port):
    base = {n: (port.parse(s), moved(port.parse(r), -1, -1)) for n, (s, r) in REFERENCE_PAIRS.items()}
    block = port.parse("2o$2o!")
    base["block"] = (block, moved(port.parse("2o$2o$2o$2o!"), -1, -1))    # the left column and what is left of it
    base["empty"] = (np.zeros(64, np.uint64), np.zeros(64, np.uint64))
    out = {}
    for n, (s, r) in base.items():
        out[n] = (moved(s, *AT), moved(r, *AT))
    for n, (s, r) in base.items():
        out[n + "_seam"] = (moved(s, *SEAM), moved(r, *SEAM))
    for i, (k, j) in enumerate(SOUP_PAIRS):
        out[f"soup{k}_{j}"] = (soup(port, 100 + i, k), soup(port, 200 + i, j))
    return out


def welds(port, recorded):
    names = list(pairs(port))
    assert len(recorded) == len(names)
    out = {n: np.asarray(w, np.uint64).reshape(4, 64) for n, w in zip(names, recorded)}
    z = np.zeros(64, np.uint64)
    for n in ("eater", "cat3", "eater_seam", "soup3_2"):
        out["plain_" + n] = np.stack([pairs(port)[n][0], z, z, z])
    lattice = np.zeros(64, np.uint64)
    lattice[::2] = np.uint64(0x5555555555555555)      # its ZOI is the whole torus
    out["plain_lattice"] = np.stack([lattice, z, z, z])
    for i, (k, j) in enumerate(SOUP_WELDS):
        out[f"soupweld{k}_{j}"] = np.stack([soup(port, 300 + i, k)] + [soup(port, 400 + 3 * i + p, j) for p in range(3)])
    return out


def actives(port):
    z = np.zeros(64, np.uint64)
    # a glider on its way into the eater's claw: eaten, the weld is itself again at generation 18
    g = moved(port.parse("3o$o$bo!"), AT[0] + 5, AT[1] + 7)
    return {"none": z, "glider": g, "glider_seam": moved(g, SEAM[0] - AT[0], SEAM[1] - AT[1]),
            "far_block": moved(port.parse("2o$2o!"), 50, 5),       # settles at once: a fixed point
            "soup3": soup(port, 500, 3), "soup4": soup(port, 501, 4), "soup5": soup(port, 502, 5),
            "soup2": soup(port, 503, 2)}


def masks(port):
    half = np.zeros(64, np.uint64)
    half[:32] = ~np.uint64(0)
    return {"all": ~np.zeros(64, np.uint64), "half": moved(half, AT[0] + 3 - 32, 0), "soup": soup(port, 600, 1)}


def _stable_cases():
    cases = [("eater", "glider", d, "all") for d in DURATIONS]
    cases += [("eater", "glider", 40, "half"), ("eater", "glider", 40, "soup"),
              ("eater_seam", "glider_seam", 8, "all"), ("eater_seam", "glider_seam", 40, "all"),
              ("eater", "far_block", 40, "all"), ("eater", "none", 40, "all"), ("empty", "soup4", 8, "all"),
              ("plain_eater", "glider", 40, "all")]
    sparse = ("soup4", "soup5", "soup3")
    for i, w in enumerate(("cat2", "cat3", "block", "cat2_seam", "cat3_seam", "block_seam")):
        for j, d in enumerate((2, 8, 40)):
            cases.append((w, sparse[(i + j) % 3], d, ("all", "half", "soup")[(i + 2 * j) % 3]))
    dense = ("soup2", "soup3", "soup4", "none")
    names = [f"soup{k}_{j}" for k, j in SOUP_PAIRS] + [f"soupweld{k}_{j}" for k, j in SOUP_WELDS]
    for i, w in enumerate(names):
        for j, d in enumerate((1, 2, 8, 40)):
            if (i + j) % 2 == 0:
                cases.append((w, dense[(i + j // 2) % 4], d, ("all", "soup", "half")[(i + j) % 3]))
    return cases


STABLE_CASES = _stable_cases()
OFFSET_OTHERS = ("eater", "soupweld3_2", "cat2_seam", "plain_eater", "soup2_4")
OFFSET_WELDS = ("eater", "cat2", "cat3", "block", "empty", "eater_seam", "cat3_seam", "block_seam", "plain_eater",
                "plain_cat3", "plain_eater_seam", "plain_soup3_2", "plain_lattice", "soup2_2", "soup3_3", "soup4_1", "soupweld2_3",
                "soupweld3_1", "soupweld4_3")
