"""Builders of the sharp inputs of Match, Convolve and InteractionOffsets:
inputs on which one lost care cell, one lost pattern cell, one lost term or
one wrong threshold changes the answer.  Seeded, deterministic, CPU only;
tests/golden/make_match_golden.py records the reference's answers on them
(tests/golden/match_sharp.npz), tests/test_match_sharp.py pins the numpy
definitions of tests/test_match_model.py to that recording and measures how
sharp the inputs are, tests/test_gpu_match.py runs the kernels on them.

  near_miss_states   for one target: a universe that matches at one planted
                     offset, then one universe per care cell with exactly that
                     cell wrong
  impulse_states     single cells (and one pair) for Convolve: the answer is
                     the pattern itself, moved, so every cell of it shows
  interaction_batch  sparse soups with two dense 4 x 4 boxes each: the masks
                     of InteractionOffsets are neither empty nor full, and
                     every count from 0 to 9 occurs on live and dead cells
  Interaction        np_interaction_offsets taken apart into (plane, plane)
                     terms, so that a mutant of the formula is a list of pairs
"""
import os

import numpy as np

import test_match_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "match_sharp.npz")
U1 = np.uint64(1)


def rotl_each(v, b):
    """word i rotated left by b[i] rows"""
    b = np.asarray(b, np.uint64) & np.uint64(63)
    return (v << b) | (v >> ((np.uint64(64) - b) & np.uint64(63))) * (b != 0)


# ---- Match: near misses -------------------------------------------------------

def _seam_shift(rng, used):
    """a shift that puts two cyclically adjacent members of `used` (coordinates
    of care cells, one axis) on 63 and 0; with no adjacent pair, any shift"""
    pairs = [a for a in sorted(used) if (a + 1) % 64 in used]
    if not pairs:
        return int(rng.integers(0, 64))
    return (63 - pairs[int(rng.integers(0, len(pairs)))]) % 64


def near_miss_states(port, target, seed):
    """(states, (dx, dy)): states[0] holds `wanted` moved by (dx, dy), with the
    care cells on both sides of both seams where the target has adjacent
    columns and rows, and every `unwanted` cell dead there: it matches at
    (dx, dy).  states[1 + i] is states[0] with care cell i flipped (a wanted
    cell cleared, an unwanted cell set; wanted first, each in the order of
    cells()): at (dx, dy) exactly one care cell is wrong.  All other cells are
    dead, except for a target with nothing wanted, which a dead board would
    match everywhere: its non-care cells hold a seeded half-density soup."""
    wanted, unwanted = target
    rng = np.random.default_rng(seed)
    cw, cu = M.cells(wanted), M.cells(unwanted)
    dx = _seam_shift(rng, {a for a, _ in cw + cu})
    dy = _seam_shift(rng, {b for _, b in cw + cu})
    base = M.at(wanted, dx, dy)
    if not cw:
        base = base | (port.fill(1, seed=seed)[0] & ~M.at(unwanted, dx, dy))
    states = np.repeat(base[None], 1 + len(cw) + len(cu), axis=0)
    for i, (a, b) in enumerate(cw + cu):
        states[1 + i, (a + dx) % 64] ^= U1 << np.uint64((b + dy) % 64)
    return states, (dx, dy)


def near_miss_cases(port, targets):
    """name -> (states, (dx, dy)) for every target with a care cell"""
    return {name: near_miss_states(port, t, 3000 + k) for k, (name, t) in enumerate(targets.items())
            if (t[0] | t[1]).any()}


def without_cell(pattern, a, b):
    p = pattern.copy()
    p[a] &= ~(U1 << np.uint64(b))
    return p


# ---- Convolve: impulses ---------------------------------------------------------

IMPULSES = ([(0, 0)], [(63, 63)], [(31, 32)], [(32, 31)], [(5, 9), (38, 42)])


def impulse_states():
    """four single cells, and two cells 33 columns and 33 rows apart"""
    return np.stack([M._cells_to_pattern(cs) for cs in IMPULSES])


# ---- InteractionOffsets: sparse soups with clusters -------------------------------

N_BATCH = 4097


def interaction_batch(port, n):
    """n universes: a soup of 1/128 density (seven ANDed fills) with two seeded
    4 x 4 half-density boxes ORed in at seeded places; in every eighth universe
    the first box lies across both seams.  A batch of n <= N_BATCH is the
    first n of the longest (the boxes are always drawn for N_BATCH)."""
    assert n <= N_BATCH
    x = port.fill(n, seed=2101)
    for seed in range(2102, 2108):
        x &= port.fill(n, seed=seed)
    rng = np.random.default_rng(2108)
    bits = rng.integers(0, 1 << 16, size=(N_BATCH, 2), dtype=np.uint64)[:n]
    place = rng.integers(0, 64, size=(N_BATCH, 2, 2))
    place[::8, 0] = rng.integers(61, 64, size=(len(place[::8]), 2))
    place = place[:n]
    u = np.arange(n)
    for box in range(2):
        for i in range(4):
            nibble = (bits[:, box] >> np.uint64(4 * i)) & np.uint64(15)
            x[u, (place[:, box, 0] + i) % 64] |= rotl_each(nibble, place[:, box, 1])
    return x


def sharp_others(port):
    """eater_seams of build_others; an R-pentomino across both seams (its
    live cells have inclusive counts 3, 3, 3, 4 and 5); a seeded 4 x 4 box"""
    o = {}
    o["eater_seams"] = M.build_others(port)["eater_seams"]
    o["r_pentomino_seams"] = M.at(port.parse("b2o$2o$bo!"), 62, 62)
    bits = np.random.default_rng(2109).integers(0, 2, size=(4, 4))
    o["random_4x4"] = M._cells_to_pattern([(40 + i, 21 + j) for i in range(4) for j in range(4) if bits[i, j]])
    return o


N_RECORDED = 64    # universes of interaction_batch whose reference answers are recorded


# ---- InteractionOffsets as a list of (plane, plane) terms -------------------------

def _planes(s):
    """M._interaction_planes (planes 0-6), then the threshold mutants:
      "3:==4"   plane 3 with count == 4        "5:>=3"  plane 5 with count >= 3
      "4:>=5"   plane 4 with count >= 5        "6:>=2"  plane 6 with count >= 2
      "4:>=3"   plane 4 with count >= 3        "1:1..2" plane 1 with count 1 or 2
                                               "2:==3"  plane 2 with count == 3"""
    live = M.unpack(s)
    count = sum(np.roll(live, (dx, dy), axis=(-2, -1)).astype(np.int8) for dx in (-1, 0, 1) for dy in (-1, 0, 1))
    dead = ~live
    p = dict(enumerate(M._interaction_planes(s)))
    for name, plane in (("3:==4", (count == 4) & live), ("4:>=5", (count >= 5) & live), ("4:>=3", (count >= 3) & live),
                        ("5:>=3", (count >= 3) & dead), ("6:>=2", (count >= 2) & dead),
                        ("1:1..2", ((count == 1) | (count == 2)) & dead), ("2:==3", (count == 3) & dead)):
        p[name] = M.pack(plane)
    return p


THRESHOLDS = ("3:==4", "4:>=5", "4:>=3", "5:>=3", "6:>=2", "1:1..2", "2:==3")
BASE = tuple((i, M.PARTNER[i]) for i in range(7))   # np_interaction_offsets: the OR of a[i] * b[PARTNER[i]]


def mutants():
    """name -> the formula as a tuple of (plane of the universe, plane of the
    mirrored other): the 7 term deletions, the 21 transpositions of two
    entries of PARTNER, the 7 threshold mutants on either side"""
    m = {}
    for t in range(7):
        m[f"delete term {t}"] = tuple(pq for pq in BASE if pq[0] != t)
    for i in range(7):
        for j in range(i + 1, 7):
            p = list(M.PARTNER)
            p[i], p[j] = p[j], p[i]
            m[f"swap partners {i} {j}"] = tuple((k, p[k]) for k in range(7))
    for name in THRESHOLDS:
        k = int(name[0])
        m[f"universe plane {name}"] = tuple((name if a == k else a, b) for a, b in BASE)
        m[f"other plane {name}"] = tuple((a, name if b == k else b) for a, b in BASE)
    return m


class Interaction:
    """InteractionOffsets of a batch with one `other`, for any formula: the
    planes of both sides once, each convolution once"""

    def __init__(self, states, other):
        self.a, self.b = _planes(states), _planes(M.np_mirrored(other))
        self.terms = {}

    def __call__(self, formula=BASE):
        out = np.zeros_like(self.a[0])
        for pq in formula:
            if pq not in self.terms:
                self.terms[pq] = M.np_convolve(self.a[pq[0]], self.b[pq[1]])
            out |= self.terms[pq]
        return out


# ---- the recording ------------------------------------------------------------------

_cache = {}


def fixture_data(port):
    """the recorded arrays of match_sharp.npz and the regenerated inputs:
      near_miss   name -> (states, (dx, dy), the target, the recorded masks)
      impulses, patterns, convolve[pattern][impulse]
      batch (the first N_RECORDED of interaction_batch), others, interaction[other][universe]"""
    if not _cache:
        z = np.load(FIXTURE)
        d = {k: z[k] for k in z.files}
        base = M.fixture_data(port)
        targets = M.build_targets(port, base["states"])
        d["near_miss"], at = {}, 0
        for name, (states, offset) in near_miss_cases(port, targets).items():
            d["near_miss"][name] = (states, offset, targets[name], d["near_miss_match"][at:at + len(states)])
            at += len(states)
        assert at == len(d["near_miss_match"]) and list(d["near_miss"]) == list(d["near_miss_names"])
        d["patterns"] = M.build_patterns(port)
        d["batch"] = interaction_batch(port, N_RECORDED)
        for a in [d["batch"], *(v[0] for v in d["near_miss"].values())] + [v for v in d.values() if isinstance(v, np.ndarray)]:
            a.flags.writeable = False
        _cache.update(d)
    return _cache
