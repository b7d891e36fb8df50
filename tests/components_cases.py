"""Builders of the inputs of FirstOn, ComponentContaining and Components:
seeded, deterministic, CPU only, numpy alone (no model of the operations).
tests/golden/make_components_golden.py records the reference's answers on them
(tests/golden/components.npz), tests/test_components_model.py pins the numpy
restatement to that recording, the facade and GPU tests run on the same inputs.

  states(port)        name -> universe, in a fixed order:
                        pair_<p>_<a>_<b>  two cells {p, p + (a, b)}, |a|, |b| <= 3,
                                          p interior (20, 30) and p = (63, 63)
                                          (the pair crosses both seams)
                        lattice512, six_cells, quad0, empty       (the order)
                        spiral, spiral_cut, full_row, full_col, row_and_col,
                        comb, staircase                           (long floods)
                        soup<k>_<i>       density 2^-k, k = 2, 3, 4, i < 12
  CORONAS             name -> corona
  seeds_for(state)    the ComponentContaining seeds of one state
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "components.npz")
U1 = np.uint64(1)


def from_cells(cells):
    s = np.zeros(64, np.uint64)
    for x, y in cells:
        s[x % 64] |= U1 << np.uint64(y % 64)
    return s


def to_cells(s):
    return [(x, y) for x in range(64) for y in range(64) if (int(s[x]) >> y) & 1]


# ---- coronas ------------------------------------------------------------------

DEFAULT_CELLS = [(a, b) for a in range(-2, 3) for b in range(-2, 3) if abs(a) + abs(b) < 4]   # b3o$5o$5o$5o$b3o!
NEAR_NON_CELLS = [(a, b) for a in range(-3, 4) for b in range(-3, 4) if (a, b) not in DEFAULT_CELLS]
assert len(DEFAULT_CELLS) == 21 and len(NEAR_NON_CELLS) == 28

CORONAS = {
    "default": from_cells(DEFAULT_CELLS),
    "3x3": from_cells([(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)]),
    "plus": from_cells([(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)]),
    "right": from_cells([(0, 0), (1, 0)]),     # asymmetric: pins Convolve's direction in x
    "down": from_cells([(0, 0), (0, 1)]),      # and in y
    "7x7": from_cells([(a, b) for a in range(-3, 4) for b in range(-3, 4)]),   # the general path
    "no_centre": from_cells([c for c in DEFAULT_CELLS if c != (0, 0)]),        # ComponentContaining only
    "none": from_cells([]),                                                   # ComponentContaining only
}
COMPONENTS_CORONAS = ("default", "3x3", "plus", "right", "down", "7x7")       # those holding (0, 0)


# ---- states -------------------------------------------------------------------

PAIR_BASES = ((20, 30), (63, 63))
PAIR_OFFSETS = [(a, b) for a in range(-3, 4) for b in range(-3, 4)]


def spiral_path():
    """the pitch-3 square spiral in [0, 60]^2, as the list of its cells in path order"""
    x = y = 0
    path = [(0, 0)]
    lengths = [60, 60, 60] + [v for k in range(57, 0, -3) for v in (k, k)]
    for i, n in enumerate(lengths):
        dx, dy = ((1, 0), (0, 1), (-1, 0), (0, -1))[i % 4]
        for _ in range(n):
            x, y = x + dx, y + dy
            path.append((x, y))
    assert len(path) == len(set(path)) == 1321
    return path


def soups(port, k, n=12):
    """n universes of density 2^-k: ANDs of k seeded half-density fills"""
    s = port.fill(n, seed=7100 + 10 * k)
    for j in range(1, k):
        s = s & port.fill(n, seed=7100 + 10 * k + j)
    return s


def states(port):
    out = {}
    for p in PAIR_BASES:
        for a, b in PAIR_OFFSETS:
            out[f"pair_{p[0]}_{a}_{b}"] = from_cells([p, (p[0] + a, p[1] + b)])
    out["lattice512"] = from_cells([(x, y) for x in range(0, 64, 2) for y in range(0, 64, 2) if (x // 2 + y // 2) % 2 == 0])
    out["six_cells"] = from_cells([(1, 9), (61, 5), (62, 0), (60, 7), (60, 3), (33, 33)])
    out["quad0"] = from_cells([(2, 7), (3, 1), (1, 40), (2, 9), (1, 50)])
    out["empty"] = from_cells([])
    path = spiral_path()
    out["spiral"] = from_cells(path)
    mid = len(path) // 2
    out["spiral_cut"] = from_cells(path[:mid - 1] + path[mid + 2:])
    out["full_row"] = from_cells([(x, 17) for x in range(64)])
    out["full_col"] = from_cells([(40, y) for y in range(64)])
    out["row_and_col"] = from_cells([(x, 17) for x in range(64)] + [(40, y) for y in range(64)] + [(10, 50)])
    out["comb"] = from_cells([(x, 5) for x in range(2, 59)] + [(x, y) for x in range(2, 59, 4) for y in range(5, 51)])
    out["staircase"] = from_cells([(2 + 2 * k, 2 + k) for k in range(20)] + [(44 + k, 2 + 2 * k) for k in range(15)])
    for k in (2, 3, 4):
        for i, s in enumerate(soups(port, k)):
            out[f"soup{k}_{i}"] = s
    for s in out.values():
        s.flags.writeable = False
    return out


# the states whose Components are recorded with every corona (all of them with the default one)
def other_corona_names(all_states):
    keep = [n for n in all_states if n.startswith("pair_")]
    keep += ["six_cells", "quad0", "empty", "spiral", "spiral_cut", "row_and_col", "comb", "staircase"]
    keep += [f"soup{k}_{i}" for k in (2, 3, 4) for i in (0, 1)]
    return keep


# ---- ComponentContaining ---------------------------------------------------------

CC_STATES = ("six_cells", "quad0", "pair_63_3_3", "staircase", "soup4_0", "soup4_1")
SEED_KINDS = ("inside", "adjacent", "far", "two", "empty", "state")


def _near(s, x, y, r):
    """some cell of s within Chebyshev distance r of (x, y) on the torus"""
    return any((int(s[(x + a) % 64]) >> ((y + b) % 64)) & 1 for a in range(-r, r + 1) for b in range(-r, r + 1))


def seeds_for(s):
    """kind -> seed: a cell of the state; a dead cell one step (a corona cell
    with |a|, |b| <= 1) from a live one; a cell with nothing within 3 of it; the
    first and the last live cell in column order together; nothing; the state"""
    on = to_cells(s)
    dead = [(x, y) for x in range(64) for y in range(64) if not (int(s[x]) >> y) & 1]
    out = {"inside": from_cells([on[len(on) // 3]]),
           "adjacent": from_cells([next(c for c in dead if _near(s, *c, 1))]),
           "far": from_cells([next(c for c in dead if not _near(s, *c, 3))]),
           "two": from_cells([on[0], on[-1]]),
           "empty": from_cells([]),
           "state": s.copy()}
    return out


def two_cells(s):
    on = to_cells(s)
    return from_cells([on[0]]), from_cells([on[-1]])
