"""Inputs of the bounded Propagate / StabiliseOptions tests
(tests/test_stable_bounded.py): seeded, deterministic, CPU only, data alone --
plus the oracle's iteration trace of a batch and, read off that trace, which
iterations the product's Propagate runs on its 32-row window.

  strips(n, seed)   (n, 640) LifeStables whose unknown cells lie in a cyclic strip
                    of 2-24 rows (first row uniform in 0..63), each cell of the
                    strip unknown with probability 0.45; every other cell known
                    OFF, the option planes zero; then 1-3 of the unknown cells
                    decided ON.  Forcing chains run along the strip step after
                    step, the rows they change few enough for the window.
  soups(port, n, seed)   the same without the strip: every cell unknown with
                    probability 0.3, one of them decided ON (soup_candidates);
                    of those, the objects every step of which changes rows all
                    over the torus: no window iteration, the deepest full ones.
  far_reaching(port)     strips over a still life (lattice_strips), of which the
                    objects with a window iteration whose changes lie 2 rows
                    beyond the previous iteration's (window_reach), and the
                    inputs of tests/golden/stable_window.npz.
  cascades(port, n, seed)   the cascade family of tests/test_ref_gpu.py (still
                    lifes on an 8-cell lattice under a large unknown region).

  Trace(port, x, which)   every object iterated to its end by the oracle's
                    single passes (Port.stable_iteration), the planes kept
                    after every iteration.
  window_route(trace)     the routing rule of stable_kernels.hpp
                    stable_iter_window, restated: iteration k >= 2 of an object
                    runs on the window when the rows in which any plane changed
                    during iteration k - 1 have a smallest cyclic window
                    (device.hpp care_window, as tests/test_cone_model.py restates
                    it) of 1 .. 32 - 4 RHO rows, RHO = 3 for Propagate; the
                    window's first row is (first changed row - 2 RHO) mod 64.

The kernel's own record of an iteration's changes (`chg` / `moved`) is that
plane difference: UpdateOptions marks r & ~plane for every option plane it ORs
r into; SignalNeighbours marks the unknown cells it settles, each of which
clears its unknown bit; SynchroniseStateKnown marks the known cells whose
options it sets (maybe_dead & known_on, maybe_live & known_off -- the
reference's third term, ~unknown & maybe_live & maybe_dead, lies inside
those), the cells whose state it sets and, beyond the reference's own
`changes`, the cells whose unknown bit it clears.  So the rule is stated on
the oracle's planes alone.  Only Propagate takes the window in the product
(kPropagateWindow; StabiliseOptions' kernels are built with the window off).
"""
import os

import numpy as np

from test_cone_model import care_window

RHO = 3                      # PropagateStep reads a cell's planes within 3 cells
WINDOW_FIT = 32 - 4 * RHO    # the most changed rows a window iteration takes: 20
STRIPS_SEED, SOUPS_SEED, CASCADES_SEED, REACH_SEED = 4242, 4248, 8080, 4250
U1 = np.uint64(1)


def _pack(bits):
    """(n, 64 columns, 64 rows) of 0/1 -> (n, 64) column words, bit i = row i"""
    w = np.packbits(bits.astype(np.uint8), axis=-1, bitorder="little")
    return np.ascontiguousarray(w).view(np.uint64).reshape(bits.shape[0], 64)


def _decide_on(rng, x, u, count):
    """`count` of object u's unknown cells decided ON (state set, unknown cleared)"""
    cells = [(c, r) for c in np.nonzero(x[u, 1])[0] for r in range(64) if (int(x[u, 1, c]) >> r) & 1]
    for i in rng.choice(len(cells), size=min(count, len(cells)), replace=False):
        c, r = cells[int(i)]
        x[u, 1, c] &= ~(U1 << np.uint64(r))
        x[u, 0, c] |= U1 << np.uint64(r)


def strips(n=600, seed=STRIPS_SEED):
    rng = np.random.default_rng(seed)
    x = np.zeros((n, 10, 64), np.uint64)
    x[:, 1] = _pack(rng.random((n, 64, 64)) < 0.45)
    for u in range(n):
        y0, h = int(rng.integers(64)), int(rng.integers(2, 25))
        x[u, 1] &= np.uint64(sum(1 << ((y0 + i) % 64) for i in range(h)))
        _decide_on(rng, x, u, int(rng.integers(1, 4)))
    return x.reshape(n, 640)


def soup_candidates(n, seed=SOUPS_SEED):
    rng = np.random.default_rng(seed)
    x = np.zeros((n, 10, 64), np.uint64)
    x[:, 1] = _pack(rng.random((n, 64, 64)) < 0.3)
    for u in range(n):
        _decide_on(rng, x, u, 1)
    return x.reshape(n, 640)


def soups(port, n=200, seed=SOUPS_SEED):
    """Of 4 n soup_candidates, those none of whose Propagate iterations is a
    window iteration (window_route), the n that run longest (ties in the
    candidates' order).  The selection is needed: about half of the raw
    candidates end on a window iteration, their last changes being a few
    cells in 3 rows."""
    x = soup_candidates(4 * n, seed)
    trace = Trace(port, x, 4)
    windowed = {u for (u, _), (y0, _) in window_route(trace).items() if y0 is not None}
    keep = np.array([u for u in range(len(x)) if u not in windowed])
    keep = keep[np.argsort(-trace.iters[keep], kind="stable")][:n]
    assert keep.size == n, keep.size
    return np.ascontiguousarray(x[np.sort(keep)])


def cascades(port, n=400, seed=CASCADES_SEED):
    """tests/test_ref_gpu.py test_propagate_cascades_vs_reference's inputs"""
    rng = np.random.default_rng(seed)
    pats = [port.parse(t) for t in ("2o$2o!", "b2o$o2bo$b2o!", "b2o$o2bo$bobo$2bo!", "2o$obo$bo!", "bo$obo$bo!")]
    x = np.zeros((n, 10, 64), np.uint64)
    for u in range(n):
        st = np.zeros(64, np.uint64)
        for gx in range(8):
            for gy in range(8):
                if rng.random() < 0.55:
                    pt = pats[int(rng.integers(len(pats)))]
                    st |= np.roll(pt, 8 * gx + 1) << np.uint64(8 * gy + 1)
        unk = np.zeros(64, np.uint64)
        y0, h = int(rng.integers(64)), int(rng.integers(10, 41))
        rows = np.uint64(sum(1 << ((y0 + i) % 64) for i in range(h)))
        x0, w = int(rng.integers(64)), int(rng.integers(10, 41))
        for c in range(w):
            unk[(x0 + c) % 64] = rows
        state = st & ~unk
        for _ in range(int(rng.integers(1, 4))):
            c, b = (x0 + int(rng.integers(w))) % 64, (y0 + int(rng.integers(h))) % 64
            unk[c] &= ~np.uint64(1 << b)
            if rng.random() < 0.5:
                state[c] |= np.uint64(1 << b)
        x[u, 0], x[u, 1] = state, unk
    return x.reshape(n, 640)


class Trace:
    """The oracle's iterations of Propagate (which 4) or StabiliseOptions (5)
    on every object of x, each run to its own end:
      after[k]   (n, 640): the planes after k iterations (after[0] = x); an
                 object that has ended keeps its last planes
      flag[k]    (n,) uint8, k >= 1: what iteration k returned (0 inconsistent,
                 1 nothing changed, 3 changed); 255 where the object ended before
      iters      (n,): the iterations the object runs (the last one inconsistent
                 or changing nothing)"""

    def __init__(self, port, x, which):
        x = np.ascontiguousarray(x, np.uint64).reshape(-1, 640)
        self.which, self.n = which, x.shape[0]
        self.after, self.flag = [x.copy()], [np.full(self.n, 255, np.uint8)]
        self.iters = np.zeros(self.n, np.int64)
        live = np.arange(self.n)
        while live.size:
            cur, fl = self.after[-1].copy(), np.full(self.n, 255, np.uint8)
            cur[live], fl[live] = port.stable_iteration(cur[live], which)
            self.after.append(cur)
            self.flag.append(fl)
            self.iters[live] += 1
            live = live[fl[live] == 3]
        self.depth = int(self.iters.max()) if self.n else 0
        self.consistent = np.array([self.flag[self.iters[u]][u] == 1 for u in range(self.n)], bool)

    def bounded(self, k):
        """(planes, flags) of Port.stable_pass_bounded(x, which, k), k >= 1, read off the trace"""
        k = min(k, self.depth)
        fl = np.empty(self.n, np.uint8)
        for u in range(self.n):
            j = int(self.iters[u])
            fl[u] = 7 if j > k else (0 if self.flag[j][u] == 0 else 1 | (2 if j > 1 else 0))
        return self.after[k], fl

    def changed_rows(self, k):
        """(n,) uint64: the rows in which any plane of the object changed during iteration k"""
        d = self.after[k] ^ self.after[k - 1]
        return np.bitwise_or.reduce(d, axis=1)


def window_route(trace):
    """{(u, k): (first_row, changed_height)} for every iteration k >= 2 that object
    u runs; first_row is the window's first row when the product's Propagate
    takes iteration k on the window, None when it takes the whole columns"""
    out = {}
    for k in range(2, trace.depth + 1):
        rows = trace.changed_rows(k - 1)
        for u in np.nonzero(trace.iters >= k)[0]:
            y0, h = care_window(int(rows[u]))
            out[(int(u), k)] = ((y0 - 2 * RHO) % 64 if 1 <= h <= WINDOW_FIT else None, h)
    return out


def window_reach(trace):
    """{(u, k): rows} for every window iteration (window_route): how many rows
    beyond the rows iteration k - 1 changed (their cyclic window) the changes
    of iteration k reach.  The window iteration looks at RHO rows beyond; a
    reach of r is wrong in a window that looks at fewer than r."""
    out = {}
    for (u, k), (first, h) in window_route(trace).items():
        if first is None:
            continue
        y0, cur, reach = (first + 2 * RHO) % 64, int(trace.changed_rows(k)[u]), 0
        for r in range(64):
            if (cur >> r) & 1:
                off = (r - y0) % 64
                reach = max(reach, 0 if off < h else min(off - h + 1, 64 - off))
        out[(u, k)] = reach
    return out


def lattice_strips(port, indices, seed=REACH_SEED):
    """strips over a still life, object u drawn from (seed, u) alone: the cascade
    family's lattice of blocks, beehives, loaves, boats and tubs, the cells of
    a cyclic strip of 3-24 rows unknown with probability 0.45, 1-3 of them
    decided: to their true value, or (one in five) to the other"""
    pats = [port.parse(t) for t in ("2o$2o!", "b2o$o2bo$b2o!", "b2o$o2bo$bobo$2bo!", "2o$obo$bo!", "bo$obo$bo!")]
    x = np.zeros((len(indices), 10, 64), np.uint64)
    for i, u in enumerate(indices):
        rng = np.random.default_rng((seed, int(u)))
        st = np.zeros(64, np.uint64)
        for gx in range(8):
            for gy in range(8):
                if rng.random() < 0.7:
                    st |= np.roll(pats[int(rng.integers(len(pats)))], 8 * gx + 1) << np.uint64(8 * gy + 1)
        y0, h = int(rng.integers(64)), int(rng.integers(3, 25))
        unk = _pack(rng.random((1, 64, 64)) < 0.45)[0] & np.uint64(sum(1 << ((y0 + j) % 64) for j in range(h)))
        x[i, 0], x[i, 1] = st & ~unk, unk
        cells = [(c, r) for c in np.nonzero(unk)[0] for r in range(64) if (int(unk[c]) >> r) & 1]
        for j in rng.choice(len(cells), size=min(int(rng.integers(1, 4)), len(cells)), replace=False):
            c, r = cells[int(j)]
            bit = U1 << np.uint64(r)
            x[i, 1, c] &= ~bit
            if bool(st[c] & bit) != (rng.random() < 0.2):
                x[i, 0, c] |= bit
    return x.reshape(len(indices), 640)


def search_far_reaching(port, candidates=4000, seed=REACH_SEED):
    """the indices FAR_REACHING lists: of lattice_strips 0 .. candidates - 1, the
    objects one of whose window iterations reaches 2 rows beyond the previous
    iteration's changes (a few in a thousand: a cell settles, and in the next
    iteration a known cell next to it forces a cell on its other side)"""
    trace = Trace(port, lattice_strips(port, range(candidates), seed), 4)
    return tuple(sorted({u for (u, _), r in window_reach(trace).items() if r >= 2}))


FAR_REACHING = (178, 306, 377, 418, 712, 829, 871, 967, 1037, 1099, 1179, 1451, 1516, 1701, 1733, 1840, 1903, 2060, 2233,
                2617, 2868, 3040, 3111)   # search_far_reaching(port)


def far_reaching(port):
    """lattice_strips FAR_REACHING and the 15 inputs of
    tests/golden/stable_window.npz, found on the GPU for the same property"""
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stable_window.npz"))["input"]
    return np.ascontiguousarray(np.concatenate([lattice_strips(port, FAR_REACHING), golden.reshape(-1, 640)]))
