"""CPU: a numpy definition of the batched LifeStable::CompleteStable
(LifeStable.hpp:1340-1458 with a node budget in place of the clock), pinned to
every run the reference recorded in tests/golden/stable_complete.npz: result,
best, nodes and deepest stack in the four flag combinations, and result, best
and nodes at the budgets {1, nodes - 1, nodes, nodes + 1}.

The model is the search written as an explicit stack over column words, with
the existing oracle's Propagate and Vulnerable inside a node (as the
PropagateAndTest model takes them); it shares nothing with the kernel but the
definitions.  `nodes` counts the entries of CompleteStableStep over the whole
call, tail calls included; "the clock is past the limit" is nodes >= budget,
tested at the entry of a step before the node counts itself and after each
search-area round.

It alone defines the three cases the reference leaves undefined:
  * unknown within state.ZOI() at the start (no round would run and `result`
    be read uninitialised): one CompleteStableStep on the object as given, the
    call going on from its result.  The recording holds such objects (class
    `within_zoi`), run by the recorder's spelled-out search, which takes the same
    definition; CompleteStable itself was not compared on them;
  * use_seed with an empty seed (the loop at :1369 would not end): result 4,
    best empty, nothing searched -- after the early returns for an empty state
    and an empty unknown, which do not look at the seed;
  * a search that needs more than max_depth frames: result 3, best empty.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stable_complete_cases as C  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COMPLETED, INCONSISTENT, TIMEOUT, TOO_DEEP, BAD_SEED = range(5)
ST, UN, D0 = 0, 1, 4
ONE = np.uint64(1)
INT_MAX = 2 ** 31 - 1
CLASSES = ("depth0", "backtracked", "bad_root", "bad_tree", "rounds2", "minimise_improves", "seed3",
           "column_seam", "row_seam", "within_zoi", "long", "deep")


def rot(w, k):
    k %= 64
    return w if k == 0 else (w << np.uint64(k)) | (w >> np.uint64(64 - k))


def zoi(w):
    """LifeState::ZOI, LifeAPI.hpp:521-536"""
    t = w | rot(w, 1) | rot(w, 63)
    return t | np.roll(t, 1) | np.roll(t, -1)


def big_zoi(w):
    """LifeState::BigZOI, LifeAPI.hpp:564-591"""
    return zoi(w | rot(w, 1) | rot(w, 63) | np.roll(w, 1) | np.roll(w, -1))


def pop(w):
    return int(np.unpackbits(np.ascontiguousarray(w, "<u8").view(np.uint8)).sum())


def first_on(w):
    """LifeState::FirstOn, LifeAPI.hpp:301-323: the LAST populated group of four columns, its
    first populated column, that column's lowest row; None for the empty state"""
    cols = np.flatnonzero(w)
    if len(cols) == 0:
        return None
    quad = int(cols[-1]) & ~3
    x = int(cols[cols >= quad][0])
    v = int(w[x])
    return x, (v & -v).bit_length() - 1


def count_is(w, k):
    """cells whose 3 x 3 neighbourhood (the cell included) holds exactly k cells of w"""
    a = C.unpack(w).astype(np.int64)
    a = a + np.roll(a, 1, 1) + np.roll(a, -1, 1)
    a = a + np.roll(a, 1, 0) + np.roll(a, -1, 0)
    return C.pack(a == k)


def set_cell(p, cell, on):
    """LifeStable::SetOn / SetOff of one cell, LifeStable.hpp:320-335"""
    x, y = cell
    bit = ONE << np.uint64(y)
    p[UN, x] &= ~bit
    if on:
        p[ST, x] |= bit
        p[4:10, x] |= bit
    else:
        p[ST, x] &= ~bit
        p[2:4, x] |= bit


class Search:
    def __init__(self, port, minimise, budget, max_depth):
        self.port, self.minimise, self.budget, self.max_depth = port, minimise, budget, max_depth
        self.nodes, self.deepest, self.max_pop, self.best = 0, 0, INT_MAX, np.zeros(64, np.uint64)

    def step(self, p, use_seed, seed):
        """CompleteStableStep (:1340-1412) of p (10, 64), changed in place, on an explicit stack"""
        stack = []
        while True:
            r = self.node(p, use_seed, seed, stack)
            if r is None:
                continue                # the off-branch was entered
            if r == TOO_DEEP or r == TIMEOUT or not stack or (not self.minimise and r == COMPLETED):
                return r
            frame, cell = stack.pop()   # then must be on: the tail call
            p[:] = frame
            set_cell(p, cell, True)

    def node(self, p, use_seed, seed, stack):
        if self.nodes >= self.budget:
            return TIMEOUT
        self.nodes += 1
        out, fl = self.port.stable_pass(p.reshape(1, 640), 4)
        p[:] = out.reshape(10, 64)
        if not fl[0] & 1:
            return INCONSISTENT
        current = pop(p[ST])
        if current >= self.max_pop:
            return COMPLETED
        settable = np.bitwise_or.reduce(p[2:10], axis=0) & p[UN] & zoi(p[D0])
        if not settable.any():
            self.best, self.max_pop = p[ST].copy(), current
            return COMPLETED
        if use_seed:
            z = seed
            while not (settable & z).any():
                z = zoi(z)
            settable = settable & z
        cell = first_on(self.port.stable_vulnerable(p.reshape(1, 640))[0] & settable)
        if cell is None:
            cell = first_on(settable & count_is(p[UN], 2))
        if cell is None:
            cell = first_on(settable & count_is(p[UN], 3))
        if cell is None:
            cell = first_on(settable)
        if cell is None:
            return INCONSISTENT
        if len(stack) == self.max_depth:
            return TOO_DEEP
        stack.append((p.copy(), cell))
        self.deepest = max(self.deepest, len(stack))
        set_cell(p, cell, False)        # try off
        return None


def complete(port, planes, seed=None, minimise=False, budget=1 << 16, max_depth=64):
    """CompleteStable of (10, 64) words: (result, best (64,), nodes, deepest stack)"""
    given = np.array(planes, np.uint64).reshape(10, 64)
    none = np.zeros(64, np.uint64)
    if not given[ST].any():
        return COMPLETED, none, 0, 0
    if not given[UN].any():
        return COMPLETED, given[ST].copy(), 0, 0
    use_seed = seed is not None
    seed = None if seed is None else np.asarray(seed, np.uint64)
    if use_seed and not seed.any():
        return BAD_SEED, none, 0, 0
    s = Search(port, minimise, budget, max_depth)
    area = zoi(given[ST])
    if not (given[UN] & ~area).any():
        r = s.step(given.copy(), use_seed, seed)            # no round would run: one step on the object as given
    else:
        while (given[UN] & ~area).any():
            area = zoi(area)
            copy = given.copy()
            copy[UN] &= area
            r = s.step(copy, use_seed, seed)
            if r == TOO_DEEP or s.best.any() or s.nodes >= s.budget:
                break
    if r == TOO_DEEP:
        return TOO_DEEP, none, s.nodes, s.deepest
    if r in (TIMEOUT, INCONSISTENT) and not s.best.any():
        return r, none, s.nodes, s.deepest
    if minimise:
        copy = given.copy()
        copy[UN] &= big_zoi(area)
        if s.step(copy, True, given[ST] | s.best) == TOO_DEEP:
            return TOO_DEEP, none, s.nodes, s.deepest
    return COMPLETED, s.best, s.nodes, s.deepest


# ---- pinned to the recording ------------------------------------------------------

class Recording:
    def __init__(self):
        z = np.load(os.path.join(GOLDEN, "stable_complete.npz"))
        self.kept = z["kept"]
        self.planes, self.seeds, self.infos = C.build(self.kept)
        self.head = z["head"].astype(np.int64)
        state = self.planes[:, 0]
        self.result, self.nodes, self.depth = self.head[:, :, 0], self.head[:, :, 1], self.head[:, :, 2]
        self.best = np.where((self.result == 0)[:, :, None], z["best"] ^ state[:, None], 0).astype(np.uint64)
        self.budgets, self.bhead = z["budgets"].astype(np.int64), z["bhead"].astype(np.int64)
        self.bbest = np.where((self.bhead[..., 0] == 0)[..., None], z["bbest"] ^ state[:, None, None], 0).astype(np.uint64)
        self.classes = {n: np.flatnonzero(z["classes"] >> c & 1) for c, n in enumerate(CLASSES)}
        self.weld = {k: z["weld_" + k] for k in ("a", "b", "mask", "tested", "counts")}

    def run(self, port, u, f, **kw):
        minimise, use_seed = C.FLAGS[f]
        return complete(port, self.planes[u], self.seeds[u] if use_seed else None, minimise, **kw)


_REC = []


def recording():
    if not _REC:
        _REC.append(Recording())
    return _REC[0]


@pytest.fixture(scope="module")
def rec():
    return recording()


def test_recording_is_not_vacuous(rec):
    for name in CLASSES:
        assert len(rec.classes[name]) >= (4 if name in ("long", "deep") else 8), name
    assert (rec.nodes <= 4096).all() and (rec.depth <= 32).all() and rec.nodes.max() >= 128 and rec.depth.max() >= 16
    for u in rec.classes["minimise_improves"]:
        assert pop(rec.best[u, 1]) < rec.head[u, 1, 4]
    assert (rec.head[rec.classes["seed3"], 2, 7] >= 3).all() and (rec.head[rec.classes["rounds2"], 0, 3] > 1).all()
    assert {r for r in rec.result.reshape(-1)} == {COMPLETED, INCONSISTENT}
    assert (rec.bhead[..., 0] == TIMEOUT).sum() >= 64


@pytest.mark.parametrize("f", range(4))
def test_model_matches_the_recording(rec, port, f):
    for u in range(len(rec.kept)):
        r, best, nodes, depth = rec.run(port, u, f)
        assert (r, nodes, depth) == (rec.result[u, f], rec.nodes[u, f], rec.depth[u, f]), (u, rec.kept[u])
        assert (best == rec.best[u, f]).all(), u


@pytest.mark.parametrize("f", range(4))
def test_model_matches_the_recorded_budgets(rec, port, f):
    """budgets 1, nodes - 1, nodes and nodes + 1: exactly `budget` nodes can run"""
    for u in range(len(rec.kept)):
        for b in range(4):
            r, best, nodes, _ = rec.run(port, u, f, budget=int(rec.budgets[u, f, b]))
            assert (r, nodes) == tuple(rec.bhead[u, f, b]), (u, b)
            assert (best == rec.bbest[u, f, b]).all(), (u, b)
    assert (rec.bhead[:, f, 2:, 1] == rec.nodes[:, f, None]).all()
    # never more nodes than the budget, and a search that times out has used all of it
    assert (rec.bhead[:, f, :, 1] <= rec.budgets[:, f]).all()
    late = rec.bhead[:, f, :, 0] == TIMEOUT
    assert late.any() and (rec.bhead[:, f, :, 1][late] == rec.budgets[:, f][late]).all()


def test_max_depth_is_exact(rec, port):
    """the recorded depth fits, one frame fewer gives 3 and the empty state"""
    for u in list(rec.classes["deep"]) + list(rec.classes["backtracked"][:4]):
        for f in range(4):
            d = int(rec.depth[u, f])
            r, best, nodes, depth = rec.run(port, u, f, max_depth=d)
            assert (r, nodes, depth) == (rec.result[u, f], rec.nodes[u, f], d) and (best == rec.best[u, f]).all()
            if d:
                r, best, _, _ = rec.run(port, u, f, max_depth=d - 1)
                assert r == TOO_DEEP and not best.any()


def test_early_returns_and_the_bad_seed(rec, port):
    p = rec.planes[0].copy()
    empty, seed = np.zeros(64, np.uint64), rec.seeds[0]
    no_state = p.copy()
    no_state[ST] = 0
    no_unknown = p.copy()
    no_unknown[UN] = 0
    for minimise in (False, True):
        for s in (None, seed, empty):       # the early returns come before the seed is looked at
            r, best, nodes, _ = complete(port, no_state, s, minimise)
            assert (r, nodes) == (COMPLETED, 0) and not best.any()
            r, best, nodes, _ = complete(port, no_unknown, s, minimise)
            assert (r, nodes) == (COMPLETED, 0) and (best == p[ST]).all()
        r, best, nodes, _ = complete(port, p, empty, minimise)
        assert (r, nodes) == (BAD_SEED, 0) and not best.any()


def test_within_zoi_runs_one_step(rec, port):
    """unknown within state.ZOI(): one step on the object as given; with every unknown cell
    settled by it the call is that step's result"""
    for u in rec.classes["within_zoi"]:
        p = rec.planes[u]
        assert not (p[UN] & ~zoi(p[ST])).any() and rec.head[u, 0, 5] == 0 and rec.head[u, 0, 3] == 0
        s = Search(port, False, 1 << 16, 64)
        r = s.step(p.copy(), False, None)
        got = complete(port, p)
        assert got[0] == r and got[2] == s.nodes and (got[1] == (s.best if r == COMPLETED else 0)).all()
