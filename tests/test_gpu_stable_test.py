"""GPU: the LifeStable lookahead kernels (strip passes, TestUnknowns,
PropagateAndTest) against every recording of tests/golden/stable_test.npz, bit
for bit, planes and flags, and against the CPU model (tests/
test_stable_test_model.py, itself pinned to the same recording).  The ragged
batches compare against the recording of the pool's objects, which the model
equals object by object (test_propagate_and_test_matches_the_recording), so the
model's eight seconds are spent once, on the CPU.  The bounded forms
(`max_iters`) have no recording; the model's bounded answers are computed once
per process (M.bounded_*, some twenty seconds) and shared by their tests."""
import numpy as np
import pytest
import torch

import stable_test_cases as C
import test_stable_test_model as M
from test_gpu_match import to_dev, to_host

pytestmark = pytest.mark.gpu

RAGGED = [1, 2, 3, 5, 63, 64, 65, 4097]
SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)


@pytest.fixture(scope="module")
def rec():
    return M.recording()


class Guarded:
    """n LifeStables to work on in place, one sentinel object before and after"""

    def __init__(self, planes):
        p = np.ascontiguousarray(planes, np.uint64).reshape(-1, 640)
        a = np.full((len(p) + 2, 640), SENTINEL, np.uint64)
        a[1:-1] = p
        self.all = to_dev(a.reshape(-1, 64)).view(len(p) + 2, 640)
        self.out = self.all[1:len(p) + 1]

    def result(self):
        h = to_host(self.all).reshape(-1, 640)
        assert (h[0] == SENTINEL).all() and (h[-1] == SENTINEL).all(), "a sentinel object was written"
        return h[1:-1].reshape(-1, 10, 64)


def dev(a, k=1):
    return to_dev(np.ascontiguousarray(a, np.uint64).reshape(-1, 64)).view(-1, k * 64)


def host_flags(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def zoi_words(w):
    """LifeState::ZOI of (..., 64) words"""
    w = np.asarray(w, np.uint64)
    one, top = np.uint64(1), np.uint64(63)
    t = w | (w << one) | (w >> top) | (w >> one) | (w << top)
    return t | np.roll(t, 1, -1) | np.roll(t, -1, -1)


# ---- every recording ------------------------------------------------------------

def test_golden_propagate_and_test(hip, rec):
    g = Guarded(rec.planes)
    fl = host_flags(hip.stable_propagate_and_test(g.out))
    assert (fl == rec.pat_flags).all(), np.flatnonzero(fl != rec.pat_flags)
    got = g.result()
    assert (got == rec.pat).all(), np.flatnonzero((got != rec.pat).any(axis=(1, 2)))


def test_golden_test_unknowns(hip, rec):
    """TestUnknowns(Vulnerable().ZOI()) after one Propagate, both taken by the existing kernels"""
    g = Guarded(rec.planes)
    hip.stable_pass(g.out, "propagate")
    cells = dev(zoi_words(to_host(hip.stable_vulnerable(g.out))))
    fl = host_flags(hip.stable_test_unknowns(g.out, cells))
    assert (fl == rec.tu_flags).all(), np.flatnonzero(fl != rec.tu_flags)
    got = g.result()
    assert (got == rec.tu).all(), np.flatnonzero((got != rec.tu).any(axis=(1, 2)))


@pytest.mark.parametrize("which", range(6))
def test_golden_strip_passes(hip, rec, which):
    k = len(rec.kept)
    start = np.repeat(rec.start.reshape(k * 2, 1, 10, 64), 8, axis=1)              # (k * 2, 8, 10, 64)
    cols = np.array([[rec.strip_column(u, c) for c in range(8)] for u in range(k) for _ in (0, 1)], np.uint8)
    want = np.stack([rec.strip(u, v, c, which) for u in range(k) for v in (0, 1) for c in range(8)])
    g = Guarded(start)
    fl = host_flags(hip.stable_strip_pass(g.out, torch.from_numpy(cols.reshape(-1)).cuda(), C.STRIP_PASSES[which]))
    assert (fl == rec.strip_flags[:, :, :, which].reshape(-1)).all()
    assert (g.result() == want).all()


# ---- ragged batches ---------------------------------------------------------------

def ragged_pick(rec, n):
    """n objects of the pool, every inconsistent one between consistent ones"""
    bad, good = np.flatnonzero(rec.pat_flags == 0), np.flatnonzero(rec.pat_flags != 0)
    pick = good[np.arange(n) % len(good)]
    pick[1::3] = bad[np.arange(len(pick[1::3])) % len(bad)]
    return pick


@pytest.mark.parametrize("n", RAGGED)
def test_ragged_propagate_and_test(hip, rec, n):
    pick = ragged_pick(rec, n)
    g = Guarded(rec.planes[pick])
    fl = host_flags(hip.stable_propagate_and_test(g.out))
    assert (fl == rec.pat_flags[pick]).all()
    assert (g.result() == rec.pat[pick]).all()
    if n >= 5:
        assert (fl == 0).any() and (fl[0::3] != 0).all() and (fl[2::3] != 0).all()


@pytest.mark.parametrize("n", RAGGED)
def test_ragged_propagate_strip_and_test_unknowns(hip, rec, n):
    pick = np.arange(n) % len(rec.kept)
    g = Guarded(rec.start[pick, 1])
    fl = host_flags(hip.stable_strip_pass(g.out, torch.from_numpy(rec.columns[pick]).cuda(), "propagate_strip"))
    want = np.stack([rec.strip(u, 1, 7, 4) for u in range(min(n, len(rec.kept)))])[pick]
    assert (fl == rec.strip_flags[pick, 1, 7, 4]).all()
    assert (g.result() == want).all()
    g = Guarded(rec.planes[pick])
    hip.stable_pass(g.out, "propagate")
    fl = host_flags(hip.stable_test_unknowns(g.out, dev(zoi_words(to_host(hip.stable_vulnerable(g.out))))))
    assert (fl == rec.tu_flags[pick]).all()
    assert (g.result() == rec.tu[pick]).all()


# ---- strip columns ----------------------------------------------------------------

def test_strip_all_columns(hip):
    """every column, a different one per object, on one eater that wraps both edges"""
    obj = next(p for p, _, info in map(C.one, range(C.NAMES.index("eater"), C.DRAWN, len(C.NAMES)))
               if info["straddles"] and info["dy"] >= 61 and info["wrong"] is None and info["region"] < 3)
    cols = np.arange(64, dtype=np.uint8)
    for which in range(6):
        g = Guarded(np.repeat(obj[None], 64, axis=0))
        fl = host_flags(hip.stable_strip_pass(g.out, torch.from_numpy(cols).cuda(), which))
        want = [M.strip_pass(obj, x, which) for x in range(64)]
        assert (fl == np.array([w[1] for w in want])).all(), which
        assert (g.result() == np.stack([w[0] for w in want])).all(), which
        # (the object as given is synchronised, and signals only next to its pattern)
        assert len({w[0].tobytes() for w in want}) == (64, 1, 2)[(which == 0) + 2 * (which == 2)], which


# ---- the forms of `cells` -----------------------------------------------------------

def test_cells_forms(hip, rec, port):
    # (not the whole-torus objects: their thousands of unknown cells cost the model seconds)
    pick = np.array([u for u, info in enumerate(rec.infos) if info["region"] < 3][::24])
    after, _ = port.stable_pass(rec.planes[pick].reshape(-1, 640), 4)
    after = after.reshape(-1, 10, 64)
    n = len(pick)
    one = np.bitwise_or.reduce(np.stack([zoi_words(zoi_words(p[0])) for p in rec.planes[pick[:4]]]))
    per = np.stack([zoi_words(p[1]) for p in after])
    per[1::2] = np.roll(per[1::2], 1, axis=1)
    for cells, masks in ((one[None], np.repeat(one[None], n, 0)), (per, per)):
        g = Guarded(after)
        fl = host_flags(hip.stable_test_unknowns(g.out, dev(cells)))
        want = [M.lookahead(p, m) for p, m in zip(after, masks)]
        assert (fl == np.array([w[1] for w in want])).all()
        assert (g.result() == np.stack([w[0] for w in want])).all()
        assert (fl == 3).any()
    # an empty mask, and a mask of known cells only: nothing to test, nothing changes
    for cells in (np.zeros((1, 64), np.uint64), ~after[:, 1]):
        g = Guarded(after)
        fl = host_flags(hip.stable_test_unknowns(g.out, dev(cells)))
        assert (fl == 1).all() and (g.result() == after).all()


# ---- the chain from the welds --------------------------------------------------------

def test_chain_from_welds(hip, port):
    """weld_to_stable, then stable_propagate_and_test = Propagate, Vulnerable, ZOI,
    TestUnknowns iterated by hand on the device until neither changes = the model"""
    import test_weld_model as W
    welds = np.stack(list(W.Recording(port).welds.values()))
    stables = hip.weld_to_stable(dev(welds, 4))
    start = to_host(stables).reshape(-1, 10, 64)
    g = Guarded(start)
    fl = host_flags(hip.stable_propagate_and_test(g.out))
    got = g.result()
    for u, s in enumerate(start):
        d = dev(s, 10)
        ever = 0
        while True:
            r = int(host_flags(hip.stable_pass(d, "propagate"))[0])
            t = 0
            if r & 1:
                cells = dev(zoi_words(to_host(hip.stable_vulnerable(d))[0]))
                t = int(host_flags(hip.stable_test_unknowns(d, cells))[0])
            if not (r & t & 1):
                hand = 0
                break
            if not (r | t) & 2:
                hand = 1 | ever
                break
            ever = 2
        assert fl[u] == hand, u
        assert (to_host(d).reshape(10, 64) == got[u]).all(), u
        want, wfl = M.propagate_and_test(port, s)
        assert fl[u] == wfl and (got[u] == want).all(), u
    assert (fl == 3).any()


# ---- the bound ------------------------------------------------------------------------

def test_bound(hip, rec, port):
    """max_iters = 1: an object whose first PropagateStep changes something (it needs a second
    one) returns 4 and its 5 KiB stay; its neighbours are unaffected; unbounded, the same
    batch matches the recording"""
    _, one_step = port.stable_pass_bounded(rec.planes.reshape(-1, 640), 4, 1)
    slow, quick = np.flatnonzero(one_step == 7), np.flatnonzero(one_step != 7)
    assert len(slow) >= 8 and len(quick) >= 8
    pick = np.empty(24, np.int64)
    pick[0::3], pick[1::3], pick[2::3] = quick[:8], slow[:8], quick[8:16] if len(quick) >= 16 else quick[:8]
    g = Guarded(rec.planes[pick])
    fl = host_flags(hip.stable_propagate_and_test(g.out, max_iters=1))
    got = g.result()
    assert (fl[1::3] == 4).all() and (got[1::3] == rec.planes[pick[1::3]]).all()
    for j, u in enumerate(pick):
        want, wfl = M.propagate_and_test(port, rec.planes[u], max_iters=1)
        assert fl[j] == wfl and (got[j] == want).all(), (j, u)
    g = Guarded(rec.planes[pick])
    fl = host_flags(hip.stable_propagate_and_test(g.out, max_iters=0))
    assert (fl == rec.pat_flags[pick]).all() and (g.result() == rec.pat[pick]).all()


# ---- the bound, bit for bit -------------------------------------------------------------
# against the model's bounded forms (test_stable_test_model.py bounded_*: computed once per
# process, pinned and proved non-vacuous there without a GPU)

def strip_run(hip, planes, columns, which, max_iters=0):
    g = Guarded(planes)
    cols = torch.from_numpy(np.ascontiguousarray(columns, np.uint8).reshape(-1)).cuda()
    fl = host_flags(hip.stable_strip_pass(g.out, cols, which, max_iters=max_iters))
    return g.result(), fl


@pytest.fixture(scope="module")
def own():
    return M.own_strips()


@pytest.mark.parametrize("k", M.BOUNDS)
@pytest.mark.parametrize("which", (4, 5))
def test_bounded_strip_loops(hip, own, which, k):
    """PropagateStrip and StabiliseOptionsStrip under max_iters = 1 .. 4: flags 7 and the planes
    after exactly k iterations where the bound stops the loop (k_stable_strip stores them), the
    unbounded answer where it does not; at 4 nothing is stopped"""
    starts, columns, _ = own
    planes, flags = M.bounded_strips()[which, k]
    got, fl = strip_run(hip, starts, columns, which, k)
    assert (fl == flags).all(), np.flatnonzero(fl != flags)
    assert (got == planes).all(), np.flatnonzero((got != planes).any(axis=(1, 2)))
    # (at 1 every loop that changes anything is stopped: its confirming iteration has not run)
    assert (fl == 7).any() == (k < 4) and (fl == 0).any() and (fl == 1).any() and (fl == 3).any() == (k > 1)


def test_bounded_strip_loop_at_fixed_columns(hip, own):
    """PropagateStrip under max_iters = 2 at columns 0, 1, 2, 31, 61, 62, 63 of every object"""
    starts = own[0]
    planes, flags = M.bounded_strips()["columns"]
    got, fl = strip_run(hip, np.repeat(starts[:, None], 7, axis=1), np.tile(C.STRIP_COLUMNS, len(starts)), 4, 2)
    assert (fl == flags.reshape(-1)).all()
    assert (got == planes.reshape(-1, 10, 64)).all()
    assert (fl == 7).sum() >= 8


@pytest.mark.parametrize("which", range(4))
def test_single_strip_passes_ignore_the_bound(hip, own, which):
    starts, columns, want = own
    got, fl = strip_run(hip, starts, columns, which, 1)
    assert (fl == want[which][1]).all() and (got == want[which][0]).all()
    free, ffl = strip_run(hip, starts, columns, which, 0)
    assert (fl == ffl).all() and (got == free).all()


@pytest.mark.parametrize("which", range(6))
def test_strip_column_high_bits(hip, own, which):
    """only the low six bits of a column count"""
    starts, columns, want = own
    for high in (0x40, 0x80, 0xC0):
        got, fl = strip_run(hip, starts, columns | np.uint8(high), which)
        assert (fl == want[which][1]).all(), high
        assert (got == want[which][0]).all(), high
    assert len(set(columns.tolist())) == 64


def sandwich(stopped):
    """an order of the rows in which unstopped and stopped ones take turns for as long as both
    last: a stopped object then lies between two that are written"""
    s, f = list(np.flatnonzero(stopped)), list(np.flatnonzero(~stopped))
    order = []
    while s and f:
        order += [f.pop(0), s.pop(0)]
    return np.array(order + f + s)


@pytest.mark.parametrize("k", M.BOUNDS)
@pytest.mark.parametrize("form", ("per", "one"))
def test_bounded_test_unknowns(hip, port, form, k):
    """TestUnknowns under max_iters = 1 .. 4, the cells per object and one universe for all: an
    object that the bound stops -- at its first cell, or at a later one after earlier cells have
    changed it in registers -- returns 4 and keeps every byte; the objects around it are the
    model's"""
    b = M.bounded_unknowns(port)
    planes, flags, stops = b.want[form, k]
    order = sandwich(flags == 4)
    g = Guarded(b.after[order])
    cells = dev(b.per[order]) if form == "per" else dev(b.one[None])
    fl = host_flags(hip.stable_test_unknowns(g.out, cells, max_iters=k))
    got = g.result()
    assert (fl == flags[order]).all(), order[fl != flags[order]]
    assert (got == planes[order]).all(), order[(got != planes[order]).any(axis=(1, 2))]
    first, later = M.stop_cells([stops[j] for j in order])
    assert len(first) >= 2 and (len(later) >= 2 or k == 1)
    for rows in (first, later):
        assert (fl[rows] == 4).all() and (got[rows] == b.after[order][rows]).all()
    inside = np.flatnonzero(fl[1:-1] == 4) + 1
    assert ((fl[inside - 1] != 4) & (fl[inside + 1] != 4)).sum() >= 2


@pytest.mark.parametrize("k", M.PAT_BOUNDS + (11,))
def test_bounded_propagate_and_test(hip, port, k):
    """PropagateAndTest under max_iters = k: wherever the bound stops the run -- the first
    Propagate, a later one, a PropagateStrip at the first or a later cell of any round, the
    outer loop -- the object returns 4 and keeps every byte, next to objects that finish; the
    same device batch, run again without a bound, is the unbounded answer.  At 10 and 11
    nothing is stopped."""
    b = M.bounded_propagate_and_test(port)
    planes, flags, ends = b.want[k] if k in b.want else (*b.free, None)
    order = sandwich(flags == 4)
    g = Guarded(b.given[order])
    fl = host_flags(hip.stable_propagate_and_test(g.out, max_iters=k))
    got = g.result()
    assert (fl == flags[order]).all(), order[fl != flags[order]]
    assert (got == planes[order]).all(), order[(got != planes[order]).any(axis=(1, 2))]
    stopped = fl == 4
    if k >= 10:
        assert not stopped.any() and (fl == b.free[1][order]).all() and (got == b.free[0][order]).all()
        return
    sites = {}
    for row, j in enumerate(order):
        if ends[j]["site"] != "finished":
            sites.setdefault((ends[j]["site"], min(ends[j]["round"], 2), ends[j]["cells"] > 0), []).append(row)
    assert sites and sum(map(len, sites.values())) == stopped.sum()
    for site, rows in sites.items():
        assert (fl[rows] == 4).all() and (got[rows] == b.given[order][rows]).all(), site
    fl2 = host_flags(hip.stable_propagate_and_test(g.out))
    again = g.result()
    assert (fl2[stopped] == b.free[1][order][stopped]).all()
    assert (again[stopped] == b.free[0][order][stopped]).all()
    # (a finished, consistent object is a fixpoint of PropagateAndTest: its last round changed nothing)
    done = ~stopped & (fl != 0)
    assert (fl2[done] == 1).all() and (again[done] == got[done]).all()

