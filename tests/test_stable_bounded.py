"""Propagate and StabiliseOptions iteration by iteration: lifeapi_stable_pass_batch_dev
with max_iters = k against k iterations of the oracle, for every k.

Propagate's iterations after the first run on a 32-row window around the
previous iteration's changes (stable_kernels.hpp stable_iter_window).
Propagation is monotone and confluent, so a window iteration that misses a
deduction, or notices an inconsistency one iteration late, still reaches the
fixpoint the comparison at max_iters = 0 checks; stopping after every k pins
each iteration's planes and flags by themselves.  The inputs
(tests/stable_bounded_cases.py) are chosen for depth and for window iterations
at every row offset; the CPU tests below hold them to that by the oracle alone,
and hold the bounded oracle (Port.stable_pass_bounded, composed from the single
passes) to the unbounded one and to the reference's own members.
"""
import numpy as np
import pytest

import stable_bounded_cases as C

SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)
PASS_NAME = {4: "propagate", 5: "stabilise"}


class Families:
    """the batches, their oracle traces and bounded results, computed once"""

    def __init__(self, port):
        self.port = port
        self.x = {"strips": C.strips(), "soups": C.soups(port), "far": C.far_reaching(port)}
        for x in self.x.values():
            x.flags.writeable = False
        self._trace, self._want = {}, {}

    def trace(self, name, which):
        if (name, which) not in self._trace:
            self._trace[name, which] = C.Trace(self.port, self.x[name], which)
        return self._trace[name, which]

    def want(self, name, which, k):
        """Port.stable_pass_bounded(x, which, k): (planes, flags), not to be modified"""
        if (name, which, k) not in self._want:
            self._want[name, which, k] = self.port.stable_pass_bounded(self.x[name], which, k)
        return self._want[name, which, k]

    def route(self, name):
        if not hasattr(self, "_route"):
            self._route = {}
        if name not in self._route:
            self._route[name] = C.window_route(self.trace(name, 4))
        return self._route[name]


@pytest.fixture(scope="module")
def fam(port):
    return Families(port)


# ---- CPU: the bounded oracle, and the batches' sharpness -----------------------

def test_bounded_oracle_ends_as_the_unbounded_one(port, fam):
    """stable_pass_bounded(x, w, 0) is stable_pass(x, w), planes and flags, on
    strips, soups and the cascade family; and for every k the bounded result
    is what the iteration trace (stable_bounded_cases.Trace, which keeps every
    iteration's planes) says it is -- flag 7 exactly on the objects that run
    more than k iterations, the planes those after k iterations."""
    batches = dict(fam.x, cascades=C.cascades(port, 200))
    for name, x in batches.items():
        for which in (4, 5):
            got, gfl = port.stable_pass_bounded(x, which, 0)
            want, wfl = port.stable_pass(x, which)
            assert (got == want).all() and (gfl == wfl).all(), (name, which)
    for name in fam.x:
        for which in (4, 5):
            tr = fam.trace(name, which)
            for k in range(1, tr.depth + 2):
                got, gfl = fam.want(name, which, k)
                want, wfl = tr.bounded(k)
                assert (got == want).all() and (gfl == wfl).all(), (name, which, k)
                assert ((gfl == 7) == (tr.iters > k)).all(), (name, which, k)
                assert np.isin(gfl, (0, 1, 3, 7)).all()
            got, gfl = fam.want(name, which, tr.depth + 1)
            want, wfl = port.stable_pass(fam.x[name], which)
            assert (got == want).all() and (gfl == wfl).all(), (name, which)


def test_bounded_oracle_flag_boundary(port, fam):
    """The boundary the header states: an object whose s-th iteration is the
    last that changes anything has flag 7 at max_iters = s (the confirming
    iteration has not run) and 3 from s + 1 on; an object inconsistent at
    iteration j has 7 up to j - 1 and 0 from j on; max_iters = 1 on a fixpoint
    gives 1."""
    tr = fam.trace("strips", 4)
    for u in (int(np.argmax(tr.consistent & (tr.iters >= 5))), int(np.argmax(~tr.consistent & (tr.iters >= 3)))):
        j = int(tr.iters[u])
        x = fam.x["strips"][u:u + 1]
        fl = [int(port.stable_pass_bounded(x, 4, k)[1][0]) for k in range(1, j + 2)]
        end = 3 if tr.consistent[u] else 0
        assert fl == [7] * (j - 1) + [end, end], (u, fl)
    fix, ffl = port.stable_pass(fam.x["strips"][tr.consistent][:20], 4)
    again, afl = port.stable_pass_bounded(fix, 4, 1)
    assert (ffl == 3).all() and (afl == 1).all() and (again == fix).all()


def test_bounded_oracle_vs_reference_members(port, ref, fam):
    """... and the reference's own Propagate() and StabiliseOptions()
    (LifeStable.hpp:677-729) on a sample of each family"""
    batches = dict(fam.x, cascades=C.cascades(port, 60))
    for name, x in batches.items():
        x = x[::7][:50]
        for which in (4, 5):
            got, gfl = port.stable_pass_bounded(x, which, 0)
            for u in range(len(x)):
                obj = x[u].copy()  # (the reference's pass works in place)
                fl = ref.stable_pass(obj, which)
                assert fl == gfl[u] and (obj == got[u]).all(), (name, which, u)


def test_batches_are_sharp(fam):
    """What the inputs must offer, by the oracle and the restated routing rule
    alone (conditions on the inputs, not measurements of the kernel).  Obtained
    with the committed seeds: strips 1302 window iterations, 698 of them with
    a window first row >= 32, 40 ending inconsistent, every first row 0..63;
    112 objects inconsistent at iteration >= 2; changed-row heights 20 and 21
    both present; the deepest object 14 iterations (StabiliseOptions 11).
    soups: no window iteration, the deepest object 13 iterations
    (StabiliseOptions 15).  far: 38 objects, each with a window iteration
    whose changes lie 2 rows beyond the previous iteration's (38 such
    iterations, 86 at 1 row, 96 at none); on strips the changes never move
    more than 1 row an iteration (178 of the 1302), so strips cannot tell a
    window that looks 1 row beyond from the product's, and far is there to.
    No iteration of any family reaches more than 2 rows -- the window looks
    at RHO = 3."""
    tr, route = fam.trace("strips", 4), fam.route("strips")
    win = {uk: y0 for uk, (y0, _) in route.items() if y0 is not None}
    heights = {h for _, h in route.values()}
    assert len(win) >= 800, len(win)
    assert sum(y0 >= 32 for y0 in win.values()) >= 300
    assert sum(tr.flag[k][u] == 0 for u, k in win) >= 15
    assert int((~tr.consistent & (tr.iters >= 2)).sum()) >= 60
    assert set(win.values()) == set(range(64))
    assert C.WINDOW_FIT in heights and C.WINDOW_FIT + 1 in heights
    assert tr.depth >= 10
    assert all(y0 is None for (_, k), (y0, _) in route.items() if k == 2)  # iteration 1 changes every row
    ts = fam.trace("soups", 4)
    assert ts.depth >= 12, ts.depth
    assert all(y0 is None for y0, _ in fam.route("soups").values())
    assert fam.trace("strips", 5).depth >= 8 and fam.trace("soups", 5).depth >= 8
    reach = {name: C.window_reach(fam.trace(name, 4)) for name in fam.x}
    far = reach["far"]
    assert {u for (u, _), r in far.items() if r == 2} == set(range(len(fam.x["far"])))
    assert sum(fam.trace("far", 4).consistent) >= 20  # (a missed deduction may be made up for before their fixpoint)
    assert max(max(r.values(), default=0) for r in reach.values()) <= C.RHO


# ---- GPU ------------------------------------------------------------------------

def upload(x, aligned=True, guard=False):
    """x on the device in a sentinel-filled buffer, 16-byte aligned or 8 mod 16,
    with one sentinel object before and after when `guard`: (buffer, the (n, 640) view)"""
    import torch
    x = np.ascontiguousarray(x, np.uint64).reshape(-1, 640)
    pad = 640 if guard else 0
    buf = torch.full((x.size + 2 * pad + 2,), int(SENTINEL.view(np.int64)), dtype=torch.int64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    lo = pad + (0 if aligned else 1)
    body = buf[lo:lo + x.size].view(-1, 640)
    body.copy_(torch.from_numpy(x.view(np.int64).copy()))
    assert body.data_ptr() % 16 == (0 if aligned else 8)
    return buf, body


def download(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def guards_intact(buf, body):
    h = download(buf)
    lo = (body.data_ptr() - buf.data_ptr()) // 8
    return bool((h[:lo] == SENTINEL).all() and (h[lo + body.numel():] == SENTINEL).all())


def sweep(hip, fam, name, which):
    tr = fam.trace(name, which)
    route = fam.route(name) if which == 4 else {}
    x = fam.x[name]
    for aligned in (True, False):
        for k in range(1, tr.depth + 2):
            want, wfl = fam.want(name, which, k)
            _, d = upload(x, aligned)
            fl = hip.stable_pass(d, PASS_NAME[which], max_iters=k).cpu().numpy()
            got = download(d)
            bad = np.nonzero((got != want).any(axis=1) | (fl != wfl))[0]
            report = [dict(k=k, object=int(u), oracle_flag=int(wfl[u]), gpu_flag=int(fl[u]),
                           window_iteration=route.get((int(u), k), (None, 0))[0] is not None,
                           window_first_row=route.get((int(u), k), (None, 0))[0],
                           words=int((got[u] != want[u]).sum())) for u in bad[:6]]
            assert bad.size == 0, (name, PASS_NAME[which], "aligned" if aligned else "8 mod 16", bad.size, report)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["strips", "soups", "far"])
def test_propagate_bounded_every_k(hip, fam, name):
    """Propagate with max_iters = k, for every k up to one past the deepest
    object's iterations, on fresh copies: all 640 words and the flag of every
    object against k oracle PropagateSteps, on a 16-byte aligned batch and on
    one that is 8 mod 16.  On strips most iterations from the third on are
    window iterations, at every first row; on soups none is."""
    sweep(hip, fam, name, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["strips", "soups"])
def test_stabilise_bounded_every_k(hip, fam, name):
    """The same for StabiliseOptions; the alignment chooses the kernel
    (16-byte aligned: the LDS-DMA kernel, which stores only the planes that
    changed; 8 mod 16: k_stable)."""
    sweep(hip, fam, name, 5)


def run(hip, x, which, k, aligned=True):
    _, d = upload(x, aligned)
    fl = hip.stable_pass(d, which, max_iters=k).cpu().numpy()
    return download(d), fl


@pytest.mark.gpu
@pytest.mark.parametrize("which", [4, 5])
def test_bound_flag_semantics(hip, port, fam, which):
    """The flag at the bound, on objects the oracle picks (s: an object's
    changing iterations): max_iters = s gives the planes after s iterations --
    the fixpoint's, the confirming iteration changes no plane -- with flag 7;
    s + 1 and 0 the same planes with flag 3; an object inconsistent at
    iteration j gives 0 from max_iters = j on and 7 with the planes of j - 1
    iterations at j - 1; a fixpoint gives 1 for every k >= 1; 2^32 - 1 is as
    0; and the single passes 0-3 ignore max_iters."""
    x, tr = fam.x["strips"], fam.trace("strips", which)
    name = PASS_NAME[which]
    final, ffl = fam.want("strips", which, tr.depth + 1)
    checked = 0
    for j in range(2, tr.depth + 1):
        s = j - 1
        # consistent: iterations 1..s change, iteration j = s + 1 confirms
        pick = np.nonzero(tr.consistent & (tr.iters == j))[0]
        if pick.size:
            assert (tr.after[s][pick] == final[pick]).all()  # (by the oracle: the fixpoint is there after s)
            got, fl = run(hip, x[pick], name, s)
            assert (fl == 7).all() and (got == final[pick]).all(), (name, "s", s, fl)
            for k in (s + 1, 0):
                got, fl = run(hip, x[pick], name, k, aligned=k == 0)
                assert (fl == 3).all() and (got == final[pick]).all(), (name, "s + 1 / 0", s, k, fl)
            checked += pick.size
        # inconsistent at iteration j
        pick = np.nonzero(~tr.consistent & (tr.iters == j))[0]
        if pick.size:
            for k in (j, j + 1, 0):
                got, fl = run(hip, x[pick], name, k)
                assert (fl == 0).all() and (got == final[pick]).all(), (name, "inconsistent at", j, k, fl)
            got, fl = run(hip, x[pick], name, j - 1, aligned=False)
            assert (fl == 7).all() and (got == tr.after[j - 1][pick]).all(), (name, "before inconsistent", j, fl)
            checked += pick.size
    first = np.nonzero(~tr.consistent & (tr.iters == 1))[0]
    got, fl = run(hip, x[first], name, 1)
    assert first.size and (fl == 0).all() and (got == final[first]).all()
    assert checked + first.size == len(x), checked
    # fixpoints
    fix = final[ffl == 3][:100]
    again, afl = port.stable_pass_bounded(fix, which, 1)
    assert len(fix) == 100 and (afl == 1).all() and (again == fix).all()
    for k in (1, 2, 5, 0):
        got, fl = run(hip, fix, name, k, aligned=k != 2)
        assert (fl == 1).all() and (got == fix).all(), (name, "fixpoint", k, fl)
    got, fl = run(hip, x, name, 2 ** 32 - 1)
    assert (fl == ffl).all() and (got == final).all(), name
    if which == 4:
        for w, single in enumerate(hip.STABLE_PASSES[:4]):
            want, wfl = port.stable_pass(x, w)
            for aligned in (True, False):
                got, fl = run(hip, x, single, 1, aligned)
                assert (fl == wfl).all() and (got == want).all(), (single, aligned)


def one_line_cases(tr, steps):
    """(start, objects): objects that still run after `start` iterations and
    whose next `steps` iterations change columns of one 128-byte line (16
    columns of every plane) only"""
    out = []
    for start in range(1, tr.depth - steps + 1):
        end = start + steps
        d = (tr.after[end] != tr.after[start]).reshape(tr.n, 10, 64).any(axis=1)
        lines = d.reshape(tr.n, 4, 16).any(axis=2).sum(axis=1)
        pick = np.nonzero((tr.iters > start) & (lines == 1))[0]
        if pick.size:
            out.append((start, pick))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("which", [4, 5])
def test_bounded_changed_lines_only(hip, port, fam, which):
    """A bounded run stores the 128-byte lines holding a changed column and no
    other: objects taken after `start` oracle iterations whose next 1, 2 or 3
    iterations change columns of one line only (picked by the oracle), the
    device buffer holding the input, compared with the oracle afterwards --
    a change the bounded loop failed to record leaves its line stale.  One
    sentinel object before and after the batch, guard bytes around the flags."""
    import torch
    tr = fam.trace("strips", which)
    seen_lines, total = set(), 0
    for steps in (1, 2, 3):
        cases = one_line_cases(tr, steps)
        assert cases, steps
        x = np.concatenate([tr.after[start][pick] for start, pick in cases])
        want, wfl = port.stable_pass_bounded(x, which, steps)
        d = (want != x).reshape(len(x), 10, 4, 16).any(axis=(1, 3))
        assert (d.sum(axis=1) == 1).all()
        seen_lines |= set(np.nonzero(d.any(axis=0))[0].tolist())
        total += len(x)
        for aligned in (True, False):
            buf, body = upload(x, aligned, guard=True)
            flags = torch.full((len(x) + 32,), 0xA5, dtype=torch.uint8, device="cuda")
            hip._check(hip.lib.lifeapi_stable_pass_batch_dev(body.data_ptr(), flags.data_ptr() + 16, len(x), which,
                                                             steps, hip._stream(None)))
            got, fl = download(body), flags.cpu().numpy()
            assert guards_intact(buf, body), "a sentinel object was written"
            assert (fl[:16] == 0xA5).all() and (fl[16 + len(x):] == 0xA5).all(), "a flags guard byte was written"
            bad = np.nonzero((got != want).any(axis=1) | (fl[16:16 + len(x)] != wfl))[0]
            assert bad.size == 0, (PASS_NAME[which], steps, aligned, bad[:8], fl[16:][bad[:4]], wfl[bad[:4]])
    assert seen_lines == {0, 1, 2, 3} and total >= 100, (seen_lines, total)


@pytest.mark.gpu
def test_bounded_host_pointer_twin(hip, fam):
    """lifeapi_stable_pass_batch (host pointers) hands max_iters on: 67 strips
    at max_iters 1, 3 and 0 against the same oracle"""
    n = 67
    for k in (1, 3, 0):
        want, wfl = fam.want("strips", 4, k if k else fam.trace("strips", 4).depth + 1)
        h = np.ascontiguousarray(fam.x["strips"][:n]).copy()
        flags = np.full(n, 0xA5, np.uint8)
        hip._check(hip.lib.lifeapi_stable_pass_batch(h.ctypes.data, flags.ctypes.data, n, 4, k, 0))
        assert (h == want[:n]).all() and (flags == wfl[:n]).all(), k
    assert {0, 7} <= set(fam.want("strips", 4, 3)[1][:n].tolist()) and {0, 3} <= set(wfl[:n].tolist())
