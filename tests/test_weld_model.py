"""CPU: numpy definitions of LifeWeld::FromRequired, ToTarget, ToStable and
InteractionOffsets (LifeWeld.hpp:133-400), pinned to every answer the reference
recorded in tests/golden/weld_family.npz.  They work on cell arrays and integer counts,
not on bit planes, so they share nothing with the kernels but the definitions.

ToStable(active, duration, mask) is written twice: as the reference's two
replays, and as the one fused replay the kernel and the facade run (with the
early stop at a fixed point).  Both must equal the recording on every case.

Every term of the definitions must count: with any single RestrictOptions line,
the SetOff(everActive), any of the seven convolutions or either masking oddity
taken out (TERMS), the definition contradicts at least one recorded answer.  The
witnesses are printed by `python tests/test_weld_model.py`.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import weld_cases as C  # noqa: E402

GOLDEN = C.FIXTURE
PLANES = ("state", "unknown", "live2", "live3", "dead0", "dead1", "dead2", "dead4", "dead5", "dead6")
OPTIONS = PLANES[2:]
NOBODY = frozenset()


# ---- cells <-> words: cells[x, y] = bit y of column x -----------------------------

def cells(words):
    w = np.ascontiguousarray(words, np.uint64)
    return ((w[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool)


def words(c):
    return (c.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(axis=-1, dtype=np.uint64)


def count(c):
    """the 3 x 3 count, the centre included"""
    n = np.zeros(c.shape, np.int64)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            n += np.roll(c, (dx, dy), (0, 1))
    return n


def zoi(c):
    return count(c) > 0


def frozen_number(w):
    return 4 * w[1].astype(np.int64) + 2 * w[2] + w[3]


def weld_step(state, w):
    """LifeWeld::Step (LifeWeld.hpp:169-186): the Life rule on (count + frozen) mod 8"""
    t = (count(state) + frozen_number(w)) % 8
    return (t == 3) | (state & (t == 4))


def convolve(a, b):
    """Convolve (LifeAPI.hpp:1293-1370): a cell where a and b, moved there, meet"""
    if not a.any() or not b.any():
        return np.zeros((64, 64), bool)
    return np.fft.irfft2(np.fft.rfft2(a.astype(float)) * np.fft.rfft2(b.astype(float)), (64, 64)) > 0.5


def mirrored(c):
    return np.roll(c[::-1, ::-1], (1, 1), (0, 1))       # (x, y) -> (-x, -y)


# ---- the four functions ---------------------------------------------------------

def from_required(state, required):
    s, r = cells(state), cells(required)
    reach = zoi(zoi(s) & ~r)
    stator = s & ~reach
    kept = s & ~stator
    n = count(kept)
    frozen = (reach & r) | (((n == 3) | (kept & (n == 4))) & ~kept)
    c = count(stator) * frozen                            # (bit 3 of the count is dropped)
    return np.stack([words(kept), words((c & 4) > 0), words((c & 2) > 0), words((c & 1) > 0)])


def to_target(weld):
    w = cells(weld)
    s = w[0]
    return np.stack([words(s), words(zoi(s & ~(w[1] | w[2] | w[3])) & ~s)])


class Stable:
    def __init__(self):
        self.p = {n: np.zeros((64, 64), bool) for n in PLANES}
        self.p["unknown"][:] = True

    def restrict(self, which, keep):
        """RestrictOptions: `which` lose every option not in `keep`"""
        for n in OPTIONS:
            if n not in keep:
                self.p[n] |= which

    def set_on(self, which):
        self.p["state"] |= which
        self.p["unknown"] &= ~which
        self.restrict(which, ("live2", "live3"))

    def set_off(self, which):
        self.p["state"] &= ~which
        self.p["unknown"] &= ~which
        self.restrict(which, OPTIONS[2:])

    def words(self):
        return np.stack([words(self.p[n]) for n in PLANES])


# (who, (sum count, kept option)) of ToStable()'s seven lines
STATIC_LINES = [("live", 3, "live2"), ("live", 4, "live3"), ("dead", 1, "dead1"), ("dead", 2, "dead2"),
                ("dead", 4, "dead4"), ("dead", 5, "dead5"), ("dead", 6, "dead6")]
# the replay's fourteen: (fate, count of current, count of state, option): born cells
# KEEP the option, cells that stay dead LOSE it
REPLAY_LINES = [("born", 3, 0, "dead0"), ("born", 3, 1, "dead1"), ("born", 3, 2, "dead2"),
                ("stay", 1, 0, "dead2"), ("stay", 2, 0, "dead1"), ("stay", 2, 1, "dead2"), ("stay", 1, 2, "dead4"),
                ("stay", 0, 2, "dead5"), ("stay", 3, 4, "dead4"), ("stay", 2, 4, "dead5"), ("stay", 1, 4, "dead6"),
                ("stay", 3, 5, "dead5"), ("stay", 2, 5, "dead6"), ("stay", 3, 6, "dead6")]
# (LifeWeld.hpp:376-394 has fourteen RestrictOptions lines: three for births, eleven
# for cells that stay dead)
STATIC_TERMS = [f"static:{who}{n}" for who, n, _ in STATIC_LINES]
REPLAY_TERMS = [f"replay:{fate}{now}_{mine}" for fate, now, mine, _ in REPLAY_LINES]


def to_stable0(weld, omit=NOBODY):
    w = cells(weld)
    s, frozen = w[0], w[1] | w[2] | w[3]
    total = (count(s) + frozen_number(w)) % 16            # four bits, the last carry dropped
    st = Stable()
    st.set_on(s)
    st.set_off(~s & zoi(s & ~frozen))
    for (who, n, keep), term in zip(STATIC_LINES, STATIC_TERMS):
        if term not in omit:
            st.restrict(frozen & (s if who == "live" else ~s) & (total == n), (keep,))
    return st


def replay_lines(st, w, cur, nxt, mask, mine, omit):
    s = w[0]
    dead = mask & ~s & ~cur
    fate = {"born": dead & nxt, "stay": dead & ~nxt}
    now = count(cur)
    for (f, a, b, opt), term in zip(REPLAY_LINES, REPLAY_TERMS):
        if term in omit:
            continue
        which = fate[f] & (now == a) & (mine == b)
        st.restrict(which, (opt,) if f == "born" else tuple(o for o in OPTIONS if o != opt))


def to_stable_two_replays(weld, active, duration, mask, omit=NOBODY):
    """as the reference writes it (LifeWeld.hpp:327-400)"""
    st = to_stable0(weld, omit)
    w, s, m = cells(weld), cells(weld)[0], cells(mask)
    ever, cur = np.zeros((64, 64), bool), s | cells(active)
    for _ in range(duration):
        ever |= s ^ cur
        cur = weld_step(cur, w)
    if "set_off_ever_active" not in omit:
        st.set_off(m & ~s & ever)
    mine, cur = count(s), s | cells(active)
    for _ in range(duration):
        nxt = weld_step(cur, w)
        replay_lines(st, w, cur, nxt, m, mine, omit)
        cur = nxt
    return st.words()


def to_stable_fused(weld, active, duration, mask, settled=None):
    """one replay, stopping after the first generation that repeats itself;
    settled (a list) receives the number of generations replayed"""
    st = to_stable0(weld)
    w, s, m = cells(weld), cells(weld)[0], cells(mask)
    ever, cur, mine, g = np.zeros((64, 64), bool), s | cells(active), count(s), 0
    while g < duration:
        g += 1
        ever |= s ^ cur
        nxt = weld_step(cur, w)
        replay_lines(st, w, cur, nxt, m, mine, NOBODY)
        if (nxt == cur).all():
            break
        cur = nxt
    st.set_off(m & ~s & ever)
    if settled is not None:
        settled.append(g)
    return st.words()


def side_planes(s):
    n = count(s)
    return {"cells": s, "dead1": ~s & (n == 1), "dead2": ~s & (n == 2), "live3": s & (n == 3), "live4up": s & (n >= 4),
            "dead2up": ~s & (n >= 2), "dead1up": ~s & (n >= 1)}


# (first operand, second operand); a/b = the side, then the plane
OFFSET_TERMS = [("a.cells", "b.cells"), ("a.dead1", "b.dead2"), ("b.dead1", "a.dead2"), ("a.live3", "b.dead2up"),
                ("a.live4up", "b.dead1up"), ("b.live3", "a.dead2up"), ("b.live4up", "a.dead1up")]
CONVOLUTION_TERMS = [f"offsets:{x}*{y}" for x, y in OFFSET_TERMS]
ODDITY_TERMS = ["oddity:b.dead2_under_a", "oddity:a.dead2_under_b"]


def interaction_offsets(weld, other, omit=NOBODY):
    a, b = cells(weld), cells(other)
    keep = {"a": zoi(a[0] & ~(a[1] | a[2] | a[3])), "b": mirrored(zoi(b[0] & ~(b[1] | b[2] | b[3])))}
    planes = {"a": side_planes(a[0]), "b": side_planes(mirrored(b[0]))}
    out = np.zeros((64, 64), bool)
    for i, ((x, y), term) in enumerate(zip(OFFSET_TERMS, CONVOLUTION_TERMS)):
        if term in omit:
            continue
        (xs, xp), (ys, yp) = x.split("."), y.split(".")
        first, second = planes[xs][xp], planes[ys][yp]
        if i > 0:
            first = first & keep[xs]
            # the birth terms cut the second operand by the FIRST one's side (LifeWeld.hpp:238-239)
            odd = i in (1, 2) and ODDITY_TERMS[i - 1] not in omit
            second = second & keep[xs if odd else ys]
        out |= convolve(first, second)
    return words(out)


TERMS = STATIC_TERMS + REPLAY_TERMS + ["set_off_ever_active"] + CONVOLUTION_TERMS + ODDITY_TERMS


# ---- the recording ----------------------------------------------------------------

class Recording:
    def __init__(self, port):
        g = dict(np.load(GOLDEN))
        self.pairs = C.pairs(port)
        self.from_required = g["from_required"].reshape(-1, 4, 64)
        self.welds = C.welds(port, self.from_required)
        self.names = list(self.welds)
        self.target = g["target"].reshape(-1, 2, 64)
        self.stable0 = g["stable0"].reshape(-1, 10, 64)
        self.stable = g["stable"].reshape(-1, 10, 64)
        self.offsets = g["offsets"].reshape(len(C.OFFSET_OTHERS), len(C.OFFSET_WELDS), 64)
        self.state_offsets = g["state_offsets"].reshape(len(C.OFFSET_WELDS), 64)
        self.actives, self.masks = C.actives(port), C.masks(port)
        assert len(self.target) == len(self.stable0) == len(self.names) and len(self.stable) == len(C.STABLE_CASES)

    def stable_inputs(self, case):
        w, a, d, m = case
        return self.welds[w], self.actives[a], d, self.masks[m]


@pytest.fixture(scope="module")
def rec(port):
    return Recording(port)


def test_from_required(rec):
    for (name, (s, r)), want in zip(rec.pairs.items(), rec.from_required):
        assert (from_required(s, r) == want).all(), name
    for name in C.REFERENCE_PAIRS:       # the reference's own test: a still life with a frozen count
        w = rec.welds[name]
        assert (words(weld_step(cells(w)[0], cells(w))) == w[0]).all() and w[1:].any(), name


def test_to_target(rec):
    for (name, w), want in zip(rec.welds.items(), rec.target):
        assert (to_target(w) == want).all(), name


def test_to_stable_static(rec):
    for (name, w), want in zip(rec.welds.items(), rec.stable0):
        assert (to_stable0(w).words() == want).all(), name


def test_to_stable_two_replays_and_fused(rec):
    """the reference's two replays and the kernel's one are the same function"""
    early = 0
    for case, want in zip(C.STABLE_CASES, rec.stable):
        settled = []
        assert (to_stable_two_replays(*rec.stable_inputs(case)) == want).all(), case
        assert (to_stable_fused(*rec.stable_inputs(case), settled=settled) == want).all(), case
        early += settled[0] < case[2]
    assert early >= 3          # the early stop is taken, and changes nothing


def test_duration_zero_is_the_static_form(rec):
    for case, want in zip(C.STABLE_CASES, rec.stable):
        if case[2] == 0:
            assert (want == rec.stable0[rec.names.index(case[0])]).all()
            assert (to_stable_fused(rec.welds[case[0]], rec.actives["soup2"], 0, rec.masks["soup"]) == want).all()


def test_interaction_offsets(rec):
    for i, o in enumerate(C.OFFSET_OTHERS):
        for j, n in enumerate(C.OFFSET_WELDS):
            assert (interaction_offsets(rec.welds[n], rec.welds[o]) == rec.offsets[i, j]).all(), (n, o)


def test_no_frozen_count_is_the_state_form(rec):
    """with no frozen count on either side the result lies inside
    LifeState::InteractionOffsets of the states, and equals it where a's ZOI covers
    everything (the oddity cuts b's birth plane by a's region)"""
    i = C.OFFSET_OTHERS.index("plain_eater")
    seen = 0
    for j, n in enumerate(C.OFFSET_WELDS):
        if n.startswith("plain_"):
            assert not (rec.offsets[i, j] & ~rec.state_offsets[j]).any(), n
            seen += 1
    j = C.OFFSET_WELDS.index("plain_lattice")
    assert (rec.offsets[i, j] == rec.state_offsets[j]).all() and seen >= 4


def witnesses(rec):
    """term -> the first recorded case that the definition without it contradicts"""
    found = {}
    for term in TERMS:
        omit = frozenset([term])
        if term.startswith("static:"):
            hits = (n for (n, w), want in zip(rec.welds.items(), rec.stable0) if (to_stable0(w, omit).words() != want).any())
        elif term.startswith("replay:") or term == "set_off_ever_active":
            hits = (c for c, want in zip(C.STABLE_CASES, rec.stable)
                    if (to_stable_two_replays(*rec.stable_inputs(c), omit=omit) != want).any())
        else:
            hits = ((n, o) for i, o in enumerate(C.OFFSET_OTHERS) for j, n in enumerate(C.OFFSET_WELDS)
                    if (interaction_offsets(rec.welds[n], rec.welds[o], omit) != rec.offsets[i, j]).any())
        found[term] = next(hits, None)
    return found


def test_every_term_has_a_witness(rec):
    assert len(STATIC_TERMS) == 7 and len(CONVOLUTION_TERMS) == 7 and len(TERMS) == len(set(TERMS))
    found = witnesses(rec)
    assert not [t for t, w in found.items() if w is None], found


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle.oracle import Port
    for t, w in witnesses(Recording(Port())).items():
        print(f"| {t} | {w} |")
