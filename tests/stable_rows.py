"""Which truth-table rows do LifeStable planes feed the three fragment
networks, and a batch that feeds them every row they can ever get.

The count / signal / vulnerable networks (lifeapi_amd/csrc/stable_*_circuit.inc)
are exact only on the care set, tools/cgp_stable.py reachable_rows.  This
module is the row model the tests share:

  cell_rows / rows_of   the row every cell of a board presents to each
                        fragment (the formation the passes do, restated
                        with numpy on NeighbourCount's inclusive 3x3 count);
  enumerated_rows       the rows of all 4^9 neighbourhoods, options free;
  covering_batch        seeded boards of 3x3 probes, one per care row (and
                        per count 8 / 9 that aliases 0 / 1 mod 8), that
                        together present every care row.

Planes are (n, 640) uint64: {state, unknown, live2, live3, dead0, dead1,
dead2, dead4, dead5, dead6} x 64 columns; word x is column x, bit y is row y.
Cell arrays are bool with trailing axes (x, y).  A row index has input x[i]
of the fragment as bit i (the order of tests/golden/stable_*_tt.npz).
"""
from __future__ import annotations

import ctypes
import os
import sys
from dataclasses import dataclass

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
FRAGMENTS = ("count", "signal", "vulnerable")
PITCH, SIDE = 5, 12           # probes on a pitch of 5: 12 x 12 per board
PER_BOARD = SIDE * SIDE
ARRANGEMENTS = 4              # placements of its neighbours tried per probe before it goes alone
# Vulnerable's result is an AND of an "on" and an "off" side, so what a probe's
# centre puts out shows only where its neighbours' outputs let it through: its
# probes come once per density of ruled-out options in the 8 neighbours
# (test_stable_rows.py KILLED has what that buys).  The centre's option byte is
# the row's; count and signal probes keep their neighbours' options open.
NB_OPTION_DENSITY = (0.0, 0.5, 0.15, 0.85)
_NB = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))


def care_rows(fragment: str) -> np.ndarray:
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    from cgp_stable import reachable_rows
    return reachable_rows(fragment)


def tables() -> dict:
    """the reference fragments' complete truth tables, (outputs, 2^inputs) uint8"""
    return {f: np.ascontiguousarray(np.load(os.path.join(GOLD, f"stable_{f}_tt.npz"))["tt"].astype(np.uint8))
            for f in FRAGMENTS}


# ---- the row model ----

def _inclusive_count(plane: np.ndarray) -> np.ndarray:
    """NeighbourCount (NeighbourCount.hpp:40-70) per cell of bool planes on
    the torus of their last two axes: the 3x3 block's population, centre
    included"""
    p = plane.astype(np.int32)
    return sum(np.roll(np.roll(p, dx, -2), dy, -1) for dx in (-1, 0, 1) for dy in (-1, 0, 1))


def _rowint(cols):
    return sum(np.asarray(c).astype(np.int32) << i for i, c in enumerate(cols))


def _bits(v, hi):
    return [(v >> k) & 1 for k in range(hi, -1, -1)]


def _count_rows(on_c, off_c, st, off):
    return _rowint(_bits(on_c % 8, 2) + _bits(off_c, 3) + [st, off])


def _signal_rows(opt, on_c, m_c, st, un):
    return _rowint(list(opt) + _bits(on_c % 8, 2) + _bits(m_c, 3) + [st, un])


def _vulnerable_rows(opt, on_c, u_c):
    return _rowint(list(opt) + _bits(on_c % 8, 2) + _bits(u_c, 3))


def cell_rows(st, un, opt, fragments=FRAGMENTS) -> dict:
    """the row each cell presents to each fragment: st, un bool (..., X, Y)
    on the torus of the last two axes, opt the 8 option planes live2 .. dead6"""
    st, un = np.asarray(st, bool), np.asarray(un, bool)
    off = ~un & ~st
    on_c = _inclusive_count(st)
    out = {}
    if "count" in fragments:
        out["count"] = _count_rows(on_c, _inclusive_count(off), st, off)
    if "signal" in fragments:
        out["signal"] = _signal_rows(opt, on_c, _inclusive_count(st | un), st, un)
    if "vulnerable" in fragments:
        out["vulnerable"] = _vulnerable_rows(opt, on_c, _inclusive_count(un))
    return out


def unpack(planes: np.ndarray) -> np.ndarray:
    """(n, 640) uint64 planes -> (n, 10, 64, 64) bool cells [plane, x, y]"""
    p = np.ascontiguousarray(planes, dtype=np.uint64).reshape(-1, 10, 64, 1)
    return np.unpackbits(p.view(np.uint8), axis=3, bitorder="little").astype(bool)


def pack(cells: np.ndarray) -> np.ndarray:
    """(n, 10, 64, 64) bool cells -> (n, 640) uint64 planes"""
    b = np.packbits(np.asarray(cells, bool), axis=3, bitorder="little")
    return np.ascontiguousarray(b).view(np.uint64).reshape(-1, 640)


def rows_of(planes: np.ndarray, fragments=FRAGMENTS) -> dict:
    """{fragment: int array (n, 64, 64) [board, x, y]}: the row every cell of
    every board of (n, 640) planes presents to the fragment's network"""
    c = unpack(planes)
    return cell_rows(c[:, 0], c[:, 1], [c[:, 2 + k] for k in range(8)], fragments)


def row_set(planes: np.ndarray, fragment: str, chunk: int = 256) -> np.ndarray:
    """the sorted distinct rows of rows_of(planes)[fragment], a chunk of
    boards at a time"""
    planes = np.asarray(planes).reshape(-1, 640)
    seen = [np.unique(rows_of(planes[i:i + chunk], (fragment,))[fragment]) for i in range(0, len(planes), chunk)]
    return np.unique(np.concatenate(seen)) if seen else np.zeros(0, np.int32)


def enumerated_rows() -> dict:
    """{fragment: sorted rows} over all 4^9 3x3 neighbourhoods of (state,
    unknown) cells, the centre's 8 options free (they are the low 8 bits of
    a signal / vulnerable row, so every class of counts takes all 256)"""
    t = (np.arange(4 ** 9)[:, None] >> (2 * np.arange(9))) & 3      # cell 4 is the centre
    st, un = (t & 1).astype(bool), (t >> 1).astype(bool)
    off = ~st & ~un
    on_c, off_c, m_c, u_c = st.sum(1), off.sum(1), (st | un).sum(1), un.sum(1)
    none = [np.zeros(len(t), bool)] * 8
    opts = np.arange(256)
    return {"count": np.unique(_count_rows(on_c, off_c, st[:, 4], off[:, 4])),
            "signal": np.unique(np.unique(_signal_rows(none, on_c, m_c, st[:, 4], un[:, 4]))[:, None] | opts),
            "vulnerable": np.unique(np.unique(_vulnerable_rows(none, on_c, u_c))[:, None] | opts)}


# ---- the oracle's passes, restated on rows (to place probes; the tests
# ---- check every board it packs with the oracle itself) ----

def _hollow(s):
    return sum(np.roll(np.roll(s, dx, -2), dy, -1) for dx, dy in _NB).astype(bool)


def signal_consistent(st, un, opt, tt_signal) -> np.ndarray:
    """SignalNeighbours' verdict (LifeStable.hpp:617-675: no unknown cell is
    signalled both ways) per torus of the last two axes"""
    r = cell_rows(st, un, opt, ("signal",))["signal"]
    soff, son, coff, con = (tt_signal[k][r].astype(bool) for k in range(4))
    clash = (_hollow(soff) | coff) & (_hollow(son) | con) & un
    return ~clash.any(axis=(-1, -2))


def count_consistent(st, un, opt, tt_count) -> np.ndarray:
    """UpdateOptions' verdict (LifeStable.hpp:558-615: no cell's row aborts)"""
    r = cell_rows(st, un, opt, ("count",))["count"]
    return ~tt_count[8][r].astype(bool).any(axis=(-1, -2))


# ---- probes ----
# A cell's type is state | unknown << 1: 0 known off, 1 known on, 2 unknown,
# 3 state and unknown both set (the planes may overlap; the passes read it
# as state for the counts of state, as unknown for the counts of unknown).

def _probes(fragment: str, rng):
    """(centre (P,), neighbours (P, 8) cell types in no particular order,
    option byte (P,)): one probe per realisation of the fragment's counts and
    centre -- every count 0..9, so the counts 8 and 9 that alias 0 and 1 in
    the row's three state-count bits come as themselves too -- times every
    option byte where the fragment reads options"""
    centre, nb, opt = [], [], []

    def emit(c, kinds, nopt):
        """nopt probes: centre type c, neighbours the 8 types `kinds`"""
        c = np.full(nopt, c)
        k = np.tile(np.array(kinds), (nopt, 1))
        # a cell in `state` may have `unknown` set too: a coin per such cell
        k = np.where(k == 1, k | (rng.integers(0, 2, k.shape) << 1), k)
        if fragment != "signal":  # (signal reads the centre's unknown bit: its type is the row's)
            c = np.where(c == 1, c | (rng.integers(0, 2, nopt) << 1), c)
        centre.append(c), nb.append(k), opt.append(np.arange(nopt))

    if fragment == "count":      # on = state, off = neither plane, else unknown only
        for c in (1, 0, 2):
            for a in range(9):
                for b in range(9 - a):
                    emit(c, [1] * a + [0] * b + [2] * (8 - a - b), 1)
    elif fragment == "signal":   # in state, unknown only, neither
        for c in range(4):
            for a in range(9):
                for b in range(9 - a):
                    emit(c, [1] * a + [2] * b + [0] * (8 - a - b), 256)
    else:                        # vulnerable: counts of state and of unknown, overlapping at will
        for s in range(10):
            for u in range(10):
                ways = [(c, o) for c in range(4) for o in range(9)
                        if 0 <= s - (c & 1) <= 8 and 0 <= u - (c >> 1) <= 8
                        and max(0, s - (c & 1) + u - (c >> 1) - 8) <= o <= min(s - (c & 1), u - (c >> 1))]
                pick = rng.integers(0, len(ways), 256)
                c = np.array([ways[i][0] for i in pick])
                k = np.zeros((256, 8), np.int64)
                for i, w in enumerate(pick):
                    a, b, o = s - (ways[w][0] & 1), u - (ways[w][0] >> 1), ways[w][1]
                    k[i] = [3] * o + [1] * (a - o) + [2] * (b - o) + [0] * (8 - a - b + o)
                centre.append(c), nb.append(k), opt.append(np.arange(256))
    return np.concatenate(centre), np.concatenate(nb), np.concatenate(opt)


def _probe_rows(fragment, centre, nb, opt):
    """the row each probe's centre presents"""
    cells = np.concatenate([nb[:, :4], centre[:, None], nb[:, 4:]], axis=1)
    st, un = (cells & 1).astype(bool), (cells >> 1).astype(bool)
    off = ~st & ~un
    o = [(opt >> k) & 1 for k in range(8)]
    if fragment == "count":
        return _count_rows(st.sum(1), off.sum(1), st[:, 4], off[:, 4])
    if fragment == "signal":
        return _signal_rows(o, st.sum(1), (st | un).sum(1), st[:, 4], un[:, 4])
    return _vulnerable_rows(o, st.sum(1), un.sum(1))


def _tiles(centre, nb, opt, nbopt):
    """(P, 10, 7, 7) bool: each probe (its centre's option byte opt, its
    neighbours' nbopt) in the middle of a 7 x 7 patch of known-off cells with
    no option ruled out"""
    t = np.zeros((len(centre), 10, 7, 7), bool)
    t[:, 0, 3, 3], t[:, 1, 3, 3] = centre & 1, centre >> 1
    for k in range(8):
        t[:, 2 + k, 3, 3] = (opt >> k) & 1
    for j, (dx, dy) in enumerate(_NB):
        t[:, 0, 3 + dx, 3 + dy], t[:, 1, 3 + dx, 3 + dy] = nb[:, j] & 1, nb[:, j] >> 1
        for k in range(8):
            t[:, 2 + k, 3 + dx, 3 + dy] = (nbopt[:, j] >> k) & 1
    return t


def _place(nboards, board, slot, shift, centre, nb, opt, nbopt, chunk=1024):
    """(nboards, 640) planes: probe i's centre at slot[i] of board[i], the
    board then moved by its shift[board] (so probes straddle column 63|0 and
    row 63|0); every other cell known off, no option ruled out"""
    out = np.zeros((nboards, 640), np.uint64)
    x = (PITCH * (slot // SIDE) + 1 + shift[board, 0]) % 64
    y = (PITCH * (slot % SIDE) + 1 + shift[board, 1]) % 64
    for lo in range(0, nboards, chunk):
        m = (board >= lo) & (board < lo + chunk)
        cells = np.zeros((min(chunk, nboards - lo), 10, 64, 64), bool)
        b, cx, cy = board[m] - lo, x[m], y[m]
        cells[b, 0, cx, cy], cells[b, 1, cx, cy] = centre[m] & 1, centre[m] >> 1
        for k in range(8):
            cells[b, 2 + k, cx, cy] = (opt[m] >> k) & 1
        for j, (dx, dy) in enumerate(_NB):
            cells[b, 0, (cx + dx) % 64, (cy + dy) % 64] = nb[m, j] & 1
            cells[b, 1, (cx + dx) % 64, (cy + dy) % 64] = nb[m, j] >> 1
            for k in range(8):
                cells[b, 2 + k, (cx + dx) % 64, (cy + dy) % 64] = (nbopt[m, j] >> k) & 1
        out[lo:lo + chunk] = pack(cells)
    return out


@dataclass
class Batch:
    fragment: str
    planes: np.ndarray        # (n, 640) uint64
    probe_row: np.ndarray     # (P,) the care row of probe i
    probe_board: np.ndarray   # (P,) the board probe i sits on
    packed: int               # boards 0 .. packed-1 hold up to 144 probes, the rest one each

    def rows_on(self, board: int) -> list:
        return sorted(set(self.probe_row[self.probe_board == board].tolist()))

    def boards_of(self) -> dict:
        """{care row: the boards a probe of it sits on}"""
        d = {}
        for r, b in zip(self.probe_row.tolist(), self.probe_board.tolist()):
            d.setdefault(r, []).append(b)
        return d

    def alone(self, board: int) -> bool:
        return board >= self.packed


def covering_batch(fragment: str, tt: dict | None = None, seed: int = 20250) -> Batch:
    """Boards whose cells present every care row of `fragment`.  Probes sit
    144 to a board.  A pass's verdict is one flag per board, and
    SignalNeighbours leaves the planes of an inconsistent board alone, so a
    probe that its pass (SignalNeighbours; UpdateOptions for count) finds
    inconsistent in every one of ARRANGEMENTS placements of its neighbours
    gets a board to itself, and the packed boards are consistent.  The
    verdicts come from the restatements above on the probe in a 7 x 7 patch
    (probes two cells apart do not interact: signals reach one cell, and only
    unknown cells, all inside probes, can clash); the tests check every board
    with the oracle.  count has one more board, of all its probes together
    (UpdateOptions writes the option planes whatever its flag says).
    Vulnerable has no verdict: all its probes are packed, once per
    NB_OPTION_DENSITY.  Every board is moved by a seeded (dx, dy), so probes
    straddle column 63|0 and row 63|0."""
    tt = tt or tables()
    rng = np.random.default_rng([seed, FRAGMENTS.index(fragment)])
    centre, nb, opt = _probes(fragment, rng)
    nbopt = np.zeros(nb.shape, np.int64)
    if fragment == "vulnerable":
        centre, nb, opt = (np.concatenate([a] * len(NB_OPTION_DENSITY)) for a in (centre, nb, opt))
        nbopt = np.concatenate([_rowint(rng.random((8,) + nbopt.shape) < d).astype(np.int64)
                                for d in NB_OPTION_DENSITY])
    rows = _probe_rows(fragment, centre, nb, opt)
    nb = rng.permuted(nb, axis=1)
    lone = np.zeros(len(rows), bool)      # probes that go alone, not packed
    verdict = {"signal": signal_consistent, "count": count_consistent}.get(fragment)
    if verdict:
        lone[:] = True
        for k in range(ARRANGEMENTS):
            idx = np.nonzero(lone)[0]
            if k:
                nb[idx] = rng.permuted(nb[idx], axis=1)
            t = _tiles(centre[idx], nb[idx], opt[idx], nbopt[idx])
            ok = verdict(t[:, 0], t[:, 1], [t[:, 2 + j] for j in range(8)], tt[fragment])
            lone[idx[ok]] = False
    pk = np.nonzero(~lone)[0]
    pk = pk[rng.permutation(len(pk))]     # neighbours on a board are not neighbours in the row order
    if fragment == "count":               # and one board of all the probes, aborting or not
        assert len(rows) <= PER_BOARD and len(pk) <= PER_BOARD
        pk = np.concatenate([pk, np.full(PER_BOARD - len(pk), -1), rng.permutation(len(rows))])
    al = np.nonzero(lone)[0]
    npk = -(-len(pk) // PER_BOARD)
    order = np.concatenate([pk, al])
    board = np.concatenate([np.arange(len(pk)) // PER_BOARD, npk + np.arange(len(al))])
    slot = np.concatenate([np.arange(len(pk)) % PER_BOARD, rng.integers(0, PER_BOARD, len(al))])
    order, board, slot = order[order >= 0], board[order >= 0], slot[order >= 0]
    n = npk + len(al)
    shift = rng.integers(0, 64, (n, 2))
    planes = _place(n, board, slot, shift, centre[order], nb[order], opt[order], nbopt[order])
    return Batch(fragment, planes, rows[order], board, npk)


# ---- the oracle with any tables ----

_u8p = ctypes.POINTER(ctypes.c_uint8)
_u64p = ctypes.POINTER(ctypes.c_uint64)


def oracle_pass(port, planes, which: int, tt: dict):
    """port.stable_pass with the count / signal tables given (a mutant's, say)"""
    out = np.ascontiguousarray(planes, dtype=np.uint64).reshape(-1, 640).copy()
    flags = np.zeros(len(out), np.uint8)
    tc, ts = tt["count"].ctypes.data_as(_u8p), tt["signal"].ctypes.data_as(_u8p)
    for u in range(len(out)):
        flags[u] = port.lib.oracle_stable_pass(out[u].ctypes.data_as(_u64p), which, tc, ts)
    return out, flags


def oracle_vulnerable(port, planes, tt: dict):
    src = np.ascontiguousarray(planes, dtype=np.uint64).reshape(-1, 640)
    out = np.zeros((len(src), 64), np.uint64)
    tv = tt["vulnerable"].ctypes.data_as(_u8p)
    for u in range(len(src)):
        port.lib.oracle_stable_vulnerable(src[u].ctypes.data_as(_u64p), out[u].ctypes.data_as(_u64p), tv)
    return out
