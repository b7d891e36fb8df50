"""GPU: the launch paths of the product library that only a large batch, a
second call on the same batch or a stream of the caller's own reaches.

* A -- the later chunks of every capped grid (step.hip, reduce.hip,
  cone_launch.hpp): a wave of k_cone_adapt, k_pop<kRedU> or the merged split
  kernel takes a second chunk only once the batch exceeds blocks per CU x CUs
  x 4 waves x universes per chunk, which no other test's batch does; and the
  second object of a wave of k_stable_strip (stable_test.hip), past blocks per
  CU x CUs x 4 objects;
* B -- the reversed launch order of k_weld, k_step_contains<8> and k_step
  (host.hip launch_reverse), with the order of every launch asserted through
  the book (the tuning build's order_probe / order_note);
* C -- every *_dev entry point on a side stream.

Every batch size comes from the constants in the sources and the device's CU
count, so a retune moves the tests.  Every comparison is bit-exact against
the CPU oracle over all n outputs."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from test_gpu_parity import _off8, to_dev, to_host
from test_ref_gpu import _column_box_target

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lifeapi_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools", "tune"))
THREADS = 16
ZERO = np.zeros(64, np.uint64)


def source_constant(name: str) -> int:
    """`constexpr <type> name = <integer or a << b>;` read out of lifeapi_amd/csrc"""
    for f in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, f)) as fh:
            m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*([^;]+);", fh.read())
        if m:
            expr = re.sub(r"(?<=\d)(ull|ul|u)\b", "", m.group(1).strip())
            assert re.fullmatch(r"\d+(\s*<<\s*\d+)?", expr), (name, m.group(1))
            return int(eval(expr, {"__builtins__": {}}))  # noqa: S307 - digits and << only (checked above)
    raise AssertionError(f"constant {name} not found in {CSRC}")


class Limits:
    """the thresholds of the launches, from the sources and the device"""

    def __init__(self, cus: int):
        self.cus = cus
        for name in ("kConeAdaptBlocksPerCU", "kFilterIterBlocksPerCU", "kRedBlocksPerCU", "kRedU",
                     "kOrderMinUniverses", "kFilterOrderUniverses", "kConeWholeWinGens"):
            setattr(self, name, source_constant(name))

    def waves(self, blocks_per_cu: int) -> int:
        return self.cus * blocks_per_cu * 4

    def cap(self, blocks_per_cu: int, universes: int) -> int:
        """universes one pass of a grid capped at blocks_per_cu covers"""
        return self.waves(blocks_per_cu) * universes


@pytest.fixture(scope="module")
def lim(hip):
    return Limits(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module")
def tune(hip):
    import tune_hip
    return tune_hip


# ---- inputs ---------------------------------------------------------------

def hits_of(s: np.ndarray, w: np.ndarray, u: np.ndarray) -> np.ndarray:
    """((s ^ w) & (w | u)) == 0 on every column (the columns without care cells pass)"""
    m = w | u
    cols = np.nonzero(m)[0]
    if len(cols) == 0:
        return np.ones(len(s), bool)
    if len(cols) < 64:
        s, w, m = s[:, cols], w[cols], m[cols]
    return (((s ^ w) & m) == 0).all(axis=1)


def first_hits(states, w, u, gens: int) -> np.ndarray:
    """states[g]: the batch after g generations; first g in 1..gens that hits, 0 = never"""
    res = np.zeros(len(states[0]), np.uint32)
    for g in range(1, gens + 1):
        res[(res == 0) & hits_of(states[g], w, u)] = g
    return res


def soup_with_copies(port, n: int, seed: int, fills: int, gens: int):
    """test_cone_contains_and_filter_vs_reference's construction: a soup of
    ANDed fills in which every 5th universe is a copy of universe 0, whose
    own future the targets are cut from (the hits); and the batch after 1 ..
    gens generations.  So that no stride of 5 hides a misread universe and the
    answers depend on the target, a seeded tenth of the other universes are
    copies with one random cell flipped: those hit exactly when the flip's
    light cone misses the target's care cells."""
    x = port.fill(n, seed=seed)
    for k in range(1, fills):
        x &= port.fill(n, seed=seed + k)
    rng = np.random.default_rng(seed)
    x[::5] = x[0]
    near = np.nonzero(rng.random(n) < 0.1)[0]
    near = near[near % 5 != 0]
    x[near] = x[0]
    x[near, rng.integers(64, size=len(near))] ^= np.uint64(1) << rng.integers(64, size=len(near)).astype(np.uint64)
    states = [x]
    for _ in range(gens):
        states.append(port.step_batch(states[-1], 1, nthreads=THREADS))
    return states


def cut(state: np.ndarray, box: np.ndarray):
    """the target that `state` meets on the cells of `box`"""
    return state & box, box & ~state


def rows_mask(y0: int, h: int) -> np.uint64:
    m = 0
    for r in range(y0, y0 + h):
        m |= 1 << (r % 64)
    return np.uint64(m)


def rows_box(rng, y0: int, h: int) -> np.ndarray:
    """care cells in every column (the whole board at any generation count),
    on rows [y0, y0 + h) mod 64 only, the first and last of them in column 0"""
    full = int(rows_mask(y0, h))
    box = np.array([int(rng.integers(1, 1 << 63)) & full for _ in range(64)], dtype=np.uint64)
    box |= np.uint64(1 << (y0 % 64))
    box[0] |= np.uint64(1 << (y0 % 64) | 1 << ((y0 + h - 1) % 64))
    return box


def full_box(rng) -> np.ndarray:
    """care cells in every column and on rows more than 32 apart: no window"""
    box = np.array([int(rng.integers(1, 1 << 63)) for _ in range(64)], dtype=np.uint64)
    box[0] |= np.uint64(1 | 1 << 20 | 1 << 41)
    return box


# name -> target(rng, state, g): the target cut from `state` (universe 0 after
# g generations) whose light cone over g generations has the named shape
def _columns(x0: int, k: int):
    def make(rng, state, g):
        w = k - 2 * g
        return _column_box_target(rng, state, x0, w) if w >= 1 else None
    return make


def _rows(y0: int, h: int):
    return lambda rng, state, g: cut(state, rows_box(rng, y0, h))


CONE16_TARGETS = {
    "whole_full_height": lambda rng, state, g: cut(state, full_box(rng)),
    "whole_1_row_low": _rows(10, 1),          # PK = 4, y0 < 32
    "whole_1_row_across_63": _rows(63, 1),    # PK = 4, the window from row 62 / 61 on: across row 63
    "whole_10_rows_low": _rows(8, 10),        # PK = 2
    "whole_10_rows_across_63": _rows(59, 10),
    "whole_26_rows_low": _rows(3, 26),        # PK = 1
    "whole_26_rows_across_63": _rows(50, 26),
    "cone_12_columns": _columns(20, 12),      # cone_wave<16,16>
    "cone_24_columns_seam": _columns(52, 24),  # cone_wave<32,16>, across column 63|0
    "cone_40_columns": _columns(7, 40),       # cone_wave<64,16>
}
CONE64_TARGETS = {
    "cone_4_columns": _columns(62, 4),        # cone_wave<4,64> (no such cone at 2 generations)
    "cone_7_columns": _columns(30, 7),        # cone_wave<8,64>
}


def assert_hit_share(hit: np.ndarray, what):
    share = hit.mean()
    assert 0.10 <= share <= 0.90, (what, "the oracle's hit share", float(share))


def assert_second_chunks_mixed(hit: np.ndarray, waves: int, chunk: int, what):
    """the oracle's answers for the universes of every wave's second chunk
    ([waves x chunk, 2 x waves x chunk), `chunk` per wave) hold hits and misses"""
    lo, n = waves * chunk, len(hit)
    assert n > lo, (what, "no wave takes a second chunk", n, lo)
    for a in range(lo, min(2 * lo, n), chunk):
        part = hit[a:a + chunk]
        if len(part) >= 8:  # (a ragged tail of a few universes may be all misses)
            assert part.any() and not part.all(), (what, "second chunk without both answers", a)


class ConeBatch:
    def __init__(self, port, n, seed):
        self.n, self.seed = n, seed
        self.states = soup_with_copies(port, n, seed, fills=2, gens=2)

    def cases(self, name, make):
        """(g, wanted, unwanted, the oracle's answers): Contains at g = 0, the
        filter's first hits at g = 1, 2, the target cut from generation g"""
        out = []
        for g in (0, 1, 2):
            rng = np.random.default_rng(self.seed + 17 * g + sum(map(ord, name)))
            t = make(rng, self.states[g][0], g)
            if t is None:
                continue
            w, u = t
            want = hits_of(self.states[0], w, u).astype(np.uint8) if g == 0 else first_hits(self.states, w, u, g)
            out.append((g, w, u, want))
        return out


def run_cone_case(hip, d, g, w, u):
    dw, du = to_dev(w[None]), to_dev(u[None])
    if g == 0:
        got = hip.contains(d, dw, du)
    else:
        got, _ = hip.step_contains(d, dw, du, g)
    torch.cuda.synchronize()
    return got.cpu().numpy()


# ---- A1: k_cone_adapt's later chunks ---------------------------------------

@pytest.fixture(scope="module")
def cone16(hip, port, lim):
    """2 x cap + 4099 universes: every wave of the 16-universe forms takes a
    second chunk, the first 4099 / 16 a third, the tail is ragged; on the
    device at both alignments"""
    b = ConeBatch(port, 2 * lim.cap(lim.kConeAdaptBlocksPerCU, 16) + 4099, seed=4100)
    b.dev = {16: to_dev(b.states[0]), 8: _off8(b.states[0])}
    yield b
    del b.dev
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name", list(CONE16_TARGETS))
def test_cone_adapt_later_chunks_16_universe_forms(hip, lim, cone16, name):
    """Contains and the 1-2 generation filter without final states on more
    than two passes of k_cone_adapt's capped grid (kConeAdaptBlocksPerCU): the
    loop-carried part of cone_wave_full_dma and cone_wave_rows_dma (PK = 4, 2,
    1 x WRAP; the vmcnt(1) wait behind a chunk's answer store, base(t) for
    t >= 2, the answers of one chunk after another in `mine`, the early
    prefetch handed in) on the 16-byte aligned batch, cone_wave_full16 for
    Contains, cone_wave<64,16>
    on the 8-byte aligned batch, and cone_wave<16|32|64,16> on column windows
    of 12, 24 (across column 63|0) and 40 columns of light cone.  Every answer
    against the oracle; its hits are 10-90 % and every wave's second chunk has
    both answers."""
    waves = lim.waves(lim.kConeAdaptBlocksPerCU)
    cases = cone16.cases(name, CONE16_TARGETS[name])
    assert len(cases) == 3
    for g, w, u, want in cases:
        assert_hit_share(want > 0, (name, g))
        assert_second_chunks_mixed(want > 0, waves, 16, (name, g))
        assert cone16.n > 2 * waves * 16  # a third chunk
        for align, d in cone16.dev.items():
            got = run_cone_case(hip, d, g, w, u)
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, (name, g, align, bad.size, bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.fixture(scope="module")
def cone64(hip, port, lim):
    return ConeBatch(port, lim.cap(lim.kConeAdaptBlocksPerCU, 64) + 4099, seed=6400)


@pytest.mark.parametrize("align", [16, 8])
def test_cone_adapt_second_chunk_64_universe_forms(hip, lim, cone64, align):
    """cone_wave<4,64> and cone_wave<8,64> (light cones of at most 4 and of 7
    columns, 64 universes per chunk) on one pass of the capped grid plus 4099
    universes: the first 65 waves take a second chunk, the last of them
    ragged; Contains and the 1-2 generation filter, one alignment per case
    (the batch is freed in between), every answer against the oracle"""
    waves = lim.waves(lim.kConeAdaptBlocksPerCU)
    d = to_dev(cone64.states[0]) if align == 16 else _off8(cone64.states[0])
    ran = 0
    for name, make in CONE64_TARGETS.items():
        for g, w, u, want in cone64.cases(name, make):
            assert_hit_share(want > 0, (name, g))
            assert_second_chunks_mixed(want > 0, waves, 64, (name, g))
            got = run_cone_case(hip, d, g, w, u)
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, (name, g, align, bad.size, bad[:8], got[bad[:8]], want[bad[:8]])
            ran += 1
    assert ran == 5  # (4 columns: 0 and 1 generations; 7 columns: 0, 1 and 2)
    del d
    torch.cuda.empty_cache()


# ---- A2: k_pop<kRedU>'s loop -----------------------------------------------

def test_pop_8_byte_fallback_second_chunk(hip, port, lim):
    """GetPop on a batch that is only 8-byte aligned (k_pop<kRedU> on at most
    kRedBlocksPerCU blocks per CU) of one pass of that grid plus 4099
    universes: the waves' second trip through the grid-stride loop, ragged;
    and the 16-byte form on the same batch.  Populations vary (an AND of two
    fills), so a misread universe shows."""
    n = lim.cap(lim.kRedBlocksPerCU, lim.kRedU) + 4099
    x = port.fill(n, seed=2100) & port.fill(n, seed=2101)
    want = port.pop(x)
    assert len(np.unique(want[-4099:])) > 50
    for d in (_off8(x), to_dev(x)):
        got = hip.pop(d).cpu().numpy().astype(np.uint32)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (d.data_ptr() % 16, bad.size, bad[:8])


# ---- A3: the iterated filter's loop ----------------------------------------

def filter_targets():
    """test_filter_on_8_byte_aligned_batches' three: block + ring, the one-row
    whole board, the full-height whole board"""
    bw, bu = np.zeros(64, np.uint64), np.zeros(64, np.uint64)
    bw[10] = bw[11] = np.uint64(3 << 40)
    bu[9:13] = np.uint64(15 << 39)
    bu &= ~bw
    ru = np.zeros(64, np.uint64)
    ru[0::3] = np.uint64(1 << 10)
    fu = np.zeros(64, np.uint64)
    for y in range(0, 64, 4):
        fu[(3 * y) % 64] |= np.uint64(1 << y)
    return {"block_ring": (bw, bu), "one_row": (ZERO, ru), "full_height": (ZERO, fu)}


def plant_blocks(x: np.ndarray) -> None:
    """Every 5th universe gets the block + ring target's block on an empty
    patch of 4 + 2 m columns and rows, m = 0, 2 or 9 by turns (m = 0 is
    test_step_contains_final_states_capped_grid's planting).  The soup
    reaches a ring m cells away after m generations at the earliest, so the
    two universes in 15 with m >= 2 hit at generations 1 and 2 whatever is
    around them (13 % of the batch), those with m = 0 only sometimes."""
    bw, _ = filter_targets()["block_ring"]
    for k, m in enumerate((0, 2, 9)):
        patch = np.zeros(64, np.uint64)
        patch[9 - m:13 + m] = rows_mask(39 - m, 4 + 2 * m)
        x[5 * k::15] = (x[5 * k::15] & ~patch) | bw


def filter_soup(port, n: int, gens: int):
    """An AND of three fills with plant_blocks' blocks, and the batch after 1
    .. gens generations.  The one-row and full-height targets (dead cells
    only) are hit by the soup itself: 39-61 % and 54-76 % of the universes
    within 3-8 generations, on the CPU."""
    x = port.fill(n, seed=3100) & port.fill(n, seed=3101) & port.fill(n, seed=3102)
    plant_blocks(x)
    states = [x]
    for _ in range(gens):
        states.append(port.step_batch(states[-1], 1, nthreads=THREADS))
    return states


@pytest.fixture(scope="module")
def filter_batch(hip, port, lim):
    n = 2 * lim.cap(lim.kFilterIterBlocksPerCU, 4) + 4099
    states = filter_soup(port, n, 8)
    dev = {16: to_dev(states[0]), 8: _off8(states[0])}
    yield n, states, dev
    dev.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("gens", [3, 7, 8])
def test_iterated_filter_later_chunks(hip, lim, filter_batch, gens):
    """The 3+ generation filter without final states (the merged split
    kernel on at most kFilterIterBlocksPerCU blocks per CU, 4 universes per
    wave and trip) on two passes of its grid plus 4099 universes: every wave
    loops twice, some three times, the tail ragged; at 3 generations and on
    both sides of kConeWholeWinGens (7: the whole board's row window in the
    LDS-DMA packed pass, 8: the window split layout); block + ring, one-row
    and full-height whole boards, both alignments, against the oracle.  The
    oracle's hits are 10-90 % of the batch and of the universes past the
    grid's first pass (a chunk of 4 universes is too few to hold both answers
    every time; every 64 consecutive ones must)."""
    n, states, dev = filter_batch
    assert gens in (3, lim.kConeWholeWinGens - 1, lim.kConeWholeWinGens)
    first_pass = lim.cap(lim.kFilterIterBlocksPerCU, 4)
    assert n > 2 * first_pass
    for name, (w, u) in filter_targets().items():
        want = first_hits(states, w, u, gens)
        assert_hit_share(want > 0, (name, gens))
        assert_hit_share(want[first_pass:] > 0, (name, gens, "later chunks"))
        assert_second_chunks_mixed(want > 0, first_pass // 64, 64, (name, gens))
        dw, du = to_dev(w[None]), to_dev(u[None])
        for align, d in dev.items():
            first, _ = hip.step_contains(d, dw, du, gens)
            got = first.cpu().numpy().astype(np.uint32)
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, (name, gens, align, bad.size, bad[:8], got[bad[:8]], want[bad[:8]])


# ---- A4: the LifeStable strip passes' loop ----------------------------------

@pytest.fixture(scope="module")
def strip_batch(hip, lim):
    """One pass of k_stable_strip's grid (kBlocksPerCu blocks per CU, a wave per
    object) plus 4097 objects, drawn from the recorded objects and starts: the
    first pass by seeded permutations of all 512, the later objects each a
    seeded, nonzero step away from the object its wave took first -- so no
    wave's second object is its first and no period of the batch meets the
    grid's.  (pick, first pass, starts, columns on the device, recorded planes
    and flags per pass)"""
    import test_stable_test_model as M
    starts, own_columns, want = M.own_strips()
    pool = len(starts)
    first_pass = lim.waves(source_constant("kBlocksPerCu"))
    rng = np.random.default_rng(8192)
    pick = np.concatenate([rng.permutation(pool) for _ in range(-(-first_pass // pool))])[:first_pass]
    pick = np.concatenate([pick, (pick[:4097] + rng.integers(1, pool, 4097)) % pool])
    columns = torch.from_numpy(own_columns[pick]).cuda()
    return pick, first_pass, starts, columns, want


@pytest.mark.parametrize("which", range(6))
def test_stable_strip_later_objects(hip, strip_batch, which):
    """The six strip passes on more objects than k_stable_strip's capped grid
    has waves (Grid{n, kBlocksPerCu}): 4097 waves take a second object, the
    others one.  Every object's planes and flags against the reference's
    recording; the second objects hold every flag the pass can give.
    (k_stable_test's loop is out of a test's reach: its grid is Grid{n}, one
    wave per object, and runs the loop again only where launch() has to cap it
    at 2^30 blocks.)"""
    from test_gpu_stable_test import Guarded
    pick, first_pass, starts, columns, want = strip_batch
    planes, flags = want[which]
    assert len(pick) == first_pass + 4097 and (pick[first_pass:] != pick[:4097]).all()
    later = set(flags[pick[first_pass:]].tolist())
    assert later == set(flags.tolist()) and later >= ({1, 3} if which == 1 else {0, 1, 3}), later
    g = Guarded(starts[pick])
    fl = hip.stable_strip_pass(g.out, columns, which)
    torch.cuda.synchronize()
    fl = fl.cpu().numpy()
    bad = np.nonzero(fl != flags[pick])[0]
    assert bad.size == 0, (which, bad.size, bad[:8])
    got = g.result()
    bad = np.nonzero((got != planes[pick]).any(axis=(1, 2)))[0]
    assert bad.size == 0, (which, bad.size, bad[:8])
    del g
    torch.cuda.empty_cache()


# ---- B: the order of every launch, asserted --------------------------------

class Book:
    """Reads the launch-order book without disturbing the batch's entry:
    order_probe(out, scratch) is True exactly when `out` is recorded as
    written forward, and records only `scratch` (an allocation of its own of
    the same extent, so that its entry overlaps no other batch)."""

    def __init__(self, tune, nbytes):
        self.tune, self.nbytes = tune, nbytes
        self.scratch = torch.empty(nbytes // 8, dtype=torch.int64, device="cuda")

    def note_forward(self, t):
        """`t` counts as written forward: the next launch that reads it reverses"""
        self.tune.order_note(t.data_ptr(), self.nbytes)

    def ran_reversed(self, out) -> bool:
        return not self.tune.order_probe(out.data_ptr(), self.scratch.data_ptr(), self.nbytes)


def weld_planes(port, n, seed):
    w = port.fill(n * 4, seed=seed).reshape(n, 256)
    w[:, 64:] &= port.fill(n * 3, seed=seed + 1).reshape(n, 192)
    return w


@pytest.mark.parametrize("gens", [1, 11])
@pytest.mark.parametrize("n", [1, 2, 3, 3003])
def test_weld_in_place_orders_alternate(hip, port, tune, n, gens):
    """k_weld<true, 2> (fewer than 12 generations; 11 is its last) four times
    in place on the same welds, the first call's input recorded as written
    forward: the launches run reversed (kWeldReverse: g0 = (groups - 1 - k) *
    2, the guarded odd weld first), forward, reversed, forward -- asserted
    through the book -- and each equals the oracle's LifeWeld::Step of the
    running state; n of one weld, one full group, an odd tail, many blocks."""
    cur = weld_planes(port, n, 7000 + 10 * n + gens)
    d = to_dev(cur).reshape(n, 256)
    book = Book(tune, n * 2048)
    book.note_forward(d)
    orders = []
    for call in range(4):
        hip.weld_step(d, gens)
        orders.append(book.ran_reversed(d))
        cur = port.weld_step(cur, gens)
        assert (to_host(d).reshape(n, 256) == cur).all(), (n, gens, call)
    assert orders == [True, False, True, False]


@pytest.mark.parametrize("gens", [0, 11, 12, 31, 32])
@pytest.mark.parametrize("n", [5, 3003])
def test_weld_generation_boundaries(hip, port, n, gens):
    """LifeWeld::Step `generations` times at the boundaries of the launch: 0
    (the welds unchanged), 11 (the last k_weld), 12 (the first k_weld_split),
    31 and 32 (its nontemporal and plain forms)"""
    w = weld_planes(port, n, 7100 + gens)
    d = to_dev(w).reshape(n, 256)
    hip.weld_step(d, gens)
    want = port.weld_step(w, gens)
    if gens == 0:
        assert (want == w).all()
    assert (to_host(d).reshape(n, 256) == want).all()


def planted_block_soup(port, n, seed):
    """an AND of two fills with plant_blocks' blocks, and the block + ring target"""
    x = port.fill(n, seed=seed) & port.fill(n, seed=seed + 1)
    plant_blocks(x)
    w, u = filter_targets()["block_ring"]
    return x, w, u


@pytest.mark.parametrize("gens", [1, 2])
@pytest.mark.parametrize("keyed", [True, False])
def test_filter_with_final_states_orders(hip, port, tune, lim, gens, keyed):
    """k_step_contains<8> with final states at 1-2 generations on
    kOrderMinUniverses + 5 universes (order-keyed, plain-stored tail; ragged
    against 8 per wave, so the reversed launch takes the ragged group first):
    four calls ping-pong and three in place (`final` is the input), the first
    input recorded as written forward, so the launches run reversed, forward,
    reversed, forward -- asserted -- with first hits and final states against
    the oracle after every call; and on kOrderMinUniverses - 3 universes,
    where every launch must run forward."""
    n = lim.kOrderMinUniverses + 5 if keyed else lim.kOrderMinUniverses - 3
    assert n <= lim.kFilterOrderUniverses and n % 8
    x, w, u = planted_block_soup(port, n, 8000 + gens)
    dw, du = to_dev(w[None]), to_dev(u[None])
    states, firsts = [x], []
    for _ in range(4):
        chain = [states[-1]]
        for _ in range(gens):
            chain.append(port.step_batch(chain[-1], 1, nthreads=THREADS))
        firsts.append(first_hits(chain, w, u, gens))
        states.append(chain[-1])
    assert_hit_share(firsts[0] > 0, "the first call")  # (plant_blocks: 2 universes in 15 at the least)
    assert all((f > 0).sum() > n // 100 for f in firsts)  # the blocks on the widest patch last all four calls
    book = Book(tune, n * 512)
    expect = [True, False, True, False] if keyed else [False] * 4
    a, b = to_dev(x), torch.zeros((n, 64), dtype=torch.int64, device="cuda")
    book.note_forward(a)
    orders = []
    for call in range(4):
        first, _ = hip.step_contains(a, dw, du, gens, final=b)
        orders.append(book.ran_reversed(b))
        assert (first.cpu().numpy().astype(np.uint32) == firsts[call]).all(), ("ping-pong first", call)
        assert (to_host(b) == states[call + 1]).all(), ("ping-pong final", call)
        a, b = b, a
    assert orders == expect
    del a, b
    d = to_dev(x)
    book.note_forward(d)
    orders = []
    for call in range(3):
        first, _ = hip.step_contains(d, dw, du, gens, final=d)
        orders.append(book.ran_reversed(d))
        assert (first.cpu().numpy().astype(np.uint32) == firsts[call]).all(), ("in place first", call)
        assert (to_host(d) == states[call + 1]).all(), ("in place final", call)
    assert orders == expect[:3]


@pytest.mark.parametrize("keyed", [True, False])
def test_step_orders_at_the_order_threshold(hip, port, tune, lim, keyed):
    """k_step at 1 generation on kOrderMinUniverses + 1 universes (the
    smallest order-keyed batch, ragged against 4 per wave): four launches
    ping-pong and two in place run reversed, forward, reversed, forward after
    an input recorded as written forward -- asserted -- and on
    kOrderMinUniverses - 1 every launch runs forward; every result against the
    oracle"""
    n = lim.kOrderMinUniverses + 1 if keyed else lim.kOrderMinUniverses - 1
    x = port.fill(n, seed=9000 + n % 7)
    want = [x]
    for _ in range(4):
        want.append(port.step_batch(want[-1], 1, nthreads=THREADS))
    book = Book(tune, n * 512)
    expect = [True, False, True, False] if keyed else [False] * 4
    a, b = to_dev(x), torch.zeros((n, 64), dtype=torch.int64, device="cuda")
    book.note_forward(a)
    orders = []
    for k in range(1, 5):
        hip.step(a, out=b, generations=1)
        orders.append(book.ran_reversed(b))
        assert (to_host(b) == want[k]).all(), ("ping-pong", k)
        a, b = b, a
    assert orders == expect
    del a, b
    d = to_dev(x)
    book.note_forward(d)
    orders = []
    for k in range(1, 3):
        hip.step(d, out=d, generations=1)
        orders.append(book.ran_reversed(d))
        assert (to_host(d) == want[k]).all(), ("in place", k)
    assert orders == expect[:2]


# ---- C: a stream of the caller's own ---------------------------------------

def side_stream_oracle(port):
    """the inputs and the oracle's results of the side-stream chain below"""
    from types import SimpleNamespace

    from test_gpu_rle import moved32
    n, big, period, pgens = 4099, 16384, 509, 2000
    base = port.fill(period, seed=5001) & port.fill(period, seed=5002)
    x0 = base[np.arange(big) % period]
    want_a = port.step_batch(base, pgens, nthreads=THREADS)[np.arange(big) % period]
    want_b = port.step_batch(want_a[:n], 1, nthreads=THREADS)
    chain = [want_b, port.step_batch(want_b, 1, nthreads=THREADS)]
    chain.append(port.step_batch(chain[-1], 1, nthreads=THREADS))
    want_c = chain[2]
    alive = np.zeros((64, 64), np.int64)   # [column, row]: universes of want_c alive there
    for r in range(64):
        alive[:, r] = ((want_c >> np.uint64(r)) & np.uint64(1)).sum(axis=0)
    col, row = np.unravel_index(np.argmax(alive), alive.shape)
    w, u = np.zeros(64, np.uint64), np.zeros(64, np.uint64)
    w[col] = np.uint64(1 << int(row))           # the cell most often alive, and a dead neighbour
    u[(col + 1) % 64] = np.uint64(1 << int(row))
    want_first2 = first_hits(chain, w, u, 2)
    want_first1 = first_hits([want_c, port.step_batch(want_c, 1, nthreads=THREADS)], w, u, 1)
    want_hit = hits_of(want_c, w, u)
    assert 0 < want_hit.sum() < n and want_first1.any() and want_first2.any()
    want_pop, want_hash = port.pop(want_c), port.hashes(want_c)
    want_nc = np.stack([port.neighbour_count(s) for s in want_c])
    want_ic = np.stack([port.interaction_counts(s) for s in want_c])
    want_weld = port.weld_step(want_ic.reshape(n, 256), 3)
    m = n * 256 // 640
    want_st, want_fl = port.stable_pass(want_weld.reshape(-1)[:m * 640].reshape(m, 640), 0)
    want_vul = port.stable_vulnerable(want_st)
    k = m // 11
    want_ref = port.refined_step(want_vul.reshape(-1)[:k * 704].reshape(k, 704))
    texts = [port.rle(s) for s in want_c[:300]]
    want_parsed = moved32(want_c[:300])
    want_rle = [port.rle(p) for p in want_parsed]
    return SimpleNamespace(**{k_: v for k_, v in locals().items() if k_ not in ("port", "SimpleNamespace")})


def test_every_dev_entry_point_on_a_side_stream(hip, port):
    """Every *_dev entry point enqueued on a torch side stream `s`, the
    default stream idle, no synchronisation in between: first a long producer
    (Step of 16384 universes x 2000 generations into `a`), then a chain in
    which every call reads what the call before it wrote on `s` -- step,
    step_contains with and without final states, contains, pop, hashes,
    neighbour_count, interaction_counts, weld_step, a LifeStable pass,
    stable_vulnerable, refined_step, parse_rle (its text copied device to
    device on `s`) and rle (under torch.cuda.stream(s)).  All buffers are
    zeroed beforehand, so a call enqueued on another stream runs ahead of the
    producer on zeros and fails its comparison with the oracle.  The
    producer's universes repeat with period 509, which keeps the oracle's 2000
    generations to a second."""
    from test_gpu_rle import blob_dev
    o = side_stream_oracle(port)
    n, m, k = o.n, o.m, o.k

    dev = lambda *shape: torch.zeros(shape, dtype=torch.int64, device="cuda")  # noqa: E731
    din, a, b, c = to_dev(o.x0), dev(o.big, 64), dev(n, 64), dev(n, 64)
    dw, du = to_dev(o.w[None]), to_dev(o.u[None])
    welds, st, refin = dev(n, 256), dev(m, 640), dev(k, 704)
    text_src, offs = blob_dev(o.texts)
    text = torch.zeros_like(text_src)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()

    hip.step(din, out=a, generations=o.pgens, stream=s)
    hip.step(a[:n], out=b, generations=1, stream=s)
    first2, _ = hip.step_contains(b, dw, du, 2, final=c, stream=s)
    first1, _ = hip.step_contains(c, dw, du, 1, stream=s)
    hit = hip.contains(c, dw, du, stream=s)
    pop = hip.pop(c, stream=s)
    hsh = hip.hashes(c, stream=s)
    nc = hip.neighbour_count(c, stream=s)
    ic = hip.interaction_counts(c, with_next=True, stream=s)
    with torch.cuda.stream(s):  # (the copies between the calls' buffers run on `s` too)
        welds.copy_(ic.view(n, 256))
    hip.weld_step(welds, 3, stream=s)
    with torch.cuda.stream(s):
        st.copy_(welds.view(-1)[:m * 640].view(m, 640))
    flags = hip.stable_pass(st, "sync", stream=s)
    vul = hip.stable_vulnerable(st, stream=s)
    with torch.cuda.stream(s):
        refin.copy_(vul.view(-1)[:k * 704].view(k, 704))
        text.copy_(text_src)
    ref = hip.refined_step(refin, stream=s)
    parsed, status = hip.parse_rle(text, offs, stream=s)
    with torch.cuda.stream(s):
        rle_text, rle_offs = hip.rle(parsed)
    s.synchronize()
    torch.cuda.synchronize()

    u64 = lambda t: t.cpu().numpy().view(np.uint64)  # noqa: E731
    assert (to_host(a) == o.want_a).all(), "producer"
    assert (to_host(b) == o.want_b).all(), "step"
    assert (to_host(c) == o.want_c).all(), "step_contains final states"
    assert (first2.cpu().numpy().astype(np.uint32) == o.want_first2).all(), "step_contains with final states"
    assert (first1.cpu().numpy().astype(np.uint32) == o.want_first1).all(), "step_contains"
    assert (hit.cpu().numpy().astype(bool) == o.want_hit).all(), "contains"
    assert (pop.cpu().numpy().astype(np.uint32) == o.want_pop).all(), "pop"
    assert (u64(hsh) == o.want_hash).all(), "hashes"
    assert (u64(nc) == o.want_nc).all(), "neighbour_count"
    assert (u64(ic) == o.want_ic).all(), "interaction_counts"
    assert (u64(welds) == o.want_weld).all(), "weld_step"
    assert (u64(st) == o.want_st).all() and (flags.cpu().numpy() == o.want_fl).all(), "stable_pass"
    assert (to_host(vul) == o.want_vul).all(), "stable_vulnerable"
    assert (u64(ref) == o.want_ref).all(), "refined_step"
    assert not status.any().item() and (to_host(parsed) == o.want_parsed).all(), "parse_rle"
    offs_h, t = rle_offs.cpu().numpy(), rle_text.cpu().numpy().tobytes()
    assert [t[offs_h[i]:offs_h[i + 1]].decode() for i in range(len(o.texts))] == o.want_rle, "rle"
