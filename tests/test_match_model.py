"""CPU: the definitions of Match, Convolve and InteractionOffsets that the GPU
tests of tests/test_gpu_match.py compare against, restated in vectorised numpy
and pinned here to the reference's own outputs (tests/golden/match.npz,
recorded by tests/golden/make_match_golden.py from LifeState::Match(const
LifeTarget&), Convolve and InteractionOffsets; LifeTarget.hpp:53-55,
LifeAPI.hpp:432-435, 1066-1095, 1293-1370).

With s(x, y) = bit y of column x and every index mod 64:
  Convolve(A, B)(x, y) = OR over (a, b) in B of A(x - a, y - b)
  Match(w, u)(x, y)    = every (a, b) in w has s(x + a, y + b) = 1 and every
                         (a, b) in u has s(x + a, y + b) = 0
  Mirrored(): (x, y) -> (-x, -y)
InteractionOffsets has no definition but the reference's formula, restated
below on count planes.

Also here: the builders of the fixture's inputs (the generator and the tests
share them) and the entry points' argument checks, which need no device."""
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "match.npz")
U1 = np.uint64(1)
ALL = np.uint64(2**64 - 1)
ROWS = np.arange(64, dtype=np.uint64)


# ---- the definitions ------------------------------------------------------

def cells(p):
    """(a, b) of every live cell of a pattern of 64 column words"""
    return [(a, b) for a in range(64) for b in range(64) if (int(p[a]) >> b) & 1]


def rotl(v, b):
    b &= 63
    return v if b == 0 else (v << np.uint64(b)) | (v >> np.uint64(64 - b))


def np_convolve(states, pattern):
    out = np.zeros_like(states)
    for a, b in cells(pattern):
        out |= rotl(np.roll(states, a, axis=-1), b)        # column x - a, row y - b
    return out


def np_match(states, wanted, unwanted):
    ok = np.full_like(states, ALL)
    for a, b in cells(wanted):
        ok &= rotl(np.roll(states, -a, axis=-1), -b)       # column x + a, row y + b
    for a, b in cells(unwanted):
        ok &= ~rotl(np.roll(states, -a, axis=-1), -b)
    return ok


def unpack(a):
    """(..., 64) words -> (..., 64 columns, 64 rows) bool"""
    return ((a[..., None] >> ROWS) & U1).astype(bool)


def pack(b):
    return np.bitwise_or.reduce(b.astype(np.uint64) << ROWS, axis=-1)


def np_mirrored(p):
    return pack(np.roll(unpack(p)[..., ::-1, ::-1], (1, 1), axis=(-2, -1)))


def _interaction_planes(s):
    """the seven planes of one side (LifeAPI.hpp:1067-1093), packed"""
    live = unpack(s)
    count = sum(np.roll(live, (dx, dy), axis=(-2, -1)).astype(np.int8) for dx in (-1, 0, 1) for dy in (-1, 0, 1))
    dead = ~live
    return [pack(p) for p in (live, (count == 1) & dead, (count == 2) & dead, (count == 3) & live,
                              (count >= 4) & live, (count >= 2) & dead, (count >= 1) & dead)]


PARTNER = (0, 2, 1, 5, 6, 3, 4)  # plane i of one side is convolved with plane PARTNER[i] of the other


def np_interaction_offsets(states, other):
    a, b = _interaction_planes(states), _interaction_planes(np_mirrored(other))
    out = np.zeros_like(states)
    for i in range(7):
        out |= np_convolve(a[i], b[PARTNER[i]])
    return out


def popcount(a):
    return unpack(a).sum(axis=(-2, -1)).astype(np.uint32)


# ---- the fixture's inputs ---------------------------------------------------

def at(pattern, x, y):
    """pattern moved by (x, y) on the torus"""
    return rotl(np.roll(pattern, x), y)


def boundary(p):
    """GetBoundary (LifeAPI.hpp:521-538): the 3x3 dilation minus the pattern"""
    return np_convolve(p, _cells_to_pattern([(i, j) for i in (-1, 0, 1) for j in (-1, 0, 1)])) & ~p


def seam_cases(port):
    """tests/test_gpu_parity.py::seam_cases, rebuilt"""
    out = []
    s = np.zeros(64, np.uint64)
    s[0] = s[63] = s[1] = np.uint64(0x8000000000000003)
    out.append(s.copy())
    s = np.zeros(64, np.uint64)
    s[62] = s[63] = s[0] = np.uint64((1 << 63) | 1)
    out.append(s.copy())
    out.append(np.full(64, ALL))
    out.append(np.array([0xAAAAAAAAAAAAAAAA if x % 2 == 0 else 0x5555555555555555 for x in range(64)], np.uint64))
    g = port.parse("bo$2bo$3o!")
    out.append(np.roll(g, 62))
    out.append(np.array([(int(w) << 62 | int(w) >> 2) & (2**64 - 1) for w in g], np.uint64))
    out.append(np.zeros(64, np.uint64))
    return np.stack(out)


def special_states(port):
    chk = np.array([0xAAAAAAAAAAAAAAAA if x % 2 == 0 else 0x5555555555555555 for x in range(64)], np.uint64)
    return np.concatenate([np.stack([np.zeros(64, np.uint64), np.full(64, ALL), chk]), seam_cases(port)])


N_SPECIAL, N_RANDOM = 10, 16


def all_states(port, special):
    """the special states, then 16 seeded random states at full and 16 at
    quarter density (regenerated, not stored)"""
    full = port.fill(N_RANDOM, seed=1101)
    quarter = port.fill(N_RANDOM, seed=1102) & port.fill(N_RANDOM, seed=1103)
    return np.concatenate([special, full, quarter])


def _cells_to_pattern(cs):
    p = np.zeros(64, np.uint64)
    for a, b in cs:
        p[a % 64] |= U1 << np.uint64(b % 64)
    return p


def block_ring(x=20, y=30):
    blk = _cells_to_pattern([(x + i, y + j) for i in (0, 1) for j in (0, 1)])
    return blk, boundary(blk)


def care8(seed, x0, y0):
    """3 live + 5 dead care cells inside the 5 x 5 window at (x0, y0)"""
    rng = np.random.default_rng(seed)
    pick = rng.permutation(25)[:8]
    cs = [(x0 + int(k) // 5, y0 + int(k) % 5) for k in pick]
    return _cells_to_pattern(cs[:3]), _cells_to_pattern(cs[3:])


def build_targets(port, states):
    """name -> (wanted, unwanted)"""
    z = np.zeros(64, np.uint64)
    rng = np.random.default_rng(77)
    glider = port.parse("bo$2bo$3o!")
    t = {}
    t["empty"] = (z, z)
    t["wanted_empty"] = (z, _cells_to_pattern([(3, 4), (5, 9)]))
    t["unwanted_empty"] = (_cells_to_pattern([(3, 4), (4, 4), (60, 1)]), z)
    t["cell_0_0"] = (_cells_to_pattern([(0, 0)]), z)
    t["cell_63_63"] = (_cells_to_pattern([(63, 63)]), z)
    t["dead_cell_63_63"] = (z, _cells_to_pattern([(63, 63)]))
    t["block_ring"] = block_ring()
    g = at(glider, 62, 62)  # columns 62..0, rows 62..0
    t["glider_seams"] = (g, boundary(g))
    col = z.copy()
    col[17] = ALL
    t["full_column"] = (col, z)                       # a column equal to ~0 (LifeAPI.hpp:1304)
    t["full_column_dead"] = (z, col)
    t["full_row"] = (np.full(64, U1 << np.uint64(41)), z)
    t["full_row_dead"] = (z, np.full(64, U1 << np.uint64(41)))
    bits = rng.integers(0, 2, size=(5, 5))
    w5 = _cells_to_pattern([(30 + i, 12 + j) for i in range(5) for j in range(5) if bits[i, j]])
    u5 = _cells_to_pattern([(30 + i, 12 + j) for i in range(5) for j in range(5) if not bits[i, j]])
    t["random_5x5"] = (w5, u5)
    # random care cells over the whole board, taken from a recorded state so
    # that it matches somewhere: the first full-density state, at offset (3, 5)
    care = port.fill(1, seed=1201)[0] & port.fill(1, seed=1202)[0] & port.fill(1, seed=1203)[0]
    s = states[N_SPECIAL]
    t["random_care_board"] = (at(s & care, -3, -5), at(~s & care, -3, -5))
    run = z.copy()
    run[9] = np.uint64((1 << 40) - 1) << np.uint64(10)  # 40 rows: longer than the reference's min(runlength, 32)
    t["run_40_rows"] = (run, z)
    run_wrap = z.copy()
    run_wrap[9] = rotl(np.uint64((1 << 40) - 1), 50)
    t["run_40_rows_wrapped_dead"] = (z, run_wrap)
    t["care8"] = care8(5, 40, 20)
    t["care8_seams"] = care8(6, 62, 62)               # the window crosses both seams
    t["care8_b"] = care8(7, 10, 50)
    return t


def build_patterns(port):
    z = np.zeros(64, np.uint64)
    rng = np.random.default_rng(78)
    p = {}
    p["empty"] = z
    p["cell_0_0"] = _cells_to_pattern([(0, 0)])
    p["cell_63_63"] = _cells_to_pattern([(63, 63)])
    p["3x3"] = _cells_to_pattern([(i, j) for i in (-1, 0, 1) for j in (-1, 0, 1)])  # ZOI's pattern
    p["glider_seams"] = at(port.parse("bo$2bo$3o!"), 62, 62)
    col = z.copy()
    col[17] = ALL
    p["full_column"] = col
    p["full_row"] = np.full(64, U1 << np.uint64(41))
    run = z.copy()
    run[9] = np.uint64((1 << 40) - 1) << np.uint64(10)
    run[10] = rotl(np.uint64((1 << 40) - 1), 50)
    run[11] = np.uint64(0xF0F0FF0000000F01)
    p["runs"] = run
    bits = rng.integers(0, 2, size=(5, 5))
    p["random_5x5"] = _cells_to_pattern([(30 + i, 12 + j) for i in range(5) for j in range(5) if bits[i, j]])
    p["random_sparse_board"] = port.fill(1, seed=1301)[0] & port.fill(1, seed=1302)[0] & port.fill(1, seed=1303)[0] \
        & port.fill(1, seed=1304)[0] & port.fill(1, seed=1305)[0] & port.fill(1, seed=1306)[0]
    p["7x7"] = _cells_to_pattern([(i, j) for i in range(7) for j in range(7)])
    return p


def build_others(port):
    o = {}
    o["empty"] = np.zeros(64, np.uint64)
    o["cell"] = _cells_to_pattern([(5, 7)])
    o["block"] = port.parse("2o$2o!")
    o["glider"] = port.parse("bo$2bo$3o!")
    o["eater"] = at(port.parse("2o$obo$2bo$2b2o!"), 30, 30)
    o["eater_seams"] = at(port.parse("2o$obo$2bo$2b2o!"), 62, 62)
    return o


_cache = {}


def fixture_data(port):
    """the recorded arrays, the full state list and the inputs by name"""
    if not _cache:
        z = np.load(FIXTURE)
        d = {k: z[k] for k in z.files}
        d["states"] = all_states(port, d["special_states"])
        for a in d.values():
            a.flags.writeable = False
        _cache.update(d)
    return _cache


# ---- tests ------------------------------------------------------------------

def test_builders_give_the_recorded_inputs(port):
    d = fixture_data(port)
    assert (special_states(port) == d["special_states"]).all()
    for key, built in (("target", build_targets(port, d["states"])), ("pattern", build_patterns(port)),
                       ("other", build_others(port))):
        assert list(built) == list(d[key + "_names"])
        assert (np.stack([np.stack(v) if isinstance(v, tuple) else v for v in built.values()]) == d[key + "s"]).all()


def test_boundary_is_get_boundary(port):
    """the builders' boundary() is GetBoundary (LifeAPI.hpp:521-538): ZOI minus the pattern"""
    blk, ring = block_ring(20, 30)
    want = np.zeros(64, np.uint64)
    for c in (19, 20, 21, 22):
        want[c] = np.uint64(0b1111 << 29)
    assert (ring == want & ~blk).all()


def test_numpy_match_equals_the_reference(port):
    d = fixture_data(port)
    for k, name in enumerate(d["target_names"]):
        w, u = d["targets"][k]
        assert (np_match(d["states"], w, u) == d["match"][k]).all(), name


def test_numpy_convolve_equals_the_reference(port):
    d = fixture_data(port)
    for k, name in enumerate(d["pattern_names"]):
        assert (np_convolve(d["states"], d["patterns"][k]) == d["convolve"][k]).all(), name


def test_numpy_interaction_offsets_equals_the_reference(port):
    d = fixture_data(port)
    for k, name in enumerate(d["other_names"]):
        assert (np_interaction_offsets(d["states"], d["others"][k]) == d["interaction"][k]).all(), name


def test_recorded_matches_are_not_vacuous(port):
    """what the generator asserted when it recorded the fixture"""
    d = fixture_data(port)
    assert nonvacuity(d["states"], d["targets"], d["match"]) == (True, True, True)


def nonvacuity(states, targets, match):
    """on the reference's outputs alone: >= 8 (state, target) pairs whose mask
    is neither empty nor full, >= 3 of them with a match whose care cells
    occupy columns 63 and 0, >= 3 with one whose care cells occupy rows 63
    and 0"""
    mixed = colx = rowx = 0
    for k in range(len(targets)):
        care = cells(targets[k][0] | targets[k][1])
        if not care:
            continue
        ca, cb = np.array([a for a, _ in care]), np.array([b for _, b in care])
        for i in range(len(states)):
            m = match[k][i]
            if not m.any() or (m == ALL).all():
                continue
            mixed += 1
            hits = np.argwhere(unpack(m))
            cols = (hits[:, :1] + ca[None, :]) & 63
            rows = (hits[:, 1:] + cb[None, :]) & 63
            colx += bool((((cols == 63).any(axis=1)) & ((cols == 0).any(axis=1))).any())
            rowx += bool((((rows == 63).any(axis=1)) & ((rows == 0).any(axis=1))).any())
    return mixed >= 8, colx >= 3, rowx >= 3


def test_argument_validation_without_device():
    import lifeapi_amd.hip as hip
    L = hip.lib
    S, W, U_, O, C = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20  # disjoint, aligned, never dereferenced
    n = 4
    # both outputs NULL
    assert L.lifeapi_match_batch_dev(S, W, U_, None, None, n, None) == -1
    assert b"null" in L.lifeapi_last_error()
    # null inputs
    assert L.lifeapi_match_batch_dev(None, W, U_, O, None, n, None) == -1
    assert L.lifeapi_match_batch_dev(S, None, U_, O, None, n, None) == -1
    assert L.lifeapi_match_batch_dev(S, W, None, None, C, n, None) == -1
    assert L.lifeapi_convolve_batch_dev(S, None, O, n, None) == -1
    assert L.lifeapi_convolve_batch_dev(S, W, None, n, None) == -1
    assert L.lifeapi_interaction_offsets_batch_dev(None, W, O, n, None) == -1
    # misaligned
    assert L.lifeapi_match_batch_dev(S + 4, W, U_, O, None, n, None) == -1
    assert L.lifeapi_match_batch_dev(S, W + 4, U_, O, None, n, None) == -1
    assert L.lifeapi_match_batch_dev(S, W, U_, O + 4, None, n, None) == -1
    assert L.lifeapi_match_batch_dev(S, W, U_, None, C + 2, n, None) == -1
    assert L.lifeapi_convolve_batch_dev(S, W + 4, O, n, None) == -1
    assert L.lifeapi_interaction_offsets_batch_dev(S, W, O + 4, n, None) == -1
    # partial overlap (in == out is the one overlap allowed)
    assert L.lifeapi_match_batch_dev(S, W, U_, S + 512, None, n, None) == -1
    assert b"overlap" in L.lifeapi_last_error()
    assert L.lifeapi_match_batch_dev(S, O + 512, U_, O, None, n, None) == -1   # the target inside the output
    assert L.lifeapi_match_batch_dev(S, W, U_, O, O + 8, n, None) == -1        # the counts inside the output
    assert L.lifeapi_match_batch_dev(S, W, U_, None, S + 8, n, None) == -1     # the counts inside the input
    assert L.lifeapi_convolve_batch_dev(S, W, S + 512, n, None) == -1
    assert L.lifeapi_convolve_batch_dev(S, S + 512, S, n, None) == -1
    assert L.lifeapi_interaction_offsets_batch_dev(S, W, S - 512, n, None) == -1
    # n == 0 is a no-op success even with null pointers
    assert L.lifeapi_match_batch_dev(None, None, None, None, None, 0, None) == 0
    assert L.lifeapi_convolve_batch_dev(None, None, None, 0, None) == 0
    assert L.lifeapi_interaction_offsets_batch_dev(None, None, None, 0, None) == 0
    assert L.lifeapi_match_batch(None, None, None, None, None, 0, 0) == 0
    assert L.lifeapi_convolve_batch(None, None, None, 0, 0) == 0
    assert L.lifeapi_interaction_offsets_batch(None, None, None, 0, 0) == 0
    # the host forms check before they look for a device
    x = np.zeros((n, 64), np.uint64)
    p = x.ctypes.data
    assert L.lifeapi_match_batch(p, p, p, None, None, n, 0) == -1
    assert L.lifeapi_match_batch(p, p, p, p + 512, None, n, 0) == -1
    assert L.lifeapi_convolve_batch(p, None, p, n, 0) == -1
    assert L.lifeapi_interaction_offsets_batch(p + 4, p, p, n, 0) == -1
