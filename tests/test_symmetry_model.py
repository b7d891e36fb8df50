"""CPU: numpy definitions of the reference's symmetry layer -- Transform then
Move (Symmetry.hpp:105-173, LifeAPI.hpp:682-735), Symmetricize (Symmetry.hpp:
565-654), XYBounds (LifeAPI.hpp:446-484) and SymmetryOrbit[Representatives]
(Symmetry.hpp:798-830) -- pinned to every array of tests/golden/symmetry.npz,
which tests/golden/make_symmetry_golden.py recorded from the reference itself.

The model moves cells one by one through an affine map of the torus,
(x, y) -> A (x, y) + b: nothing in it resembles the kernels' lane and bit
permutations.  The table of maps is not taken on trust: the test derives each
transform's A and b from the recorded images of single cells.  Every mutation
listed at the end must contradict a recorded answer.

tests/golden/symmetry_sweeps.npz (make_symmetry_golden.py --only-sweeps) holds
the reference's answers on the sweeps built below: every residue of a shift
for every transform, every symmetry along two lines of 141 offsets, the
bounds and orbit masks of every pair of populated columns and of rows, a
state for every stabiliser subgroup of D4, and two states whose images
differ in one 32-row half only.

The GPU tests (tests/test_gpu_symmetry.py) and the generator import the
models and the inputs from here.
"""
import itertools
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "symmetry.npz")

TRANSFORMS = ("Identity", "ReflectAcrossXEven", "ReflectAcrossX", "ReflectAcrossYEven", "ReflectAcrossY",
              "Rotate90Even", "Rotate90", "Rotate270Even", "Rotate270", "Rotate180OddBoth",
              "Rotate180EvenHorizontal", "Rotate180EvenVertical", "Rotate180EvenBoth", "ReflectAcrossYeqX",
              "ReflectAcrossYeqNegX", "ReflectAcrossYeqNegXP1")
T = {name: k for k, name in enumerate(TRANSFORMS)}
# StaticSymmetry values (Symmetry.hpp:57-79) that Symmetricize defines
SYMMETRIES = {"C1": 0, "D2AcrossX": 1, "D2AcrossY": 3, "D2negdiagodd": 5, "D2diagodd": 6, "C2": 7, "C4": 11,
              "D4": 13, "D4diag": 17}
UNDEFINED_SYMMETRIES = (2, 4, 8, 9, 10, 12, 14, 15, 16, 18, 19, 20, 21)
# SymmetryOrbit's transforms in its order (Symmetry.hpp:801-803)
ORBIT_ORDER = (T["Identity"], T["ReflectAcrossX"], T["ReflectAcrossYeqX"], T["ReflectAcrossY"],
               T["ReflectAcrossYeqNegXP1"], T["Rotate90"], T["Rotate270"], T["Rotate180OddBoth"])

# ---- the recorded inputs ----
CELLS = ((0, 0), (63, 0), (0, 63), (63, 63), (31, 32), (17, 42))
MOVES = ((1, 0), (0, 1), (-1, -1), (31, 33), (32, 32), (64, -64), (65, -65), (1000, -999))
OFFSETS = ((0, 0), (7, -3), (-3, 7), (40, 50), (-40, 13), (5, 6))
ORBIT_MOVES = ((0, 0), (-2, -1), (30, 31), (40, 50))
PATTERNS = {"empty": None, "cell": "o!", "block": "2o$2o!", "row3": "3o!", "L3": "2o$o!", "T4": "3o$bo!",
            "S6": "2o$bo$bo$b2o!", "L4": "3o$o!", "R5": "b2o$2o$bo!", "glider": "bo$2bo$3o!"}
N_RANDOM = 8


# ---- bits <-> cells: g[x, y] = bit y of word x ----
def unpack(state):
    s = np.asarray(state, np.uint64).reshape(64)
    return ((s[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)


def pack(g):
    return (g.astype(np.uint64) << np.arange(64, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)


def cell(x, y):
    s = np.zeros(64, np.uint64)
    s[x] = np.uint64(1) << np.uint64(y)
    return s


# ---- the affine maps.  A map is (swap, sx, sy, bx, by): (x, y) -> (sx x + bx, sy y + by), or with swap
# (sx y + bx, sy x + by).  The primitives as the reference comments them (LifeAPI.hpp:754-764) ----
IDENTITY = (False, 1, 1, 0, 0)
FLIP_X = (False, 1, -1, 0, -1)       # BitReverse: row y -> 63 - y
FLIP_Y = (False, -1, 1, -1, 0)       # Reverse: column x -> 63 - x
TRANSPOSE = {False: (True, 1, 1, 0, 0), True: (True, -1, -1, -1, -1)}


def then(f, g):
    """the map: f first, then g"""
    fs, fx, fy, fbx, fby = f
    gs, gx, gy, gbx, gby = g
    if not gs:
        return (fs, gx * fx, gy * fy, gx * fbx + gbx, gy * fby + gby)
    return (not fs, gx * fy, gy * fx, gx * fby + gbx, gy * fbx + gby)


def move(dx, dy):
    return (False, 1, 1, dx, dy)


def build_table(transpose=TRANSPOSE, plus=1):
    """the 16 maps from Transform's switch (Symmetry.hpp:105-173); the
    arguments are what the mutations change"""
    fx, fy, tr, m = FLIP_X, FLIP_Y, transpose, lambda a, b: move(plus * a, plus * b)
    both = then(fx, fy)
    return (IDENTITY, fx, then(fx, m(0, 1)), fy, then(fy, m(1, 0)),
            then(fx, tr[False]), then(then(fx, tr[False]), m(1, 0)),
            then(fy, tr[False]), then(then(fy, tr[False]), m(0, 1)),
            then(both, m(1, 1)), then(both, m(0, 1)), then(both, m(1, 0)), both,
            tr[False], tr[True], then(tr[True], m(1, 1)))


TABLE = build_table()


def apply_map(state, f):
    swap, sx, sy, bx, by = f
    g = unpack(state)
    x, y = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
    u, v = (y, x) if swap else (x, y)
    out = np.zeros_like(g)
    out[(sx * u + bx) % 64, (sy * v + by) % 64] = g[x, y]
    return pack(out)


def np_transform(state, t, dx=0, dy=0, table=TABLE, move_first=False):
    """state.Transformed(t).Moved(dx, dy)"""
    f = then(move(dx, dy), table[t]) if move_first else then(table[t], move(dx, dy))
    return apply_map(state, f)


def np_transform_batch(states, t, dx=0, dy=0):
    """the same for (n, 64) states at once, read backwards: the cell that lands on (X, Y)"""
    swap, sx, sy, bx, by = then(TABLE[t], move(dx, dy))
    s = np.ascontiguousarray(states, np.uint64).reshape(-1, 64)
    g = np.unpackbits(s.view(np.uint8).reshape(-1, 64, 8), axis=2, bitorder="little").reshape(-1, 64, 64)
    k = np.arange(64)
    fx, fy = (sx * (k - bx)) % 64, (sy * (k - by)) % 64   # X -> x (or y with swap), Y -> y (or x)
    out = g.take(fy, axis=1).take(fx, axis=2).transpose(0, 2, 1) if swap else g.take(fx, axis=1).take(fy, axis=2)
    return np.packbits(np.ascontiguousarray(out).reshape(-1), bitorder="little").view(np.uint64).reshape(-1, 64)


# ---- Symmetricize ----
def c_div(a, b):  # C++'s truncating division and remainder
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def c_mod(a, b):
    return a - b * c_div(a, b)


def perp_trunc(kind, ox, oy):
    """PerpComponent (Symmetry.hpp:540-563) in C++'s int arithmetic"""
    x, y = c_mod(ox + 32, 64) - 32, c_mod(oy + 32, 64) - 32
    if kind == "YeqX":
        return c_mod(c_div(x - y + 128, 2), 64), c_mod(c_div(-x + y + 128, 2), 64)
    return (c_mod(c_div(x + y + 128, 2), 64),) * 2


def perp_floor(kind, ox, oy):  # mutation: Python's floor division and modulo throughout
    x, y = (ox + 32) % 64 - 32, (oy + 32) % 64 - 32
    if kind == "YeqX":
        return ((x - y + 128) // 2) % 64, ((-x + y + 128) // 2) % 64
    return (((x + y + 128) // 2) % 64,) * 2


def perp_mod64(kind, ox, oy):  # mutation: the offset reduced mod 64 first
    return perp_trunc(kind, ox % 64, oy % 64)


def np_symmetricize(state, sym, dx, dy, perp=perp_trunc, table=TABLE):
    s = np.asarray(state, np.uint64)
    if s.ndim == 2:   # a batch: the vectorised transform
        tf = np_transform_batch
    else:
        tf = lambda a, t, x, y: np_transform(a, t, x, y, table=table)  # noqa: E731
    name = {v: k for k, v in SYMMETRIES.items()}[sym]
    if name == "C1":
        return s.copy()
    if name == "C2":
        return s | tf(s, T["Rotate180EvenBoth"], dx + 1, dy + 1)
    if name == "C4":
        a = s | tf(s, T["Rotate90"], dx, dy)
        return a | tf(a, T["Rotate180EvenBoth"], dx - dy + 1, dy + dx + 1)
    if name == "D2AcrossX":
        return s | tf(s, T["ReflectAcrossXEven"], dx, dy + 1)
    if name == "D2AcrossY":
        return s | tf(s, T["ReflectAcrossYEven"], dx + 1, dy)
    if name == "D2diagodd":
        return s | tf(s, T["ReflectAcrossYeqX"], dx, dy)
    if name == "D2negdiagodd":
        return s | tf(s, T["ReflectAcrossYeqNegX"], dx + 1, dy + 1)
    if name == "D4":
        a = s | tf(s, T["ReflectAcrossXEven"], 0, dy + 1)
        return a | tf(a, T["ReflectAcrossYEven"], dx + 1, 0)
    assert name == "D4diag"
    px, py = perp("YeqX", dx, dy)
    qx, qy = perp("YeqNegXP1", dx, dy)
    a = s | tf(s, T["ReflectAcrossYeqX"], px, py)
    return a | tf(a, T["ReflectAcrossYeqNegX"], qx + 1, qy + 1)


# ---- XYBounds and the orbit ----
def rotr64(v, k):
    v, k = int(v), k % 64
    return ((v >> k) | (v << (64 - k))) & (2 ** 64 - 1)


def np_bounds(state, rotated=True):
    s = np.asarray(state, np.uint64).reshape(64)
    cols = sum(1 << x for x in range(64) if s[x])
    rows = int(np.bitwise_or.reduce(s))
    if rows == 0:
        return (-1, -1, -1, -1)
    if not rotated:  # mutation: the unrotated window, columns and rows 0..63
        f = lambda m: ((m & -m).bit_length() - 1, m.bit_length() - 1)  # noqa: E731
        (l, r), (t, b) = f(cols), f(rows)
        return (l, t, r, b)
    c, r = rotr64(cols, 32), rotr64(rows, 32)
    ctz = lambda m: (m & -m).bit_length() - 1  # noqa: E731
    return (ctz(c) - 32, ctz(r) - 32, 31 - (64 - c.bit_length()), 31 - (64 - r.bit_length()))


def np_orbit(state, order=ORBIT_ORDER, normalise=True):
    """(the eight images, the mask of those equal to no earlier one)"""
    images, mask = [], 0
    for i, t in enumerate(order):
        img = np_transform(state, t)
        if normalise:
            b = np_bounds(img)
            img = np_transform(img, 0, -b[0], -b[1])
        if not any((img == e).all() for e in images):
            mask |= 1 << i
        images.append(img)
    return np.stack(images), mask


def np_bounds_batch(states):
    return np.array([np_bounds(s) for s in np.asarray(states, np.uint64).reshape(-1, 64)], np.int32).reshape(-1, 4)


def np_orbit_batch(states):
    """np_orbit for (n, 64) states: ((n, 8, 64) images, (n,) uint8 masks)"""
    s = np.ascontiguousarray(states, np.uint64).reshape(-1, 64)
    images, masks = np.zeros((len(s), 8, 64), np.uint64), np.zeros(len(s), np.uint8)
    k = np.arange(64)
    for i, t in enumerate(ORBIT_ORDER):
        img = np_transform_batch(s, t)
        b = np_bounds_batch(img)
        # Moved(-left, -top): column x from column x + left, every word rotated right by top
        img = np.take_along_axis(img, (k[None, :] + b[:, :1]) % 64, axis=1)
        top = (b[:, 1:2] % 64).astype(np.uint64)
        img = np.where(top == 0, img, (img >> top) | (img << ((np.uint64(64) - top) % np.uint64(64))))
        images[:, i] = img
        new = np.ones(len(s), bool)
        for j in range(i):
            new &= (images[:, j] != img).any(axis=1)
        masks |= new.astype(np.uint8) << np.uint8(i)
    return images, masks


# ---- the inputs the golden was recorded on (regenerated, not stored) ----
def transform_states(port):
    return np.concatenate([port.fill(N_RANDOM, seed=121), np.stack([cell(x, y) for x, y in CELLS])])


def sparse_states(port):
    return port.fill(2, seed=122) & port.fill(2, seed=123) & port.fill(2, seed=124)


def symmetricize_states(port):
    return np.concatenate([np_transform(port.parse(PATTERNS["R5"]), 0, 3, 5)[None], sparse_states(port)])


def orbit_bases(port):
    """the states the orbit cases move: the named patterns at the origin, a
    full-density random state and one ANDed down to 1/16"""
    named = [np.zeros(64, np.uint64) if r is None else port.parse(r) for r in PATTERNS.values()]
    thin = port.fill(1, seed=126) & port.fill(1, seed=127) & port.fill(1, seed=128) & port.fill(1, seed=129)
    return np.stack(named + [port.fill(1, seed=125)[0], thin[0]])


ORBIT_NAMES = tuple(PATTERNS) + ("dense", "thin")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


# ---- the sweeps (tests/golden/symmetry_sweeps.npz): every residue of a shift, every symmetry at every offset
# of two lines, the extreme pairs of a bounding box, every stabiliser subgroup, and images that differ in one
# half only.  Inputs are built here and never stored. ----
SWEEPS = os.path.join(os.path.dirname(GOLDEN), "symmetry_sweeps.npz")
SWEEP_CELL = (17, 42)
SHIFT_SWEEPS = {"dx": tuple((k, -27) for k in range(64)), "dy": tuple((13, k) for k in range(64)),
                "both": tuple((k, k) for k in range(64))}
SHIFT_EXTREMES = ((-1, -64), (64, 63), (-65, 129), (2 ** 31 - 1, -2 ** 31))
SHIFTS = SHIFT_SWEEPS["dx"] + SHIFT_SWEEPS["dy"] + SHIFT_SWEEPS["both"] + SHIFT_EXTREMES
IN_PLACE_K = (0, 16, 31, 32, 33, 63)        # of each sweep: also run in place on the GPU
SYM_SWEEP_DX = tuple((dx, 13) for dx in range(-70, 71))
SYM_SWEEP_DY = tuple((-40, dy) for dy in range(-70, 71))
SYM_SWEEP = SYM_SWEEP_DX + SYM_SWEEP_DY
# the 10 subgroups of the orbit's eight transforms, as indices into ORBIT_ORDER (0 Identity, 1 ReflectAcrossX,
# 2 ReflectAcrossYeqX, 3 ReflectAcrossY, 4 ReflectAcrossYeqNegXP1, 5 Rotate90, 6 Rotate270, 7 Rotate180OddBoth)
SUBGROUPS = {"1": (0,), "AcrossX": (0, 1), "YeqX": (0, 2), "AcrossY": (0, 3), "YeqNegX": (0, 4), "C2": (0, 7),
             "C4": (0, 5, 6, 7), "D2axes": (0, 1, 3, 7), "D2diag": (0, 2, 4, 7), "D4": tuple(range(8))}
STABILISER_SPOTS = ((0, 0), (-3, 40), (29, 30))   # the last straddles the window's seam
STABILISER_MASKS = (0xFF, 0x1D, 0x1B, 0x17, 0x0F, 0x27, 0x05, 0x03, 0x01)
FRAME_EXTRA = ((5, 35), (35, 5))            # the one cell added to the 40 x 40 frame, in frame coordinates


def cells(points):
    s = np.zeros(64, np.uint64)
    for x, y in points:
        s[x % 64] |= np.uint64(1) << np.uint64(y % 64)
    return s


def pair_states():
    """{(a, 5), (b, 40)} and then {(7, a), (50, b)} for all a, b in 0..63: every
    pair of populated columns, then of populated rows"""
    word = np.uint64(1) << np.arange(64, dtype=np.uint64)
    a, b = (v.ravel() for v in np.meshgrid(np.arange(64), np.arange(64), indexing="ij"))
    s, n = np.zeros((8192, 64), np.uint64), np.arange(4096)
    s[n, a] |= word[5]
    s[n, b] |= word[40]
    s[4096 + n, 7] |= word[a]
    s[4096 + n, 50] |= word[b]
    return s


def stabiliser_pattern():
    """7 seeded cells within radius 6 of the origin, at the origin"""
    rng = np.random.default_rng(909)
    at = rng.choice(13 * 13, size=7, replace=False)
    return cells([(int(k) // 13 - 6, int(k) % 13 - 6) for k in at])


def stabiliser_states():
    """per subgroup H and spot, the union over H of the pattern's images, moved
    to the spot; then Symmetricize(pattern, sym, 0, 0) for the 9 symmetries"""
    p = stabiliser_pattern()
    out = []
    for h in SUBGROUPS.values():
        u = np.bitwise_or.reduce([np_transform(p, ORBIT_ORDER[i]) for i in h])
        out += [np_transform(u, 0, dx, dy) for dx, dy in STABILISER_SPOTS]
    out += [np_symmetricize(p, sym, 0, 0) for sym in SYMMETRIES.values()]
    return np.stack(out)


STABILISER_NAMES = tuple(f"{h}@{spot}" for h in SUBGROUPS for spot in STABILISER_SPOTS) + tuple(SYMMETRIES)


def frame_states():
    """the 40 x 40 square frame at (-20, -20) and one more cell: taller and
    wider than 32, all eight images distinct, two of them in one half only"""
    frame = [(x - 20, y - 20) for x in range(40) for y in range(40) if x in (0, 39) or y in (0, 39)]
    return np.stack([cells(frame + [(fx - 20, fy - 20)]) for fx, fy in FRAME_EXTRA])


def orbit_sweep_states():
    return np.concatenate([stabiliser_states(), frame_states()])


def first_masks(images, keep=np.uint64(2 ** 64 - 1), columns=slice(None)):
    """the orbit's mask from (n, 8, 64) images, compared on the rows of `keep`
    and the given columns only"""
    v = (np.asarray(images, np.uint64) & keep)[:, :, columns]
    masks = np.zeros(len(v), np.uint8)
    for i in range(8):
        new = np.ones(len(v), bool)
        for j in range(i):
            new &= (v[:, j] != v[:, i]).any(axis=1)
        masks |= new.astype(np.uint8) << np.uint8(i)
    return masks


@pytest.fixture(scope="module")
def sweeps():
    return dict(np.load(SWEEPS))


# ---- the table is derived from the recorded impulses ----
def where(state):
    g = unpack(state)
    assert g.sum() == 1
    x, y = np.argwhere(g)[0]
    return int(x), int(y)


def test_affine_maps_derived_from_impulses(gold):
    """b from the image of (0, 0), A's columns from those of (-1, 0) and
    (0, -1); the model's table is that map, and it sends the other recorded
    cells where the reference did"""
    images = gold["transform"][:, N_RANDOM:]
    seen = set()
    for t in range(16):
        at = [where(images[t][k]) for k in range(len(CELLS))]
        b = at[0]
        wrap = lambda v: (v + 32) % 64 - 32  # noqa: E731
        ex = tuple(wrap(b[k] - at[1][k]) for k in (0, 1))   # A (1, 0) = b - image of (-1, 0)
        ey = tuple(wrap(b[k] - at[2][k]) for k in (0, 1))
        assert sorted(map(abs, ex + ey)) == [0, 0, 1, 1] and abs(ex[0]) != abs(ey[0]), (t, ex, ey)
        swap = ex[0] == 0
        derived = (swap, ey[0] if swap else ex[0], ex[1] if swap else ey[1], wrap(b[0]), wrap(b[1]))
        assert derived == TABLE[t], (TRANSFORMS[t], derived, TABLE[t])
        seen.add(derived)
        for (x, y), got in zip(CELLS, at):
            u, v = (y, x) if swap else (x, y)
            assert got == ((derived[1] * u + derived[3]) % 64, (derived[2] * v + derived[4]) % 64)
    assert len(seen) == 16


def test_transform_golden(port, gold):
    states = transform_states(port)
    for t in range(16):
        for k, s in enumerate(states):
            assert (np_transform(s, t) == gold["transform"][t][k]).all(), (TRANSFORMS[t], k)
        assert (np_transform_batch(states, t) == gold["transform"][t]).all()


def test_transform_then_move_golden(port, gold):
    states = transform_states(port)[:2]
    for t in range(16):
        for m, (dx, dy) in enumerate(MOVES):
            assert (np_transform_batch(states, t, dx, dy) == gold["transform_move"][t][m]).all(), (TRANSFORMS[t], dx, dy)
            assert (np_transform(states[1], t, dx, dy) == gold["transform_move"][t][m][1]).all()


def test_symmetricize_golden(port, gold):
    states = symmetricize_states(port)
    for k, sym in enumerate(SYMMETRIES.values()):
        for i, s in enumerate(states):
            for o, (dx, dy) in enumerate(OFFSETS):
                assert (np_symmetricize(s, sym, dx, dy) == gold["symmetricize"][k][i][o]).all(), (sym, i, dx, dy)
        for o, (dx, dy) in enumerate(OFFSETS):   # and the batch form
            assert (np_symmetricize(states, sym, dx, dy) == gold["symmetricize"][k][:, o]).all(), (sym, dx, dy)


def test_bounds_and_orbit_golden(port, gold):
    bases = orbit_bases(port)
    for p, base in enumerate(bases):
        for m, (dx, dy) in enumerate(ORBIT_MOVES):
            s = np_transform(base, 0, dx, dy)
            assert (s == gold["orbit_states"][p][m]).all(), (ORBIT_NAMES[p], dx, dy)
            assert np_bounds(s) == tuple(gold["bounds"][p][m]), (ORBIT_NAMES[p], dx, dy)
            images, mask = np_orbit(s)
            assert (images == gold["orbit_images"][p][m]).all(), (ORBIT_NAMES[p], dx, dy)
            assert mask == gold["orbit_mask"][p][m], (ORBIT_NAMES[p], dx, dy)
    flat = gold["orbit_states"].reshape(-1, 64)
    assert (np_bounds_batch(flat) == gold["bounds"].reshape(-1, 4)).all()
    images, masks = np_orbit_batch(flat)
    assert (images == gold["orbit_images"].reshape(-1, 8, 64)).all() and (masks == gold["orbit_mask"].ravel()).all()


def test_golden_sharp_edges(gold):
    """the cases the reference's semantics are sharp on"""
    p, m = ORBIT_NAMES.index("block"), ORBIT_MOVES.index((30, 31))
    assert tuple(gold["bounds"][p][m]) == (30, -32, 31, 31) and bin(gold["orbit_mask"][p][m]).count("1") == 3
    assert bin(gold["orbit_mask"][ORBIT_NAMES.index("L3")][m]).count("1") == 7
    e = ORBIT_NAMES.index("empty")
    assert (gold["bounds"][e] == -1).all() and (gold["orbit_mask"][e] == 1).all()
    assert (gold["orbit_images"][e] == 0).all()
    masks = set(gold["orbit_mask"].ravel().tolist())
    assert len(masks) >= 8 and {0x01, 0xFF, 0x07, 0x7F} <= masks
    assert any(k & (k >> 1) != k >> 1 for k in masks)   # a set bit above a clear one


# ---- the sweeps ----
def test_shift_sweep_golden(sweeps):
    """Transformed(t).Moved(dx, dy) of one cell at every residue of dx, of dy
    and of both, and at moves far out of range"""
    s = cell(*SWEEP_CELL)
    for t in range(16):
        for m, (dx, dy) in enumerate(SHIFTS):
            want = cell(*sweeps["shift_landing"][t][m].tolist())
            assert (np_transform(s, t, dx, dy) == want).all(), (TRANSFORMS[t], dx, dy)
            assert (np_transform_batch(s[None], t, dx, dy)[0] == want).all(), (TRANSFORMS[t], dx, dy)
    # on the recording alone: the 64 residues of a sweep land the cell on 64 places
    for k in range(3):
        for t in range(16):
            assert len({tuple(c) for c in sweeps["shift_landing"][t][64 * k:64 * k + 64].tolist()}) == 64, (k, t)
    # and a far move is its residue: (-1, -64) and (2^31 - 1, -2^31) are both (63, 0) mod 64
    far = sweeps["shift_landing"][:, 192:]
    assert (far[:, 0] == far[:, 3]).all() and (far[:, 0] != far[:, 1]).any(axis=1).all()


def test_symmetricize_sweep_golden(port, sweeps):
    s = symmetricize_states(port)[0]
    for k, sym in enumerate(SYMMETRIES.values()):
        for o, (dx, dy) in enumerate(SYM_SWEEP):
            assert (np_symmetricize(s, sym, dx, dy) == sweeps["symmetricize_sweep"][k][o]).all(), (sym, dx, dy)
            assert (np_symmetricize(s[None], sym, dx, dy)[0] == sweeps["symmetricize_sweep"][k][o]).all()


def test_extreme_pairs_golden(sweeps):
    pairs = pair_states()
    bounds = np_bounds_batch(pairs)
    assert (bounds == sweeps["pair_bounds"]).all()
    assert (np_orbit_batch(pairs)[1] == sweeps["pair_mask"]).all()
    for u in range(0, 8192, 97):   # and the scalar forms on a sample
        assert np_bounds(pairs[u]) == tuple(sweeps["pair_bounds"][u]) and np_orbit(pairs[u])[1] == sweeps["pair_mask"][u]
    # on the recording alone: most boxes of the window occur
    assert len({tuple(b) for b in sweeps["pair_bounds"].tolist()}) >= 4000


def test_stabilisers_and_frames_golden(sweeps):
    states = orbit_sweep_states()
    assert len(states) == len(STABILISER_NAMES) + 2 == len(sweeps["orbit_mask"])
    assert (np_bounds_batch(states) == sweeps["orbit_bounds"]).all()
    images, masks = np_orbit_batch(states)
    assert (images == sweeps["orbit_images"]).all() and (masks == sweeps["orbit_mask"]).all()
    for u, s in enumerate(states):
        one, mask = np_orbit(s)
        assert (one == sweeps["orbit_images"][u]).all() and mask == sweeps["orbit_mask"][u], u


def test_sweeps_sharp_edges(sweeps):
    """on the recording alone: every stabiliser subgroup's mask occurs, the two
    subgroups that share a mask differ in their images, and the frames' images
    differ in one half only"""
    images, masks = sweeps["orbit_images"], sweeps["orbit_mask"]
    stab = masks[:len(STABILISER_NAMES)]
    assert set(STABILISER_MASKS) <= set(stab.tolist()), sorted(set(stab.tolist()))
    c4, klein = STABILISER_NAMES.index("C4@(0, 0)"), STABILISER_NAMES.index("D2diag@(0, 0)")
    assert masks[c4] == masks[klein] == 0x03 and (images[c4] != images[klein]).any()
    # C4 sends the pattern's reflection to one other image, the diagonal Klein group to the pattern itself
    assert (images[c4][1] == images[c4][2]).all() and (images[klein][0] == images[klein][2]).all()
    assert (sweeps["orbit_bounds"][-2:] == (-20, -20, 19, 19)).all() and (masks[-2:] == 0xFF).all()
    assert (first_masks(images) == masks).all()
    low = np.uint64(0xFFFFFFFF)
    assert first_masks(images[-2:], keep=low).tolist() == [0xA7, 0x5B]           # rows < 32 only
    assert first_masks(images[-2:], keep=~low).tolist() == [0x5B, 0xA7]          # rows >= 32 only
    assert first_masks(images[-2:], columns=slice(0, 32)).tolist() == [0x37, 0xCD]
    assert first_masks(images[-2:], columns=slice(32, 64)).tolist() == [0xCD, 0x37]
    tall = images[-2]
    assert ((tall[0] ^ tall[3]) & low == 0).all() and (tall[0] != tall[3]).any()   # images 0 and 3: a row >= 32


# ---- mutations: each must contradict a recorded answer ----
def test_mutation_perp_component_sweep(port, sweeps):
    """floor division, or the offset reduced mod 64 first, in PerpComponent:
    each is contradicted on the dx sweep, where the reference truncates"""
    s, k = symmetricize_states(port)[0], list(SYMMETRIES).index("D4diag")
    for perp in (perp_floor, perp_mod64):
        told = [(np_symmetricize(s, SYMMETRIES["D4diag"], dx, dy, perp=perp) != sweeps["symmetricize_sweep"][k][o]).any()
                for o, (dx, dy) in enumerate(SYM_SWEEP_DX)]
        assert any(told), perp.__name__


def transform_contradicted(gold, port, **kw):
    states = transform_states(port)
    return any((np_transform(s, t, **kw) != gold["transform"][t][k]).any()
               for t in range(16) for k, s in enumerate(states))


def test_mutation_exchanged_transforms(gold):
    """any two of the 16 exchanged: the cell (17, 42) alone tells"""
    k = N_RANDOM + CELLS.index((17, 42))
    s = cell(17, 42)
    for i, j in itertools.combinations(range(16), 2):
        table = list(TABLE)
        table[i], table[j] = table[j], table[i]
        assert (np_transform(s, i, table=table) != gold["transform"][i][k]).any(), (TRANSFORMS[i], TRANSFORMS[j])


def test_mutation_dropped_plus_one(gold, port):
    """the Move(.., 1) of each odd transform dropped: it becomes its even twin"""
    twins = {"ReflectAcrossX": "ReflectAcrossXEven", "ReflectAcrossY": "ReflectAcrossYEven",
             "Rotate90": "Rotate90Even", "Rotate270": "Rotate270Even", "Rotate180OddBoth": "Rotate180EvenBoth",
             "Rotate180EvenHorizontal": "Rotate180EvenBoth", "Rotate180EvenVertical": "Rotate180EvenBoth",
             "ReflectAcrossYeqNegXP1": "ReflectAcrossYeqNegX"}
    dropped = build_table(plus=0)
    states = transform_states(port)
    for odd, even in twins.items():
        assert dropped[T[odd]] == TABLE[T[even]]
        for k, s in enumerate(states):
            assert (np_transform(s, T[odd], table=dropped) != gold["transform"][T[odd]][k]).any(), (odd, k)


def test_mutation_wrong_diagonal(gold, port):
    wrong = build_table(transpose={False: TRANSPOSE[True], True: TRANSPOSE[False]})
    states = transform_states(port)
    for t in range(16):
        if TABLE[t][0]:
            for k, s in enumerate(states):
                assert (np_transform(s, t, table=wrong) != gold["transform"][t][k]).any(), (TRANSFORMS[t], k)
    # and in Symmetricize's two diagonal cases
    s = symmetricize_states(port)[0]
    for name in ("D2diagodd", "D2negdiagodd", "D4diag"):
        k = list(SYMMETRIES).index(name)
        assert (np_symmetricize(s, SYMMETRIES[name], 7, -3, table=wrong) != gold["symmetricize"][k][0][1]).any(), name


def test_mutation_move_first(gold, port):
    """Move before the transform instead of after: told by every transform
    whose linear part is not the identity"""
    s = transform_states(port)[0]
    dx, dy = MOVES[7]   # (40, 25) mod 64: no element of D4 but the identity fixes it
    for t in range(1, 16):
        assert (np_transform(s, t, dx, dy, move_first=True) != gold["transform_move"][t][7][0]).any(), TRANSFORMS[t]


def test_mutation_perp_component(gold, port):
    k, states = list(SYMMETRIES).index("D4diag"), symmetricize_states(port)
    for perp in (perp_floor, perp_mod64):
        assert any((np_symmetricize(s, SYMMETRIES["D4diag"], dx, dy, perp=perp) != gold["symmetricize"][k][i][o]).any()
                   for i, s in enumerate(states) for o, (dx, dy) in enumerate(OFFSETS)), perp.__name__


def test_mutation_unrotated_bounds(gold):
    """told by every pattern once it is moved off the quadrant both windows share"""
    for p in range(1, len(ORBIT_NAMES)):
        assert any(np_bounds(gold["orbit_states"][p][m], rotated=False) != tuple(gold["bounds"][p][m])
                   for m in range(len(ORBIT_MOVES))), ORBIT_NAMES[p]


def test_mutation_orbit(gold):
    states, masks = gold["orbit_states"].reshape(-1, 64), gold["orbit_mask"].ravel()
    raw = [np_orbit(s, normalise=False)[1] for s in states]
    assert any(a != b for a, b in zip(raw, masks)), "comparing without normalising"
    enum_order = tuple(sorted(ORBIT_ORDER))
    assert any(np_orbit(s, order=enum_order)[1] != b for s, b in zip(states, masks)), "the enum's order"
    assert any((np_orbit(s, order=enum_order)[0] != g).any()
               for s, g in zip(states, gold["orbit_images"].reshape(-1, 8, 64)))


# ---- ABI: argument validation without a device ----
def test_argument_validation_without_device():
    import lifeapi_amd.hip as hip
    L = hip.lib
    a, b, far = 4096, 4096 + 8 * 512, 1 << 30   # fake device addresses: never dereferenced
    for f, extra in ((L.lifeapi_transform_batch_dev, (6,)), (L.lifeapi_symmetricize_batch_dev, (11,))):
        assert f(None, None, 4, *extra, 1, 2, None) == -1
        assert b"null" in L.lifeapi_last_error()
        assert f(a + 4, b, 4, *extra, 1, 2, None) == -1
        assert b"aligned" in L.lifeapi_last_error()
        assert f(a, a + 512, 4, *extra, 1, 2, None) == -1
        assert b"overlap" in L.lifeapi_last_error()
        assert f(None, None, 0, *extra, 1, 2, None) == 0
    assert L.lifeapi_transform_batch_dev(a, b, 4, 16, 0, 0, None) == -1
    assert b"transform" in L.lifeapi_last_error()
    for sym in UNDEFINED_SYMMETRIES:
        assert L.lifeapi_symmetricize_batch_dev(a, b, 4, sym, 0, 0, None) == -1
        assert b"undefined" in L.lifeapi_last_error()
    # bounds
    assert L.lifeapi_bounds_batch_dev(None, far, 4, None) == -1
    assert L.lifeapi_bounds_batch_dev(a, None, 4, None) == -1
    assert L.lifeapi_bounds_batch_dev(a + 4, far, 4, None) == -1
    assert L.lifeapi_bounds_batch_dev(a, far + 2, 4, None) == -1
    assert b"misaligned" in L.lifeapi_last_error()
    assert L.lifeapi_bounds_batch_dev(a, a + 3 * 512, 4, None) == -1
    assert b"overlap" in L.lifeapi_last_error()
    assert L.lifeapi_bounds_batch_dev(None, None, 0, None) == 0
    # the orbit
    assert L.lifeapi_symmetry_orbit_batch_dev(a, None, None, 4, None) == -1
    assert b"both" in L.lifeapi_last_error()
    assert L.lifeapi_symmetry_orbit_batch_dev(None, far, far - 64, 4, None) == -1
    assert L.lifeapi_symmetry_orbit_batch_dev(a + 4, far, None, 4, None) == -1
    assert L.lifeapi_symmetry_orbit_batch_dev(a, far + 4, None, 4, None) == -1
    assert b"misaligned" in L.lifeapi_last_error()
    assert L.lifeapi_symmetry_orbit_batch_dev(a, a + 512, None, 4, None) == -1
    assert b"overlap" in L.lifeapi_last_error()
    assert L.lifeapi_symmetry_orbit_batch_dev(far, far - 8 * 512 * 4 + 8, None, 4, None) == -1   # the last word
    assert b"overlap" in L.lifeapi_last_error()
    assert L.lifeapi_symmetry_orbit_batch_dev(a, None, a + 4 * 512 - 1, 4, None) == -1
    assert b"overlap" in L.lifeapi_last_error()
    assert L.lifeapi_symmetry_orbit_batch_dev(a, far, far + 100, 4, None) == -1
    assert b"d_first overlaps" in L.lifeapi_last_error()
    assert L.lifeapi_symmetry_orbit_batch_dev(None, None, None, 0, None) == 0
