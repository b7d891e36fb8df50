"""CPU: numpy definitions of IntersectingOffsets (Symmetry.hpp:729-772), of
a.Convolve(b.Transformed(t)) (LifeAPI.hpp:1293-1370) and of Halve / HalveX /
HalveY / Skew / InvSkew (Symmetry.hpp:681-727), pinned to every array of
tests/golden/pair.npz, which tests/golden/make_pair_golden.py recorded from
the reference itself.

The model moves cells one by one: Convolve is the OR over the cells (p, q) of
the second operand of the first operand moved by (p, q); the transform is the
affine map of tests/test_symmetry_model.py.  Nothing in it resembles the
kernels' walk, the choice of the walked operand or the bit tricks of Halve.
Every mutation listed at the end must contradict a recorded answer.

The per-universe-offset calls need no recording of their own: their model is
M.np_transform / M.np_symmetricize row by row, pinned here to the sweeps of
tests/golden/symmetry_sweeps.npz with universe u carrying offset u.

The GPU tests (tests/test_gpu_pair.py), the facade test and the generator
import the models and the inputs from here.
"""
import os

import numpy as np
import pytest

import test_symmetry_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair.npz")

# the symmetries IntersectingOffsets defines, with the transform it applies to pat1 (Symmetry.hpp:733-767)
IO_TRANSFORM = {"C2": "Identity", "C4": "Rotate270", "D2AcrossX": "ReflectAcrossY", "D2AcrossY": "ReflectAcrossX",
                "D2diagodd": "ReflectAcrossYeqNegXP1", "D2negdiagodd": "ReflectAcrossYeqX"}
IO_SYMS = tuple(IO_TRANSFORM)
IO_VALUES = {"C2": 7, "C4": 11, "D2AcrossX": 1, "D2AcrossY": 3, "D2diagodd": 6, "D2negdiagodd": 5}
IO_UNDEFINED = tuple(v for v in range(22) if v not in IO_VALUES.values())      # C1, D4 and D4diag among them
# the nearest wrong transforms: the other rotation, the other axis, the other diagonal, the Even variants
IO_WRONG = {"C4": ("Rotate90", "Rotate270Even"), "D2AcrossX": ("ReflectAcrossX", "ReflectAcrossYEven"),
            "D2AcrossY": ("ReflectAcrossY", "ReflectAcrossXEven"),
            "D2diagodd": ("ReflectAcrossYeqX", "ReflectAcrossYeqNegX"), "D2negdiagodd": ("ReflectAcrossYeqNegXP1",)}
SPOTS = ((0, 0), (30, 31), (-2, -1), (31, 5), (7, 30), (40, 50))     # some on the window's seams
N_SPARSE, N_PAIR16 = 40, 6
HALVE_MODES = ("Halve", "HalveX", "HalveY")


# ---- the definitions ----
def pop(state):
    return int(M.unpack(state).sum())


def np_convolve(a, b):
    """a.Convolve(b): the OR over the cells (p, q) of b of a moved by (p, q)"""
    g, out = M.unpack(a), np.zeros((64, 64), bool)
    for p, q in zip(*np.nonzero(M.unpack(b))):
        out |= np.roll(g, (int(p), int(q)), axis=(0, 1))
    return M.pack(out)


def np_convolve_words(a, b):
    """the same on the 64 words, for the GPU tests' large batches: cell (p, q) of b ORs in
    column x of a, rotated left by q, at column x + p (pinned to the recording below)"""
    a, out = np.asarray(a, np.uint64), np.zeros(64, np.uint64)
    for p, q in zip(*np.nonzero(M.unpack(b))):
        r = np.uint64(q)
        out |= np.roll(a if q == 0 else (a << r) | (a >> (np.uint64(64) - r)), int(p))
    return out


def np_convolve_pair(a, b, t):
    return np_convolve(a, M.np_transform(b, t))


def np_intersecting(pat1, pat2, sym, transforms=IO_TRANSFORM):
    """IntersectingOffsets(pat1, pat2, sym) = pat2.Convolve(pat1.Transformed(t)); sym by name"""
    return np_convolve_pair(pat2, pat1, M.T[transforms[sym]])


def np_halve(state, mode, odd=False):
    """Halve (0), HalveX (1), HalveY (2): every second column and / or row, repeated in both halves"""
    g, k = M.unpack(state), 2 * (np.arange(64) % 32) + (1 if odd else 0)
    if mode != 2:
        g = g[k, :]
    if mode != 1:
        g = g[:, k]
    return M.pack(g)


def np_skew(state, inverse=False):
    """Skew (x, y) -> (x, y + x); InvSkew (x, y) -> (x, y - x)"""
    g, out = M.unpack(state), np.zeros((64, 64), bool)
    x, y = np.nonzero(g)
    out[x, (y - x if inverse else y + x) % 64] = True
    return M.pack(out)


def np_transform_offsets(states, t, offsets):
    return np.stack([M.np_transform(s, t, int(dx), int(dy)) for s, (dx, dy) in zip(states, offsets)])


def np_symmetricize_offsets(states, sym, offsets):
    return np.stack([M.np_symmetricize(s, sym, int(dx), int(dy)) for s, (dx, dy) in zip(states, offsets)])


# ---- the inputs the golden was recorded on (regenerated, not stored) ----
RESIDUE_PAT2 = M.SWEEP_CELL                       # (17, 42)
RESIDUE_PAT1 = M.SHIFT_SWEEPS["dx"] + M.SHIFT_SWEEPS["dy"] + M.SHIFT_SWEEPS["both"]   # 3 lines of 64 cells


def residue_states():
    """(192, 64): pat1 of the residue sweep, one cell each"""
    return np.stack([M.cells([c]) for c in RESIDUE_PAT1])


def small_pattern(rng, spot):
    """2..24 seeded cells in a box of at most 12 x 12, its corner at `spot`"""
    w, h = (int(v) for v in rng.integers(2, 13, size=2))
    k = int(rng.integers(2, min(24, w * h) + 1))
    at = rng.choice(w * h, size=k, replace=False)
    return M.cells([(spot[0] + int(c) // h, spot[1] + int(c) % h) for c in at])


def sparse_pairs():
    """((40, 64) pat1, (40, 64) pat2): every pair differs, the spots of the two run through all 36 pairs"""
    rng = np.random.default_rng(1818)
    p1 = np.stack([small_pattern(rng, SPOTS[i % 6]) for i in range(N_SPARSE)])
    p2 = np.stack([small_pattern(rng, SPOTS[(i // 6 + i) % 6]) for i in range(N_SPARSE)])
    assert all((a != b).any() for a, b in zip(p1, p2))
    return p1, p2


def choice_cases(port):
    """(name, x, y) of the operand-choice cases; each is recorded as
    IntersectingOffsets(x, y, sym) and IntersectingOffsets(y, x, sym)"""
    dense, empty = port.fill(1, seed=1820)[0], np.zeros(64, np.uint64)
    few = [(9, 5), (33, 62), (60, 31)]
    p1, p2 = sparse_pairs()
    five = [M.cells([(3, 4), (5, 40), (31, 31), (32, 0), (63, 63)]), M.cells([(0, 1), (1, 0), (20, 33), (44, 7), (45, 9)])]
    column = np.zeros(64, np.uint64)
    column[21] = ~np.uint64(0)                                    # the reference's special case (LifeAPI.hpp:1304)
    run40 = M.cells([(50, y) for y in range(10, 50)])             # its min(runlength, 32)
    high = M.cells([(2, 32), (2, 47), (40, 63), (63, 33), (17, 50)])   # rows >= 32 only
    glider = M.cells([(1, 0), (2, 1), (0, 2), (1, 2), (2, 2)])
    return (("dense x 1", dense, M.cells(few[:1])), ("dense x 2", dense, M.cells(few[:2])),
            ("dense x 3", dense, M.cells(few)), ("equal", five[0], five[1]),
            ("empty x sparse", empty, p1[3]), ("empty x dense", empty, dense), ("both empty", empty, empty),
            ("full column", column, glider), ("run of 40", run40, glider), ("high rows", high, p2[5]))


def halve_states(port):
    """8 random states, the 64 single-column states (a seeded word each), the 64 single-row states"""
    words = port.fill(1, seed=1822)[0]
    cols = np.zeros((64, 64), np.uint64)
    cols[np.arange(64), np.arange(64)] = words
    on = M.unpack(port.fill(1, seed=1823)[0])          # [y, x]: the populated columns of row y's state
    rows = np.where(on, np.uint64(1) << np.arange(64, dtype=np.uint64)[:, None], np.uint64(0)).astype(np.uint64)
    return np.concatenate([port.fill(8, seed=1821), cols, rows])


def pair16():
    """six sparse pairs for lifeapi_convolve_pair with each of the 16 transforms"""
    p1, p2 = sparse_pairs()
    return p1[:N_PAIR16], p2[7:7 + N_PAIR16]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


# ---- the model is the recording ----
def test_residue_sweep(gold):
    pat2 = M.cells([RESIDUE_PAT2])
    for k, sym in enumerate(IO_SYMS):
        for c, at in zip(RESIDUE_PAT1, gold["residue_landing"][k]):
            assert (np_intersecting(M.cells([c]), pat2, sym) == M.cell(*at.tolist())).all(), (sym, c)


def test_sparse_pairs(gold):
    p1, p2 = sparse_pairs()
    for k, sym in enumerate(IO_SYMS):
        for i in range(N_SPARSE):
            assert (np_intersecting(p1[i], p2[i], sym) == gold["sparse_pairs"][k, i]).all(), (sym, i)
            assert (np_intersecting(p1[i], p1[i], sym) == gold["sparse_self"][k, i]).all(), (sym, i)
            t1 = M.np_transform(p1[i], M.T[IO_TRANSFORM[sym]])
            assert (np_convolve_words(p2[i], t1) == gold["sparse_pairs"][k, i]).all(), (sym, i, "words")
            assert (np_convolve_words(t1, p2[i]) == gold["sparse_pairs"][k, i]).all(), (sym, i, "words, exchanged")


def test_operand_choice(gold, port):
    cases = choice_cases(port)
    assert gold["choice"].shape == (len(IO_SYMS), len(cases), 2, 64)
    for k, sym in enumerate(IO_SYMS):
        for i, (name, x, y) in enumerate(cases):
            assert (np_intersecting(x, y, sym) == gold["choice"][k, i, 0]).all(), (sym, name)
            assert (np_intersecting(y, x, sym) == gold["choice"][k, i, 1]).all(), (sym, name, "exchanged")
            if "empty" in name:
                assert not gold["choice"][k, i].any(), (sym, name)
            t = M.np_transform(x, M.T[IO_TRANSFORM[sym]])
            assert (np_convolve_words(y, t) == gold["choice"][k, i, 0]).all(), (sym, name, "words")
            assert (np_convolve_words(t, y) == gold["choice"][k, i, 0]).all(), (sym, name, "words, exchanged")
    # Convolve is symmetric in its operands: with no transform the reference's two orders agree
    assert (gold["choice"][IO_SYMS.index("C2"), :, 0] == gold["choice"][IO_SYMS.index("C2"), :, 1]).all()


def test_convolve_pair_every_transform(gold):
    a, b = pair16()
    for t in range(16):
        for i in range(N_PAIR16):
            assert (np_convolve_pair(a[i], b[i], t) == gold["convolve_pair"][t, i]).all(), (M.TRANSFORMS[t], i)


def test_halve_and_skew(gold, port):
    states = halve_states(port)
    assert len(states) == 136
    for i, s in enumerate(states):
        for mode in range(3):
            assert (np_halve(s, mode) == gold["halve"][mode, i]).all(), (HALVE_MODES[mode], i)
        for inverse in (False, True):
            assert (np_skew(s, inverse) == gold["skew"][int(inverse), i]).all(), (inverse, i)


def test_per_universe_offsets_are_the_sweeps(port):
    """universe u carrying offset u: the recorded Symmetricize sweep of the
    R-pentomino and the landing of the cell under every transform at every shift"""
    sweeps = dict(np.load(M.SWEEPS))
    r5 = M.symmetricize_states(port)[0]
    batch = np.repeat(r5[None], len(M.SYM_SWEEP), axis=0)
    for k, sym in enumerate(M.SYMMETRIES.values()):
        assert (np_symmetricize_offsets(batch, sym, M.SYM_SWEEP) == sweeps["symmetricize_sweep"][k]).all(), sym
    one = np.repeat(M.cell(*M.SWEEP_CELL)[None], len(M.SHIFTS), axis=0)
    for t in range(16):
        want = np.stack([M.cell(*at.tolist()) for at in sweeps["shift_landing"][t]])
        assert (np_transform_offsets(one, t, M.SHIFTS) == want).all(), M.TRANSFORMS[t]


# ---- every mutation contradicts a recorded answer ----
def test_mutation_operands_exchanged(gold):
    """C4's transform is no involution: IntersectingOffsets(pat2, pat1) is another mask"""
    p1, p2 = sparse_pairs()
    k = IO_SYMS.index("C4")
    assert sum((np_intersecting(p2[i], p1[i], "C4") != gold["sparse_pairs"][k, i]).any() for i in range(N_SPARSE)) >= 30


def test_mutation_wrong_transform(gold):
    p1, p2 = sparse_pairs()
    for sym, wrongs in IO_WRONG.items():
        k = IO_SYMS.index(sym)
        for w in wrongs:
            mutant = dict(IO_TRANSFORM, **{sym: w})
            bad = sum((np_intersecting(p1[i], p2[i], sym, mutant) != gold["sparse_pairs"][k, i]).any()
                      for i in range(N_SPARSE))
            assert bad >= 30, (sym, w, bad)


def np_intersecting_wrong_side(pat1, pat2, sym):
    """mutation: the walked (sparser) operand is taken for the transformed one"""
    t = M.T[IO_TRANSFORM[sym]]
    if pop(pat2) < pop(pat1):
        return np_convolve(pat1, M.np_transform(pat2, t))
    return np_convolve(pat2, M.np_transform(pat1, t))


def test_mutation_transform_follows_the_walk(gold, port):
    cases = choice_cases(port)
    for k, sym in enumerate(IO_SYMS):
        if sym == "C2":
            continue    # Identity: nothing to misplace
        got = [[np_intersecting_wrong_side(x, y, sym), np_intersecting_wrong_side(y, x, sym)] for _, x, y in cases]
        bad = [(name, o) for (name, _, _), g, w in zip(cases, got, gold["choice"][k]) for o in (0, 1)
               if (g[o] != w[o]).any()]
        assert any(name.startswith("dense x") for name, _ in bad), (sym, bad)


def test_mutation_halve_odd(gold, port):
    states = halve_states(port)
    for mode in range(3):
        assert any((np_halve(s, mode, odd=True) != gold["halve"][mode, i]).any() for i, s in enumerate(states[:8]))
    # a single odd column or row vanishes, a single even one does not
    for i in range(64):
        assert gold["halve"][1, 8 + i].any() == (i % 2 == 0) and gold["halve"][0, 8 + i].any() == (i % 2 == 0)
        assert gold["halve"][2, 72 + i].any() == (i % 2 == 0) and gold["halve"][0, 72 + i].any() == (i % 2 == 0)


def test_mutation_skew_sign(gold, port):
    states = halve_states(port)
    for inverse in (False, True):
        bad = sum((np_skew(s, not inverse) != gold["skew"][int(inverse), i]).any() for i, s in enumerate(states))
        assert bad >= 100, bad
