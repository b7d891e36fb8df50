"""CPU: a numpy restatement of FirstOn, ComponentContaining and Components
(LifeAPI.hpp:301-323, 655-676) pinned to the reference's recorded answers
(tests/golden/components.npz, inputs from tests/components_cases.py), a
restatement of the GPU kernel's own schedule (components_kernels.hpp: the fixed
networks of the three centred coronas, the exit test after the round, the hard
bounds) checked on the same cases, and mutants of the definitions that each
contradict a recorded answer.  The GPU tests use the definitions here.

With s(x, y) = bit y of word x, indices mod 64:
  Convolve(A, B)(x, y) = OR over (a, b) in B of A(x - a, y - b)
  ComponentContaining(seed, corona): result = 0, tocheck = seed; while tocheck:
      nb = tocheck.Convolve(corona) & state; tocheck = nb & ~result; result |= nb
  FirstOn: the last non-empty group of four columns, its lowest non-empty
      column, that column's lowest set row; (-1, -1) for the empty state
  Components(corona): the component of FirstCell of what remains, removed, until
      nothing remains
"""
import numpy as np
import pytest

import components_cases as C

GOLDEN = C.FIXTURE
U64 = np.uint64
ONE = U64(1)


def rotl(v, b):
    b = b % 64
    return v if b == 0 else (v << U64(b)) | (v >> U64(64 - b))


def cells_of_corona(corona):
    """(a, b) with a, b in [-32, 31]"""
    return [(x - 64 * (x > 31), y - 64 * (y > 31)) for x, y in C.to_cells(corona)]


def np_convolve(s, cells, wrap_cols=True, wrap_rows=True, mirror_x=False, mirror_y=False):
    """s (n, 64) convolved with the cells (a, b): cell (x, y) -> (x + a, y + b)"""
    out = np.zeros_like(s)
    for a, b in cells:
        a, b = (-a if mirror_x else a), (-b if mirror_y else b)
        t = rotl(s, b)
        if not wrap_rows:
            t = s << U64(b) if b >= 0 else s >> U64(-b)
        t = np.roll(t, a, axis=1)
        if not wrap_cols:
            if a > 0:
                t[:, :a] = 0
            elif a < 0:
                t[:, a:] = 0
        out |= t
    return out


def np_component_containing(states, seeds, corona, cap=None, or_seed=False, **conv):
    """(n, 64) states and seeds (or one seed), one corona"""
    states = np.atleast_2d(states)
    cells = cells_of_corona(corona)
    result = np.zeros_like(states)
    tocheck = np.broadcast_to(np.atleast_2d(seeds), states.shape).copy()
    if or_seed:
        result |= tocheck
    active = np.flatnonzero(tocheck.any(axis=1))
    rounds = 0
    while active.size and (cap is None or rounds < cap):
        nb = np_convolve(tocheck[active], cells, **conv) & states[active]
        tocheck[active] = nb & ~result[active]
        result[active] |= nb
        active = active[tocheck[active].any(axis=1)]
        rounds += 1
    return result


def np_first_on(states, quad="last", column="lowest", row="lowest"):
    """(n, 2) int32"""
    states = np.atleast_2d(states)
    out = np.full((len(states), 2), -1, np.int32)
    for u, s in enumerate(states):
        quads = [q for q in range(0, 64, 4) if s[q:q + 4].any()]
        if not quads:
            continue
        q = quads[-1] if quad == "last" else quads[0]
        cols = [x for x in range(q, q + 4) if s[x]]
        x = cols[0] if column == "lowest" else cols[-1]
        w = int(s[x])
        out[u] = (x, (w & -w).bit_length() - 1 if row == "lowest" else w.bit_length() - 1)
    return out


def np_components(states, corona, first_on=None, limit=4096, **cc):
    """per universe the list of its components in the reference's order; a
    universe whose seed's component comes out empty (the reference would not
    terminate) ends with None"""
    states = np.atleast_2d(states)
    remaining = states.copy()
    parts = [[] for _ in states]
    active = np.flatnonzero(remaining.any(axis=1))
    for _ in range(limit):
        if not active.size:
            break
        cells = np_first_on(remaining[active], **(first_on or {}))
        seeds = np.zeros((active.size, 64), U64)
        seeds[np.arange(active.size), cells[:, 0]] = ONE << cells[:, 1].astype(U64)
        comp = np_component_containing(remaining[active], seeds, corona, **cc)
        remaining[active] &= ~comp
        stuck = ~(comp & states[active]).any(axis=1)
        for k, u in enumerate(active):
            parts[u].append(None if stuck[k] else comp[k])
        active = active[~stuck]
        active = active[remaining[active].any(axis=1)]
    return parts


# ---- the kernel's own schedule (components_kernels.hpp) --------------------------

def kernel_dilate(f, kind):
    """dilate_fixed: the networks of the default corona, the 3 x 3 block and the plus"""
    p, q = np.roll(f, 1, axis=1), np.roll(f, -1, axis=1)      # columns x - 1 and x + 1
    up, dn = (lambda v: rotl(v, 1)), (lambda v: rotl(v, 63))
    if kind == "plus":
        return f | up(f) | dn(f) | p | q
    u1 = p | f | q
    if kind == "3x3":
        return u1 | up(u1) | dn(u1)
    t = u1 | np.roll(p, 1, axis=1) | np.roll(q, -1, axis=1)
    return t | up(t) | dn(t) | rotl(u1, 2) | rotl(u1, 62)


def kernel_flood(states, seeds, kind, corona, max_rounds=4096):
    """flood<KIND, U>: every universe of the group runs until all have converged,
    the exit test follows the round"""
    states = np.atleast_2d(states)
    res = np.zeros_like(states)
    front = np.broadcast_to(np.atleast_2d(seeds), states.shape).copy()
    cells = cells_of_corona(corona)
    rounds = 0
    for rounds in range(1, max_rounds + 1):
        nb = (np_convolve(front, cells) if kind == "general" else kernel_dilate(front, kind)) & states
        front = nb & ~res
        res |= nb
        if not front.any():
            break
    return res, rounds


def kernel_first_on(s):
    """first_on: the ballot of populated columns, then scalar bit scans"""
    cols = sum(1 << x for x in range(64) if s[x])
    if not cols:
        return None
    quad = (cols.bit_length() - 1) & ~3
    low = (cols >> quad) & 0xF
    x = quad + (low & -low).bit_length() - 1
    w = int(s[x])
    return x, (w & -w).bit_length() - 1


def kernel_components(s, kind, corona, max_components=4096):
    rem, parts, rounds = s.copy(), [], 0
    while len(parts) < max_components:
        cell = kernel_first_on(rem)
        if cell is None:
            break
        comp, r = kernel_flood(rem, C.from_cells([cell]), kind, corona)
        rounds = max(rounds, r)
        parts.append(comp[0])
        rem &= ~comp[0]
    return parts, rounds


def kernel_kind(name):
    return {"default": "default", "3x3": "3x3", "plus": "plus"}.get(name, "general")


# ---- fixtures ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def states(port):
    return C.states(port)


def recorded_parts(gold, states, corona):
    """name -> (count, 64) components as the reference returned them"""
    use = list(states) if corona == "default" else C.other_corona_names(states)
    ends = np.cumsum(gold["count_" + corona])
    return {n: gold["comp_" + corona][e - c:e] for n, c, e in zip(use, gold["count_" + corona], ends)}


def same_parts(got, want):
    return len(got) == len(want) and all(g is not None and (g == w).all() for g, w in zip(got, want))


def cc_seeds(states):
    return {n: C.seeds_for(states[n]) for n in C.CC_STATES}


# ---- the definitions against every recorded array -------------------------------------

def test_fixture_is_complete(gold, states):
    assert gold["first_on"].shape == (len(states), 2)
    assert gold["count_default"].shape == (len(states),)
    assert gold["cc"].shape == (len(C.CORONAS), len(C.CC_STATES), len(C.SEED_KINDS), 64)
    for corona in C.COMPONENTS_CORONAS:
        assert gold["comp_" + corona].shape == (int(gold["count_" + corona].sum()), 64)
    d = dict(zip(states, gold["count_default"].tolist()))
    assert d["lattice512"] == 512 and d["spiral"] == 1 and d["spiral_cut"] == 2 and d["empty"] == 0
    soup = [v for n, v in d.items() if n.startswith("soup")]
    assert min(soup) <= 3 and max(soup) >= 100


def test_first_on(gold, states):
    assert (np_first_on(np.stack(list(states.values()))) == gold["first_on"]).all()
    for s, want in zip(states.values(), gold["first_on"]):
        assert (kernel_first_on(s) or (-1, -1)) == tuple(want)


@pytest.mark.parametrize("corona", C.COMPONENTS_CORONAS)
def test_components(gold, states, corona):
    want = recorded_parts(gold, states, corona)
    got = np_components(np.stack([states[n] for n in want]), C.CORONAS[corona])
    for n, g in zip(want, got):
        assert same_parts(g, want[n]), (corona, n)


def test_component_containing(gold, states):
    seeds = cc_seeds(states)
    for c, corona in enumerate(C.CORONAS):
        for k, kind in enumerate(C.SEED_KINDS):
            got = np_component_containing(np.stack([states[n] for n in C.CC_STATES]),
                                          np.stack([seeds[n][kind] for n in C.CC_STATES]), C.CORONAS[corona])
            assert (got == gold["cc"][c, :, k]).all(), (corona, kind)


# ---- the kernel's schedule against every recorded array ------------------------------

@pytest.mark.parametrize("corona", C.COMPONENTS_CORONAS)
def test_kernel_schedule_components(gold, states, corona):
    """and the hard bounds are far from the longest flood and the longest list"""
    want = recorded_parts(gold, states, corona)
    longest = 0
    for n in want:
        got, rounds = kernel_components(states[n], kernel_kind(corona), C.CORONAS[corona])
        assert same_parts(got, want[n]), (corona, n)
        longest = max(longest, rounds)
    assert max(len(w) for w in want.values()) <= 4096 // 2 and longest <= 4096 // 2
    if corona == "default":
        assert longest >= 600          # the spiral


def test_kernel_schedule_component_containing(gold, states):
    seeds = cc_seeds(states)
    for c, corona in enumerate(C.CORONAS):
        for i, n in enumerate(C.CC_STATES):
            for k, kind in enumerate(C.SEED_KINDS):
                got, _ = kernel_flood(states[n], seeds[n][kind], kernel_kind(corona), C.CORONAS[corona])
                assert (got[0] == gold["cc"][c, i, k]).all(), (corona, n, kind)
    # two universes of one wave run the longer one's rounds: the extra rounds change nothing
    pair = np.stack([states["spiral"], states["six_cells"]])
    seed = np.stack([C.from_cells([(60, 0)]), C.from_cells([(33, 33)])])
    got, rounds = kernel_flood(pair, seed, "default", C.CORONAS["default"])
    assert rounds > 600 and (got[0] == states["spiral"]).all() and (got[1] == C.from_cells([(33, 33)])).all()


# ---- mutants: each contradicts recorded answers ----------------------------------------

def broken(gold, states, corona="default", names=None, corona_value=None, first_on=None, **cc):
    """the number of recorded Components cases (states of one corona) a variant gets wrong"""
    want = recorded_parts(gold, states, corona)
    names = [n for n in want if names is None or n in names]
    value = C.CORONAS[corona] if corona_value is None else corona_value
    got = np_components(np.stack([states[n] for n in names]), value, first_on=first_on, **cc)
    return sum(not same_parts(g, want[n]) for n, g in zip(names, got))


def pair_names(a, b):
    return {f"pair_{p[0]}_{s * a}_{s * b}" for p in C.PAIR_BASES for s in (1, -1)}


@pytest.mark.parametrize("cell", C.DEFAULT_CELLS)
def test_mutant_corona_cell_dropped(gold, states, cell):
    """without (a, b) the pair {p, p + (a, b)} falls apart where FirstOn starts at
    p (one of the two pairs +-(a, b) at each base, at least); without (0, 0)
    nothing has a component at all"""
    value = C.from_cells([c for c in C.DEFAULT_CELLS if c != cell])
    names = pair_names(*cell)
    assert broken(gold, states, names=names, corona_value=value) >= (len(names) if cell == (0, 0) else 1)


@pytest.mark.parametrize("cell", C.NEAR_NON_CELLS)
def test_mutant_near_cell_added(gold, states, cell):
    """with (a, b) added the pair {p, p + (a, b)} is joined where FirstOn starts at p"""
    value = C.from_cells(C.DEFAULT_CELLS + [cell])
    assert broken(gold, states, names=pair_names(*cell), corona_value=value) >= 1


# floors: the cases the reasoning in each comment names, not what the variant happens to break
FIRST_ON_MUTANTS = {
    # any state with cells in two groups of four columns: six_cells, lattice512, the two spirals, full_row,
    # row_and_col, comb, staircase (and every soup)
    "first quad": (dict(quad="first"), 8),
    # two populated columns in the last group: the pairs (20, 30) + (a, b), a in 1..3 (21 of them)
    "highest column": (dict(column="highest"), 21),
    # two rows in the chosen column: the pairs with a = 0, b != 0 at both bases (12)
    "highest row": (dict(row="highest"), 12),
}


@pytest.mark.parametrize("name", FIRST_ON_MUTANTS)
def test_mutant_first_on(gold, states, name):
    variant, floor = FIRST_ON_MUTANTS[name]
    got = np_first_on(np.stack(list(states.values())), **variant)
    assert int((got != gold["first_on"]).any(axis=1).sum()) >= floor
    # and the order of Components follows: the six cells' pieces, or the lattice's column 60, come out in another order
    assert broken(gold, states, names={"six_cells", "lattice512"}, first_on=variant) >= 1


FLOOD_MUTANTS = {
    # the pairs at (63, 63) with a in {1, 2} inside the corona cross the column seam (5 + 3), and the full row
    "no column wrap": (dict(wrap_cols=False), "default", 8),
    # the same with b in {1, 2}
    "no row wrap": (dict(wrap_rows=False), "default", 8),
    # the spiral's 612 rounds and its outer half's 300
    "round cap 64": (dict(cap=64), "default", 2),
    "round cap 256": (dict(cap=256), "default", 1),
    # (20, 30) + (1, 0) and (63, 63) + (1, 0) are joined to the right only; (0, +-1) downwards only (4 pairs)
    "mirrored in x": (dict(mirror_x=True), "right", 2),
    "mirrored in y": (dict(mirror_y=True), "down", 4),
}


@pytest.mark.parametrize("name", FLOOD_MUTANTS)
def test_mutant_flood(gold, states, name):
    variant, corona, floor = FLOOD_MUTANTS[name]
    assert broken(gold, states, corona=corona, **variant) >= floor


def test_mutant_seed_always_in_result(gold, states):
    """a seed outside the state must stay outside: the adjacent and the far seed
    of each of the six states, with the default corona alone"""
    seeds = cc_seeds(states)
    wrong = 0
    for i, n in enumerate(C.CC_STATES):
        for k, kind in enumerate(C.SEED_KINDS):
            got = np_component_containing(states[n], seeds[n][kind], C.CORONAS["default"], or_seed=True)
            wrong += bool((got[0] != gold["cc"][0, i, k]).any())
    assert list(C.CORONAS)[0] == "default" and wrong >= 12
