"""CPU: the numpy definitions of tests/test_match_model.py against the
reference's recorded answers on the sharp inputs of tests/match_sharp.py
(tests/golden/match_sharp.npz), and how sharp those inputs are: every care
cell of every target, every cell of every pattern, every term, partner and
threshold of InteractionOffsets changes a recorded answer when it is lost."""
import numpy as np
import pytest

import match_sharp as S
import test_match_model as M


@pytest.fixture(scope="module")
def data(port):
    return S.fixture_data(port)


# ---- the builders -------------------------------------------------------------

def test_builders_give_the_recorded_inputs(port, data):
    assert (S.impulse_states() == data["impulse_states"]).all()
    assert list(data["patterns"]) == list(data["pattern_names"])
    others = S.sharp_others(port)
    assert list(others) == list(data["other_names"])
    assert (np.stack(list(others.values())) == data["others"]).all()
    targets = M.build_targets(port, M.fixture_data(port)["states"])
    assert list(data["near_miss"]) == [k for k in targets if k != "empty"]


def test_near_misses_are_one_flipped_care_cell(data):
    """universe 0 has every care cell right at the planted offset and, where
    anything is wanted, no other live cell; universe 1 + i differs from it in
    care cell i alone; the care cells lie across both seams wherever the
    target has two adjacent columns (rows)"""
    total = 0
    for name, (states, (dx, dy), (w, u), _) in data["near_miss"].items():
        care = M.cells(w) + M.cells(u)
        assert len(states) == 1 + len(care)
        total += len(states)
        moved_w, moved_u = M.at(w, dx, dy), M.at(u, dx, dy)
        assert ((states[0] & moved_w) == moved_w).all() and not (states[0] & moved_u).any(), name
        if w.any():
            assert (states[0] == moved_w).all(), name
        else:
            assert M.popcount(states[:1])[0] > 1024, name            # the soup
        for i, (a, b) in enumerate(care):
            diff = states[1 + i] ^ states[0]
            assert (diff == M._cells_to_pattern([(a + dx, b + dy)])).all(), (name, i)
        for axis, shift in ((0, dx), (1, dy)):
            used = {c[axis] for c in care}
            if any((c + 1) % 64 in used for c in used):
                assert {63, 0} <= {(c + shift) % 64 for c in used}, (name, axis)
    assert total == 939


def test_interaction_batch_shape(port):
    x = S.interaction_batch(port, 300)
    assert (x == S.interaction_batch(port, S.N_BATCH)[:300]).all()     # a prefix of the longest
    pop = M.popcount(x)
    assert 32 <= pop.mean() <= 64 and pop.max() < 128                  # 4096 / 128 cells of soup + about 16 in boxes
    live = M.unpack(x)
    assert (live[:, 63] & live[:, 0]).any(axis=1).sum() >= 300 // 16   # cells on both sides of the column seam
    assert (live[:, :, 63] & live[:, :, 0]).any(axis=1).sum() >= 300 // 16


# ---- the definitions equal the recording -------------------------------------------

def test_numpy_match_equals_the_reference_on_near_misses(data):
    """and the recording is what the near misses are for: the planted offset
    matches in universe 0 and in no other"""
    for name, (states, (dx, dy), (w, u), recorded) in data["near_miss"].items():
        assert (M.np_match(states, w, u) == recorded).all(), name
        hit = (recorded[:, dx] >> np.uint64(dy)) & M.U1
        assert hit[0] == 1 and not hit[1:].any(), name


def test_numpy_convolve_equals_the_reference_on_impulses(data):
    for k, (name, p) in enumerate(data["patterns"].items()):
        assert (M.np_convolve(data["impulse_states"], p) == data["convolve"][k]).all(), name


def test_numpy_interaction_offsets_equals_the_reference_on_the_batch(data):
    for k, name in enumerate(data["other_names"]):
        assert (M.np_interaction_offsets(data["batch"], data["others"][k]) == data["interaction"][k]).all(), name


def test_interaction_terms_are_the_definition(data):
    """S.Interaction with the formula BASE is np_interaction_offsets, so a
    mutant below is a mutant of the definition"""
    for k, name in enumerate(data["other_names"]):
        assert (S.Interaction(data["batch"], data["others"][k])() == M.np_interaction_offsets(
            data["batch"], data["others"][k])).all(), name


# ---- what the recording pins ------------------------------------------------------------

def test_every_removed_care_cell_changes_a_recorded_match(data):
    """the target minus one care cell differs from the reference's recorded
    masks, for every care cell of every target: it does so on that cell's
    own near miss, universe 1 + i (evaluated alone, to keep this quick)"""
    for name, (states, _, (w, u), recorded) in data["near_miss"].items():
        cw, cu = M.cells(w), M.cells(u)
        lesser = [(S.without_cell(w, a, b), u) for a, b in cw] + [(w, S.without_cell(u, a, b)) for a, b in cu]
        escaped = [(cw + cu)[i] for i, (w1, u1) in enumerate(lesser)
                   if (M.np_match(states[1 + i], w1, u1) == recorded[1 + i]).all()]
        assert not escaped, (name, escaped)


def test_every_removed_pattern_cell_changes_a_recorded_convolve(data):
    for k, (name, p) in enumerate(data["patterns"].items()):
        escaped = [(a, b) for a, b in M.cells(p)
                   if (M.np_convolve(data["impulse_states"], S.without_cell(p, a, b)) == data["convolve"][k]).all()]
        assert not escaped, (name, escaped)


def test_no_transposition_of_partner_is_an_identity():
    """A mutant is an identity on the formula when it gives the same set of
    (plane, plane) terms.  Exchanging two entries of PARTNER never does: term
    i becomes a[i] * b[PARTNER[j]], which is no term of the formula since
    PARTNER is a permutation.  That holds for j = PARTNER[i] too: exchanging
    entries 3 and 5 gives a[3] * b[3] | a[5] * b[5] for a[3] * b[5] | a[5] *
    b[3], two other convolutions and not the same two in another order.  So
    no mutant is exempt below."""
    base = set(S.BASE)
    assert len(S.mutants()) == 7 + 21 + 14
    assert not [name for name, formula in S.mutants().items() if set(formula) == base]


def test_every_mutant_differs_from_the_recorded_interaction_offsets(data):
    """each deleted term, exchanged pair of partners and moved threshold (on
    the universe's planes and on the other's) disagrees with the reference's
    recorded masks on some recorded universe with some other"""
    inter = [S.Interaction(data["batch"], o) for o in data["others"]]
    escaped = [name for name, formula in S.mutants().items()
               if all((i(formula) == data["interaction"][k]).all() for k, i in enumerate(inter))]
    assert not escaped, escaped


# ---- the large batch, on the model alone ---------------------------------------------------

# universes of interaction_batch(4097) with eater_seams whose mask a mutant
# changes, measured on the numpy model with the committed seeds
FLOORS = {
    "delete term 0": 124, "delete term 1": 4097, "delete term 2": 4079, "delete term 3": 1350,
    "delete term 4": 2039, "delete term 5": 1623, "delete term 6": 2315,
    "swap partners 0 1": 4097, "swap partners 0 2": 4082, "swap partners 0 3": 2604, "swap partners 0 4": 3918,
    "swap partners 0 5": 111, "swap partners 0 6": 3916, "swap partners 1 2": 4097, "swap partners 1 3": 2121,
    "swap partners 1 4": 4097, "swap partners 1 5": 4097, "swap partners 1 6": 4058, "swap partners 2 3": 4091,
    "swap partners 2 4": 4061, "swap partners 2 5": 2824, "swap partners 2 6": 4097, "swap partners 3 4": 3269,
    "swap partners 3 5": 4058, "swap partners 3 6": 4058, "swap partners 4 5": 4058, "swap partners 4 6": 4097,
    "swap partners 5 6": 3921,
    "universe plane 3:==4": 1350, "other plane 3:==4": 1623, "universe plane 4:>=5": 1879,
    "other plane 4:>=5": 2315, "universe plane 4:>=3": 2473, "other plane 4:>=3": 3916,
    "universe plane 5:>=3": 1612, "other plane 5:>=3": 1350, "universe plane 6:>=2": 2214,
    "other plane 6:>=2": 1898, "universe plane 1:1..2": 4058, "other plane 1:1..2": 4058,
    "universe plane 2:==3": 4084, "other plane 2:==3": 4097,
}


def test_large_batch_is_unsaturated_and_kills_every_mutant(port, data):
    """interaction_batch(4097): with every sharp other at least 90 % of the
    masks are between 5 % and 95 % full (measured: all of them, 9.8 % to
    49.7 % full), and with eater_seams every mutant changes at least 8
    universes and no fewer than measured"""
    x = S.interaction_batch(port, S.N_BATCH)
    for k, name in enumerate(data["other_names"]):
        inter = S.Interaction(x, data["others"][k])
        full = M.popcount(inter()) / 4096.0
        assert ((full >= 0.05) & (full <= 0.95)).mean() >= 0.9, name
        if name != "eater_seams":
            continue
        assert set(FLOORS) == set(S.mutants())
        changed = {m: int((inter(f) != inter()).any(axis=1).sum()) for m, f in S.mutants().items()}
        assert min(changed.values()) >= 8
        assert not {m: (c, FLOORS[m]) for m, c in changed.items() if c < FLOORS[m]}
