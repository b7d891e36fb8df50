"""GPU: batched Transform / Move, Symmetricize, XYBounds and SymmetryOrbit
(symmetry_kernels.hpp) through lifeapi_amd.hip, bit-exact against (1) the
reference's recorded outputs (tests/golden/symmetry.npz) and (2) the numpy
definitions of tests/test_symmetry_model.py, which CPU tests pin to the same
fixture; then group properties on the GPU alone.

The sweeps (tests/golden/symmetry_sweeps.npz and the builders of the model's
file) run every residue of a shift through k_transform, every offset of two
lines through k_symmetricize's ds_bpermute path, every pair of populated
columns and rows through k_bounds and the orbit's per-image maps, and a state
of every stabiliser subgroup of D4 through the orbit's comparison."""
import os
import subprocess

import numpy as np
import pytest
import torch

import test_symmetry_model as M
from test_gpu_match import to_dev, to_host

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RAGGED = [1, 2, 3, 5, 63, 64, 65, 4097]
MOVE = (13, -27)                                   # the ragged batches' (dx, dy)
# every symmetry Symmetricize defines, one offset each: odd x - y for D4diag, components below -64 and at 64
RAGGED_SYMMETRIES = {"C4": (7, -3), "D4diag": (-40, 13), "D2AcrossX": (5, 6), "C1": (3, 4), "D2AcrossY": (-70, 9),
                     "D2negdiagodd": (12, -65), "D2diagodd": (-1, 33), "C2": (31, -32), "D4": (-67, 64)}
assert set(RAGGED_SYMMETRIES) == set(M.SYMMETRIES)
PLANTED = 60                                       # the every-7th slot the stabiliser states start at


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(M.GOLDEN))


@pytest.fixture(scope="module")
def ragged(port):
    """4097 seeded universes, alternating full and quarter density, every 7th
    a small pattern of the golden's list, some of them on the window's seam,
    or (slots 60 .. 100, which repeat slots 0 .. 40) a state of each
    stabiliser subgroup of D4; and the numpy definitions' answers, computed
    once.  A batch of n is the first n of them."""
    x = port.fill(4097, seed=3030)
    x[1::2] &= port.fill(4097, seed=3031)[1::2] & port.fill(4097, seed=3032)[1::2]
    bases = M.orbit_bases(port)[:len(M.PATTERNS)]
    spots = ((0, 0), (30, 31), (-2, -1), (31, 5), (7, 30), (40, 50))
    for k, u in enumerate(range(0, 4097, 7)):
        x[u] = M.np_transform(bases[k % len(bases)], 0, *spots[(k // len(bases)) % len(spots)])
    planted = M.stabiliser_states()
    x[7 * PLANTED:7 * (PLANTED + len(planted)):7] = planted
    want = {("transform", t): M.np_transform_batch(x, t, *MOVE) for t in range(16)}
    for name, off in RAGGED_SYMMETRIES.items():
        want["symmetricize", name] = M.np_symmetricize(x, M.SYMMETRIES[name], *off)
    want["bounds"] = M.np_bounds_batch(x)
    want["images"], want["mask"] = M.np_orbit_batch(x)
    assert set(M.STABILISER_MASKS) <= set(want["mask"].tolist()), sorted(set(want["mask"].tolist()))
    for a in (x, *want.values()):
        a.flags.writeable = False
    return x, want


# ---- every golden case against the reference's recorded outputs -------------

def test_golden_transform(hip, port, gold):
    states = M.transform_states(port)
    s = to_dev(states)
    for t in range(16):
        assert (to_host(hip.transform(s, t)) == gold["transform"][t]).all(), M.TRANSFORMS[t]
        assert (to_host(hip.transform(s, M.TRANSFORMS[t])) == gold["transform"][t]).all()
        for m, (dx, dy) in enumerate(M.MOVES):
            got = to_host(hip.transform(s[:2], t, dx, dy))
            assert (got == gold["transform_move"][t][m]).all(), (M.TRANSFORMS[t], dx, dy)
    assert (to_host(s) == states).all()


def test_golden_symmetricize(hip, port, gold):
    states = M.symmetricize_states(port)
    s = to_dev(states)
    for k, (name, sym) in enumerate(M.SYMMETRIES.items()):
        for o, (dx, dy) in enumerate(M.OFFSETS):
            assert (to_host(hip.symmetricize(s, sym, dx, dy)) == gold["symmetricize"][k][:, o]).all(), (name, dx, dy)
        assert (to_host(hip.symmetricize(s, name, 7, -3)) == gold["symmetricize"][k][:, 1]).all(), name
    assert (to_host(s) == states).all()
    for sym in M.UNDEFINED_SYMMETRIES:
        with pytest.raises(hip.LifeApiError):
            hip.symmetricize(s, sym)


def test_golden_bounds_and_orbit(hip, gold):
    """images + mask, mask only, images only"""
    states = gold["orbit_states"].reshape(-1, 64)
    s = to_dev(states)
    assert (to_host(hip.bounds(s)).view(np.int32) == gold["bounds"].reshape(-1, 4)).all()
    images, mask = hip.symmetry_orbit(s)
    assert (to_host(images) == gold["orbit_images"].reshape(-1, 8, 64)).all()
    assert (mask.cpu().numpy() == gold["orbit_mask"].ravel()).all()
    assert (hip.symmetry_orbit(s, images=False).cpu().numpy() == gold["orbit_mask"].ravel()).all()
    assert (to_host(hip.symmetry_orbit(s, first=False)) == gold["orbit_images"].reshape(-1, 8, 64)).all()
    assert (to_host(s) == states).all()


# ---- ragged sizes against the numpy definitions -------------------------------

@pytest.mark.parametrize("n", RAGGED)
def test_ragged_transform(hip, ragged, n):
    """out of place, in place, and on a batch that is only 8-byte aligned"""
    x, want = ragged
    for t in range(16):
        for offset8 in (False, True):
            s = to_dev(x[:n], offset8)
            assert (to_host(hip.transform(s, t, *MOVE)) == want["transform", t][:n]).all(), (t, offset8)
            assert (to_host(s) == x[:n]).all()
            assert hip.transform(s, t, *MOVE, out=s) is s
            assert (to_host(s) == want["transform", t][:n]).all(), (t, offset8, "in place")


@pytest.mark.parametrize("n", RAGGED)
def test_ragged_symmetricize(hip, ragged, n):
    x, want = ragged
    for name, off in RAGGED_SYMMETRIES.items():
        for offset8 in (False, True):
            s = to_dev(x[:n], offset8)
            assert (to_host(hip.symmetricize(s, name, *off)) == want["symmetricize", name][:n]).all(), (name, offset8)
            assert (to_host(s) == x[:n]).all()
            assert hip.symmetricize(s, name, *off, out=s) is s
            assert (to_host(s) == want["symmetricize", name][:n]).all(), (name, offset8, "in place")


@pytest.mark.parametrize("n", RAGGED)
def test_ragged_bounds_and_orbit(hip, ragged, n):
    x, want = ragged
    for offset8 in (False, True):
        s = to_dev(x[:n], offset8)
        assert (to_host(hip.bounds(s)).view(np.int32) == want["bounds"][:n]).all(), offset8
        images, mask = hip.symmetry_orbit(s)
        assert (mask.cpu().numpy() == want["mask"][:n]).all(), offset8
        assert (to_host(images) == want["images"][:n]).all(), offset8
        assert (hip.symmetry_orbit(s, images=False).cpu().numpy() == want["mask"][:n]).all(), offset8
        assert (to_host(s) == x[:n]).all()


def test_mask_only_touches_nothing_else(hip, ragged):
    """with d_images NULL nothing but the n mask bytes is written, and bounds
    writes its 4 n numbers alone: the guard bytes around both stay"""
    x, want = ragged
    n, guard = 4097, 64
    s = to_dev(x)
    buf = torch.full((n + 2 * guard,), 0x5A, dtype=torch.uint8, device="cuda")
    hip._check(hip.lib.lifeapi_symmetry_orbit_batch_dev(s.data_ptr(), None, buf.data_ptr() + guard, n,
                                                        hip._stream(None)))
    got = buf.cpu().numpy()
    assert (got[:guard] == 0x5A).all() and (got[-guard:] == 0x5A).all() and (got[guard:-guard] == want["mask"]).all()
    b = torch.full((4 * n + 2 * guard,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    hip._check(hip.lib.lifeapi_bounds_batch_dev(s.data_ptr(), b.data_ptr() + 4 * guard, n, hip._stream(None)))
    got = b.cpu().numpy()
    assert (got[:guard] == 0x5A5A5A5A).all() and (got[-guard:] == 0x5A5A5A5A).all()
    assert (got[guard:-guard].reshape(-1, 4) == want["bounds"]).all()
    assert (to_host(s) == x).all()


def test_side_stream(hip, ragged):
    x, want = ragged
    side = torch.cuda.Stream()
    s = to_dev(x)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        tr = hip.transform(s, 6, *MOVE, stream=side)
        sy = hip.symmetricize(s, "C4", *RAGGED_SYMMETRIES["C4"], stream=side)
        bo = hip.bounds(s, stream=side)
        images, mask = hip.symmetry_orbit(s, stream=side)
    side.synchronize()
    assert (to_host(tr) == want["transform", 6]).all()
    assert (to_host(sy) == want["symmetricize", "C4"]).all()
    assert (to_host(bo).view(np.int32) == want["bounds"]).all()
    assert (to_host(images) == want["images"]).all() and (mask.cpu().numpy() == want["mask"]).all()


@pytest.mark.parametrize("device,shards", [(0, None), (-1, 3)])
def test_host_forms(hip, ragged, monkeypatch, device, shards):
    if shards:
        monkeypatch.setenv("LIFEAPI_HOST_SHARDS", str(shards))
    x, want = ragged
    for t in (0, 1, 6, 14):
        assert (hip.transform_host(x, t, *MOVE, device=device) == want["transform", t]).all(), t
    y = x.copy()
    assert hip.transform_host(y, 6, *MOVE, out=y, device=device) is y                 # in place
    assert (y == want["transform", 6]).all()
    for name, off in RAGGED_SYMMETRIES.items():
        assert (hip.symmetricize_host(x, name, *off, device=device) == want["symmetricize", name]).all(), name
    assert (hip.bounds_host(x, device=device) == want["bounds"]).all()
    images, mask = hip.symmetry_orbit_host(x, device=device)
    assert (images == want["images"]).all() and (mask == want["mask"]).all()
    assert (hip.symmetry_orbit_host(x, images=False, device=device) == want["mask"]).all()
    assert (hip.symmetry_orbit_host(x, first=False, device=device) == want["images"]).all()


# ---- the sweeps: every residue, offset, box and stabiliser -----------------------

@pytest.fixture(scope="module")
def sweeps():
    return dict(np.load(M.SWEEPS))


@pytest.fixture(scope="module")
def five(port):
    """one wave's group of four and a tail of one: a full-density state, one
    ANDed down to 1/8, the cell (17, 42), a glider across rows 31 | 32 and
    columns 31 | 32, and the empty state"""
    eighth = port.fill(1, seed=5051) & port.fill(1, seed=5052) & port.fill(1, seed=5053)
    glider = M.np_transform(port.parse(M.PATTERNS["glider"]), 0, 30, 31)
    x = np.stack([port.fill(1, seed=5050)[0], eighth[0], M.cell(*M.SWEEP_CELL), glider, np.zeros(64, np.uint64)])
    x.flags.writeable = False
    return x


def first_difference(got, want, cases):
    bad = np.argwhere((got != want).reshape(len(cases), -1).any(axis=1))
    return None if len(bad) == 0 else (len(bad), cases[int(bad[0][0])])


def test_transform_every_residue(hip, five, sweeps):
    """every transform at every residue of dx, of dy and of both, and at moves
    far out of range: each launch writes its slice of one buffer, which is
    compared once.  The single cell must land where the reference put it, the
    other four universes where the model does.  In place at the residues
    around the half swap and at both ends."""
    cases = [(t, dx, dy) for t in range(16) for dx, dy in M.SHIFTS]
    want = np.stack([M.np_transform_batch(five, *c) for c in cases])
    for (t, dx, dy), w, at in zip(cases, want, sweeps["shift_landing"].reshape(-1, 2)):
        assert (w[2] == M.cell(*at.tolist())).all(), (M.TRANSFORMS[t], dx, dy)      # the model is the recording
    s = to_dev(five)
    out = torch.empty((len(cases), 5, 64), dtype=torch.int64, device="cuda")
    for k, (t, dx, dy) in enumerate(cases):
        hip.transform(s, t, dx, dy, out=out[k])
    assert first_difference(to_host(out), want, cases) is None
    assert (to_host(s) == five).all()
    again = [k for k, (t, dx, dy) in enumerate(cases)
             if any((dx, dy) == sweep[j] for sweep in M.SHIFT_SWEEPS.values() for j in M.IN_PLACE_K)]
    assert len(again) == 16 * 3 * len(M.IN_PLACE_K)
    out = s.unsqueeze(0).repeat(len(again), 1, 1)
    for k, v in zip(again, out.unbind(0)):
        assert hip.transform(v, *cases[k], out=v) is v
    assert first_difference(to_host(out), want[again], [cases[k] for k in again]) is None


def test_symmetricize_every_offset(hip, port, five, sweeps):
    """the 8 symmetries that do something at (dx, 13), dx = -70 .. 70, and at
    (-40, dy), dy = -70 .. 70, on the five universes and, sixth, the moved
    R-pentomino the reference was recorded on: that one is compared with the
    recording, the rest with the model"""
    r5 = M.symmetricize_states(port)[0]
    x = np.concatenate([five, r5[None]])
    names = [name for name in M.SYMMETRIES if name != "C1"]
    cases = [(name, dx, dy) for name in names for dx, dy in M.SYM_SWEEP]
    want = np.stack([M.np_symmetricize(x, M.SYMMETRIES[name], dx, dy) for name, dx, dy in cases])
    recorded = np.stack([sweeps["symmetricize_sweep"][list(M.SYMMETRIES).index(name)] for name in names])
    want[:, 5] = recorded.reshape(-1, 64)
    s = to_dev(x)
    out = torch.empty((len(cases), 6, 64), dtype=torch.int64, device="cuda")
    for k, (name, dx, dy) in enumerate(cases):
        hip.symmetricize(s, name, dx, dy, out=out[k])
    assert first_difference(to_host(out), want, cases) is None
    assert (to_host(s) == x).all()


def test_bounds_and_orbit_extreme_pairs(hip, sweeps):
    """every pair of populated columns and every pair of populated rows: the
    bounds and the masks against the recording, the images (two cells each)
    against the model; and the first 8191 from a buffer that is only 8-byte
    aligned"""
    x = M.pair_states()
    want_images, want_mask = M.np_orbit_batch(x)
    assert (want_mask == sweeps["pair_mask"]).all()
    for n, offset8 in ((8192, False), (8191, True)):
        s = to_dev(x[:n], offset8)
        assert (to_host(hip.bounds(s)).view(np.int32) == sweeps["pair_bounds"][:n]).all(), offset8
        images, mask = hip.symmetry_orbit(s)
        assert (mask.cpu().numpy() == sweeps["pair_mask"][:n]).all(), offset8
        assert (to_host(images) == want_images[:n]).all(), offset8
        assert (hip.symmetry_orbit(s, images=False).cpu().numpy() == sweeps["pair_mask"][:n]).all(), offset8
        assert (to_host(s) == x[:n]).all()


def test_orbit_every_stabiliser(hip, sweeps):
    """a state for each of the 10 stabiliser subgroups at three places, the 9
    symmetricized patterns, and the two frames whose images differ in one half
    only, against the recording; then each of them at either place of a wave's
    two universes, next to the empty state"""
    x = M.orbit_sweep_states()
    n = len(x)
    for order in ("once", "paired"):
        if order == "once":
            at = np.arange(n)
            batch = x
        else:   # s, empty, empty, s
            at = 4 * np.arange(n)
            batch = np.zeros((4 * n, 64), np.uint64)
            batch[at] = batch[at + 3] = x
        s = to_dev(batch)
        images, mask = hip.symmetry_orbit(s)
        images, mask = to_host(images), mask.cpu().numpy()
        only = hip.symmetry_orbit(s, images=False).cpu().numpy()
        bounds = to_host(hip.bounds(s)).view(np.int32)
        for k in ((0,) if order == "once" else (0, 3)):
            assert (mask[at + k] == sweeps["orbit_mask"]).all(), (order, k)
            assert (only[at + k] == sweeps["orbit_mask"]).all(), (order, k)
            assert (images[at + k] == sweeps["orbit_images"]).all(), (order, k)
            assert (bounds[at + k] == sweeps["orbit_bounds"]).all(), (order, k)
        if order == "paired":
            for k in (1, 2):
                assert (mask[at + k] == 1).all() and (only[at + k] == 1).all() and (images[at + k] == 0).all()
                assert (bounds[at + k] == -1).all()
        assert (to_host(s) == batch).all()


# ---- the order book ---------------------------------------------------------------

@pytest.fixture(scope="module")
def tune(hip):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools", "tune"))
    import tune_hip
    return tune_hip


@pytest.mark.parametrize("case", ["transform", "transform_transposing", "symmetricize", "orbit_images"])
def test_output_batch_recorded_as_written_forward(tune, hip, case):
    """tests/test_gpu_match.py's check for these writers: a batch the order
    book holds as written in reverse is held as written forward once one of
    them has rewritten it, so the next order-keyed reader of that extent reverses"""
    n = 4096
    per = 8 * 512 if case == "orbit_images" else 512
    src = torch.zeros(n * 16 * 64, dtype=torch.int64, device="cuda").data_ptr()  # (the book never reads memory)
    y = torch.zeros((n, 64), dtype=torch.int64, device="cuda")
    out = torch.zeros((n, per // 8), dtype=torch.int64, device="cuda")
    first = torch.zeros(n, dtype=torch.uint8, device="cuda")
    write = {"transform": lambda: hip.transform(y, 1, 3, 4, out=out),
             "transform_transposing": lambda: hip.transform(y, 6, 3, 4, out=out),
             "symmetricize": lambda: hip.symmetricize(y, "C4", 3, 4, out=out),
             "orbit_images": lambda: hip._check(hip.lib.lifeapi_symmetry_orbit_batch_dev(
                 y.data_ptr(), out.data_ptr(), first.data_ptr(), n, hip._stream(None)))}[case]
    nbytes = n * per
    tune.order_note(src, nbytes)
    assert tune.order_probe(src, out.data_ptr(), nbytes) is True     # recorded as written in reverse
    write()
    torch.cuda.synchronize()
    assert tune.order_probe(out.data_ptr(), src + nbytes, nbytes) is True   # rewritten forward: its reader reverses


def test_mask_and_bounds_record_no_batch(tune, hip):
    """bounds and the mask-only orbit write no batch: the book's entry for the states stays"""
    n = 4096
    y = torch.zeros((n, 64), dtype=torch.int64, device="cuda")
    src = torch.zeros(n * 16 * 64, dtype=torch.int64, device="cuda").data_ptr()
    tune.order_note(src, n * 512)
    assert tune.order_probe(src, y.data_ptr(), n * 512) is True      # y recorded as written in reverse
    hip.bounds(y)
    hip.symmetry_orbit(y, images=False)
    torch.cuda.synchronize()
    assert tune.order_probe(y.data_ptr(), src + 8 * n * 512, n * 512) is False   # still: its reader runs forward


# ---- group properties, on the GPU alone ------------------------------------------

INVERSE = {5: 7, 6: 8, 7: 5, 8: 6}     # TransformInverse (Symmetry.hpp:47-55); the rest are involutions


def test_group_properties(hip, port):
    x = port.fill(4097, seed=4040)
    s = to_dev(x)
    for t in range(16):
        back = hip.transform(hip.transform(s, t), INVERSE.get(t, t))
        assert torch.equal(back, s), M.TRANSFORMS[t]
    r = s
    for _ in range(4):
        r = hip.transform(r, "Rotate90")
    assert torch.equal(r, s)
    assert not torch.equal(hip.transform(hip.transform(s, "Rotate90"), "Rotate90"), s)
    stepped = hip.step(s)
    for t in range(16):
        assert torch.equal(hip.transform(stepped, t, *MOVE), hip.step(hip.transform(s, t, *MOVE))), M.TRANSFORMS[t]
    assert (to_host(s) == x).all()


# ---- the C++ facade ---------------------------------------------------------------

def test_symmetry_batch_cpp(tmp_path, port, gold):
    """tests/cpp/symmetry_batch_test.cpp: TransformBatch (both forms),
    SymmetricizeBatch, XYBoundsBatch, SymmetryOrbitRepresentativesBatch and
    SymmetryOrbitBatch on 65 universes against the golden file"""
    import test_symmetry_facade as F
    exe = F.build("symmetry_batch_test", gpu=True)
    path = tmp_path / "cases.bin"
    F.write_cases(path, port, gold)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
