"""GPU: batched IntersectingOffsets / Convolve with both operands per universe,
Halve and Skew (pair_kernels.hpp) and the per-universe-offset forms of
Transform and Symmetricize (symmetry_kernels.hpp) through lifeapi_amd.hip,
bit-exact against (1) the reference's recorded outputs (tests/golden/pair.npz,
tests/golden/symmetry_sweeps.npz) and (2) the numpy definitions of
tests/test_pair_model.py, which CPU tests pin to the same fixtures; then one
property that ties IntersectingOffsets to Symmetricize on the GPU alone."""
import subprocess

import numpy as np
import pytest
import torch

import test_pair_facade as F
import test_pair_model as P
import test_symmetry_model as M
from test_gpu_match import to_dev, to_host

pytestmark = pytest.mark.gpu

RAGGED = [1, 2, 3, 5, 63, 64, 65, 4097]
OFFSET_SYMMETRIES = ("C4", "D4diag", "D2negdiagodd", "D4")      # of the 4097 batch with random offsets
OFFSET_TRANSFORMS = ("Identity", "ReflectAcrossXEven", "Rotate90")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(P.GOLDEN))


@pytest.fixture(scope="module")
def sweeps():
    return dict(np.load(M.SWEEPS))


def model(pat1, pat2, sym):
    """np_intersecting on (n, 64) batches, with each universe's sparser operand
    as Convolve's second (the one the model moves the other by, cell by cell):
    Convolve is symmetric in its operands, as the reference's recorded answers
    show (test_pair_model.py::test_operand_choice, which also pins
    np_convolve_words)"""
    p1, p2 = np.asarray(pat1).reshape(-1, 64), np.asarray(pat2).reshape(-1, 64)
    t1 = M.np_transform_batch(p1, M.T[P.IO_TRANSFORM[sym]])
    return np.stack([P.np_convolve_words(y, x) if P.pop(x) <= P.pop(y) else P.np_convolve_words(x, y)
                     for x, y in zip(t1, p2)])


@pytest.fixture(scope="module")
def ragged(port):
    """4097 pairs and their answers for the six symmetries, computed once; a
    batch of n is the first n.  Every 7th slot both operands are sparse;
    elsewhere a half-density state meets a sparse pattern, the dense one first
    in odd slots and second in even ones, so that a wave (four neighbouring
    universes) switches the walked operand between its universes; some
    operands are empty.  `sparse` (all of them small or empty) is the batch
    of the self form."""
    rng = np.random.default_rng(1830)
    dense = port.fill(4097, seed=1831)
    sparse = np.stack([P.small_pattern(rng, P.SPOTS[u % 6]) for u in range(4097)])
    other = np.stack([P.small_pattern(rng, P.SPOTS[(u // 6) % 6]) for u in range(4097)])
    u = np.arange(4097)
    a = np.where((u % 2 == 1)[:, None], dense, sparse)
    b = np.where((u % 2 == 1)[:, None], sparse, dense)
    both = u % 7 == 0
    a[both], b[both] = sparse[both], other[both]
    a[u % 31 == 5] = 0
    b[u % 31 == 6] = 0
    a[u % 97 == 9] = b[u % 97 == 9] = 0
    sparse[u % 31 == 5] = 0
    want = {sym: model(a, b, sym) for sym in P.IO_SYMS}
    want_self = {sym: model(sparse, sparse, sym) for sym in P.IO_SYMS}
    assert all((want[s][1:64] != 0).any(axis=1).sum() > 50 for s in P.IO_SYMS)
    for arr in (a, b, sparse, *want.values(), *want_self.values()):
        arr.flags.writeable = False
    return a, b, sparse, want, want_self


# ---- every golden case against the reference's recorded outputs -------------

def test_golden_cases(hip, port, gold):
    """every case of pair.npz, one launch per (call, argument)"""
    groups = {}
    for kind, arg, a, b, out in F.cases(port, gold):
        groups.setdefault((kind, arg), []).append((a, b, out))
    assert len(groups) == 6 + 16 + 3 + 2
    for (kind, arg), rows in groups.items():
        a, b, want = (np.stack(v) for v in zip(*rows))
        da, db = to_dev(a), to_dev(b)
        if kind == 0:
            got = hip.intersecting_offsets(da, arg, db)
            name = hip.SYMMETRIES[arg]
            assert (to_host(hip.intersecting_offsets(da, name, db)) == want).all(), name
        elif kind == 1:
            got = hip.convolve_pair(da, db, arg)
            assert (to_host(hip.convolve_pair(da, db, hip.TRANSFORMS[arg])) == want).all(), arg
        elif kind == 2:
            got = hip.halve(da, arg)
            assert (to_host(hip.halve(da, hip.HALVE_MODES[arg])) == want).all(), arg
            assert hip.halve(db, arg, out=db) is db and not to_host(db).any()
        else:
            got = hip.skew(da, bool(arg))
            back = hip.skew(got, not arg)
            assert (to_host(back) == a).all(), arg
        assert (to_host(got) == want).all(), (kind, arg)
        assert (to_host(da) == a).all()
        if kind >= 2:        # in place
            f = hip.halve if kind == 2 else hip.skew
            assert f(da, arg, out=da) is da and (to_host(da) == want).all(), (kind, arg, "in place")
    s = to_dev(np.zeros((2, 64), np.uint64))
    for sym in P.IO_UNDEFINED:
        with pytest.raises(hip.LifeApiError):
            hip.intersecting_offsets(s, sym)
    with pytest.raises(hip.LifeApiError):
        hip.halve(s, 3)
    with pytest.raises(hip.LifeApiError):
        hip.convolve_pair(s, s, 16)


def test_residue_sweep(hip, gold):
    """192 universes and a tail, each with its own one-cell pat1 against the
    cell (17, 42): every column fetch distance and every row rotate of the
    per-universe walk, the half swap included; then with the operands
    exchanged, against the model"""
    tail = np.stack([M.cells([c]) for c in ((17, 42), (0, 0), (63, 63))])
    pat1 = np.concatenate([P.residue_states(), tail])
    pat2 = np.repeat(M.cells([P.RESIDUE_PAT2])[None], len(pat1), axis=0)
    d1, d2 = to_dev(pat1), to_dev(pat2)
    for k, sym in enumerate(P.IO_SYMS):
        got = to_host(hip.intersecting_offsets(d1, sym, d2))
        want = np.stack([M.cell(*at.tolist()) for at in gold["residue_landing"][k]])
        assert (got[:192] == want).all(), sym
        assert (got[192:] == model(tail, pat2[192:], sym)).all(), sym
        got = to_host(hip.intersecting_offsets(d2, sym, d1))
        assert (got == model(pat2, pat1, sym)).all(), (sym, "exchanged")
    assert (to_host(d1) == pat1).all() and (to_host(d2) == pat2).all()


# ---- ragged sizes against the numpy definitions -------------------------------

@pytest.mark.parametrize("n", RAGGED)
def test_ragged_pairs(hip, ragged, n):
    """out of place (also on batches that are only 8-byte aligned), in place on
    either operand, and the self form by aliasing, out of place and in place"""
    a, b, sparse, want, want_self = ragged
    for sym in P.IO_SYMS:
        for offset8 in (False, True):
            d1, d2 = to_dev(a[:n], offset8), to_dev(b[:n], offset8)
            assert (to_host(hip.intersecting_offsets(d1, sym, d2)) == want[sym][:n]).all(), (sym, offset8)
            assert (to_host(d1) == a[:n]).all() and (to_host(d2) == b[:n]).all()
        assert hip.intersecting_offsets(d1, sym, d2, out=d1) is d1
        assert (to_host(d1) == want[sym][:n]).all() and (to_host(d2) == b[:n]).all(), (sym, "in place on pat1")
        d1 = to_dev(a[:n])
        assert hip.intersecting_offsets(d1, sym, d2, out=d2) is d2
        assert (to_host(d2) == want[sym][:n]).all() and (to_host(d1) == a[:n]).all(), (sym, "in place on pat2")
        s = to_dev(sparse[:n])
        assert (to_host(hip.intersecting_offsets(s, sym)) == want_self[sym][:n]).all(), (sym, "self")
        assert (to_host(hip.intersecting_offsets(s, sym, s)) == want_self[sym][:n]).all(), (sym, "self, aliased")
        assert (to_host(s) == sparse[:n]).all()
        assert hip.intersecting_offsets(s, sym, out=s) is s
        assert (to_host(s) == want_self[sym][:n]).all(), (sym, "self, in place")


def test_operand_order_is_the_same_answer(hip, ragged):
    """C2 transforms nothing, so exchanging the operands exchanges only which
    one each wave walks"""
    a, b, _, want, _ = ragged
    d1, d2 = to_dev(a), to_dev(b)
    assert (to_host(hip.intersecting_offsets(d2, "C2", d1)) == want["C2"]).all()
    assert (to_host(hip.convolve_pair(d1, d2)) == want["C2"]).all()
    assert (to_host(hip.convolve_pair(d2, d1, "Identity")) == want["C2"]).all()
    # two half-density operands, and the dense self-pair: the long walk (some 2000 cells)
    x, y = a[1:10:2], b[2:11:2]
    for sym in ("C2", "D2negdiagodd"):
        assert (to_host(hip.intersecting_offsets(to_dev(x), sym, to_dev(y))) == model(x, y, sym)).all(), sym
        assert (to_host(hip.intersecting_offsets(to_dev(x), sym)) == model(x, x, sym)).all(), (sym, "self")


def test_side_stream(hip, ragged):
    a, b, sparse, want, want_self = ragged
    side = torch.cuda.Stream()
    d1, d2, s = to_dev(a), to_dev(b), to_dev(sparse)
    offsets = torch.zeros((4097, 2), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        io = hip.intersecting_offsets(d1, "C4", d2, stream=side)
        io_self = hip.intersecting_offsets(s, "D2diagodd", stream=side)
        hv, sk = hip.halve(s, 0, stream=side), hip.skew(s, stream=side)
        sy = hip.symmetricize_offsets(s, "C2", offsets, stream=side)
        tr = hip.transform_offsets(s, "Rotate90", offsets, stream=side)
    side.synchronize()
    assert (to_host(io) == want["C4"]).all() and (to_host(io_self) == want_self["D2diagodd"]).all()
    assert (to_host(hv)[:65] == np.stack([P.np_halve(x, 0) for x in sparse[:65]])).all()
    assert (to_host(sk)[:65] == np.stack([P.np_skew(x) for x in sparse[:65]])).all()
    assert (to_host(sy) == to_host(hip.symmetricize(s, "C2"))).all()
    assert (to_host(tr) == to_host(hip.transform(s, "Rotate90"))).all()


@pytest.mark.parametrize("device,shards", [(0, None), (-1, 3)])
def test_host_forms(hip, ragged, monkeypatch, device, shards):
    if shards:
        monkeypatch.setenv("LIFEAPI_HOST_SHARDS", str(shards))
    a, b, sparse, want, want_self = ragged
    for sym in ("C4", "D2AcrossX"):
        assert (hip.intersecting_offsets_host(a, sym, b, device=device) == want[sym]).all(), sym
        assert (hip.intersecting_offsets_host(sparse, sym, device=device) == want_self[sym]).all(), sym
    y = a.copy()
    assert hip.intersecting_offsets_host(y, "D2diagodd", b, out=y, device=device) is y          # in place
    assert (y == want["D2diagodd"]).all()
    assert (hip.convolve_pair_host(b, a, "ReflectAcrossX", device=device) == want["D2AcrossY"]).all()
    assert (hip.convolve_pair_host(sparse, device=device) == want_self["C2"]).all()
    rng = np.random.default_rng(1832)
    offsets = rng.integers(-200, 201, size=(4097, 2)).astype(np.int32)
    d, o = to_dev(sparse), torch.from_numpy(offsets).cuda()
    assert (hip.symmetricize_offsets_host(sparse, "D4diag", offsets, device=device) ==
            to_host(hip.symmetricize_offsets(d, "D4diag", o))).all()
    assert (hip.transform_offsets_host(sparse, "Rotate270Even", offsets, device=device) ==
            to_host(hip.transform_offsets(d, "Rotate270Even", o))).all()
    for mode in range(3):
        assert (hip.halve_host(a, mode, device=device) == to_host(hip.halve(to_dev(a), mode))).all(), mode
    for inverse in (False, True):
        assert (hip.skew_host(a, inverse, device=device) == to_host(hip.skew(to_dev(a), inverse))).all(), inverse
    assert (hip.halve_host(a[:136], 0, device=device) == np.stack([P.np_halve(x, 0) for x in a[:136]])).all()
    assert (hip.skew_host(a[:136], True, device=device) == np.stack([P.np_skew(x, True) for x in a[:136]])).all()


@pytest.mark.parametrize("n", RAGGED)
def test_ragged_halve_and_skew(hip, ragged, n):
    a = ragged[0]
    m = min(n, 136)                                       # the model's rows; the rest against the first launch
    for offset8 in (False, True):
        d = to_dev(a[:n], offset8)
        for mode in range(3):
            got = to_host(hip.halve(d, mode))
            assert (got[:m] == np.stack([P.np_halve(x, mode) for x in a[:m]])).all(), (mode, offset8)
            assert (got[:, 32:] == got[:, :32]).all() if mode != 2 else True
            assert ((got >> np.uint64(32)) == (got & np.uint64(0xFFFFFFFF))).all() if mode != 1 else True
        for inverse in (False, True):
            got = hip.skew(d, inverse)
            assert (to_host(got)[:m] == np.stack([P.np_skew(x, inverse) for x in a[:m]])).all(), (inverse, offset8)
            assert (to_host(hip.skew(got, not inverse, out=got)) == a[:n]).all(), (inverse, offset8)
        assert (to_host(d) == a[:n]).all()


# ---- an offset per universe -----------------------------------------------------

def offsets_dev(offsets):
    return torch.from_numpy(np.asarray(offsets, np.int64).astype(np.int32).reshape(-1, 2)).cuda()


def test_symmetricize_sweep_in_one_launch(hip, port, sweeps):
    """the recorded 282-offset sweep of the R-pentomino, universe u carrying
    offset u, for each of the nine symmetries; then in place"""
    r5 = M.symmetricize_states(port)[0]
    batch = np.repeat(r5[None], len(M.SYM_SWEEP), axis=0)
    o = offsets_dev(M.SYM_SWEEP)
    for k, (name, sym) in enumerate(M.SYMMETRIES.items()):
        d = to_dev(batch)
        assert (to_host(hip.symmetricize_offsets(d, sym, o)) == sweeps["symmetricize_sweep"][k]).all(), name
        assert (to_host(d) == batch).all()
        assert hip.symmetricize_offsets(d, name, o, out=d) is d
        assert (to_host(d) == sweeps["symmetricize_sweep"][k]).all(), (name, "in place")
    for sym in M.UNDEFINED_SYMMETRIES:
        with pytest.raises(hip.LifeApiError):
            hip.symmetricize_offsets(d, sym, o)


def test_shift_sweep_in_one_launch(hip, sweeps):
    """the landing of the cell (17, 42) under every transform at every shift
    (the residues of dx, dy and both, and moves far out of range), universe u
    carrying shift u"""
    batch = np.repeat(M.cell(*M.SWEEP_CELL)[None], len(M.SHIFTS), axis=0)
    o = offsets_dev(M.SHIFTS)
    d = to_dev(batch)
    for t in range(16):
        want = np.stack([M.cell(*at.tolist()) for at in sweeps["shift_landing"][t]])
        assert (to_host(hip.transform_offsets(d, t, o)) == want).all(), M.TRANSFORMS[t]
        e = to_dev(batch, offset8=True)
        assert hip.transform_offsets(e, M.TRANSFORMS[t], o, out=e) is e and (to_host(e) == want).all(), (t, "in place")
    assert (to_host(d) == batch).all()


def test_random_offsets_against_the_model(hip, ragged):
    """4097 universes (half density and sparse), offsets in [-200, 200]"""
    a = ragged[0]
    rng = np.random.default_rng(1833)
    offsets = rng.integers(-200, 201, size=(4097, 2))
    d, o = to_dev(a), offsets_dev(offsets)
    for name in OFFSET_SYMMETRIES:
        got = to_host(hip.symmetricize_offsets(d, name, o))
        assert (got == P.np_symmetricize_offsets(a, M.SYMMETRIES[name], offsets)).all(), name
    for name in OFFSET_TRANSFORMS:
        got = to_host(hip.transform_offsets(d, name, o))
        assert (got == P.np_transform_offsets(a, M.T[name], offsets)).all(), name
    assert (to_host(d) == a).all() and (o.cpu().numpy() == offsets).all()


@pytest.mark.parametrize("n", RAGGED)
def test_equal_offsets_are_the_single_offset_call(hip, ragged, n):
    """bit for bit, every symmetry and transform, at an offset whose D4diag
    halves truncate and one beyond a turn"""
    a = ragged[0]
    d = to_dev(a[:n])
    for dx, dy in ((7, -3), (-70, 129)):
        o = offsets_dev([(dx, dy)] * n)
        for name in M.SYMMETRIES:
            assert torch.equal(hip.symmetricize_offsets(d, name, o), hip.symmetricize(d, name, dx, dy)), (name, dx, dy)
        for t in range(16):
            assert torch.equal(hip.transform_offsets(d, t, o), hip.transform(d, t, dx, dy)), (t, dx, dy)


# ---- IntersectingOffsets is where Symmetricize overlaps ---------------------------

def test_offsets_in_the_mask_are_the_overlapping_ones(hip, ragged):
    """for C2 and the four D2 symmetries, on sparse self-pairs: bit o of
    IntersectingOffsets(A, sym) is set iff Symmetricize(A, sym, o) has fewer
    than twice A's cells (A and its image share a cell).  Per universe four
    offsets of its mask and four outside it, in one launch."""
    sparse = ragged[2]
    keep = np.flatnonzero(sparse.any(axis=1))[:256]
    x = sparse[keep]
    d = to_dev(x)
    pops = hip.pop(d).cpu().numpy()
    rng = np.random.default_rng(1834)
    for sym in ("C2", "D2AcrossX", "D2AcrossY", "D2diagodd", "D2negdiagodd"):
        mask = to_host(hip.intersecting_offsets(d, sym))
        offsets, inside = [], []
        for m in mask:
            g = M.unpack(m)
            on, off = np.argwhere(g), np.argwhere(~g)
            assert len(on) >= 1 and len(off) >= 4
            pick = np.concatenate([on[rng.integers(0, len(on), size=4)], off[rng.integers(0, len(off), size=4)]])
            offsets.append(pick)
            inside.append([True] * 4 + [False] * 4)
        offsets, inside = np.concatenate(offsets), np.concatenate(inside)
        got = hip.pop(hip.symmetricize_offsets(to_dev(np.repeat(x, 8, axis=0)), sym, offsets_dev(offsets))).cpu().numpy()
        assert ((got < 2 * np.repeat(pops, 8)) == inside).all(), sym
        assert (got[~inside] == 2 * np.repeat(pops, 8)[~inside]).all(), sym


# ---- the C++ facade ---------------------------------------------------------------

def test_pair_batch_cpp(tmp_path, port, gold):
    """tests/cpp/pair_batch_test.cpp: IntersectingOffsetsBatch (both forms),
    ConvolvePairBatch, HalveBatch, SkewBatch and the per-universe-offset
    overloads of TransformBatch and SymmetricizeBatch against the golden file
    and the facade's CPU members"""
    exe = F.build("pair_batch_test", gpu=True)
    path = tmp_path / "cases.bin"
    F.write_cases(path, port, gold)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "pair_batch_test: ok" in r.stdout
