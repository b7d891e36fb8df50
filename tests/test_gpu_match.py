"""GPU: batched Match, Convolve and InteractionOffsets (match_kernels.hpp)
through lifeapi_amd.hip, bit-exact against (1) the reference's recorded
outputs (tests/golden/match.npz, and tests/golden/match_sharp.npz on the
sharp inputs of tests/match_sharp.py: near misses, impulses, sparse soups
with clusters) and (2) the numpy definitions of tests/test_match_model.py,
which CPU tests pin to the same fixtures."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import match_sharp as S
import test_match_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "tune"))

RAGGED = [1, 2, 3, 5, 63, 64, 65, 4097]


def to_dev(a: np.ndarray, offset8: bool = False) -> torch.Tensor:
    """(n, 64) device copy, 16-byte aligned or (offset8) only 8-byte aligned:
    a view offset by one word"""
    a = np.ascontiguousarray(a).view(np.int64).reshape(-1)
    t = torch.empty(a.size + 1, dtype=torch.int64, device="cuda")
    t = t[1:] if offset8 else t[:-1]
    assert t.data_ptr() % 16 == (8 if offset8 else 0)
    t.copy_(torch.from_numpy(a.copy()))
    return t.view(-1, 64)


def to_host(t: torch.Tensor) -> np.ndarray:
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64 if t.dtype == torch.int64 else np.uint32)


@pytest.fixture(scope="module")
def data(port):
    return M.fixture_data(port)


@pytest.fixture(scope="module")
def ragged(port):
    """4097 seeded universes (full density, every other one quarter density),
    three targets, a pattern and an `other`, and the numpy definitions'
    answers, computed once; a batch of n is the first n of them"""
    x = port.fill(4097, seed=2024)
    x[1::2] &= port.fill(4097, seed=2025)[1::2]
    t = M.build_targets(port, x)
    targets = {k: t[k] for k in ("block_ring", "glider_seams", "care8_seams")}
    assert len(M.cells(targets["care8_seams"][0] | targets["care8_seams"][1])) == 8
    pattern, other = M.build_patterns(port)["3x3"], M.build_others(port)["eater_seams"]
    want = {k: M.np_match(x, w, u) for k, (w, u) in targets.items()}
    want["convolve"] = M.np_convolve(x, pattern)
    want["interaction"] = M.np_interaction_offsets(x, other)
    assert all(0 < int(M.popcount(v).sum()) for v in want.values())
    for a in (x, *want.values()):
        a.flags.writeable = False
    return x, targets, pattern, other, want


# ---- every fixture case against the reference's recorded outputs ----------

def test_fixture_match(hip, data):
    """mask, mask + count, count only"""
    s = to_dev(data["states"])
    for k, name in enumerate(data["target_names"]):
        w, u = to_dev(data["targets"][k][0]), to_dev(data["targets"][k][1])
        want = data["match"][k]
        assert (to_host(hip.match(s, w, u)) == want).all(), name
        mask, count = hip.match(s, w, u, count=True)
        assert (to_host(mask) == want).all(), name
        assert (to_host(count) == M.popcount(want)).all(), name
        assert (to_host(hip.match(s, w, u, count="only")) == M.popcount(want)).all(), name
    assert (to_host(s) == data["states"]).all()


def test_fixture_convolve(hip, data):
    s = to_dev(data["states"])
    for k, name in enumerate(data["pattern_names"]):
        assert (to_host(hip.convolve(s, to_dev(data["patterns"][k]))) == data["convolve"][k]).all(), name


def test_fixture_interaction_offsets(hip, data):
    s = to_dev(data["states"])
    for k, name in enumerate(data["other_names"]):
        got = to_host(hip.interaction_offsets(s, to_dev(data["others"][k])))
        assert (got == data["interaction"][k]).all(), name


# ---- ragged sizes against the numpy definitions -----------------------------

@pytest.mark.parametrize("n", RAGGED)
def test_ragged_match(hip, ragged, n):
    """out of place, in place, and on a batch that is only 8-byte aligned"""
    x, targets, _, _, want = ragged
    for name, (w, u) in targets.items():
        dw, du = to_dev(w), to_dev(u)
        for offset8 in (False, True):
            s = to_dev(x[:n], offset8)
            mask, count = hip.match(s, dw, du, count=True)
            assert (to_host(mask) == want[name][:n]).all(), (name, offset8)
            assert (to_host(count) == M.popcount(want[name][:n])).all(), (name, offset8)
            assert (to_host(s) == x[:n]).all()
            assert hip.match(s, dw, du, out=s) is s                                  # in place
            assert (to_host(s) == want[name][:n]).all(), (name, offset8, "in place")


@pytest.mark.parametrize("n", RAGGED)
def test_ragged_convolve_and_interaction_offsets(hip, ragged, n):
    x, _, pattern, other, want = ragged
    dp, do = to_dev(pattern), to_dev(other)
    for offset8 in (False, True):
        for fn, arg, key in ((hip.convolve, dp, "convolve"), (hip.interaction_offsets, do, "interaction")):
            s = to_dev(x[:n], offset8)
            assert (to_host(fn(s, arg)) == want[key][:n]).all(), (key, offset8)
            assert fn(s, arg, out=s) is s
            assert (to_host(s) == want[key][:n]).all(), (key, offset8, "in place")


# ---- the sharp inputs: one wrong cell, one lost term or threshold shows --------

@pytest.fixture(scope="module")
def sharp(port):
    return S.fixture_data(port)


@pytest.fixture(scope="module")
def clustered(port, sharp):
    """interaction_batch(4097) and the numpy definition's answer for every
    sharp other, computed once; a batch of n is the first n"""
    x = S.interaction_batch(port, S.N_BATCH)
    want = {name: M.np_interaction_offsets(x, sharp["others"][k]) for k, name in enumerate(sharp["other_names"])}
    for k, name in enumerate(sharp["other_names"]):
        assert (want[name][:S.N_RECORDED] == sharp["interaction"][k]).all()
    for a in (x, *want.values()):
        a.flags.writeable = False
    return x, want


@pytest.mark.parametrize("offset8", [False, True])
def test_near_miss_match(hip, sharp, offset8):
    """every target on its own near misses against the reference's recorded
    masks: mask, mask + count, count only, in place.  Universe 0 matches at
    the planted offset and no near miss does."""
    for name, (states, (dx, dy), (w, u), want) in sharp["near_miss"].items():
        dw, du, s = to_dev(w), to_dev(u), to_dev(states, offset8)
        pops = M.popcount(want)
        got = to_host(hip.match(s, dw, du))
        assert (got == want).all(), name
        hit = (got[:, dx] >> np.uint64(dy)) & M.U1
        assert hit[0] == 1 and not hit[1:].any(), name
        mask, count = hip.match(s, dw, du, count=True)
        assert (to_host(mask) == want).all(), name
        assert (to_host(count) == pops).all(), name
        assert (to_host(hip.match(s, dw, du, count="only")) == pops).all(), name
        assert (to_host(s) == states).all(), name
        assert hip.match(s, dw, du, out=s) is s
        assert (to_host(s) == want).all(), (name, "in place")


@pytest.mark.parametrize("offset8", [False, True])
def test_impulse_convolve(hip, sharp, offset8):
    """every pattern on the single cells and the pair: the answer is the
    pattern moved, so each of its cells shows"""
    for k, (name, p) in enumerate(sharp["patterns"].items()):
        s, dp = to_dev(sharp["impulse_states"], offset8), to_dev(p)
        assert (to_host(hip.convolve(s, dp)) == sharp["convolve"][k]).all(), name
        assert hip.convolve(s, dp, out=s) is s
        assert (to_host(s) == sharp["convolve"][k]).all(), (name, "in place")


def test_recorded_interaction_offsets(hip, sharp):
    s = to_dev(sharp["batch"])
    for k, name in enumerate(sharp["other_names"]):
        got = to_host(hip.interaction_offsets(s, to_dev(sharp["others"][k])))
        assert (got == sharp["interaction"][k]).all(), name
    assert (to_host(s) == sharp["batch"]).all()


@pytest.mark.parametrize("n", RAGGED)
def test_ragged_clustered_interaction_offsets(hip, sharp, clustered, n):
    """out of place and in place, 16- and 8-byte aligned, every sharp other"""
    x, want = clustered
    for k, name in enumerate(sharp["other_names"]):
        do = to_dev(sharp["others"][k])
        for offset8 in (False, True):
            s = to_dev(x[:n], offset8)
            assert (to_host(hip.interaction_offsets(s, do)) == want[name][:n]).all(), (name, offset8)
            assert (to_host(s) == x[:n]).all()
            assert hip.interaction_offsets(s, do, out=s) is s
            assert (to_host(s) == want[name][:n]).all(), (name, offset8, "in place")


def test_clustered_interaction_offsets_side_stream(hip, sharp, clustered):
    x, want = clustered
    side = torch.cuda.Stream()
    s = to_dev(x)
    others = [to_dev(o) for o in sharp["others"]]
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        got = [hip.interaction_offsets(s, do, stream=side) for do in others]
    side.synchronize()
    for name, g in zip(sharp["other_names"], got):
        assert (to_host(g) == want[name]).all(), name


@pytest.mark.parametrize("device,shards", [(0, None), (-1, 3)])
def test_clustered_interaction_offsets_host_forms(hip, sharp, clustered, monkeypatch, device, shards):
    if shards:
        monkeypatch.setenv("LIFEAPI_HOST_SHARDS", str(shards))
    x, want = clustered
    for k, name in enumerate(sharp["other_names"]):
        assert (hip.interaction_offsets_host(x, sharp["others"][k], device=device) == want[name]).all(), name
    y = x.copy()
    assert hip.interaction_offsets_host(y, sharp["others"][0], out=y, device=device) is y
    assert (y == want[sharp["other_names"][0]]).all()


# ---- counts -------------------------------------------------------------------

def test_count_only_touches_nothing_else(hip, ragged):
    """the count is the mask's population for every universe, and with d_out
    NULL nothing but the n counts is written: guard words around the count
    array and the states stay as they were"""
    x, targets, _, _, want = ragged
    n, guard = 4097, 64
    w, u = (to_dev(p) for p in targets["care8_seams"])
    s = to_dev(x)
    buf = torch.full((n + 2 * guard,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    hip._check(hip.lib.lifeapi_match_batch_dev(s.data_ptr(), w.data_ptr(), u.data_ptr(), None,
                                               buf.data_ptr() + 4 * guard, n, hip._stream(None)))
    got = to_host(buf)
    assert (got[:guard] == 0x5A5A5A5A).all() and (got[-guard:] == 0x5A5A5A5A).all()
    pops = M.popcount(want["care8_seams"])
    assert (got[guard:-guard] == pops).all()
    assert len(set(pops.tolist())) > 8                         # the counts tell universes apart
    assert (to_host(s) == x).all()


# ---- streams and the order book ---------------------------------------------

def test_side_stream(hip, ragged):
    x, targets, pattern, other, want = ragged
    side = torch.cuda.Stream()
    s = to_dev(x)
    w, u = (to_dev(p) for p in targets["block_ring"])
    dp, do = to_dev(pattern), to_dev(other)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        mask, count = hip.match(s, w, u, count=True, stream=side)
        conv = hip.convolve(s, dp, stream=side)
        inter = hip.interaction_offsets(s, do, stream=side)
    side.synchronize()
    assert (to_host(mask) == want["block_ring"]).all()
    assert (to_host(count) == M.popcount(want["block_ring"])).all()
    assert (to_host(conv) == want["convolve"]).all()
    assert (to_host(inter) == want["interaction"]).all()


@pytest.fixture(scope="module")
def tune(hip):
    import tune_hip
    return tune_hip


@pytest.mark.parametrize("case", ["match", "match_with_count", "convolve", "interaction_offsets"])
def test_output_batch_recorded_as_written_forward(tune, hip, case):
    """tests/test_launch_policy.py::test_device_writer_records_its_output's
    check for the new writers: a batch the order book holds as written in
    reverse is held as written forward once one of them has rewritten it, so
    the next order-keyed reader of that extent reverses"""
    n = 4096
    src = torch.zeros(n * 16 * 64, dtype=torch.int64, device="cuda").data_ptr()  # (the book never reads memory)
    zp = src + 8 * n * 512
    y = torch.zeros((n, 64), dtype=torch.int64, device="cuda")
    out = torch.zeros((n, 64), dtype=torch.int64, device="cuda")
    zero = torch.zeros((1, 64), dtype=torch.int64, device="cuda")
    write = {"match": lambda: hip.match(y, zero, zero, out=out),
             "match_with_count": lambda: hip.match(y, zero, zero, out=out, count=True),
             "convolve": lambda: hip.convolve(y, zero, out=out),
             "interaction_offsets": lambda: hip.interaction_offsets(y, zero, out=out)}[case]
    nbytes = n * 512
    tune.order_note(src, nbytes)
    assert tune.order_probe(src, out.data_ptr(), nbytes) is True     # recorded as written in reverse
    write()
    torch.cuda.synchronize()
    assert tune.order_probe(out.data_ptr(), zp, nbytes) is True      # rewritten forward: the next reader reverses


def test_count_only_records_no_batch(tune, hip):
    """a count-only Match writes no batch: the book's entry for the states stays"""
    n = 4096
    y = torch.zeros((n, 64), dtype=torch.int64, device="cuda")
    zero = torch.zeros((1, 64), dtype=torch.int64, device="cuda")
    src = torch.zeros(n * 16 * 64, dtype=torch.int64, device="cuda").data_ptr()
    tune.order_note(src, n * 512)
    assert tune.order_probe(src, y.data_ptr(), n * 512) is True      # y recorded as written in reverse
    hip.match(y, zero, zero, count="only")
    torch.cuda.synchronize()
    assert tune.order_probe(y.data_ptr(), src + 8 * n * 512, n * 512) is False   # still: its reader runs forward


# ---- host forms -----------------------------------------------------------------

@pytest.mark.parametrize("device,shards", [(0, None), (-1, 3)])
def test_host_forms(hip, ragged, monkeypatch, device, shards):
    if shards:
        monkeypatch.setenv("LIFEAPI_HOST_SHARDS", str(shards))
    x, targets, pattern, other, want = ragged
    for name, (w, u) in targets.items():
        mask, count = hip.match_host(x, w, u, count=True, device=device)
        assert (mask == want[name]).all() and (count == M.popcount(want[name])).all(), name
    w, u = targets["care8_seams"]
    assert (hip.match_host(x, w, u, device=device) == want["care8_seams"]).all()
    assert (hip.match_host(x, w, u, count="only", device=device) == M.popcount(want["care8_seams"])).all()
    y = x.copy()
    assert hip.match_host(y, w, u, out=y, device=device) is y                         # in place
    assert (y == want["care8_seams"]).all()
    assert (hip.convolve_host(x, pattern, device=device) == want["convolve"]).all()
    assert (hip.interaction_offsets_host(x, other, device=device) == want["interaction"]).all()


# ---- the C++ facade ---------------------------------------------------------------

def test_match_batch_cpp():
    """tests/cpp/match_batch_test.cpp: MatchBatch / MatchCountBatch /
    ConvolveBatch / InteractionOffsetsBatch on 1000 seeded states, dense and
    sparse with clusters, and on near misses, against the facade's own CPU
    members"""
    exe = os.path.join(ROOT, "build", "match_batch_test")
    if not os.path.exists(exe):
        import __graft_entry__ as g
        g.build_cpp_tests()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
