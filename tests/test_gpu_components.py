"""GPU: batched FirstOn, ComponentContaining and Components
(components_kernels.hpp) through lifeapi_amd.hip, bit-exact against (1) the
reference's recorded outputs (tests/golden/components.npz) and (2) the numpy
definitions of tests/test_components_model.py, which CPU tests pin to the same
fixture; then properties on the GPU alone."""
import os
import subprocess

import numpy as np
import pytest
import torch

import components_cases as C
import test_components_model as M
from test_gpu_match import to_dev, to_host

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RAGGED = [1, 2, 3, 5, 63, 64, 65, 4097]
SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)
RAGGED_CAP = 8


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(M.GOLDEN))


@pytest.fixture(scope="module")
def states(port):
    return C.states(port)


def sentinel(*shape):
    return torch.full(shape, int(SENTINEL.view(np.int64)), dtype=torch.int64, device="cuda")


def padded(parts, cap):
    """(n, cap, 64): each universe's first min(count, cap) components, then the sentinel"""
    out = np.full((len(parts), cap, 64), SENTINEL, np.uint64)
    for u, p in enumerate(parts):
        k = min(len(p), cap)
        if k:
            out[u, :k] = np.stack(p[:k])
    return out


@pytest.fixture(scope="module")
def ragged(port, states):
    """4097 universes drawn from a pool of fixture states and seeded soups of
    three densities, interleaved so that the two universes of a wave converge
    after very different numbers of rounds: the spiral sits next to the empty
    state and a one-cell state at both parities.  The numpy definitions'
    answers are computed once on the pool; a batch of n is the first n."""
    pool = [states[n] for n in ("spiral", "empty", "pair_20_0_0", "six_cells", "comb", "spiral_cut", "staircase",
                                "quad0", "row_and_col", "pair_63_3_3", "full_row")]
    pool += [states[f"soup{k}_{i}"] for k in (2, 3, 4) for i in range(4)]
    extra = port.fill(12, seed=9090) & port.fill(12, seed=9091) & port.fill(12, seed=9092)
    extra[6:] &= port.fill(6, seed=9093)
    pool = np.stack(pool + list(extra))
    rng = np.random.default_rng(5150)
    idx = rng.integers(0, len(pool), 4097)
    for at, trio in ((0, (0, 1, 2)), (5, (1, 0, 2)), (10, (2, 0, 1)), (17, (0, 2, 1)), (62, (1, 0, 0)), (4094, (2, 1, 0))):
        idx[at:at + 3] = trio
    seed_pool = port.fill(len(pool), seed=9190)
    for j in range(1, 5):
        seed_pool &= port.fill(len(pool), seed=9190 + j)
    one_seed = C.from_cells([(33, 33), (60, 0), (2, 5)])
    want = {"first_on": M.np_first_on(pool)[idx],
            "cc_per": M.np_component_containing(pool, seed_pool, C.CORONAS["default"])[idx],
            "cc_one": M.np_component_containing(pool, one_seed, C.CORONAS["default"])[idx],
            "cc_7x7": M.np_component_containing(pool, seed_pool, C.CORONAS["7x7"])[idx]}
    parts = M.np_components(pool, C.CORONAS["default"])
    want["count"] = np.array([len(p) for p in parts], np.uint32)[idx]
    want["parts"] = padded(parts, RAGGED_CAP)[idx]
    parts3 = M.np_components(pool, C.CORONAS["down"])
    want["count_down"] = np.array([len(p) for p in parts3], np.uint32)[idx]
    x, seeds = pool[idx], seed_pool[idx]
    assert want["count"].min() == 0 and want["count"].max() > 100 and (want["cc_per"] != want["cc_7x7"]).any()
    for a in (x, seeds, one_seed, *want.values()):
        a.flags.writeable = False
    return x, seeds, one_seed, want


# ---- every golden case against the reference's recorded outputs -------------

def test_golden_first_on(hip, gold, states):
    x = np.stack(list(states.values()))
    s = to_dev(x)
    assert (hip.first_on(s).cpu().numpy() == gold["first_on"]).all()
    assert (to_host(s) == x).all()


@pytest.mark.parametrize("corona", C.COMPONENTS_CORONAS)
def test_golden_components(hip, gold, states, corona):
    """counts only, components only, both together; the default corona also as None"""
    want = M.recorded_parts(gold, states, corona)
    x = np.stack([states[n] for n in want])
    counts = gold["count_" + corona].astype(np.uint32)
    cap = int(counts.max())
    full = padded(list(want.values()), cap)
    s = to_dev(x)
    for value in [C.CORONAS[corona]] + ([None] if corona == "default" else []):
        assert (to_host(hip.components(s, value)).view(np.uint32) == counts).all(), corona
        comps = hip.components(s, value, max_components=cap, count=False, components_out=sentinel(len(x), cap, 64))
        assert (to_host(comps) == full).all(), corona
        comps, got = hip.components(s, value, max_components=cap, components_out=sentinel(len(x), cap, 64))
        assert (to_host(comps) == full).all() and (to_host(got).view(np.uint32) == counts).all(), corona
    assert (to_host(s) == x).all()


def test_golden_component_containing(hip, gold, states):
    seeds = M.cc_seeds(states)
    x = np.stack([states[n] for n in C.CC_STATES])
    s = to_dev(x)
    for c, corona in enumerate(C.CORONAS):
        for k, kind in enumerate(C.SEED_KINDS):
            sd = to_dev(np.stack([seeds[n][kind] for n in C.CC_STATES]))
            got = hip.component_containing(s, sd, C.CORONAS[corona])
            assert (to_host(got) == gold["cc"][c, :, k]).all(), (corona, kind)
            if corona == "default":
                assert (to_host(hip.component_containing(s, sd)) == gold["cc"][c, :, k]).all(), kind
            for i in range(len(x)):      # one universe, one seed
                got = hip.component_containing(s[i:i + 1], sd[i:i + 1], C.CORONAS[corona])
                assert (to_host(got)[0] == gold["cc"][c, i, k]).all(), (corona, kind, i)
    # one seed for the whole batch: the recorded answer where the seed is that state's own
    for i, n in enumerate(C.CC_STATES):
        sd = to_dev(seeds[n]["two"][None])
        got = to_host(hip.component_containing(s, sd))
        assert (got[i] == gold["cc"][0, i, C.SEED_KINDS.index("two")]).all(), n
        assert (got == M.np_component_containing(x, seeds[n]["two"], C.CORONAS["default"])).all(), n
    assert (to_host(s) == x).all()


@pytest.mark.parametrize("cap", [1, 3, 512, 600])
def test_cap(hip, gold, states, cap):
    """the count is the true one, exactly the first min(count, cap) slots are
    the reference's, the others keep the sentinel"""
    want = M.recorded_parts(gold, states, "default")
    names = ["lattice512", "soup3_0", "empty", "spiral"]
    x = np.stack([states[n] for n in names])
    counts = np.array([len(want[n]) for n in names], np.uint32)
    assert counts[0] == 512 and 3 < counts[1] < 512
    comps, got = hip.components(to_dev(x), max_components=cap, components_out=sentinel(len(x), cap, 64))
    assert (to_host(got).view(np.uint32) == counts).all()
    assert (to_host(comps) == padded([list(want[n]) for n in names], cap)).all()


# ---- ragged sizes against the numpy definitions -------------------------------

@pytest.mark.parametrize("n", RAGGED)
def test_ragged_first_on_and_containing(hip, ragged, n):
    """out of place, with out = states and out = seeds, on a batch that is only 8-byte aligned"""
    x, seeds, one_seed, want = ragged
    for offset8 in (False, True):
        s, sd, one = to_dev(x[:n], offset8), to_dev(seeds[:n], offset8), to_dev(one_seed[None], offset8)
        assert (hip.first_on(s).cpu().numpy() == want["first_on"][:n]).all(), offset8
        assert (to_host(hip.component_containing(s, sd)) == want["cc_per"][:n]).all(), offset8
        if n > 1:
            assert (to_host(hip.component_containing(s, one)) == want["cc_one"][:n]).all(), offset8
        assert (to_host(hip.component_containing(s, sd, C.CORONAS["7x7"])) == want["cc_7x7"][:n]).all(), offset8
        assert (to_host(s) == x[:n]).all() and (to_host(sd) == seeds[:n]).all()
        assert hip.component_containing(s, sd, out=sd) is sd
        assert (to_host(sd) == want["cc_per"][:n]).all(), (offset8, "out = seeds")
        sd = to_dev(seeds[:n], offset8)
        assert hip.component_containing(s, sd, out=s) is s
        assert (to_host(s) == want["cc_per"][:n]).all(), (offset8, "out = states")


@pytest.mark.parametrize("n", RAGGED)
def test_ragged_components(hip, ragged, n):
    x, _, _, want = ragged
    for offset8 in (False, True):
        s = to_dev(x[:n], offset8)
        assert (to_host(hip.components(s)).view(np.uint32) == want["count"][:n]).all(), offset8
        assert (to_host(hip.components(s, C.CORONAS["down"])).view(np.uint32) == want["count_down"][:n]).all(), offset8
        comps, got = hip.components(s, max_components=RAGGED_CAP, components_out=sentinel(n, RAGGED_CAP, 64))
        assert (to_host(got).view(np.uint32) == want["count"][:n]).all(), offset8
        assert (to_host(comps) == want["parts"][:n]).all(), offset8
        assert (to_host(s) == x[:n]).all()


def test_side_stream(hip, ragged):
    x, seeds, _, want = ragged
    side = torch.cuda.Stream()
    s, sd = to_dev(x), to_dev(seeds)
    out = sentinel(len(x), RAGGED_CAP, 64)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        cells = hip.first_on(s, stream=side)
        cc = hip.component_containing(s, sd, stream=side)
        comps, counts = hip.components(s, max_components=RAGGED_CAP, components_out=out, stream=side)
    side.synchronize()
    assert (cells.cpu().numpy() == want["first_on"]).all() and (to_host(cc) == want["cc_per"]).all()
    assert (to_host(counts).view(np.uint32) == want["count"]).all() and (to_host(comps) == want["parts"]).all()


@pytest.mark.parametrize("device,shards", [(0, None), (-1, 3)])
def test_host_forms(hip, ragged, monkeypatch, device, shards):
    if shards:
        monkeypatch.setenv("LIFEAPI_HOST_SHARDS", str(shards))
    x, seeds, one_seed, want = ragged
    assert (hip.first_on_host(x, device=device) == want["first_on"]).all()
    assert (hip.component_containing_host(x, seeds, device=device) == want["cc_per"]).all()
    assert (hip.component_containing_host(x, one_seed, device=device) == want["cc_one"]).all()
    assert (hip.component_containing_host(x, seeds, C.CORONAS["7x7"], device=device) == want["cc_7x7"]).all()
    y = seeds.copy()
    assert hip.component_containing_host(x, y, out=y, device=device) is y                 # out = seeds
    assert (y == want["cc_per"]).all()
    assert (hip.components_host(x, device=device) == want["count"]).all()
    out = np.full((len(x), RAGGED_CAP, 64), SENTINEL, np.uint64)
    comps, counts = hip.components_host(x, max_components=RAGGED_CAP, components_out=out, device=device)
    assert (counts == want["count"]).all() and (comps == want["parts"]).all()
    assert (hip.components_host(x, max_components=RAGGED_CAP, count=False, components_out=out, device=device)
            == want["parts"]).all()


# ---- properties, on the GPU alone ------------------------------------------------

def test_properties(hip, ragged):
    x, _, _, want = ragged
    s = to_dev(x)
    counts = hip.components(s)
    cap = int(counts.max())
    comps = hip.components(s, max_components=cap, count=False,
                           components_out=torch.zeros((len(x), cap, 64), dtype=torch.int64, device="cuda"))
    # pairwise disjoint and OR to the state: every cell lies in exactly one component
    union = torch.zeros_like(s)
    for i in range(cap):
        assert not (union & comps[:, i]).any(), i
        union |= comps[:, i]
    assert torch.equal(union, s)
    # the count is the number of non-empty slots
    assert torch.equal((comps != 0).any(dim=2).sum(dim=1).to(torch.int32), counts)
    # a component is the component of itself
    for i in (0, 1, cap // 2, cap - 1):
        assert torch.equal(hip.component_containing(s, comps[:, i].contiguous()), comps[:, i]), i
    # the count is invariant under translation
    for dx, dy in ((1, 0), (0, 1), (13, -27), (32, 32)):
        assert torch.equal(hip.components(hip.transform(s, "Identity", dx, dy)), counts), (dx, dy)
    assert (to_host(s) == x).all()


# ---- the C++ facade ---------------------------------------------------------------

def test_components_batch_cpp(tmp_path, port, gold):
    """tests/cpp/components_batch_test.cpp: FirstOn, ComponentContaining (one
    seed, a seed per universe), ComponentCounts and Components on a type of the
    reference's shape, against the golden file"""
    import test_components_facade as F
    exe = F.build("components_batch_test", gpu=True)
    path = tmp_path / "cases.bin"
    F.write_cases(path, port, gold)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
