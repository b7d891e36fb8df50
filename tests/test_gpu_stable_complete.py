"""GPU: k_stable_complete against every run of tests/golden/stable_complete.npz,
bit for bit -- result, best and nodes -- and against the CPU model (tests/
test_stable_complete_model.py, itself pinned to the same recording) where the
recording has nothing: the two results only the batched search has, the early
returns, and the shared-seed form.  Each test takes the recorded objects (92,
at most 140 nodes and 21 frames each) through one or a few launches."""
import numpy as np
import pytest
import torch

import stable_complete_cases as C
import test_stable_complete_model as M
import weld_cases as WC
from test_gpu_match import to_dev, to_host

pytestmark = pytest.mark.gpu

FRAME, HEADER = 5376, 256


@pytest.fixture(scope="module")
def rec():
    return M.recording()


def dev(a, k=1):
    return to_dev(np.ascontiguousarray(a, np.uint64).reshape(-1, 64)).view(-1, k * 64)


def run(hip, planes, f=0, seeds=None, **kw):
    """(result, best, nodes) as numpy, of (n, 10, 64) planes in flag combination f"""
    minimise, use_seed = C.FLAGS[f]
    d = dev(planes, 10)
    before = d.clone()
    result, best, nodes = hip.stable_complete(d, minimise=minimise, seed=dev(seeds) if use_seed else None, **kw)
    torch.cuda.synchronize()
    assert torch.equal(d, before), "the planes were written"
    return result.cpu().numpy(), to_host(best).reshape(-1, 64), nodes.cpu().numpy()


def expect(rec, got, f, pick=None):
    pick = np.arange(len(rec.kept)) if pick is None else np.asarray(pick)
    result, best, nodes = got
    assert (result == rec.result[pick, f]).all(), np.flatnonzero(result != rec.result[pick, f])
    assert (nodes == rec.nodes[pick, f]).all(), np.flatnonzero(nodes != rec.nodes[pick, f])
    assert (best == rec.best[pick, f]).all()


# ---- every recording ------------------------------------------------------------

@pytest.mark.parametrize("f", range(4))
def test_golden(hip, rec, f):
    for name in ("column_seam", "row_seam", "within_zoi", "minimise_improves", "rounds2", "bad_tree", "seed3"):
        assert len(rec.classes[name]) >= 8, name
    expect(rec, run(hip, rec.planes, f, rec.seeds), f)


@pytest.mark.parametrize("f", range(4))
def test_single_objects(hip, rec, f):
    for u in (0, int(rec.classes["long"][0]), int(rec.classes["bad_tree"][0]), int(rec.classes["minimise_improves"][0])):
        expect(rec, run(hip, rec.planes[u:u + 1], f, rec.seeds[u:u + 1]), f, [u])


def test_host_form(hip, rec):
    for f in range(4):
        minimise, use_seed = C.FLAGS[f]
        got = hip.stable_complete_host(rec.planes, minimise=minimise, seed=rec.seeds if use_seed else None)
        expect(rec, got, f)


# ---- the workspace: one wave, a full grid, a grid and one object more ---------------

def full_waves(hip, depth):
    return (hip.stable_complete_workspace_bytes(1 << 20, depth) - HEADER) // (depth * FRAME)


def test_outputs_and_workspace_are_guarded(hip, rec):
    """n = 5 through a workspace of exactly one stack, sentinels around every output, a canary behind
    the workspace; then a full workspace: the same answers"""
    depth = 24
    pick = [int(rec.classes["long"][0]), int(rec.classes["depth0"][0]), int(rec.classes["deep"][0]),
            int(rec.classes["bad_root"][0]), int(rec.classes["minimise_improves"][0])]
    n, one = len(pick), HEADER + depth * FRAME
    assert hip.stable_complete_workspace_bytes(1, depth) == one
    planes, seeds = dev(rec.planes[pick], 10), dev(rec.seeds[pick])
    answers = []
    for ws_bytes in (one, hip.stable_complete_workspace_bytes(n, depth)):
        for f in range(4):
            best = torch.full((n + 2, 64), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda")
            nodes = torch.full((n + 2,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda")
            result = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            ws = torch.full((ws_bytes + 1024,), 0xC3, dtype=torch.uint8, device="cuda")
            assert ws.data_ptr() % 128 == 0
            rc = hip.lib.lifeapi_stable_complete_batch_dev(
                planes.data_ptr(), seeds.data_ptr(), 1, f, 0, depth, best[1:].data_ptr(), result[32:].data_ptr(),
                nodes[1:].data_ptr(), n, ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream)
            assert rc == 0, hip.lib.lifeapi_last_error()
            torch.cuda.synchronize()
            b, k, r, w = (t.cpu().numpy() for t in (best, nodes, result, ws))
            assert (b[0] == b[0, 0]).all() and (b[-1] == b[0, 0]).all() and k[0] == k[-1] == b[0, 0]
            assert (r[:32] == 0xA5).all() and (r[32 + n:] == 0xA5).all() and (w[ws_bytes:] == 0xC3).all()
            got = (r[32:32 + n], b[1:-1].view(np.uint64), k[1:-1])
            expect(rec, got, f, pick)
            answers.append(got)
    for a, b in zip(answers[:4], answers[4:]):
        assert all((x == y).all() for x, y in zip(a, b))


@pytest.mark.parametrize("f", (0, 3))
def test_a_wave_claims_a_second_object(hip, rec, f):
    """n = the full grid's waves + 1, long searches next to depth-0 ones: a stale stack, counter,
    best or maxPop would show in the object a wave takes next"""
    depth = 24
    waves = full_waves(hip, depth)
    assert waves % 4 == 0 and waves >= 12
    order = np.concatenate([rec.classes["long"], rec.classes["depth0"][:4], rec.classes["deep"],
                            rec.classes["bad_root"][:4], rec.classes["minimise_improves"][:4]])
    pick = np.resize(order, waves + 1)
    got = run(hip, rec.planes[pick], f, rec.seeds[pick], max_depth=depth)
    expect(rec, got, f, pick)
    # ... and many objects per wave: a workspace of three stacks
    ws = torch.empty(HEADER + 3 * depth * FRAME, dtype=torch.uint8, device="cuda")
    pick = np.resize(np.arange(len(rec.kept)), 301)
    expect(rec, run(hip, rec.planes[pick], f, rec.seeds[pick], max_depth=depth, workspace=ws), f, pick)


# ---- the budget and the stack bound ----------------------------------------------------

@pytest.mark.parametrize("f", range(4))
def test_budgets(hip, rec, f):
    """budgets nodes - 1, nodes and nodes + 1 (and 1) of every object, against the recorded runs"""
    checked = 0
    for budget in np.unique(rec.budgets[:, f]):
        u, b = np.nonzero(rec.budgets[:, f] == budget)
        result, best, nodes = run(hip, rec.planes[u], f, rec.seeds[u], node_budget=int(budget))
        assert (result == rec.bhead[u, f, b, 0]).all() and (nodes == rec.bhead[u, f, b, 1]).all(), budget
        assert (best == rec.bbest[u, f, b]).all(), budget
        checked += len(u)
    assert checked == rec.budgets[:, f].size
    assert (rec.bhead[:, f, :, 0] == M.TIMEOUT).sum() >= 16


def test_max_depth(hip, rec, port):
    """max_depth at an object's recorded depth, and one below: code 3 there, the others unaffected"""
    for u in (int(rec.classes["deep"][0]), int(rec.classes["backtracked"][0])):
        for f in (0, 1):
            d = int(rec.depth[u, f])
            assert d >= 1
            for depth in (d, d - 1):
                if depth == 0:
                    continue
                result, best, nodes = run(hip, rec.planes, f, rec.seeds, max_depth=depth)
                deep = rec.depth[:, f] > depth
                assert deep[u] == (depth < d) and (~deep).sum() >= 8
                assert (result[deep] == M.TOO_DEEP).all() and not best[deep].any()
                ok = np.flatnonzero(~deep)
                expect(rec, (result[ok], best[ok], nodes[ok]), f, ok)
                if deep[u]:
                    want = rec.run(port, u, f, max_depth=depth)
                    assert (want[0], want[2]) == (M.TOO_DEEP, nodes[u])
    with pytest.raises(hip.LifeApiError):
        run(hip, rec.planes[:1], 0, max_depth=0)


# ---- seeds, the early returns ---------------------------------------------------------

def test_seed_forms(hip, rec, port):
    """one seed for the batch = that seed for every object; an empty seed among good ones is code 4"""
    pick = np.concatenate([rec.classes["seed3"][:6], rec.classes["backtracked"][:4]])
    k = int(pick[0])
    shared = run(hip, rec.planes[pick], 2, rec.seeds[k:k + 1])
    each = run(hip, rec.planes[pick], 2, np.tile(rec.seeds[k], (len(pick), 1)))
    assert all((a == b).all() for a, b in zip(shared, each))
    expect(rec, tuple(a[:1] for a in shared), 2, [k])
    for i in (1, 5, 9):
        want = M.complete(port, rec.planes[pick[i]], rec.seeds[k])
        assert (shared[0][i], shared[2][i]) == (want[0], want[2]) and (shared[1][i] == want[1]).all()
    seeds = rec.seeds.copy()
    empty = np.arange(3, len(seeds), 7)
    seeds[empty] = 0
    for f in (2, 3):
        result, best, nodes = run(hip, rec.planes, f, seeds)
        # (an object with no ON cell known returns early, before its seed is looked at)
        no_state = ~rec.planes[empty][:, M.ST].any(axis=1)
        assert (~no_state).sum() >= 6
        assert (result[empty] == np.where(no_state, M.COMPLETED, M.BAD_SEED)).all()
        assert not best[empty].any() and not nodes[empty].any()
        ok = np.setdiff1d(np.arange(len(seeds)), empty)
        expect(rec, (result[ok], best[ok], nodes[ok]), f, ok)


def early_cases(rec):
    """twelve recorded objects with a known ON cell: every third with its state emptied, every
    third with its unknown emptied; the first six with an empty seed"""
    pick = np.flatnonzero(rec.planes[:, M.ST].any(axis=1))[:12]
    planes, seeds = rec.planes[pick].copy(), rec.seeds[pick].copy()
    planes[0:12:3, M.ST] = 0
    planes[1:12:3, M.UN] = 0
    seeds[:6] = 0
    return pick, planes, seeds


def test_early_returns(hip, rec, port):
    """an empty state completes to the empty state, an empty unknown to the state, no node entered,
    before the seed is looked at"""
    pick, planes, seeds = early_cases(rec)
    for f in range(4):
        minimise, use_seed = C.FLAGS[f]
        result, best, nodes = run(hip, planes, f, seeds)
        for u in range(12):
            want = M.complete(port, planes[u], seeds[u] if use_seed else None, minimise)
            assert (result[u], nodes[u]) == (want[0], want[2]) and (best[u] == want[1]).all(), (f, u)
            if u % 3 == 0:
                assert (result[u], nodes[u]) == (M.COMPLETED, 0) and not best[u].any()
            elif u % 3 == 1:
                assert (result[u], nodes[u]) == (M.COMPLETED, 0) and (best[u] == planes[u, M.ST]).all()
            elif use_seed and u < 6:
                assert (result[u], nodes[u]) == (M.BAD_SEED, 0) and not best[u].any()
            else:
                assert nodes[u] == rec.nodes[pick[u], f] >= 1


# ---- the chain a search runs: weld_to_stable, then stable_complete ------------------------

def placements(rec, c):
    cells = [(x, y) for x in range(64) for y in range(64) if int(rec.weld["tested"][c][x]) >> y & 1]
    a, b = rec.weld["a"][c], rec.weld["b"][c]
    return cells, np.stack([a | WC.moved(b, x, y) for x, y in cells])


def test_chain_from_welds(hip, rec):
    """UnweldableMask's placements on the device, weld_to_stable -> stable_complete, against the same
    through the host forms and against the reference's recorded mask"""
    for c in range(len(rec.weld["a"])):
        cells, welds = placements(rec, c)
        assert 16 <= len(cells) <= 64
        stables = hip.weld_to_stable(dev(welds, 4))
        result, best, nodes = hip.stable_complete(stables, node_budget=C.WELD_BUDGET)
        torch.cuda.synchronize()
        got = (result.cpu().numpy(), to_host(best).reshape(-1, 64), nodes.cpu().numpy())
        host = hip.stable_complete_host(hip.weld_to_stable_host(welds), node_budget=C.WELD_BUDGET)
        assert all((a == b).all() for a, b in zip(got, host))
        assert np.bincount(got[0], minlength=3).tolist() == rec.weld["counts"][c].tolist()
        bad = np.zeros(64, np.uint64)
        for (x, y), r in zip(cells, got[0]):
            if r == M.INCONSISTENT:
                bad[x] |= np.uint64(1) << np.uint64(y)
        assert (bad == rec.weld["mask"][c] & rec.weld["tested"][c]).all()
