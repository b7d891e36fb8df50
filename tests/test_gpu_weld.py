"""GPU: batched LifeWeld::FromRequired, ToTarget, ToStable and InteractionOffsets
(weld_kernels.hpp) through lifeapi_amd.hip, bit-exact against (1) the reference's
recorded outputs (tests/golden/weld_family.npz) and (2) the numpy definitions of
tests/test_weld_model.py, which CPU tests pin to the same fixture; then
properties on the GPU alone, and the two chains into the existing kernels."""
import os
import subprocess

import numpy as np
import pytest
import torch

import test_weld_model as M
import weld_cases as C
from test_gpu_match import to_dev, to_host

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RAGGED = [1, 2, 3, 5, 63, 64, 65, 4097]
SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)
RAGGED_DURATION = 8


@pytest.fixture(scope="module")
def rec(port):
    return M.Recording(port)


class Guarded:
    """an output of n objects of k planes with one sentinel object before and after"""

    def __init__(self, n, k):
        self.all = torch.full((n + 2, k * 64), int(SENTINEL.view(np.int64)), dtype=torch.int64, device="cuda")
        self.out = self.all[1:n + 1]

    def result(self):
        h = to_host(self.all)
        assert (h[0] == SENTINEL).all() and (h[-1] == SENTINEL).all(), "a sentinel object was written"
        return h[1:-1]


def dev(a, k=1):
    return to_dev(np.ascontiguousarray(a, np.uint64).reshape(-1, 64)).view(-1, k * 64)


# ---- every golden case against the reference's recorded outputs -------------------

def test_golden_from_required(hip, rec):
    s, r = (np.stack(x) for x in zip(*rec.pairs.values()))
    ds, dr, g = dev(s), dev(r), Guarded(len(s), 4)
    hip.weld_from_required(ds, dr, out=g.out)
    assert (g.result().reshape(-1, 4, 64) == rec.from_required).all()
    assert (to_host(ds) == s).all() and (to_host(dr) == r).all()
    for u in (0, 7, len(s) - 1):      # one universe at a time, the one-required form
        got = to_host(hip.weld_from_required(dev(s[u]), dev(r[u])))
        assert (got.reshape(4, 64) == rec.from_required[u]).all(), u


def test_golden_to_target(hip, rec):
    w = np.stack(list(rec.welds.values()))
    dw, gw, gu = dev(w, 4), Guarded(len(w), 1), Guarded(len(w), 1)
    hip.weld_to_target(dw, wanted=gw.out, unwanted=gu.out)
    assert (gw.result() == rec.target[:, 0]).all() and (gu.result() == rec.target[:, 1]).all()
    assert (to_host(dw).reshape(w.shape) == w).all()


def test_golden_to_stable_static_and_duration_zero(hip, rec):
    w = np.stack(list(rec.welds.values()))
    dw, g = dev(w, 4), Guarded(len(w), 10)
    hip.weld_to_stable(dw, out=g.out)
    assert (g.result().reshape(-1, 10, 64) == rec.stable0).all()
    # duration 0 with any active (one, or one per weld) and any mask is the same thing
    one, per = dev(rec.actives["soup2"]), dev(np.stack([rec.actives["soup3"], rec.actives["glider"]] * len(w))[:len(w)])
    for active in (one, per):
        for mask in (None, dev(rec.masks["soup"])):
            got = to_host(hip.weld_to_stable(dw, active, 0, mask))
            assert (got.reshape(-1, 10, 64) == rec.stable0).all()
    assert (to_host(dw).reshape(w.shape) == w).all()


def test_golden_to_stable_cases(hip, rec):
    """every recorded ToStable(active, duration, mask): one at a time with the
    one-active form, then grouped by (duration, mask) with an active per weld"""
    groups = {}
    for i, case in enumerate(C.STABLE_CASES):
        w, a, d, m = rec.stable_inputs(case)
        g = Guarded(1, 10)
        hip.weld_to_stable(dev(w, 4), dev(a), d, dev(m), out=g.out)
        assert (g.result().reshape(10, 64) == rec.stable[i]).all(), case
        groups.setdefault((d, case[3]), []).append(i)
    assert max(len(v) for v in groups.values()) >= 5
    for (d, m), members in groups.items():
        w = np.stack([rec.welds[C.STABLE_CASES[i][0]] for i in members])
        a = np.stack([rec.actives[C.STABLE_CASES[i][1]] for i in members])
        g = Guarded(len(members), 10)
        hip.weld_to_stable(dev(w, 4), dev(a), d, None if m == "all" else dev(rec.masks[m]), out=g.out)
        assert (g.result().reshape(-1, 10, 64) == rec.stable[members]).all(), (d, m)


def test_golden_interaction_offsets(hip, rec):
    w = np.stack([rec.welds[n] for n in C.OFFSET_WELDS])
    dw = dev(w, 4)
    for i, o in enumerate(C.OFFSET_OTHERS):
        g = Guarded(len(w), 1)
        hip.weld_interaction_offsets(dw, dev(rec.welds[o], 4), out=g.out)
        got = g.result()
        bad = [n for n, a, b in zip(C.OFFSET_WELDS, got, rec.offsets[i]) if (a != b).any()]
        assert not bad, (o, bad)
    assert (to_host(dw).reshape(w.shape) == w).all()


# ---- ragged batches against the numpy definitions --------------------------------

@pytest.fixture(scope="module")
def ragged(port, rec):
    """4097 objects drawn from a pool, the answers computed once on the pool.
    The empty object sits next to the densest ones at both parities of every
    grouping (1, 2 and 4 objects per wave)."""
    names = list(rec.welds)
    pool_w = np.stack(list(rec.welds.values()))
    pair_s, pair_r = (np.stack(x) for x in zip(*rec.pairs.values()))
    act_names = list(rec.actives)
    pool_a = np.stack([rec.actives[act_names[i % len(act_names)]] for i in range(len(pool_w))])
    mask, other = rec.masks["soup"], rec.welds["soupweld3_2"]
    want_pool = {
        "from_per": rec.from_required,
        "from_one": np.stack([M.from_required(s, pair_r[0]) for s in pair_s]),
        "target": rec.target,
        "stable0": rec.stable0,
        "stable": np.stack([M.to_stable_fused(w, a, RAGGED_DURATION, mask) for w, a in zip(pool_w, pool_a)]),
        "offsets": np.stack([M.interaction_offsets(w, other) for w in pool_w]),
    }
    rng = np.random.default_rng(1414)
    wi, pi = rng.integers(0, len(pool_w), 4097), rng.integers(0, len(pair_s), 4097)
    we, wd = names.index("empty"), names.index("soupweld1_2")
    pe, pd = list(rec.pairs).index("empty"), list(rec.pairs).index("soup1_1")
    for at, trio in ((0, (0, 1, 1)), (4, (1, 0, 1)), (9, (1, 1, 0)), (18, (0, 1, 0)), (61, (1, 0, 0)), (4093, (1, 1, 0, 1))):
        for k, dense in enumerate(trio):
            wi[at + k], pi[at + k] = (wd if dense else we), (pd if dense else pe)
    data = {"w": pool_w[wi], "a": pool_a[wi], "s": pair_s[pi], "r": pair_r[pi], "r0": pair_r[0], "mask": mask, "other": other}
    want = {k: v[pi if k.startswith("from") else wi] for k, v in want_pool.items()}
    assert (want["stable"] != want["stable0"]).any() and (want["from_per"] != want["from_one"]).any()
    for a in (*data.values(), *want.values()):
        a.flags.writeable = False
    return data, want


@pytest.mark.parametrize("n", RAGGED)
def test_ragged(hip, ragged, n):
    data, want = ragged
    w, a, s, r = dev(data["w"][:n], 4), dev(data["a"][:n]), dev(data["s"][:n]), dev(data["r"][:n])
    g = Guarded(n, 4)
    hip.weld_from_required(s, r, out=g.out)
    assert (g.result().reshape(-1, 4, 64) == want["from_per"][:n]).all()
    g = Guarded(n, 4)
    hip.weld_from_required(s, dev(data["r0"]), out=g.out)
    assert (g.result().reshape(-1, 4, 64) == want["from_one"][:n]).all()
    gw, gu = Guarded(n, 1), Guarded(n, 1)
    hip.weld_to_target(w, wanted=gw.out, unwanted=gu.out)
    assert (gw.result() == want["target"][:n, 0]).all() and (gu.result() == want["target"][:n, 1]).all()
    g = Guarded(n, 10)
    hip.weld_to_stable(w, out=g.out)
    assert (g.result().reshape(-1, 10, 64) == want["stable0"][:n]).all()
    g = Guarded(n, 10)
    hip.weld_to_stable(w, a, RAGGED_DURATION, dev(data["mask"]), out=g.out)
    got = g.result().reshape(-1, 10, 64)
    assert (got == want["stable"][:n]).all()      # (n == 1: one active for a batch of one)
    g = Guarded(n, 1)
    hip.weld_interaction_offsets(w, dev(data["other"], 4), out=g.out)
    assert (g.result() == want["offsets"][:n]).all()
    assert (to_host(w).reshape(-1, 4, 64) == data["w"][:n]).all() and (to_host(a) == data["a"][:n]).all()


# ---- properties --------------------------------------------------------------------

def test_one_for_all_equals_a_copy_per_object(hip, ragged):
    data, _ = ragged
    n = 67
    w, s = dev(data["w"][:n], 4), dev(data["s"][:n])
    r0, a0 = data["r0"], data["a"][3]
    one = to_host(hip.weld_from_required(s, dev(r0)))
    per = to_host(hip.weld_from_required(s, dev(np.tile(r0, (n, 1)))))
    assert (one == per).all()
    mask = dev(data["mask"])
    one = to_host(hip.weld_to_stable(w, dev(a0), 5, mask))
    per = to_host(hip.weld_to_stable(w, dev(np.tile(a0, (n, 1))), 5, mask))
    assert (one == per).all() and a0.any()


def test_null_mask_is_all_ones(hip, ragged):
    data, _ = ragged
    n = 67
    w, a = dev(data["w"][:n], 4), dev(data["a"][:n])
    ones = dev(~np.zeros(64, np.uint64))
    assert (to_host(hip.weld_to_stable(w, a, 6, None)) == to_host(hip.weld_to_stable(w, a, 6, ones))).all()
    assert (to_host(hip.weld_to_stable(w, a, 6, None)) != to_host(hip.weld_to_stable(w, a, 6, dev(data["mask"])))).any()


def test_fixed_point_stops_the_replay(hip, rec):
    """the eaten glider: the weld is itself again after 18 generations, so 4096
    generations are the recorded 40, and the generations replayed by then"""
    case = ("eater", "glider", 40, "all")
    w, a, _, m = rec.stable_inputs(case)
    settled = []
    want = M.to_stable_fused(w, a, 4096, m, settled=settled)
    assert settled[0] < 40 and (want == rec.stable[C.STABLE_CASES.index(case)]).all()
    dw, da = dev(w, 4), dev(a)
    assert (to_host(hip.weld_to_stable(dw, da, 4096)).reshape(10, 64) == want).all()
    assert (to_host(hip.weld_to_stable(dw, da, settled[0])).reshape(10, 64) == want).all()
    short = M.to_stable_fused(w, a, settled[0] - 2, m)
    assert (short != want).any() and (to_host(hip.weld_to_stable(dw, da, settled[0] - 2)).reshape(10, 64) == short).all()
    # in a batch the settled weld waits for nobody: its neighbours run on
    both = np.stack([w, rec.welds["soupweld2_3"]])
    acts = np.stack([a, rec.actives["soup3"]])
    got = to_host(hip.weld_to_stable(dev(both, 4), dev(acts), 64)).reshape(2, 10, 64)
    assert (got[0] == want).all() and (got[1] == M.to_stable_fused(both[1], acts[1], 64, m)).all()


def test_host_forms_agree(hip, ragged):
    data, want = ragged
    for n in (3, 4097):
        w, a, s, r = data["w"][:n], data["a"][:n], data["s"][:n], data["r"][:n]
        assert (hip.weld_from_required_host(s, r).reshape(-1, 4, 64) == want["from_per"][:n]).all()
        assert (hip.weld_from_required_host(s, data["r0"]).reshape(-1, 4, 64) == want["from_one"][:n]).all()
        wanted, unwanted = hip.weld_to_target_host(w)
        assert (wanted == want["target"][:n, 0]).all() and (unwanted == want["target"][:n, 1]).all()
        assert (hip.weld_to_stable_host(w).reshape(-1, 10, 64) == want["stable0"][:n]).all()
        got = hip.weld_to_stable_host(w, a, RAGGED_DURATION, data["mask"]).reshape(-1, 10, 64)
        assert (got == want["stable"][:n]).all()
        got = hip.weld_to_stable_host(w, data["a"][3], RAGGED_DURATION)
        dev_form = to_host(hip.weld_to_stable(dev(w, 4), dev(data["a"][3]), RAGGED_DURATION))
        assert (got == dev_form).all()
        assert (hip.weld_interaction_offsets_host(w, data["other"]) == want["offsets"][:n]).all()


# ---- the chains into the existing kernels -----------------------------------------

def test_chain_to_stable_into_propagate(hip, port, rec):
    """weld_to_stable's output, fed to the existing Propagate pass, is what the
    oracle's Propagate makes of the recorded stable"""
    names = [n for n in rec.welds if not n.startswith("soup")] + ["soup3_3", "soup4_1", "soupweld4_3"]
    idx = [rec.names.index(n) for n in names]
    planes = hip.weld_to_stable(dev(np.stack([rec.welds[n] for n in names]), 4))
    flags = hip.stable_pass(planes, "propagate")
    want, want_flags = port.stable_pass(rec.stable0[idx].reshape(-1, 640), 4)
    assert (to_host(planes) == want).all()
    assert ((flags.cpu().numpy() & 3) == (want_flags & 3)).all()
    # ... and after a replay
    case = ("eater", "glider", 40, "all")
    w, a, d, m = rec.stable_inputs(case)
    planes = hip.weld_to_stable(dev(w, 4), dev(a), d)
    hip.stable_pass(planes, "propagate")
    want, _ = port.stable_pass(rec.stable[C.STABLE_CASES.index(case)].reshape(-1, 640), 4)
    assert (to_host(planes) == want).all()


def np_match(state, wanted, unwanted):
    """Match (LifeTarget.hpp:53-55): the offsets at which the target fits"""
    s, ok = M.cells(state), np.ones((64, 64), bool)
    for plane, alive in ((wanted, True), (unwanted, False)):
        for a, b in zip(*np.nonzero(M.cells(plane))):
            moved = np.roll(s, (-a, -b), (0, 1))
            ok &= moved if alive else ~moved
    return M.words(ok)


def test_chain_to_target_into_match(hip, rec):
    """weld_to_target's output is a target the existing Match takes: the eater's
    weld found where it stands and where a copy was put, not where one is broken"""
    w = rec.welds["eater"]
    wanted, unwanted = hip.weld_to_target(dev(w, 4))
    field = w[0] | C.moved(w[0], 17, -9) | C.moved(w[0], -12, 20)
    field[(C.AT[0] - 12 + 2) % 64] ^= np.uint64(1) << np.uint64((C.AT[1] + 20) % 64)      # breaks the third copy
    universes = np.stack([field, w[0], np.zeros(64, np.uint64)])
    got = to_host(hip.match(dev(universes), wanted, unwanted))
    want = np.stack([np_match(u, rec.target[0, 0], rec.target[0, 1]) for u in universes])
    assert rec.names[0] == "eater" and (got == want).all()
    pops = [int(M.cells(x).sum()) for x in want]
    assert pops == [2, 1, 0], pops


def test_weld_batch_cpp(tmp_path, port, rec):
    """tests/cpp/weld_batch_test.cpp: the batched templates on the lifeapi::
    structs against the facade's CPU members"""
    import test_weld_facade as F
    exe = F.build("weld_batch_test", gpu=True)
    path = tmp_path / "cases.bin"
    F.write_cases(path, rec)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "weld_batch_test: ok" in r.stdout
