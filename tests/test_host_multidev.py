"""GPU: the multi-device branch of the host-pointer lifeapi_step_batch and
lifeapi_step_contains_batch (device = -1: contiguous shards, one host thread
each, the arrays pinned once for all shards; host.hip over_devices).  A 1-GPU box has one device, so the shard count is
forced with LIFEAPI_HOST_SHARDS (shard s on device s mod ndev): the threads,
the shard arithmetic and the shared pins all run as they would over 8 GPUs.  Checked against the reference's own Step() (oracle/_ref)
where built, else the C port.  Also here: the Contains target, which the host
calls stage with every chunk of every shard (host.hip host_chunked,
HostIO::whole)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture
def shards(monkeypatch):
    def set_(k):
        monkeypatch.setenv("LIFEAPI_HOST_SHARDS", str(k))
    return set_


@pytest.fixture(scope="module")
def stepper():
    from oracle.oracle import Port, Ref
    return Ref() if Ref.available() else Port()


@pytest.mark.parametrize("k", [2, 3, 8])
@pytest.mark.parametrize("n,gens", [(1, 1), (7, 3), (4099, 1), (20001, 5), (70000, 1)])
def test_sharded_host_step(hip, stepper, shards, k, n, gens):
    shards(k)
    from oracle.oracle import Port
    x = Port().fill(n, seed=900 + n + k)
    got = hip.step_host(x, gens, device=-1)
    assert (got == stepper.step_batch(x, gens)).all()


def test_sharded_in_place_large(hip, stepper, shards):
    # > kPinMinBytes, so the call pins the arrays once for all 4 shard threads
    shards(4)
    from oracle.oracle import Port
    x = Port().fill(40000, seed=4242)
    want = stepper.step_batch(x, 2)
    hip.step_host(x, 2, device=-1, out=x)
    assert (x == want).all()


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("n,gens,keep", [(5, 1, True), (4099, 2, False), (20001, 13, True)])
def test_sharded_host_search_loop(hip, shards, k, n, gens, keep):
    """the search loop (Step + Contains every generation) sharded the same
    way: first-hit generations and final states against the reference's own
    loop (oracle/_ref ref_step_contains_batch) where built, else the port"""
    shards(k)
    from oracle.oracle import Port, Ref
    P = Port()
    w, u = np.zeros(64, np.uint64), np.zeros(64, np.uint64)
    w[10] = w[11] = np.uint64(3 << 40)
    for c in (9, 10, 11, 12):
        u[c] = np.uint64(15 << 39)
    u &= ~w
    x = P.fill(n, seed=300 + n) & P.fill(n, seed=301 + n) & P.fill(n, seed=302 + n)
    clear = np.zeros(64, np.uint64)
    clear[2:20] = np.uint64(0x3FFFF << 32)
    x[::5] = (x[::5] & ~clear) | w
    fin = np.empty_like(x) if keep else None
    first = hip.step_contains_host(x, w, u, gens, final=fin, device=-1)
    if Ref.available():
        want_first, want_fin = Ref().step_contains_batch(x, w, u, gens, nthreads=4)
    else:
        want_first, s = np.zeros(n, np.uint32), x.copy()
        for g in range(1, gens + 1):
            s = P.step_batch(s, 1)
            hit = np.array([P.contains(s[i], w, u) for i in range(n)])
            want_first[(want_first == 0) & hit] = g
        want_fin = s
    assert (first == want_first).all()
    assert (want_first > 0).any()
    if keep:
        assert (fin == want_fin).all()


@pytest.mark.parametrize("k", [2, 3])
def test_sharded_host_forms(hip, shards, k):
    """every other host form (pop, contains, counts, weld, refined, LifeStable
    pass and Vulnerable) sharded the same way equals its one-device result"""
    from oracle.oracle import Port
    P = Port()
    n = 3001
    x = P.fill(n, seed=77) & P.fill(n, seed=78)
    w = x[5].copy()
    one = {"pop": hip.pop_host(x, device=0)}
    shards(k)
    assert (hip.pop_host(x, device=-1) == one["pop"]).all()
    lib, c = hip.lib, __import__("ctypes")

    def call(name, *args):
        hip._check(getattr(lib, name)(*args))

    def host_twice(fn):
        a, b = fn(0), fn(-1)
        assert all((p == q).all() for p, q in zip(a, b))
        return a

    def contains(dev):
        out = np.zeros(n, np.uint8)
        call("lifeapi_contains_batch", x.ctypes.data, w.ctypes.data, w.ctypes.data, out.ctypes.data, n, dev)
        return (out,)
    assert host_twice(contains)[0][5] == 1

    def counts(dev):
        out = np.zeros((n, 4, 64), np.uint64)
        call("lifeapi_neighbour_count_batch", x.ctypes.data, out.ctypes.data, n, dev)
        out3 = np.zeros((n, 3, 64), np.uint64)
        call("lifeapi_interaction_counts_batch", x.ctypes.data, out3.ctypes.data, n, 0, dev)
        return out, out3
    host_twice(counts)

    welds0 = P.fill(n * 4, seed=79).reshape(n, 256)

    def weld(dev):
        wd = welds0.copy()
        call("lifeapi_weld_step_batch", wd.ctypes.data, n, 3, dev)
        return (wd,)
    host_twice(weld)

    planes11 = P.fill(n * 11, seed=80).reshape(n, 11 * 64)

    def refined(dev):
        out = np.zeros((n, 3 * 64), np.uint64)
        call("lifeapi_refined_step_batch", planes11.ctypes.data, out.ctypes.data, n, dev)
        return (out,)
    host_twice(refined)

    st0 = P.fill(n * 10, seed=81).reshape(n, 640)
    st0[:, 128:] &= P.fill(n * 8, seed=82).reshape(n, 512)

    def stable(dev):
        st = st0.copy()
        flags = np.zeros(n, np.uint8)
        call("lifeapi_stable_pass_batch", st.ctypes.data, flags.ctypes.data, n, 3, 0, dev)
        vul = np.zeros((n, 64), np.uint64)
        call("lifeapi_stable_vulnerable_batch", st0.ctypes.data, vul.ctypes.data, n, dev)
        return st, flags, vul
    host_twice(stable)


@pytest.mark.parametrize("device", [0, -1])
def test_sharded_stable_lookahead_host_forms(hip, port, shards, device):
    """The host-pointer forms of the LifeStable lookahead family on 67 objects,
    on one device (two chunks) and in three shards: the 1-byte `columns` and
    `flags`, the per-object `cells` and the one `cells` for the whole batch cut
    where the chunks and shards are cut, every object with a column, a mask and
    an answer of its own; `pass` and `max_iters` as given -- at max_iters = 2
    the model's flags 7 and 4, which the unbounded call does not give.  Against
    the recording and the model (tests/test_stable_test_model.py)."""
    import test_stable_test_model as M
    shards(3)
    rec, n = M.recording(), 67
    strips = M.bounded_strips()
    starts, columns, recorded = M.own_strips()
    # the strip passes: by turns a row that pass 0 changes, one that max_iters = 2 stops in pass 4,
    # and any other
    rng = np.random.default_rng(67)
    slow = np.flatnonzero(strips[4, 2][1] == 7)
    rows = rng.permutation(np.setdiff1d(np.arange(len(starts)), slow))[:n]
    rows[0::3] = rng.permutation(np.flatnonzero(recorded[0][1] == 3))[:len(rows[0::3])]
    rows[1::3] = slow[:len(rows[1::3])]
    thirds = ((0, 22), (22, 44), (44, 67))
    assert len(set(columns[rows].tolist())) >= 24
    given = starts[rows].copy()
    for which in range(6):
        want = recorded[which][0][rows]
        got, fl = hip.stable_strip_pass_host(given, columns[rows], which, device=device)
        assert (fl == recorded[which][1][rows]).all(), which
        assert (got.reshape(n, 10, 64) == want).all(), which
        same = (want == given).all(axis=(1, 2))
        assert all(same[a:c].any() and not same[a:c].all() for a, c in thirds), which
    for which in (4, 5):
        planes, flags = strips[which, 2]
        got, fl = hip.stable_strip_pass_host(given, columns[rows], which, max_iters=2, device=device)
        assert (fl == flags[rows]).all() and (got.reshape(n, 10, 64) == planes[rows]).all(), which
        assert all((fl[a:c] == 7).any() for a, c in thirds), which
    assert (given == starts[rows]).all()
    # TestUnknowns: each object's own cells, and one universe of cells for all
    b = M.bounded_unknowns(port)
    rows = np.arange(n) % len(b.pick)
    after = b.after[rows].copy()
    assert len(b.pick) < n and len({m.tobytes() for m in b.per}) >= 48
    got, fl = hip.stable_test_unknowns_host(after, b.per[rows], device=device)
    assert (fl == rec.tu_flags[b.pick][rows]).all() and (got.reshape(n, 10, 64) == rec.tu[b.pick][rows]).all()
    assert not (fl == 4).any() and (fl == 3).any()
    for form, cells in (("per", b.per[rows]), ("one", b.one)):
        planes, flags, _ = b.want[form, 2]
        got, fl = hip.stable_test_unknowns_host(after, cells, max_iters=2, device=device)
        assert (fl == flags[rows]).all() and (got.reshape(n, 10, 64) == planes[rows]).all(), form
        assert all((fl[a:c] == 4).any() and (fl[a:c] != 4).any() for a, c in thirds), form
    assert (after == b.after[rows]).all()
    # PropagateAndTest
    p = M.bounded_propagate_and_test(port)
    rows = np.arange(0, len(p.given), 3)
    assert len(rows) == n
    given = p.given[rows].copy()
    got, fl = hip.stable_propagate_and_test_host(given, device=device)
    assert (fl == p.free[1][rows]).all() and (got.reshape(n, 10, 64) == p.free[0][rows]).all()
    assert not (fl == 4).any()
    planes, flags, _ = p.want[2]
    got, fl = hip.stable_propagate_and_test_host(given, max_iters=2, device=device)
    assert (fl == flags[rows]).all() and (got.reshape(n, 10, 64) == planes[rows]).all()
    assert all((fl[a:c] == 4).any() and (fl[a:c] != 4).any() for a, c in thirds)
    assert (given == p.given[rows]).all()


def _block_and_ring():
    blk, ring = np.zeros(64, np.uint64), np.zeros(64, np.uint64)
    blk[20] = blk[21] = np.uint64(0b11 << 30)
    for c in (19, 20, 21, 22):
        ring[c] = np.uint64(0b1111 << 29)
    return blk, ring & ~blk


def _contains_host(hip, x, wanted, unwanted, device=0):
    out = np.full(len(x), 7, np.uint8)
    hip._check(hip.lib.lifeapi_contains_batch(x.ctypes.data, wanted.ctypes.data, unwanted.ctypes.data,
                                              out.ctypes.data, len(x), device))
    return out


@pytest.fixture(scope="module")
def three_chunks():
    """Sparse soups with the block-and-ring target planted every tenth
    universe, as test_gpu_parity.test_host_step_contains builds them, and the
    oracle's Contains and 2-generation search loop.  512 + 256 staged bytes
    per universe and 64 MiB chunks: 87,381 universes per chunk, so 180,001 is
    three chunks on two lanes (the third reuses the first's buffer, target
    slots included) and the last chunk is ragged."""
    from oracle.oracle import Port, Ref
    P, n = Port(), 180_001
    blk, ring = _block_and_ring()
    x = P.fill(n, seed=61) & P.fill(n, seed=62) & P.fill(n, seed=63)
    x[::5] &= ~ring & ~blk
    x[::10] |= blk
    if Ref.available():
        R = Ref()
        hit = R.contains_batch(x, blk, ring)
        first, fin = R.step_contains_batch(x, blk, ring, 2, nthreads=8)
    else:
        def contains(s):
            return (((s ^ blk) & (blk | ring)) == 0).all(axis=1)
        hit = contains(x).astype(np.uint8)
        first, fin = np.zeros(n, np.uint32), x
        for g in (1, 2):
            fin = P.step_batch(fin, 1, nthreads=8)
            first[(first == 0) & contains(fin)] = g
    for want in (hit, first):  # the first and the third chunk both have hits to lose
        assert want[:200].any() and want[-200:].any()
    for a in (x, hit, first, fin):
        a.flags.writeable = False
    return x, blk, ring, hit, first, fin


@pytest.mark.parametrize("device,k", [(0, None), (-1, 3)])
def test_target_restaged_across_lane_reuse(hip, three_chunks, shards, device, k):
    """the target is staged with every chunk (host.hip host_chunked): every
    chunk of a three-chunk call, and every shard, tests against it"""
    if k:
        shards(k)
    x, blk, ring, hit, first, fin = three_chunks
    assert (_contains_host(hip, x, blk, ring, device) == hit).all()
    assert (hip.step_contains_host(x, blk, ring, 2, device=device) == first).all()
    y = x.copy()
    assert (hip.step_contains_host(y, blk, ring, 2, final=y, device=device) == first).all()
    assert (y == fin).all()


def test_no_stale_target(hip):
    """consecutive host Contains calls on the same states: each result follows
    the target current at its call, whether the second target is another pair
    of arrays or the first pair rewritten in place"""
    from oracle.oracle import Port
    P, n = Port(), 2001
    x = P.fill(n, seed=71) & P.fill(n, seed=72)
    blk, ring = _block_and_ring()
    x[::10] = (x[::10] & ~ring) | blk
    targets = [(blk, ring), (x[7] & x[8], ~(x[7] | x[8]) & ring)]
    want = [np.array([P.contains(s, w, u) for s in x], np.uint8) for w, u in targets]
    assert all(0 < e.sum() < n for e in want) and (want[0] != want[1]).any()
    for e, (w, u) in zip(want, targets):
        assert (_contains_host(hip, x, w, u) == e).all()
    w, u = np.empty(64, np.uint64), np.empty(64, np.uint64)
    for k in (0, 1, 0):
        w[:], u[:] = targets[k]
        assert (_contains_host(hip, x, w, u) == want[k]).all()


def _at_4_mod_8(a):
    """a copy of uint64 array `a` at an address that is 4 mod 8"""
    buf = np.zeros(a.nbytes + 8, np.uint8)
    at = (4 - buf.ctypes.data) % 8
    b = buf[at:at + a.nbytes].view(np.uint64).reshape(a.shape)
    b[...] = a
    assert b.ctypes.data % 8 == 4
    return b


def test_unaligned_target_arrays(hip):
    """wanted / unwanted at an address that is 4 mod 8 are accepted (they are
    copied to 8-byte-aligned device memory); states there are rejected"""
    from oracle.oracle import Port
    P, n = Port(), 5
    x = P.fill(n, seed=81) & P.fill(n, seed=82)
    blk, ring = _block_and_ring()
    x[1::2] = (x[1::2] & ~ring) | blk
    want = np.array([P.contains(s, blk, ring) for s in x], np.uint8)
    assert want.any() and not want.all()
    assert (_contains_host(hip, x, _at_4_mod_8(blk), _at_4_mod_8(ring)) == want).all()
    with pytest.raises(hip.LifeApiError) as e:
        _contains_host(hip, _at_4_mod_8(x), blk, ring)
    assert e.value.code == -1  # LIFEAPI_E_INVALID


def test_bad_device_index(hip):
    x = np.zeros((2, 64), np.uint64)
    with pytest.raises(hip.LifeApiError) as e:
        hip.step_host(x, 1, device=hip.device_count())
    assert e.value.code == -2
    with pytest.raises(hip.LifeApiError):
        hip.step_host(x, 1, device=-2)


@pytest.mark.parametrize("bad", ["0", "65", "100000", "-3", "4x", " "])
def test_shard_override_rejects_bad_values(hip, shards, bad):
    """LIFEAPI_HOST_SHARDS outside 1..64 (or not an integer) is a caller
    error, not a request for that many threads (host.hip over_devices)"""
    shards(bad)
    from oracle.oracle import Port
    x = Port().fill(5, seed=5)
    with pytest.raises(hip.LifeApiError) as e:
        hip.step_host(x, 1, device=-1)
    assert e.value.code == -1 and "LIFEAPI_HOST_SHARDS" in str(e.value)  # LIFEAPI_E_INVALID


def test_shard_override_empty_means_unset(hip, stepper, shards):
    """`export LIFEAPI_HOST_SHARDS=` leaves the variable set but empty: that
    is no override (one shard per visible device), not an error"""
    shards("")
    from oracle.oracle import Port
    x = Port().fill(7, seed=77)
    assert (hip.step_host(x, 3, device=-1) == stepper.step_batch(x, 3)).all()


def test_shard_override_capped_at_n(hip, stepper, shards):
    """more shards than universes: one shard per universe, no empty shards"""
    shards(64)
    from oracle.oracle import Port
    x = Port().fill(3, seed=33)
    assert (hip.step_host(x, 2, device=-1) == stepper.step_batch(x, 2)).all()
