"""The LifeStable fragment networks on every input row they can be given.

The count / signal / vulnerable networks are exact only on the care set
(tools/cgp_stable.py reachable_rows).  Here: the care set is exactly what
neighbourhoods can produce (by enumeration); a seeded batch of probes
(tests/stable_rows.py covering_batch) presents every care row -- asserted
with the row model before anything runs; the oracle equals the reference on
that batch; the kernels equal the oracle on it, pass by pass and composed,
through k_stable_dma and through k_stable; and single-bit mutants of the
truth tables, run through the oracle on the same boards, say how much of
each row the boards can see.
"""
import time

import numpy as np
import pytest

import stable_rows as sr

PASSES = ("sync", "options", "signal", "step", "propagate", "stabilise")
OWN_PASS = {"count": 1, "signal": 2}        # the pass that evaluates the fragment's network


@pytest.fixture(scope="module")
def tt():
    return sr.tables()


@pytest.fixture(scope="module")
def batches(tt):
    out = {}
    for f in sr.FRAGMENTS:
        t0 = time.process_time()
        out[f] = sr.covering_batch(f, tt)
        print(f"covering_batch({f}): {len(out[f].planes)} boards ({out[f].packed} packed, "
              f"{len(out[f].planes) - out[f].packed} of one probe), {out[f].planes.nbytes / 2**20:.1f} MiB, "
              f"{time.process_time() - t0:.2f} s CPU")
    return out


@pytest.fixture(scope="module")
def expected(port, batches):
    """the oracle's answers on the batches, computed once: expected(fragment)
    -> {pass name: (planes, flags), "vulnerable": of the raw planes,
    "vulnerable_propagated": of Propagate's}"""
    cache = {}

    def get(f):
        if f not in cache:
            x = batches[f].planes
            e = {name: port.stable_pass(x, w) for w, name in enumerate(PASSES)}
            e["vulnerable"] = port.stable_vulnerable(x)
            e["vulnerable_propagated"] = port.stable_vulnerable(e["propagate"][0])
            cache[f] = e
        return cache[f]
    return get


# ---- CPU: the care set, the batch's coverage, the oracle ----

def test_care_set_is_the_enumerated_row_set():
    """All 4^9 neighbourhoods of (state, unknown) cells, options free: the
    rows they present are exactly reachable_rows -- nothing the kernels can
    see is missing from the care set, and nothing in it is unreachable (the
    networks give up exactness on no row for nothing)."""
    got = sr.enumerated_rows()
    for f, n in (("count", 132), ("signal", 176 * 256), ("vulnerable", 80 * 256)):
        care = sr.care_rows(f)
        assert len(care) == n, f
        assert np.array_equal(got[f], care), (f, len(got[f]), len(care))


@pytest.mark.parametrize("fragment", sr.FRAGMENTS)
def test_covering_batch_presents_every_care_row(batches, fragment):
    """rows_of the batch, every cell of every board, is a superset of the
    care set -- all of it -- and within it (the boards are real planes); each
    probe's row is on the board the batch says it is on."""
    b = batches[fragment]
    care = sr.care_rows(fragment)
    assert b.planes.nbytes < 300 << 20
    seen = []
    for lo in range(0, len(b.planes), 256):
        rows = sr.rows_of(b.planes[lo:lo + 256], (fragment,))[fragment]
        have = np.unique((np.arange(lo, lo + len(rows), dtype=np.int64)[:, None, None] << 20 | rows).ravel())
        m = (b.probe_board >= lo) & (b.probe_board < lo + 256)
        assert np.isin(b.probe_board[m].astype(np.int64) << 20 | b.probe_row[m], have).all(), (fragment, lo)
        seen.append(np.unique(have & 0xFFFFF))
    seen = np.unique(np.concatenate(seen))
    missing = np.setdiff1d(care, seen)
    assert len(missing) == 0, (fragment, len(missing), missing[:8])
    assert len(np.setdiff1d(seen, care)) == 0, fragment
    assert set(b.probe_row.tolist()) == set(care.tolist()), fragment


@pytest.mark.parametrize("fragment", ["count", "signal"])
def test_every_row_is_seen_by_its_pass_verdict(port, batches, expected, fragment):
    """A pass gives one flag per board, and SignalNeighbours leaves an
    inconsistent board's planes alone: every care row sits on a board its
    pass finds consistent (so the planes show what the row did), or alone on
    its board (so the verdict is the row's).  The packed boards the builder
    judged consistent are, by the oracle; so the builder's restatement of the
    verdict holds there, and on the boards of one probe too."""
    b = batches[fragment]
    _, fl = expected(fragment)[PASSES[OWN_PASS[fragment]]]
    ok = (fl & 1).astype(bool)
    packed_clean = b.packed if fragment == "signal" else b.packed - 1  # count's last packed board: every probe
    assert ok[:packed_clean].all(), (fragment, np.nonzero(~ok[:packed_clean])[0][:8])
    assert not ok[b.packed:].any(), (fragment, np.nonzero(ok[b.packed:])[0][:8])
    for row, boards in b.boards_of().items():
        assert any(ok[k] or b.alone(k) for k in boards), (fragment, row, boards)
    print(f"{fragment}: {len(fl) - b.packed} boards of one probe, {b.packed} packed")


@pytest.mark.parametrize("fragment", sr.FRAGMENTS)
def test_oracle_equals_reference_on_covering_batch(ref, batches, expected, fragment):
    """The C restatement is pinned to the reference on sampled planes
    elsewhere; here on every care row: all six passes and Vulnerable through
    the reference's own LifeStable, planes and flags."""
    b, e = batches[fragment], expected(fragment)
    for w, name in enumerate(PASSES):
        got = b.planes.copy()
        fl = np.array([ref.stable_pass(got[u], w) for u in range(len(got))], np.uint8)
        _same(got, e[name][0], b, fragment, name, "reference")
        _same(fl, e[name][1], b, fragment, name + " flags", "reference")
    for key, x in (("vulnerable", b.planes), ("vulnerable_propagated", e["propagate"][0])):
        got = np.stack([ref.stable_vulnerable(x[u]) for u in range(len(x))])
        _same(got, e[key], b, fragment, key, "reference")


def _same(got, want, batch, fragment, what, how):
    """got == want, or say which fragment, pass, form and board (with the
    care rows its probes hold) differ first"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (fragment, what, how, got.shape, want.shape)
    if (got == want).all():
        return
    bad = np.nonzero((got != want).reshape(len(got), -1).any(axis=1))[0]
    k = int(bad[0])
    pytest.fail(f"{fragment} batch, {what}, {how}: {len(bad)} of {len(got)} boards differ; first board {k} "
                f"({'one probe' if batch.alone(k) else 'packed'}) holds rows {batch.rows_on(k)}", pytrace=False)


# ---- GPU: the kernels on every care row ----

ALIGNMENTS = ((0, "16-byte aligned (k_stable_dma but Propagate)"), (1, "8 mod 16 (k_stable)"))


def _dev(planes, offset):
    """the planes on the device, the batch at 16 | 8 mod 16 bytes"""
    import torch
    n = len(planes)
    buf = torch.empty(n * 640 + 2, dtype=torch.int64, device="cuda")
    d = buf[offset: offset + n * 640].view(n, 640)
    assert (d.data_ptr() % 16 == 0) == (offset == 0)
    d.copy_(torch.from_numpy(np.ascontiguousarray(planes).view(np.int64).reshape(n, 640)))
    return d


def _host(t, width):
    return t.cpu().numpy().view(np.uint64).reshape(-1, width)


def _gpu_pass(hip, x, name, offset):
    d = _dev(x, offset)
    fl = hip.stable_pass(d, name).cpu().numpy()
    return _host(d, 640), fl


def _gpu_vulnerable(hip, x, offset):
    return _host(hip.stable_vulnerable(_dev(x, offset)), 64)


@pytest.mark.gpu
@pytest.mark.parametrize("fragment", sr.FRAGMENTS)
def test_own_pass_on_every_care_row(hip, batches, expected, fragment):
    """Each network's own pass alone on its batch: UpdateOptions on count's,
    SignalNeighbours on signal's, Vulnerable on vulnerable's; planes and
    flags word for word, both kernels."""
    b, e = batches[fragment], expected(fragment)
    for offset, how in ALIGNMENTS:
        if fragment == "vulnerable":
            _same(_gpu_vulnerable(hip, b.planes, offset), e["vulnerable"], b, fragment, "Vulnerable", how)
        else:
            name = PASSES[OWN_PASS[fragment]]
            got, fl = _gpu_pass(hip, b.planes, name, offset)
            _same(got, e[name][0], b, fragment, name, how)
            _same(fl, e[name][1], b, fragment, name + " flags", how)


@pytest.mark.gpu
@pytest.mark.parametrize("fragment", sr.FRAGMENTS)
def test_every_pass_on_every_batch(hip, batches, expected, fragment):
    """Every batch through all six passes (PropagateStep forms the signal
    network's counts as 9 - NeighbourCount(off); Propagate and
    StabiliseOptions iterate), and Vulnerable on the raw and on the
    propagated planes; both kernels."""
    b, e = batches[fragment], expected(fragment)
    for offset, how in ALIGNMENTS:
        for name in hip.STABLE_PASSES:
            got, fl = _gpu_pass(hip, b.planes, name, offset)
            _same(got, e[name][0], b, fragment, name, how)
            _same(fl, e[name][1], b, fragment, name + " flags", how)
        _same(_gpu_vulnerable(hip, b.planes, offset), e["vulnerable"], b, fragment, "Vulnerable", how)
        _same(_gpu_vulnerable(hip, e["propagate"][0], offset), e["vulnerable_propagated"], b, fragment,
              "Vulnerable of the propagated planes", how)
    assert tuple(hip.STABLE_PASSES) == PASSES


# ---- how sharp is the batch: single-bit mutants of the tables, through the oracle ----

# A mutant is a fragment's truth table with one output inverted at one care
# row; it is killed if the oracle with that table, run (the fragment's own
# pass) on the boards that hold the row's probes, gives other planes, flags or
# Vulnerable output than with the real table.  Every count row; of the signal
# and vulnerable rows those whose option byte is a multiple of OPTION_STEP = 3
# (86 of the 256 bytes, every option bit both ways), which keeps the run to a
# few seconds.  Measured with the oracle and the reference's tables only -- no
# kernel is involved -- and guarded: killed mutants per output, of the mutants
# run.  What survives, and why no LifeStable could tell:
#   count    the eight option outputs: none survive.  abort: probes that have
#            an aborting neighbour in every arrangement tried (a known cell
#            with too many neighbours on or off shares them with its
#            neighbours): the board's flag is 0 with or without the centre's
#            abort.
#   signal   signaloff / signalon reach only the 8 neighbours, and only
#            unknown ones take them: survivors have no unknown neighbour, or
#            a neighbour already signalled the same way by another cell of
#            the probe (the ZOI is an OR), or sit on a board of one probe that
#            stays inconsistent (a clash elsewhere in the probe: the planes
#            are not written).  centeroff / centeron act on the centre only
#            where it is unknown: every row with a known centre survives
#            (half of the rows), plus the inconsistent boards as above.
#   vulnerable  the result is (ZOI(on) | center_on) & (ZOI(off) | center_off):
#            a flip on one side shows only in a cell where the other side is
#            1 and, for a flip to 0, where no other cell of the probe raises
#            the same side.  The probes come with their neighbours' options
#            open, half, mostly open and mostly ruled out
#            (stable_rows.NB_OPTION_DENSITY) to open that gate more often;
#            with the neighbours' options all open only, 16 % of
#            vulnerable_on and 4 % of vulnerable_center_on mutants died.
OPTION_STEP = 3
KILLED = {
    "count": ((132, 132),) * 8 + ((97, 132),),
    # signaloff 76 %, signalon 83 %, centeroff 42 %, centeron 45 % (85 % and 89 % of the unknown centres)
    "signal": ((11451, 15136), (12561, 15136), (6420, 15136), (6764, 15136)),
    # vulnerable_on 73 %, vulnerable_off 81 %, vulnerable_center_on 50 %, vulnerable_center_off 75 %
    "vulnerable": ((5030, 6880), (5539, 6880), (3468, 6880), (5139, 6880)),
}


def _mutant_kills(port, batch, tt, step):
    """[(killed, run)] per output of the fragment"""
    import ctypes
    f = batch.fragment
    u8, u64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64)
    tab = tt[f]
    if f == "vulnerable":
        base, bfl = sr.oracle_vulnerable(port, batch.planes, tt), None
    else:
        base, bfl = sr.oracle_pass(port, batch.planes, OWN_PASS[f], tt)
    tc, ts, tv = (tt[k].ctypes.data_as(u8) for k in sr.FRAGMENTS)
    work, out = np.zeros(640, np.uint64), np.zeros(64, np.uint64)
    wp, op = work.ctypes.data_as(u64), out.ctypes.data_as(u64)
    killed, run = [0] * len(tab), [0] * len(tab)
    for row, boards in batch.boards_of().items():
        if f != "count" and (row & 0xFF) % step:
            continue
        for k in range(len(tab)):
            tab[k, row] ^= 1
            dead = False
            for bd in boards:
                if f == "vulnerable":
                    port.lib.oracle_stable_vulnerable(batch.planes[bd].ctypes.data_as(u64), op, tv)
                    dead = not np.array_equal(out, base[bd])
                else:
                    work[:] = batch.planes[bd]
                    fl = port.lib.oracle_stable_pass(wp, OWN_PASS[f], tc, ts)
                    dead = fl != bfl[bd] or not np.array_equal(work, base[bd])
                if dead:
                    break
            tab[k, row] ^= 1
            run[k] += 1
            killed[k] += bool(dead)
    return list(zip(killed, run))


@pytest.mark.parametrize("fragment", sr.FRAGMENTS)
def test_mutant_kill_rate_does_not_fall(port, batches, fragment):
    """Single-bit mutants of the fragment's table on its covering batch (see
    KILLED): as many die as when the batch was built -- a change to the
    builder that makes the boards see less of a row fails here."""
    tt = sr.tables()   # a private copy: the mutants are written into it
    got = _mutant_kills(port, batches[fragment], tt, OPTION_STEP)
    assert all((tt[f] == t).all() for f, t in sr.tables().items())
    print(f"{fragment}: killed / run per output: {got}")
    want = KILLED[fragment]
    assert len(got) == len(want)
    for k, ((killed, run), (killed0, run0)) in enumerate(zip(got, want)):
        assert run == run0 and killed >= killed0, (fragment, k, got)
