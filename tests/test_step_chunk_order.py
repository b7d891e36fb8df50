"""CPU: the index arithmetic of the streaming step's launch order
(lifeapi_amd/csrc/step_order.hpp step_take, what k_step's waves run on the
device), compiled into a host program (tests/cpp/step_chunk_order_probe.cpp)
and checked for every wave of every one-shot grid of 1..40 blocks -- every
grid size mod 8, grids smaller than the 8 XCDs included -- with each of the
four group counts that need that grid (ragged against the 4 waves of a
block), chunked and not, forward and reversed, with a plain-stored tail of 0,
1, half and all of the groups.

Store policy never changes a result, so no GPU test can tell which groups a
launch stored plain; this one can."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_BLOCKS = 40
WPB = 4  # common.hpp kWavesPerBlock
COLS = ("nb", "groups", "chunk", "reverse", "plain_from", "b", "wib", "place", "index", "group", "plain")


@pytest.fixture(scope="module")
def launches(tmp_path_factory):
    """{(nb, groups, chunk, reverse, plain_from): rows of the probe, one per
    wave in dispatch order, as a dict of column arrays}"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("step_chunk_order") / "probe")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                    "-I" + os.path.join(ROOT, "lifeapi_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "step_chunk_order_probe.cpp"), "-o", exe], check=True)
    text = subprocess.run([exe, str(MAX_BLOCKS)], check=True, capture_output=True, text=True).stdout
    rows = np.array(text.split(), dtype=np.int64).reshape(-1, len(COLS))
    out = {}
    key = rows[:, :5]
    cuts = np.nonzero((key[1:] != key[:-1]).any(axis=1))[0] + 1
    for part in np.split(rows, cuts):
        k = tuple(int(v) for v in part[0, :5])
        assert k not in out
        out[k] = {c: part[:, i] for i, c in enumerate(COLS)}
        # one line per wave, in dispatch order
        assert (part[:, 5] * WPB + part[:, 6] == np.arange(k[0] * WPB)).all(), k
    assert {k[0] for k in out} == set(range(1, MAX_BLOCKS + 1))
    for nb in range(1, MAX_BLOCKS + 1):  # every ragged group count of the grid
        assert {k[1] for k in out if k[0] == nb} == set(range(4 * nb - 3, 4 * nb + 1))
    return out


def test_place_is_a_bijection(launches):
    """(a) block -> place is onto the grid, chunked and not; and so the waves
    that take a group take every group exactly once, in either order"""
    for k, r in launches.items():
        nb, groups = k[0], k[1]
        assert sorted(r["place"][::WPB]) == list(range(nb)), k
        assert (r["index"] == r["place"] * WPB + r["wib"]).all(), k
        taken = r["group"][r["index"] < groups]
        assert sorted(taken) == list(range(groups)), k
        assert (r["group"][r["index"] >= groups] == -1).all(), k


def test_each_xcd_takes_one_contiguous_run(launches):
    """(b) under chunks the places of XCD x (blocks x, x + 8, ...) are one
    contiguous run, taken in ascending order, and the runs follow one another
    in the order of the XCDs"""
    for k, r in launches.items():
        if not k[2]:
            continue
        place, end = r["place"][::WPB], 0
        for x in range(8):
            run = place[x::8]
            assert (run == end + np.arange(len(run))).all(), (k, x)
            end += len(run)
        assert end == k[0]


def test_reversed_launch_mirrors_the_forward_one(launches):
    """(c) a reversed launch takes at every wave the group the forward launch
    took at the wave with the mirrored index (groups - 1 - index); on a grid
    of 8q blocks filled with groups that is exactly: dispatch position t of
    XCD x takes what position T - 1 - t of XCD 7 - x took forward."""
    for k, r in launches.items():
        nb, groups, chunk, reverse, plain_from = k
        if not reverse:
            continue
        fwd = launches[(nb, groups, chunk, 0, plain_from)]
        ok = r["index"] < groups
        assert (fwd["index"] == r["index"]).all() and (fwd["group"][ok] == r["index"][ok]).all(), k
        assert (r["group"][ok] == groups - 1 - r["index"][ok]).all(), k
        if chunk and nb % 8 == 0 and groups == nb * WPB:
            q = nb // 8
            for b in range(nb):
                x, i = b % 8, b // 8
                for wib in range(WPB):  # t = i * WPB + wib of T = q * WPB
                    mirror = ((7 - x) + 8 * (q - 1 - i)) * WPB + (WPB - 1 - wib)
                    assert r["group"][b * WPB + wib] == fwd["group"][mirror], (k, b, wib)


@pytest.mark.parametrize("upw", [4, 8])
def test_plain_tail_is_the_end_of_the_dispatch(launches, upw):
    """(d) the plain-stored groups are exactly those taken at dispatch
    positions >= plain_from; under chunks they are the end of every XCD's run;
    and they cover the requested tail: at least the requested number of groups
    (launch.hpp launch_order rounds the bytes up to groups), so at least the
    requested bytes -- less only what the batch's one ragged group falls short
    of a full one where it lies in the tail, as in the unchunked order."""
    for k, r in launches.items():
        nb, groups, chunk, reverse, plain_from = k
        pos = r["b"] * WPB + r["wib"]
        assert (r["plain"] == (pos >= plain_from)).all(), k
        ok = r["index"] < groups
        plain_groups = r["group"][ok & (r["plain"] == 1)]
        tail = groups - plain_from  # what the launcher asked for, in groups
        assert len(plain_groups) >= tail, k
        if not chunk:
            assert len(plain_groups) == tail, k
        else:
            for x in range(8):  # a suffix of each XCD's blocks
                flags = r["plain"][::WPB][x::8], r["plain"][WPB - 1::WPB][x::8]
                for f in flags:
                    assert (np.diff(f) >= 0).all(), (k, x)
        for short in (0, upw - 1):  # n a multiple of upw, and one universe in the last group
            n = groups * upw - short
            size = np.full(groups, upw)
            size[-1] -= short
            for asked in {max(tail * upw * 512 - 511, 0), tail * upw * 512}:  # both round up to `tail` groups
                asked = min(asked, n * 512)
                assert size[plain_groups].sum() * 512 >= asked - short * 512, (k, n, asked)
                if short == 0:
                    assert size[plain_groups].sum() * 512 >= asked, (k, n, asked)


def test_unchunked_is_the_former_arithmetic(launches):
    """(e) with chunks off: wave b * 4 + wib takes group grp = b * 4 + wib
    (reversed: groups - 1 - grp) and stores it plain unless grp < plain_from"""
    for k, r in launches.items():
        nb, groups, chunk, reverse, plain_from = k
        if chunk:
            continue
        grp = r["b"] * WPB + r["wib"]
        assert (r["place"] == r["b"]).all() and (r["index"] == grp).all(), k
        ok = grp < groups
        assert (r["group"][ok] == (groups - 1 - grp[ok] if reverse else grp[ok])).all(), k
        assert (r["plain"] == ~(grp < plain_from)).all(), k
