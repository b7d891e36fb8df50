"""GPU: the streaming step with each XCD on a contiguous eighth of the batch
AND a plain-stored tail (step_kernels.hpp step_body through step_order.hpp
step_take: the tail by dispatch position, the end of every XCD's eighth).
Store policy never changes a result, so these tests hold the results of every
combination to the oracle word for word; which groups are stored plain is
tests/test_step_chunk_order.py's to check, on the host."""
import os
import sys

import numpy as np
import pytest
import torch

from test_gpu_parity import seam_cases, to_dev, to_host

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "tune"))

# 4099 at 4 per wave: 1025 groups in 257 blocks, no multiple of the 8 XCDs;
# 33 / 32 / 31 and 9 / 8 / 7: the 4-wave block edge at 8 and the group edge;
# grids smaller than the 8 XCDs from 33 down
SIZES = [4099, 33, 32, 31, 9, 8, 7, 1]
NMAX = max(SIZES)
GENS = (0, 1, 2)


@pytest.fixture(scope="module")
def tune(hip):
    import tune_hip
    return tune_hip


@pytest.fixture(scope="module")
def small(port):
    """(x, {gens: x stepped}) for NMAX universes; a test takes the first n of
    each (universes are independent).  Read-only."""
    x = np.concatenate([seam_cases(port), port.fill(NMAX, seed=1717)])[:NMAX]
    want = {0: x.copy(), 1: port.step_batch(x, 1, nthreads=8), 2: port.step_batch(x, 2, nthreads=8)}
    for a in (x, *want.values()):
        a.setflags(write=False)
    return x, want


def tails(n, upw):
    """no plain tail, one group, half the batch, everything"""
    return (0, upw * 512, n * 512 // 2, n * 512)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("upw", [4, 8])
def test_chunked_step_with_a_plain_tail(tune, small, upw, n):
    x, want = small
    d = to_dev(x[:n])
    out = torch.empty_like(d)
    for gens in GENS:
        for reverse in (False, True):
            for plain in tails(n, upw):
                out.fill_(-1)
                tune.step_order(d, out, gens, reverse=reverse, nts=True, resident=0, upw=upw, plain_bytes=plain,
                                xcd_chunk=True)
                bad = np.nonzero((to_host(out) != want[gens][:n]).any(axis=1))[0]
                assert bad.size == 0, (gens, reverse, plain, bad[:8])
    assert (to_host(d) == x[:n]).all()  # (the input untouched)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("upw", [4, 8])
def test_chunked_step_in_place(tune, small, upw, n):
    x, want = small
    for gens in GENS:
        for reverse in (False, True):
            for plain in tails(n, upw):
                d = to_dev(x[:n])
                tune.step_order(d, d, gens, reverse=reverse, nts=True, resident=0, upw=upw, plain_bytes=plain,
                                xcd_chunk=True)
                assert (to_host(d) == want[gens][:n]).all(), (gens, reverse, plain)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("upw", [4, 8])
def test_chunked_step_on_offset_views(tune, small, upw, n):
    """input and output 8 bytes off a 16-byte boundary; the words around the
    output stay as they were"""
    x, want = small
    src = torch.zeros(n * 64 + 2, dtype=torch.int64, device="cuda")
    dst = torch.full((n * 64 + 2,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    d, out = src[1:-1].view(n, 64), dst[1:-1].view(n, 64)
    assert d.data_ptr() % 16 == 8 and out.data_ptr() % 16 == 8
    d.copy_(to_dev(x[:n]))
    for gens in GENS:
        for reverse in (False, True):
            for plain in tails(n, upw):
                out.fill_(-1)
                tune.step_order(d, out, gens, reverse=reverse, nts=True, resident=0, upw=upw, plain_bytes=plain,
                                xcd_chunk=True)
                assert (to_host(out) == want[gens][:n]).all(), (gens, reverse, plain)
    torch.cuda.synchronize()
    assert dst[0].item() == 0x5A5A5A5A and dst[-1].item() == 0x5A5A5A5A


def test_product_chunked_step_alternates(hip, port, tune):
    """hip.step at the smallest batch at which the shipped policy sets XCD
    chunks (step.hip kChunkMinUniverses) plus 5 universes, so ragged against 4
    per wave and a grid that is no multiple of 8: four launches ping-pong and
    two in place run reversed, forward, reversed, forward after an input
    recorded as written forward -- asserted through the order book -- with
    the plain tail live; every result against the oracle, compared on the
    device"""
    from test_launch_paths import Book, source_constant
    n = source_constant("kChunkMinUniverses") + 5
    assert n >= source_constant("kOrderMinUniverses") and n < source_constant("kChunkStopUniverses")
    assert n % 4 and ((n + 3) // 4 + 3) // 4 % 8
    x = port.fill(n, seed=1718)
    want = [x]
    for _ in range(4):
        want.append(port.step_batch(want[-1], 1, nthreads=16))
    want = [to_dev(w) for w in want]
    book = Book(tune, n * 512)
    a, b = want[0].clone(), torch.zeros((n, 64), dtype=torch.int64, device="cuda")
    book.note_forward(a)
    orders = []
    for k in range(1, 5):
        hip.step(a, out=b, generations=1)
        orders.append(book.ran_reversed(b))
        assert torch.equal(b, want[k]), ("ping-pong", k)
        a, b = b, a
    assert orders == [True, False, True, False]
    del a, b
    d = want[0].clone()
    book.note_forward(d)
    orders = []
    for k in range(1, 3):
        hip.step(d, out=d, generations=1)
        orders.append(book.ran_reversed(d))
        assert torch.equal(d, want[k]), ("in place", k)
    assert orders == [True, False]
