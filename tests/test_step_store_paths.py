"""The streaming step's two paths (step_kernels.hpp step_group): full groups
of U universes load and store unconditionally, the ragged last group keeps
its guards -- every batch size around the group and block edges, either group
order (reversed, the ragged group is the first one taken), every plain-stored
tail, in place and on views 8 bytes off a 16-byte boundary, bit-exact against
the C oracle (and the reference build where it exists).  Round 6's body
(tools/tune/step_r6.hpp, the A/B's other side) passes the same cases."""
import os
import sys

import numpy as np
import pytest
import torch

from test_gpu_parity import seam_cases, to_dev, to_host

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "tune"))

# n < U, n = 0, 1 and U - 1 mod U for U = 4 and 8, the 4-wave block edge
# (16 / 32 universes +- 1), and smoke()'s size
SIZES = [1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 4099]
NMAX = max(SIZES)
GENS = (0, 1, 2)
BIG = (3 << 16) + 5  # step.hip kOrderMinUniverses + 5: the alternating order and the plain tail are live


@pytest.fixture(scope="module")
def tune(hip):
    import tune_hip
    return tune_hip


@pytest.fixture(scope="module")
def small(port):
    """(x, {gens: x stepped}) for NMAX universes; a test takes the first n of
    each (universes are independent).  Read-only."""
    from oracle.oracle import Ref
    x = np.concatenate([seam_cases(port), port.fill(NMAX, seed=777)])[:NMAX]
    want = {0: x.copy()}
    for g in (1, 2, 3):
        want[g] = port.step_batch(x, g, nthreads=8)
        if Ref.available():
            assert (Ref().step_batch(x, g, nthreads=8) == want[g]).all()
    for a in (x, *want.values()):
        a.setflags(write=False)
    return x, want


@pytest.fixture(scope="module")
def big(port):
    """BIG universes and their first three generations."""
    from oracle.oracle import Ref
    x = port.fill(BIG, seed=778)
    want = [x]
    for _ in range(3):
        want.append(port.step_batch(want[-1], 1, nthreads=8))
    if Ref.available():
        assert (Ref().step_batch(x, 2, nthreads=8) == want[2]).all()
    for a in want:
        a.setflags(write=False)
    return want


def plain_cases(n, upw):
    """no plain tail, one group, half the batch (for odd n a cut inside a
    group, rounded up to whole groups), everything"""
    return (0, upw * 512, n * 512 // 2, n * 512)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("upw", [4, 8])
@pytest.mark.parametrize("body", ["r7", "r6"])
def test_step_order_paths(tune, small, body, upw, n):
    x, want = small
    d = to_dev(x[:n])
    out = torch.empty_like(d)
    for gens in GENS:
        for reverse in (False, True):
            for plain in plain_cases(n, upw):
                for nts in (False, True):
                    out.fill_(-1)
                    tune.step_order(d, out, gens, reverse=reverse, nts=nts, resident=0, upw=upw, plain_bytes=plain,
                                    body=body)
                    bad = np.nonzero((to_host(out) != want[gens][:n]).any(axis=1))[0]
                    assert bad.size == 0, (gens, reverse, plain, nts, bad[:8])
    assert (to_host(d) == x[:n]).all()  # (the input untouched)


@pytest.mark.parametrize("body", ["r7", "r6"])
def test_step_order_xcd_chunk(tune, small, body):
    """8 per wave at 4099 universes: 513 groups in 129 blocks, no multiple of
    the 8 XCDs"""
    x, want = small
    d = to_dev(x)
    out = torch.empty_like(d)
    for gens in GENS:
        for reverse in (False, True):
            for plain in plain_cases(NMAX, 8):
                out.fill_(-1)
                tune.step_order(d, out, gens, reverse=reverse, nts=True, resident=0, upw=8, plain_bytes=plain,
                                xcd_chunk=True, body=body)
                assert (to_host(out) == want[gens]).all(), (gens, reverse, plain)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("upw", [4, 8])
@pytest.mark.parametrize("body", ["r7", "r6"])
def test_step_order_in_place(tune, small, body, upw, n):
    x, want = small
    for reverse in (False, True):
        d = to_dev(x[:n])
        tune.step_order(d, d, 1, reverse=reverse, nts=True, resident=0, upw=upw, plain_bytes=upw * 512, body=body)
        assert (to_host(d) == want[1][:n]).all(), reverse


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("upw", [4, 8])
@pytest.mark.parametrize("body", ["r7", "r6"])
def test_step_order_offset_views(tune, small, body, upw, n):
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
            tune.step_order(d, out, gens, reverse=reverse, nts=True, resident=0, upw=upw, plain_bytes=n * 512 // 2,
                            body=body)
            assert (to_host(out) == want[gens][:n]).all(), (gens, reverse)
    torch.cuda.synchronize()
    assert dst[0].item() == 0x5A5A5A5A and dst[-1].item() == 0x5A5A5A5A


def test_product_step_ping_pong(hip, big):
    """hip.step above kOrderMinUniverses: three launches ping-ponged between
    two batches (forward, reversed, forward; the plain tail live), each
    launch's output against the oracle"""
    a, b = to_dev(big[0]), torch.empty((BIG, 64), dtype=torch.int64, device="cuda")
    for g in (1, 2, 3):
        hip.step(a, out=b, generations=1)
        bad = np.nonzero((to_host(b) != big[g]).any(axis=1))[0]
        assert bad.size == 0, (g, bad[:8])
        a, b = b, a


def test_product_step_in_place(hip, big):
    d = to_dev(big[0])
    for g in (1, 2, 3):
        hip.step(d, out=d, generations=1)
        bad = np.nonzero((to_host(d) != big[g]).any(axis=1))[0]
        assert bad.size == 0, (g, bad[:8])
    d = to_dev(big[0])
    hip.step(d, out=d, generations=2)
    assert (to_host(d) == big[2]).all()


@pytest.mark.parametrize("n", [1, 7, 8, 9, 4099, BIG])
@pytest.mark.parametrize("gens", [1, 2])
def test_step_contains_final(hip, small, big, n, gens):
    """the fused 1-2 generation step with final states (k_step_contains<8>):
    first hits and final states against the oracle; then one more generation
    from the final states it left (above kOrderMinUniverses that launch takes
    the groups in reverse, the plain tail live)"""
    steps = big if n == BIG else [small[1][g][:n] for g in (0, 1, 2, 3)]
    # a target that stepped states hold: universe 0's own cells in a 3 x 3
    # window after one generation
    box = np.zeros(64, np.uint64)
    for c in (20, 21, 22):
        box[c] = np.uint64(0b111 << 30)
    w, u = steps[1][0] & box, box & ~steps[1][0]
    dw, du = to_dev(w[None]), to_dev(u[None])

    def first_hits(start, count):
        want = np.zeros(n, np.int64)
        for g in range(1, count + 1):
            hit = (((steps[start + g] ^ w) & (w | u)) == 0).all(axis=1)
            want[(want == 0) & hit] = g
        return want

    assert first_hits(0, gens)[0] == 1
    src = to_dev(steps[0])
    for start, count in ((0, gens), (gens, 1)):
        fin = torch.full((n, 64), -1, dtype=torch.int64, device="cuda")
        first, _ = hip.step_contains(src, dw, du, count, final=fin)
        assert (first.cpu().numpy() == first_hits(start, count)).all(), (start, count)
        bad = np.nonzero((to_host(fin) != steps[start + count]).any(axis=1))[0]
        assert bad.size == 0, (start, count, bad[:8])
        src = fin


@pytest.mark.parametrize("n", [1, 7, 8, 9, 4099])
@pytest.mark.parametrize("gens", [1, 2])
def test_step_contains_fast_form(tune, hip, small, n, gens):
    """the tuning build's k_step_contains with the same treatment (256 + 8:
    full groups unconditional, one group per wave; measured, not shipped)
    against the product's launch, with and without final states"""
    x = to_dev(small[0][:n])
    box = np.zeros(64, np.uint64)
    for c in (20, 21, 22):
        box[c] = np.uint64(0b111 << 30)
    s1 = small[1][1][0]
    dw, du = to_dev((s1 & box)[None]), to_dev((box & ~s1)[None])
    want_first, want_fin = hip.step_contains(x, dw, du, gens, final=torch.empty_like(x))
    assert (to_host(want_fin) == small[1][gens][:n]).all()
    fin = torch.full((n, 64), -1, dtype=torch.int64, device="cuda")
    assert torch.equal(tune.step_contains_nat(x, dw, du, gens, 256 + 8, 0, final=fin), want_first)
    assert torch.equal(fin, want_fin)
    assert torch.equal(tune.step_contains_nat(x, dw, du, gens, 256 + 8, 0), want_first)
