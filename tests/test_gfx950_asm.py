"""CPU: what tools/gfx950_asm.py's machine refuses (an instruction it does not
know, an LDS read of unwritten bytes, a VGPR touched while a ds_read that
will write it is outstanding, LDS operations left at the end), and the
constraint lists of every generated inline-asm function against its
instructions."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_pair_asm  # noqa: E402
import gen_split_asm  # noqa: E402
import gen_tile_asm  # noqa: E402
from gfx950_asm import AsmFn, Machine, check_operands, lane_addresses, vreg  # noqa: E402


def _machine():
    m = Machine(12, 1024)
    m.v[0], m.v[1], _ = lane_addresses()      # v0: this lane's slot, v1: lane i-1's
    m.v[2:6] = np.arange(4 * 64, dtype=np.uint32).reshape(4, 64)
    return m


def test_unknown_instruction_raises():
    _machine().run(["v_mov_b32 v6, v2"])
    with pytest.raises(ValueError, match="unknown instruction"):
        _machine().run(["v_frobnicate_b32 v6, v2, v3"])


EXCHANGE = ["ds_write_b128 v0, v[2:5]", "ds_read_b128 v[6:9], v1"]


def test_missed_wait_raises():
    """v7 belongs to a ds_read_b128 that nothing has retired, or that
    lgkmcnt(1) does not retire (only the write before it); lgkmcnt(0) does"""
    m = _machine().run(EXCHANGE + ["s_waitcnt lgkmcnt(0)", "v_mov_b32 v10, v7"])
    assert (m.v[10] == np.roll(m.v[3], 1)).all()             # lane i-1's second word
    for touch in ("v_mov_b32 v10, v7", "v_mov_b32 v7, v2"):  # reading it, overwriting it
        for wait in ([], ["s_waitcnt lgkmcnt(1)"]):
            with pytest.raises(ValueError, match="v7 is still to be written"):
                _machine().run(EXCHANGE + wait + [touch])


def test_lds_reads_and_leftovers_raise():
    with pytest.raises(ValueError, match="no lane has written"):
        _machine().run(["ds_read_b128 v[6:9], v1", "s_waitcnt lgkmcnt(0)"])
    with pytest.raises(ValueError, match="out of range"):
        _machine().run(["ds_write_b128 v0, v[2:5] offset:16"])
    with pytest.raises(ValueError, match="outstanding at the end"):
        _machine().run(EXCHANGE + ["s_waitcnt lgkmcnt(1)"])


def test_operand_rules_see_each_mistake():
    ok = dict(name="f", sig="()", comment="", lines=EXCHANGE + ["s_waitcnt lgkmcnt(0)", "v_mov_b32 v2, v6"],
              outs=[[vreg(2, "r", "+")]], ins=[[vreg(0, "a"), vreg(1, "b"), vreg(3, "c"), vreg(4, "d"), vreg(5, "e")]],
              clobbers=[6, 7, 8, 9])
    assert check_operands(AsmFn(**ok)) == []
    assert len(check_operands(AsmFn(**{**ok, "clobbers": [6, 7, 8]}))) == 1          # v9 written, undeclared
    assert len(check_operands(AsmFn(**{**ok, "clobbers": [5, 6, 7, 8, 9]}))) == 1    # v5 clobber and input
    assert len(check_operands(AsmFn(**{**ok, "ins": [ok["ins"][0][:-1]]}))) == 1     # v5 read, undeclared


def test_operand_rules_hold_for_every_generated_function():
    fns = {"split_asm.inc": gen_split_asm.product_fns(), "split_asm_tune.inc": gen_split_asm.tune_fns(),
           "pair_asm.inc": gen_pair_asm.functions(), "tile_asm.inc": [gen_tile_asm.function()]}
    assert {k: len(v) for k, v in fns.items()} == \
        {"split_asm.inc": 6, "split_asm_tune.inc": 26, "pair_asm.inc": 6, "tile_asm.inc": 1}
    names = [f.name for v in fns.values() for f in v]
    assert len(set(names)) == 39
    assert [bad for v in fns.values() for f in v for bad in check_operands(f)] == []
