"""What the inline-assembly generators (gen_split_asm.py, gen_pair_asm.py,
gen_tile_asm.py) share.

Emitting: the truth tables, op(), the by-bank register Pool, bank_conflicts(),
the six-LUT tail (tail6) and AsmFn / render_fn, the one description of an
inline-asm function and its one rendering as C++.

Checking, on the CPU, before any of the text reaches a GPU:
  Machine         executes the emitted lines as they stand on 64 numpy lanes:
                  VGPRs, the named scalar operands (%[name]), SCC, numeric
                  local labels and Nf / Nb branches, a byte-addressed LDS.  It
                  raises on a mnemonic it does not know, on an LDS access out
                  of range or a read of bytes no lane has written, on an
                  instruction that touches a VGPR an unretired ds_read will
                  still write (LDS operations complete in issue order;
                  s_waitcnt lgkmcnt(N) retires all but the youngest N), and on
                  an LDS operation still outstanding when the text ends.
  check_operands  an AsmFn's constraint lists against its instructions.
"""
from __future__ import annotations

import bisect
import functools
import re
from dataclasses import dataclass

import numpy as np

# v_bitop3_b32 truth tables (bit 4 a + 2 b + c of the table = f(a, b, c))
XOR3, MAJ, NAE = 0x96, 0xE8, 0x7E
N1, N4, N6 = 0xE9, 0x52, 0xE0                    # the six-LUT tail (device.hpp life_tail6)
LE1, EVEN, T1, T2, T3 = 0x17, 0x69, 0x34, 0x58, 0x28     # rule 3's tail (device.hpp kLe1 .. kT3)

WAVE = 64
M32 = 0xFFFFFFFF


# ---- emitting ---------------------------------------------------------------

def op(dst, a, b, c, tt):
    return f"v_bitop3_b32 v{dst}, v{a}, v{b}, v{c} bitop3:0x{tt:02x}"


class Pool:
    """registers by VGPR bank (vN mod 4), handed out first in, first out"""

    def __init__(self, regs):
        self.free = {b: [r for r in regs if r % 4 == b] for b in range(4)}

    def get(self, bank):
        return self.free[bank % 4].pop(0)

    def put(self, r):
        self.free[r % 4].append(r)


def bank_conflicts(lines):
    """(VALU instructions, those with two sources in one bank)"""
    n, bad = 0, []
    for l in lines:
        if not l.startswith("v_"):
            continue
        n += 1
        srcs = {int(x) for x in re.findall(r"v(\d+)", l.split(",", 1)[1])}
        banks = [s % 4 for s in srcs]
        if len(banks) != len(set(banks)):
            bad.append(l)
    return n, bad


def tail6(j, r, h0, h1, rot, temps):
    """the six LUTs of row j: r[j] = next state from the h-layer h0 / h1 (the
    ring's rows -1 and len(r) in rot["h0u"], rot["h1u"], rot["h0d"],
    rot["h1d"]); temps(j) chooses the registers of g1 (also g4), g2, g3, g5.
    Returns (lines, those temps)."""
    a0 = rot["h0u"] if j == 0 else h0[j - 1]
    c0 = rot["h0d"] if j == len(r) - 1 else h0[j + 1]
    a1 = rot["h1u"] if j == 0 else h1[j - 1]
    c1 = rot["h1d"] if j == len(r) - 1 else h1[j + 1]
    g1, g2, g3, g5 = temps(j)
    return [op(g1, h1[j], a1, c1, N1),        # SB in {0,2,3}
            op(g2, c1, a1, c0, MAJ),
            op(g3, c0, a0, h0[j], NAE),       # SA in {1,2}
            op(g5, h0[j], c0, a0, XOR3),      # SA odd
            op(g1, g3, g2, g1, N4),           # g4 (in g1's register)
            op(r[j], g1, g5, r[j], N6)], (g1, g2, g3, g5)   # next = g4 & (g5 | a)


@dataclass
class AsmFn:
    """One inline-asm function.  outs / ins: rows (one source line each) of
    operands (constraint, C expression[, asm name]); a VGPR operand's
    constraint names its register, "+{v3}" or "{v46}"."""
    name: str
    sig: str          # the parameter list as it is laid out, "(...)"
    comment: str
    lines: list
    outs: list
    ins: list
    clobbers: list    # VGPR numbers
    decls: tuple = ()

    def vgprs(self, rows):
        return {int(x) for row in rows for o in row for x in re.findall(r"\{v(\d+)\}", o[0])}


def vreg(reg, expr, rw=""):
    return (f"{rw}{{v{reg}}}", expr)


def sreg(name, expr, constraint="+s"):
    return (constraint, expr, name)


def render_fn(f: AsmFn) -> str:
    def rows(rs):
        return ",\n        ".join(", ".join((f"[{o[2]}] " if len(o) > 2 else "") + f'"{o[0]}"({o[1]})' for o in r)
                                  for r in rs)
    return (f"\n{f.comment}\n__device__ __forceinline__ void {f.name}{f.sig} {{\n" +
            "".join(f"  {d}\n" for d in f.decls) + "  asm volatile(\n" +
            "".join(f'      "{l}\\n"\n' for l in f.lines) +
            f"      : {rows(f.outs)}\n      : {rows(f.ins)}\n      : " +
            ", ".join(f'"v{x}"' for x in f.clobbers) + ', "scc", "memory");\n}\n')


def loop_text(prologue, body):
    """nothing at 0 generations, else prologue, then body until %[g] (which
    body decrements) is 0, then the exchange drained"""
    return ["s_cmp_eq_u32 %[g], 0", "s_cbranch_scc1 2f"] + prologue + ["1:"] + body + \
        ["s_cmp_lg_u32 %[g], 0", "s_cbranch_scc1 1b", "s_waitcnt lgkmcnt(0)", "2:"]


# ---- reading the text back --------------------------------------------------

def _vregs(operand):
    m = re.fullmatch(r"v(\d+)|v\[(\d+):(\d+)\]", operand)
    if not m:
        return ()
    return (int(m[1]),) if m[1] else tuple(range(int(m[2]), int(m[3]) + 1))


@functools.lru_cache(maxsize=None)
def decode(line):
    """(mnemonic, operands, modifiers {name: value}, VGPRs read, VGPRs written)"""
    mn, _, rest = line.partition(" ")
    ops, mods = [], {}
    for piece in rest.split(","):
        words = piece.split()
        ops += words[:1]
        mods.update(w.split(":", 1) for w in words[1:])
    regs = [_vregs(o) for o in ops]
    if not mn.startswith(("v_", "ds_")) or mn in ("v_cmp_ne_u32_e64", "v_readlane_b32", "ds_write_b128"):
        dst = ()
    else:
        dst = regs[0]
    src = {x for r in (regs if not dst or mn == "v_or_b32_dpp" else regs[1:]) for x in r}   # DPP keeps masked lanes
    return mn, tuple(ops), mods, frozenset(src), frozenset(dst)


def check_operands(f: AsmFn):
    """the constraint lists against the text: every VGPR written is an output
    or a clobber, no clobber is an input or an output, every VGPR read before
    its first write (in text order) is an input or an output.  Returns the
    violations."""
    outs, ins, clob = f.vgprs(f.outs), f.vgprs(f.ins), set(f.clobbers)
    bad = [f"{f.name}: v{x} is a clobber and an operand" for x in sorted(clob & (ins | outs))]
    written = set()
    for l in f.lines:
        _, _, _, src, dst = decode(l)
        bad += [f"{f.name}: v{x} read before written, not an operand: {l}" for x in sorted(src - written - ins - outs)]
        bad += [f"{f.name}: v{x} written, neither output nor clobber: {l}" for x in sorted(dst - outs - clob)]
        written |= dst
    return bad


def lane_addresses(group=WAVE):
    """(self, prev, next): the LDS byte address of each lane's 16-B slot and of
    its neighbours' within groups of `group` lanes, wrapping, as the kernels
    pass a_self / a_prev / a_next (base 0)"""
    lane = np.arange(WAVE)
    g0 = lane & ~(group - 1)
    return lane * 16, (g0 | ((lane + group - 1) & (group - 1))) * 16, (g0 | ((lane + 1) & (group - 1))) * 16


def _bitop3(a, b, c, tt):
    out = np.zeros(WAVE, np.uint32)
    for k in range(8):
        if tt >> k & 1:
            out |= (a if k & 4 else ~a) & (b if k & 2 else ~b) & (c if k & 1 else ~c)
    return out


def _dpp(v, d, a, b, mods):
    """v_or_b32_dpp vd, va, vb: vd = dpp(va) | vb in the lanes that have a
    source and whose row is in row_mask"""
    rm = int(mods["row_mask"], 16)
    src, lane = np.zeros(WAVE, np.uint32), np.arange(WAVE)
    if "row_shr" in mods:
        n = int(mods["row_shr"])
        ok = lane % 16 >= n
        src[ok] = v[a][lane[ok] - n]
    else:
        n = int(mods["row_bcast"])
        ok = lane >= 16 if n == 15 else lane >= 32
        src[ok] = v[a][(lane[ok] // 16) * 16 - 1] if n == 15 else v[a][31]
    ok &= (rm >> (lane // 16)) & 1 == 1
    out = v[d].copy()
    out[ok] = src[ok] | v[b][ok]
    v[d] = out


# scalar ALU: (a, b, SCC in) -> (result, SCC out; None = unchanged)
_SALU = {
    "s_add_u32": lambda a, b, c: (a + b, a + b > M32),
    "s_addc_u32": lambda a, b, c: (a + b + c, a + b + c > M32),
    "s_sub_u32": lambda a, b, c: (a - b, b > a),
    "s_mul_i32": lambda a, b, c: (a * b, None),
    "s_and_b32": lambda a, b, c: (a & b, a & b != 0),
    "s_or_b32": lambda a, b, c: (a | b, a | b != 0),
    "s_andn2_b32": lambda a, b, c: (a & ~b, a & ~b & M32 != 0),
    "s_nor_b32": lambda a, b, c: (~(a | b), ~(a | b) & M32 != 0),
    "s_lshr_b32": lambda a, b, c: (a >> (b & 31), a >> (b & 31) != 0),
    "s_bfe_u32": lambda a, b, c: ((a >> (b & 31)) & ((1 << (b >> 16 & 0x7F)) - 1),) * 2,
}
_SCMP = {
    "s_cmp_eq_u32": lambda a, b: a == b,
    "s_cmp_lg_u32": lambda a, b: a != b,
    "s_cmp_eq_u64": lambda a, b: a == b,
    "s_bitcmp1_b32": lambda a, b: a >> (b & 31) & 1,
}
_NO_EFFECT = ("s_setprio", "s_nop")


class Machine:
    """One wave.  v: uint32 [n_vgpr, 64]; s: the scalar operands by name (a
    64-bit one, a lane mask, is one entry); lds: bytes."""

    def __init__(self, n_vgpr, lds_bytes, **sregs):
        self.v = np.zeros((n_vgpr, WAVE), np.uint32)
        self.s = dict(sregs)
        self.scc = 0
        self.lds = np.zeros(lds_bytes, np.uint8)
        self.lds_written = np.zeros(lds_bytes, bool)
        self.outstanding = []        # LDS operations in issue order: the VGPRs each will still write

    def sval(self, x):
        return self.s[x[2:-1]] if x.startswith("%[") else int(x, 0) & M32

    def src(self, x):
        return self.v[int(x[1:])] if x[0] == "v" else np.uint32(self.sval(x))

    def _lds_bytes(self, addr_reg, mods, line, reading):
        at = self.v[addr_reg].astype(np.int64) + int(mods.get("offset", 0))
        idx = at[:, None] + np.arange(16)
        if idx.min() < 0 or idx.max() >= len(self.lds):
            raise ValueError(f"LDS access out of range: {line}")
        if reading and not self.lds_written[idx].all():
            raise ValueError(f"LDS read of bytes no lane has written: {line}")
        return idx

    def run(self, lines, max_steps=10 ** 7):
        labels = {}
        for i, l in enumerate(lines):
            if re.fullmatch(r"\d+:", l):
                labels.setdefault(l[:-1], []).append(i)

        def target(t, pc):   # "3f": the next label 3 after pc; "3b": the last one before it
            at = labels.get(t[:-1], [])
            k = bisect.bisect(at, pc) - (t[-1] == "b")
            if not 0 <= k < len(at):
                raise ValueError(f"no label for {t}: {lines[pc]}")
            return at[k]

        v, pc = self.v, 0
        for _ in range(max_steps):
            if pc >= len(lines):
                break
            line = lines[pc]
            pc += 1
            mn, o, mods, rd, wr = decode(line)
            for pending in self.outstanding:
                if pending & (rd | wr):
                    raise ValueError(f"v{min(pending & (rd | wr))} is still to be written by an LDS read: {line}")
            if re.fullmatch(r"\d+:", line):
                pass
            elif mn == "v_bitop3_b32":
                v[int(o[0][1:])] = _bitop3(self.src(o[1]), self.src(o[2]), self.src(o[3]), int(mods["bitop3"], 16))
            elif mn == "v_alignbit_b32":
                x = (self.src(o[1]).astype(np.uint64) << np.uint64(32)) | self.src(o[2]).astype(np.uint64)
                v[int(o[0][1:])] = ((x >> np.uint64(self.sval(o[3]))) & np.uint64(M32)).astype(np.uint32)
            elif mn == "v_mov_b32":
                v[int(o[0][1:])] = self.src(o[1])
            elif mn == "v_and_b32":
                v[int(o[0][1:])] = self.src(o[1]) & self.src(o[2])
            elif mn == "v_lshl_or_b32":
                v[int(o[0][1:])] = (self.src(o[1]) << np.uint32(self.sval(o[2]))) | self.src(o[3])
            elif mn == "v_or_b32_dpp":
                _dpp(v, *(int(x[1:]) for x in o), mods)
            elif mn == "v_cmp_ne_u32_e64":
                ne = self.src(o[1]) != self.src(o[2])
                self.s[o[0][2:-1]] = sum(1 << i for i in np.flatnonzero(ne))
            elif mn == "v_readlane_b32":
                self.s[o[0][2:-1]] = int(v[int(o[1][1:]), int(o[2])])
            elif mn == "ds_write_b128":
                base = _vregs(o[1])[0]
                idx = self._lds_bytes(int(o[0][1:]), mods, line, False)
                self.lds[idx] = np.ascontiguousarray(v[base:base + 4].T).view(np.uint8)
                self.lds_written[idx] = True
                self.outstanding.append(frozenset())
            elif mn == "ds_read_b128":
                base = _vregs(o[0])[0]
                idx = self._lds_bytes(int(o[1][1:]), mods, line, True)
                v[base:base + 4] = np.ascontiguousarray(self.lds[idx]).view(np.uint32).T
                self.outstanding.append(wr)
            elif mn == "s_waitcnt" and re.fullmatch(r"lgkmcnt\(\d+\)", o[0]):
                del self.outstanding[:max(0, len(self.outstanding) - int(o[0][8:-1]))]
            elif mn in _NO_EFFECT:
                pass
            elif mn in _SALU:
                y, scc = _SALU[mn](self.sval(o[1]), self.sval(o[2]), self.scc)
                self.s[o[0][2:-1]] = y & M32
                self.scc = self.scc if scc is None else int(bool(scc))
            elif mn in _SCMP:
                self.scc = int(bool(_SCMP[mn](self.sval(o[0]), self.sval(o[1]))))
            elif mn == "s_mov_b32":
                self.s[o[0][2:-1]] = self.sval(o[1])
            elif mn == "s_brev_b32":
                self.s[o[0][2:-1]] = int(f"{self.sval(o[1]):032b}"[::-1], 2)
            elif mn == "s_cselect_b32":
                self.s[o[0][2:-1]] = self.sval(o[1]) if self.scc else self.sval(o[2])
            elif mn == "s_branch":
                pc = target(o[0], pc - 1)
            elif mn in ("s_cbranch_scc0", "s_cbranch_scc1"):
                if self.scc == (mn == "s_cbranch_scc1"):
                    pc = target(o[0], pc - 1)
            else:
                raise ValueError(f"unknown instruction: {line}")
        else:
            raise RuntimeError(f"no end after {max_steps} instructions")
        if self.outstanding:
            raise ValueError(f"{len(self.outstanding)} LDS operations outstanding at the end of the text")
        return self
