#!/usr/bin/env python3
"""Generate the hand-allocated generation loop of rule 11 (8-way row split, 4
universes per wave interleaved bit by bit, LDS exchange, the 6-LUT tail of
device.hpp's life_tail6) as inline gfx950 assembly:
lifeapi_amd/csrc/split_asm.inc, used by k_step_split with LIFEAPI_XCHG_ASM.

Why: the compiler's allocation of the rule-11 loop puts 30 of its 68 VALU on
two sources in one VGPR bank (bank = vN mod 4, tools/vbank.py), and such a
v_bitop3 issues at about half rate (tools/ab/bank_probe.hip).  16 of them are the
h-layer xor3 / maj(L, r, R), which cannot avoid it: r, L and R all live in
even-aligned b128 tuples (ds_write_b128 / ds_read_b128), so word j sits at the
same position parity in each and only two banks are left for three operands.
The other 52 (the tails and the ring rotates) are conflict-free here:

  r[j]  bank j        (v0..v7, the ds_write_b128 tuples)
  L[j]  bank j + 2    (ds_read_b128 at v[10:13], v[14:17])
  R[j]  bank j        (ds_read_b128 at v[20:23], v[24:27]); h1[j] overwrites R[j]
                      (h1[3] in v51: see H1)
  h0[j] bank j + 1,  h1[j] bank j  (vertical triples j-1, j, j+1 span 3 banks;
        maj(h1[j+1], h1[j-1], h0[j+1]) needs h0's offset odd against h1's)
  tail temps by bank: g1/g4 j+1, g2 j+2, g3 j+3, g5 j+2 (g4, g5 and r[j]
        distinct for the last LUT)

The emitting helpers, the description of an inline-asm function and the
interpreter of the emitted text are tools/gfx950_asm.py's.  simulate*() here
only fill its machine's registers (the LDS addresses as k_step_split passes
them) and run asm_text / asm_text2 / contains_text / batch_text as emitted:
labels, branches, waits and byte-addressed LDS included.
tests/test_split_asm.py checks that against gen_split's network on random
states, the bank rules, and every function's constraint lists against its
instructions.

Usage: python tools/gen_split_asm.py [--check]
"""
from __future__ import annotations

import os
import sys

from gfx950_asm import (MAJ, XOR3, AsmFn, Machine, Pool, lane_addresses, loop_text, op, render_fn, sreg, tail6,
                        vreg)
from gfx950_asm import bank_conflicts as check_banks   # the name the tests call it by

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "lifeapi_amd", "csrc", "split_asm.inc")

S, P = 8, 4

R = [j for j in range(8)]                       # r[j]: v0..v7
L = [10 + j for j in range(4)] + [14 + j - 4 for j in range(4, 8)]
RR = [20 + j for j in range(4)] + [24 + j - 4 for j in range(4, 8)]
# h1[j] overwrites R[j], except h1[3]: rows 4..7's tails still read it after
# the next generation's plane-0 reads have refilled v[20:23] (PIPE)
H1 = RR[:3] + [51] + RR[4:]
H0 = [29 + j for j in range(8)]                 # bank j + 1
H0U, H0D, H1U, H1D = 40, 41, 39, 44              # banks 0, 1, 3, 0 (as h0[-1], h0[8], h1[-1], h1[8])
ROT = {"h0u": H0U, "h0d": H0D, "h1u": H1U, "h1d": H1D}
# three per bank: a pair of interleaved tails needs at most three of one bank
TEMPS = [8, 9, 18, 19, 28, 37, 38, 42, 43, 45, 47, 48]
A_SELF, A_PREV, A_NEXT = 46, 49, 50
N_VGPR = 52
PLANE = 1024                                     # bytes of one 16-B-per-lane LDS plane

# ---- two groups per wave (G = 2): each group's exchange hides behind the
# other group's h-layer and tails; 8 more universes per wave in flight.
RB_REGS = list(range(56, 64))                    # group B's r[j]: bank j
LB2 = [66 + j for j in range(4)] + [70 + j - 4 for j in range(4, 8)]    # bank j + 2
RRB2 = [76 + j for j in range(4)] + [80 + j - 4 for j in range(4, 8)]   # bank j
N_VGPR2 = 84


def tail_pair(j, k, al, r=R, h1=H1):
    """rows j and k's tails interleaved; their temps are free again only
    after both are emitted"""
    def temps(i):
        return al.get(i + 1), al.get(i + 2), al.get(i + 3), al.get(i + 2)
    (a, ra), (b, rb) = tail6(j, r, H0, h1, ROT, temps), tail6(k, r, H0, h1, ROT, temps)
    for t in ra + rb:
        al.put(t)
    return [x for xy in zip(a, b) for x in xy]


def hlayer(js, r=R, l=L, rr=RR, h1=H1):
    out = []
    for j in js:
        out.append(op(H0[j], l[j], r[j], rr[j], XOR3))
        out.append(op(h1[j], l[j], r[j], rr[j], MAJ))
    return out


def rotates(h1=H1):
    """rows -1 (rotl P of row 7's h) and 8 (rotr P of row 0's)"""
    return [f"v_alignbit_b32 v{H0U}, v{H0[S - 1]}, v{H0[S - 1]}, {32 - P}",
            f"v_alignbit_b32 v{H1U}, v{h1[S - 1]}, v{h1[S - 1]}, {32 - P}",
            f"v_alignbit_b32 v{H0D}, v{H0[0]}, v{H0[0]}, {P}",
            f"v_alignbit_b32 v{H1D}, v{h1[0]}, v{h1[0]}, {P}"]


# Variants of the loop's schedule (same instructions, different order).  All
# issue the NEXT generation's exchange inside this one, plane 0 right after
# rows 0..3's tails and plane 1 at the end ("pipe"), and raise the wave's
# priority from the arrival of its exchange until it has published the next
# generation's plane 0, so that a wave with data in hand keeps the LDS pipe
# fed before the others' tails:
#   "pipe_prio"    s_setprio 2
#   "pipe_prio_e"  "pipe_prio", and raised again for rows 6..7 and the
#                  plane-1 exchange (low only during rows 4..5)
#   "pipe_prio_m"  priority dropped after rows 0..1's tails
#   "pipe_prio1"   "pipe_prio" with s_setprio 1
# v0 (LIFEAPI_XCHG_ASM) is VARIANTS[0]; the others are LIFEAPI_XCHG_ASM_V(k).
# Measured on config 3 (profiles/r01/tune_c3asm_*.jsonl), schedules no longer
# generated included: "plain" (plane by plane, write then its two reads, at
# the top of each generation; lgkmcnt(3) before plane 0's h-layer, as the
# compiler orders the compiled loop) 1.349 ms, "early" ("plain" with rows 1
# and 2, which read only plane-0 h values, before the wait for plane 1) 1.363,
# "pipe" without the priority 1.330-1.373, the compiled loop 1.370-1.392;
# "pipe_prio" 1.287-1.307, dropping the priority right after the h-layer
# 1.361, s_setprio 3 instead of 2 1.320.
VARIANTS = ("pipe_prio", "pipe_prio_e", "pipe_prio_m", "pipe_prio1")
DEFAULT = VARIANTS[0]


def exchange(plane, grp=0):
    """publish four of group grp's rows and read both neighbours' (group b's
    planes sit 2 KiB after group a's)"""
    off = 2 * PLANE * grp + PLANE * plane
    o = f" offset:{off}" if off else ""
    r, l, rr = (R, L, RR) if grp == 0 else (RB_REGS, LB2, RRB2)
    lo = 4 * plane
    return [f"ds_write_b128 v{A_SELF}, v[{r[lo]}:{r[lo] + 3}]{o}",
            f"ds_read_b128 v[{l[lo]}:{l[lo] + 3}], v{A_PREV}{o}",
            f"ds_read_b128 v[{rr[lo]}:{rr[lo] + 3}], v{A_NEXT}{o}"]


def prologue():
    return exchange(0) + exchange(1)


def body(variant=DEFAULT):
    prio = 1 if variant.endswith("prio1") else 2
    again, mid = variant.endswith("prio_e"), variant.endswith("prio_m")
    al = Pool(TEMPS)
    lines = ["s_sub_u32 %[g], %[g], 1", "s_waitcnt lgkmcnt(3)", f"s_setprio {prio}"]
    lines += hlayer(range(4)) + ["s_waitcnt lgkmcnt(0)"] + hlayer(range(4, 8)) + rotates()
    lines += tail_pair(0, 1, al)
    if mid:
        lines.append("s_setprio 0")
    lines += tail_pair(2, 3, al)
    lines += exchange(0)   # rows 0..3 are final: publish plane 0
    if not mid:
        lines.append("s_setprio 0")
    lines += tail_pair(4, 5, al)
    if again:
        lines.append(f"s_setprio {prio}")
    lines += tail_pair(6, 7, al)
    return lines + exchange(1)


def asm_text(variant=DEFAULT):
    return loop_text(prologue(), body(variant))


def group_gen(grp):
    """one generation of group grp (its exchange already landed)"""
    r, l, rr = (R, L, RR) if grp == 0 else (RB_REGS, LB2, RRB2)
    al = Pool(TEMPS)                              # h1[j] overwrites R[j]
    return hlayer(range(S), r, l, rr, rr) + rotates(rr) + \
        [x for j in range(0, S, 2) for x in tail_pair(j, j + 1, al, r, rr)]


def asm_text2():
    # in order: A's 6 LDS ops, then B's 6 are outstanding at the top
    body2 = ["s_sub_u32 %[g], %[g], 1", "s_waitcnt lgkmcnt(6)"] + group_gen(0) + \
        exchange(0, 0) + exchange(1, 0) + ["s_waitcnt lgkmcnt(6)"] + group_gen(1) + \
        exchange(0, 1) + exchange(1, 1)
    return loop_text(exchange(0, 0) + exchange(1, 0) + exchange(0, 1) + exchange(1, 1), body2)


ADDR_INS = [vreg(A_SELF, "a_self"), vreg(A_PREV, "a_prev"), vreg(A_NEXT, "a_next")]
PINNED = sorted(set(L + RR + H1 + H0 + [H0U, H0D, H1U, H1D] + TEMPS))


def r_outs(regs, name):
    return [[vreg(regs[j], f"{name}[{j}]", "+")] for j in range(S)]


def fn2():
    return AsmFn(
        name="split_gens_asm2",
        sig="(uint32_t (&a)[8], uint32_t (&b)[8], uint32_t gens,\n" + " " * 48 +
            "uint32_t a_self, uint32_t a_prev, uint32_t a_next)",
        comment="// Two groups per wave (G = 2): a / b are the groups' r[j]; group b's planes\n"
                "// sit 2 KiB after group a's.  Each group's exchange is in flight while the\n"
                f"// other group's generation runs.  {N_VGPR2} VGPRs pinned.",
        lines=asm_text2(), outs=r_outs(R, "a") + r_outs(RB_REGS, "b") + [[sreg("g", "gens")]], ins=[ADDR_INS],
        clobbers=sorted(set(L + RR + LB2 + RRB2 + H0 + [H0U, H0D, H1U, H1D] + TEMPS)))


# ---- fused Step + Contains(LifeTarget) on the same loop (k_step_contains_split):
# after each generation, d = OR_j (r_j ^ w_j) & m_j (m = wanted | unwanted,
# LifeTarget.hpp:44-51), one ballot per universe (its bits are every 4th),
# and the first generation with an empty ballot is kept per universe in SGPRs.
W_REGS = [53, 54, 55, 56, 57, 58, 59, 60]        # w_j: bank j + 1
M_REGS = [62, 63, 52, 61, 66, 67, 64, 65]        # m_j: bank j + 2
N_VGPR_C = 68
# the "low" layout for targets of at most 4 rows: w_0..3 / m_0..3 in v52..v59
# (same banks) and the batched test's block word in v60, so that the
# kernel's VGPR count, and with it the waves per SIMD, stays at the plain
# step's 8 (at most 64 VGPRs) instead of 5 (87 VGPRs with all eight rows)
W_LO = [53, 54, 55, 56]
M_LO = [58, 59, 52, 57]
LOW_H = 4
WM = {"low": (W_LO, M_LO), "high": (W_REGS, M_REGS)}    # by register layout
DIFF = 0x28        # (r ^ w) & m
OR3 = 0xFE         # a | b | c
ORAND = 0xA8       # (a | b) & c


def _or_to_two(d, al):
    """OR-reduce the difference registers d to two values (y, z) with
    y | z = OR(d), in as few OR3 as possible; (lines, y, z)"""
    h = len(d)
    if h == 1:
        return [], d[0], d[0]
    if h == 2:
        return [], d[0], d[1]
    x = al.get(1)
    lines = [op(x, d[0], d[1], d[2], OR3)]
    if h == 3:
        return lines, x, x
    if h == 4:
        return lines, x, d[3]
    y = al.get(2)
    if h == 5:
        return lines + [op(y, d[3], d[4], d[4], OR3)], x, y
    lines.append(op(y, d[3], d[4], d[5], OR3))
    if h == 6:
        return lines, x, y
    z = al.get(3)
    if h == 7:
        return lines + [op(z, d[6], x, x, OR3)], y, z
    return lines + [op(z, d[6], d[7], x, OR3)], y, z


def contains_check(lean=False, h=S, layout="high"):
    """lean: the per-universe bookkeeping on the fast path is 2 SALU per
    universe (s_cmp_eq_u64 + s_addc_u32 building the clean mask, universe 0
    in bit 3) and one s_andn2 + branch; a hit (rare) branches to a slow path
    that records it.  Otherwise 8 SALU per universe per generation.
    h < 8 (lean only): the target's care rows all lie in residues 0..h-1 of
    the 8-way split (the kernel rotates universes and target so), so only
    registers 0..h-1 are differenced."""
    al = Pool(TEMPS)
    d = []
    for j in range(h):
        t = al.get(j)
        d.append(t)
    wr, mr = WM[layout]
    lines = [op(d[j], R[j], wr[j], mr[j], DIFF) for j in range(h)]
    if lean:
        red, y, z = _or_to_two(d, al)
        lines += red
        for t in set(d) - {y, z}:  # consumed: the masked ORs may reuse them
            al.put(t)
        lines.append("s_add_u32 %[gc], %[gc], 1")
        ts = [al.get(b) for b in range(P)]
        for u in range(P):
            lines += [f"v_bitop3_b32 v{ts[u]}, v{y}, v{z}, %[m{u}] bitop3:0x{ORAND:02x}",
                      f"v_cmp_ne_u32_e64 %[cmp{u}], 0, v{ts[u]}"]
        return lines + contains_salu()
    assert h == S
    x, y = al.get(1), al.get(2)
    z = al.get(3)
    lines += [op(x, d[0], d[1], d[2], OR3), op(y, d[3], d[4], d[5], OR3), op(z, d[6], d[7], x, OR3)]
    t = al.get(0)
    lines.append("s_add_u32 %[gc], %[gc], 1")
    for u in range(P):
        lines += [f"v_bitop3_b32 v{t}, v{y}, v{z}, %[m{u}] bitop3:0x{ORAND:02x}",
                  f"v_cmp_ne_u32_e64 %[cmp], 0, v{t}",
                  "s_cmp_eq_u64 %[cmp], 0",                 # SCC = universe u clean
                  f"s_cselect_b32 %[c], {1 << u}, 0",
                  "s_andn2_b32 %[c], %[c], %[found]",      # fresh hit
                  "s_cmp_lg_u32 %[c], 0",
                  f"s_cselect_b32 %[h{u}], %[gc], %[h{u}]",
                  "s_or_b32 %[found], %[found], %[c]"]
    return lines


def contains_salu():
    """the lean check's scalar part: the clean mask from the four compares
    (universe 0 in bit 3), fresh hits, and the branch to the slow path"""
    lines = ["s_mov_b32 %[c], 0"]
    for u in range(P):
        lines += [f"s_cmp_eq_u64 %[cmp{u}], 0",       # SCC = universe u clean
                  "s_addc_u32 %[c], %[c], %[c]"]      # c = 2c + SCC
    return lines + ["s_andn2_b32 %[c], %[c], %[found]",     # fresh hits; SCC = any
                    "s_cbranch_scc1 3f",
                    "4:"]


def contains_slowpath():
    """the lean check's hit handler, placed after the loop: record gc for
    every fresh universe (bit 3 - u of c) and jump back"""
    lines = ["3:", "s_or_b32 %[found], %[found], %[c]"]
    for u in range(P):
        lines += [f"s_bitcmp1_b32 %[c], {P - 1 - u}",
                  f"s_cselect_b32 %[h{u}], %[gc], %[h{u}]"]
    return lines + ["s_branch 4b"]


def contains_body(lean=False, h=S, late=False, layout="high"):
    """the default schedule's body with the check after rows 6..7 (all eight
    rows final), before the plane-1 exchange; late (lean only): the check's
    scalar part after that exchange, so the compares' results have landed
    in their SGPRs when the SALU reads them"""
    b = body(DEFAULT)
    k = b.index(exchange(1)[0])
    chk = contains_check(lean, h, layout)
    if not late:
        return b[:k] + chk + b[k:]
    sal = contains_salu()
    assert chk[-len(sal):] == sal
    return b[:k] + chk[:-len(sal)] + b[k:] + sal


def contains_text(lean=False, h=S, late=False, layout="high"):
    lines = loop_text(prologue(), contains_body(lean, h, late, layout))[:-1]
    if lean:
        lines += ["s_branch 2f"] + contains_slowpath()
    return lines + ["2:"]


_SIG_CONT_LAID_OUT = ("(uint32_t (&r)[8], const uint32_t (&w)[8],\n" + " " * 35 +
                      "const uint32_t (&m)[8], uint32_t gens, uint32_t a_self,\n" + " " * 35 +
                      "uint32_t a_prev, uint32_t a_next, uint32_t (&hit)[4])")
_CMP4 = [sreg(f"cmp{u}", f"cmp{u}", "=&s") for u in range(P)]


def _contains_fn(name, comment, lines, scalars, decls, layout, nt, clobbers):
    """what the fused loops share: r and the hits out, the addresses, the
    target's first nt rows and the universes' bit masks in"""
    wr, mr = WM[layout]
    return AsmFn(
        name=name, sig=_SIG_CONT_LAID_OUT, comment=comment, lines=lines, decls=decls, clobbers=clobbers,
        outs=r_outs(R, "r") + [[sreg(f"h{u}", f"hit[{u}]")] for u in range(P)] + scalars,
        ins=[ADDR_INS, [vreg(wr[j], f"w[{j}]") for j in range(nt)] + [vreg(mr[j], f"m[{j}]") for j in range(nt)] +
             [sreg(f"m{u}", f"0x11111111u << {u}", "s") for u in range(P)]])


def fn_contains(lean=False, h=S, late=False, layout="high"):
    low = layout == "low"
    scalars = [sreg("g", "gens"), sreg("gc", "gc"), sreg("found", "found"), sreg("c", "c", "=&s")]
    if lean:
        name = "split_contains_asm_lean" + ("_late" if late else "") + ("_lo" if low else "" if h == S else f"_h{h}")
        cmps, cmp_outs = "uint64_t cmp0, cmp1, cmp2, cmp3;", _CMP4
        doc = ("// The same with the per-universe bookkeeping cut to two SALU per universe on\n"
               "// the fast path (the clean mask built by s_cmp + s_addc; hits branch to a\n"
               "// slow path after the loop)" +
               ("." if h == S else f", differencing only registers 0..{h - 1} (a target whose\n"
                f"// care rows the kernel has rotated into residues 0..{h - 1})."))
    else:
        name, cmps, cmp_outs = "split_contains_asm", "uint64_t cmp;", [sreg("cmp", "cmp", "=&s")]
        doc = ("// Fused Step + Contains on the default schedule: after every generation the\n"
               "// containment test of all four universes (hit[u] = first generation whose\n"
               "// state contains the target, 0 = none yet).  w / m: the target's wanted and\n"
               f"// wanted | unwanted planes in the same register layout.  {N_VGPR_C} VGPRs pinned.")
    return _contains_fn(name, doc, contains_text(lean, h, late, layout), [scalars + cmp_outs],
                        ("uint32_t gc = 0, found = 0, c;", cmps), layout, h if low else S, PINNED)


# ---- the batched test (split_contains_asm_batch_h<h>, h <= 7): the same
# differences, but the cross-lane part runs once per EIGHT generations.  With
# the target's care rows rotated into rows 0..h-1, every difference register
# is zero outside its bits 0..3 (row j of the four universes), and so is
# their OR x_k; generation k of a block therefore packs into bits 4k..4k+3 of
# one word with a single v_lshl_or_b32 (x_0 is written as is).  The OR of that
# word over the 64 lanes is a DPP chain (row_shr 1/2/4/8, row_bcast 15/31)
# issued inside the next block's first h-layer, so that its two-wait-state
# hazards are filled by independent work, then one v_readlane and one s_nor:
# universe u is clean at generation k iff bit 4k + u is clear in every lane.
# Per wave-generation (h = 4): 4 differences, 2 ORs, 1 shift-OR and 7 / 8
# for the chain = 7.9 VALU against 13, and 3 SALU per block instead of 12 per
# generation.  gens % 8 leading generations run the lean per-generation loop.
# The block word needs one register, free in both layouts: w[7] (h <= 7) or
# v60 (low).
ACC_HI, ACC_LO = 60, 60
# h = 8 (any target: every register differenced, w[7] in v60 taken): the
# block word in v68, one VGPR past the lean loop's 68; each generation's OR
# of differences is folded onto its low nibble first (rotates by 16, 8, 4:
# the universe index, bit & 3, is kept), 6 VALU, then packed as above
ACC_H8 = 68
KB = 8             # generations per block
BATCH_MAX_H = 7


def _acc(layout, h=None):
    if layout == "high" and h == S:
        return ACC_H8
    return {"low": ACC_LO, "high": ACC_HI}[layout]


def _or_into(d, dst, al):
    """dst = OR of registers d (OR3 tree, the last OR writing dst)"""
    lines, d = [], list(d)
    while len(d) > 3:
        t = al.get(len(lines) + 1)
        lines.append(op(t, d[0], d[1], d[2], OR3))
        d = d[3:] + [t]
    a, b, c = (d + d[-1:] * 2)[:3]
    return lines + [op(dst, a, b, c, OR3)]


def batch_x_full(k, al, layout):
    """batch_x for h = 8: the eight differences OR-ed in place (their
    temps reused), folded onto the low nibble, then packed"""
    acc = _acc(layout, S)
    wr, mr = WM[layout]
    d = [al.get(j) for j in range(S)]
    lines = [op(d[j], R[j], wr[j], mr[j], DIFF) for j in range(S)]
    x, t = d[6], d[7]
    lines += [op(d[0], d[0], d[1], d[2], OR3), op(d[3], d[3], d[4], d[5], OR3), op(x, d[6], t, d[0], OR3),
              op(x, x, d[3], d[3], OR3)]
    for sh in (16, 8, 4):
        lines += [f"v_alignbit_b32 v{t}, v{x}, v{x}, {sh}", op(x, x, t, t, OR3)]
    if k == 0:
        return lines + [f"v_and_b32 v{acc}, 15, v{x}"]
    return lines + [f"v_and_b32 v{t}, 15, v{x}", f"v_lshl_or_b32 v{acc}, v{t}, {4 * k}, v{acc}"]


def batch_x(h, k, al, layout):
    """generation k of the block: ACC = x_k (k = 0) or ACC |= x_k << 4k,
    x_k = OR_j (r_j ^ w_j) & m_j over the h care registers"""
    if h == S:
        return batch_x_full(k, al, layout)
    acc = _acc(layout)
    wr, mr = WM[layout]
    if h == 1 and k == 0:
        return [op(acc, R[0], wr[0], mr[0], DIFF)]
    d = [al.get(j) for j in range(h)]
    lines = [op(d[j], R[j], wr[j], mr[j], DIFF) for j in range(h)]
    if k == 0:
        return lines + _or_into(d, acc, al)
    if h == 1:
        return lines + [f"v_lshl_or_b32 v{acc}, v{d[0]}, {4 * k}, v{acc}"]
    x = al.get(3)
    return lines + _or_into(d, x, al) + [f"v_lshl_or_b32 v{acc}, v{x}, {4 * k}, v{acc}"]


def batch_chain(h=None, layout="high"):
    """the lane OR of the block word into lane 63 (six in-place DPP ORs)"""
    a = _acc(layout, h)
    return [f"v_or_b32_dpp v{a}, v{a}, v{a} row_shr:{n} row_mask:0xf bank_mask:0xf" for n in (1, 2, 4, 8)] + \
           [f"v_or_b32_dpp v{a}, v{a}, v{a} row_bcast:15 row_mask:0xa bank_mask:0xf",
            f"v_or_b32_dpp v{a}, v{a}, v{a} row_bcast:31 row_mask:0xc bank_mask:0xf"]


def batch_check(slow, back):
    """the pending block's scalar test: c = generations x universes clean and
    not yet found (nibble k, bit u); any -> the slow path"""
    return ["s_nor_b32 %[c], %[rl], %[fm]",            # SCC = c != 0
            f"s_cbranch_scc1 {slow}f",
            f"{back}:"]


def batch_slowpath(lbl, back):
    """record the first clean generation of every fresh universe: nibble k of
    c is generation gc - 7 + k (gc already counts the pending block)"""
    lines = [f"{lbl}:", f"s_sub_u32 %[gk], %[gc], {KB - 1}"]
    for k in range(KB):
        lines += [f"s_bfe_u32 %[t], %[c], 0x{(4 << 16) | (4 * k):x}",
                  "s_andn2_b32 %[t], %[t], %[fu]",
                  "s_or_b32 %[fu], %[fu], %[t]"]
        for u in range(P):
            lines += [f"s_bitcmp1_b32 %[t], {u}",
                      f"s_cselect_b32 %[h{u}], %[gk], %[h{u}]"]
        lines.append("s_add_u32 %[gk], %[gk], 1")
    return lines + ["s_mul_i32 %[fm], %[fu], 0x11111111", f"s_branch {back}b"]


def batch_block(h, layout):
    """eight generations; the first carries the previous block's lane OR and
    scalar test between its h-layer's VALU"""
    acc = _acc(layout, h)
    out = []
    for k in range(KB):
        b = body(DEFAULT)
        if k:
            b.remove("s_sub_u32 %[g], %[g], 1")
        else:   # the pending chain, two VALU apart (DPP reads a fresh VGPR after 2 wait states)
            chain = batch_chain(h, layout) + [f"v_readlane_b32 %[rl], v{acc}, 63"]
            valu = [i for i, l in enumerate(b) if l.startswith("v_")]
            pos = {valu[2 * i]: c for i, c in enumerate(chain[:6])}
            pos[valu[13]] = chain[6]
            nb = []
            for i, l in enumerate(b):
                if i in pos:
                    nb.append(pos[i])
                nb.append(l)
                if i == valu[15]:
                    nb += batch_check(8, 9)
            b = nb
        ex = b.index(exchange(1)[0])
        chk = batch_x(h, k, Pool(TEMPS), layout)
        if k == KB - 1:
            chk.append(f"s_add_u32 %[gc], %[gc], {KB}")
        out += b[:ex] + chk + b[ex:]
    return out


def batch_text(h, layout="high"):
    acc = _acc(layout, h)
    assert 1 <= h <= {"low": LOW_H, "high": S}[layout]
    lean = [l.replace("%[g]", "%[rem]") for l in contains_body(True, h, layout=layout)]
    flush = []
    for c in batch_chain(h, layout):
        flush += [c, "s_nop 1"]
    flush += [f"v_readlane_b32 %[rl], v{acc}, 63"] + batch_check(10, 11)
    return (["s_cmp_eq_u32 %[g], 0", "s_cbranch_scc1 2f"] + prologue() +
            [f"s_and_b32 %[rem], %[g], {KB - 1}", "s_lshr_b32 %[g], %[g], 3",
             "s_cmp_eq_u32 %[rem], 0", "s_cbranch_scc1 5f", "1:"] + lean +
            ["s_cmp_lg_u32 %[rem], 0", "s_cbranch_scc1 1b",
             "5:", "s_cmp_eq_u32 %[g], 0", "s_cbranch_scc1 7f",
             f"v_mov_b32 v{acc}, -1",                   # no pending block
             "s_brev_b32 %[fu], %[found]", "s_lshr_b32 %[fu], %[fu], 28",  # bit 3 - u -> bit u
             "s_mul_i32 %[fm], %[fu], 0x11111111", "6:"] + batch_block(h, layout) +
            ["s_cmp_lg_u32 %[g], 0", "s_cbranch_scc1 6b"] + flush +
            ["7:", "s_waitcnt lgkmcnt(0)", "s_branch 2f"] + contains_slowpath() +
            batch_slowpath(8, 9) + batch_slowpath(10, 11) + ["2:"])


def fn_batch(h, layout="high"):
    wr, mr = WM[layout]
    extra = {"low": [ACC_LO], "high": W_REGS + M_REGS + ([ACC_H8] if h == S else [])}[layout]
    name = {"low": "split_contains_asm_batch_lo", "high": f"split_contains_asm_batch_h{h}"}[layout]
    note = {"low": ";\n// the low register layout (any target of at most 4 rows)", "high": ""}[layout]
    return _contains_fn(
        name,
        f"// The lean test batched over eight generations ({'any target' if h == S else f'rows 0..{h - 1}'}): "
        "per block one\n"
        f"// lane OR (DPP) and one scalar test of a word holding a nibble per generation{note}.",
        batch_text(h, layout),
        [[sreg("g", "gens"), sreg("gc", "gc"), sreg("found", "found"), sreg("c", "c", "=&s"),
          sreg("rem", "rem", "=&s")],
         [sreg(x, x, "=&s") for x in ("fu", "fm", "rl", "t", "gk")], _CMP4],
        ("uint32_t gc = 0, found = 0, c, rem, fu, fm, rl, t, gk;", "uint64_t cmp0, cmp1, cmp2, cmp3;"),
        layout, h, sorted(set(PINNED + extra) - set(wr[:h] + mr[:h])))


def fn_loop(name, variant):
    return AsmFn(name=name, comment=f'// schedule "{variant}" (see tools/gen_split_asm.py)',
                 sig="(uint32_t (&r)[8], uint32_t gens, uint32_t a_self, uint32_t a_prev,\n" +
                     " " * (len(name) + 32) + "uint32_t a_next)",
                 lines=asm_text(variant), outs=r_outs(R, "r") + [[sreg("g", "gens")]], ins=[ADDR_INS],
                 clobbers=PINNED)


# ---- the generated text on tools/gfx950_asm.py's machine -------------------

def _machine(lines, n_vgpr, planes, regs, **scalars):
    """run lines on a wave with the LDS addresses k_step_split passes
    (step_kernels.hpp: self = lane * 16, prev / next = the lanes beside it,
    wrapping over the wave) and the given (registers, values)"""
    m = Machine(n_vgpr, planes * PLANE, **scalars)
    m.v[[A_SELF, A_PREV, A_NEXT]] = lane_addresses()
    for at, val in regs:
        m.v[at] = val
    return m.run(lines)


def simulate(r, gens, two=None, variant=DEFAULT):
    """split_gens_asm_v<k> on r = uint32 [8, 64] (register j, lane); with
    `two` (a second group), split_gens_asm2; returns r (and two)."""
    if two is None:
        return _machine(asm_text(variant), N_VGPR, 2, [(R, r)], g=gens).v[R].copy()
    m = _machine(asm_text2(), N_VGPR2, 4, [(R, r), (RB_REGS, two)], g=gens)
    return m.v[R].copy(), m.v[RB_REGS].copy()


def _simulate_hits(lines, n_vgpr, r, w, m, nt, gens, layout):
    wr, mr = WM[layout]
    mach = _machine(lines, n_vgpr, 2, [(R, r), (wr[:nt], w[:nt]), (mr[:nt], m[:nt])], g=gens, gc=0, found=0,
                    **{f"h{u}": 0 for u in range(P)}, **{f"m{u}": 0x11111111 << u for u in range(P)})
    return mach.v[R].copy(), [mach.s[f"h{u}"] for u in range(P)]


def simulate_contains(r, w, m, gens, lean=False, h=S, late=False, layout="high"):
    """split_contains_asm[_lean[_late][_h<h> | _lo]]: returns (r, hits[4])"""
    return _simulate_hits(contains_text(lean, h, late, layout), N_VGPR_C, r, w, m, len(WM[layout][0]), gens, layout)


def simulate_batch(r, w, m, gens, h, layout="high"):
    """split_contains_asm_batch_h<h> / _batch_lo: returns (r, hits[4])"""
    return _simulate_hits(batch_text(h, layout), ACC_H8 + 1, r, w, m, h, gens, layout)


OUT_TUNE = os.path.join(ROOT, "tools", "tune", "split_asm_tune.inc")

_SIG_LOOP = "(uint32_t (&r)[8], uint32_t gens, uint32_t a_self, uint32_t a_prev, uint32_t a_next)"
_SIG_CONT = ("(uint32_t (&r)[8], const uint32_t (&w)[8], const uint32_t (&m)[8], uint32_t gens, "
             "uint32_t a_self, uint32_t a_prev, uint32_t a_next, uint32_t (&hit)[4])")
_SIG_TWO = "(uint32_t (&a)[8], uint32_t (&b)[8], uint32_t gens, uint32_t a_self, uint32_t a_prev, uint32_t a_next)"


# what the product include defines: the step loop, the full lean test (any
# target), the batched test for windows of 5..7 rows and, in the low layout,
# for windows of at most 4 rows; everything else is the tuning build's
PRODUCT_BATCH_H = range(LOW_H + 1, BATCH_MAX_H + 1)


def product_fns():
    return [fn_loop("split_gens_asm_v0", VARIANTS[0]), fn_contains(lean=True)] + \
        [fn_batch(h) for h in PRODUCT_BATCH_H] + [fn_batch(LOW_H, "low")]


def tune_fns():
    return [fn_loop(f"split_gens_asm_v{k}", v) for k, v in enumerate(VARIANTS) if k] + [fn2(), fn_contains()] + \
        [fn_contains(True, h) for h in range(1, S)] + [fn_contains(True, h, True) for h in range(1, S + 1)] + \
        [fn_batch(h) for h in list(range(1, LOW_H + 1)) + [S]] + [fn_contains(True, LOW_H, layout="low")]


def _ablation_decls():
    """forward declarations of the tuning build's loops: step_kernels.hpp
    (k_step_split) and contains_kernels.hpp (k_step_contains_split) name them
    in template branches the product never instantiates"""
    names = [(f"split_gens_asm_v{k}", _SIG_LOOP) for k in range(1, len(VARIANTS))]
    names += [("split_gens_asm2", _SIG_TWO), ("split_contains_asm", _SIG_CONT)]
    names += [(f"split_contains_asm_lean_h{h}", _SIG_CONT) for h in range(1, S)]
    names += [("split_contains_asm_lean_late" + ("" if h == S else f"_h{h}"), _SIG_CONT) for h in range(1, S + 1)]
    names += [(f"split_contains_asm_batch_h{h}", _SIG_CONT) for h in range(1, LOW_H + 1)]
    names += [("split_contains_asm_lean_lo", _SIG_CONT)]
    return "".join(f"__device__ __forceinline__ void {n}{sig};\n" for n, sig in names)


def emit():
    n, bad = check_banks(body())
    return f"""// split_asm.inc -- GENERATED by tools/gen_split_asm.py; do not edit.
// The generation loop of rule 11 (8-way row split, 4 universes per wave,
// LDS exchange, the 6-LUT tail) with hand-allocated VGPRs: of its {n} VALU
// per generation only the {len(bad)} h-layer ones read two sources from one
// bank (see the generator).  {N_VGPR} VGPRs pinned.
//
// split_gens_asm_v0(r, gens, a_self, a_prev, a_next): r is gen_split's r[j]
// for S = 8; a_self / a_prev / a_next are the LDS byte addresses of this
// lane's / lane i-1's / lane i+1's 16-B slot in the wave's two 1-KiB planes
// (schedule "{VARIANTS[0]}").  The same loop with the fused Contains test
// (k_step_contains_split): split_contains_asm_batch_lo (a target window of at
// most 4 rows, the test batched over eight generations, 61 VGPRs pinned),
// split_contains_asm_batch_h<5..7> (windows of 5..7 rows, 68 pinned) and
// split_contains_asm_lean (any target, per generation, 68 pinned).  The measured
// alternatives (other schedules, two groups per wave, the round-1 contains
// bookkeeping, the per-generation test on narrower windows, a late scalar
// test) are generated into tools/tune/split_asm_tune.inc for the tuning
// build; they are only declared here.
#pragma once

namespace lifeapi_impl {{
{"".join(render_fn(f) for f in product_fns())}
{_ablation_decls()}
}}  // namespace lifeapi_impl
"""


def emit_tune():
    return f"""// split_asm_tune.inc -- GENERATED by tools/gen_split_asm.py; do not edit.
// The tuning build's variants of the rule-11 assembly loop (see
// lifeapi_amd/csrc/split_asm.inc and the generator): schedules
// {", ".join(f"v{k} = {v}" for k, v in enumerate(VARIANTS) if k)}; two groups per wave
// (split_gens_asm2); the round-1 fused-Contains bookkeeping
// (split_contains_asm); the per-generation lean test on windows of 1..7 rows
// (split_contains_asm_lean_h<h>, and _lo in the low layout), with its scalar
// part late (split_contains_asm_lean_late[_h<h>]); the batched test in the
// full layout on windows of 1..4 rows (split_contains_asm_batch_h<1..4>) and
// on any target, differences folded onto a nibble (split_contains_asm_batch_h8:
// no gain over the lean test, profiles/r06/batch_h8_ab/).
#pragma once

namespace lifeapi_impl {{
{"".join(render_fn(f) for f in tune_fns())}
}}  // namespace lifeapi_impl
"""


if __name__ == "__main__":
    texts = {OUT: emit(), OUT_TUNE: emit_tune()}
    if "--check" in sys.argv:
        sys.exit(0 if all(open(p).read() == t for p, t in texts.items()) else 1)
    for p, t in texts.items():
        with open(p, "w") as f:
            f.write(t)
    n, bad = check_banks(body())
    print(f"{OUT} (+ {OUT_TUNE}): {n} VALU, {len(bad)} with a bank conflict")
