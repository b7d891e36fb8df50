// life_gen.hpp -- the generation networks: one generation of Life on a
// column word per lane (LifeState::Step(), LifeAPI.hpp:1196-1216), by
// exchange X and network RULE.  The step kernels (step_kernels.hpp), the
// fused Step + Contains (contains_kernels.hpp) and the light-cone passes
// (cone_passes.hpp) all step with it.
#pragma once

#include "device.hpp"

namespace lifeapi_impl {
// internal linkage: every library that includes this header gets its own
// kernels (the product and the tuning build never share instantiations)
namespace {

// the vertical neighbours on the even/odd row layout (split_layout.hpp to_eo)
__device__ __forceinline__ uint32_t rotl1(uint32_t x) { return __builtin_amdgcn_alignbit(x, x, 31); }
__device__ __forceinline__ uint32_t rotr1(uint32_t x) { return __builtin_amdgcn_alignbit(x, x, 1); }

template <int X, int RULE>
__device__ __forceinline__ W life_gen(W a, uint64_t *slot, int lane) {
  if constexpr (RULE == 4) {
    // the RULE 3 network on the (E, O) layout: 18 v_bitop3 + 4 v_alignbit
    // per generation plus the exchange
    W L, R;
    neighbour_cols<X>(a, L, R, slot, lane);
    const W h0 = lut3<kXor3>(L, a, R), h1 = lut3<kMaj>(L, a, R);
    const uint32_t h0u = rotl1(h0.hi), h0d = rotr1(h0.lo);  // rows 2k-1 (for E), 2k+2 (for O)
    const uint32_t h1u = rotl1(h1.hi), h1d = rotr1(h1.lo);
    const W s0{lut3<kLe1>(h0u, h0.lo, h0.hi), lut3<kLe1>(h0.lo, h0.hi, h0d)};
    const W s1{lut3<kNae>(h0u, h0.lo, h0.hi), lut3<kNae>(h0.lo, h0.hi, h0d)};
    const W s2{lut3<kLe1>(h1u, h1.lo, h1.hi), lut3<kLe1>(h1.lo, h1.hi, h1d)};
    const W s3{lut3<kEven>(h1u, h1.lo, h1.hi), lut3<kEven>(h1.lo, h1.hi, h1d)};
    const W t1 = lut3<kT1>(s0, s1, a);
    const W t2 = lut3<kT2>(s2, a, t1);
    return lut3<kT3>(s1, s3, t2);
  }
  if constexpr (RULE == 3) {
    // row-first exchange and rotations as RULE 2, then the 7-LUT network:
    // 26 VALU per generation plus the exchange
    W L, R;
    neighbour_cols<X>(a, L, R, slot, lane);
    const W h0 = lut3<kXor3>(L, a, R), h1 = lut3<kMaj>(L, a, R);
    const W h0u = rot_up(h0), h0d = rot_dn(h0), h1u = rot_up(h1), h1d = rot_dn(h1);
    const W s0 = lut3<kLe1>(h0u, h0, h0d), s1 = lut3<kNae>(h0u, h0, h0d);
    const W s2 = lut3<kLe1>(h1u, h1, h1d), s3 = lut3<kEven>(h1u, h1, h1d);
    const W t1 = lut3<kT1>(s0, s1, a);
    const W t2 = lut3<kT2>(s2, a, t1);
    return lut3<kT3>(s1, s3, t2);
  }
  if constexpr (RULE == 14) {
    // RULE 3's exchange, h-layer and rotates with the 6-LUT tail
    // (life_tail6) per 32-bit half: 24 VALU per generation plus the exchange
    W L, R;
    neighbour_cols<X>(a, L, R, slot, lane);
    const W h0 = lut3<kXor3>(L, a, R), h1 = lut3<kMaj>(L, a, R);
    const W h0u = rot_up(h0), h0d = rot_dn(h0), h1u = rot_up(h1), h1d = rot_dn(h1);
    return W{life_tail6(h0u.lo, h0.lo, h0d.lo, h1u.lo, h1.lo, h1d.lo, a.lo),
             life_tail6(h0u.hi, h0.hi, h0d.hi, h1u.hi, h1.hi, h1d.hi, a.hi)};
  }
  if constexpr (RULE == 2) {
    // Row-first form of the same adder network.  A DPP move issues at half
    // the VALU rate on gfx950 (tools/ab/valu_probe.hip: 8 DPP of 32 instructions
    // cost 25 % of the loop), so exchange the raw column (4 DPP) instead of
    // its two vertical-sum planes (8 DPP):
    //   horizontal 3-sums  H0 = xor3(L,a,R), H1 = maj(L,a,R)   (2-bit, 0..3)
    //   vertical    FullAdd(H0 up, H0, H0 down) -> fs, fc
    //               FullAdd(H1 up, H1, H1 down) -> cs, cc
    // and the 3x3 count is again fs + 2(fc + cs) + 4cc, so the rule tail is
    // StepAlt's (LifeAPI.hpp:1251-1252).  Addition is commutative, so this is
    // bit-identical to CountRows-then-columns (LifeAPI.hpp:897-907,1218-1254).
    W L, R;
    neighbour_cols<X>(a, L, R, slot, lane);
    const W h0 = lut3<kXor3>(L, a, R), h1 = lut3<kMaj>(L, a, R);
    const W h0u = rot_up(h0), h0d = rot_dn(h0), h1u = rot_up(h1), h1d = rot_dn(h1);
    const W fs = lut3<kXor3>(h0u, h0, h0d), fc = lut3<kMaj>(h0u, h0, h0d);
    const W cs = lut3<kXor3>(h1u, h1, h1d), cc = lut3<kMaj>(h1u, h1, h1d);
    const W b2 = lut3<kCarry2>(cc, fc, cs);
    const W p = lut3<kLive>(fs, b2, a);
    const W q = lut3<kXor3>(fc, cs, b2);
    return W{p.lo & q.lo, p.hi & q.hi};
  }
  const W up = rot_up(a), dn = rot_dn(a);
  if constexpr (RULE == 0) {
    // CountRows (LifeAPI.hpp:897-907): vertical 3-sum as two planes
    const W c0 = lut3<kXor3>(up, dn, a);
    const W c1 = lut3<kMaj>(up, dn, a);
    W L0, R0, L1, R1;
    neighbours<X>(c0, c1, L0, R0, L1, R1, slot, lane);
    // FullAdd x2 (LifeAPI.hpp:826-833, StepAlt :1246-1249): 3x3 inclusive
    // count = fs + 2(fc + cs) + 4cc
    const W fs = lut3<kXor3>(L0, c0, R0), fc = lut3<kMaj>(L0, c0, R0);
    const W cs = lut3<kXor3>(L1, c1, R1), cc = lut3<kMaj>(L1, c1, R1);
    // StepAlt :1251-1252: cc ^= fc & cs;  next = (fs^cc) & (fc^cs^cc) & (a|fs)
    const W b2 = lut3<kCarry2>(cc, fc, cs);
    const W p = lut3<kLive>(fs, b2, a);
    const W q = lut3<kXor3>(fc, cs, b2);
    return W{p.lo & q.lo, p.hi & q.hi};
  } else {
    // the same network in plain and/or/xor (the compiler folds the DPP moves
    // into v_*_dpp consumers); kept as an ablation of the bitop3 form
    const uint64_t av = join(a), u = join(up), d = join(dn);
    const uint64_t c0v = u ^ d ^ av, c1v = (u & d) | ((u ^ d) & av);
    W L0, R0, L1, R1;
    neighbours<X>(split(c0v), split(c1v), L0, R0, L1, R1, slot, lane);
    const uint64_t l0 = join(L0), r0 = join(R0), l1 = join(L1), r1 = join(R1);
    const uint64_t h0 = l0 ^ c0v, h1 = l1 ^ c1v;
    const uint64_t fs = h0 ^ r0, fc = (l0 & c0v) | (r0 & h0);
    const uint64_t cs = h1 ^ r1;
    uint64_t cc = (l1 & c1v) | (r1 & h1);
    cc ^= fc & cs;
    return split((fs ^ cc) & (fc ^ cs ^ cc) & (av | fs));
  }
}

}  // namespace
}  // namespace lifeapi_impl
