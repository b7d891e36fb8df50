// weld_kernels.hpp -- making LifeWelds and what a search derives from them:
// LifeWeld::FromRequired (LifeWeld.hpp:133-159), ToTarget (:188-191), ToStable()
// and ToStable(active, duration, mask) (:279-400) and InteractionOffsets(const
// LifeWeld &) (:206-245).  weld.hip launches them.
//
// One wave per object, lane = column, natural layout: LifeWeld = {state,
// frozen2, frozen1, frozen0} x 64 words, LifeStable = {state, unknown, live2,
// live3, dead0, dead1, dead2, dead4, dead5, dead6} x 64 words (member order).
// ZOI() is the 3 x 3 dilation (rot_up / rot_dn, then the neighbour columns by
// DPP); the inclusive 3 x 3 count is count4 (match_kernels.hpp); the loop over
// the groups is wave_groups.hpp's.  All four functions are total: nothing is assumed about
// the planes (frozen counts on live cells, `required` unrelated to the state,
// `active` over the state are all computed as the reference computes them).
//
// ToStable(active, duration, mask).  The reference replays the reaction twice,
// once collecting everActive and once restricting options.  Every update is an
// OR into an option plane or an AND-NOT into unknown, with operands that do
// not depend on the stable being built, so one replay does both
// (tests/test_weld_model.py proves the two forms equal).  A generation with
// next == current repeats itself for ever and adds nothing new: the loop stops
// after it.  Option planes are "1 = ruled out"; RestrictOptions(cells, opts)
// ORs cells into every plane not in opts (LifeStable.hpp:308-318).
//
// InteractionOffsets(weld).  The seven convolutions of
// LifeState::InteractionOffsets, the overlap term as it is, each plane of the
// other six masked by keep = (state & ~frozen2 & ~frozen1 & ~frozen0).ZOI() --
// with one oddity that is reproduced bit for bit: in both birth terms the
// SECOND operand is masked by the FIRST operand's side (LifeWeld.hpp:238-239):
//   (a_dead1 & a_keep) x (b_dead2 & a_keep)      b's plane under a's mask
//   (b_dead1 & b_keep) x (a_dead2 & b_keep)      a's plane under b's mask
// (b's planes and b_keep are those of Mirrored(b)).  The first pattern thus
// differs per universe and takes one dilate<1> each; the second is a's plane
// under a wave-uniform mask and stays a dilate<U>.
//
// Registers (build/asm, gfx950; .private_segment_fixed_size 0 and no LDS in
// all four):
//   k_weld_from_required<2>         48 VGPRs, 8 waves per SIMD
//   k_weld_to_target<4>             28 VGPRs, 8 waves per SIMD
//   k_weld_to_stable                71 VGPRs, 7 waves per SIMD
//   k_weld_interaction_offsets<2>   79 VGPRs, 6 waves per SIMD
// k_weld_to_stable holds one weld per wave: its four planes, the six
// exact-count planes of its state, current, everActive, the mask and eight
// option planes stay in registers across the generation loop; two welds per
// wave would need about 130 (3 waves per SIMD): not built.
// Measured on 1M objects (profiles/r14/README.md): FromRequired and ToTarget
// 3.3-3.6 x the 1-generation step's time, ToStable() 8.2 x (bytes-bound, at
// 0.84-0.92 of the step's bytes per second), ToStable(active, 40, mask) 9.5 ms,
// InteractionOffsets with an eater's weld 4.1 x.
#pragma once

#include "match_kernels.hpp"

namespace lifeapi_impl {
namespace {

// ZOI(): the 3 x 3 dilation
__device__ __forceinline__ uint64_t zoi(uint64_t a, int lane) {
  const W s = split(a);
  const W v = lut3<kOr3>(s, rot_up(s), rot_dn(s));
  W L, R;
  neighbour_cols<XDPP>(v, L, R, nullptr, lane);
  return join(lut3<kOr3>(v, L, R));
}

// count + the frozen 3-bit number, bit3 = count.bit3 ^ the last carry
// (LifeWeld.hpp:295-299); Step() uses bits 2..0 of it (:177-185)
__device__ __forceinline__ Count4 add_frozen(const Count4 &c, uint64_t f2, uint64_t f1, uint64_t f0) {
  const uint64_t k0 = c.b0 & f0;
  const uint64_t k1 = (c.b1 & f1) | (c.b1 & k0) | (f1 & k0);
  const uint64_t k2 = (c.b2 & f2) | (c.b2 & k1) | (f2 & k1);
  return Count4{c.b3 ^ k2, c.b2 ^ f2 ^ k1, c.b1 ^ f1 ^ k0, c.b0 ^ f0};
}
// the Life rule on bits 2..0 of an inclusive sum
__device__ __forceinline__ uint64_t rule(const Count4 &s, uint64_t state) {
  return (s.b0 ^ s.b2) & (s.b1 ^ s.b2) & (state | s.b0);
}

// a plane held as one 64-bit word, stored as ld<true> loads (spelled out, not
// st<true>(p, split(v)): the trip through the halves changes the listings of
// k_weld_from_required and k_weld_to_target)
__device__ __forceinline__ void stw(uint64_t *p, uint64_t v) { __builtin_nontemporal_store(v, p); }

// welds[u] = LifeWeld::FromRequired(states[u], required[per ? u : 0])
template <int U>
__global__ __launch_bounds__(kBlock) void k_weld_from_required(const uint64_t *__restrict__ states,
                                                               const uint64_t *__restrict__ required, uint32_t per,
                                                               uint64_t *__restrict__ welds, uint64_t n) {
  const int lane = wave_lane(), wib = wave_in_block();
  const WaveGroups at = wave_groups<U>(wib, n);
  for (uint64_t g = at.first; g < at.groups; g += at.stride) {
    const uint64_t u0 = g * U;
    uint64_t s[U], r[U];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const bool ok = u0 + k < n;  // (one guard for the planes: a load_object each changes the listing)
      s[k] = ok ? join(ld<true>(states + (u0 + k) * kWave + lane)) : 0;
      r[k] = ok ? (per ? join(ld<true>(required + (u0 + k) * kWave + lane)) : required[lane]) : 0;
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const uint64_t active = zoi(s[k], lane) & ~r[k], za = zoi(active, lane);
      const uint64_t stator = s[k] & ~za, kept = s[k] & ~stator;
      // the frozen cells: required ones next to the active region, and
      // births the kept part would have on its own
      const uint64_t frozen = (za & r[k]) | (rule(count4(kept, lane), kept) & ~kept);
      const Count4 c = count4(stator, lane);
      if (u0 + k < n) {  // (one guard for the planes, as above)
        uint64_t *q = welds + (u0 + k) * 4 * kWave + lane;
        stw(q, kept);
        stw(q + kWave, c.b2 & frozen);
        stw(q + 2 * kWave, c.b1 & frozen);
        stw(q + 3 * kWave, c.b0 & frozen);
      }
    }
  }
}

// (wanted[u], unwanted[u]) = welds[u].ToTarget()
template <int U>
__global__ __launch_bounds__(kBlock) void k_weld_to_target(const uint64_t *__restrict__ welds,
                                                           uint64_t *__restrict__ wanted,
                                                           uint64_t *__restrict__ unwanted, uint64_t n) {
  const int lane = wave_lane(), wib = wave_in_block();
  const WaveGroups at = wave_groups<U>(wib, n);
  for (uint64_t g = at.first; g < at.groups; g += at.stride) {
    const uint64_t u0 = g * U;
    uint64_t s[U], f[U];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const uint64_t *p = welds + (u0 + k) * 4 * kWave + lane;
      const bool ok = u0 + k < n;  // (one guard for the planes: a load_object each changes the listing)
      s[k] = ok ? join(ld<true>(p)) : 0;
      f[k] = ok ? join(ld<true>(p + kWave)) | join(ld<true>(p + 2 * kWave)) | join(ld<true>(p + 3 * kWave)) : 0;
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const uint64_t uw = zoi(s[k] & ~f[k], lane) & ~s[k];
      if (u0 + k < n) {  // (one guard for the planes, as above)
        stw(wanted + (u0 + k) * kWave + lane, s[k]);
        stw(unwanted + (u0 + k) * kWave + lane, uw);
      }
    }
  }
}

// stables[u] = welds[u].ToStable(active, duration, mask); duration == 0 is
// ToStable().  active: null (empty), one state (per == 0) or one per weld;
// mask: null (all ones) or one state.  One weld per wave.
__global__ __launch_bounds__(kBlock) void k_weld_to_stable(const uint64_t *__restrict__ welds,
                                                           const uint64_t *__restrict__ active, uint32_t per,
                                                           const uint64_t *__restrict__ mask, uint32_t duration,
                                                           uint64_t *__restrict__ stables, uint64_t n) {
  const int lane = wave_lane(), wib = wave_in_block();
  const uint64_t m = mask ? mask[lane] : ~0ull;
  const WaveGroups at = wave_groups<1>(wib, n);
  for (uint64_t u = at.first; u < at.groups; u += at.stride) {
    const uint64_t *p = welds + u * 4 * kWave + lane;
    const uint64_t s = join(ld<true>(p)), f2 = join(ld<true>(p + kWave)), f1 = join(ld<true>(p + 2 * kWave)),
                   f0 = join(ld<true>(p + 3 * kWave));
    uint64_t cur = s;
    if (active && duration) cur |= per ? join(ld<true>(active + u * kWave + lane)) : active[lane];

    // ---- ToStable() (LifeWeld.hpp:279-325) ----
    const Count4 sc = count4(s, lane);
    const uint64_t frozen = f2 | f1 | f0;
    const uint64_t off = ~s & zoi(s & ~frozen, lane);  // SetOff; SetOn is s
    uint64_t live2, live3, dead0, dead1, dead2, dead4, dead5, dead6;
    {
      const Count4 sum = add_frozen(sc, f2, f1, f0);  // (the sum includes the centre)
      const uint64_t fl = frozen & s, fd = frozen & ~s;
      const uint64_t l2 = fl & sum.exactly(3), l3 = fl & sum.exactly(4);
      const uint64_t d1 = fd & sum.exactly(1), d2 = fd & sum.exactly(2), d4 = fd & sum.exactly(4),
                     d5 = fd & sum.exactly(5), d6 = fd & sum.exactly(6);
      const uint64_t anyd = d1 | d2 | d4 | d5 | d6, anyl = l2 | l3;
      live2 = off | l3 | anyd;
      live3 = off | l2 | anyd;
      const uint64_t base = s | anyl;
      dead0 = base | anyd;
      dead1 = base | d2 | d4 | d5 | d6;
      dead2 = base | d1 | d4 | d5 | d6;
      dead4 = base | d1 | d2 | d5 | d6;
      dead5 = base | d1 | d2 | d4 | d6;
      dead6 = base | d1 | d2 | d4 | d5;
    }

    // ---- the replay (LifeWeld.hpp:327-400), both of the reference's loops in one ----
    uint64_t ever = 0;
    if (duration) {
      const uint64_t s0 = sc.exactly(0), s1 = sc.exactly(1), s2 = sc.exactly(2), s4 = sc.exactly(4),
                     s5 = sc.exactly(5), s6 = sc.exactly(6);
      for (uint32_t g = 0; g < duration; ++g) {
        ever |= s ^ cur;
        const Count4 cc = count4(cur, lane);
        const uint64_t next = rule(add_frozen(cc, f2, f1, f0), cur);
        const uint64_t dead = m & ~s & ~cur, born = dead & next, stay = dead & ~next;
        const uint64_t c0 = stay & cc.exactly(0), c1 = stay & cc.exactly(1), c2 = stay & cc.exactly(2),
                       c3 = stay & cc.exactly(3), b3 = born & cc.exactly(3);
        const uint64_t r0 = b3 & s0, r1 = b3 & s1, r2 = b3 & s2, rb = r0 | r1 | r2;
        live2 |= rb;
        live3 |= rb;
        dead0 |= r1 | r2;
        dead1 |= r0 | r2 | (c2 & s0);
        dead2 |= r0 | r1 | (c1 & s0) | (c2 & s1);
        dead4 |= rb | (c1 & s2) | (c3 & s4);
        dead5 |= rb | (c0 & s2) | (c2 & s4) | (c3 & s5);
        dead6 |= rb | (c1 & s4) | (c2 & s5) | (c3 & s6);
        const bool fixed = __ballot(next != cur) == 0ull;
        cur = next;
        if (fixed) break;  // every later generation repeats this one
      }
    }
    const uint64_t was = m & ~s & ever;  // SetOff(mask & ~state & everActive)
    uint64_t *q = stables + u * 10 * kWave + lane;
    stw(q, s);
    stw(q + kWave, ~(s | off | was));
    stw(q + 2 * kWave, live2 | was);
    stw(q + 3 * kWave, live3 | was);
    stw(q + 4 * kWave, dead0);
    stw(q + 5 * kWave, dead1);
    stw(q + 6 * kWave, dead2);
    stw(q + 7 * kWave, dead4);
    stw(q + 8 * kWave, dead5);
    stw(q + 9 * kWave, dead6);
  }
}

// (x, y) -> (-x, -y) of a plane whose column j is p[j]: this lane's column
__device__ __forceinline__ uint64_t mirrored_col(const uint64_t *p, int lane) {
  const uint64_t o = __builtin_bitreverse64(p[(kWave - lane) & (kWave - 1)]);
  return o << 1 | o >> 63;
}

// out[u] = welds[u].InteractionOffsets(other), other one LifeWeld
template <int U>
__global__ __launch_bounds__(kBlock) void k_weld_interaction_offsets(const uint64_t *__restrict__ welds,
                                                                     const uint64_t *__restrict__ other,
                                                                     uint64_t *__restrict__ out, uint64_t n) {
  const int lane = wave_lane(), wib = wave_in_block();
  W bp[7], bkeep;  // Mirrored(other)'s planes, 1..6 under its own mask, but
  W bdead2;        // dead2 kept unmasked as well: the first birth term masks it by a's side
  {
    const uint64_t bs = mirrored_col(other, lane);
    const uint64_t bf = mirrored_col(other + kWave, lane) | mirrored_col(other + 2 * kWave, lane) |
                        mirrored_col(other + 3 * kWave, lane);
    bkeep = split(zoi(bs & ~bf, lane));  // (ZOI commutes with Mirrored)
    interaction_planes(split(bs), bp, lane);
    bdead2 = bp[2];
#pragma unroll
    for (int i = 1; i < 7; ++i) bp[i] = W{bp[i].lo & bkeep.lo, bp[i].hi & bkeep.hi};
  }
  const WaveGroups at = wave_groups<U>(wib, n);
  for (uint64_t g = at.first; g < at.groups; g += at.stride) {
    const uint64_t u0 = g * U;
    W s[U], keep[U], acc[U], ap[U][7];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const uint64_t *p = welds + (u0 + k) * 4 * kWave + lane;
      const bool ok = u0 + k < n;  // (one guard for the planes: a load_object each changes the listing)
      s[k] = ok ? ld<true>(p) : W{0u, 0u};
      keep[k] = ok ? split(join(ld<true>(p + kWave)) | join(ld<true>(p + 2 * kWave)) | join(ld<true>(p + 3 * kWave))) : W{0u, 0u};
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
      keep[k] = split(zoi(join(s[k]) & ~join(keep[k]), lane));
      interaction_planes(s[k], ap[k], lane);
      acc[k] = W{0u, 0u};
    }
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      if (i == 1) {
        // (a_dead1 & a_keep) x (b_dead2 & a_keep): the pattern is this universe's own
#pragma unroll
        for (int k = 0; k < U; ++k) {
          W one[1] = {acc[k]};
          const W src[1] = {W{ap[k][1].lo & keep[k].lo, ap[k][1].hi & keep[k].hi}};
          dilate<1>(one, src, W{bdead2.lo & keep[k].lo, bdead2.hi & keep[k].hi}, lane);
          acc[k] = one[0];
        }
        continue;
      }
      // i == 2 is (b_dead1 & b_keep) x (a_dead2 & b_keep): a's plane under b's mask
      W src[U];
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const W mk = i == 0 ? W{~0u, ~0u} : i == 2 ? bkeep : keep[k];
        src[k] = W{ap[k][i].lo & mk.lo, ap[k][i].hi & mk.hi};
      }
      dilate<U>(acc, src, bp[kPartner[i]], lane);
    }
#pragma unroll
    for (int k = 0; k < U; ++k) store_object(out, u0 + k, n, lane, acc[k]);
  }
}

}  // namespace
}  // namespace lifeapi_impl
