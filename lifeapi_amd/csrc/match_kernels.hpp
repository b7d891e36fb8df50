// match_kernels.hpp -- the per-offset questions of a search loop: Match
// (LifeTarget.hpp:53-55 -> MatchLiveAndDead, LifeAPI.hpp:432-435), Convolve
// (LifeAPI.hpp:1293-1370) and InteractionOffsets (LifeAPI.hpp:1066-1095).
// match.hip launches them.
//
// With s(x, y) = bit y of column x, indices mod 64:
//   Convolve(A, B)(x, y) = OR  over (a, b) in B of A(x - a, y - b)
//   Match(w, u)(x, y)    = AND over (a, b) in w of  s(x + a, y + b)
//                        & AND over (a, b) in u of ~s(x + a, y + b)
// One wave per universe, lane = column, U universes per wave with their loads
// issued first (the loop and the guarded loads and stores: wave_groups.hpp).
// The pattern is one for the launch: each wave loads its 64
// words once (lane j = column j) and walks its cells in scalar loops -- the
// populated columns from a ballot, a column's word from v_readlane, the set
// rows from s_ff1.  For pattern column a the universe's column x -+ a comes
// from one ds_bpermute per 32-bit half; for row b that word is rotated by b,
// which is wave-uniform: two v_alignbit_b32 on the halves, taken straight for
// b < 32 and swapped for b >= 32 (two loops, so the swap is a renaming).  Two
// rotated terms are folded into the accumulator per v_bitop3_b32.  Match
// forms neither Mirrored() nor the complements the reference convolves: it
// accumulates all_w &= rotr(t, b) and any_u |= rotr(t, b), and the answer is
// all_w & ~any_u.
//
// The work is proportional to the pattern's population: per universe and pair
// of cells of one column half, 4 v_alignbit_b32 + 2 v_bitop3_b32 (3 VALU per
// cell), per populated column 2 ds_bpermute_b32.  A pattern of many cells, up
// to the whole board (4096 cells), takes the same loops and is correct, only
// slow in proportion; there is no separate path for it.  Runs of consecutive
// rows are taken bit by bit (the reference's run trick, LifeAPI.hpp:1309-1366,
// by doubling: not built, not measured; by instruction count a run of 7 rows
// would take 16 VALU against 22, a run of 4 the same 12, profiles/r11/README.md).
//
// Registers (build/asm, gfx950; .private_segment_fixed_size 0 and no LDS in
// all three):
//   k_match<4>                 60 VGPRs, 8 waves per SIMD
//   k_convolve<4>              51 VGPRs, 8 waves per SIMD
//   k_interaction_offsets<2>   67 VGPRs, 7 waves per SIMD
// Measured on 1M universes (profiles/r11/README.md): Match of a block and its
// ring 1.10 x the 1-generation step's time, Convolve with the 3 x 3 block
// 1.11 x (bytes-bound), a 5 x 5 target 1.29-1.43 x, InteractionOffsets with
// an eater 5.2-5.4 x (issue-bound).
#pragma once

#include "wave_groups.hpp"

namespace lifeapi_impl {
namespace {

constexpr uint32_t kOr3 = (TA | TB | TC) & 0xFF, kAnd3 = (TA & TB & TC) & 0xFF;

// t rotated right by s rows, s < 32 wave-uniform (an SGPR shift operand)
__device__ __forceinline__ W rotr_lt32(W t, uint32_t s) {
  return W{__builtin_amdgcn_alignbit(t.hi, t.lo, s), __builtin_amdgcn_alignbit(t.lo, t.hi, s)};
}

// acc[k] (&|)= rotr(t[k], b) for every set bit b of `rows` (wave-uniform),
// two terms per v_bitop3
template <int U, bool AND>
__device__ __forceinline__ void fold_rows(W (&acc)[U], const W (&t)[U], uint32_t rows) {
  while (rows) {
    const uint32_t b0 = (uint32_t)__builtin_ctz(rows);
    rows &= rows - 1;
    if (rows) {
      const uint32_t b1 = (uint32_t)__builtin_ctz(rows);
      rows &= rows - 1;
#pragma unroll
      for (int k = 0; k < U; ++k)
        acc[k] = lut3<AND ? kAnd3 : kOr3>(acc[k], rotr_lt32(t[k], b0), rotr_lt32(t[k], b1));
    } else {
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const W r = rotr_lt32(t[k], b0);
        acc[k] = AND ? W{acc[k].lo & r.lo, acc[k].hi & r.hi} : W{acc[k].lo | r.lo, acc[k].hi | r.hi};
      }
    }
  }
}
// the same for a 64-bit set of rotations: rows >= 32 on the swapped halves
template <int U, bool AND>
__device__ __forceinline__ void fold_rows64(W (&acc)[U], const W (&t)[U], uint32_t rows_lo, uint32_t rows_hi) {
  fold_rows<U, AND>(acc, t, rows_lo);
  if (rows_hi) {
    W x[U];
#pragma unroll
    for (int k = 0; k < U; ++k) x[k] = W{t[k].hi, t[k].lo};
    fold_rows<U, AND>(acc, x, rows_hi);
  }
}

// column (lane + d) mod 64 of each of the wave's universes, d wave-uniform
template <int U>
__device__ __forceinline__ void fetch_cols(W (&t)[U], const W (&s)[U], int lane, uint32_t d) {
  const int at = (int)(((uint32_t)lane + d) & (kWave - 1)) << 2;
#pragma unroll
  for (int k = 0; k < U; ++k)
    t[k] = W{(uint32_t)__builtin_amdgcn_ds_bpermute(at, (int)s[k].lo),
             (uint32_t)__builtin_amdgcn_ds_bpermute(at, (int)s[k].hi)};
}

__device__ __forceinline__ uint64_t readlane64(W v, uint32_t l) {
  return (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)v.lo, (int)l) |
         (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)v.hi, (int)l) << 32;
}

// acc[k] |= Convolve(src[k], pattern) (LifeAPI.hpp:1293-1370), the pattern's
// column j in lane j (pat): cell (a, b) ORs in column x - a rotated LEFT by b
// = right by -b, so the set of right rotations is the column's word with bit
// b moved to bit -b mod 64 (a bit reversal and one rotate, scalar)
template <int U>
__device__ __forceinline__ void dilate(W (&acc)[U], const W (&src)[U], W pat, int lane) {
  uint64_t cols = __ballot((pat.lo | pat.hi) != 0u);
  while (cols) {
    const uint32_t a = (uint32_t)__builtin_ctzll(cols);
    cols &= cols - 1;
    const uint64_t word = readlane64(pat, a), rev = __builtin_bitreverse64(word);
    const uint64_t rows = rev << 1 | rev >> 63;
    W t[U];
    fetch_cols<U>(t, src, lane, (uint32_t)kWave - a);
    fold_rows64<U, false>(acc, t, (uint32_t)rows, (uint32_t)(rows >> 32));
  }
}

// out[u] = in[u].Match(LifeTarget{wanted, unwanted}); count[u] = its
// population.  out or count may be null (not both).  in == out is allowed:
// a wave loads its universes before it stores them and touches no other's.
template <int U>
__global__ __launch_bounds__(kBlock) void k_match(const uint64_t *in, uint64_t *out,
                                                  const uint64_t *__restrict__ wanted,
                                                  const uint64_t *__restrict__ unwanted,
                                                  uint32_t *__restrict__ count, uint64_t n) {
  const int lane = wave_lane(), wib = wave_in_block();
  const W w = split(wanted[lane]), uw = split(unwanted[lane]);
  const uint64_t care = __ballot((w.lo | w.hi | uw.lo | uw.hi) != 0u);
  const WaveGroups at = wave_groups<U>(wib, n);
  for (uint64_t g = at.first; g < at.groups; g += at.stride) {
    const uint64_t u0 = g * U;
    W s[U], all[U], any[U];
#pragma unroll
    for (int k = 0; k < U; ++k) s[k] = load_object(in, u0 + k, n, lane);
#pragma unroll
    for (int k = 0; k < U; ++k) {
      all[k] = W{~0u, ~0u};
      any[k] = W{0u, 0u};
    }
    for (uint64_t cols = care; cols;) {
      const uint32_t a = (uint32_t)__builtin_ctzll(cols);
      cols &= cols - 1;
      const uint64_t ww = readlane64(w, a), wu = readlane64(uw, a);
      W t[U];
      fetch_cols<U>(t, s, lane, a);
      fold_rows64<U, true>(all, t, (uint32_t)ww, (uint32_t)(ww >> 32));
      fold_rows64<U, false>(any, t, (uint32_t)wu, (uint32_t)(wu >> 32));
    }
    W m[U];
#pragma unroll
    for (int k = 0; k < U; ++k) m[k] = W{all[k].lo & ~any[k].lo, all[k].hi & ~any[k].hi};
    if (out) {
#pragma unroll
      for (int k = 0; k < U; ++k) store_object(out, u0 + k, n, lane, m[k]);
    }
    if (count) {
      uint32_t h = 0;  // lanes 0 .. U-1 store the U wave-uniform counts with one vector store
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const uint32_t c = wave_sum_u32_dpp((uint32_t)(__popc(m[k].lo) + __popc(m[k].hi)));
        h = lane == k ? c : h;
      }
      // (spelled out: through holds_scalar this kernel's listing changes)
      if (lane < U && u0 + (uint64_t)lane < n) count[u0 + lane] = h;
    }
  }
}

// out[u] = in[u].Convolve(pattern); in == out allowed as above
template <int U>
__global__ __launch_bounds__(kBlock) void k_convolve(const uint64_t *in, uint64_t *out,
                                                     const uint64_t *__restrict__ pattern, uint64_t n) {
  const int lane = wave_lane(), wib = wave_in_block();
  const W pat = split(pattern[lane]);
  const WaveGroups at = wave_groups<U>(wib, n);
  for (uint64_t g = at.first; g < at.groups; g += at.stride) {
    const uint64_t u0 = g * U;
    W s[U], acc[U];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      s[k] = load_object(in, u0 + k, n, lane);
      acc[k] = W{0u, 0u};
    }
    dilate<U>(acc, s, pat, lane);
#pragma unroll
    for (int k = 0; k < U; ++k) store_object(out, u0 + k, n, lane, acc[k]);
  }
}

// The inclusive 3 x 3 count as four planes (CountNeighbourhood, LifeAPI.hpp:
// 909-952, NeighbourCount.hpp:40-70): column-first, the two planes of each
// column's vertical triple, then the FullAdds across the neighbour columns and
// the carry.  (k_counts, stencil_kernels.hpp, has the same network inside the
// kernel: a tuned family, left as it is.)
struct Count4 {
  uint64_t b3, b2, b1, b0;
  __device__ __forceinline__ uint64_t exactly(unsigned n) const {
    return (n & 1 ? b0 : ~b0) & (n & 2 ? b1 : ~b1) & (n & 4 ? b2 : ~b2) & (n & 8 ? b3 : ~b3);
  }
};
__device__ __forceinline__ Count4 count4(uint64_t s, int lane) {
  const W a = split(s), up = rot_up(a), dn = rot_dn(a);
  const W c0 = lut3<kXor3>(up, dn, a), c1 = lut3<kMaj>(up, dn, a);
  W L0, R0, L1, R1;
  neighbours<XDPP>(c0, c1, L0, R0, L1, R1, nullptr, lane);
  const uint64_t fs = join(lut3<kXor3>(L0, c0, R0)), fc = join(lut3<kMaj>(L0, c0, R0));
  const uint64_t cs = join(lut3<kXor3>(L1, c1, R1)), cc = join(lut3<kMaj>(L1, c1, R1));
  const uint64_t carry = fc & cs;
  return Count4{cc & carry, cc ^ carry, fc ^ cs, fs};
}

// The seven planes InteractionOffsets convolves, of one side (LifeAPI.hpp:
// 1067-1093; the other side's partner of plane i is kPartner[i]):
//   0 state                         3 count == 3 & state
//   1 count == 1 & ~state           4 count >= 4 & state
//   2 count == 2 & ~state           5 count >= 2 & ~state
//                                   6 count >= 1 & ~state
// count = the inclusive 3x3 count (count4).
constexpr int kPartner[7] = {0, 2, 1, 5, 6, 3, 4};
__device__ __forceinline__ void interaction_planes(W a, W (&p)[7], int lane) {
  const uint64_t s = join(a);
  const Count4 c = count4(s, lane);
  const uint64_t b0 = c.b0, b1 = c.b1, hi = c.b3 | c.b2;
  p[0] = a;
  p[1] = split(~hi & ~b1 & b0 & ~s);
  p[2] = split(~hi & b1 & ~b0 & ~s);
  p[3] = split(~hi & b1 & b0 & s);
  p[4] = split(hi & s);
  p[5] = split((hi | b1) & ~s);
  p[6] = split((hi | b1 | b0) & ~s);
}

// out[u] = in[u].InteractionOffsets(other): the OR of seven convolutions of
// a plane of the universe with a plane of Mirrored(other) (LifeAPI.hpp:789-795:
// (x, y) -> (-x, -y), a lane reversal, a bit reversal and one row rotate),
// whose planes each wave derives once and keeps in registers
template <int U>
__global__ __launch_bounds__(kBlock) void k_interaction_offsets(const uint64_t *in, uint64_t *out,
                                                                const uint64_t *__restrict__ other, uint64_t n) {
  const int lane = wave_lane(), wib = wave_in_block();
  W bp[7];
  {
    const uint64_t o = __builtin_bitreverse64(other[(kWave - lane) & (kWave - 1)]);
    interaction_planes(split(o << 1 | o >> 63), bp, lane);
  }
  const WaveGroups at = wave_groups<U>(wib, n);
  for (uint64_t g = at.first; g < at.groups; g += at.stride) {
    const uint64_t u0 = g * U;
    W s[U], acc[U], ap[U][7];
#pragma unroll
    for (int k = 0; k < U; ++k) s[k] = load_object(in, u0 + k, n, lane);
#pragma unroll
    for (int k = 0; k < U; ++k) {
      interaction_planes(s[k], ap[k], lane);
      acc[k] = W{0u, 0u};
    }
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      W src[U];
#pragma unroll
      for (int k = 0; k < U; ++k) src[k] = ap[k][i];
      dilate<U>(acc, src, bp[kPartner[i]], lane);
    }
#pragma unroll
    for (int k = 0; k < U; ++k) store_object(out, u0 + k, n, lane, acc[k]);
  }
}

}  // namespace
}  // namespace lifeapi_impl
