// pair_kernels.hpp -- the offset questions of a symmetric search, with both
// operands per universe: IntersectingOffsets (Symmetry.hpp:729-772), which is
// pat2.Convolve(pat1.Transformed(t)), and the members that turn doubled
// collision coordinates into offsets, Halve / HalveX / HalveY / Skew / InvSkew
// (Symmetry.hpp:681-727).  pair.hip launches them.
//
// k_convolve_pair: out[u] = a[u].Convolve(b[u].Transformed(t)), Convolve as in
// match_kernels.hpp.  One wave per universe at a time, lane = column, U
// universes per wave with all their loads issued first; with SELF (b == a)
// each universe is loaded once.  b's transform is one Affine for the launch,
// applied in registers by affine_apply (symmetry_kernels.hpp; skipped for the
// identity).  Then the wave takes its universes one after another, so that
// everything in the walk stays wave-uniform:
//   * Convolve is symmetric in its operands (the OR over all pairs of cells
//     of the cell at their sum), and dilate's cost is that of the operand it
//     walks: 3 VALU per cell, 2 ds_bpermute_b32 per populated column.  Both
//     populations come from one DPP sum (packed in 16-bit fields: a board has
//     at most 4096 cells); the sparser operand is walked over the other one,
//     b on a tie.  The choice is four v_cndmask_b32 on the operands, so there
//     is one walk loop per universe in the code, not two.
//   * An empty operand is the sparser one, and its walk has no column to
//     visit: the result is the empty state.
// The walk itself is match_kernels.hpp's dilate with one universe: the ballot
// of populated columns, v_readlane of a column's word, s_ff1 over its rows.
//
// k_halve: HalveX and Halve take column 2 (x & 31) by load index.  HalveY and
// Halve compress the even rows of each 32-bit half into its low 16 bits
// (mask 0x55555555, then (x | x >> s) & m for s = 1, 2, 4, 8: the fixed form of
// the reference's compress_right for this mask), join the two into rows
// 0..31 and repeat them in rows 32..63.
// k_skew: column x rotated left (Skew) or right (InvSkew) by x: the halves
// exchanged in the lanes whose amount is 32 or more, then two v_alignbit_b32
// by a per-lane amount.
//
// Registers: DESIGN.md 3.14 (from build/asm; no LDS and a private segment of
// 0 in all of them).
#pragma once

#include "symmetry_kernels.hpp"

namespace lifeapi_impl {
namespace {

template <bool SELF, int U>
__global__ __launch_bounds__(kBlock) void k_convolve_pair(const uint64_t *a, const uint64_t *b, uint64_t *out,
                                                          Affine t, uint32_t plain, uint64_t n) {
  const int lane = wave_lane(), wib = wave_in_block();
  const TransposeLane c = transpose_lane(lane);
  const WaveGroups at = wave_groups<U>(wib, n);
  for (uint64_t g = at.first; g < at.groups; g += at.stride) {
    const uint64_t u0 = g * U;
    W sa[U], sb[U], tb[U];
#pragma unroll
    for (int k = 0; k < U; ++k) sa[k] = load_object(a, u0 + k, n, lane);
#pragma unroll
    for (int k = 0; k < U; ++k) {
      if constexpr (SELF) sb[k] = sa[k];
      else sb[k] = load_object(b, u0 + k, n, lane);
    }
    if (plain) {
#pragma unroll
      for (int k = 0; k < U; ++k) tb[k] = sb[k];
    } else {
      affine_apply<U>(tb, sb, t, lane, c);
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const uint32_t pops = wave_sum_u32_dpp((uint32_t)(__popc(sa[k].lo) + __popc(sa[k].hi)) |
                                             (uint32_t)(__popc(tb[k].lo) + __popc(tb[k].hi)) << 16);
      const bool walk_b = (pops >> 16) <= (pops & 0xFFFFu);
      const W pat = walk_b ? tb[k] : sa[k];
      W src[1] = {walk_b ? sa[k] : tb[k]}, acc[1] = {W{0u, 0u}};
      dilate<1>(acc, src, pat, lane);
      sa[k] = acc[0];
    }
#pragma unroll
    for (int k = 0; k < U; ++k) store_object(out, u0 + k, n, lane, sa[k]);
  }
}

// the even bits of v in the low 16 bits
__device__ __forceinline__ uint32_t even_bits(uint32_t v) {
  v &= 0x55555555u;
  v = (v | v >> 1) & 0x33333333u;
  v = (v | v >> 2) & 0x0F0F0F0Fu;
  v = (v | v >> 4) & 0x00FF00FFu;
  return (v | v >> 8) & 0x0000FFFFu;
}

// out[u] = in[u].Halve() (mode 0), HalveX() (1) or HalveY() (2); in == out is
// allowed: a wave loads its universes whole before it stores them
template <int U>
__global__ __launch_bounds__(kBlock) void k_halve(const uint64_t *in, uint64_t *out, uint32_t mode, uint64_t n) {
  const int lane = wave_lane(), wib = wave_in_block();
  const int col = mode == 2 ? lane : 2 * (lane & 31);
  const WaveGroups at = wave_groups<U>(wib, n);
  for (uint64_t g = at.first; g < at.groups; g += at.stride) {
    const uint64_t u0 = g * U;
    W s[U];
#pragma unroll
    for (int k = 0; k < U; ++k) s[k] = load_object(in, u0 + k, n, col);
    if (mode != 1) {
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const uint32_t h = even_bits(s[k].lo) | even_bits(s[k].hi) << 16;
        s[k] = W{h, h};
      }
    }
#pragma unroll
    for (int k = 0; k < U; ++k) store_object(out, u0 + k, n, lane, s[k]);
  }
}

// out[u] = in[u].Skew() (column x rotated left by x) or InvSkew() (right)
template <int U>
__global__ __launch_bounds__(kBlock) void k_skew(const uint64_t *in, uint64_t *out, uint32_t inverse, uint64_t n) {
  // (the lane spelled out: through wave_lane() this kernel's listing changes)
  const int lane = threadIdx.x & (kWave - 1), wib = wave_in_block();
  const uint32_t r = (inverse ? (uint32_t)lane : 64u - (uint32_t)lane) & 63u;  // the right-rotate
  const bool swap = (r & 32u) != 0;
  const WaveGroups at = wave_groups<U>(wib, n);
  for (uint64_t g = at.first; g < at.groups; g += at.stride) {
    const uint64_t u0 = g * U;
    W s[U];
#pragma unroll
    for (int k = 0; k < U; ++k) s[k] = load_object(in, u0 + k, n, lane);
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const W x = swap ? W{s[k].hi, s[k].lo} : s[k];
      s[k] = W{__builtin_amdgcn_alignbit(x.hi, x.lo, r & 31u), __builtin_amdgcn_alignbit(x.lo, x.hi, r & 31u)};
    }
#pragma unroll
    for (int k = 0; k < U; ++k) store_object(out, u0 + k, n, lane, s[k]);
  }
}

}  // namespace
}  // namespace lifeapi_impl
