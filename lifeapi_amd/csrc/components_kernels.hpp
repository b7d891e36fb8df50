// components_kernels.hpp -- the connected-component family over a batch:
// FirstOn / FirstCell (LifeAPI.hpp:301-323, 358), ComponentContaining
// (LifeAPI.hpp:655-665, 1184-1188) and Components (LifeAPI.hpp:667-676,
// 1189-1193).  components.hip launches them.
//
// With N(t) = t.Convolve(corona) & state, ComponentContaining(seed, corona) is
// the least R with R = N(seed) | N(R).  One wave per universe, lane = column,
// the universe, the result and the frontier in VGPRs for the whole flood:
//   result = 0; front = seed
//   repeat: nb = N(front); front = nb & ~result; result |= nb
//   until no lane of the wave gained a cell (one ballot, a wave-uniform branch)
// which is the reference's own loop (its exit test taken after the round, so
// an empty seed costs one round of zeros).  Every round but the last adds a
// cell, so at most 4096 rounds run; the loop carries that bound (kMaxRounds)
// so that no mistake in the exit test can spin a wave.
//
// The dilation front.Convolve(corona):
//   kDefault, k3x3, kPlus   the reference's default corona (the 21 cells with
//             |a|, |b| <= 2, |a| + |b| < 4), the 3 x 3 block and the 5-cell
//             plus, all centred: neighbour columns by DPP wave rotates (x -+ 1
//             one move, x -+ 2 two), rows by v_alignbit_b32 on the halves,
//             merged by v_bitop3_b32.  For the default corona, with
//             u1 = f[x-1] | f[x] | f[x+1] and u2 = f[x-2] | f[x+2]:
//               t = u1 | u2;  new = t | rot+-1(t) | rot+-2(u1)
//             (8 DPP moves, 8 v_alignbit_b32 and 7 v_bitop3_b32 per universe
//             and round).  No LDS crossbar.
//   kGeneral  any other corona: dilate<U> of match_kernels.hpp, the corona's
//             columns in lanes (two ds_bpermute_b32 per populated column and
//             universe, 3 VALU per cell).
// The corona arrives by value in the kernel's arguments (512 bytes), so a
// launch owns no staging buffer.
//
// Components(corona): the wave loops over the components of its universe --
// FirstOn of what remains on the scalar unit (the populated columns from a
// ballot, the last populated group of four columns by s_flbit, its first
// populated column by s_ff1, that column's word by v_readlane, its lowest row
// by s_ff1), the flood from that cell inside what remains, one coalesced
// 512-byte store of the component while it is below the cap, remaining &=
// ~component.  Each component holds its seed because the corona holds (0, 0)
// (the host rejects any other), so at most 4096 components exist; the loop
// carries that bound (kMaxComponents).
//
// Registers (build/asm, gfx950; .private_segment_fixed_size 0 and no LDS in
// all of them) and the measurements are in DESIGN.md 3.10.
#pragma once

#include "match_kernels.hpp"

namespace lifeapi_impl {

struct Corona {  // a kernel argument by value: word x = column x, as a LifeState
  uint64_t w[kWave];
};

enum CoronaKind { kGeneral = 0, kDefault = 1, k3x3 = 2, kPlus = 3 };

constexpr uint32_t kMaxRounds = 4096, kMaxComponents = 4096;

namespace {

// rotates by K rows, 0 < K < 32: up is rotl (cell y <- y - K)
template <int K>
__device__ __forceinline__ W rot_up_by(W a) {
  return W{__builtin_amdgcn_alignbit(a.lo, a.hi, 32 - K), __builtin_amdgcn_alignbit(a.hi, a.lo, 32 - K)};
}
template <int K>
__device__ __forceinline__ W rot_dn_by(W a) {
  return W{__builtin_amdgcn_alignbit(a.hi, a.lo, K), __builtin_amdgcn_alignbit(a.lo, a.hi, K)};
}
__device__ __forceinline__ W or3(W a, W b, W c) { return lut3<kOr3>(a, b, c); }
__device__ __forceinline__ W col_prev(W a) { return W{dpp_prev(a.lo), dpp_prev(a.hi)}; }
__device__ __forceinline__ W col_next(W a) { return W{dpp_next(a.lo), dpp_next(a.hi)}; }

// f.Convolve(corona) for the three centred coronas (all symmetric in both axes)
template <int KIND>
__device__ __forceinline__ W dilate_fixed(W f) {
  static_assert(KIND == kDefault || KIND == k3x3 || KIND == kPlus, "the coronas with a fixed network");
  const W p = col_prev(f), q = col_next(f);
  if constexpr (KIND == kPlus) {
    const W v = or3(f, rot_up(f), rot_dn(f));
    return or3(v, p, q);
  } else {
    const W u1 = or3(p, f, q);
    if constexpr (KIND == k3x3) {
      return or3(u1, rot_up(u1), rot_dn(u1));
    } else {
      const W pp = col_prev(p), qq = col_next(q);
      const W t = or3(u1, pp, qq);
      const W v = or3(t, rot_up(t), rot_dn(t));
      return or3(v, rot_up_by<2>(u1), rot_dn_by<2>(u1));
    }
  }
}

// res[k] = state[k].ComponentContaining(seed[k], corona) (LifeAPI.hpp:655-665);
// pat: the corona's column j in lane j (kGeneral only).  Wave-uniform control
// flow throughout: every lane of the wave is active at the DPP moves.
template <int KIND, int U>
__device__ __forceinline__ void flood(W (&res)[U], const W (&state)[U], const W (&seed)[U], W pat, int lane) {
  W front[U];
#pragma unroll
  for (int k = 0; k < U; ++k) {
    res[k] = W{0u, 0u};
    front[k] = seed[k];
  }
  for (uint32_t round = 0; round < kMaxRounds; ++round) {
    W nb[U];
    if constexpr (KIND == kGeneral) {
#pragma unroll
      for (int k = 0; k < U; ++k) nb[k] = W{0u, 0u};
      dilate<U>(nb, front, pat, lane);
    } else {
#pragma unroll
      for (int k = 0; k < U; ++k) nb[k] = dilate_fixed<KIND>(front[k]);
    }
    uint32_t grew = 0;
#pragma unroll
    for (int k = 0; k < U; ++k) {
      nb[k] = W{nb[k].lo & state[k].lo, nb[k].hi & state[k].hi};
      front[k] = W{nb[k].lo & ~res[k].lo, nb[k].hi & ~res[k].hi};
      res[k] = W{res[k].lo | nb[k].lo, res[k].hi | nb[k].hi};
      grew |= front[k].lo | front[k].hi;
    }
    if (__ballot(grew != 0u) == 0ull) break;
  }
}

// FirstOn (LifeAPI.hpp:301-323) of the wave's universe, wave-uniform: the
// LAST populated group of four columns, in it the lowest populated column, in
// that column the lowest set row; false for the empty state
__device__ __forceinline__ bool first_on(W s, uint32_t &x, uint32_t &y) {
  const uint64_t cols = __ballot((s.lo | s.hi) != 0u);
  if (cols == 0) return false;
  const uint32_t quad = (63u - (uint32_t)__builtin_clzll(cols)) & ~3u;
  x = quad + (uint32_t)__builtin_ctzll((cols >> quad) & 0xFull);
  y = (uint32_t)__builtin_ctzll(readlane64(s, x));
  return true;
}

// cells[2u], cells[2u + 1] = states[u].FirstOn(), (-1, -1) for the empty
// state: U universes per wave, whose 2U numbers lanes 0 .. 2U-1 store with
// one vector store
template <int U>
__global__ __launch_bounds__(kBlock) void k_first_on(const uint64_t *__restrict__ in, int32_t *__restrict__ cells,
                                                     uint64_t n) {
  const int lane = wave_lane(), wib = wave_in_block();
  const WaveGroups at = wave_groups<U>(wib, n);
  for (uint64_t g = at.first; g < at.groups; g += at.stride) {
    const uint64_t u0 = g * U;
    W s[U];
    // (spelled out: through load_object this kernel's listing changes)
#pragma unroll
    for (int k = 0; k < U; ++k) s[k] = u0 + k < n ? ld<true>(in + (u0 + k) * kWave + lane) : W{0u, 0u};
    int h = 0;
#pragma unroll
    for (int k = 0; k < U; ++k) {
      uint32_t x = 0, y = 0;
      const bool on = first_on(s[k], x, y);
      h = lane == 2 * k ? (on ? (int)x : -1) : lane == 2 * k + 1 ? (on ? (int)y : -1) : h;
    }
    if (holds_scalar<U, 2>(u0, n, lane)) cells[u0 * 2 + lane] = h;
  }
}

// out[u] = states[u].ComponentContaining(seed, corona), seed = seeds[u]
// (per_universe) or seeds[0].  out == states, and out == seeds when
// per-universe, are allowed: a wave loads its universes and seeds whole before
// it stores, and touches no other's.
template <int KIND, int U>
__global__ __launch_bounds__(kBlock) void k_component_containing(const uint64_t *states, const uint64_t *seeds,
                                                                 uint32_t per_universe, Corona corona, uint64_t *out,
                                                                 uint64_t n) {
  const int lane = wave_lane(), wib = wave_in_block();
  W pat{0u, 0u}, one{0u, 0u};
  if constexpr (KIND == kGeneral) pat = split(corona.w[lane]);
  if (!per_universe) one = split(seeds[lane]);
  const WaveGroups at = wave_groups<U>(wib, n);
  for (uint64_t g = at.first; g < at.groups; g += at.stride) {
    const uint64_t u0 = g * U;
    W s[U], seed[U], res[U];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const bool live = u0 + k < n;  // (one guard for both loads: through load_object the listing changes)
      s[k] = live ? ld<true>(states + (u0 + k) * kWave + lane) : W{0u, 0u};
      seed[k] = !live ? W{0u, 0u} : per_universe ? ld<true>(seeds + (u0 + k) * kWave + lane) : one;
    }
    flood<KIND, U>(res, s, seed, pat, lane);
#pragma unroll
    for (int k = 0; k < U; ++k) store_object(out, u0 + k, n, lane, res[k]);
  }
}

// Components(corona) (LifeAPI.hpp:667-676) of states[u], one wave each:
// count[u] = the number of components (count may be null); component
// i < min(count, max_components) at components[(u * max_components + i) * 64]
// (components may be null), in the reference's order; later slots untouched.
template <int KIND>
__global__ __launch_bounds__(kBlock) void k_components(const uint64_t *__restrict__ states, Corona corona,
                                                       uint32_t *__restrict__ count, uint64_t *__restrict__ components,
                                                       uint32_t max_components, uint64_t n) {
  const int lane = wave_lane(), wib = wave_in_block();
  W pat{0u, 0u};
  if constexpr (KIND == kGeneral) pat = split(corona.w[lane]);
  const WaveGroups at = wave_groups<1>(wib, n);
  for (uint64_t u = at.first; u < at.groups; u += at.stride) {
    W rem[1] = {ld<true>(states + u * kWave + lane)};
    uint32_t found = 0;
    for (; found < kMaxComponents; ++found) {
      uint32_t x = 0, y = 0;
      if (!first_on(rem[0], x, y)) break;
      const uint32_t bit = (uint32_t)lane == x ? 1u << (y & 31u) : 0u;
      const W seed[1] = {y < 32u ? W{bit, 0u} : W{0u, bit}};
      W comp[1];
      flood<KIND, 1>(comp, rem, seed, pat, lane);
      if (components && found < max_components)
        st<true>(components + (u * max_components + found) * kWave + lane, comp[0]);
      rem[0] = W{rem[0].lo & ~comp[0].lo, rem[0].hi & ~comp[0].hi};
    }
    if (count && lane == 0) count[u] = found;
  }
}

}  // namespace
}  // namespace lifeapi_impl
