// cone_kernels.hpp -- Contains(LifeTarget) (LifeTarget.hpp:44-51) and the
// 1-2 generation search filter (Step(), LifeAPI.hpp:1196-1216, then
// Contains) reading only the target's light cone.
//
// Whether generation g of a universe contains a target depends only on the
// input columns within distance g of the target's care columns (wanted |
// unwanted): a cell's next state reads its 3x3 neighbourhood.  Every wave
// finds the smallest cyclic window [x0, x0 + w) of columns holding the care
// cells (care_window, the same search as the row window of the iterated
// kernel) and loads only columns [x0 - g, x0 + w + g) mod 64 -- K = w + 2g
// columns, K * 8 bytes of each 512-byte universe, so that the 128-byte lines
// outside never leave HBM.
//
// Lane layout: P = the next power of two >= K lanes per universe, 64 / P
// universes per wave register ("set"); lane j of group q holds column
// (x0 - g + j) mod 64 of its universe.  The generation is the streaming
// step's network (life_gen<XDPP, 3>) unchanged: its 64-lane DPP rotate hands
// a group's edge lanes their neighbour group's columns, which is wrong data
// -- but only for the g margin columns on either side, which the test never
// reads (after g generations the error has moved g columns in).  The care
// columns are exact.  A window with K >= 64 loads the whole board from
// column 0, where the rotate is the true torus.
//
// The window tests (cone_window, cone_whole, cone_fits, cone_rows) are in
// cone_window.hpp, the passes over a wave's universes (cone_wave and the
// rest) in cone_passes.hpp, the window split layout in cone_split.hpp; all
// are shared with the iterated search loop's k_step_contains_split
// (contains_kernels.hpp).  This file holds the kernels that run them:
// k_cone_adapt (shipped: the chunk of universes per wave chosen from the
// window) and k_cone (fixed shapes, the tuning build's A/Bs).  Their
// launchers are host code: cone_launch.hpp (k_cone_adapt, with the shipped
// shape's measurements) and tools/tune/tune_cone.hip (k_cone).
#pragma once

#include <type_traits>

#include "cone_passes.hpp"
#include "cone_split.hpp"

namespace lifeapi_impl {
// internal linkage: every library that includes this header gets its own
// kernels (the product and the tuning build never share instantiations)
namespace {

// UPW universes per wave (one-shot grid of ceil(n / UPW) waves), every wave
// choosing its lane layout from the window (wave-uniform: the target is the
// same for all).  Each choice runs its own copy of the pass.  A16: the batch
// is 16-byte aligned (Contains over the whole board then takes 16-byte loads).
// kmax: a wave whose window K exceeds it returns at once (the iterated
// search loop's split-layout kernels answer those, step.hip).
template <int UPW, int RMAX, bool FIRST, typename OutT, bool A16 = false, bool PIPE = false>
__global__ __launch_bounds__(kBlock) void k_cone(const uint64_t *in, const uint64_t *__restrict__ wanted,
                                                 const uint64_t *__restrict__ unwanted, OutT *__restrict__ out,
                                                 uint64_t n, uint32_t gens, uint32_t kmax) {
  const int lane = threadIdx.x & (kWave - 1);
  const uint64_t wave = (uint64_t)blockIdx.x * kWavesPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const uint64_t u0 = wave * UPW, step = (uint64_t)gridDim.x * kWavesPerBlock * UPW;  // grid-stride (capped grids)
  if (u0 >= n) return;
  const uint32_t g = FIRST ? gens : 0u;
  const uint64_t care_col = wanted[lane] | unwanted[lane];
  uint32_t xs = 0, K = kWave;
  if (!cone_whole(care_col, g)) cone_window(care_col, g, xs, K);  // (a whole-board target skips the search)
  if (K > kmax) return;
  if constexpr (!FIRST && A16) {
    if (K == (uint32_t)kWave) return cone_wave_full16<UPW, RMAX>(in, wanted, unwanted, out, n, u0, step, lane);
  }
  // (a wave of UPW universes takes whole register sets: P >= 64 / UPW)
  auto pass = [&](auto p) __attribute__((always_inline)) {
    cone_wave<decltype(p)::value, UPW, RMAX, FIRST, OutT, PIPE>(in, wanted, unwanted, out, n, u0, step, gens, xs, K,
                                                                lane);
  };
  if (K <= 4 && UPW >= 16) pass(std::integral_constant<int, (UPW >= 16 ? 4 : 8)>{});
  else if (K <= 8) pass(std::integral_constant<int, 8>{});
  else if (K <= 16) pass(std::integral_constant<int, 16>{});
  else if (K <= 32) pass(std::integral_constant<int, 32>{});
  else pass(std::integral_constant<int, 64>{});
}

// k_cone with the chunk size chosen by the window: 64 universes per wave
// chunk while P <= 8 lanes per universe (one pass), 16 for wider cones (one
// pass of 16 / 4 / 1 universes per register set), on a grid of ceil(n / 16)
// waves capped at the caller's blocks per CU, every wave looping over the
// batch with its own chunk size.
// DMA (a 16-byte aligned batch): the whole board (K = 64) through LDS
// (cone_wave_full_dma, RMAX sets per pass, chunks of 2 RMAX universes), on
// the uncapped grid; every other window keeps the capped shape, the first
// cap_waves waves looping over the batch and the rest returning after the
// whole-board test (0: no cap).
// WIN: from kConeRowsWindowGens generations on, a target whose rows fit
// 32 (16) takes the window split layout (cone_split.hpp cone_wave_split) on
// the capped grid instead of the packed row-window passes.
// EARLY (DMA): a whole board's first pass is fetched as soon as the
// whole-board test passes, so the row-window search runs under it.  1M
// universes, back to back, against the tuning build's EARLY = false
// (profiles/r06/ab/early_fetch.jsonl): full-height and random whole boards at
// 2 generations 0.133 / 0.132 ms against 0.138 / 0.139, the one-row target
// and 1 generation within +-3 %, small targets unchanged.
template <int RMAX, bool FIRST, typename OutT, bool A16 = false, bool DMA = false, bool ROWS = true, bool WIN = false,
          bool EARLY = true>
__global__ __launch_bounds__(kBlock) void k_cone_adapt(const uint64_t *in, const uint64_t *__restrict__ wanted,
                                                       const uint64_t *__restrict__ unwanted, OutT *__restrict__ out,
                                                       uint64_t n, uint32_t gens, uint32_t kmax, uint32_t cap_waves) {
  const int lane = threadIdx.x & (kWave - 1);
  const uint64_t wave = (uint64_t)blockIdx.x * kWavesPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  uint64_t nw = (uint64_t)gridDim.x * kWavesPerBlock;
  // (the smallest chunk any path takes: a wave starting past n has no work)
  // (WIN: the window split layout's sets are as small as 8 universes, 64
  // lanes x 32 rows)
  constexpr uint64_t kMinChunk = WIN ? 8 : DMA && 2 * RMAX < 16 ? 2 * RMAX : 16;
  if (wave * kMinChunk >= n) return;
  const uint32_t g = FIRST ? gens : 0u;
  const uint64_t w64 = wanted[lane], m64 = w64 | unwanted[lane], care_col = m64;
  uint32_t xs = 0, K = kWave;
  // the window split layout (WIN, cone_split.hpp)
  auto split_pass = [&](int pk_, uint32_t y0_, uint64_t nw_) __attribute__((always_inline)) {
    cone_split_pass(in, wanted, unwanted, out, n, wave, nw_, gens, xs, K, pk_, y0_, lane);
  };
  if constexpr (DMA) {
    __shared__ uint64_t img_all[kWavesPerBlock][RMAX * kWave];
    uint64_t *img = img_all[__builtin_amdgcn_readfirstlane(threadIdx.x / kWave)];
    const uint64_t c = 2 * RMAX;
    // (round 5 fetched a whole board's first pass before the whole-board test
    // when the last launch on the same target pointers had reported one;
    // round 6 reads no report and fetches it right after that test, DESIGN.md
    // 3.2)
    int pk = 0;
    uint32_t y0 = 0;
    if (cone_whole(care_col, g)) {
      // (not before a pass that loads by itself: the window split layout)
      const bool early = EARLY && kmax >= (uint32_t)kWave && wave * c < n &&
                         !(WIN && FIRST && gens >= kConeWholeWinGens);
      if (early) dma_fetch_pass<RMAX>(in, n, wave * c, lane, img);
      if constexpr (FIRST) pk = cone_rows(care_col, gens, y0);
      if (kmax < (uint32_t)kWave) return;
      if constexpr (FIRST && WIN) {
        if (pk > 0 && gens >= kConeWholeWinGens) {  // (its sets may be 8 universes: before the chunk test)
          if (cap_waves) {
            if (wave >= cap_waves) return;
            nw = nw < cap_waves ? nw : cap_waves;
          }
          return split_pass(pk, y0, nw);
        }
      }
      if (wave * c >= n) return;
      if constexpr (FIRST && ROWS) {
        auto rows = [&](auto pk_c, auto wrap_c) __attribute__((always_inline)) {
          cone_wave_rows_dma<RMAX, decltype(pk_c)::value, decltype(wrap_c)::value>(
              in, w64, m64, out, n, wave * c, nw * c, gens, y0, lane, img, early);
        };
        using T = std::true_type;
        using F = std::false_type;
        using P1 = std::integral_constant<int, 1>;
        using P2 = std::integral_constant<int, 2>;
        using P4 = std::integral_constant<int, 4>;
        if (pk == 4) return y0 >= 32u ? rows(P4{}, T{}) : rows(P4{}, F{});
        if (pk == 2) return y0 >= 32u ? rows(P2{}, T{}) : rows(P2{}, F{});
        if (pk == 1) return y0 >= 32u ? rows(P1{}, T{}) : rows(P1{}, F{});
      }
      return cone_wave_full_dma<RMAX, FIRST>(in, w64, m64, out, n, wave * c, nw * c, gens, lane, img, early);
    }
    if (cap_waves) {
      if (wave >= cap_waves) return;
      nw = nw < cap_waves ? nw : cap_waves;
    }
    cone_window(care_col, g, xs, K);
    if (K > kmax) return;
    if (K == (uint32_t)kWave) {
      if (wave * c >= n) return;
      return cone_wave_full_dma<RMAX, FIRST>(in, w64, m64, out, n, wave * c, nw * c, gens, lane, img, false);
    }
  } else {
    int pk = 0;
    uint32_t y0 = 0;
    if (!cone_whole(care_col, g)) {
      cone_window(care_col, g, xs, K);
      // (the row window of a column window: cone_wave_rows, below)
      if constexpr (FIRST && ROWS) {
        if (gens >= kConeRowsWindowGens) pk = cone_rows(care_col, gens, y0);
      }
    } else if constexpr (FIRST && ROWS) {
      if (gens >= kConeRowsWindowGens) pk = cone_rows(care_col, gens, y0);
    }
    if (K > kmax) return;
    if constexpr (FIRST && ROWS) {
      // a column window of more than 4 columns (the whole board too, in this
      // capped form) whose rows, widened by the cone, fit 32 (16) rows: 1 (2)
      // universes per register and lane, rows cut to the window
      // (cone_wave_rows)
      if constexpr (WIN) {
        if (pk > 0 && K > 4u && gens >= kConeRowsWindowGens) return split_pass(pk, y0, nw);
      }
      if (pk > 0 && K > 4u && gens >= kConeRowsWindowGens) {
        auto rw = [&](auto p_c, auto upw_c, auto pk_c, auto wrap_c) __attribute__((always_inline)) {
          constexpr int UPWc = decltype(upw_c)::value;
          if (wave * UPWc >= n) return;
          cone_wave_rows<decltype(p_c)::value, UPWc, RMAX, decltype(pk_c)::value, decltype(wrap_c)::value>(
              in, wanted, unwanted, out, n, wave * UPWc, nw * UPWc, gens, xs, K, y0, lane);
        };
        using I8 = std::integral_constant<int, 8>;
        using I16 = std::integral_constant<int, 16>;
        using I32 = std::integral_constant<int, 32>;
        using I64 = std::integral_constant<int, 64>;
        using K1 = std::integral_constant<int, 1>;
        using K2 = std::integral_constant<int, 2>;
        using T = std::true_type;
        using F = std::false_type;
        const bool wrap = y0 >= 32u, two = pk >= 2;
        if (K <= 8u) {
          if (two) return wrap ? rw(I8{}, I64{}, K2{}, T{}) : rw(I8{}, I64{}, K2{}, F{});
          return wrap ? rw(I8{}, I64{}, K1{}, T{}) : rw(I8{}, I64{}, K1{}, F{});
        }
        if (K <= 16u) {
          if (two) return wrap ? rw(I16{}, I16{}, K2{}, T{}) : rw(I16{}, I16{}, K2{}, F{});
          return wrap ? rw(I16{}, I16{}, K1{}, T{}) : rw(I16{}, I16{}, K1{}, F{});
        }
        if (K <= 32u) {
          if (two) return wrap ? rw(I32{}, I16{}, K2{}, T{}) : rw(I32{}, I16{}, K2{}, F{});
          return wrap ? rw(I32{}, I16{}, K1{}, T{}) : rw(I32{}, I16{}, K1{}, F{});
        }
        if (two) return wrap ? rw(I64{}, I16{}, K2{}, T{}) : rw(I64{}, I16{}, K2{}, F{});
        return wrap ? rw(I64{}, I16{}, K1{}, T{}) : rw(I64{}, I16{}, K1{}, F{});
      }
    }
  }
  if constexpr (!FIRST && A16 && !DMA) {
    if (K == (uint32_t)kWave) return cone_wave_full16<16, RMAX>(in, wanted, unwanted, out, n, wave * 16, nw * 16, lane);
  }
  if (K <= 8) {
    if (wave * 64 >= n) return;
    if (K <= 4) cone_wave<4, 64, RMAX, FIRST>(in, wanted, unwanted, out, n, wave * 64, nw * 64, gens, xs, K, lane);
    else cone_wave<8, 64, RMAX, FIRST>(in, wanted, unwanted, out, n, wave * 64, nw * 64, gens, xs, K, lane);
  } else if (K <= 16) {
    cone_wave<16, 16, RMAX, FIRST>(in, wanted, unwanted, out, n, wave * 16, nw * 16, gens, xs, K, lane);
  } else if (K <= 32) {
    cone_wave<32, 16, RMAX, FIRST>(in, wanted, unwanted, out, n, wave * 16, nw * 16, gens, xs, K, lane);
  } else {
    cone_wave<64, 16, RMAX, FIRST>(in, wanted, unwanted, out, n, wave * 16, nw * 16, gens, xs, K, lane);
  }
}

// (kConeRowsWindowGens, kConeWholeWinGens: cone_window.hpp)
// The iterated search loop (gens > 2, no final states) steps the light cone
// while it spans at most this many columns (P <= 32 lanes per universe: at
// most half the natural layout's work per universe-generation, against the
// split layout's 18 issue slots plus its layout change) -- inside
// kContainsLo (contains_kernels.hpp, kConeLoUniverses = 8 universes per wave
// chunk: that work is VALU-bound, and 64 per wave would leave 64K universes
// one wave per SIMD).
constexpr uint32_t kConeIterColumns = 32;
static_assert(kConeIterColumns <= 32, "kContainsLo's cone passes take P <= 32");

}  // namespace
}  // namespace lifeapi_impl
