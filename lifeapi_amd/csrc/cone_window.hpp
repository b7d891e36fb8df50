// cone_window.hpp -- the window tests of the light-cone kernels: which
// columns (cone_window, cone_whole, cone_fits) and rows (cone_rows) of a
// universe generation `gens` of a target's care cells can depend on, and the
// two generation thresholds that route a target between the passes
// (cone_passes.hpp, cone_split.hpp).  Every wave of k_cone / k_cone_adapt
// (cone_kernels.hpp) and of k_step_contains_split (contains_kernels.hpp) asks
// them; tests/test_cone_model.py restates them on the CPU.
#pragma once

#include "device.hpp"

namespace lifeapi_impl {
// internal linkage: every library that includes this header gets its own
// kernels (the product and the tuning build never share instantiations)
namespace {

// (rotr64, care_window: device.hpp)
// The column window of a target's care cells, widened by the light cone of
// `gens` generations: xs = first column, K = columns (64: the whole board
// from column 0; also for gens >= 32, whatever the window).  The light-cone
// kernels (cone_kernels.hpp) load exactly these columns.
// care_col: this lane's column of care cells (wanted | unwanted).
__device__ __forceinline__ void cone_window(uint64_t care_col, uint32_t gens, uint32_t &xs, uint32_t &K) {
  const uint64_t cols = __ballot(care_col != 0ull);  // bit x: column x has care cells
  uint32_t x0, w;
  care_window(cols, x0, w);
  K = gens >= (uint32_t)kWave / 2 ? (uint32_t)kWave : w + 2 * gens;
  xs = (x0 - gens) & (kWave - 1);
  if (K >= (uint32_t)kWave) K = kWave, xs = 0;
}
// Whether the cyclic mask e holds a run of at least L (1 .. 64) set bits:
// runs of 2^k by doubling, then the binary digits of L (about 40 scalar
// instructions, no data-dependent selects).
__device__ __forceinline__ bool has_run(uint64_t e, uint32_t L) {
  if (L >= 64u) return e == ~0ull;
  uint64_t run[6];
  run[0] = e;
#pragma unroll
  for (int k = 1; k < 6; ++k) run[k] = run[k - 1] & rotr64(run[k - 1], 1u << (k - 1));
  uint64_t cur = ~0ull;
  uint32_t len = 0;
#pragma unroll
  for (int k = 5; k >= 0; --k)
    if ((L >> k) & 1u) cur &= rotr64(run[k], len), len += 1u << k;
  return cur != 0ull;
}
// Whether cone_window's K is 64 (the whole board from column 0): the care
// columns leave no cyclic run of 2 gens + 1 empty columns, or gens >= 32.
// The light-cone kernels ask this before the full window search, which a
// whole-board target then skips.
__device__ __forceinline__ bool cone_whole(uint64_t care_col, uint32_t gens) {
  return gens >= (uint32_t)kWave / 2 || !has_run(~__ballot(care_col != 0ull), 2u * gens + 1u);
}
// Whether cone_window's K is at most kmax, for 2 gens < kmax <= 64: the care
// columns then leave a cyclic run of at least L = 64 - kmax + 2 gens > 32
// empty columns -- tested directly (runs of 32 by doubling, then one shifted
// AND for the rest, about 25 scalar instructions against care_window's ~100;
// the split kernels' waves ask this on every launch of the iterated loop).
__device__ __forceinline__ bool cone_fits(uint64_t care_col, uint32_t gens, uint32_t kmax) {
  uint64_t run = ~__ballot(care_col != 0ull);  // bit p: column p empty
#pragma unroll
  for (int k = 0; k < 5; ++k) run &= rotr64(run, 1u << k);  // bit p: columns p .. p + 2^(k+1) - 1 empty
  return (run & rotr64(run, 64u - kmax + 2u * gens - 32u)) != 0ull;
}
__device__ __forceinline__ void cone_window(const uint64_t *__restrict__ wanted,
                                            const uint64_t *__restrict__ unwanted, uint32_t gens, int lane,
                                            uint32_t &xs, uint32_t &K) {
  cone_window(wanted[lane] | unwanted[lane], gens, xs, K);
}

// The row window of a filter's whole-board pass (cone_passes.hpp
// cone_wave_rows_dma) and of the window split layout (cone_split.hpp): the
// smallest cyclic window of the target's care rows, widened by `gens` rows on
// either side, and the most universes per 32-bit word whose field holds it
// (PK = 4, 2, 1: fields of 8, 16, 32 rows); 0 when it needs more than 32 rows.
__device__ __forceinline__ int cone_rows(uint64_t care_col, uint32_t gens, uint32_t &y0) {
  const uint32_t lo = wave_or_u32_dpp((uint32_t)care_col), hi = wave_or_u32_dpp((uint32_t)(care_col >> 32));
  uint32_t cy0, h;
  care_window((uint64_t)lo | (uint64_t)hi << 32, cy0, h);
  if (gens >= 16u) return 0;
  const uint32_t need = h + 2u * gens;
  y0 = (cy0 - gens) & 63u;
  return need <= 8u ? 4 : need <= 16u ? 2 : need <= 32u ? 1 : 0;
}

// A column window (5-32 columns) takes the row window too from this many
// generations on (cone_wave_rows; below it the pass is not VALU-bound).
constexpr uint32_t kConeRowsWindowGens = 3;
// A whole board whose care rows fit a row window takes the LDS-DMA packed
// form (cone_wave_rows_dma) below this many generations, the
// window split layout (cone_split.hpp) from it on (one-row target, 1M
// universes: 3 / 5 generations 0.080 / 0.116 ms against 0.102 / 0.113 for
// the split window; 8 / 13: 0.203 / 0.289 against 0.199 / 0.279;
// profiles/r06/ab/)
constexpr uint32_t kConeWholeWinGens = 8;

}  // namespace
}  // namespace lifeapi_impl
