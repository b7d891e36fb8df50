// cone_launch.hpp -- host only: the launch of k_cone_adapt (cone_kernels.hpp)
// for Contains (reduce.hip), the 1-2 generation search filter (step.hip) and
// the tuning build's A/Bs of its forms (tools/tune/tune_cone.hip).
#pragma once

#include "cone_kernels.hpp"
#include "launch.hpp"

namespace lifeapi_impl {
namespace {

// The shipped shape (round 4's last): k_cone_adapt, register sets 8 at a
// time, at most 16 blocks per CU, for Contains and the 1-2 generation filter.
// Same process, 1M universes, back to back (tools/cone_ab.py,
// profiles/r04/r04x/cone_ab.jsonl), against k_cone with 64 universes per wave
// on a one-shot grid (shipped before): filter 0.0223 / 0.0226 ms on the
// 4-column target, 0.0436 / 0.0471 on 14 columns, 0.0658 / 0.0696 on 30, the
// whole board 0.0884 / 0.0898; Contains 0.0199 / 0.0213, 0.0409 / 0.0411,
// 0.0616 / 0.0626, 0.0790 / 0.0803.  Caps of 4 / 8 / 32 and no cap: slower
// on some target each (32: +7 % on the 4-column filter; none: +40 %).
// k_cone's fixed shapes, before: 64 per wave best for P <= 8 (0.0270 against
// 0.0288 ms with 32 per wave, each launch after a scrub,
// profiles/r04/r04g/cone_grid_ab.jsonl), 16 per wave best for 14-30 columns.
constexpr int kConeSets = 8;
constexpr int kConeAdaptBlocksPerCU = 16;
// (Round 5 routed the filter without final states by the generation count,
// the batch size and the last launch report: k_cone_adapt alone up to 4
// generations (6 for batches of at most 256K), the row-window passes up to
// 15, the split pair beyond; its constants and measurements are in the git
// history and DESIGN.md 3.2.)

// Launches k_cone_adapt on ceil(n / 16) waves, at most blocks_per_cu blocks
// per CU (0: no cap), on a device of `cus` CUs (0: not asked yet).  DMA: a
// whole-board window takes cone_wave_full_dma when the batch is 16-byte
// aligned, on a grid of at most dma_blocks_per_cu blocks per CU (0: uncapped;
// blocks_per_cu then caps the waves of a windowed target).  Contains (!FIRST)
// over a 16-byte aligned batch takes the A16 form.  Neither output is a batch
// of universes.
template <int RMAX, bool FIRST, typename OutT, bool DMA = false, bool ROWS = true, bool WIN = false, bool EARLY = true>
int launch_cone_adapt(const uint64_t *d_in, const uint64_t *d_wanted, const uint64_t *d_unwanted, OutT *d_out,
                      size_t n, uint32_t gens, int cus, hipStream_t stream, int blocks_per_cu,
                      uint32_t kmax = kWave, int dma_blocks_per_cu = 0) {
  void (*fn)(const uint64_t *, const uint64_t *, const uint64_t *, OutT *, uint64_t, uint32_t, uint32_t, uint32_t) =
      k_cone_adapt<RMAX, FIRST, OutT, false, false, ROWS, WIN>;
  int cap = blocks_per_cu;
  uint32_t cap_waves = 0;
  if constexpr (!FIRST) {
    if (aligned16(d_in)) fn = k_cone_adapt<RMAX, FIRST, OutT, true, false, ROWS, WIN>;
  }
  if constexpr (DMA) {
    if (aligned16(d_in)) {
      if (int rc = cus ? LIFEAPI_OK : device_cus(cus); rc != LIFEAPI_OK) return rc;  // (for cap_waves)
      fn = k_cone_adapt<RMAX, FIRST, OutT, true, true, ROWS, WIN, EARLY>;
      cap = dma_blocks_per_cu;
      cap_waves = blocks_per_cu > 0 ? (uint32_t)(cus * blocks_per_cu * kWavesPerBlock) : 0u;
    }
  }
  return launch(fn, "k_cone_adapt launch", Grid{(n + 15) / 16, cap, 0, cus}, stream, kWritesNoBatch, d_in, d_wanted,
                d_unwanted, d_out, n, gens, kmax, cap_waves);
}

}  // namespace
}  // namespace lifeapi_impl
