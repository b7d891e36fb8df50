// step.hip -- batched LifeState::Step() (LifeAPI.hpp:1196-1216, Stepped(n)
// :877-886) and the fused Step + Contains (LifeTarget.hpp:44-51): the
// shipped kernel configurations and their C ABI (include/lifeapi_hip.h).
// The kernels are in step_kernels.hpp (Step), contains_kernels.hpp (Step +
// Contains) and cone_kernels.hpp (the light-cone filter); the measured alternatives (other
// networks, exchanges, layouts and schedules) live in the tuning build,
// tools/tune/tune_step.hip, and are not part of this library.
#include <algorithm>

#include "cone_launch.hpp"
#include "contains_kernels.hpp"
#include "launch.hpp"
#include "step_kernels.hpp"

using namespace lifeapi_impl;

namespace {

using StepFn = void (*)(const uint64_t *, uint64_t *, uint64_t, uint32_t, uint64_t);

// The shipped configurations (profiles/r01/tune_*.jsonl):
// * gens <= 2 -- HBM-streaming: natural layout, DPP exchange, the 7-LUT
//   network, 4 universes in flight per wave, nontemporal loads (no layout
//   change to pay for);
// * gens > 2 -- VALU-bound: 8-way row split with 4 universes interleaved bit
//   by bit, LDS exchange, the 6-LUT tail, state resident in VGPRs for all
//   generations, as the hand-allocated loop of split_asm.inc; nontemporal
//   below 32 generations.  One-shot grids: every capped grid-stride grid
//   measured slower.
//
// The streaming step, round 7 (tools/step_store_ab.py, same process, both
// bodies interleaved round by round, 20 launches per event pair;
// profiles/r07/step_store_ab/*.jsonl, profiles/r07/README.md).  A wave of
// k_step now issues its 4 stores back to back and ends behind them
// (step_kernels.hpp step_group); round 6's body waited for each store before
// the next.  Under round 6's launch policy the new body is 3.1 % faster at 1M
// universes (0.1475 against 0.1522 ms, 4.7 x the old body's round-to-round
// spread, rounds disjoint), 2.5 % at 512K, equal at 4M and 16M, and slower at
// 2M and 8M (+3.2 %, +0.9 %): a wave that no longer holds its slot through its
// stores wants fewer waves resident.  The sweep on the new body (universes per
// wave {4, 8} x resident blocks per CU {all 8, 7, 6} x plain tail x order, or
// x XCD chunks above 4M) moved these, each by more than 3 x the spread:
// * resident blocks per CU (unused dynamic LDS, launch.hpp Grid): 7
//   at 1M universes (0.1461 against 0.1475 ms uncapped), 6 from 2M on (2M
//   0.3131 against 0.3216 uncapped and 0.3167 with 7; 4M 0.6571 against
//   0.6810 / 0.6722; 8M 1.296 against 1.318 / 1.303; 16M 2.664 against 3.011
//   / 2.846).  At 512K 7 blocks gained 1.1 %, 1.4 x the spread: not enough,
//   so batches below 1M stay uncapped; between two measured sizes the cap is
//   the smaller one's.  Round 6 ran uncapped up to 4M and 7 above.
// * 4 universes per wave above 4M too (round 4 chose 8 there for 8M): 8M 1.296
//   against 1.342 ms, 16M 2.664 against 2.702, both at 6 blocks.
// Unchanged, because nothing beat them: the alternating order with the last
// min(256 MiB, half the batch) stored plain up to 4M (every other tail or a
// fixed order 7-15 % slower at 1M), and XCD chunks above (16M: the plain block
// mapping is 0.7 % faster at 6 blocks, 8M: 2.4 % slower).
// Against round 6's launch, same process: 512K -2.5 %, 1M -4.0 %, 2M +0.4 %
// (inside the spread), 4M -3.2 %, 8M -3.2 %, 16M -1.8 %.
//
// Launch order and store policy (tools/ab/order_ab.py, profiles/r02/order_*.jsonl,
// same process, ping-pong as the bench): a launch whose input batch an
// earlier launch wrote takes the groups in the reverse of that launch's order
// (launch.hpp launch_order, keyed on the batch), so it starts on what was
// written last; the groups that store the last min(256 MiB, half
// the batch) of a launch use plain stores, which leave that part in the 256 MB
// memory-side Infinity Cache, and the rest nontemporal ones, which do not
// evict it.  ("Last" is by dispatch position: under XCD chunks the end of
// every XCD's eighth, round 17 below.)
//
// Round 17: the two together (tools/step_chunk_ab.py, round 7's method and
// rule; profiles/r17/step_chunk_ab/*.jsonl, profiles/r17/README.md).  The
// plain-stored tail is now decided by dispatch position (step_order.hpp
// step_take), so with kXcdChunk it is the end of every XCD's eighth, which is
// what a chunked launch writes last, and the reversed launch that follows
// starts on those ends.  Chunks x order x tail x resident blocks x universes
// per wave at every size, against the launch shipped until then (ms, median of
// 7 rounds; gain over that launch's p10-p90 spread in brackets):
// * 512K: chunks, alternating, half the batch plain, 7 blocks: 0.0740 against
//   0.0756 (8.9 x); without chunks 7 blocks gain 0.9 % (4.0 x);
// * 1M: chunks, alternating, 256 MiB, 7 blocks: 0.1437 against 0.1459 (10.8 x);
// * 2M: nothing passed; the best chunked launch (alternating, 256 MiB, 6
//   blocks) is 2.0 % slower, so 2M up to 4M keeps the plain block mapping;
// * 4M: chunks, alternating, 256 MiB, 6 blocks: 0.6403 against 0.6575 (8.6 x),
//   on a second box 0.6363 against 0.6576 (9.2 x); a third ran the former
//   launch at 0.6359 and this one at 0.6410, inside the former's own range;
// * 8M: the same: 1.2934 against 1.3181 (10.6 x); * 16M: 2.6125 against 2.6341
//   (8.7 x).  Above 4M a fixed order with the tail gains a third of that, the
//   alternating order without a tail nothing: it is the reuse.
// 4 universes per wave everywhere; between two measured sizes the smaller
// one's setting.
constexpr uint64_t kChunkMinUniverses = 1ull << 19;   // XCD chunks from here ...
constexpr uint64_t kChunkStopUniverses = 1ull << 21;  // ... up to here (excluded),
constexpr uint64_t kChunkBigUniverses = 1ull << 22;   // and from here on
bool stream_chunks(uint64_t n) {
  return (n >= kChunkMinUniverses && n < kChunkStopUniverses) || n >= kChunkBigUniverses;
}
// resident blocks per CU of the streaming step (0 = as many as fit, 8)
constexpr uint64_t kCap7Universes = 1ull << 19;  // 7 from here (round 17; 1M before)
constexpr uint64_t kCap6Universes = 1ull << 21;  // 6 from here
constexpr int kStreamResidentBlocks = 6;
int stream_resident_blocks(uint64_t n) {
  return n < kCap7Universes ? 0 : n < kCap6Universes ? 7 : kStreamResidentBlocks;
}
// Below this batch size the order stays fixed: at 64K universes (64 MiB per
// launch) the fixed order was 4 % faster, single batch and two interleaved,
// and at 128K the two boxes disagreed (-4 / +1 %); from 192K on the
// batch-keyed order is as fast or faster (+1-3 % at 192K-384K, +7-8 % for two
// interleaved 512K batches, +16 % for one 1M batch; tools/ab/order_interleave_ab.py,
// profiles/r03/order_interleave*.jsonl)
constexpr uint64_t kOrderMinUniverses = 3ull << 16;
constexpr uint64_t kPlainBytes = 256ull << 20;
constexpr uint64_t kFilterOrderUniverses = 1ull << 21;  // the same for the 1-2 generation search filter
// Two names: the launches up to kChunkBigUniverses (with it: some chunked, some
// not) and the ones above, all chunked (kXcdChunk, device.hpp xcd_chunk_block).
constexpr const char *kStreamName =
    "k_step<dpp, 4 universes/wave, nt loads, 7-LUT network; alternating order, the last min(256 MiB, half) of "
    "each launch stored plain, the rest nt; each XCD a contiguous eighth from 512K up to 2M and from 4M universes>";
constexpr const char *kStreamBigName =
    "k_step<dpp, 4 universes/wave, nt loads, 7-LUT network; each XCD a contiguous eighth, the order reversed from "
    "launch to launch, the last 32 MiB of every eighth stored plain, the rest nt>";
struct StepLaunch {
  StepFn fn;
  uint64_t universes_per_wave;
  int resident_blocks;   // per CU, 0 = as many as fit
  bool alternate;        // alternate the group order between launches
  uint64_t plain_bytes;  // the last bytes of a launch stored plain
  const char *name;
  uint32_t flags;        // kXcdChunk or 0
};
StepLaunch shipped_step(uint32_t gens, uint64_t n) {
  if (gens <= 2)
    return {k_step<XDPP, 4, true, 3, true, true>, 4, stream_resident_blocks(n), true,
            std::min<uint64_t>(kPlainBytes, n * 512 / 2), n > kChunkBigUniverses ? kStreamBigName : kStreamName,
            stream_chunks(n) ? kXcdChunk : 0u};
  if (gens < 32)
    return {k_step_split<8, 1, true, 6, kAsmLoop>, 4, 0, false, 0,
            "k_step_split<8-way split, 4 universes/wave, nt, 6-LUT tail, assembly loop>", 0u};
  return {k_step_split<8, 1, false, 6, kAsmLoop>, 4, 0, false, 0,
          "k_step_split<8-way split, 4 universes/wave, 6-LUT tail, assembly loop>", 0u};
}

// ---- lifeapi_step_contains_batch_dev: its four forms ----

// The merged split kernel (below, 3+ generations without final states) on a
// grid of at most this many blocks per CU looping over the batch (round 6; 1M
// universes: 16 and 32 within 1-3 % of each other on every target, 8 up to
// 9 % slower on the one-row whole board; profiles/r06/ab/)
constexpr int kFilterIterBlocksPerCU = 16;
// The split pair (below, final states at 3+ generations) runs on grids of at
// most 32 blocks per CU looping over the batch: one of the two always idles,
// and the working one is faster capped from 256K universes on.
constexpr int kSplitIterBlocksPerCU = 32;

using SplitFn = void (*)(const uint64_t *, uint64_t *, const uint64_t *, const uint64_t *, uint32_t *, uint64_t,
                         uint32_t, uint32_t);

// First hits only at 1-2 generations, the search filter proper: the
// target's light cone, or the whole board, in the natural layout
// (cone_kernels.hpp k_cone_adapt, DMA form): a whole-board target takes
// the universes through LDS (cone_passes.hpp cone_wave_full_dma / cone_wave_rows_dma, 8
// per pass by global_load_lds, the next pass fetched while this one
// steps), every other window its cone (cone_wave); every wave decides,
// on a grid of at most kConeAdaptBlocksPerCU blocks per CU looping over
// the batch.  Round 6: no launch report -- round 5 chose the grid per
// target pointers from the last call's report, which a loop that rewrites
// its target buffers read stale (+13 % per call, tools/report_loop_probe.py,
// profiles/r06/).  1M universes, median of 5 x 10 back to back
// (tools/filter_iter_probe.py, profiles/r06/): the one-row whole board
// 0.083 / 0.086 ms at 1 / 2 generations against 0.082 / 0.081 on the
// reported uncapped grid, the full-height and random whole boards 5-9 %
// faster, the block + ring unchanged (0.023 / 0.026).
int filter_cone(const uint64_t *d_in, const uint64_t *d_wanted, const uint64_t *d_unwanted, uint32_t *d_first_gen,
                size_t n, uint32_t generations, void *stream) {
  return launch_cone_adapt<kConeSets, true, uint32_t, true>(d_in, d_wanted, d_unwanted, d_first_gen, n, generations, 0,
                                                            (hipStream_t)stream, kConeAdaptBlocksPerCU, kWave,
                                                            kConeAdaptBlocksPerCU);
}

// First hits only at 3+ generations (round 6): one launch of the merged
// split kernel (contains_kernels.hpp k_step_contains_split, kContainsAll),
// whose waves take the pass their target calls for -- no report, so a
// loop that rewrites its target buffers loses nothing:
// * care rows that fit 32 with the light cone (cone_rows): on a whole
//   board below kConeWholeWinGens generations the packed LDS-DMA pass
//   (cone_wave_rows_dma), else the window split layout (cone_split.hpp)
//   on the column window, on half the lanes once the cone's columns fit
//   (a whole board's chunks fetched by LDS-DMA);
// * else a cone of <= 32 columns: the natural layout on the cone
//   (cone_wave);
// * else the 8-way row split with the test fused (the loop its row
//   window picks), the next group of universes fetched into LDS while
//   this one steps.
// 1M universes, median of 5 x 10 back to back (tools/filter_iter_probe.py,
// profiles/r06/): block + ring at 3 / 5 / 8 / 13 generations 0.042 / 0.058
// / 0.096 / 0.137 ms (round 5: 0.047 / 0.057 / 0.154 / 0.222;
// profiles/r06/shrink_ab/), a full-height target 0.179 / 0.235 / 0.309 /
// 0.435 (0.18 / 0.24 / 0.32 / 0.47 on the split pair).
int filter_iterated(const uint64_t *d_in, const uint64_t *d_wanted, const uint64_t *d_unwanted,
                    uint32_t *d_first_gen, size_t n, uint32_t generations, void *stream) {
  const SplitFn fn = aligned16(d_in) ? k_step_contains_split<8, kContainsNet, kContainsAll, true, true>
                                     : k_step_contains_split<8, kContainsNet, kContainsAll, false, true>;
  return launch(fn, "k_step_contains_split launch", Grid{(n + 3) / 4, kFilterIterBlocksPerCU}, stream,
                kWritesNoBatch, d_in, nullptr, d_wanted, d_unwanted, d_first_gen, n, generations, kConeIterColumns);
}

// Final states at 3+ generations, in the layout of the shipped step for
// gens > 2: two kernels, one per register layout (a target window of <= 4
// rows in 62 VGPRs, 8 waves per SIMD; the rest in 71, 7 waves): each wave
// finds the window and only the matching kernel works (contains_kernels.hpp
// kContainsLo / kContainsHi); every universe steps the whole board (no light
// cone: the kernels' last argument is 0).  Both grids are capped (blocks per
// CU, looping over the batch), so that the idle kernel's waves cost a few
// microseconds instead of a wave launch per 4 universes
// (tools/ab/search_iter_caps_ab.py): 1M universes x 8 / 64
// generations 0.467 -> 0.394-0.398 / 1.78-1.80 -> 1.70 ms, 256K 0.112 ->
// 0.101 ms; at config 3's 64K the cap does not bind (tools/ab/final_caps_ab.py,
// profiles/r04/r04ar).
int final_split_pair(const uint64_t *d_in, uint64_t *d_final, const uint64_t *d_wanted, const uint64_t *d_unwanted,
                     uint32_t *d_first_gen, size_t n, uint32_t generations, void *stream) {
  int cus = 0, rc = device_cus(cus);  // (once for both launches)
  Written w{d_final, (uint64_t)n * 512};  // (recorded once for the pair)
  for (const SplitFn fn : {SplitFn(k_step_contains_split<8, kContainsNet, kContainsLo>),
                           SplitFn(k_step_contains_split<8, kContainsNet, kContainsHi>)}) {
    if (rc != LIFEAPI_OK) return rc;
    rc = launch(fn, "k_step_contains_split launch", Grid{(n + 3) / 4, kSplitIterBlocksPerCU, 0, cus}, stream, w, d_in,
                d_final, d_wanted, d_unwanted, d_first_gen, n, generations, 0u);
    w.recorded = true;
  }
  return rc;
}

// Final states at 1-2 generations: k_step_contains<8>, 8 universes per wave,
// every block slot (tools/ab/filter_ab.py, profiles/r02/filter_ab.jsonl, 1M
// universes x 1 generation, same process): 0.181 ms with final states
// (5.96 TB/s on 1028 B per universe); 4 per wave 0.179, with fewer blocks
// resident slower; one per wave 0.229.
// The launch order and plain-stored tail of the step (above): a loop that
// filters the states the last call left gets them partly from the Infinity
// Cache (tools/ab/filter_order_ab.py).  Up to 2M universes: +3.4 % at 512K
// and 1M, +2 % at 2M, none at 4M (profiles/r02/filter_order_ab.jsonl).
int final_stream(const uint64_t *d_in, uint64_t *d_final, const uint64_t *d_wanted, const uint64_t *d_unwanted,
                 uint32_t *d_first_gen, size_t n, uint32_t generations, void *stream) {
  const uint64_t groups = (n + 7) / 8;
  const bool keyed = n <= kFilterOrderUniverses && n >= kOrderMinUniverses;
  const LaunchOrder o = launch_order(d_in, d_final, (uint64_t)n * 512, groups, 8 * 512, keyed,
                                     keyed ? std::min<uint64_t>(kPlainBytes, n * 512 / 2) : 0);
  return launch(k_step_contains<8>, "k_step_contains launch", Grid{groups}, stream, o.written, d_in, d_final,
                d_wanted, d_unwanted, d_first_gen, n, generations | (o.reverse ? kReverse : 0u), o.plain_from);
}

}  // namespace

extern "C" {

const char *lifeapi_step_kernel_name_n(uint32_t generations, size_t n) {
  return shipped_step(generations, n).name;
}
const char *lifeapi_step_kernel_name(uint32_t generations) { return shipped_step(generations, 1).name; }

int lifeapi_step_batch_dev(const uint64_t *d_in, uint64_t *d_out, size_t n, uint32_t generations,
                           void *stream) {
  int rc = check_batch(d_in, d_out, n);
  if (rc != LIFEAPI_OK || n == 0) return rc;
  const StepLaunch l = shipped_step(generations, n);
  const uint64_t waves = (n + l.universes_per_wave - 1) / l.universes_per_wave;
  const LaunchOrder o = launch_order(d_in, d_out, (uint64_t)n * 512, waves, l.universes_per_wave * 512,
                                     l.alternate && n >= kOrderMinUniverses, l.plain_bytes);
  // one-shot, and k_step's waves take one group each (step_body ONESHOT)
  return launch(l.fn, "k_step launch", Grid{waves, 0, l.resident_blocks, 0, true}, stream, o.written, d_in, d_out, n,
                generations | (o.reverse ? kReverse : 0u) | l.flags, o.plain_from);
}

int lifeapi_step_contains_batch_dev(const uint64_t *d_in, uint64_t *d_final,
                                    const uint64_t *d_wanted, const uint64_t *d_unwanted,
                                    uint32_t *d_first_gen, size_t n, uint32_t generations,
                                    void *stream) {
  if (n == 0) return LIFEAPI_OK;
  if (!d_in || !d_wanted || !d_unwanted || !d_first_gen || !aligned8(d_in) ||
      !aligned8(d_wanted) || !aligned8(d_unwanted) || ((uintptr_t)d_first_gen & 3u))
    return fail(LIFEAPI_E_INVALID, "bad pointer to lifeapi_step_contains_batch_dev%s");
  if (!d_final) {
    if (generations <= 2) return filter_cone(d_in, d_wanted, d_unwanted, d_first_gen, n, generations, stream);
    return filter_iterated(d_in, d_wanted, d_unwanted, d_first_gen, n, generations, stream);
  }
  const int rc = check_batch(d_in, d_final, n);
  if (rc != LIFEAPI_OK) return rc;
  if (generations > 2)
    return final_split_pair(d_in, d_final, d_wanted, d_unwanted, d_first_gen, n, generations, stream);
  return final_stream(d_in, d_final, d_wanted, d_unwanted, d_first_gen, n, generations, stream);
}

}  // extern "C"
