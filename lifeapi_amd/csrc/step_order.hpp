// step_order.hpp -- the index arithmetic of the streaming step's launch order
// (step_kernels.hpp step_body), for the device and the host alike: which
// place a block has in the batch, which group of universes a wave takes
// there, forward or reversed, and whether it stores that group plain.  No HIP
// in here: tests/test_step_chunk_order.py compiles it into a host program.
#pragma once

#include "common.hpp"

#if defined(__HIPCC__)
#define LIFEAPI_HD __host__ __device__ __forceinline__
#else
#define LIFEAPI_HD inline
#endif

namespace lifeapi_impl {

// Block b's place in a grid of nb blocks with each XCD dealt one contiguous
// run of places (device.hpp xcd_chunk_block, where the numbering is derived).
LIFEAPI_HD uint64_t xcd_chunk_place(uint32_t b, uint32_t nb) {
  const uint32_t q = nb >> 3, r = nb & 7u, x = b & 7u;
  return (uint64_t)x * q + (x < r ? x : r) + (b >> 3);
}

// What wave `wib` of block b takes on its `pass`-th stride over the batch (a
// one-shot grid has pass 0 only), in a launch of nb blocks over `groups`
// groups:
// * index: its number in the launch's order, b's place (chunked or not) x
//   waves per block + wib, a grid further per pass; it takes a group only if
//   index < groups;
// * group: the group of universes, `index` counted from the front or, in a
//   reversed launch, from the back of the batch;
// * plain: by DISPATCH POSITION, b x waves per block + wib (a grid further
//   per pass), from plain_from on.  Blocks are dispatched in the order of b,
//   round-robin over the XCDs, so position says when in the launch the wave
//   runs, and the plain-stored tail is what the launch writes last: without
//   chunks the last groups of its order (index = position), with chunks the
//   end of every XCD's run.
// Reversal mirrors the chunked order as a whole: on a grid of 8q blocks
// filled with groups, position t of XCD x takes what position T - 1 - t of
// XCD 7 - x took in the forward launch, so a reversed launch still reads
// first what the forward one wrote last (on any other grid the runs differ
// by a block and the mirror image is off by at most that).
struct StepTake {
  uint64_t index, group;
  bool plain;
};
LIFEAPI_HD StepTake step_take(uint32_t b, uint32_t nb, uint32_t wib, uint64_t pass, uint64_t groups, bool chunk,
                              bool reverse, uint64_t plain_from) {
  const uint64_t off = wib + pass * nb * kWavesPerBlock;
  const uint64_t index = (chunk ? xcd_chunk_place(b, nb) : (uint64_t)b) * kWavesPerBlock + off;
  return {index, reverse ? groups - 1 - index : index, (uint64_t)b * kWavesPerBlock + off >= plain_from};
}

}  // namespace lifeapi_impl
