// wave_groups.hpp -- the vocabulary of the kernels that run one wave per group
// of U objects with lane = column (match, pair, symmetry, components and weld
// kernels): the wave's place and its loop over the groups, the load and the
// store of an object with the batch's ragged end guarded, and the lanes that
// store a group's wave-uniform per-object scalars.  Each helper compiles to
// the instructions the kernels had with the same text spelled out; the few
// spots where it does not are left spelled out and say so
// (profiles/r19/README.md has the list and the shapes that were tried).
#pragma once

#include "device.hpp"

namespace lifeapi_impl {
namespace {

// the wave's place: its lane, and which wave of the block it is (through
// readfirstlane, so that what is computed from it is scalar)
__device__ __forceinline__ int wave_lane() { return threadIdx.x & (kWave - 1); }
__device__ __forceinline__ int wave_in_block() { return __builtin_amdgcn_readfirstlane(threadIdx.x / kWave); }

// The groups of U objects this wave takes:
//   const WaveGroups at = wave_groups<U>(wib, n);
//   for (uint64_t g = at.first; g < at.groups; g += at.stride) { objects g * U .. g * U + U - 1, those < n }
// Wave wib of block b starts at group b * kWavesPerBlock + wib (blockIdx.x as
// it is, no XCD chunking) and strides by the grid's waves: a grid with a wave
// for every group runs the body once, a capped one loops.
struct WaveGroups {
  uint64_t first, groups, stride;
};
template <int U>
__device__ __forceinline__ WaveGroups wave_groups(int wib, uint64_t n) {
  const uint64_t groups = (n + U - 1) / U, stride = (uint64_t)gridDim.x * kWavesPerBlock;
  return {(uint64_t)blockIdx.x * kWavesPerBlock + wib, groups, stride};
}

// Word `col` of object u, the objects WORDS words apart (kWave: states; a
// multiple: one plane of an object of several, `base` at the plane); zero
// past the batch's end.
template <int WORDS = kWave>
__device__ __forceinline__ W load_object(const uint64_t *base, uint64_t u, uint64_t n, int col) {
  return u < n ? ld<true>(base + u * WORDS + col) : W{0u, 0u};
}
template <int WORDS = kWave>
__device__ __forceinline__ void store_object(uint64_t *base, uint64_t u, uint64_t n, int lane, W v) {
  if (u < n) st<true>(base + u * WORDS + lane, v);
}

// A group's PER * U wave-uniform scalars, PER per object, go out with one
// vector store: lane PER * k + j picks up object u0 + k's j-th as it is found
// (h = lane == PER * k + j ? value : h) and, if it holds one of an object
// below n, stores it: if (holds_scalar<U, PER>(u0, n, lane)) out[u0 * PER + lane] = h.
template <int U, int PER>
__device__ __forceinline__ bool holds_scalar(uint64_t u0, uint64_t n, int lane) {
  return lane < PER * U && u0 + (uint64_t)(lane / PER) < n;
}

}  // namespace
}  // namespace lifeapi_impl
