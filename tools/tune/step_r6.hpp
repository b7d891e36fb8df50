// step_r6.hpp -- the streaming step's body as round 6 shipped it, kept for
// the tuning build's same-process A/B against the product's step_body
// (tools/step_store_ab.py; lifeapi_tune_step_order_body, body 6).  Every load
// and every store sits under its own `u0 + k < n` branch, and the waves
// stride over the groups: the compiler then waits for everything outstanding
// (vmcnt(0)) before each store and once more behind the last one, so a wave's
// stores complete one after another before it ends.
#pragma once

#include "step_kernels.hpp"

namespace lifeapi_impl {
namespace {

template <int X, int U, bool NT, int RULE, bool NTS>
__device__ __forceinline__ void step_body_r6(const uint64_t *in, uint64_t *out, uint64_t n, uint32_t gens,
                                          uint64_t plain_from) {
  __shared__ uint64_t lds[uses_lds(X) ? kWavesPerBlock * U * 2 * kWave : 1];
  const int lane = threadIdx.x & (kWave - 1);
  // wave index in the block, made provably wave-uniform so that the tail
  // tests below are scalar branches
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const bool rev = (gens & kReverse) != 0;
  const uint64_t blk = (gens & kXcdChunk) ? xcd_chunk_block() : (uint64_t)blockIdx.x;
  gens &= ~(kReverse | kXcdChunk);
  const uint64_t groups = (n + U - 1) / U, wstride = (uint64_t)gridDim.x * kWavesPerBlock;
  for (uint64_t grp = blk * kWavesPerBlock + wib; grp < groups; grp += wstride) {
    const uint64_t u0 = (rev ? groups - 1 - grp : grp) * U;
    W a[U];
#pragma unroll
    for (int k = 0; k < U; ++k)
      a[k] = (u0 + k < n) ? ld<NT>(in + (u0 + k) * kWave + lane) : W{0u, 0u};
    if constexpr (RULE == 4) {
#pragma unroll
      for (int k = 0; k < U; ++k) a[k] = to_eo(a[k]);
    }
    for (uint32_t g = 0; g < gens; ++g) {
#pragma unroll
      for (int k = 0; k < U; ++k)
        a[k] = life_gen<X, RULE>(a[k], lds + (wib * U + k) * 2 * kWave, lane);
    }
    if constexpr (RULE == 4) {
#pragma unroll
      for (int k = 0; k < U; ++k) a[k] = from_eo(a[k]);
    }
    if (grp < plain_from) {
#pragma unroll
      for (int k = 0; k < U; ++k)
        if (u0 + k < n) st<NTS>(out + (u0 + k) * kWave + lane, a[k]);
    } else {
#pragma unroll
      for (int k = 0; k < U; ++k)
        if (u0 + k < n) st<false>(out + (u0 + k) * kWave + lane, a[k]);
    }
  }
}

template <int X, int U, bool NT, int RULE, bool NTS = NT>
__global__ __launch_bounds__(kBlock) void k_step_r6(const uint64_t *in, uint64_t *out, uint64_t n,
                                                    uint32_t gens, uint64_t plain_from) {
  step_body_r6<X, U, NT, RULE, NTS>(in, out, n, gens, plain_from);
}

}  // namespace
}  // namespace lifeapi_impl
