// step_kernels.hpp -- the step kernels of batched LifeState::Step()
// (LifeAPI.hpp:1196-1216, Stepped(n) :877-886): k_step (natural layout, one
// column per lane), k_step_dma (the same through LDS) and k_step_split (8-way
// row split, state resident in VGPRs across generations).  The generation
// networks are in life_gen.hpp, the fused Step + Contains kernels in
// contains_kernels.hpp.  step.hip instantiates the shipped configurations;
// the tuning build (tools/tune/tune_step.hip) instantiates the measured
// alternatives.
#pragma once

#include "life_gen.hpp"
#include "split_layout.hpp"
#include "split_asm.inc"
#include "step_order.hpp"

namespace lifeapi_impl {
// internal linkage: every library that includes this header gets its own
// kernels (the product and the tuning build never share instantiations)
namespace {

// out[u] = in[u] stepped `gens` times.  Wave w of the grid takes groups of U
// consecutive universes, grid-strided.  All branches are wave-uniform.
// in == out is allowed (Step() in place), so neither pointer is
// __restrict__: each wave loads its universes before it stores them and no
// wave touches another's (the same holds for k_step_split).
// Bit 31 of `gens` (kReverse) reverses the order in which waves take the
// groups: alternated between launches, each launch first reads what the one
// before it wrote last.  The waves from dispatch position `plain_from` on
// (block x waves per block + wave, the order in which the grid is dispatched)
// store with plain stores, the rest as NTS says: the last-written part then
// stays in the memory-side Infinity Cache for the next launch to read first,
// and the nontemporal rest does not evict it.  The launcher
// sets both only for gens <= 2.
constexpr uint32_t kReverse = 1u << 31;
// Bit 30 of `gens` (kXcdChunk): each XCD takes a contiguous eighth of the
// groups (xcd_chunk_block); the plain-stored tail is then the end of every
// XCD's eighth, and a reversed launch starts on those ends.
constexpr uint32_t kXcdChunk = 1u << 30;
// step_body takes all of this from step_order.hpp step_take, which a host
// test checks wave by wave (tests/test_step_chunk_order.py).  (The decode of
// the two bits is written out in step_body_dma and contains_kernels.hpp
// k_step_contains, and the store tail in k_step_contains too, by group index
// as before: through shared helpers those kernels compiled to other code,
// tools/isa_diff.py and profiles/r08/README.md; k_step's difference under
// step_take is in profiles/r17/README.md.)

// NTS: nontemporal stores (default: as the loads) before `plain_from`.
//
// One group of U universes from u0 on.  FULL: all U lie below n, so loads and
// stores are unconditional and the wave's memory schedule is U loads back to
// back, each universe's generations behind a wait for its own load only, and
// U stores back to back.  gfx9's vmcnt counts stores with loads, and a store
// under a branch of its own (the ragged form, FULL = false) makes the
// compiler wait for everything outstanding before every store: the stores of
// a wave then complete one after another.
template <int X, int U, bool NT, int RULE, bool NTS, bool FULL>
__device__ __forceinline__ void step_group(const uint64_t *in, uint64_t *out, uint64_t n, uint32_t gens,
                                           uint64_t u0, bool nts, uint64_t *slot, int lane) {
  W a[U];
#pragma unroll
  for (int k = 0; k < U; ++k)
    a[k] = (FULL || u0 + k < n) ? ld<NT>(in + (u0 + k) * kWave + lane) : W{0u, 0u};
  if constexpr (RULE == 4) {
#pragma unroll
    for (int k = 0; k < U; ++k) a[k] = to_eo(a[k]);
  }
  for (uint32_t g = 0; g < gens; ++g) {
#pragma unroll
    for (int k = 0; k < U; ++k) a[k] = life_gen<X, RULE>(a[k], slot + k * 2 * kWave, lane);
  }
  if constexpr (RULE == 4) {
#pragma unroll
    for (int k = 0; k < U; ++k) a[k] = from_eo(a[k]);
  }
  if (nts) {
#pragma unroll
    for (int k = 0; k < U; ++k)
      if (FULL || u0 + k < n) st<NTS>(out + (u0 + k) * kWave + lane, a[k]);
  } else {
    // (the two comments keep the arms apart: unconditional stores to the same
    // addresses in both are hoisted or sunk into one run, which loses the
    // nontemporal hint -- metadata to the optimiser)
    if constexpr (FULL) asm volatile("; plain-stored tail");
#pragma unroll
    for (int k = 0; k < U; ++k)
      if (FULL || u0 + k < n) st<false>(out + (u0 + k) * kWave + lane, a[k]);
    if constexpr (FULL) asm volatile("; plain-stored tail end");
  }
}

// ONESHOT: the grid has a wave for every group (grid_for(groups, cus, 0), as
// every launch of the product), so a wave takes one group and ends behind its
// stores without waiting for them; else waves stride over the groups.
template <int X, int U, bool NT, int RULE, bool NTS, bool ONESHOT = false>
__device__ __forceinline__ void step_body(const uint64_t *in, uint64_t *out, uint64_t n, uint32_t gens,
                                          uint64_t plain_from) {
  __shared__ uint64_t lds[uses_lds(X) ? kWavesPerBlock * U * 2 * kWave : 1];
  const int lane = threadIdx.x & (kWave - 1);
  // wave index in the block, made provably wave-uniform so that the tail
  // tests below are scalar branches
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const bool rev = (gens & kReverse) != 0, chunk = (gens & kXcdChunk) != 0;
  gens &= ~(kReverse | kXcdChunk);
  const uint64_t groups = (n + U - 1) / U;
  uint64_t *slot = lds + (uses_lds(X) ? wib * U * 2 * kWave : 0);
  // the wave's pass-th group: its index in the launch's order, the group, and
  // whether it stores plain (by dispatch position: step_order.hpp step_take)
  auto take = [&](uint64_t pass) __attribute__((always_inline)) {
    const StepTake t = step_take(blockIdx.x, gridDim.x, wib, pass, groups, chunk, rev, plain_from);
    if (t.index >= groups) return false;
    const uint64_t u0 = t.group * U;
    if (u0 + U <= n) step_group<X, U, NT, RULE, NTS, true>(in, out, n, gens, u0, !t.plain, slot, lane);
    else step_group<X, U, NT, RULE, NTS, false>(in, out, n, gens, u0, !t.plain, slot, lane);
    return true;
  };
  if constexpr (ONESHOT) {
    take(0);
  } else {
    for (uint64_t pass = 0; take(pass); ++pass) {
    }
  }
}

template <int X, int U, bool NT, int RULE, bool NTS = NT, bool ONESHOT = false>
__global__ __launch_bounds__(kBlock) void k_step(const uint64_t *in, uint64_t *out, uint64_t n,
                                                 uint32_t gens, uint64_t plain_from) {
  step_body<X, U, NT, RULE, NTS, ONESHOT>(in, out, n, gens, plain_from);
}
// The same kernel under another name, for the tuning build's side launches
// (bench.py's cache-neutral and copy figures, the order A/Bs), so that a
// rocprofv3 trace of the bench tells them from the product's launches.
template <int X, int U, bool NT, int RULE, bool NTS = NT, bool ONESHOT = false>
__global__ __launch_bounds__(kBlock) void k_step_ab(const uint64_t *in, uint64_t *out, uint64_t n,
                                                    uint32_t gens, uint64_t plain_from) {
  step_body<X, U, NT, RULE, NTS, ONESHOT>(in, out, n, gens, plain_from);
}

// step_body with the wave's U universes moved through LDS (the LifeStable
// passes' LDS-DMA form, stable_kernels.hpp k_stable_dma): U / 2
// sixteen-byte-per-lane global_load_lds in (lanes 0-31 one universe, 32-63 the
// next), ds_read_b64 out to lane = column; WIDE: the results back through the
// image, 16 bytes per lane (ds_write_b64, ds_read_b128, global_store_dwordx4),
// else 8-byte stores from the lanes.  Order and XCD chunking as step_body;
// the plain-stored tail by group index (with chunks: not the part written
// last).  The batch must be 16-byte aligned.
template <int U, int RULE, bool NTS, bool WIDE>
__device__ __forceinline__ void step_body_dma(const uint64_t *in, uint64_t *out, uint64_t n, uint32_t gens,
                                              uint64_t plain_from) {
  static_assert(U % 2 == 0, "pairs of universes per 16-byte load");
  __shared__ uint64_t img_all[kWavesPerBlock][U * kWave];
  const int lane = threadIdx.x & (kWave - 1);
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  uint64_t *img = img_all[wib];
  const bool rev = (gens & kReverse) != 0;
  const uint64_t blk = (gens & kXcdChunk) ? xcd_chunk_block() : (uint64_t)blockIdx.x;
  gens &= ~(kReverse | kXcdChunk);
  const uint64_t groups = (n + U - 1) / U, wstride = (uint64_t)gridDim.x * kWavesPerBlock;
  for (uint64_t grp = blk * kWavesPerBlock + wib; grp < groups; grp += wstride) {
    const uint64_t u0 = (rev ? groups - 1 - grp : grp) * U;
#pragma unroll
    for (int i = 0; i < U / 2; ++i) {  // (cone_passes.hpp dma_fetch_pass, written out)
      uint64_t u = u0 + 2 * i + (lane >> 5);
      if (u >= n) u = n - 1;  // (a valid address; the result is not stored)
      const char *src = reinterpret_cast<const char *>(in + u * kWave) + (lane & 31) * 16;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                       (__attribute__((address_space(3))) void *)(img + i * 2 * kWave), 16, 0, 2);
    }
    __builtin_amdgcn_s_waitcnt(kWaitVm0);
    W a[U];
#pragma unroll
    for (int k = 0; k < U; ++k) a[k] = split(img[k * kWave + lane]);
    for (uint32_t g = 0; g < gens; ++g) {
#pragma unroll
      for (int k = 0; k < U; ++k) a[k] = life_gen<XDPP, RULE>(a[k], nullptr, lane);
    }
    const bool nt = NTS && grp < plain_from;
    if constexpr (WIDE) {
#pragma unroll
      for (int k = 0; k < U; ++k) img[k * kWave + lane] = join(a[k]);
      const u64x2 *src = reinterpret_cast<const u64x2 *>(img) + lane;
#pragma unroll
      for (int i = 0; i < U / 2; ++i) {
        const uint64_t u = u0 + 2 * i + (lane >> 5);
        const u64x2 v = src[i * kWave];
        u64x2 *dst = reinterpret_cast<u64x2 *>(out + u * kWave) + (lane & 31);
        if (u < n) {
          if (nt) __builtin_nontemporal_store(v, dst);
          else *dst = v;
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < U; ++k)
        if (u0 + k < n) {
          if (nt) st<true>(out + (u0 + k) * kWave + lane, a[k]);
          else st<false>(out + (u0 + k) * kWave + lane, a[k]);
        }
    }
  }
}

template <int U, int RULE, bool NTS, bool WIDE>
__global__ __launch_bounds__(kBlock) void k_step_dma(const uint64_t *in, uint64_t *out, uint64_t n, uint32_t gens,
                                                     uint64_t plain_from) {
  step_body_dma<U, RULE, NTS, WIDE>(in, out, n, gens, plain_from);
}

// k_step for the split layouts: wave w takes G groups of P = S/2
// consecutive universes, grid-strided; all branches wave-uniform.  NET: the
// tail network (7 = RULE 3's, 6 = life_tail6); D: registers exchanged by DPP
// instead of LDS (gen_split), or kPipe: the software-pipelined LDS loop
// (gens_split_pipe).
constexpr int kPipe = -1;
constexpr int kAsmLoop = -3;  // the hand-allocated rule-11 loop (split_asm.inc)
// WPB: waves per block (the tuning build's A/B of finer blocks; the product
// launches kWavesPerBlock).
template <int S, int G, bool NT, int NET, int D = 0, int V = 0, int WPB = kWavesPerBlock>
__global__ __launch_bounds__(WPB * kWave) void k_step_split(const uint64_t *in, uint64_t *out, uint64_t n,
                                                            uint32_t gens, uint64_t /* plain_from: k_step's */) {
  constexpr int P = S / 2;
  __shared__ uint32_t lds[WPB * G * S * kWave];
  const int lane = threadIdx.x & (kWave - 1);
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const uint64_t per_wave = (uint64_t)G * P;
  const uint64_t stride = (uint64_t)gridDim.x * WPB * per_wave;
  for (uint64_t u0 = ((uint64_t)blockIdx.x * WPB + wib) * per_wave; u0 < n; u0 += stride) {
    uint32_t r[G][S];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      W c[P];
#pragma unroll
      for (int u = 0; u < P; ++u) {
        const uint64_t x = u0 + g * P + u;
        c[u] = x < n ? ld<NT>(in + x * kWave + lane) : W{0u, 0u};
      }
      Split<S>::load(c, r[g]);
    }
    if constexpr (D == kPipe) {
#pragma unroll
      for (int g = 0; g < G; ++g) gens_split_pipe<S, NET>(r[g], lds + (wib * G + g) * S * kWave, lane, gens);
    } else if constexpr (D == kAsmLoop) {
      static_assert(S == 8 && NET == 6 && G <= 2, "split_asm.inc is rule 11, one or two groups");
      const uint32_t base = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)(
          lds + wib * G * S * kWave);  // group g's planes at base + 2 KiB * g
      const uint32_t self = base + lane * 16u, prev = base + ((lane + kWave - 1) & (kWave - 1)) * 16u,
                     next = base + ((lane + 1) & (kWave - 1)) * 16u;
      if constexpr (G == 2) split_gens_asm2(r[0], r[1], gens, self, prev, next);
      else if constexpr (V == 1) split_gens_asm_v1(r[0], gens, self, prev, next);
      else if constexpr (V == 2) split_gens_asm_v2(r[0], gens, self, prev, next);
      else if constexpr (V == 3) split_gens_asm_v3(r[0], gens, self, prev, next);
      else split_gens_asm_v0(r[0], gens, self, prev, next);
    } else {
      for (uint32_t it = 0; it < gens; ++it) {
#pragma unroll
        for (int g = 0; g < G; ++g) gen_split<S, NET, D>(r[g], lds + (wib * G + g) * S * kWave, lane);
      }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      W c[P];
      Split<S>::store(r[g], c);
#pragma unroll
      for (int u = 0; u < P; ++u) {
        const uint64_t x = u0 + g * P + u;
        if (x < n) st<NT>(out + x * kWave + lane, c[u]);
      }
    }
  }
}

}  // namespace
}  // namespace lifeapi_impl
