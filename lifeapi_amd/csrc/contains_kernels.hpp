// contains_kernels.hpp -- Step() (LifeAPI.hpp:1196-1216) fused with
// Contains(LifeTarget) (LifeTarget.hpp:44-51) after every generation, the
// search loop's filter: k_step_contains (gens <= 2, the streaming step's
// shape) and k_step_contains_split (the 8-way split layout of k_step_split
// with the test inside the assembly loops of split_asm.inc; its waves hand a
// target with a small light cone to the passes of cone_passes.hpp and
// cone_split.hpp).  step.hip instantiates the shipped configurations; the
// tuning build (tools/tune/tune_step.hip) instantiates the measured
// alternatives.
#pragma once

#include <type_traits>

#include "cone_passes.hpp"
#include "cone_split.hpp"
#include "step_kernels.hpp"

namespace lifeapi_impl {
// internal linkage: every library that includes this header gets its own
// kernels (the product and the tuning build never share instantiations)
namespace {

// Step + Contains fused for gens <= 2 (k_step_contains_split takes more):
// first generation in 1..gens whose state contains the target (0 = never);
// the state keeps stepping to `gens` for d_final.  The streaming step's
// shape -- U universes per wave, loads issued first, nontemporal -- so the
// search filter of SURVEY 8(f) row 1 reads 512 B and writes 4 B per
// universe.  `in` and `fin` may be the same array (the host form stages
// through one buffer), so neither is __restrict__: each wave loads its
// universes before it stores them, and no wave touches another's universes.
// Group order (kReverse in `gens`) and the plain-stored tail of the final
// states (`plain_from`) as k_step's.
// X / RULE: the exchange and network of the generation (life_gen).  PF: each
// wave loads the next group's states before it works on the current one (a
// grid of at most the resident waves, looping over the batch).
// FAST (the 8-byte form on a one-shot grid, a wave for every group): a full
// group loads and stores unconditionally and the wave ends behind its stores,
// as step_group's FULL path; the ragged last group keeps the guards.
template <int U, bool WIDE = false, int X = XDPP, int RULE = 3, bool PF = false, bool FAST = false>
__global__ __launch_bounds__(kBlock) void k_step_contains(const uint64_t *in, uint64_t *fin,
                                                          const uint64_t *__restrict__ wanted,
                                                          const uint64_t *__restrict__ unwanted,
                                                          uint32_t *__restrict__ first,
                                                          uint64_t n, uint32_t gens, uint64_t plain_from) {
  // WIDE: the states move as 16-byte accesses (two adjacent columns per
  // lane, two universes per wave-instruction) staged through the wave's own
  // U x 512 B of LDS, which turns them into lane = column (and back for the
  // final states); the batch must be 16-byte aligned
  __shared__ uint64_t stage[WIDE || uses_lds(X) ? kWavesPerBlock * U * kWave : 1];
  const int lane = threadIdx.x & (kWave - 1);
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const W w = split(wanted[lane]), uw = split(unwanted[lane]);
  // (step_body's decode of the launch order and step_group's store tail,
  // both written out again: through shared helpers the shipped <8> form keeps
  // its registers but compiles to a different instruction stream,
  // tools/isa_diff.py, profiles/r08/README.md)
  const bool rev = (gens & kReverse) != 0;
  const uint64_t blk = (gens & kXcdChunk) ? xcd_chunk_block() : (uint64_t)blockIdx.x;
  gens &= ~(kReverse | kXcdChunk);
  const uint64_t groups = (n + U - 1) / U, wstride = (uint64_t)gridDim.x * kWavesPerBlock;
  uint64_t *st_w = stage + (WIDE || uses_lds(X) ? wib * U * kWave : 0);
  const int half = lane >> 5, col = (lane & 31) * 2;
  static_assert(!(PF && WIDE), "the prefetching loop is the 8-byte form's");
  static_assert(!(FAST && (PF || WIDE)), "the one-shot fast path is the plain 8-byte form's");
  W an[U];
  auto load_group = [&](uint64_t g, W (&dst)[U]) __attribute__((always_inline)) {
    const uint64_t v0 = (rev ? groups - 1 - g : g) * U;
#pragma unroll
    for (int k = 0; k < U; ++k) dst[k] = (v0 + k < n) ? ld<true>(in + (v0 + k) * kWave + lane) : W{0u, 0u};
  };
  if constexpr (PF) {
    const uint64_t g0 = blk * kWavesPerBlock + wib;
    if (g0 < groups) load_group(g0, an);
  }
  // one group; full_c: all of its U universes lie below n (FAST only)
  auto group = [&](uint64_t grp, auto full_c) __attribute__((always_inline)) {
    constexpr bool FULL = decltype(full_c)::value;
    const uint64_t u0 = (rev ? groups - 1 - grp : grp) * U;
    W a[U];
    if constexpr (PF) {
#pragma unroll
      for (int k = 0; k < U; ++k) a[k] = an[k];
      if (grp + wstride < groups) load_group(grp + wstride, an);
    } else if constexpr (WIDE) {
      static_assert(U % 2 == 0, "universes come in pairs");
      u64x2 v[U / 2];
#pragma unroll
      for (int k = 0; k < U / 2; ++k) {
        const uint64_t u = u0 + 2 * k + half;
        v[k] = u < n ? __builtin_nontemporal_load(reinterpret_cast<const u64x2 *>(in + u * kWave + col))
                     : u64x2{0ull, 0ull};
      }
#pragma unroll
      for (int k = 0; k < U / 2; ++k)
        *reinterpret_cast<u64x2 *>(st_w + (2 * k + half) * kWave + col) = v[k];
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int k = 0; k < U; ++k) a[k] = split(st_w[k * kWave + lane]);
      __builtin_amdgcn_wave_barrier();  // (the final states reuse the stage below)
    } else {
#pragma unroll
      for (int k = 0; k < U; ++k)
        a[k] = (FULL || u0 + k < n) ? ld<true>(in + (u0 + k) * kWave + lane) : W{0u, 0u};
    }
    uint32_t hit[U];
#pragma unroll
    for (int k = 0; k < U; ++k) hit[k] = 0;
    for (uint32_t g = 1; g <= gens; ++g) {
#pragma unroll
      for (int k = 0; k < U; ++k) {
        a[k] = life_gen<X, RULE>(a[k], uses_lds(X) ? st_w + k * kWave : nullptr, lane);
        if (hit[k] == 0 && wave_contains(a[k], w, uw)) hit[k] = g;
      }
    }
    // lanes 0..U-1 write the U first-hit generations with one store (FULL:
    // ahead of the final states, whose registers it would else wait for)
    auto store_first = [&]() __attribute__((always_inline)) {
      uint32_t h = hit[0];
#pragma unroll
      for (int k = 1; k < U; ++k) h = lane == k ? hit[k] : h;
      if (lane < U && (FULL || u0 + lane < n)) first[u0 + lane] = h;
    };
    if constexpr (FULL) store_first();
    if constexpr (WIDE) {
      if (fin) {
#pragma unroll
        for (int k = 0; k < U; ++k) st_w[k * kWave + lane] = join(a[k]);
        __builtin_amdgcn_wave_barrier();
        const bool nt = grp < plain_from;
#pragma unroll
        for (int k = 0; k < U / 2; ++k) {
          const uint64_t u = u0 + 2 * k + half;
          const u64x2 v = *reinterpret_cast<const u64x2 *>(st_w + (2 * k + half) * kWave + col);
          u64x2 *dst = reinterpret_cast<u64x2 *>(fin + u * kWave + col);
          if (u < n) {
            if (nt) __builtin_nontemporal_store(v, dst);
            else *dst = v;
          }
        }
        __builtin_amdgcn_wave_barrier();  // (the next group's loads reuse the stage)
      }
    } else if (fin && grp < plain_from) {
#pragma unroll
      for (int k = 0; k < U; ++k)
        if (FULL || u0 + k < n) st<true>(fin + (u0 + k) * kWave + lane, a[k]);
    } else if (fin) {
      // (the comments keep this arm apart from the nontemporal one: step_group)
      if constexpr (FULL) asm volatile("; plain-stored tail");
#pragma unroll
      for (int k = 0; k < U; ++k)
        if (FULL || u0 + k < n) st<false>(fin + (u0 + k) * kWave + lane, a[k]);
      if constexpr (FULL) asm volatile("; plain-stored tail end");
    }
    if constexpr (!FULL) store_first();
  };
  if constexpr (FAST) {
    const uint64_t grp = blk * kWavesPerBlock + wib;
    if (grp < groups) {
      if ((rev ? groups - 1 - grp : grp) * U + U <= n) group(grp, std::true_type{});
      else group(grp, std::false_type{});
    }
  } else {
    for (uint64_t grp = blk * kWavesPerBlock + wib; grp < groups; grp += wstride) group(grp, std::false_type{});
  }
}

// The same on the 8-way split layout (k_step_split): 4 universes per wave.
// The target is put into the same register layout once, replicated for the
// 4 universes; after every generation (r ^ w) & (w | u) is OR-ed over the
// registers and tested per universe (its bits are every P-th).
// Without d_final, a wave of the compiled loop stops once all its universes
// have hit.
constexpr uint32_t kDiff = ((TA ^ TB) & (TB | TC)) & 0xFF;  // (s ^ wanted) & (wanted | unwanted)
constexpr int kContainsNet = 6;  // tail network of the fused kernel (as k_step's default, rule 11)
// ASM selects the loop (times: config 3, 64K universes x 1024 generations,
// a block + ring target, against the plain step's 1.27-1.30 ms;
// profiles/r02/contains_ab*.jsonl):
//   0  the compiled loop below (a ballot per universe and generation)
//   1  the assembly loop of split_asm.inc with the test after every
//      generation: 8 differences, 3 OR3, per universe a masked OR + compare
//      and 8 SALU (1.760 ms)
//   2  1 with lean bookkeeping: two SALU per universe and generation, hits
//      on a slow path (1.668)
//   3  2 on the target's row window: every wave finds the smallest cyclic
//      window [y0, y0 + h) of rows that holds all of the target's care cells
//      (wanted | unwanted) and, when h <= 8, rotates the universes and the
//      target up by y0 rows (Life on the torus commutes with translation,
//      and so does Contains), so that the care rows are the split layout's
//      residues 0..h-1 and the test differences only h of the 8 registers;
//      d_final is rotated back (1.558-1.621; 78-87 VGPRs, 5-6 waves/SIMD)
//   4  3 with the scalar part after the plane-1 exchange (no gain)
//   5  3 with the test batched over eight generations for h <= 7: each
//      generation's OR of differences occupies bits 0..3 only, so it packs
//      into a nibble of one word, whose lane OR (DPP) and scalar test run
//      once per block (1.456; 92 VGPRs, 4 waves)
//   6  3 in the low register layout: a window of at most 4 rows, the target
//      in v52..v59 (1.563: the occupancy alone gains nothing)
//   7  5 in the low layout (1.397, +9.8 %: 64 VGPRs, 8 waves)
//   8  the rest of 5: windows of more than 4 rows (batched up to 7, the
//      per-generation test on 8 and on targets with no window)
// 6 and 7 do nothing for a window wider than 4 rows, 8 nothing for the
// others.  step.hip ships kContainsLo then kContainsHi: every wave of both
// finds the same window, so exactly one of them works and the other's waves
// return at once.  Each wave-uniform choice of loop runs its own copy of the
// pass over the universes (`universes` below), so the register allocator
// sees one assembly loop's pins at a time: 8 takes 71 VGPRs (7 waves per
// SIMD; profiles/r08/README.md), where one shared pass took 84 (5), and 7
// takes 62 (8 waves).
constexpr int kContainsLo = 7, kContainsHi = 8;
// 9: both in one kernel (each wave takes the loop its window calls for), so
// that one launch answers any target; the kernel takes kContainsHi's 72
// VGPRs (7 waves per SIMD), which costs the low layout nothing measurable
// (6 above: the low layout's occupancy alone gained nothing)
constexpr int kContainsAll = 9;
// (Measured, commit 5278498: targets with no row window of at most 7 rows
// batched over eight generations, each generation's differences folded onto
// a nibble, instead of the lean per-generation test -- no gain, 1M x 3-13
// generations within -2 .. +3 %, profiles/r06/batch_h8_ab/; the lean test
// stays.  tools/tune/split_asm_tune.inc keeps split_contains_asm_batch_h8.)
// the light-cone path of kContainsLo (cone_max below): universes per wave chunk
// (Measured in the compiler's allocation, not shipped: the whole board in the
// natural layout for wider cones at <= 4 generations -- 10-35 % faster there
// -- costs kContainsLo 7 VGPRs (62 -> 69, any register-set count) or
// kContainsHi 7 (70 -> 77), a wave per SIMD for every other target.)
// (16-universe chunks for cones of 9-32 columns: 6-8 % slower at 64K x 8-13
// generations, +4 % at 1M x 3, equal at 1M x 8-13; profiles/r04/r04ag)
constexpr int kConeLoUniverses = 8;
constexpr uint32_t kLowRows = 4;  // tools/gen_split_asm.py LOW_H

// cone_max: with no final states, a target whose light cone spans at most
// cone_max columns (0 = never) is answered on that cone: kContainsLo's waves
// step only those columns in the natural layout (cone_wave, 8 universes per
// wave chunk, looping over the batch), every other ASM's waves return at once.
// PF (16-byte aligned batch, no final states): the wave's next group of P
// universes is fetched into LDS by P / 2 sixteen-byte-per-lane
// global_load_lds (LDS-DMA: no VGPR destination, so the assembly loops keep
// their registers) as soon as the current group has been read out, and
// streams in while the current group steps; the generation loops' own LDS
// traffic is the exchange area, a different 2 KiB.
// WIN (no final states, 3 <= gens < 16): a target whose care rows, widened
// by the light cone, fit 32 rows (cone_rows) takes the window split layout
// (cone_split.hpp) on its column window -- or, on a whole board below
// kConeWholeWinGens generations, the packed LDS-DMA row pass.
template <int S, int NET, int ASM = 0, bool PF = false, bool WIN = false>
// (amdgpu_waves_per_eu(7): the shrinking window pass (cone_split.hpp) lifts
// the kernel's allocation 72 -> 76 VGPRs on its own, a wave per SIMD for
// every target; held at 72 it spills 12 bytes, reloaded once per chunk)
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(7))) void k_step_contains_split(const uint64_t *in, uint64_t *fin,
                                                                const uint64_t *__restrict__ wanted,
                                                                const uint64_t *__restrict__ unwanted,
                                                                uint32_t *__restrict__ first, uint64_t n,
                                                                uint32_t gens, uint32_t cone_max) {
  constexpr int P = S / 2;
  constexpr uint32_t every = P == 1 ? ~0u : P == 2 ? 0x55555555u : P == 4 ? 0x11111111u : 0x01010101u;
  // 4 KiB of LDS per wave: the exchange area of the generation loops
  // (S words per lane), then PF's fetch stage (P universes); the whole-board
  // row-window pass (WIN) takes all of it as its image (8 universes)
  static_assert(S * kWave * 4 + P * kWave * 8 <= 4096, "4 KiB per wave");
  __shared__ uint64_t wave_lds[kWavesPerBlock][512];
  const int lane = threadIdx.x & (kWave - 1);
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  uint32_t *const lds = reinterpret_cast<uint32_t *>(wave_lds[0]);  // (wave w's area: lds + w * 1024)
  // the target's care cells in this lane's column (both windows read it;
  // the cone test first: after the row window's, it costs kContainsHi 6
  // VGPRs, 70 -> 76)
  const uint64_t care_col = wanted[lane] | unwanted[lane];
  if constexpr (WIN) {
    if (!fin && gens >= kConeRowsWindowGens && gens < 16u) {
      uint32_t y0w = 0;
      const int pk = cone_rows(care_col, gens, y0w);
      if (pk > 0) {
        const uint64_t wave = (uint64_t)blockIdx.x * kWavesPerBlock + wib, nw = (uint64_t)gridDim.x * kWavesPerBlock;
        uint32_t xs = 0, K = kWave;
        const bool whole = cone_whole(care_col, gens);
        if (!whole) cone_window(care_col, gens, xs, K);
        if constexpr (PF) {  // (a 16-byte aligned batch)
          if (whole && gens < kConeWholeWinGens) {
            // the whole board's row window below kConeWholeWinGens: the
            // packed LDS-DMA pass (cone_passes.hpp cone_wave_rows_dma, chunks
            // of 16 universes, 8 per pass fetched while the last steps)
            const uint64_t w64 = wanted[lane], m64 = w64 | unwanted[lane];
            uint64_t *img = wave_lds[wib];
            auto rows = [&](auto pk_c, auto wrap_c) __attribute__((always_inline)) {
              cone_wave_rows_dma<8, decltype(pk_c)::value, decltype(wrap_c)::value>(
                  in, w64, m64, first, n, wave * 16, nw * 16, gens, y0w, lane, img, false);
            };
            using T = std::true_type;
            using F = std::false_type;
            using P1 = std::integral_constant<int, 1>;
            using P2 = std::integral_constant<int, 2>;
            using P4 = std::integral_constant<int, 4>;
            if (pk == 4) return y0w >= 32u ? rows(P4{}, T{}) : rows(P4{}, F{});
            if (pk == 2) return y0w >= 32u ? rows(P2{}, T{}) : rows(P2{}, F{});
            return y0w >= 32u ? rows(P1{}, T{}) : rows(P1{}, F{});
          }
        }
        return cone_split_pass(in, wanted, unwanted, first, n, wave, nw, gens, xs, K, pk, y0w, lane,
                               reinterpret_cast<uint32_t *>(wave_lds[wib]), PF);
      }
    }
  }
  // (2 gens in 64 bits: in 32 it wraps for gens >= 2^31)
  if (cone_max && cone_max <= 32u && !fin && 2ull * gens < cone_max && cone_fits(care_col, gens, cone_max)) {
    if constexpr (ASM == kContainsLo || ASM == kContainsAll) {
      uint32_t cxs, cK;
      cone_window(care_col, gens, cxs, cK);  // cK <= cone_max (cone_fits)
      {
        constexpr int U = kConeLoUniverses;
        const uint64_t u0 = ((uint64_t)blockIdx.x * kWavesPerBlock + wib) * U,
                       step = (uint64_t)gridDim.x * kWavesPerBlock * U;
        if (cK <= 8) cone_wave<8, U, 8, true>(in, wanted, unwanted, first, n, u0, step, gens, cxs, cK, lane);
        else if (cK <= 16) cone_wave<16, U, 8, true>(in, wanted, unwanted, first, n, u0, step, gens, cxs, cK, lane);
        else cone_wave<32, U, 8, true>(in, wanted, unwanted, first, n, u0, step, gens, cxs, cK, lane);
      }
    }
    return;
  }
  uint32_t y0 = 0, h = S;  // the row window of ASM 3 (else: no rotation, all registers)
  if constexpr (ASM >= 3) {
    const uint32_t lo = wave_or_u32_dpp((uint32_t)care_col), hi = wave_or_u32_dpp((uint32_t)(care_col >> 32));
    care_window((uint64_t)lo | (uint64_t)hi << 32, y0, h);
    if (h > S) y0 = 0, h = S;
    if (ASM == 8 && h <= kLowRows) return;  // the low layout's target
  }
  if constexpr (ASM == 6 || ASM == 7) {
    if (h > kLowRows) return;  // the low layout: windows of <= 4 rows only (8 the rest)
  }
  uint32_t tw[S], tu[S];
  {
    W c[P];
#pragma unroll
    for (int u = 0; u < P; ++u) c[u] = split(rotr64(wanted[lane], y0));
    Split<S>::load(c, tw);
#pragma unroll
    for (int u = 0; u < P; ++u) c[u] = split(rotr64(unwanted[lane], y0));
    Split<S>::load(c, tu);
  }
  uint32_t tm[S];  // wanted | unwanted (the assembly loop's second target plane)
#pragma unroll
  for (int j = 0; j < S; ++j) tm[j] = tw[j] | tu[j];

  // one pass over this wave's groups of P universes with `gens_loop(r, hit)`
  // as the generation loop; every wave-uniform choice of loop (below) gets
  // its own copy of this pass, so that each assembly loop's pinned registers
  // are all the register allocator sees around it
  auto universes_pf = [&](auto &&gens_loop) __attribute__((always_inline)) {
    static_assert(P % 2 == 0, "pairs of universes per 16-byte load");
    uint64_t *img = wave_lds[wib] + S * kWave / 2;  // (after the exchange area)
    const uint64_t stride = (uint64_t)gridDim.x * kWavesPerBlock * P;
    // (dma_fetch_pass written out, on a fresh lane index per fetch so that
    // none stays live across the loops: through the helper the compiler
    // associates the address sums the other way round, which reschedules
    // some 800 lines of the shipped kernel around the assembly loops)
    auto fetch = [&](uint64_t ub) __attribute__((always_inline)) {
      const uint32_t ln = lane_id_fresh();
#pragma unroll
      for (int i = 0; i < P / 2; ++i) {
        uint64_t u = ub + 2 * i + (ln >> 5);
        if (u >= n) u = n - 1;  // (a valid address; its answer is not stored)
        const char *src = reinterpret_cast<const char *>(in + u * kWave) + (ln & 31) * 16;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                         (__attribute__((address_space(3))) void *)(img + i * 2 * kWave), 16, 0, 2);
      }
    };
    uint64_t u0 = ((uint64_t)blockIdx.x * kWavesPerBlock + wib) * P;
    if (u0 >= n) return;
    fetch(u0);
    bool stored = false;  // an answer store was issued after the pending fetch
    for (; u0 < n; u0 += stride) {
      const uint64_t left = n - u0;
      const uint32_t avail = (left >> 2) ? (uint32_t)P : (uint32_t)left;
      // the fetch is the only older vector-memory op but the answer store
      // (in issue order: MI355X_MICROARCH.md, s_waitcnt vmcnt)
      if (stored) __builtin_amdgcn_s_waitcnt(kWaitVm1);
      else __builtin_amdgcn_s_waitcnt(kWaitVm0);
      uint32_t r[S];
      {
        // the P columns of this lane, read in one assembly block: a compiled
        // LDS read after an LDS-DMA makes the compiler wait for every
        // outstanding vector-memory op (vmcnt(0)), the last answer store
        // included; the counted wait above is the one this read needs
        static_assert(P == 4, "four universes per group");
        const uint32_t at = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)img +
                            lane_id_fresh() * 8u;
        uint64_t v0, v1, v2, v3;
        asm volatile(
            "ds_read_b64 %0, %4\n"
            "ds_read_b64 %1, %4 offset:512\n"
            "ds_read_b64 %2, %4 offset:1024\n"
            "ds_read_b64 %3, %4 offset:1536\n"
            "s_waitcnt lgkmcnt(0)\n"
            : "=&v"(v0), "=&v"(v1), "=&v"(v2), "=&v"(v3)
            : "v"(at)
            : "memory");
        W c[P] = {split(v0), split(v1), split(v2), split(v3)};
        if (y0) {  // (wave-uniform)
#pragma unroll
          for (int u = 0; u < P; ++u) c[u] = split(rotr64(join(c[u]), y0));
        }
        if (u0 + stride < n) fetch(u0 + stride);  // (the stage is read out: the next group may land)
        Split<S>::load(c, r);
      }
      uint32_t hit[P];
#pragma unroll
      for (int u = 0; u < P; ++u) hit[u] = 0;
      gens_loop(r, hit);
      const uint32_t ln2 = lane_id_fresh();
      // (lanes 0..P-1 take hit[u], as k_step_contains's store_first; a helper
      // taking hit[] by reference has the compiler move it to LDS here: 48 B
      // of scratch and 4 KiB more LDS per block)
      uint32_t h = hit[0];
#pragma unroll
      for (int u = 1; u < P; ++u) h = ln2 == (uint32_t)u ? hit[u] : h;
      if (ln2 < avail) first[u0 + ln2] = h;  // one store instruction
      stored = true;
    }
  };
  auto universes = [&](auto &&gens_loop) __attribute__((always_inline)) {
    if constexpr (PF) {
      if (!fin) return universes_pf(gens_loop);
    }
    const uint64_t stride = (uint64_t)gridDim.x * kWavesPerBlock * P;
    for (uint64_t u0 = ((uint64_t)blockIdx.x * kWavesPerBlock + wib) * P; u0 < n; u0 += stride) {
      // the wave's universes u0 .. u0 + avail - 1 from scalar bases: a 64-bit
      // lane address or a vector copy of n kept across the loop would cost
      // VGPRs, and the low layout's occupancy hangs on the last four
      const uint64_t left = n - u0;
      const uint32_t avail = (left >> 2) ? (uint32_t)P : (uint32_t)left;
      const uint64_t *src = in + u0 * kWave;
      const uint32_t ln = lane_id_fresh();
      uint32_t r[S];
      W c[P];
#pragma unroll
      for (int u = 0; u < P; ++u) c[u] = (uint32_t)u < avail ? split(src[u * kWave + ln]) : W{0u, 0u};
      if (y0) {  // (wave-uniform: the row window's rotation, none for a window of 8 rows from row 0)
#pragma unroll
        for (int u = 0; u < P; ++u) c[u] = split(rotr64(join(c[u]), y0));
      }
      Split<S>::load(c, r);
      uint32_t hit[P];
#pragma unroll
      for (int u = 0; u < P; ++u) hit[u] = 0;
      gens_loop(r, hit);
      const uint32_t ln2 = lane_id_fresh();  // not kept live across the loop
      if (fin) {
        Split<S>::store(r, c);
        uint64_t *dst = fin + u0 * kWave;
#pragma unroll
        for (int u = 0; u < P; ++u)
          if ((uint32_t)u < avail) dst[u * kWave + ln2] = y0 ? rotr64(join(c[u]), 64 - y0) : join(c[u]);
      }
      if (ln2 == 0) {
#pragma unroll
        for (int u = 0; u < P; ++u)
          if ((uint32_t)u < avail) first[u0 + u] = hit[u];
      }
    }
  };
  if constexpr (ASM) {  // split_asm.inc: the default generation loop with the test fused in
    static_assert(S == 8 && NET == 6 && P == 4, "split_contains_asm is rule 11");
    // (this lane's 16 bytes of the exchange area and its cyclic neighbours',
    // as k_step_split: a shared helper is simplified on its own before it is
    // inlined and leaves both shipped kernels other address arithmetic)
    const uint32_t base = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)(lds + wib * 1024);
    const uint32_t self = base + lane * 16u, prev = base + ((lane + kWave - 1) & (kWave - 1)) * 16u,
                   next = base + ((lane + 1) & (kWave - 1)) * 16u;
#define LIFEAPI_RUN(fn)                                                                          \
  universes([&](uint32_t(&r)[S], uint32_t(&hit)[P]) __attribute__((always_inline)) {            \
    fn(r, tw, tm, gens, self, prev, next, hit);                                                  \
  })
#define LIFEAPI_BY_H(pre, wide)                                                                  \
  switch (h) { /* wave-uniform */                                                                \
    case 1: LIFEAPI_RUN(pre##1); break;                                                          \
    case 2: LIFEAPI_RUN(pre##2); break;                                                          \
    case 3: LIFEAPI_RUN(pre##3); break;                                                          \
    case 4: LIFEAPI_RUN(pre##4); break;                                                          \
    case 5: LIFEAPI_RUN(pre##5); break;                                                          \
    case 6: LIFEAPI_RUN(pre##6); break;                                                          \
    case 7: LIFEAPI_RUN(pre##7); break;                                                          \
    default: LIFEAPI_RUN(wide); break;                                                           \
  }
    if constexpr (ASM == 2) {
      LIFEAPI_RUN(split_contains_asm_lean);
    } else if constexpr (ASM == 8) {
      if (h == 5) LIFEAPI_RUN(split_contains_asm_batch_h5);
      else if (h == 6) LIFEAPI_RUN(split_contains_asm_batch_h6);
      else if (h == 7) LIFEAPI_RUN(split_contains_asm_batch_h7);
      else LIFEAPI_RUN(split_contains_asm_lean);
    } else if constexpr (ASM == kContainsAll) {
      if (h <= kLowRows) LIFEAPI_RUN(split_contains_asm_batch_lo);
      else if (h == 5) LIFEAPI_RUN(split_contains_asm_batch_h5);
      else if (h == 6) LIFEAPI_RUN(split_contains_asm_batch_h6);
      else if (h == 7) LIFEAPI_RUN(split_contains_asm_batch_h7);
      else LIFEAPI_RUN(split_contains_asm_lean);
    } else if constexpr (ASM == 7) {
      LIFEAPI_RUN(split_contains_asm_batch_lo);
    } else if constexpr (ASM == 6) {
      LIFEAPI_RUN(split_contains_asm_lean_lo);
    } else if constexpr (ASM == 5) {
      LIFEAPI_BY_H(split_contains_asm_batch_h, split_contains_asm_lean)
    } else if constexpr (ASM == 4) {
      LIFEAPI_BY_H(split_contains_asm_lean_late_h, split_contains_asm_lean_late)
    } else if constexpr (ASM == 3) {
      LIFEAPI_BY_H(split_contains_asm_lean_h, split_contains_asm_lean)
    } else {
      LIFEAPI_RUN(split_contains_asm);
    }
#undef LIFEAPI_BY_H
#undef LIFEAPI_RUN
  } else {
    universes([&](uint32_t(&r)[S], uint32_t(&hit)[P]) __attribute__((always_inline)) {
      uint32_t found = 0;
      for (uint32_t g = 1; g <= gens; ++g) {
        gen_split<S, NET>(r, lds + wib * 1024, lane);
        uint32_t d = 0;
#pragma unroll
        for (int j = 0; j < S; ++j) d |= lut3<kDiff>(r[j], tw[j], tu[j]);
        // straight-line: a ballot per universe, the bookkeeping in scalar registers
        uint32_t clean = 0;
#pragma unroll
        for (int u = 0; u < P; ++u) clean |= (__ballot((d & (every << u)) != 0) == 0 ? 1u : 0u) << u;
        const uint32_t fresh = clean & ~found;
#pragma unroll
        for (int u = 0; u < P; ++u) hit[u] = (fresh >> u) & 1 ? g : hit[u];
        found |= fresh;
        if (!fin && found == (1u << P) - 1) break;
      }
    });
  }
}

}  // namespace
}  // namespace lifeapi_impl
