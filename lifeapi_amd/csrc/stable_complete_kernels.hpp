// stable_complete_kernels.hpp -- LifeStable::CompleteStable (LifeStable.hpp:
// 1340-1458) as a wave-per-LifeStable backtracking search: k_stable_complete.
// stable_complete.hip launches it.
//
// One wave per LifeStable, lane x = column x of its 10 planes, as
// stable_kernels.hpp; the object under search stays in registers.  The
// reference's recursion is one explicit stack: the on-branch is a tail call
// (:1409), so only a pending "try off first" holds a frame -- the object after
// its Propagate() and the chosen cell.  A frame is pushed before the off-branch;
// when the off-branch returns INCONSISTENT (or, minimising, COMPLETED) it is
// popped and SetOn(cell) applied; TIMEOUT, and COMPLETED when not minimising,
// drop the whole stack.  The stacks live in a global workspace, one per
// resident wave (not per object), frames written and read as whole 128-byte
// lines by vector stores and loads, each lane its own words only.  The waves
// take their objects from a counter at the head of the workspace (a vector
// atomic add from lane 0): a node's cost depends on the data, and a fixed
// stride through a periodic batch gives one wave every slow object (DESIGN.md
// 3.12).
//
// The reference's clock is a per-object node budget: `nodes` counts entries of
// CompleteStableStep over the whole call, tail calls included, and "past the
// time limit" is nodes >= budget at the two places the reference reads the
// time (:1343, :1439).  Every branch comes from a ballot or a reduced scalar
// and is wave-uniform.  No LDS.  Registers and measurements: DESIGN.md 3.13.
#pragma once

#include "stable_test_kernels.hpp"

namespace lifeapi_impl {

enum : int { kCompleted = 0, kInconsistent = 1, kTimeout = 2, kTooDeep = 3, kBadSeed = 4 };
// the workspace: a header (the claim counter), then per wave max_depth frames of
// 10 planes x 512 bytes and the cell, 4 bytes per lane
constexpr size_t kCompleteHeaderBytes = 256, kCompleteFrameBytes = 10 * 512 + 256;
constexpr uint32_t kCompleteFlagMinimise = 1u, kCompleteFlagUseSeed = 2u;

namespace {

// LifeState::GetPop (wave-uniform)
__device__ __forceinline__ uint32_t get_pop(W a) {
  return wave_sum_u32_dpp((uint32_t)__builtin_popcount(a.lo) + (uint32_t)__builtin_popcount(a.hi));
}
// LifeState::ZOI, LifeAPI.hpp:521-536: the 3 x 3 neighbourhoods' OR on the torus
__device__ __forceinline__ W zoi_full(W s) {
  const W t = s | rot_up(s) | rot_dn(s);
  W L, R;
  cols_lr(t, L, R);
  return L | t | R;
}
// LifeState::BigZOI, LifeAPI.hpp:564-591: the plus, then its 3 x 3
__device__ __forceinline__ W zoi_big(W s) {
  W L, R;
  cols_lr(s, L, R);
  return zoi_full(s | rot_up(s) | rot_dn(s) | L | R);
}
__device__ __forceinline__ W one_cell(int lane, uint32_t x, uint32_t y) {
  const uint32_t bit = (uint32_t)lane == x ? 1u << (y & 31u) : 0u;
  return y < 32u ? W{bit, 0u} : W{0u, bit};
}

// The cell CompleteStableStep branches on (:1378-1391): the first of
// Vulnerable() & settable, else of the settable cells with two unknown
// neighbours (NeighbourCount(unknown), the cell included), else with three,
// else of settable; false when there is none
__device__ __forceinline__ bool branch_cell(const W (&p)[10], W settable, uint32_t &x, uint32_t &y) {
  if (first_on(stable_vulnerable(p) & settable, x, y)) return true;
  W u3, u2, u1, u0;
  ncount4(p[PUN], u3, u2, u1, u0);
  const W low = settable & ~u3 & ~u2 & u1;
  if (first_on(low & ~u0, x, y)) return true;
  if (first_on(low & u0, x, y)) return true;
  return first_on(settable, x, y);
}

// CompleteStable of objects claimed from *counter, one at a time per wave.
// flags: kCompleteFlag*; budget: the node budget (1 .. 1 << 24); stacks: wave
// w's frames at stacks + w * max_depth * kCompleteFrameBytes, for the first
// `waves` waves of the grid (the rest leave at once).  result[u]: kCompleted
// .. kBadSeed; best[u]: the completion, empty unless kCompleted; nodes[u]
// (may be null): the nodes entered.  The planes are not written.
__global__ __launch_bounds__(kBlock) void k_stable_complete(const uint64_t *__restrict__ planes,
                                                            const uint64_t *__restrict__ seeds, uint32_t per_object,
                                                            uint32_t flags, uint32_t budget, uint32_t max_depth,
                                                            uint64_t *__restrict__ best_out,
                                                            uint8_t *__restrict__ result, uint64_t *__restrict__ nodes_out,
                                                            unsigned long long *counter, char *stacks, uint64_t waves,
                                                            uint64_t n) {
  const int lane = threadIdx.x & (kWave - 1);
  const uint64_t wave = (uint64_t)blockIdx.x * kWavesPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  if (wave >= waves) return;
  char *const stack = stacks + wave * max_depth * kCompleteFrameBytes;
  const bool minimise = (flags & kCompleteFlagMinimise) != 0u, seeded = (flags & kCompleteFlagUseSeed) != 0u;
  const W none = W{0u, 0u}, all = W{~0u, ~0u};
  for (;;) {
    unsigned long long claimed = 0;
    if (lane == 0) claimed = atomicAdd(counter, 1ull);
    const uint64_t u = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)claimed) |
                       (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(claimed >> 32)) << 32;
    if (u >= n) break;
    const uint64_t *q = planes + u * 10 * kWave + lane;
    const W state0 = ld<true>(q), unknown0 = ld<true>(q + kWave);
    W best = none, seed = none;
    if (seeded) seed = ld<false>(seeds + (per_object ? u * kWave : 0) + lane);
    uint32_t nodes = 0, max_pop = 0x7FFFFFFFu;
    int res;
    if (!wave_any(state0)) {
      res = kCompleted;  // :1415
    } else if (!wave_any(unknown0)) {
      res = kCompleted;  // :1418
      best = state0;
    } else if (seeded && !wave_any(seed)) {
      res = kBadSeed;  // the reference's loop at :1369 would not end
    } else {
      // the search-area rounds (:1431-1442), then the minimise pass (:1450-1455)
      W area = zoi_full(state0);
      const bool once = !wave_any(unknown0 & ~area);  // no round would run: one step on the object as given
      if (!once) area = zoi_full(area);
      W mask = once ? all : area;
      bool use_seed = seeded, second = false;
      for (;;) {
        W p[10];
#pragma unroll
        for (int k = 0; k < 10; ++k) p[k] = ld<false>(q + k * kWave);
        p[PUN] = p[PUN] & mask;
        // ---- CompleteStableStep (:1340-1412) on its stack ----
        uint32_t sp = 0;
        int r;
        for (;;) {
          r = -1;
          if (nodes >= budget) {
            r = kTimeout;
          } else {
            ++nodes;
            W chg = none;
            if (!(stable_loop<3, false>(p, chg, 1u << 20) & 1)) {
              r = kInconsistent;
            } else {
              const uint32_t pop = get_pop(p[PST]);
              W settable = (p[PL2] | p[PL3] | p[PD0] | p[PD1] | p[PD2] | p[PD4] | p[PD5] | p[PD6]) & p[PUN] &
                           zoi_full(p[PD0]);
              if (pop >= max_pop) {
                r = kCompleted;
              } else if (!wave_any(settable)) {
                best = p[PST];
                max_pop = pop;
                r = kCompleted;
              } else {
                if (use_seed) {
                  // a non-empty seed's 64th ZOI is the whole torus
                  W z = seed;
                  for (int grow = 0; grow < 64 && !wave_any(settable & z); ++grow) z = zoi_full(z);
                  settable = settable & z;
                }
                uint32_t x = 0, y = 0;
                if (!branch_cell(p, settable, x, y)) {
                  r = kInconsistent;
                } else if (sp == max_depth) {
                  r = kTooDeep;
                } else {
                  uint64_t *f = reinterpret_cast<uint64_t *>(stack + (size_t)sp * kCompleteFrameBytes) + lane;
#pragma unroll
                  for (int k = 0; k < 10; ++k) st<false>(f + k * kWave, p[k]);
                  reinterpret_cast<uint32_t *>(f - lane + 10 * kWave)[lane] = x | y << 8;
                  ++sp;
                  stable_set(p, none, one_cell(lane, x, y));  // try off
                }
              }
            }
          }
          if (r < 0) continue;
          if (r == kTooDeep || r == kTimeout || sp == 0 || (!minimise && r == kCompleted)) break;
          --sp;  // then must be on
          const uint64_t *f = reinterpret_cast<const uint64_t *>(stack + (size_t)sp * kCompleteFrameBytes) + lane;
#pragma unroll
          for (int k = 0; k < 10; ++k) p[k] = ld<false>(f + k * kWave);
          const uint32_t cell =
              (uint32_t)__builtin_amdgcn_readfirstlane(reinterpret_cast<const uint32_t *>(f - lane + 10 * kWave)[lane]);
          stable_set(p, one_cell(lane, cell & 63u, cell >> 8), none);
        }
        // ---- CompleteStable after a step ----
        if (r == kTooDeep) {
          res = kTooDeep;
          best = none;
          break;
        }
        if (second) {  // a timeout in the minimise pass is ignored
          res = kCompleted;
          break;
        }
        const bool found = wave_any(best);
        if (!once && !found && nodes < budget && wave_any(unknown0 & ~area)) {
          area = zoi_full(area);
          mask = area;
          continue;
        }
        if (!found && r != kCompleted) {
          res = r;
          break;
        }
        if (!minimise) {
          res = kCompleted;
          break;
        }
        second = true;  // again with a little more space, near what was found
        mask = zoi_big(area);
        use_seed = true;
        seed = state0 | best;
      }
    }
    st<true>(best_out + u * kWave + lane, best);
    if (lane == 0) {
      result[u] = (uint8_t)res;
      if (nodes_out) nodes_out[u] = nodes;
    }
  }
}

}  // namespace
}  // namespace lifeapi_impl
