// stable_test_kernels.hpp -- the LifeStable strip passes (LifeStable.hpp:
// 921-948, 995-1249), TestUnknown / TestUnknowns (:1251-1284, :1321-1338, Join
// :217-233) and PropagateAndTest (:163-184) as wave-per-LifeStable kernels:
// k_stable_strip<PASS> and k_stable_test<OP>.  stable_test.hip launches them.
//
// One wave per LifeStable, lane x = column x of its 10 planes, as
// stable_kernels.hpp.  A strip pass at column x is the full pass under two
// lane masks (the torus: d = (lane - x + 2) & 63):
//   S6 = columns x-2 .. x+3 (d < 6)   GetStrip<6>: state, unknown, the writes
//   S4 = columns x-1 .. x+2 (1 <= d <= 4)   GetStrip<4>: the option planes
// CountNeighbourhoodStrip's counts at the S4 columns read S6 only, so they are
// the full counts there (ncount4).  SynchroniseStateKnownStrip is the column
// pass on S6; UpdateOptionsStrip keeps the count fragment's eight outputs and
// its abort on S4; SignalNeighboursStrip keeps the signal fragment's four
// outputs on S4 before the hollow ZOI, whose writes then land in S6 by
// themselves.  Where the strip passes differ from the full ones in what an
// inconsistent object is left as, the strip's form is kept: sync and options
// finish their columns and then report, signal returns before writing, the
// step stops at the first inconsistent pass.
//
// TestUnknown keeps the object and its two trials in registers (3 x 10 planes
// x 2 VGPRs); the trials run one after the other through the same code (a
// two-turn loop that is not unrolled), the first parked in `on` while the
// second runs.  Every branch comes from a ballot or a scalar and is
// wave-uniform.  No LDS.  Registers and measurements: DESIGN.md 3.12.
#pragma once

#include "components_kernels.hpp"
#include "stable_kernels.hpp"

namespace lifeapi_impl {

// TestUnknowns erases a cell per turn
constexpr uint32_t kMaxTestTurns = 4096;

namespace {

struct StripMask {
  W s6, s4;
};
__device__ __forceinline__ StripMask strip_mask(int lane, uint32_t x) {
  const uint32_t d = ((uint32_t)lane - x + 2u) & 63u;
  const uint32_t m6 = d < 6u ? ~0u : 0u, m4 = (d - 1u) < 4u ? ~0u : 0u;
  return {W{m6, m6}, W{m4, m4}};
}

// Every strip pass returns the reference's PropagateResult as it stands,
// consistent | changed << 1.

// SynchroniseStateKnownStrip, LifeStable.hpp:921-948 (the column pass :892-919)
__device__ __forceinline__ int strip_sync(W (&p)[10], const StripMask &m) {
  const W known_on = ~p[PUN] & p[PST] & m.s6;
  const W maybe_dead = ~(p[PD0] & p[PD1] & p[PD2] & p[PD4] & p[PD5] & p[PD6]);
  W changes = maybe_dead & known_on;
#pragma unroll
  for (int k = PD0; k <= PD6; ++k) p[k] = p[k] | known_on;
  const W known_off = ~p[PUN] & ~p[PST] & m.s6;
  const W maybe_live = ~(p[PL2] & p[PL3]);
  changes = changes | (maybe_live & known_off);
  p[PL2] = p[PL2] | known_off;
  p[PL3] = p[PL3] | known_off;
  const W on = maybe_live & ~maybe_dead & m.s6, both = maybe_live & maybe_dead;
  changes = changes | (~p[PST] & on);
  p[PST] = p[PST] | on;
  changes = changes | (~p[PUN] & both & m.s6);
  p[PUN] = p[PUN] & (both | ~m.s6);
  return (wave_any(~maybe_live & ~maybe_dead & m.s6) ? 0 : 1) | (wave_any(changes) ? 2 : 0);
}

// UpdateOptionsStrip, LifeStable.hpp:1111-1195
__device__ __forceinline__ int strip_options(W (&p)[10], const StableCounts &c, const StripMask &m) {
  const W off = ~p[PUN] & ~p[PST];
  const W x[9] = {c.s2, c.s1, c.s0, c.o3, c.o2, c.o1, c.o0, p[PST], off};
  W r[8], ab;
  stable_count_circuit(x, r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], ab);
  W changes = W{0u, 0u};
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const W rk = r[k] & m.s4;
    changes = changes | (rk & ~p[PL2 + k]);
    p[PL2 + k] = p[PL2 + k] | rk;
  }
  return (wave_any(ab & m.s4) ? 0 : 1) | (wave_any(changes) ? 2 : 0);
}

// SignalNeighboursStrip, LifeStable.hpp:995-1109; s = the count of the state,
// mx = of state | unknown
__device__ __forceinline__ int strip_signal(W (&p)[10], W s2, W s1, W s0, W m3, W m2, W m1, W m0,
                                            const StripMask &m) {
  const W x[17] = {p[PL2], p[PL3], p[PD0], p[PD1], p[PD2], p[PD4], p[PD5], p[PD6], s2, s1, s0,
                   m3, m2, m1, m0, p[PST], p[PUN]};
  W soff, son, coff, con;
  stable_signal_circuit(x, soff, son, coff, con);
  const W off_zoi = zoi_hollow(soff & m.s4) | (coff & m.s4), on_zoi = zoi_hollow(son & m.s4) | (con & m.s4);
  if (wave_any(off_zoi & on_zoi & p[PUN])) return 0;
  const W w_off = off_zoi & p[PUN], w_on = on_zoi & p[PUN];
  p[PST] = (p[PST] & ~w_off) | w_on;
  p[PUN] = p[PUN] & ~(w_off | w_on);
  p[PL2] = p[PL2] | w_off;
  p[PL3] = p[PL3] | w_off;
#pragma unroll
  for (int k = PD0; k <= PD6; ++k) p[k] = p[k] | w_on;
  return 1 | (wave_any(w_off | w_on) ? 2 : 0);
}
__device__ __forceinline__ int strip_signal(W (&p)[10], const StripMask &m) {
  W s3, s2, s1, s0, m3, m2, m1, m0;
  ncount4(p[PST], s3, s2, s1, s0);
  ncount4(p[PST] | p[PUN], m3, m2, m1, m0);
  return strip_signal(p, s2, s1, s0, m3, m2, m1, m0, m);
}

// PropagateStepStrip, LifeStable.hpp:1215-1236: the state and unknown planes
// do not change between the options and the signal pass, so the counts are
// taken once (stable_step's form)
__device__ __forceinline__ int strip_step(W (&p)[10], const StripMask &m) {
  const int k = strip_sync(p, m);
  if (!(k & 1)) return 0;
  const StableCounts c = stable_counts(p);
  const int o = strip_options(p, c, m);
  if (!(o & 1)) return 0;
  W m3, m2, m1, m0;
  nine_minus(c.o3, c.o2, c.o1, c.o0, m3, m2, m1, m0);
  const int s = strip_signal(p, c.s2, c.s1, c.s0, m3, m2, m1, m0, m);
  if (!(s & 1)) return 0;
  return 1 | ((k | o | s) & 2);
}

// PropagateStrip (IT 3, LifeStable.hpp:1238-1249) and StabiliseOptionsStrip
// (IT 5, :1197-1213): 0 inconsistent, else 1 | changed << 1, | 4 when
// max_iters stopped the loop (stable_loop's form)
template <int IT>
__device__ __forceinline__ int strip_loop(W (&p)[10], const StripMask &m, uint32_t max_iters) {
  int ever = 0;
  for (uint32_t it = 0; it < max_iters; ++it) {
    int s;
    if constexpr (IT == 3) {
      s = strip_step(p, m);
    } else {
      static_assert(IT == 5, "PropagateStrip's or StabiliseOptionsStrip's iteration");
      const int k = strip_sync(p, m);
      if (!(k & 1)) return 0;
      const int o = strip_options(p, stable_counts(p), m);
      if (!(o & 1)) return 0;
      s = 1 | ((k | o) & 2);
    }
    if (!(s & 1)) return 0;
    if (!(s & 2)) return 1 | ever;
    ever = 2;
  }
  return 1 | ever | 4;
}

// The strip passes in place, each LifeStable at its own column (columns[u] &
// 63).  A strip pass changes columns of S6 only: their 128-byte lines are
// stored.
template <int PASS>
__global__ __launch_bounds__(kBlock) void k_stable_strip(uint64_t *__restrict__ planes,
                                                         const uint8_t *__restrict__ columns,
                                                         uint8_t *__restrict__ flags, uint64_t n, uint32_t max_iters) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const uint64_t stride = (uint64_t)gridDim.x * kWavesPerBlock;
  for (uint64_t u = (uint64_t)blockIdx.x * kWavesPerBlock + wib; u < n; u += stride) {
    uint64_t *q = planes + u * 10 * kWave + lane;
    W p[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) p[k] = ld<true>(q + k * kWave);
    const StripMask m = strip_mask(lane, (uint32_t)columns[u] & 63u);
    int r;
    if constexpr (PASS == 0) r = strip_sync(p, m);
    else if constexpr (PASS == 1) r = strip_options(p, stable_counts(p), m);
    else if constexpr (PASS == 2) r = strip_signal(p, m);
    else if constexpr (PASS == 3) r = strip_step(p, m);
    else if constexpr (PASS == 4) r = strip_loop<3>(p, m, max_iters);
    else r = strip_loop<5>(p, m, max_iters);
    const uint64_t dirty = __ballot(m.s6.lo != 0u);
    if ((dirty >> (lane & 48)) & 0xFFFFull) {
#pragma unroll
      for (int k = 0; k < 10; ++k) st<true>(q + k * kWave, p[k]);
    }
    if (lane == 0) flags[u] = (uint8_t)r;
  }
}

// SetOn / SetOff of cells (LifeStable.hpp:320-335)
__device__ __forceinline__ void stable_set(W (&p)[10], W on, W off) {
  p[PST] = (p[PST] | on) & ~off;
  p[PUN] = p[PUN] & ~(on | off);
  p[PL2] = p[PL2] | off;
  p[PL3] = p[PL3] | off;
#pragma unroll
  for (int k = PD0; k <= PD6; ++k) p[k] = p[k] | on;
}

// TestUnknown of cell (x, y), LifeStable.hpp:1251-1284: 0 inconsistent, 1 |
// changed << 1, or 4 when max_iters stopped a PropagateStrip.  The reference
// propagates the off-trial inside *this when the on-trial is inconsistent and
// inside a copy otherwise; both are the copy `t` here, taken back into p in
// the first case, so whatever the reference leaves in *this is in p.
__device__ __forceinline__ int test_unknown(W (&p)[10], uint32_t x, uint32_t y, int lane, uint32_t max_iters) {
  const StripMask m = strip_mask(lane, x);
  const uint32_t bit = (uint32_t)lane == x ? 1u << (y & 31u) : 0u;
  const W cell = y < 32u ? W{bit, 0u} : W{0u, bit};
  W on[10], t[10];
  int ron = 0, roff = 0;
#pragma unroll 1
  for (int trial = 0; trial < 2; ++trial) {
#pragma unroll
    for (int k = 0; k < 10; ++k) t[k] = p[k];
    const W none = W{0u, 0u};
    stable_set(t, trial == 0 ? cell : none, trial == 0 ? none : cell);
    const int r = strip_loop<3>(t, m, max_iters);
    if (r & 4) return 4;
    if (trial == 0) {
#pragma unroll
      for (int k = 0; k < 10; ++k) on[k] = t[k];
      ron = r;
    } else {
      roff = r;
    }
  }
  if (!(ron & 1)) {
#pragma unroll
    for (int k = 0; k < 10; ++k) p[k] = t[k];
    return (roff & 1) ? 3 : 0;
  }
  if (!(roff & 1)) {
#pragma unroll
    for (int k = 0; k < 10; ++k) p[k] = on[k];
    return 3;
  }
  if ((ron & 2) && (roff & 2)) {
    // Join, LifeStable.hpp:217-233
    W j[10];
    j[PUN] = on[PUN] | t[PUN] | (on[PST] ^ t[PST]);
    j[PST] = on[PST] & ~j[PUN];
#pragma unroll
    for (int k = PL2; k <= PD6; ++k) j[k] = on[k] & t[k];
    W diff = W{0u, 0u};
#pragma unroll
    for (int k = 0; k < 10; ++k) {
      diff = diff | (j[k] ^ p[k]);
      p[k] = j[k];
    }
    return 1 | (wave_any(diff) ? 2 : 0);
  }
  return 1;
}

// TestUnknowns(cells), LifeStable.hpp:1321-1338, in FirstOn order; `touched`
// takes the lanes whose columns a TestUnknown may have changed (its S6)
__device__ __forceinline__ int test_unknowns(W (&p)[10], W cells, int lane, uint32_t max_iters, uint32_t &touched) {
  W rem = cells & p[PUN];
  int any = 0;
  for (uint32_t turn = 0; turn < kMaxTestTurns; ++turn) {
    uint32_t x, y;
    if (!first_on(rem, x, y)) break;
    const uint32_t bit = (uint32_t)lane == x ? 1u << (y & 31u) : 0u;
    rem = rem & ~(y < 32u ? W{bit, 0u} : W{0u, bit});
    touched |= strip_mask(lane, x).s6.lo;
    const int r = test_unknown(p, x, y, lane, max_iters);
    if (r & 4) return 4;
    if (!(r & 1)) return 0;
    any |= r & 2;
    rem = rem & p[PUN];
  }
  return 1 | any;
}

// Vulnerable(), LifeStable.hpp:366-412 (k_stable_vulnerable's network)
__device__ __forceinline__ W stable_vulnerable(const W (&p)[10]) {
  W s3, s2, s1, s0, u3, u2, u1, u0;
  ncount4(p[PST], s3, s2, s1, s0);
  ncount4(p[PUN], u3, u2, u1, u0);
  const W x[15] = {p[PL2], p[PL3], p[PD0], p[PD1], p[PD2], p[PD4], p[PD5], p[PD6],
                   s2,     s1,     s0,     u3,     u2,     u1,     u0};
  W von, voff, vcon, vcoff;
  stable_vulnerable_circuit(x, von, voff, vcon, vcoff);
  return (zoi_hollow(von) | vcon) & (zoi_hollow(voff) | vcoff);
}

// PropagateAndTest, LifeStable.hpp:163-184: Propagate, then
// TestUnknowns(Vulnerable().ZOI()), until neither changes.  max_iters bounds
// the outer loop, every Propagate and every PropagateStrip, each on its own.
__device__ __forceinline__ int propagate_and_test(W (&p)[10], int lane, uint32_t max_iters, W &chg, uint32_t &touched) {
  int ever = 0;
  for (uint32_t round = 0; round < max_iters; ++round) {
    const int r = stable_loop<3, false>(p, chg, max_iters);
    if (r & 4) return 4;
    if (!(r & 1)) return 0;
    const W v = stable_vulnerable(p);
    const int t = test_unknowns(p, zoi_hollow(v) | v, lane, max_iters, touched);
    if (t & 4) return 4;
    if (!(t & 1)) return 0;
    if (!((r | t) & 2)) return 1 | ever;
    ever = 2;
  }
  return 4;
}

// OP 0: TestUnknowns(cells_u), cells one universe (per_object 0) or one per
// LifeStable; OP 1: PropagateAndTest (cells unused).  flags[u] = consistent |
// changed << 1, or 4 when max_iters stopped a loop: that LifeStable is then
// not written.
// (150 / 145 VGPRs, 3 waves per SIMD, no scratch.  Capped at 128 for a fourth
// wave, amdgpu_waves_per_eu(4), it spills 21 / 17 VGPRs to 84 / 72 bytes of
// scratch, so it is not.)
template <int OP>
__global__ __launch_bounds__(kBlock) void k_stable_test(uint64_t *__restrict__ planes,
                                                        const uint64_t *__restrict__ cells, uint32_t per_object,
                                                        uint8_t *__restrict__ flags, uint64_t n, uint32_t max_iters) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const uint64_t stride = (uint64_t)gridDim.x * kWavesPerBlock;
  for (uint64_t u = (uint64_t)blockIdx.x * kWavesPerBlock + wib; u < n; u += stride) {
    uint64_t *q = planes + u * 10 * kWave + lane;
    W p[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) p[k] = ld<true>(q + k * kWave);
    W chg = W{0u, 0u};
    uint32_t touched = 0;
    int r;
    if constexpr (OP == 0) {
      const W c = ld<false>(cells + (per_object ? u * kWave : 0) + lane);
      r = test_unknowns(p, c, lane, max_iters, touched);
    } else {
      r = propagate_and_test(p, lane, max_iters, chg, touched);
    }
    const uint64_t dirty = __ballot((chg.lo | chg.hi | touched) != 0u);
    if (r != 4 && ((dirty >> (lane & 48)) & 0xFFFFull)) {
#pragma unroll
      for (int k = 0; k < 10; ++k) st<true>(q + k * kWave, p[k]);
    }
    if (lane == 0) flags[u] = (uint8_t)r;
  }
}

}  // namespace
}  // namespace lifeapi_impl
