// cone_passes.hpp -- one wave's passes over its universes on a target's
// light cone (cone_window.hpp), in the natural layout: lane = column, P lanes
// per universe.  cone_wave (the column window), cone_wave_rows (column and row
// window, universes packed into 32-bit words), and the whole-board forms:
// cone_wave_full16 (Contains with 16-byte loads), cone_wave_full_dma and
// cone_wave_rows_dma (through LDS, dma_fetch_pass).  The kernels that run
// them are k_cone / k_cone_adapt (cone_kernels.hpp) and the iterated search
// loop's k_step_contains_split (contains_kernels.hpp); the window split layout
// is in cone_split.hpp.
#pragma once

#include "cone_window.hpp"
#include "life_gen.hpp"

namespace lifeapi_impl {
// internal linkage: every library that includes this header gets its own
// kernels (the product and the tuning build never share instantiations)
namespace {

// The light-cone pass (the kernels: cone_kernels.hpp, and the iterated search
// loop's low-layout kernel, contains_kernels.hpp).  One wave's chunks of UPW universes u0 .. u0 + UPW - 1, u0 = u_first,
// u_first + u_step, ... (< n), under the window (xs = first loaded column,
// K <= P loaded columns).  FIRST: out[u] = the first
// generation in 1..gens whose state contains the target (0 = never), else
// out[u] = Contains(target) of the state as loaded (gens unused).  Register
// sets go RMAX at a time: all their loads are issued before the first test.
// PIPE: a pass issues the next pass's loads before it steps its own sets
// (twice the registers for the data; an A/B, tools/cone_ab.py).
template <int P, int UPW, int RMAX, bool FIRST, typename OutT, bool PIPE = false>
__device__ __forceinline__ void cone_wave(const uint64_t *in, const uint64_t *__restrict__ wanted,
                                          const uint64_t *__restrict__ unwanted, OutT *__restrict__ out,
                                          uint64_t n, uint64_t u_first, uint64_t u_step, uint32_t gens,
                                          uint32_t xs, uint32_t K, int lane) {
  constexpr int GPS = kWave / P;  // universes per register set
  static_assert(UPW % GPS == 0, "a wave takes whole register sets");
  constexpr int R = UPW / GPS;
  constexpr int RB = R < RMAX ? R : RMAX;
  static_assert(R % RB == 0, "passes of RB sets");
  const uint32_t j = (uint32_t)lane & (P - 1), q = (uint32_t)lane / P;
  const uint32_t col = (xs + j) & (kWave - 1);
  const bool live = j < K;
  // the target's column under this lane (zero outside the window: the care
  // columns all lie in [x0, x0 + w), and no lane j >= K or margin lane maps
  // onto one while K <= 64)
  const uint64_t w64 = live ? wanted[col] : 0ull, m64 = live ? (w64 | unwanted[col]) : 0ull;
  const W tw = split(w64), tm = split(m64);
  const uint32_t sh = q * P;
  auto clean = [&](W s) __attribute__((always_inline)) {
    const uint32_t d = ((s.lo ^ tw.lo) & tm.lo) | ((s.hi ^ tw.hi) & tm.hi);
    const uint64_t bad = __ballot(d != 0u);  // wave-uniform
    if constexpr (P == kWave) return bad == 0ull;
    else return ((bad >> sh) & ((1ull << P) - 1)) == 0ull;
  };
  static_assert(UPW <= kWave, "one result per lane");
  for (uint64_t u0 = u_first; u0 < n; u0 += u_step) {
    uint32_t mine = 0;  // lane L: the result of universe u0 + L (one coalesced store per chunk)
    auto load = [&](int pass, W (&a)[RB]) __attribute__((always_inline)) {
      const uint64_t ub = u0 + (uint64_t)pass * RB * GPS + q;
#pragma unroll
      for (int k = 0; k < RB; ++k) {
        const uint64_t u = ub + (uint64_t)k * GPS;
        a[k] = (live && u < n) ? ld<true>(in + u * kWave + col) : W{0u, 0u};
      }
    };
    W nx[RB];
    if constexpr (PIPE) load(0, nx);
#pragma unroll 1
    for (int pass = 0; pass < R / RB; ++pass) {
      W a[RB];
      if constexpr (PIPE) {
#pragma unroll
        for (int k = 0; k < RB; ++k) a[k] = nx[k];
        if (pass + 1 < R / RB) load(pass + 1, nx);
      } else {
        load(pass, a);
      }
      uint32_t res[RB];
      if constexpr (FIRST) {
#pragma unroll
        for (int k = 0; k < RB; ++k) res[k] = 0;
        for (uint32_t g = 1; g <= gens; ++g) {
#pragma unroll
          for (int k = 0; k < RB; ++k) {
            a[k] = life_gen<XDPP, 3>(a[k], nullptr, lane);
            if (res[k] == 0 && clean(a[k])) res[k] = g;
          }
        }
      } else {
#pragma unroll
        for (int k = 0; k < RB; ++k) res[k] = clean(a[k]) ? 1u : 0u;
      }
      // set k's group q is universe u0 + pass * RB * GPS + k * GPS + q: its
      // result (uniform over the group) moves to that lane
#pragma unroll
      for (int k = 0; k < RB; ++k) {
        const uint32_t first = (uint32_t)(pass * RB + k) * GPS, rel = (uint32_t)lane - first;
        uint32_t v = res[k];
        if constexpr (GPS > 1) v = (uint32_t)__shfl((int)v, (int)((rel & (GPS - 1)) * P));
        if (rel < (uint32_t)GPS) mine = v;
      }
    }
    if (lane < UPW && u0 + lane < n) out[u0 + lane] = (OutT)mine;
  }
}

// cone_wave with the rows cut to the light cone too (the column window's
// counterpart of cone_wave_rows_dma, below): each lane's column is
// cut to rows y0 .. y0 + FW - 1 (FW = 32 / PK) by one v_alignbit (WRAP: the
// window crosses row 63), PK universes share one 32-bit register (universe
// field f in bits f FW ..), and the generation runs with 1-bit shifts for the
// vertical neighbours: the bits shifted in at a field's edges are wrong and
// move one row inwards per generation, never onto a care row, which lies at
// least `gens` rows inside its field (FIRST only; gens < 16).  Lanes as
// cone_wave: P per universe, GPS = 64 / P universes per register set, so one
// register holds PK GPS universes: register k, field f, group q is universe
// u0 + k PK GPS + f GPS + q.
template <int P, int UPW, int RMAX, int PK, bool WRAP, typename OutT>
__device__ __forceinline__ void cone_wave_rows(const uint64_t *in, const uint64_t *__restrict__ wanted,
                                               const uint64_t *__restrict__ unwanted, OutT *__restrict__ out,
                                               uint64_t n, uint64_t u_first, uint64_t u_step, uint32_t gens,
                                               uint32_t xs, uint32_t K, uint32_t y0, int lane) {
  constexpr int GPS = kWave / P, FW = 32 / PK, UPR = GPS * PK;
  static_assert(PK == 1 || PK == 2 || PK == 4, "fields of 32, 16 or 8 rows");
  static_assert(UPW % UPR == 0 && UPW <= kWave, "a wave takes whole registers, one result per lane");
  constexpr int R = UPW / UPR;
  constexpr int RB = R < RMAX ? R : RMAX;
  static_assert(R % RB == 0, "passes of RB registers");
  constexpr uint32_t fmask = FW == 32 ? ~0u : (1u << FW) - 1u;
  constexpr uint32_t rep = PK == 1 ? 1u : PK == 2 ? 0x00010001u : 0x01010101u;
  constexpr uint32_t kDiff = ((TA ^ TB) & TC) & 0xFF;  // (s ^ wanted) & care
  const uint32_t j = (uint32_t)lane & (P - 1), q = (uint32_t)lane / P;
  const uint32_t col = (xs + j) & (kWave - 1);
  const bool live = j < K;
  const uint32_t sh = y0 & 31u, gsh = q * P;
  auto cut = [&](uint64_t v) __attribute__((always_inline)) {
    const W w = split(v);
    return WRAP ? __builtin_amdgcn_alignbit(w.lo, w.hi, sh) : __builtin_amdgcn_alignbit(w.hi, w.lo, sh);
  };
  const uint64_t w64 = live ? wanted[col] : 0ull, m64 = live ? (w64 | unwanted[col]) : 0ull;
  const uint32_t tw = (cut(w64) & fmask) * rep, tm = (cut(m64) & fmask) * rep;
  for (uint64_t u0 = u_first; u0 < n; u0 += u_step) {
    uint32_t mine = 0;  // lane L: the result of universe u0 + L
#pragma unroll 1
    for (int pass = 0; pass < R / RB; ++pass) {
      const uint64_t ub = u0 + (uint64_t)pass * RB * UPR + q;
      uint32_t a[RB];
#pragma unroll
      for (int k = 0; k < RB; ++k) {
        uint32_t e[PK];
#pragma unroll
        for (int f = 0; f < PK; ++f) {
          const uint64_t u = ub + (uint64_t)(k * UPR + f * GPS);
          e[f] = (live && u < n) ? cut(__builtin_nontemporal_load(in + u * kWave + col)) : 0u;
        }
        if constexpr (PK == 1) {
          a[k] = e[0];
        } else if constexpr (PK == 2) {
          a[k] = __builtin_amdgcn_perm(e[1], e[0], 0x05040100u);
        } else {
          const uint32_t p01 = __builtin_amdgcn_perm(e[1], e[0], 0x0C0C0400u);
          const uint32_t p23 = __builtin_amdgcn_perm(e[3], e[2], 0x0C0C0400u);
          a[k] = __builtin_amdgcn_perm(p23, p01, 0x05040100u);
        }
      }
      uint32_t res[RB][PK];
#pragma unroll
      for (int k = 0; k < RB; ++k)
#pragma unroll
        for (int f = 0; f < PK; ++f) res[k][f] = 0;
      for (uint32_t g = 1; g <= gens; ++g) {
#pragma unroll
        for (int k = 0; k < RB; ++k) {
          const uint32_t L = dpp_prev(a[k]), Rt = dpp_next(a[k]);
          const uint32_t h0 = lut3<kXor3>(L, a[k], Rt), h1 = lut3<kMaj>(L, a[k], Rt);
          a[k] = life_tail6(h0 << 1, h0, h0 >> 1, h1 << 1, h1, h1 >> 1, a[k]);
          const uint32_t d = lut3<kDiff>(a[k], tw, tm);
#pragma unroll
          for (int f = 0; f < PK; ++f) {
            const uint64_t bad = __ballot((d & (fmask << (f * FW))) != 0u);
            bool clean;
            if constexpr (P == kWave) clean = bad == 0ull;
            else clean = ((bad >> gsh) & ((1ull << P) - 1)) == 0ull;
            if (res[k][f] == 0 && clean) res[k][f] = g;
          }
        }
      }
      // register k, field f, group q is universe u0 + (pass RB + k) UPR + f GPS + q:
      // its result (uniform over the group) moves to that lane
#pragma unroll
      for (int k = 0; k < RB; ++k)
#pragma unroll
        for (int f = 0; f < PK; ++f) {
          const uint32_t first = (uint32_t)((pass * RB + k) * UPR + f * GPS), rel = (uint32_t)lane - first;
          uint32_t v = res[k][f];
          if constexpr (GPS > 1) v = (uint32_t)__shfl((int)v, (int)((rel & (GPS - 1)) * P));
          if (rel < (uint32_t)GPS) mine = v;
        }
    }
    if (lane < UPW && u0 + lane < n) out[u0 + lane] = (OutT)mine;
  }
}

// Contains over the whole board (K = 64) on a 16-byte aligned batch: lane l
// reads words 2(l mod 32), 2(l mod 32) + 1 of universe 2k + l / 32 (one
// dwordx4 moves two universes per wave-instruction, as k_contains16), RMAX
// loads in flight per pass.
template <int UPW, int RMAX>
__device__ __forceinline__ void cone_wave_full16(const uint64_t *in, const uint64_t *__restrict__ wanted,
                                                 const uint64_t *__restrict__ unwanted, uint8_t *__restrict__ out,
                                                 uint64_t n, uint64_t u_first, uint64_t u_step, int lane) {
  constexpr int RB = UPW / 2 < RMAX ? UPW / 2 : RMAX;
  static_assert(UPW % (2 * RB) == 0, "passes of 2 RB universes");
  const int half = lane >> 5, col = (lane & 31) * 2;
  const uint64_t w0 = wanted[col], w1 = wanted[col + 1];
  const uint64_t m0 = w0 | unwanted[col], m1 = w1 | unwanted[col + 1];
  for (uint64_t u0 = u_first; u0 < n; u0 += u_step) {
    uint32_t mine = 0;  // lane L: the answer for universe u0 + L
#pragma unroll 1
    for (int pass = 0; pass < UPW / (2 * RB); ++pass) {
      const uint64_t ub = u0 + (uint64_t)pass * 2 * RB;
      u64x2 v[RB];
#pragma unroll
      for (int k = 0; k < RB; ++k) {
        const uint64_t u = ub + 2 * k + half;
        v[k] = u < n ? __builtin_nontemporal_load(reinterpret_cast<const u64x2 *>(in + u * kWave + col))
                     : u64x2{w0, w1};
      }
#pragma unroll
      for (int k = 0; k < RB; ++k) {
        const uint64_t d = ((v[k][0] ^ w0) & m0) | ((v[k][1] ^ w1) & m1);
        const uint64_t bad = __ballot(d != 0ull);  // lanes 0-31: universe 2k, 32-63: 2k+1
        const uint32_t rel = (uint32_t)lane - (uint32_t)(pass * 2 * RB + 2 * k);
        if (rel < 2u) mine = (uint32_t)(bad >> (32 * rel)) == 0u ? 1u : 0u;
      }
    }
    if (lane < UPW && u0 + lane < n) out[u0 + lane] = (uint8_t)mine;
  }
}

// One pass of the whole-board LDS form: the RB universes from ub on (RB * 512
// contiguous bytes; past n, universe n - 1 again: a valid address whose
// answer is never stored) into img by RB / 2 sixteen-byte-per-lane
// global_load_lds (lanes 0-31 one universe, 32-63 the next).
// (step_kernels.hpp step_body_dma and contains_kernels.hpp universes_pf write
// the same fetch out: through this helper their kernels compile to other code,
// profiles/r08/README.md.)
template <int RB>
__device__ __forceinline__ void dma_fetch_pass(const uint64_t *in, uint64_t n, uint64_t ub, int lane, uint64_t *img) {
#pragma unroll
  for (int i = 0; i < RB / 2; ++i) {
    uint64_t u = ub + 2 * i + (lane >> 5);
    if (u >= n) u = n - 1;
    const char *src = reinterpret_cast<const char *>(in + u * kWave) + (lane & 31) * 16;
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                     (__attribute__((address_space(3))) void *)(img + i * 2 * kWave), 16, 0, 2);
  }
}

// The whole-board pass (K = 64) through LDS: each register set is one
// universe, RB sets per pass; the RB universes of a pass (RB * 512
// contiguous bytes) arrive by RB / 2 sixteen-byte-per-lane global_load_lds
// (LDS-DMA, no VGPR destination: lanes 0-31 fill one universe, 32-63 the
// next) and leave by ds_read_b64 with lane = column, and the next pass's are
// fetched as soon as this pass has been read out, so that they stream in
// while this pass steps.  Chunks of 2 RB universes per wave, u_step apart;
// one coalesced store of answers per chunk.  `img`: this wave's RB * 512
// bytes of LDS.  The batch must be 16-byte aligned.
template <int RB, bool FIRST, typename OutT>
__device__ __forceinline__ void cone_wave_full_dma(const uint64_t *in, uint64_t w64, uint64_t m64,
                                                   OutT *__restrict__ out, uint64_t n, uint64_t u_first,
                                                   uint64_t u_step, uint32_t gens, int lane, uint64_t *img,
                                                   bool prefetched) {
  static_assert(RB % 2 == 0 && 2 * RB <= kWave, "passes of pairs of universes, one answer per lane");
  const W tw = split(w64), tm = split(m64);
  auto clean = [&](W s) __attribute__((always_inline)) {
    const uint32_t d = ((s.lo ^ tw.lo) & tm.lo) | ((s.hi ^ tw.hi) & tm.hi);
    return __ballot(d != 0u) == 0ull;
  };
  // pass t: universes [base(t), base(t) + RB); chunk t / 2
  auto base = [&](uint64_t t) { return u_first + (t >> 1) * u_step + (t & 1) * RB; };
  auto fetch = [&](uint64_t ub) __attribute__((always_inline)) { dma_fetch_pass<RB>(in, n, ub, lane, img); };
  if (u_first >= n) return;
  if (!prefetched) fetch(u_first);  // (else the caller issued it)
  uint32_t mine = 0;  // lane L: the answer for universe (chunk start) + L
  int after = 0;      // vector-memory ops issued after the pending fetch (the chunk's answer store)
  for (uint64_t t = 0;; ++t) {
    const uint64_t ub = base(t);
    if (ub >= n) break;
    if (after) __builtin_amdgcn_s_waitcnt(kWaitVm1);
    else __builtin_amdgcn_s_waitcnt(kWaitVm0);
    W a[RB];
#pragma unroll
    for (int k = 0; k < RB; ++k) a[k] = split(img[k * kWave + lane]);
    __builtin_amdgcn_s_waitcnt(kWaitLgkm0);  // read out before the next fetch lands
    const uint64_t nb = base(t + 1);
    if (nb < n) fetch(nb);
    uint32_t res[RB];
    if constexpr (FIRST) {
#pragma unroll
      for (int k = 0; k < RB; ++k) res[k] = 0;
      for (uint32_t g = 1; g <= gens; ++g) {
#pragma unroll
        for (int k = 0; k < RB; ++k) {
          a[k] = life_gen<XDPP, 3>(a[k], nullptr, lane);
          if (res[k] == 0 && clean(a[k])) res[k] = g;
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < RB; ++k) res[k] = clean(a[k]) ? 1u : 0u;
    }
#pragma unroll
    for (int k = 0; k < RB; ++k)
      if ((uint32_t)lane == (uint32_t)((t & 1) * RB + k)) mine = res[k];
    after = 0;
    if ((t & 1) || ub + RB >= n) {  // the chunk's last pass: store its answers
      const uint64_t u0 = base(t & ~1ull);
      if (lane < 2 * RB && u0 + lane < n) out[u0 + lane] = (OutT)mine;
      mine = 0;
      after = 1;
    }
  }
}

// The whole-board pass of the filter (FIRST, gens >= 1) when the target's care
// rows, widened by the light cone, fit FW = 32 / PK rows: rows y0 .. y0 + FW - 1
// of each universe's column are cut out by one v_alignbit (WRAP: the window
// crosses row 63), PK universes share one 32-bit register (v_perm, universe j
// of the word in bits j FW .. j FW + FW - 1), and the generation runs on the
// packed words with 1-bit shifts for the vertical neighbours.  The bits
// shifted in at a field's edges (the next field's, or zero) are wrong, and the
// error moves one row inwards per generation -- never onto a care row, which
// lies at least `gens` rows inside its field (cone_rows).  Columns are whole
// (the DPP rotate is the torus), so the care cells are exact.  Same passes,
// LDS image and answers as cone_wave_full_dma; a universe costs one cut, a
// share of the pack, 1 / PK of the network and its field's test.
template <int RB, int PK, bool WRAP, typename OutT, int SLEEP = 0>
__device__ __forceinline__ void cone_wave_rows_dma(const uint64_t *in, uint64_t w64, uint64_t m64,
                                                   OutT *__restrict__ out, uint64_t n, uint64_t u_first,
                                                   uint64_t u_step, uint32_t gens, uint32_t y0, int lane,
                                                   uint64_t *img, bool prefetched) {
  static_assert(RB % 2 == 0 && RB % PK == 0 && 2 * RB <= kWave, "passes of whole words and pairs of universes");
  static_assert(PK == 1 || PK == 2 || PK == 4, "fields of 32, 16 or 8 rows");
  constexpr int FW = 32 / PK, NW = RB / PK;
  constexpr uint32_t fmask = FW == 32 ? ~0u : (1u << FW) - 1u;
  constexpr uint32_t rep = PK == 1 ? 1u : PK == 2 ? 0x00010001u : 0x01010101u;
  const uint32_t sh = y0 & 31u;
  auto cut = [&](uint64_t v) __attribute__((always_inline)) {
    const W w = split(v);
    return WRAP ? __builtin_amdgcn_alignbit(w.lo, w.hi, sh) : __builtin_amdgcn_alignbit(w.hi, w.lo, sh);
  };
  const uint32_t tw = (cut(w64) & fmask) * rep, tm = (cut(m64) & fmask) * rep;
  constexpr uint32_t kDiff = ((TA ^ TB) & TC) & 0xFF;  // (s ^ wanted) & care
  auto base = [&](uint64_t t) { return u_first + (t >> 1) * u_step + (t & 1) * RB; };
  auto fetch = [&](uint64_t ub) __attribute__((always_inline)) { dma_fetch_pass<RB>(in, n, ub, lane, img); };
  if (u_first >= n) return;
  if (!prefetched) fetch(u_first);  // (else the caller issued it)
  uint32_t mine = 0;  // lane L: the answer for universe (chunk start) + L
  int after = 0;      // vector-memory ops issued after the pending fetch (the chunk's answer store)
  for (uint64_t t = 0;; ++t) {
    const uint64_t ub = base(t);
    if (ub >= n) break;
    if (after) __builtin_amdgcn_s_waitcnt(kWaitVm1);
    else __builtin_amdgcn_s_waitcnt(kWaitVm0);
    uint32_t a[NW];
#pragma unroll
    for (int m = 0; m < NW; ++m) {
      uint32_t e[PK];
#pragma unroll
      for (int j = 0; j < PK; ++j) e[j] = cut(img[(m * PK + j) * kWave + lane]);
      if constexpr (PK == 1) {
        a[m] = e[0];
      } else if constexpr (PK == 2) {
        a[m] = __builtin_amdgcn_perm(e[1], e[0], 0x05040100u);  // low halves: e0 | e1 << 16
      } else {
        const uint32_t p01 = __builtin_amdgcn_perm(e[1], e[0], 0x0C0C0400u);  // e0.b0, e1.b0
        const uint32_t p23 = __builtin_amdgcn_perm(e[3], e[2], 0x0C0C0400u);  // e2.b0, e3.b0
        a[m] = __builtin_amdgcn_perm(p23, p01, 0x05040100u);
      }
    }
    __builtin_amdgcn_s_waitcnt(kWaitLgkm0);  // read out before the next fetch lands
    const uint64_t nb = base(t + 1);
    if (nb < n) fetch(nb);
    if constexpr (SLEEP > 0) __builtin_amdgcn_s_sleep(SLEEP);  // (the tuning build's pacing probe)
    uint32_t res[RB];
#pragma unroll
    for (int k = 0; k < RB; ++k) res[k] = 0;
    for (uint32_t g = 1; g <= gens; ++g) {
#pragma unroll
      for (int m = 0; m < NW; ++m) {
        const uint32_t L = dpp_prev(a[m]), R = dpp_next(a[m]);
        const uint32_t h0 = lut3<kXor3>(L, a[m], R), h1 = lut3<kMaj>(L, a[m], R);
        a[m] = life_tail6(h0 << 1, h0, h0 >> 1, h1 << 1, h1, h1 >> 1, a[m]);
        const uint32_t d = lut3<kDiff>(a[m], tw, tm);
#pragma unroll
        for (int j = 0; j < PK; ++j) {
          const bool clean = __ballot((d & (fmask << (j * FW))) != 0u) == 0ull;
          if (res[m * PK + j] == 0 && clean) res[m * PK + j] = g;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < RB; ++k)
      if ((uint32_t)lane == (uint32_t)((t & 1) * RB + k)) mine = res[k];
    after = 0;
    if ((t & 1) || ub + RB >= n) {  // the chunk's last pass: store its answers
      const uint64_t u0 = base(t & ~1ull);
      if (lane < 2 * RB && u0 + lane < n) out[u0 + lane] = (OutT)mine;
      mine = 0;
      after = 1;
    }
  }
}

}  // namespace
}  // namespace lifeapi_impl
