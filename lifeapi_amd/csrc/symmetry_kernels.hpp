// symmetry_kernels.hpp -- the reference's symmetry layer over a batch:
// Transform / FlipX / FlipY / Transpose / Move (LifeAPI.hpp:682-806,
// Symmetry.hpp:105-173), Symmetricize (Symmetry.hpp:565-654), XYBounds
// (LifeAPI.hpp:446-484) and SymmetryOrbit[Representatives] (Symmetry.hpp:
// 798-830).  symmetry.hip launches them.
//
// Every SymmetryTransform followed by any Move is an affine map of the torus,
// p -> A p + b mod 64 with A in D4.  Read backwards (which cell of the input
// lands on (x, y)), a map that does not exchange the axes is
//   out(x, y) = in(+-x + c, +-y + r)
// and one that does is the plain transpose of such a map:
//   out(x, y) = g(y, x),  g(x, y) = in(+-x + c, +-y + r)
// (a column shift after a transpose is a row rotate before it, so all of the
// translation is applied before).  The host reduces (transform, dx, dy) to
// an Affine: column flip and offset, row flip and rotate, transpose or not.
// With lane = column:
//   columns   lane x takes column (+-x + c) mod 64: a permuted load index in
//             k_transform (still one 512-byte read), one ds_bpermute_b32 per
//             half on registers (k_symmetricize, k_symmetry_orbit)
//   rows      w'(y) = w(+-y + r): v_bfrev_b32 on the exchanged halves, then a
//             wave-uniform rotate (two v_alignbit_b32, the halves renamed for
//             a rotate of 32 or more)
//   transpose the 64 x 64 bit transpose across the wave, six block-swap
//             stages j = 32 .. 1: the bits whose row index and lane index
//             differ in bit j are exchanged with lane ^ j.
//               j = 32  one v_permlane32_swap (vdst = lo, src = hi)
//               j = 16  per half one v_permlane16_swap of the word with its
//                       copy and one v_perm_b32 (a per-lane byte selector)
//               j = 8   row_ror:8;  j = 4  row_half_mirror then quad_perm
//                       [3,2,1,0];  j = 2, 1  quad_perm; each then one
//                       v_alignbit_b32 by a per-lane amount (the partner's
//                       word rotated by -+j) and one v_bitop3_b32 (a select
//                       under a per-lane mask)
//             9 per-lane constants per wave; as compiled about 60 VALU per
//             universe (8 v_alignbit_b32, 8 v_bitop3_b32, 10 DPP moves, 3
//             swaps, 2 v_perm_b32, and the v_mov_b32 copies the swaps and the
//             DPP moves' old values take).
//
// Registers (build/asm, gfx950; .private_segment_fixed_size 0 and no LDS in
// all five; 8 waves per SIMD each):
//   k_transform<false, 4>   24 VGPRs      k_bounds<4>           18 VGPRs
//   k_transform<true, 4>    36 VGPRs      k_symmetry_orbit<2>   37 VGPRs
//   k_symmetricize<4>       36 VGPRs
// Measured on 1M universes (profiles/r12/README.md), as multiples of the
// 1-generation step's time: Identity + move 1.12, FlipX 1.12-1.13, Transpose
// 1.16-1.18, Rotate90 + move 1.19-1.20 (bytes-bound, like Match of a small
// target); Symmetricize C2 1.09, C4 1.28-1.29, D4diag 1.50-1.52 (the second
// and third issue-bound on one and two transposes); XYBounds 0.65-0.67 (the
// read); the orbit's mask alone 2.9-3.0 (issue-bound: about 240 VALU and 350
// SALU per universe), with the images 5.8-5.9 (4.6 KB per universe at 0.66 of
// 8 TB/s).
#pragma once

#include "match_kernels.hpp"

namespace lifeapi_impl {

// out = [transpose of] g, g(x, y) = in((colflip ? -x : x) + coloff,
// (rowflip ? -y : y) + r), with rowrot the right-rotate that does the row
// part after the optional bit reversal: r for rowflip == 0, 63 - r otherwise
struct Affine {
  uint32_t colflip, coloff, rowflip, rowrot, transpose;
};

namespace {

// ---- the descriptors, shared by the host (one offset per launch) and the
// kernels that take an offset per universe ----

// A forward affine map of the torus, (x, y) -> (sx x + bx, sy y + by), or
// with `swap` (sx y + bx, sy x + by): where the cell at (x, y) goes.
struct Forward {
  bool swap;
  int sx, sy;
  long long bx, by;
};

// The 16 SymmetryTransforms in the enum's order (Symmetry.hpp:7-26), read
// off Transform (Symmetry.hpp:105-173): FlipX is (x, -y - 1), FlipY
// (-x - 1, y), Transpose(false) (y, x), Transpose(true) (-y - 1, -x - 1),
// Move(a, b) adds (a, b).
constexpr Forward kTransforms[16] = {
    {false, 1, 1, 0, 0},     // Identity
    {false, 1, -1, 0, -1},   // ReflectAcrossXEven
    {false, 1, -1, 0, 0},    // ReflectAcrossX
    {false, -1, 1, -1, 0},   // ReflectAcrossYEven
    {false, -1, 1, 0, 0},    // ReflectAcrossY
    {true, -1, 1, -1, 0},    // Rotate90Even
    {true, -1, 1, 0, 0},     // Rotate90
    {true, 1, -1, 0, -1},    // Rotate270Even
    {true, 1, -1, 0, 0},     // Rotate270
    {false, -1, -1, 0, 0},   // Rotate180OddBoth
    {false, -1, -1, -1, 0},  // Rotate180EvenHorizontal
    {false, -1, -1, 0, -1},  // Rotate180EvenVertical
    {false, -1, -1, -1, -1}, // Rotate180EvenBoth
    {true, 1, 1, 0, 0},      // ReflectAcrossYeqX
    {true, -1, -1, -1, -1},  // ReflectAcrossYeqNegX
    {true, -1, -1, 0, 0},    // ReflectAcrossYeqNegXP1
};

__host__ __device__ inline Forward moved(Forward f, long long dx, long long dy) {
  f.bx += dx;
  f.by += dy;
  return f;
}

__host__ __device__ inline uint32_t mod64(long long v) { return (uint32_t)(((v % 64) + 64) % 64); }

// The map read backwards, as the kernels apply it:
// out(X, Y) = in(sx (X - bx), sy (Y - by)); with swap out(X, Y) = g(Y, X),
// g(u, v) = in(sy (u - by), sx (v - bx)).
__host__ __device__ inline Affine backwards(const Forward &f) {
  const int cs = f.swap ? f.sy : f.sx, rs = f.swap ? f.sx : f.sy;
  const long long cb = f.swap ? f.by : f.bx, rb = f.swap ? f.bx : f.by;
  Affine a;
  a.colflip = cs < 0;
  a.coloff = mod64(-cs * cb);
  a.rowflip = rs < 0;
  const uint32_t r = mod64(-rs * rb);  // w'(y) = w(+-y + r)
  a.rowrot = a.rowflip ? (63u - r) & 63u : r;
  a.transpose = f.swap;
  return a;
}

// PerpComponent (Symmetry.hpp:540-563) for the two diagonal reflections, in
// the reference's own int arithmetic (truncating / and %): not a function of
// the offset mod 64 alone
__host__ __device__ inline void perp_diag(int ox, int oy, bool negative, int &px, int &py) {
  const int x = (ox + 32) % 64 - 32, y = (oy + 32) % 64 - 32;
  if (negative) {
    px = py = ((x + y + 128) / 2) % 64;
  } else {
    px = ((x - y + 128) / 2) % 64;
    py = ((-x + y + 128) / 2) % 64;
  }
}

// StaticSymmetry values (Symmetry.hpp:57-79) Symmetricize defines
enum : uint32_t { kC1 = 0, kD2AcrossX = 1, kD2AcrossY = 3, kD2negdiagodd = 5, kD2diagodd = 6, kC2 = 7, kC4 = 11,
                  kD4 = 13, kD4diag = 17 };

// Symmetricize(state, symmetry, {dx, dy}) as rounds of acc |= map(acc)
// (Symmetry.hpp:565-654); -1 for a symmetry the reference leaves undefined
__host__ __device__ inline int symmetricize_maps(uint32_t symmetry, int dx, int dy, Forward (&m)[2]) {
  const long long x = dx, y = dy;
  switch (symmetry) {
  case kC1: return 0;
  case kC2:  // FlipX, FlipY, Move(dx + 1, dy + 1)
    m[0] = moved(kTransforms[12], x + 1, y + 1);
    return 1;
  case kC4:  // Rotate90, Move(offset); then FlipX, FlipY, Move(dx - dy + 1, dy + dx + 1)
    m[0] = moved(kTransforms[6], x, y);
    m[1] = moved(kTransforms[12], x - y + 1, y + x + 1);
    return 2;
  case kD2AcrossX:  // FlipX, Move(dx, dy + 1)
    m[0] = moved(kTransforms[1], x, y + 1);
    return 1;
  case kD2AcrossY:  // FlipY, Move(dx + 1, dy)
    m[0] = moved(kTransforms[3], x + 1, y);
    return 1;
  case kD2diagodd:  // ReflectAcrossYeqX, Move(offset)
    m[0] = moved(kTransforms[13], x, y);
    return 1;
  case kD2negdiagodd:  // Transpose(true), Move(dx + 1, dy + 1)
    m[0] = moved(kTransforms[14], x + 1, y + 1);
    return 1;
  case kD4:  // PerpComponent(ReflectAcrossX) = (0, dy), PerpComponent(ReflectAcrossY) = (dx, 0)
    m[0] = moved(kTransforms[1], 0, y + 1);
    m[1] = moved(kTransforms[3], x + 1, 0);
    return 2;
  case kD4diag: {
    int px, py, qx, qy;
    perp_diag(dx, dy, false, px, py);
    perp_diag(dx, dy, true, qx, qy);
    m[0] = moved(kTransforms[13], px, py);
    m[1] = moved(kTransforms[14], (long long)qx + 1, (long long)qy + 1);
    return 2;
  }
  default: return -1;
  }
}

__device__ __forceinline__ int affine_col(int lane, const Affine &a) {
  return ((a.colflip ? -lane : lane) + (int)a.coloff) & (kWave - 1);
}

// the row part of `a` on each of the wave's words (all wave-uniform choices)
template <int U>
__device__ __forceinline__ void affine_rows(W (&w)[U], const Affine &a) {
  if (a.rowflip) {
#pragma unroll
    for (int k = 0; k < U; ++k) w[k] = W{__builtin_bitreverse32(w[k].hi), __builtin_bitreverse32(w[k].lo)};
  }
  if (a.rowrot & 32u) {
#pragma unroll
    for (int k = 0; k < U; ++k) w[k] = W{w[k].hi, w[k].lo};
  }
  const uint32_t s = a.rowrot & 31u;
#pragma unroll
  for (int k = 0; k < U; ++k) w[k] = rotr_lt32(w[k], s);
}

// the lane's constants of the transpose's stages 16 .. 1
struct TransposeLane {
  uint32_t sel16;  // v_perm_b32 selector of stage 16
  uint32_t rot[4], mask[4];  // stages 8, 4, 2, 1: rotate amount, bits taken from the partner
};
__device__ __forceinline__ TransposeLane transpose_lane(int lane) {
  TransposeLane c;
  c.sel16 = (lane & 16) ? 0x07060302u : 0x05040100u;
  constexpr uint32_t kHigh[4] = {0xFF00FF00u, 0xF0F0F0F0u, 0xCCCCCCCCu, 0xAAAAAAAAu};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t j = 8u >> i;
    const bool up = (lane & (int)j) != 0;
    c.rot[i] = up ? j : 32u - j;  // rotr by j, or rotl by j
    c.mask[i] = up ? ~kHigh[i] : kHigh[i];
  }
  return c;
}

constexpr uint32_t kSelect = ((TA & ~TC) | (TB & TC)) & 0xFF;  // c ? b : a, bitwise

// stage 16 on one 32-bit half: after the swap of v with its copy, a holds the
// word of the lane's even row (lane & ~16) and b that of its odd row; the
// even-row lane keeps its low 16 rows and takes the partner's low 16 as its
// high 16, the odd-row lane takes the partner's high 16 as its low 16
__device__ __forceinline__ uint32_t transpose_stage16(uint32_t v, uint32_t sel) {
  const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
  return __builtin_amdgcn_perm(r[1], r[0], sel);
}
template <int I>
__device__ __forceinline__ uint32_t transpose_fetch(uint32_t v) {  // lane ^ (8 >> I)'s v
  if constexpr (I == 0) return dpp_mov<0x128>(v);                  // row_ror:8
  else if constexpr (I == 1) return dpp_mov<0x1B>(dpp_mov<0x141>(v));  // l ^ 7, then l ^ 3
  else if constexpr (I == 2) return dpp_mov<0x4E>(v);              // quad_perm [2,3,0,1]
  else return dpp_mov<0xB1>(v);                                    // quad_perm [1,0,3,2]
}
template <int I>
__device__ __forceinline__ uint32_t transpose_stage(uint32_t v, const TransposeLane &c) {
  const uint32_t p = transpose_fetch<I>(v);
  return lut3<kSelect>(v, __builtin_amdgcn_alignbit(p, p, c.rot[I]), c.mask[I]);
}

// w(x, y) <- w(y, x) over the wave (lane x holds column x)
__device__ __forceinline__ W transpose64(W w, const TransposeLane &c) {
  const auto r = __builtin_amdgcn_permlane32_swap(w.lo, w.hi, false, false);
  uint32_t h[2] = {r[0], r[1]};
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    uint32_t v = transpose_stage16(h[k], c.sel16);
    v = transpose_stage<0>(v, c);
    v = transpose_stage<1>(v, c);
    v = transpose_stage<2>(v, c);
    h[k] = transpose_stage<3>(v, c);
  }
  return W{h[0], h[1]};
}

// `a` applied to registers: the columns by ds_bpermute, then the rows, then
// the transpose
template <int U>
__device__ __forceinline__ void affine_apply(W (&t)[U], const W (&s)[U], const Affine &a, int lane,
                                             const TransposeLane &c) {
  const int at = affine_col(lane, a) << 2;
#pragma unroll
  for (int k = 0; k < U; ++k)
    t[k] = W{(uint32_t)__builtin_amdgcn_ds_bpermute(at, (int)s[k].lo),
             (uint32_t)__builtin_amdgcn_ds_bpermute(at, (int)s[k].hi)};
  affine_rows<U>(t, a);
  if (a.transpose) {
#pragma unroll
    for (int k = 0; k < U; ++k) t[k] = transpose64(t[k], c);
  }
}

// out[u] = `a` of in[u].  in == out is allowed: a wave loads its universes
// whole before it stores them and touches no other's.
template <bool TRANSPOSE, int U>
__global__ __launch_bounds__(kBlock) void k_transform(const uint64_t *in, uint64_t *out, Affine a, uint64_t n) {
  const int lane = wave_lane(), wib = wave_in_block();
  const int col = affine_col(lane, a);
  TransposeLane c;
  if constexpr (TRANSPOSE) c = transpose_lane(lane);
  const WaveGroups at = wave_groups<U>(wib, n);
  for (uint64_t g = at.first; g < at.groups; g += at.stride) {
    const uint64_t u0 = g * U;
    W s[U];
    // (spelled out: through load_object the listing of k_transform<false> changes)
#pragma unroll
    for (int k = 0; k < U; ++k) s[k] = u0 + k < n ? ld<true>(in + (u0 + k) * kWave + col) : W{0u, 0u};
    affine_rows<U>(s, a);
    if constexpr (TRANSPOSE) {
#pragma unroll
      for (int k = 0; k < U; ++k) s[k] = transpose64(s[k], c);
    }
#pragma unroll
    for (int k = 0; k < U; ++k) store_object(out, u0 + k, n, lane, s[k]);
  }
}

// out[u] = in[u] after `rounds` (0..2) rounds of acc |= a[round](acc)
// (Symmetry.hpp:565-654); in == out allowed as above
struct Affine2 {
  Affine a[2];
};
template <int U>
__global__ __launch_bounds__(kBlock) void k_symmetricize(const uint64_t *in, uint64_t *out, Affine2 maps,
                                                         uint32_t rounds, uint64_t n) {
  const int lane = wave_lane(), wib = wave_in_block();
  const TransposeLane c = transpose_lane(lane);
  const WaveGroups at = wave_groups<U>(wib, n);
  for (uint64_t g = at.first; g < at.groups; g += at.stride) {
    const uint64_t u0 = g * U;
    W acc[U];
#pragma unroll
    for (int k = 0; k < U; ++k) acc[k] = load_object(in, u0 + k, n, lane);
#pragma unroll
    for (int r = 0; r < 2; ++r)
      if ((uint32_t)r < rounds) {
        W t[U];
        affine_apply<U>(t, acc, maps.a[r], lane, c);
#pragma unroll
        for (int k = 0; k < U; ++k) acc[k] = W{acc[k].lo | t[k].lo, acc[k].hi | t[k].hi};
      }
#pragma unroll
    for (int k = 0; k < U; ++k) store_object(out, u0 + k, n, lane, acc[k]);
  }
}

// ---- an offset per universe ----
// offsets: n x {dx, dy} int32.  Lanes 0 .. 2U-1 load the wave's 2U words with
// one vector load; each universe's two come back wave-uniform by v_readlane,
// and the wave builds that universe's Affine on the scalar unit from the same
// descriptor code the host runs for the single-offset kernels.
template <int U>
__device__ __forceinline__ int load_offsets(const int32_t *__restrict__ offsets, uint64_t u0, uint64_t n, int lane) {
  return lane < 2 * U && u0 * 2 + (uint64_t)lane < n * 2 ? offsets[u0 * 2 + lane] : 0;
}
__device__ __forceinline__ int offset_word(int o, int i) { return __builtin_amdgcn_readlane(o, i); }

// out[u] = in[u].Transformed(t).Moved(offsets[u]), `base` the Forward of t:
// k_transform with the permuted load index and the row rotate per universe
template <bool TRANSPOSE, int U>
__global__ __launch_bounds__(kBlock) void k_transform_offsets(const uint64_t *in, uint64_t *out, Forward base,
                                                              const int32_t *__restrict__ offsets, uint64_t n) {
  const int lane = wave_lane(), wib = wave_in_block();
  TransposeLane c;
  if constexpr (TRANSPOSE) c = transpose_lane(lane);
  const WaveGroups at = wave_groups<U>(wib, n);
  for (uint64_t g = at.first; g < at.groups; g += at.stride) {
    const uint64_t u0 = g * U;
    const int o = load_offsets<U>(offsets, u0, n, lane);
    Affine a[U];
    W s[U];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      a[k] = backwards(moved(base, offset_word(o, 2 * k), offset_word(o, 2 * k + 1)));
      s[k] = load_object(in, u0 + k, n, affine_col(lane, a[k]));
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
      W one[1] = {s[k]};
      affine_rows<1>(one, a[k]);
      s[k] = one[0];
      if constexpr (TRANSPOSE) s[k] = transpose64(s[k], c);
    }
#pragma unroll
    for (int k = 0; k < U; ++k) store_object(out, u0 + k, n, lane, s[k]);
  }
}

// out[u] = Symmetricize(in[u], symmetry, offsets[u]): k_symmetricize with the
// maps of each universe built by the wave.  symmetry is one the host has
// found defined (symmetricize_maps >= 0).
template <int U>
__global__ __launch_bounds__(kBlock) void k_symmetricize_offsets(const uint64_t *in, uint64_t *out,
                                                                 uint32_t symmetry,
                                                                 const int32_t *__restrict__ offsets, uint64_t n) {
  const int lane = wave_lane(), wib = wave_in_block();
  const TransposeLane c = transpose_lane(lane);
  const WaveGroups at = wave_groups<U>(wib, n);
  for (uint64_t g = at.first; g < at.groups; g += at.stride) {
    const uint64_t u0 = g * U;
    const int o = load_offsets<U>(offsets, u0, n, lane);
    W acc[U];
#pragma unroll
    for (int k = 0; k < U; ++k) acc[k] = load_object(in, u0 + k, n, lane);
    // one universe after another, its maps built just before they are applied
    // (building all U universes' maps first and applying each round stage by
    // stage across them was measured slower: 100 SGPRs, 7 waves per SIMD,
    // +8 to 10 % on C2, C4 and D4diag, profiles/r18/README.md)
#pragma unroll
    for (int k = 0; k < U; ++k) {
      Forward m[2] = {kTransforms[0], kTransforms[0]};
      const int rounds = symmetricize_maps(symmetry, offset_word(o, 2 * k), offset_word(o, 2 * k + 1), m);
#pragma unroll
      for (int r = 0; r < 2; ++r)
        if (r < rounds) {
          W one[1] = {acc[k]}, t[1];
          affine_apply<1>(t, one, backwards(m[r]), lane, c);
          acc[k] = W{acc[k].lo | t[0].lo, acc[k].hi | t[0].hi};
        }
    }
#pragma unroll
    for (int k = 0; k < U; ++k) store_object(out, u0 + k, n, lane, acc[k]);
  }
}

// XYBounds (LifeAPI.hpp:446-484) from the populated-columns mask and the OR
// of the columns, both wave-uniform: the margins of each rotated by 32.  An
// empty state gives -1 four times.
struct Bounds {
  int left, top, right, bottom;
};
__device__ __forceinline__ Bounds bounds_of(uint64_t cols, uint64_t rows) {
  if (rows == 0) return Bounds{-1, -1, -1, -1};
  const uint64_t c = rotr64(cols, 32), r = rotr64(rows, 32);
  return Bounds{__builtin_ctzll(c) - 32, __builtin_ctzll(r) - 32, 31 - __builtin_clzll(c), 31 - __builtin_clzll(r)};
}
__device__ __forceinline__ uint64_t wave_or_u64_dpp(W v) {
  return (uint64_t)wave_or_u32_dpp(v.lo) | (uint64_t)wave_or_u32_dpp(v.hi) << 32;
}

// bounds[4u .. 4u+3] = states[u].XYBounds(): U universes per wave, whose 4U
// numbers lanes 0 .. 4U-1 store with one vector store
template <int U>
__global__ __launch_bounds__(kBlock) void k_bounds(const uint64_t *__restrict__ in, int32_t *__restrict__ bounds,
                                                   uint64_t n) {
  const int lane = wave_lane(), wib = wave_in_block();
  const WaveGroups at = wave_groups<U>(wib, n);
  for (uint64_t g = at.first; g < at.groups; g += at.stride) {
    const uint64_t u0 = g * U;
    W s[U];
#pragma unroll
    for (int k = 0; k < U; ++k) s[k] = load_object(in, u0 + k, n, lane);
    int h = 0;
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const Bounds b = bounds_of(__ballot((s[k].lo | s[k].hi) != 0u), wave_or_u64_dpp(s[k]));
      h = lane == 4 * k ? b.left : lane == 4 * k + 1 ? b.top : lane == 4 * k + 2 ? b.right : lane == 4 * k + 3 ? b.bottom : h;
    }
    if (holds_scalar<U, 4>(u0, n, lane)) bounds[u0 * 4 + lane] = h;
  }
}

// m(-i) for a 64-bit mask: the populated columns (rows) of a column (row)
// negation
__device__ __forceinline__ uint64_t negate_mask(uint64_t m) {
  const uint64_t r = __builtin_bitreverse64(m);
  return r << 1 | r >> 63;
}

// SymmetryOrbit / SymmetryOrbitRepresentatives (Symmetry.hpp:798-830).  The
// eight transforms in the reference's order are all linear (no translation):
//   0 Identity (x, y)          4 ReflectAcrossYeqNegXP1 (-y, -x)
//   1 ReflectAcrossX (x, -y)   5 Rotate90 (-y, x)
//   2 ReflectAcrossYeqX (y, x) 6 Rotate270 (y, -x)
//   3 ReflectAcrossY (-x, y)   7 Rotate180OddBoth (-x, -y)
// so image i is the state s (i = 0, 1, 3, 7) or its transpose t (one
// transpose for the four) with its columns and / or rows negated.  An
// image's bounds follow from the state's populated columns and rows alone
// (the transpose exchanges the two masks, a negation is negate_mask), on the
// scalar unit; the move by minus (left, top) then joins the negation in one
// Affine per image: the column part one ds_bpermute per half, the row part a
// rotate.  Image i is a representative iff it equals no image j < i.
template <int U>
__global__ __launch_bounds__(kBlock) void k_symmetry_orbit(const uint64_t *__restrict__ in,
                                                           uint64_t *__restrict__ images,
                                                           uint8_t *__restrict__ first, uint64_t n) {
  // of image i: taken from the transpose; columns negated; rows negated
  constexpr bool kT[8] = {false, false, true, false, true, true, true, false};
  constexpr bool kNegCol[8] = {false, false, false, true, true, true, false, true};
  constexpr bool kNegRow[8] = {false, true, false, false, true, false, true, true};
  const int lane = wave_lane(), wib = wave_in_block();
  const TransposeLane c = transpose_lane(lane);
  const WaveGroups at = wave_groups<U>(wib, n);
  for (uint64_t g = at.first; g < at.groups; g += at.stride) {
    const uint64_t u0 = g * U;
    W s[U];
#pragma unroll
    for (int k = 0; k < U; ++k) s[k] = load_object(in, u0 + k, n, lane);
    uint32_t h = 0;
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const uint64_t cols = __ballot((s[k].lo | s[k].hi) != 0u), rows = wave_or_u64_dpp(s[k]);
      const W base[2] = {s[k], transpose64(s[k], c)};
      W img[8];
      uint32_t mask = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const uint64_t bc = kT[i] ? rows : cols, br = kT[i] ? cols : rows;
        const Bounds b = bounds_of(kNegCol[i] ? negate_mask(bc) : bc, kNegRow[i] ? negate_mask(br) : br);
        // image(x, y) = base(+-(x + left), +-(y + top))
        Affine a;
        a.colflip = kNegCol[i];
        a.coloff = (uint32_t)(kNegCol[i] ? -b.left : b.left) & 63u;
        a.rowflip = kNegRow[i];
        a.rowrot = (uint32_t)(kNegRow[i] ? 63 + b.top : b.top) & 63u;
        a.transpose = 0;
        W one[1] = {base[kT[i]]}, got[1];
        affine_apply<1>(got, one, a, lane, c);
        img[i] = got[0];
        bool seen = false;
#pragma unroll
        for (int j = 0; j < i; ++j)
          seen = seen || __ballot(((img[i].lo ^ img[j].lo) | (img[i].hi ^ img[j].hi)) != 0u) == 0ull;
        mask |= seen ? 0u : 1u << i;
        // (this guard and the one on `first` spelled out: through store_object
        // and holds_scalar this kernel's listing changes)
        if (images && u0 + k < n) st<true>(images + ((u0 + k) * 8 + i) * kWave + lane, img[i]);
      }
      h = lane == k ? mask : h;
    }
    if (first && lane < U && u0 + (uint64_t)lane < n) first[u0 + lane] = (uint8_t)h;
  }
}

}  // namespace
}  // namespace lifeapi_impl
