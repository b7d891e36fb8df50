// lifeapi/LifeState.hpp -- standalone, source-compatible subset of the
// reference's LifeState / LifeTarget (scorbiclife/LifeAPI, LifeAPI.hpp,
// LifeTarget.hpp) covering the Step() hot path, plus the batched GPU entry
// points in lifeapi/batch.hpp.
//
// Same layout (uint64_t state[64], aligned(64); word x = column x, bit y =
// row y: LifeAPI.hpp:39-40,131) and the same member names and semantics for
// the hot path, so loops written against the reference recompile against
// lifeapi::LifeState unchanged.  Single-universe Step() runs on the CPU (a
// ~50 ns operation cannot amortise a GPU launch); batches go to the GPU via
// lifeapi::StepBatch.  Code that keeps the reference's own LifeAPI.hpp can
// use lifeapi/batch.hpp directly on ::LifeState instead of this header.
#pragma once

#include <array>
#include <bit>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace lifeapi {

inline constexpr int N = 64;  // LifeAPI.hpp:12

constexpr unsigned torus_wrap(int x) { return unsigned(x) & (N - 1); }  // LifeAPI.hpp:14-16

enum class InitializedTag { UNINITIALIZED };  // LifeAPI.hpp:37

// Symmetry.hpp:7-26.  Each is an affine map of the torus; the "Even" forms
// reflect about a line between cells, the others fix (0, 0):
//   Identity (x, y)                  Rotate180OddBoth        (-x, -y)
//   ReflectAcrossXEven (x, -y-1)     Rotate180EvenHorizontal (-x-1, -y)
//   ReflectAcrossX     (x, -y)       Rotate180EvenVertical   (-x, -y-1)
//   ReflectAcrossYEven (-x-1, y)     Rotate180EvenBoth       (-x-1, -y-1)
//   ReflectAcrossY     (-x, y)       ReflectAcrossYeqX       (y, x)
//   Rotate90Even  (-y-1, x)          ReflectAcrossYeqNegX    (-y-1, -x-1)
//   Rotate90      (-y, x)            ReflectAcrossYeqNegXP1  (-y, -x)
//   Rotate270Even (y, -x-1)          Rotate270               (y, -x)
enum struct SymmetryTransform : uint32_t {
  Identity,
  ReflectAcrossXEven,
  ReflectAcrossX,
  ReflectAcrossYEven,
  ReflectAcrossY,
  Rotate90Even,
  Rotate90,
  Rotate270Even,
  Rotate270,
  Rotate180OddBoth,
  Rotate180EvenHorizontal,
  Rotate180EvenVertical,
  Rotate180EvenBoth,
  ReflectAcrossYeqX,
  ReflectAcrossYeqNegX,
  ReflectAcrossYeqNegXP1
};

// Symmetry.hpp:47-55: the two pairs of quarter turns; every other transform
// is its own inverse
inline SymmetryTransform TransformInverse(SymmetryTransform t) {
  switch (t) {
  case SymmetryTransform::Rotate90Even: return SymmetryTransform::Rotate270Even;
  case SymmetryTransform::Rotate90: return SymmetryTransform::Rotate270;
  case SymmetryTransform::Rotate270Even: return SymmetryTransform::Rotate90Even;
  case SymmetryTransform::Rotate270: return SymmetryTransform::Rotate90;
  default: return t;
  }
}

// Symmetry.hpp:57-79
enum struct StaticSymmetry : uint32_t {
  C1,
  D2AcrossX,
  D2AcrossXEven,
  D2AcrossY,
  D2AcrossYEven,
  D2negdiagodd,
  D2diagodd,
  C2,
  C2even,
  C2verticaleven,
  C2horizontaleven,
  C4,
  C4even,
  D4,
  D4even,
  D4verticaleven,
  D4horizontaleven,
  D4diag,
  D4diageven,
  D8,
  D8even,
};

struct alignas(64) LifeState {
  uint64_t state[N];

  constexpr LifeState() : state{} {}
  explicit constexpr LifeState(InitializedTag) {}

  // ---- access (LifeAPI.hpp:131-146)
  void Set(unsigned x, unsigned y) { state[x] |= uint64_t(1) << y; }
  void Erase(unsigned x, unsigned y) { state[x] &= ~(uint64_t(1) << y); }
  void Set(unsigned x, unsigned y, bool v) { v ? Set(x, y) : Erase(x, y); }
  bool Get(unsigned x, unsigned y) const { return (state[x] >> y) & 1; }
  void SetSafe(int x, int y, bool v) { Set(torus_wrap(x), torus_wrap(y), v); }
  bool GetSafe(int x, int y) const { return Get(torus_wrap(x), torus_wrap(y)); }
  void Set(std::pair<int, int> c) { Set(c.first, c.second); }
  bool Get(std::pair<int, int> c) const { return Get(c.first, c.second); }
  constexpr uint64_t &operator[](unsigned i) { return state[i]; }
  constexpr uint64_t operator[](unsigned i) const { return state[i]; }

  static LifeState Cell(std::pair<int, int> c) {
    LifeState r;
    r.Set(c.first, c.second);
    return r;
  }

  // ---- value semantics (LifeAPI.hpp:213-275)
  bool operator==(const LifeState &o) const {
    uint64_t d = 0;
    for (int i = 0; i < N; ++i) d |= state[i] ^ o.state[i];
    return d == 0;
  }
  bool operator!=(const LifeState &o) const { return !(*this == o); }
#define LIFEAPI_BINOP(op)                                                   \
  LifeState operator op(const LifeState &o) const {                         \
    LifeState r(InitializedTag::UNINITIALIZED);                             \
    for (int i = 0; i < N; ++i) r.state[i] = state[i] op o.state[i];        \
    return r;                                                               \
  }                                                                         \
  LifeState &operator op##=(const LifeState &o) {                           \
    for (int i = 0; i < N; ++i) state[i] = state[i] op o.state[i];          \
    return *this;                                                           \
  }
  LIFEAPI_BINOP(&)
  LIFEAPI_BINOP(|)
  LIFEAPI_BINOP(^)
#undef LIFEAPI_BINOP
  LifeState operator~() const {
    LifeState r(InitializedTag::UNINITIALIZED);
    for (int i = 0; i < N; ++i) r.state[i] = ~state[i];
    return r;
  }

  // ---- queries (LifeAPI.hpp:281-298)
  bool IsEmpty() const {
    uint64_t a = 0;
    for (int i = 0; i < N; ++i) a |= state[i];
    return a == 0;
  }
  unsigned GetPop() const {
    unsigned p = 0;
    for (int i = 0; i < N; ++i) p += std::popcount(state[i]);
    return p;
  }
  bool Contains(const LifeState &pat) const {  // LifeAPI.hpp:388-397
    uint64_t d = 0;
    for (int i = 0; i < N; ++i) d |= (state[i] & pat[i]) ^ pat[i];
    return d == 0;
  }
  bool AreDisjoint(const LifeState &pat) const {  // LifeAPI.hpp:377-386
    uint64_t d = 0;
    for (int i = 0; i < N; ++i) d |= state[i] & pat[i];
    return d == 0;
  }
  // the offset forms (LifeAPI.hpp:399-421): target column i against state
  // column i + dx rotated right by dy
  bool Contains(const LifeState &pat, int dx, int dy) const {
    const int y = int(torus_wrap(dy));
    for (int i = 0; i < N; ++i)
      if ((std::rotr(state[torus_wrap(i + dx)], y) & pat[i]) != pat[i]) return false;
    return true;
  }
  bool AreDisjoint(const LifeState &pat, int dx, int dy) const {
    const int y = int(torus_wrap(dy));
    for (int i = 0; i < N; ++i)
      if ((std::rotr(state[torus_wrap(i + dx)], y) & pat[i]) != 0) return false;
    return true;
  }
  inline bool Contains(const struct LifeTarget &t) const;
  inline bool Contains(const struct LifeTarget &t, int dx, int dy) const;

  // ---- ZOI (LifeAPI.hpp:521-538): the 3x3 dilation on the torus, and the
  // cells next to the pattern but not in it
  LifeState ZOI() const {
    LifeState v(InitializedTag::UNINITIALIZED), r(InitializedTag::UNINITIALIZED);
    for (int i = 0; i < N; ++i) v.state[i] = state[i] | std::rotl(state[i], 1) | std::rotr(state[i], 1);
    for (int i = 0; i < N; ++i)
      r.state[i] = v.state[(i + N - 1) & (N - 1)] | v.state[i] | v.state[(i + 1) & (N - 1)];
    return r;
  }
  LifeState GetBoundary() const { return ZOI() & ~*this; }

  // ---- Move / Moved (LifeAPI.hpp:682-735): cell (x, y) -> (x + dx, y + dy) on the torus
  void Move(int dx, int dy) { *this = Moved(dx, dy); }
  void Move(std::pair<int, int> v) { Move(v.first, v.second); }
  LifeState Moved(int dx, int dy) const {
    LifeState r(InitializedTag::UNINITIALIZED);
    const int y = int(torus_wrap(dy));
    for (int i = 0; i < N; ++i) r.state[torus_wrap(i + dx)] = std::rotl(state[i], y);
    return r;
  }
  LifeState Moved(std::pair<int, int> v) const { return Moved(v.first, v.second); }

  // ---- the symmetry layer (LifeAPI.hpp:446-484,754-806, Symmetry.hpp:105-173,
  // 798-830), CPU, single universe; batches go to the GPU via
  // lifeapi::TransformBatch / SymmetricizeBatch / XYBoundsBatch /
  // SymmetryOrbitBatch.
  // FlipY: cell (x, y) -> (-x - 1, y); FlipX = BitReverse: (x, y) -> (x, -y - 1)
  void FlipY() {
    for (int i = 0; i < N / 2; ++i) std::swap(state[i], state[N - 1 - i]);
  }
  void BitReverse() {
    for (int i = 0; i < N; ++i) {
      uint64_t v = state[i];
      v = (v >> 1 & 0x5555555555555555ULL) | (v & 0x5555555555555555ULL) << 1;
      v = (v >> 2 & 0x3333333333333333ULL) | (v & 0x3333333333333333ULL) << 2;
      v = (v >> 4 & 0x0F0F0F0F0F0F0F0FULL) | (v & 0x0F0F0F0F0F0F0F0FULL) << 4;
      v = (v >> 8 & 0x00FF00FF00FF00FFULL) | (v & 0x00FF00FF00FF00FFULL) << 8;
      v = (v >> 16 & 0x0000FFFF0000FFFFULL) | (v & 0x0000FFFF0000FFFFULL) << 16;
      state[i] = v >> 32 | v << 32;
    }
  }
  void FlipX() { BitReverse(); }
  // Transpose(false): (x, y) -> (y, x), six rounds of block exchanges (rows
  // with bit j set of column k against rows with bit j clear of column k | j);
  // Transpose(true): (x, y) -> (-y - 1, -x - 1), the same between flips
  void Transpose(bool whichDiagonal) {
    uint64_t m = 0x00000000FFFFFFFFULL;
    for (int j = N / 2; j; j >>= 1, m ^= m << j)
      for (int k = 0; k < N; ++k)
        if (!(k & j)) {
          const uint64_t t = ((state[k] >> j) ^ state[k | j]) & m;
          state[k] ^= t << j;
          state[k | j] ^= t;
        }
    if (whichDiagonal) {
      FlipX();
      FlipY();
    }
  }
  void Transpose() { Transpose(true); }
  void Transform(SymmetryTransform t) {
    using enum SymmetryTransform;
    const bool flipx = t == ReflectAcrossXEven || t == ReflectAcrossX || t == Rotate90Even || t == Rotate90 ||
                       (t >= Rotate180OddBoth && t <= Rotate180EvenBoth);
    const bool flipy = t == ReflectAcrossYEven || t == ReflectAcrossY || t == Rotate270Even || t == Rotate270 ||
                       (t >= Rotate180OddBoth && t <= Rotate180EvenBoth);
    if (flipx) FlipX();
    if (flipy) FlipY();
    if (t >= Rotate90Even && t <= Rotate270) Transpose(false);
    if (t == ReflectAcrossYeqX) Transpose(false);
    if (t == ReflectAcrossYeqNegX || t == ReflectAcrossYeqNegXP1) Transpose(true);
    const bool right = t == ReflectAcrossY || t == Rotate90 || t == Rotate180OddBoth || t == Rotate180EvenVertical ||
                       t == ReflectAcrossYeqNegXP1;
    const bool down = t == ReflectAcrossX || t == Rotate270 || t == Rotate180OddBoth ||
                      t == Rotate180EvenHorizontal || t == ReflectAcrossYeqNegXP1;
    if (right || down) Move(right, down);
  }
  LifeState Transformed(SymmetryTransform t) const {
    LifeState r = *this;
    r.Transform(t);
    return r;
  }
  // (LifeAPI.hpp:803-806: the move comes first)
  void Transform(int dx, int dy, SymmetryTransform t) {
    Move(dx, dy);
    Transform(t);
  }
  // {left, top, right, bottom} in the window of columns and rows -32 .. 31
  // (LifeAPI.hpp:446-484); an empty state gives -1 four times.  A pattern
  // straddling the window's edge is reported as the reference reports it.
  std::array<int, 4> XYBounds() const {
    uint64_t cols = 0, rows = 0;
    for (int i = 0; i < N; ++i) {
      cols |= uint64_t(state[i] != 0) << i;
      rows |= state[i];
    }
    if (rows == 0) return {-1, -1, -1, -1};
    cols = std::rotr(cols, 32);
    rows = std::rotr(rows, 32);
    return {std::countr_zero(cols) - 32, std::countr_zero(rows) - 32, 31 - std::countl_zero(cols),
            31 - std::countl_zero(rows)};
  }
  inline std::vector<LifeState> SymmetryOrbit() const;
  inline std::vector<SymmetryTransform> SymmetryOrbitRepresentatives() const;

  // ---- the per-offset questions, CPU, single universe; batches go to the
  // GPU via lifeapi::MatchBatch / ConvolveBatch / InteractionOffsetsBatch.
  // With s(x, y) = bit y of column x and indices mod 64:
  // Mirrored() (LifeAPI.hpp:789-795): cell (x, y) -> (-x, -y)
  LifeState Mirrored() const {
    LifeState r(InitializedTag::UNINITIALIZED);
    for (int i = 0; i < N; ++i) {
      uint64_t v = state[i];  // bit y -> bit 63 - y, then up one row: -y
      v = (v >> 1 & 0x5555555555555555ULL) | (v & 0x5555555555555555ULL) << 1;
      v = (v >> 2 & 0x3333333333333333ULL) | (v & 0x3333333333333333ULL) << 2;
      v = (v >> 4 & 0x0F0F0F0F0F0F0F0FULL) | (v & 0x0F0F0F0F0F0F0F0FULL) << 4;
      v = (v >> 8 & 0x00FF00FF00FF00FFULL) | (v & 0x00FF00FF00FF00FFULL) << 8;
      v = (v >> 16 & 0x0000FFFF0000FFFFULL) | (v & 0x0000FFFF0000FFFFULL) << 16;
      r.state[torus_wrap(-i)] = std::rotl(v >> 32 | v << 32, 1);
    }
    return r;
  }
  // Convolve (LifeAPI.hpp:1293-1370): the torus Minkowski sum,
  // result(x, y) = OR over (a, b) in other of s(x - a, y - b); time
  // proportional to other's population
  LifeState Convolve(const LifeState &other) const {
    LifeState r;
    for (int a = 0; a < N; ++a)
      for (uint64_t w = other.state[a]; w; w &= w - 1) {
        const int b = std::countr_zero(w);
        for (int i = 0; i < N; ++i) r.state[(i + a) & (N - 1)] |= std::rotl(state[i], b);
      }
    return r;
  }
  // ---- doubled coordinates to offsets (Symmetry.hpp:681-727), CPU, single
  // universe; batches go to the GPU via lifeapi::HalveBatch / SkewBatch.
  // Halve: cell (2x, 2y) -> (x, y), the 32 x 32 result repeated in all four
  // quarters; HalveX / HalveY halve one axis.  Cells at odd coordinates vanish.
  static uint64_t EvenRows(uint64_t v) {  // bit 2y -> bit y, then the 32 bits twice
    v &= 0x5555555555555555ULL;
    v = (v | v >> 1) & 0x3333333333333333ULL;
    v = (v | v >> 2) & 0x0F0F0F0F0F0F0F0FULL;
    v = (v | v >> 4) & 0x00FF00FF00FF00FFULL;
    v = (v | v >> 8) & 0x0000FFFF0000FFFFULL;
    v = (v | v >> 16) & 0x00000000FFFFFFFFULL;
    return v | v << 32;
  }
  LifeState Halve() const {
    LifeState r(InitializedTag::UNINITIALIZED);
    for (int i = 0; i < N / 2; ++i) r.state[i] = r.state[i + N / 2] = EvenRows(state[2 * i]);
    return r;
  }
  LifeState HalveX() const {
    LifeState r(InitializedTag::UNINITIALIZED);
    for (int i = 0; i < N / 2; ++i) r.state[i] = r.state[i + N / 2] = state[2 * i];
    return r;
  }
  LifeState HalveY() const {
    LifeState r(InitializedTag::UNINITIALIZED);
    for (int i = 0; i < N; ++i) r.state[i] = EvenRows(state[i]);
    return r;
  }
  // Skew: (x, y) -> (x, y + x); InvSkew: (x, y) -> (x, y - x)
  LifeState Skew() const {
    LifeState r(InitializedTag::UNINITIALIZED);
    for (int i = 0; i < N; ++i) r.state[i] = std::rotl(state[i], i);
    return r;
  }
  LifeState InvSkew() const {
    LifeState r(InitializedTag::UNINITIALIZED);
    for (int i = 0; i < N; ++i) r.state[i] = std::rotr(state[i], i);
    return r;
  }
  // ---- connected components, CPU, single universe; batches go to the GPU
  // via lifeapi::FirstOn / ComponentContaining / ComponentCounts / Components.
  // FirstOn (LifeAPI.hpp:301-323): the LAST group of four columns that is not
  // empty, in it the lowest non-empty column, in that column the lowest set
  // row; (-1, -1) for the empty state
  std::pair<int, int> FirstOn() const {
    int quad = 0;
    for (int x = 0; x < N; x += 4)
      if (state[x] | state[x + 1] | state[x + 2] | state[x + 3]) quad = x;
    for (int x = quad; x < quad + 4; ++x)
      if (state[x]) return {x, std::countr_zero(state[x])};
    return {-1, -1};
  }
  // FirstCell (LifeAPI.hpp:358); the empty state for the empty state, where the
  // reference sets cell (-1, -1) of nothing
  LifeState FirstCell() const {
    const std::pair<int, int> c = FirstOn();
    return c.first < 0 ? LifeState() : Cell(c);
  }
  // the reference's default corona, b3o$5o$5o$5o$b3o! at (-2, -2)
  // (LifeAPI.hpp:1185-1186): the 21 cells with |a|, |b| <= 2 and |a| + |b| < 4
  static LifeState DefaultCorona() {
    LifeState c;
    for (int a = -2; a <= 2; ++a)
      for (int b = -2; b <= 2; ++b)
        if ((a < 0 ? -a : a) + (b < 0 ? -b : b) < 4) c.SetSafe(a, b, true);
    return c;
  }
  // ComponentContaining (LifeAPI.hpp:655-665, 1184-1188): with
  // N(t) = t.Convolve(corona) & *this, the least R with R = N(seed) | N(R)
  LifeState ComponentContaining(const LifeState &seed, const LifeState &corona) const {
    LifeState result, tocheck = seed;
    while (!tocheck.IsEmpty()) {
      const LifeState neighbours = tocheck.Convolve(corona) & *this;
      tocheck = neighbours & ~result;
      result |= neighbours;
    }
    return result;
  }
  LifeState ComponentContaining(const LifeState &seed) const { return ComponentContaining(seed, DefaultCorona()); }
  // Components (LifeAPI.hpp:667-676, 1189-1193), in FirstCell's order.  The
  // reference does not terminate on a corona without cell (0, 0) (the seed's
  // component is empty, nothing is ever removed); this throws instead.
  std::vector<LifeState> Components(const LifeState &corona) const {
    if (!corona.Get(0, 0)) throw std::invalid_argument("lifeapi: Components needs a corona containing cell (0, 0)");
    std::vector<LifeState> result;
    LifeState remaining = *this;
    while (!remaining.IsEmpty()) {
      const LifeState component = remaining.ComponentContaining(remaining.FirstCell(), corona);
      result.push_back(component);
      remaining &= ~component;
    }
    return result;
  }
  std::vector<LifeState> Components() const { return Components(DefaultCorona()); }

  // MatchLive / MatchLiveAndDead (LifeAPI.hpp:427-435): result(x, y) = every
  // cell (a, b) of live has s(x + a, y + b) = 1 [and every cell of dead has
  // s(x + a, y + b) = 0]; an empty pattern is vacuously satisfied
  LifeState MatchLive(const LifeState &live) const { return MatchLiveAndDead(live, LifeState()); }
  LifeState MatchLiveAndDead(const LifeState &live, const LifeState &dead) const {
    LifeState all = ~LifeState(), any;
    for (int a = 0; a < N; ++a) {
      for (uint64_t w = live.state[a]; w; w &= w - 1)
        for (int x = 0; x < N; ++x) all.state[x] &= std::rotr(state[(x + a) & (N - 1)], std::countr_zero(w));
      for (uint64_t w = dead.state[a]; w; w &= w - 1)
        for (int x = 0; x < N; ++x) any.state[x] |= std::rotr(state[(x + a) & (N - 1)], std::countr_zero(w));
    }
    return all & ~any;
  }
  // Match (LifeAPI.hpp:440-442): the pattern with its boundary dead
  LifeState Match(const LifeState &live) const { return MatchLiveAndDead(live, live.GetBoundary()); }
  inline LifeState Match(const struct LifeTarget &t) const;            // LifeTarget.hpp:53-55
  inline LifeState InteractionOffsets(const LifeState &other) const;   // LifeAPI.hpp:1066-1095

  // ---- bitsliced adders (LifeAPI.hpp:822-833)
  static void HalfAdd(uint64_t &out0, uint64_t &out1, uint64_t a, uint64_t b) {
    out0 = a ^ b;
    out1 = a & b;
  }
  static void FullAdd(uint64_t &out0, uint64_t &out1, uint64_t a, uint64_t b, uint64_t c) {
    const uint64_t h = a ^ b;
    out0 = h ^ c;
    out1 = (a & b) | (c & h);
  }

  // ---- stepping (LifeAPI.hpp:866-907,1196-1254), CPU, single universe
  void CountRows(LifeState &__restrict__ bit0, LifeState &__restrict__ bit1) const {
    for (int i = 0; i < N; ++i) {
      const uint64_t a = state[i], l = std::rotl(a, 1), r = std::rotr(a, 1);
      bit0.state[i] = l ^ r ^ a;
      bit1.state[i] = ((l ^ r) & a) | (l & r);
    }
  }
  // Rokicki form of the B3/S23 rule (LifeAPI.hpp:837-848): the centre column
  // plus the 2-bit vertical sums of the columns above (u) and below (b)
  static uint64_t Rokicki(uint64_t a, uint64_t u0, uint64_t u1, uint64_t b0, uint64_t b1) {
    const uint64_t aw = std::rotl(a, 1), ae = std::rotr(a, 1);
    const uint64_t s0 = aw ^ ae, s1 = aw & ae;
    const uint64_t ts0 = b0 ^ u0;
    const uint64_t ts1 = (b0 & u0) | (ts0 & s0);
    return (b1 ^ u1 ^ ts1 ^ s1) & ((b1 | u1) ^ (ts1 | s1)) & ((ts0 ^ s0) | a);
  }
  // Step() (LifeAPI.hpp:1196-1216).  The torus wrap is peeled out of the
  // loop (columns 0 and 63), so the 62 interior columns are straight-line
  // code the compiler unrolls and vectorises like the reference's
  // `unroll(full)` loop.
  void Step() {
    LifeState c0(InitializedTag::UNINITIALIZED), c1(InitializedTag::UNINITIALIZED);
    CountRows(c0, c1);
    state[0] = Rokicki(state[0], c0.state[N - 1], c1.state[N - 1], c0.state[1], c1.state[1]);
#if defined(__clang__)
#pragma clang loop unroll(full)
#elif defined(__GNUC__)
#pragma GCC unroll 64
#endif
    for (int i = 1; i < N - 1; ++i)
      state[i] = Rokicki(state[i], c0.state[i - 1], c1.state[i - 1], c0.state[i + 1], c1.state[i + 1]);
    state[N - 1] = Rokicki(state[N - 1], c0.state[N - 2], c1.state[N - 2], c0.state[0], c1.state[0]);
  }
  void StepAlt() {
    LifeState c0(InitializedTag::UNINITIALIZED), c1(InitializedTag::UNINITIALIZED);
    CountRows(c0, c1);
    for (int i = 0; i < N; ++i) {
      const int u = (i + N - 1) & (N - 1), b = (i + 1) & (N - 1);
      uint64_t fs, fc, cs, cc;
      FullAdd(fs, fc, c0[u], c0[i], c0[b]);
      FullAdd(cs, cc, c1[u], c1[i], c1[b]);
      cc ^= fc & cs;
      state[i] = (fs ^ cc) & (fc ^ cs ^ cc) & (state[i] | fs);
    }
  }
  void Step(unsigned n) {
    for (unsigned g = 0; g < n; ++g) Step();
  }
  LifeState Stepped() const {
    LifeState c = *this;
    c.Step();
    return c;
  }
  LifeState Stepped(unsigned n) const {
    LifeState c = *this;
    c.Step(n);
    return c;
  }

  // ---- parsing (Parsing.hpp:143-198 semantics: header lines starting with
  // 'x' skipped; bare '$' = 1; non-'o' cell chars are dead; no wrapping)
  static LifeState Parse(const std::string &rle) {
    LifeState r;
    int cnt = 0, x = 0, y = 0;
    bool at_line_start = true, skip_line = false;
    for (char ch : rle) {
      if (at_line_start) {
        skip_line = ch == 'x';
        at_line_start = false;
      }
      if (ch == '\n') {
        at_line_start = true;
        continue;
      }
      if (skip_line) continue;
      if (ch >= '0' && ch <= '9') {
        cnt = cnt * 10 + (ch - '0');
      } else if (ch == '$') {
        if (cnt == 0) cnt = 1;
        if (cnt == 129) return r;
        y += cnt;
        x = 0;
        cnt = 0;
      } else if (ch == '!') {
        break;
      } else if (ch == '\r' || ch == ' ') {
        continue;
      } else {
        if (cnt == 0) cnt = 1;
        for (int j = 0; j < cnt; ++j, ++x)
          if (ch == 'o' && x >= 0 && x < N && y >= 0 && y < N) r.Set(x, y);
        cnt = 0;
      }
    }
    return r;
  }

  // LifeState::RLE() (Parsing.hpp:8-63,200-204): printed from x = y = 32 like
  // the reference, so Parse(s.RLE()) is s moved by (32, 32)
  std::string RLE() const {
    std::string out;
    auto count = [&](unsigned c) {
      if (c > 1) out += std::to_string(c);
    };
    unsigned rows = 0;
    for (int j = 0; j < N; ++j) {
      const int y = (j + 32) & (N - 1);
      bool last = Get(32, y);
      unsigned run = 0;
      for (int i = 0; i < N; ++i) {
        const bool v = Get((i + 32) & (N - 1), y);
        if (v && rows) {
          count(rows);
          out += '$';
          rows = 0;
        }
        if (v != last) {
          count(run);
          out += last ? 'o' : 'b';
          run = 0;
        }
        ++run;
        last = v;
      }
      if (last) {
        count(run);
        out += 'o';
      }
      ++rows;
    }
    return out + '!';
  }

  // Seeded counterpart of RandomState() (LifeAPI.hpp:18-23,63-69): each column
  // uniform on [2^61, 2^62) (row 61 on, rows 62-63 off), from a splitmix64
  // stream instead of the reference's random_device-seeded mt19937_64.
  static LifeState RandomState(uint64_t &seed) {
    LifeState r;
    for (int i = 0; i < N; ++i) {
      uint64_t z = (seed += 0x9E3779B97F4A7C15ULL);
      z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
      z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
      z ^= z >> 31;
      r.state[i] = (z & ((uint64_t(1) << 61) - 1)) | (uint64_t(1) << 61);
    }
    return r;
  }
};

static_assert(sizeof(LifeState) == 512 && alignof(LifeState) == 64, "LifeAPI.hpp:39-40 layout");

// Symmetry.hpp:798-830: the eight images under D4, each moved so that its
// bounds start at (0, 0), those equal to an earlier one dropped; and the
// transforms that gave the ones kept
namespace detail {
inline constexpr SymmetryTransform kOrbit[8] = {
    SymmetryTransform::Identity,          SymmetryTransform::ReflectAcrossX,
    SymmetryTransform::ReflectAcrossYeqX, SymmetryTransform::ReflectAcrossY,
    SymmetryTransform::ReflectAcrossYeqNegXP1, SymmetryTransform::Rotate90,
    SymmetryTransform::Rotate270,         SymmetryTransform::Rotate180OddBoth};
inline void orbit(const LifeState &s, std::vector<LifeState> &images, std::vector<SymmetryTransform> &kept) {
  for (SymmetryTransform t : kOrbit) {
    LifeState img = s.Transformed(t);
    const std::array<int, 4> b = img.XYBounds();
    img.Move(-b[0], -b[1]);
    bool seen = false;
    for (const LifeState &e : images) seen = seen || e == img;
    if (!seen) {
      images.push_back(img);
      kept.push_back(t);
    }
  }
}
}  // namespace detail
inline std::vector<LifeState> LifeState::SymmetryOrbit() const {
  std::vector<LifeState> images;
  std::vector<SymmetryTransform> kept;
  detail::orbit(*this, images, kept);
  return images;
}
inline std::vector<SymmetryTransform> LifeState::SymmetryOrbitRepresentatives() const {
  std::vector<LifeState> images;
  std::vector<SymmetryTransform> kept;
  detail::orbit(*this, images, kept);
  return kept;
}

// Symmetry.hpp:540-563: the part of `offset` across the transform's mirror
// line.  The diagonal cases halve in int arithmetic, truncating as C++ does,
// so the result is not a function of the offset mod 64 alone.
inline std::pair<int, int> PerpComponent(SymmetryTransform t, std::pair<int, int> offset) {
  const int x = (offset.first + 32) % 64 - 32, y = (offset.second + 32) % 64 - 32;
  switch (t) {
  case SymmetryTransform::ReflectAcrossX: return {0, offset.second};
  case SymmetryTransform::ReflectAcrossY: return {offset.first, 0};
  case SymmetryTransform::ReflectAcrossYeqX: return {((x - y + 128) / 2) % 64, ((-x + y + 128) / 2) % 64};
  case SymmetryTransform::ReflectAcrossYeqNegXP1: return {((x + y + 128) / 2) % 64, ((x + y + 128) / 2) % 64};
  default: return offset;
  }
}

// Symmetry.hpp:565-654: the union of `state` with its images under the
// symmetry's generators, the mirror lines / centre displaced by `offset`.
// Defined for the nine symmetries below, as in the reference.
inline LifeState Symmetricize(const LifeState &state, StaticSymmetry sym, std::pair<int, int> offset) {
  using enum SymmetryTransform;
  const auto [dx, dy] = offset;
  // acc | acc.Transformed(t).Moved(mx, my)
  auto with = [](const LifeState &acc, SymmetryTransform t, int mx, int my) {
    return acc | acc.Transformed(t).Moved(mx, my);
  };
  switch (sym) {
  case StaticSymmetry::C1: return state;
  case StaticSymmetry::C2: return with(state, Rotate180EvenBoth, dx + 1, dy + 1);
  case StaticSymmetry::C4:
    return with(with(state, Rotate90, dx, dy), Rotate180EvenBoth, dx - dy + 1, dy + dx + 1);
  case StaticSymmetry::D2AcrossX: return with(state, ReflectAcrossXEven, dx, dy + 1);
  case StaticSymmetry::D2AcrossY: return with(state, ReflectAcrossYEven, dx + 1, dy);
  case StaticSymmetry::D2diagodd: return with(state, ReflectAcrossYeqX, dx, dy);
  case StaticSymmetry::D2negdiagodd: return with(state, ReflectAcrossYeqNegX, dx + 1, dy + 1);
  case StaticSymmetry::D4: {
    const auto xo = PerpComponent(ReflectAcrossX, offset), yo = PerpComponent(ReflectAcrossY, offset);
    return with(with(state, ReflectAcrossXEven, xo.first, xo.second + 1), ReflectAcrossYEven, yo.first + 1,
                yo.second);
  }
  case StaticSymmetry::D4diag: {
    const auto yo = PerpComponent(ReflectAcrossYeqX, offset), xo = PerpComponent(ReflectAcrossYeqNegXP1, offset);
    return with(with(state, ReflectAcrossYeqX, yo.first, yo.second), ReflectAcrossYeqNegX, xo.first + 1,
                xo.second + 1);
  }
  default: __builtin_unreachable();
  }
}

// Symmetry.hpp:729-768: the offsets at which the image of pat1 under the
// symmetry touches pat2, pat2.Convolve(pat1.Transformed(t)).  Defined for the
// six symmetries below, as in the reference.  CPU, single pair; batches go to
// the GPU via lifeapi::IntersectingOffsetsBatch.
inline LifeState IntersectingOffsets(const LifeState &pat1, const LifeState &pat2, StaticSymmetry sym) {
  using enum SymmetryTransform;
  switch (sym) {
  case StaticSymmetry::C2: return pat2.Convolve(pat1);
  case StaticSymmetry::C4: return pat2.Convolve(pat1.Transformed(Rotate270));
  case StaticSymmetry::D2AcrossX: return pat2.Convolve(pat1.Transformed(ReflectAcrossY));
  case StaticSymmetry::D2AcrossY: return pat2.Convolve(pat1.Transformed(ReflectAcrossX));
  case StaticSymmetry::D2diagodd: return pat2.Convolve(pat1.Transformed(ReflectAcrossYeqNegXP1));
  case StaticSymmetry::D2negdiagodd: return pat2.Convolve(pat1.Transformed(ReflectAcrossYeqX));
  default: __builtin_unreachable();
  }
}
// Symmetry.hpp:770-772
inline LifeState IntersectingOffsets(const LifeState &active, StaticSymmetry sym) {
  return IntersectingOffsets(active, active, sym);
}

// LifeTarget.hpp:5-36 (the search-loop subset)
struct LifeTarget {
  LifeState wanted;
  LifeState unwanted;
  LifeTarget() = default;
  // the pattern and its boundary: the cells around it must be dead (:10-13)
  explicit LifeTarget(const LifeState &state) : wanted(state), unwanted(state.GetBoundary()) {}
  LifeTarget(const LifeState &w, const LifeState &u) : wanted(w), unwanted(u) {}
  LifeTarget Moved(std::pair<int, int> v) const {  // :33-35
    return LifeTarget(wanted.Moved(v), unwanted.Moved(v));
  }
  void Transform(SymmetryTransform t) {  // :20-23
    wanted.Transform(t);
    unwanted.Transform(t);
  }
  LifeTarget Transformed(SymmetryTransform t) const {  // :26-30
    return LifeTarget(wanted.Transformed(t), unwanted.Transformed(t));
  }
};

// LifeTarget.hpp:44-51
inline bool LifeState::Contains(const LifeTarget &t) const {
  uint64_t d = 0;
  for (int i = 0; i < N; ++i) d |= (state[i] ^ t.wanted[i]) & (t.wanted[i] | t.unwanted[i]);
  return d == 0;
}
// LifeTarget.hpp:38-42
inline bool LifeState::Contains(const LifeTarget &t, int dx, int dy) const {
  return Contains(t.wanted, dx, dy) && AreDisjoint(t.unwanted, dx, dy);
}

// NeighbourCount.hpp:7-102 (hot-path subset): inclusive 3x3 count 0..9 as
// four bit planes, same member order as the reference.
struct NeighbourCount {
  LifeState bit3, bit2, bit1, bit0;

  NeighbourCount() = default;
  explicit NeighbourCount(const LifeState &s) {
    LifeState c0(InitializedTag::UNINITIALIZED), c1(InitializedTag::UNINITIALIZED);
    s.CountRows(c0, c1);
    for (int i = 0; i < N; ++i) {
      const int u = (i + N - 1) & (N - 1), d = (i + 1) & (N - 1);
      uint64_t fs, fc, cs, cc;
      LifeState::FullAdd(fs, fc, c0[u], c0[i], c0[d]);
      LifeState::FullAdd(cs, cc, c1[u], c1[i], c1[d]);
      bit0[i] = fs;
      bit1[i] = fc ^ cs;
      bit2[i] = cc ^ (fc & cs);
      bit3[i] = cc & fc & cs;
    }
  }
  LifeState WithExactly(unsigned n) const {
    LifeState r = ~LifeState();
    r &= (n & 1) ? bit0 : ~bit0;
    r &= (n & 2) ? bit1 : ~bit1;
    r &= (n & 4) ? bit2 : ~bit2;
    r &= (n & 8) ? bit3 : ~bit3;
    return r;
  }
};

// LifeTarget.hpp:53-55
inline LifeState LifeState::Match(const LifeTarget &t) const { return MatchLiveAndDead(t.wanted, t.unwanted); }

// LifeAPI.hpp:1066-1095: the offsets at which `other`, moved there, overlaps
// this pattern or changes its next generation, as the OR of seven
// convolutions of count planes of this pattern with count planes of
// other.Mirrored() (count = the inclusive 3x3 count; "dead" = not in the
// pattern itself):
//   cells x cells                                    (overlap)
//   dead with count 1 x dead with count 2, both ways (births)
//   live with count 3 x dead with count >= 2, and
//   live with count >= 4 x dead with count >= 1, both ways (overcrowding)
inline LifeState LifeState::InteractionOffsets(const LifeState &other) const {
  struct Planes {
    LifeState cells, dead1, dead2, live3, live4up, dead2up, dead1up;
    explicit Planes(const LifeState &s) {
      const NeighbourCount c(s);
      const LifeState high = c.bit3 | c.bit2, low = ~high;
      cells = s;
      dead1 = low & ~c.bit1 & c.bit0 & ~s;
      dead2 = low & c.bit1 & ~c.bit0 & ~s;
      live3 = low & c.bit1 & c.bit0 & s;
      live4up = high & s;
      dead2up = (high | c.bit1) & ~s;
      dead1up = (high | c.bit1 | c.bit0) & ~s;
    }
  };
  const Planes a(*this), b(other.Mirrored());
  // (Convolve is symmetric: each is taken with other's plane as the pattern,
  // so the time is proportional to other's planes' populations)
  return a.cells.Convolve(b.cells) | a.dead1.Convolve(b.dead2) | a.dead2.Convolve(b.dead1) |
         a.live3.Convolve(b.dead2up) | a.live4up.Convolve(b.dead1up) | a.dead2up.Convolve(b.live3) |
         a.dead1up.Convolve(b.live4up);
}

// LifeStable.hpp:41-53: the ten planes of the stable-search state (options
// stored as "1 = ruled out").  Propagation runs on the GPU:
// lifeapi::PropagateStepBatch / PropagateBatch in lifeapi/batch.hpp.
enum class StableOptions : unsigned char {  // LifeStable.hpp:7-20
  LIVE2 = 1 << 0, LIVE3 = 1 << 1,
  DEAD0 = 1 << 2, DEAD1 = 1 << 3, DEAD2 = 1 << 4, DEAD4 = 1 << 5, DEAD5 = 1 << 6, DEAD6 = 1 << 7,
  IMPOSSIBLE = 0, LIVE = LIVE2 | LIVE3, DEAD = DEAD0 | DEAD1 | DEAD2 | DEAD4 | DEAD5 | DEAD6,
};
constexpr StableOptions operator~(StableOptions a) { return StableOptions((unsigned char)~(unsigned char)a); }
constexpr StableOptions operator|(StableOptions a, StableOptions b) {
  return StableOptions((unsigned char)a | (unsigned char)b);
}
constexpr StableOptions operator&(StableOptions a, StableOptions b) {
  return StableOptions((unsigned char)a & (unsigned char)b);
}

struct LifeStable {
  LifeState state, unknown;
  LifeState live2, live3;
  LifeState dead0, dead1, dead2, dead4, dead5, dead6;

  bool operator==(const LifeStable &o) const {
    return state == o.state && unknown == o.unknown && live2 == o.live2 && live3 == o.live3 && dead0 == o.dead0 &&
           dead1 == o.dead1 && dead2 == o.dead2 && dead4 == o.dead4 && dead5 == o.dead5 && dead6 == o.dead6;
  }
  // LifeStable.hpp:308-318: `cells` keep only the options in `options`, i.e.
  // every other option's plane gets them
  void RestrictOptions(const LifeState &cells, StableOptions options) {
    LifeState *const plane[8] = {&live2, &live3, &dead0, &dead1, &dead2, &dead4, &dead5, &dead6};
    for (int k = 0; k < 8; ++k)
      if (!((unsigned char)options >> k & 1)) *plane[k] |= cells;
  }
  void SetOn(const LifeState &which) {  // LifeStable.hpp:320-329
    state |= which;
    unknown &= ~which;
    RestrictOptions(which, StableOptions::LIVE);
  }
  void SetOff(const LifeState &which) {  // LifeStable.hpp:330-335
    state &= ~which;
    unknown &= ~which;
    RestrictOptions(which, StableOptions::DEAD);
  }
};

// LifeWeld.hpp:18-400 (the search subset): a state plus a frozen 3-bit
// neighbour count added when stepping.  The batched forms are
// lifeapi::Weld*Batch in lifeapi/batch.hpp.
struct LifeWeld {
  LifeState state, frozen2, frozen1, frozen0;

  bool operator==(const LifeWeld &o) const {
    return state == o.state && frozen2 == o.frozen2 && frozen1 == o.frozen1 && frozen0 == o.frozen0;
  }
  void Step() {  // LifeWeld.hpp:169-186
    const NeighbourCount c(state);
    for (int i = 0; i < N; ++i) {
      uint64_t s0, k0, s1, k1, s2, k2;
      LifeState::HalfAdd(s0, k0, c.bit0[i], frozen0[i]);
      LifeState::FullAdd(s1, k1, c.bit1[i], frozen1[i], k0);
      LifeState::FullAdd(s2, k2, c.bit2[i], frozen2[i], k1);
      state[i] = (s0 ^ s2) & (s1 ^ s2) & (state[i] | s0);
    }
  }
  LifeWeld Stepped() const {
    LifeWeld w = *this;
    w.Step();
    return w;
  }
  LifeState AllFrozen() const { return frozen2 | frozen1 | frozen0; }  // :40
  LifeWeld operator|(const LifeWeld &o) const {                         // :42-45
    return {state | o.state, frozen2 | o.frozen2, frozen1 | o.frozen1, frozen0 | o.frozen0};
  }
  LifeWeld Moved(std::pair<int, int> v) const {  // :65-68
    return {state.Moved(v), frozen2.Moved(v), frozen1.Moved(v), frozen0.Moved(v)};
  }
  // the cells with no frozen count, and everything next to one
  LifeState NonFrozenZOI() const { return (state & ~AllFrozen()).ZOI(); }

  // LifeWeld.hpp:133-159: the part of `state` within reach of the cells that
  // `required` does not cover; the stator dropped from it is remembered as a
  // frozen count on the required cells next to the active region and on the
  // cells where the kept part alone would see a birth.  (The stator's count
  // has a bit 3; it is dropped, as in the reference.)
  static LifeWeld FromRequired(const LifeState &state, const LifeState &required) {
    const LifeState reach = (state.ZOI() & ~required).ZOI();
    const LifeState stator = state & ~reach, kept = state & ~stator;
    const LifeState frozen = (reach & required) | (kept.Stepped() & ~kept);
    const NeighbourCount c(stator);
    return {kept, c.bit2 & frozen, c.bit1 & frozen, c.bit0 & frozen};
  }
  // LifeWeld.hpp:188-191: what to match to know that it has recovered
  LifeTarget ToTarget() const { return LifeTarget(state, NonFrozenZOI() & ~state); }

  // LifeWeld.hpp:279-325
  LifeStable ToStable() const {
    LifeStable st;
    st.unknown = ~LifeState();
    const NeighbourCount sum = SumCounts();
    const LifeState frozen = AllFrozen(), live = frozen & state, dead = frozen & ~state;
    st.SetOn(state);
    st.SetOff(~state & NonFrozenZOI());
    using enum StableOptions;
    st.RestrictOptions(live & sum.WithExactly(3), LIVE2);  // (the sum counts the centre)
    st.RestrictOptions(live & sum.WithExactly(4), LIVE3);
    st.RestrictOptions(dead & sum.WithExactly(1), DEAD1);
    st.RestrictOptions(dead & sum.WithExactly(2), DEAD2);
    st.RestrictOptions(dead & sum.WithExactly(4), DEAD4);
    st.RestrictOptions(dead & sum.WithExactly(5), DEAD5);
    st.RestrictOptions(dead & sum.WithExactly(6), DEAD6);
    return st;
  }
  // LifeWeld.hpp:327-400.  The reference replays the reaction twice; every
  // update is an OR into an option plane or an AND-NOT into unknown whose
  // operand does not depend on the stable, so one replay does both.
  LifeStable ToStable(const LifeState &active, unsigned duration, const LifeState &mask = ~LifeState()) const {
    LifeStable st = ToStable();
    const NeighbourCount mine(state);
    LifeWeld current = *this;
    current.state |= active;
    LifeState everActive;
    using enum StableOptions;
    // {count of current.state, count of state, the one option that goes} of the cells that stay dead
    static constexpr struct { unsigned now, mine; StableOptions gone; } kStay[11] = {
        {1, 0, DEAD2}, {2, 0, DEAD1}, {2, 1, DEAD2}, {1, 2, DEAD4}, {0, 2, DEAD5}, {3, 4, DEAD4},
        {2, 4, DEAD5}, {1, 4, DEAD6}, {3, 5, DEAD5}, {2, 5, DEAD6}, {3, 6, DEAD6}};
    for (unsigned g = 0; g < duration; ++g) {
      everActive |= state ^ current.state;
      const LifeWeld next = current.Stepped();
      const LifeState dead = mask & ~state & ~current.state;
      const LifeState born = dead & next.state, stay = dead & ~next.state;
      const NeighbourCount now(current.state);
      st.RestrictOptions(born & now.WithExactly(3) & mine.WithExactly(0), DEAD0);
      st.RestrictOptions(born & now.WithExactly(3) & mine.WithExactly(1), DEAD1);
      st.RestrictOptions(born & now.WithExactly(3) & mine.WithExactly(2), DEAD2);
      for (const auto &r : kStay) st.RestrictOptions(stay & now.WithExactly(r.now) & mine.WithExactly(r.mine), ~r.gone);
      if (next == current) break;  // a fixed point: every later generation repeats this one
      current = next;
    }
    st.SetOff(mask & ~state & everActive);
    return st;
  }

  // LifeWeld.hpp:206-245: LifeState::InteractionOffsets with every plane but
  // the overlap term's kept only inside its side's NonFrozenZOI() -- except
  // that, as in the reference (:238-239), the second operand of each birth
  // term is cut by the FIRST operand's region: other's dead2 plane by ours,
  // our dead2 plane by other's.
  LifeState InteractionOffsets(const LifeWeld &other) const {
    struct Planes {
      LifeState cells, dead1, dead2, live3, live4up, dead2up, dead1up;
      explicit Planes(const LifeState &s) {
        const NeighbourCount c(s);
        const LifeState high = c.bit3 | c.bit2, low = ~high;
        cells = s;
        dead1 = low & ~c.bit1 & c.bit0 & ~s;
        dead2 = low & c.bit1 & ~c.bit0 & ~s;
        live3 = low & c.bit1 & c.bit0 & s;
        live4up = high & s;
        dead2up = (high | c.bit1) & ~s;
        dead1up = (high | c.bit1 | c.bit0) & ~s;
      }
    };
    const Planes a(state), b(other.state.Mirrored());
    const LifeState ak = NonFrozenZOI(), bk = other.NonFrozenZOI().Mirrored();
    return a.cells.Convolve(b.cells) | (a.dead1 & ak).Convolve(b.dead2 & ak) | (b.dead1 & bk).Convolve(a.dead2 & bk) |
           (a.live3 & ak).Convolve(b.dead2up & bk) | (a.live4up & ak).Convolve(b.dead1up & bk) |
           (b.live3 & bk).Convolve(a.dead2up & ak) | (b.live4up & bk).Convolve(a.dead1up & ak);
  }

 private:
  // the inclusive count of state plus the frozen number, four bits (:295-299)
  NeighbourCount SumCounts() const {
    NeighbourCount c(state), sum;
    for (int i = 0; i < N; ++i) {
      uint64_t k0, k1, k2;
      LifeState::HalfAdd(sum.bit0[i], k0, c.bit0[i], frozen0[i]);
      LifeState::FullAdd(sum.bit1[i], k1, c.bit1[i], frozen1[i], k0);
      LifeState::FullAdd(sum.bit2[i], k2, c.bit2[i], frozen2[i], k1);
      sum.bit3[i] = c.bit3[i] ^ k2;
    }
    return sum;
  }
};

}  // namespace lifeapi

#include "batch.hpp"
