// lifeapi/batch.hpp -- batched GPU Step() for any LifeState-layout type.
//
// Works on the reference's own ::LifeState (LifeAPI.hpp:39-40: uint64_t
// state[64], aligned(64), trivially copyable) as well as lifeapi::LifeState:
// an existing search loop keeps #include "LifeAPI.hpp" and adds
//
//     #include <lifeapi/batch.hpp>
//     std::vector<LifeState> candidates = ...;
//     lifeapi::StepBatch(std::span(candidates), 4);   // == c.Step(4) for each c
//
// Semantics mirror LifeState::Step(unsigned) / Stepped(unsigned)
// (LifeAPI.hpp:877-886) element-wise.  The reference's Step() cannot fail;
// a GPU call can, so failures throw lifeapi::Error (code = the C ABI's
// return value, see lifeapi_hip.h).  Link with -llifeapi_hip.
#pragma once

#include <array>
#include <bit>
#include <cstdint>
#include <span>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../lifeapi_hip.h"

namespace lifeapi {

template <class S>
concept LifeStateLayout = sizeof(S) == 64 * sizeof(uint64_t) && alignof(S) >= alignof(uint64_t) &&
                          std::is_trivially_copyable_v<S> && std::is_standard_layout_v<S>;

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string &what) : std::runtime_error(what), code(c) {}
};

inline void check(int rc) {
  if (rc != LIFEAPI_OK) throw Error(rc, std::string("lifeapi: ") + lifeapi_last_error());
}

inline const uint64_t *words(const void *p) { return static_cast<const uint64_t *>(p); }
inline uint64_t *words(void *p) { return static_cast<uint64_t *>(p); }

// In place: states[i].Step(generations) for every i.  device = -1 shards the
// batch over every visible GPU.
template <LifeStateLayout S>
void StepBatch(std::span<S> states, unsigned generations = 1, int device = 0) {
  check(lifeapi_step_batch(words(states.data()), words(states.data()), states.size(), generations,
                           device));
}

// out[i] = in[i].Stepped(generations)
template <LifeStateLayout S>
void SteppedBatch(std::span<const S> in, std::span<S> out, unsigned generations = 1,
                  int device = 0) {
  if (out.size() != in.size()) throw Error(LIFEAPI_E_INVALID, "lifeapi: size mismatch");
  check(lifeapi_step_batch(words(in.data()), words(out.data()), in.size(), generations, device));
}

// pops[i] = states[i].GetPop()
template <LifeStateLayout S>
std::vector<uint32_t> GetPopBatch(std::span<const S> states, int device = 0) {
  std::vector<uint32_t> pops(states.size());
  check(lifeapi_pop_batch(words(states.data()), pops.data(), states.size(), device));
  return pops;
}

// ---- the other per-generation kernels, on the reference's own types ----
//
// Each concept pins the reference struct's byte layout: N LifeStates in
// member order, nothing else.
template <class T, size_t Planes>
concept PlaneLayout = sizeof(T) == Planes * 64 * sizeof(uint64_t) && std::is_trivially_copyable_v<T> &&
                      std::is_standard_layout_v<T>;
// LifeWeld {state, frozen2, frozen1, frozen0}           LifeWeld.hpp:18-20
template <class T> concept LifeWeldLayout = PlaneLayout<T, 4>;
// LifeStable {state, unknown, live2 .. dead6}            LifeStable.hpp:41-53
template <class T> concept LifeStableLayout = PlaneLayout<T, 10>;
// NeighbourCount {bit3, bit2, bit1, bit0}                NeighbourCount.hpp:7-11
template <class T> concept NeighbourCountLayout = PlaneLayout<T, 4>;
// LifeTarget {wanted, unwanted}                          LifeTarget.hpp:5-7
template <class T> concept LifeTargetLayout = PlaneLayout<T, 2>;

// welds[i].Step() `generations` times (LifeWeld.hpp:169-186)
template <LifeWeldLayout W>
void WeldStepBatch(std::span<W> welds, unsigned generations = 1, int device = 0) {
  check(lifeapi_weld_step_batch(words(welds.data()), welds.size(), generations, device));
}

// LifeStable::PropagateResult (LifeStable.hpp:123-126)
struct PropagateResult {
  bool consistent;
  bool changed;
};

namespace detail {
template <LifeStableLayout S>
std::vector<PropagateResult> stable_pass(std::span<S> s, int pass, unsigned max_iters, int device) {
  std::vector<uint8_t> f(s.size());
  check(lifeapi_stable_pass_batch(words(s.data()), f.data(), s.size(), pass, max_iters, device));
  std::vector<PropagateResult> r(s.size());
  for (size_t i = 0; i < s.size(); ++i) r[i] = {(f[i] & 1) != 0, (f[i] & 2) != 0};
  return r;
}
}  // namespace detail

// s[i].PropagateStep() / s[i].Propagate() (LifeStable.hpp:695-729), in place
template <LifeStableLayout S>
std::vector<PropagateResult> PropagateStepBatch(std::span<S> s, int device = 0) {
  return detail::stable_pass(s, 3, 0, device);
}
template <LifeStableLayout S>
std::vector<PropagateResult> PropagateBatch(std::span<S> s, int device = 0) {
  return detail::stable_pass(s, 4, 0, device);
}
// s[i].StabiliseOptions() (LifeStable.hpp:677-693), in place
template <LifeStableLayout S>
std::vector<PropagateResult> StabiliseOptionsBatch(std::span<S> s, int device = 0) {
  return detail::stable_pass(s, 5, 0, device);
}

namespace detail {
inline std::vector<PropagateResult> results(const std::vector<uint8_t> &f) {
  std::vector<PropagateResult> r(f.size());
  for (size_t i = 0; i < f.size(); ++i) r[i] = {(f[i] & 1) != 0, (f[i] & 2) != 0};
  return r;
}
}  // namespace detail

// s[i].PropagateStrip(columns[i]) (LifeStable.hpp:1238-1249), in place: the
// propagation TestUnknown runs, which stops at the strip's edge
template <LifeStableLayout S>
std::vector<PropagateResult> PropagateStripBatch(std::span<S> s, std::span<const uint8_t> columns, int device = 0) {
  if (columns.size() != s.size()) throw Error(LIFEAPI_E_INVALID, "lifeapi: size mismatch");
  std::vector<uint8_t> f(s.size());
  check(lifeapi_stable_strip_pass_batch(words(s.data()), columns.data(), f.data(), s.size(), 4, 0, device));
  return detail::results(f);
}
// s[i].TestUnknowns(cells) (LifeStable.hpp:1321-1338; TestUnknown :1251-1284,
// Join :217-233), in place: one mask for the batch, or one per object
template <LifeStableLayout S, LifeStateLayout L>
std::vector<PropagateResult> TestUnknownsBatch(std::span<S> s, const L &cells, int device = 0) {
  std::vector<uint8_t> f(s.size());
  check(lifeapi_stable_test_unknowns_batch(words(s.data()), words(&cells), 0, f.data(), s.size(), 0, device));
  return detail::results(f);
}
template <LifeStableLayout S, LifeStateLayout L>
std::vector<PropagateResult> TestUnknownsBatch(std::span<S> s, std::span<const L> cells, int device = 0) {
  if (cells.size() != s.size()) throw Error(LIFEAPI_E_INVALID, "lifeapi: size mismatch");
  std::vector<uint8_t> f(s.size());
  check(lifeapi_stable_test_unknowns_batch(words(s.data()), words(cells.data()), 1, f.data(), s.size(), 0, device));
  return detail::results(f);
}
// s[i].PropagateAndTest() (LifeStable.hpp:163-184), in place: a search node's
// Propagate / TestUnknowns(Vulnerable().ZOI()) rounds to their fixed point
template <LifeStableLayout S>
std::vector<PropagateResult> PropagateAndTestBatch(std::span<S> s, int device = 0) {
  std::vector<uint8_t> f(s.size());
  check(lifeapi_stable_propagate_and_test_batch(words(s.data()), f.data(), s.size(), 0, device));
  return detail::results(f);
}

// out[i] = s[i].Vulnerable()  (LifeStable.hpp:366-412)
template <LifeStableLayout S, LifeStateLayout L>
void VulnerableBatch(std::span<const S> s, std::span<L> out, int device = 0) {
  if (out.size() != s.size()) throw Error(LIFEAPI_E_INVALID, "lifeapi: size mismatch");
  check(lifeapi_stable_vulnerable_batch(words(s.data()), words(out.data()), s.size(), device));
}

// out[i] = NeighbourCount(in[i])  (NeighbourCount.hpp:40-70)
template <LifeStateLayout S, NeighbourCountLayout C>
void NeighbourCountBatch(std::span<const S> in, std::span<C> out, int device = 0) {
  if (out.size() != in.size()) throw Error(LIFEAPI_E_INVALID, "lifeapi: size mismatch");
  check(lifeapi_neighbour_count_batch(words(in.data()), words(out.data()), in.size(), device));
}

// r[i] = in[i].Contains(target)  (LifeTarget.hpp:44-51)
template <LifeStateLayout S, LifeTargetLayout T>
std::vector<uint8_t> ContainsBatch(std::span<const S> in, const T &target, int device = 0) {
  std::vector<uint8_t> r(in.size());
  const uint64_t *t = words(&target);
  check(lifeapi_contains_batch(words(in.data()), t, t + 64, r.data(), in.size(), device));
  return r;
}

// The target as the offset forms of the reference test it:
//     s.Contains(target, dx, dy) = s.Contains(target.wanted, dx, dy) && s.AreDisjoint(target.unwanted, dx, dy)
// (LifeTarget.hpp:38-42) reads s at column i+dx rotated right by dy against
// target column i (LifeAPI.hpp:399-421): on the torus that is the unshifted
// test against the target Moved(dx, dy) (LifeAPI.hpp:682-696).  Returns false
// when some cell is both wanted and unwanted: no state passes the offset form
// then, where the unshifted Contains(target) asks such a cell to be alive.
namespace detail {
inline bool moved_target(const uint64_t *t, int dx, int dy, uint64_t *out) {
  const unsigned x = (unsigned)dx & 63u, y = (unsigned)dy & 63u;
  uint64_t clash = 0;
  for (unsigned i = 0; i < 64; ++i) {
    clash |= t[i] & t[64 + i];
    out[(i + x) & 63u] = std::rotl(t[i], (int)y);
    out[64 + ((i + x) & 63u)] = std::rotl(t[64 + i], (int)y);
  }
  return clash == 0;
}
}  // namespace detail

// r[i] = in[i].Contains(target, dx, dy)  (LifeTarget.hpp:38-42)
template <LifeStateLayout S, LifeTargetLayout T>
std::vector<uint8_t> ContainsBatch(std::span<const S> in, const T &target, int dx, int dy, int device = 0) {
  uint64_t t[128];
  if (!detail::moved_target(words(&target), dx, dy, t)) return std::vector<uint8_t>(in.size(), 0);
  std::vector<uint8_t> r(in.size());
  check(lifeapi_contains_batch(words(in.data()), t, t + 64, r.data(), in.size(), device));
  return r;
}

// The pattern tests (LifeAPI.hpp:377-421) are targets with one plane empty:
//     s.Contains(pat)          == s.Contains(LifeTarget{pat, {}})
//     s.AreDisjoint(pat)       == s.Contains(LifeTarget{{}, pat})
// and their (dx, dy) forms the same against pat Moved(dx, dy).  All run the
// batched Contains, which reads only the columns the pattern occupies.
namespace detail {
template <LifeStateLayout S>
std::vector<uint8_t> pattern_batch(std::span<const S> in, const uint64_t *pat, bool disjoint, int dx, int dy,
                                   int device) {
  uint64_t t[128] = {};
  const unsigned x = (unsigned)dx & 63u, y = (unsigned)dy & 63u;
  uint64_t *plane = t + (disjoint ? 64 : 0);
  for (unsigned i = 0; i < 64; ++i) plane[(i + x) & 63u] = std::rotl(pat[i], (int)y);
  std::vector<uint8_t> r(in.size());
  check(lifeapi_contains_batch(words(in.data()), t, t + 64, r.data(), in.size(), device));
  return r;
}
}  // namespace detail

// r[i] = in[i].Contains(pat)  (LifeAPI.hpp:388-397)
template <LifeStateLayout S, LifeStateLayout P>
std::vector<uint8_t> ContainsBatch(std::span<const S> in, const P &pat, int device = 0) {
  return detail::pattern_batch(in, words(&pat), false, 0, 0, device);
}
// r[i] = in[i].Contains(pat, dx, dy)  (LifeAPI.hpp:399-409)
template <LifeStateLayout S, LifeStateLayout P>
std::vector<uint8_t> ContainsBatch(std::span<const S> in, const P &pat, int dx, int dy, int device = 0) {
  return detail::pattern_batch(in, words(&pat), false, dx, dy, device);
}
// r[i] = in[i].AreDisjoint(pat)  (LifeAPI.hpp:377-386)
template <LifeStateLayout S, LifeStateLayout P>
std::vector<uint8_t> AreDisjointBatch(std::span<const S> in, const P &pat, int device = 0) {
  return detail::pattern_batch(in, words(&pat), true, 0, 0, device);
}
// r[i] = in[i].AreDisjoint(pat, dx, dy)  (LifeAPI.hpp:411-421)
template <LifeStateLayout S, LifeStateLayout P>
std::vector<uint8_t> AreDisjointBatch(std::span<const S> in, const P &pat, int dx, int dy, int device = 0) {
  return detail::pattern_batch(in, words(&pat), true, dx, dy, device);
}

// ---- the per-offset questions: where does the target occur, where can a
// pattern be placed ----
//
// out[i] = in[i].Match(target)  (LifeTarget.hpp:53-55 -> MatchLiveAndDead,
// LifeAPI.hpp:432-435): bit y of column x set iff in[i] contains the target
// moved by (x, y).  out may be the same array as in.
template <LifeStateLayout S, LifeTargetLayout T>
void MatchBatch(std::span<const S> in, const T &target, std::span<S> out, int device = 0) {
  if (out.size() != in.size()) throw Error(LIFEAPI_E_INVALID, "lifeapi: size mismatch");
  const uint64_t *t = words(&target);
  check(lifeapi_match_batch(words(in.data()), t, t + 64, words(out.data()), nullptr, in.size(), device));
}
// r[i] = in[i].Match(target).GetPop(): the number of places the target
// occurs, with no mask brought back
template <LifeStateLayout S, LifeTargetLayout T>
std::vector<uint32_t> MatchCountBatch(std::span<const S> in, const T &target, int device = 0) {
  std::vector<uint32_t> r(in.size());
  const uint64_t *t = words(&target);
  check(lifeapi_match_batch(words(in.data()), t, t + 64, nullptr, r.data(), in.size(), device));
  return r;
}
// out[i] = in[i].Convolve(pattern)  (LifeAPI.hpp:1293-1370)
template <LifeStateLayout S, LifeStateLayout P>
void ConvolveBatch(std::span<const S> in, const P &pattern, std::span<S> out, int device = 0) {
  if (out.size() != in.size()) throw Error(LIFEAPI_E_INVALID, "lifeapi: size mismatch");
  check(lifeapi_convolve_batch(words(in.data()), words(&pattern), words(out.data()), in.size(), device));
}
// out[i] = in[i].InteractionOffsets(other)  (LifeAPI.hpp:1066-1095)
template <LifeStateLayout S, LifeStateLayout P>
void InteractionOffsetsBatch(std::span<const S> in, const P &other, std::span<S> out, int device = 0) {
  if (out.size() != in.size()) throw Error(LIFEAPI_E_INVALID, "lifeapi: size mismatch");
  check(lifeapi_interaction_offsets_batch(words(in.data()), words(&other), words(out.data()), in.size(),
                                          device));
}

// ---- the symmetry layer (Symmetry.hpp) ----
//
// T is a SymmetryTransform and Y a StaticSymmetry: the reference's own enums
// or lifeapi's (the same enumerators in the same order), or their values.
//
// out[i] = in[i].Transformed(t)  (Symmetry.hpp:105-173); out may be in
template <LifeStateLayout S, class T>
void TransformBatch(std::span<const S> in, std::span<S> out, T t, int device = 0) {
  if (out.size() != in.size()) throw Error(LIFEAPI_E_INVALID, "lifeapi: size mismatch");
  check(lifeapi_transform_batch(words(in.data()), words(out.data()), in.size(), static_cast<uint32_t>(t), 0, 0,
                                device));
}
// out[i] = in[i] after Transform(dx, dy, t)  (LifeAPI.hpp:803-806): Move(dx, dy)
// FIRST, then Transform(t).  With t's linear part A that is Transform(t) then
// Move(A (dx, dy)), which is the one launch the library has.
template <LifeStateLayout S, class T>
void TransformBatch(std::span<const S> in, std::span<S> out, int dx, int dy, T t, int device = 0) {
  if (out.size() != in.size()) throw Error(LIFEAPI_E_INVALID, "lifeapi: size mismatch");
  const uint32_t v = static_cast<uint32_t>(t);
  if (v > 15) throw Error(LIFEAPI_E_INVALID, "lifeapi: no such SymmetryTransform");
  // per transform: 1 = the axes are exchanged, 2 = x negated, 4 = y negated
  // (A (x, y) = (+-x, +-y), or (+-y, +-x) with the signs on the result's x, y)
  static constexpr uint8_t kLinear[16] = {0, 4, 4, 2, 2, 3, 3, 5, 5, 6, 6, 6, 6, 1, 7, 7};
  const long long x = dx & 63, y = dy & 63;  // (Move wraps)
  const long long ax = (kLinear[v] & 1) ? y : x, ay = (kLinear[v] & 1) ? x : y;
  check(lifeapi_transform_batch(words(in.data()), words(out.data()), in.size(), v,
                                (int)((kLinear[v] & 2) ? -ax : ax), (int)((kLinear[v] & 4) ? -ay : ay), device));
}
// out[i] = Symmetricize(in[i], sym, offset)  (Symmetry.hpp:565-654); out may be in
template <LifeStateLayout S, class Y>
void SymmetricizeBatch(std::span<const S> in, std::span<S> out, Y sym, std::pair<int, int> offset, int device = 0) {
  if (out.size() != in.size()) throw Error(LIFEAPI_E_INVALID, "lifeapi: size mismatch");
  check(lifeapi_symmetricize_batch(words(in.data()), words(out.data()), in.size(), static_cast<uint32_t>(sym),
                                   offset.first, offset.second, device));
}
// ---- a symmetric search's step with everything per universe: the offsets at
// which the symmetric image would touch the active region, then the state
// symmetricized at the offset chosen for it ----
namespace detail {
inline std::vector<int32_t> offset_words(std::span<const std::pair<int, int>> offsets, size_t n) {
  if (offsets.size() != n) throw Error(LIFEAPI_E_INVALID, "lifeapi: size mismatch");
  std::vector<int32_t> w(2 * n);
  for (size_t i = 0; i < n; ++i) w[2 * i] = offsets[i].first, w[2 * i + 1] = offsets[i].second;
  return w;
}
}  // namespace detail
// out[i] = in[i].Transformed(t).Moved(offsets[i])  (Symmetry.hpp:105-173,
// LifeAPI.hpp:682-735); out may be in
template <LifeStateLayout S, class T>
void TransformBatch(std::span<const S> in, std::span<S> out, T t, std::span<const std::pair<int, int>> offsets,
                    int device = 0) {
  if (out.size() != in.size()) throw Error(LIFEAPI_E_INVALID, "lifeapi: size mismatch");
  const std::vector<int32_t> w = detail::offset_words(offsets, in.size());
  check(lifeapi_transform_offsets_batch(words(in.data()), words(out.data()), in.size(), static_cast<uint32_t>(t),
                                        w.data(), device));
}
// out[i] = Symmetricize(in[i], sym, offsets[i])  (Symmetry.hpp:565-654); out may be in
template <LifeStateLayout S, class Y>
void SymmetricizeBatch(std::span<const S> in, std::span<S> out, Y sym, std::span<const std::pair<int, int>> offsets,
                       int device = 0) {
  if (out.size() != in.size()) throw Error(LIFEAPI_E_INVALID, "lifeapi: size mismatch");
  const std::vector<int32_t> w = detail::offset_words(offsets, in.size());
  check(lifeapi_symmetricize_offsets_batch(words(in.data()), words(out.data()), in.size(),
                                           static_cast<uint32_t>(sym), w.data(), device));
}
// out[i] = a[i].Convolve(b[i].Transformed(t))  (LifeAPI.hpp:1293-1370): both
// operands per universe; b may be a, out may be a or b
template <LifeStateLayout S, class T>
void ConvolvePairBatch(std::span<const S> a, std::span<const S> b, T t, std::span<S> out, int device = 0) {
  if (b.size() != a.size() || out.size() != a.size()) throw Error(LIFEAPI_E_INVALID, "lifeapi: size mismatch");
  check(lifeapi_convolve_pair_batch(words(a.data()), words(b.data()), static_cast<uint32_t>(t), words(out.data()),
                                    a.size(), device));
}
// out[i] = IntersectingOffsets(pat1[i], pat2[i], sym)  (Symmetry.hpp:729-768)
template <LifeStateLayout S, class Y>
void IntersectingOffsetsBatch(std::span<const S> pat1, std::span<const S> pat2, Y sym, std::span<S> out,
                              int device = 0) {
  if (pat2.size() != pat1.size() || out.size() != pat1.size()) throw Error(LIFEAPI_E_INVALID, "lifeapi: size mismatch");
  check(lifeapi_intersecting_offsets_batch(words(pat1.data()), words(pat2.data()), static_cast<uint32_t>(sym),
                                           words(out.data()), pat1.size(), device));
}
// out[i] = IntersectingOffsets(active[i], sym)  (Symmetry.hpp:770-772)
template <LifeStateLayout S, class Y>
void IntersectingOffsetsBatch(std::span<const S> active, Y sym, std::span<S> out, int device = 0) {
  IntersectingOffsetsBatch(active, active, sym, out, device);
}
// out[i] = in[i].Halve() / HalveX() / HalveY()  (Symmetry.hpp:681-709); out may be in
enum class HalveMode : uint32_t { Halve = 0, HalveX = 1, HalveY = 2 };
template <LifeStateLayout S>
void HalveBatch(std::span<const S> in, std::span<S> out, HalveMode mode = HalveMode::Halve, int device = 0) {
  if (out.size() != in.size()) throw Error(LIFEAPI_E_INVALID, "lifeapi: size mismatch");
  check(lifeapi_halve_batch(words(in.data()), words(out.data()), in.size(), static_cast<uint32_t>(mode), device));
}
// out[i] = in[i].Skew(), or with inverse in[i].InvSkew()  (Symmetry.hpp:711-727); out may be in
template <LifeStateLayout S>
void SkewBatch(std::span<const S> in, std::span<S> out, bool inverse = false, int device = 0) {
  if (out.size() != in.size()) throw Error(LIFEAPI_E_INVALID, "lifeapi: size mismatch");
  check(lifeapi_skew_batch(words(in.data()), words(out.data()), in.size(), inverse ? 1 : 0, device));
}
// r[i] = in[i].XYBounds()  (LifeAPI.hpp:446-484)
template <LifeStateLayout S>
std::vector<std::array<int, 4>> XYBoundsBatch(std::span<const S> in, int device = 0) {
  static_assert(sizeof(std::array<int, 4>) == 4 * sizeof(int32_t));
  std::vector<std::array<int, 4>> r(in.size());
  check(lifeapi_bounds_batch(words(in.data()), reinterpret_cast<int32_t *>(r.data()), in.size(), device));
  return r;
}
// SymmetryOrbit's eight transforms in its order (Symmetry.hpp:801-803), as
// SymmetryTransform values: bit i of a mask below stands for kOrbitTransforms[i]
inline constexpr uint32_t kOrbitTransforms[8] = {0, 2, 13, 4, 15, 6, 8, 9};
// r[i] = the mask of in[i].SymmetryOrbitRepresentatives()  (Symmetry.hpp:814-830)
template <LifeStateLayout S>
std::vector<uint8_t> SymmetryOrbitRepresentativesBatch(std::span<const S> in, int device = 0) {
  std::vector<uint8_t> r(in.size());
  check(lifeapi_symmetry_orbit_batch(words(in.data()), nullptr, r.data(), in.size(), device));
  return r;
}
// images[8 i + k] = in[i].Transformed(kOrbitTransforms[k]) moved by minus its
// bounds' (left, top); returns the masks: in[i].SymmetryOrbit()
// (Symmetry.hpp:798-812) is the images of mask i's set bits, in order
template <LifeStateLayout S>
std::vector<uint8_t> SymmetryOrbitBatch(std::span<const S> in, std::span<S> images, int device = 0) {
  if (images.size() != 8 * in.size()) throw Error(LIFEAPI_E_INVALID, "lifeapi: size mismatch");
  std::vector<uint8_t> r(in.size());
  check(lifeapi_symmetry_orbit_batch(words(in.data()), words(images.data()), r.data(), in.size(), device));
  return r;
}

// ---- connected components (LifeAPI.hpp:301-323, 655-676, 1184-1193) ----
//
// A corona is any LifeState-layout value; the overloads without one use the
// reference's default (b3o$5o$5o$5o$b3o! at (-2, -2)).
//
// r[i] = in[i].FirstOn()  (LifeAPI.hpp:301-323); (-1, -1) for the empty state
template <LifeStateLayout S>
std::vector<std::pair<int, int>> FirstOn(std::span<const S> in, int device = 0) {
  std::vector<int32_t> cells(2 * in.size());
  check(lifeapi_first_on_batch(words(in.data()), cells.data(), in.size(), device));
  std::vector<std::pair<int, int>> r(in.size());
  for (size_t i = 0; i < in.size(); ++i) r[i] = {cells[2 * i], cells[2 * i + 1]};
  return r;
}
namespace detail {
template <LifeStateLayout S>
std::vector<S> component_containing(std::span<const S> states, const S *seeds, bool per, const uint64_t *corona,
                                    int device) {
  std::vector<S> out(states.size());
  check(lifeapi_component_containing_batch(words(states.data()), words(seeds), per, corona, words(out.data()),
                                           states.size(), device));
  return out;
}
template <LifeStateLayout S>
std::vector<uint32_t> component_counts(std::span<const S> states, const uint64_t *corona, int device) {
  std::vector<uint32_t> counts(states.size());
  check(lifeapi_components_batch(words(states.data()), corona, counts.data(), nullptr, 0, states.size(), device));
  return counts;
}
// the counts first, then one call sized by their maximum
template <LifeStateLayout S>
std::vector<std::vector<S>> components(std::span<const S> states, const uint64_t *corona, int device) {
  const std::vector<uint32_t> counts = component_counts(states, corona, device);
  uint32_t cap = 0;
  for (uint32_t c : counts) cap = c > cap ? c : cap;
  std::vector<std::vector<S>> r(states.size());
  if (cap == 0) return r;
  std::vector<S> flat(states.size() * size_t(cap));
  check(lifeapi_components_batch(words(states.data()), corona, nullptr, words(flat.data()), cap, states.size(),
                                 device));
  for (size_t i = 0; i < states.size(); ++i)
    r[i].assign(flat.begin() + i * size_t(cap), flat.begin() + i * size_t(cap) + counts[i]);
  return r;
}
}  // namespace detail
// r[i] = states[i].ComponentContaining(seed[, corona])  (LifeAPI.hpp:655-665, 1184-1188): one seed for the batch
template <LifeStateLayout S>
std::vector<S> ComponentContaining(std::span<const S> states, const S &seed, int device = 0) {
  return detail::component_containing(states, &seed, false, nullptr, device);
}
template <LifeStateLayout S, LifeStateLayout C>
std::vector<S> ComponentContaining(std::span<const S> states, const S &seed, const C &corona, int device = 0) {
  return detail::component_containing(states, &seed, false, words(&corona), device);
}
// r[i] = states[i].ComponentContaining(seeds[i][, corona])
template <LifeStateLayout S>
std::vector<S> ComponentContaining(std::span<const S> states, std::span<const S> seeds, int device = 0) {
  if (seeds.size() != states.size()) throw Error(LIFEAPI_E_INVALID, "lifeapi: size mismatch");
  return detail::component_containing(states, seeds.data(), true, nullptr, device);
}
template <LifeStateLayout S, LifeStateLayout C>
std::vector<S> ComponentContaining(std::span<const S> states, std::span<const S> seeds, const C &corona,
                                   int device = 0) {
  if (seeds.size() != states.size()) throw Error(LIFEAPI_E_INVALID, "lifeapi: size mismatch");
  return detail::component_containing(states, seeds.data(), true, words(&corona), device);
}
// r[i] = states[i].Components([corona]).size()  (LifeAPI.hpp:667-676), with no component brought back
template <LifeStateLayout S>
std::vector<uint32_t> ComponentCounts(std::span<const S> states, int device = 0) {
  return detail::component_counts(states, nullptr, device);
}
template <LifeStateLayout S, LifeStateLayout C>
std::vector<uint32_t> ComponentCounts(std::span<const S> states, const C &corona, int device = 0) {
  return detail::component_counts(states, words(&corona), device);
}
// r[i] = states[i].Components([corona])  (LifeAPI.hpp:667-676, 1189-1193), in
// the reference's order.  The corona must contain cell (0, 0) (the reference
// does not terminate otherwise): lifeapi::Error with LIFEAPI_E_INVALID.
template <LifeStateLayout S>
std::vector<std::vector<S>> Components(std::span<const S> states, int device = 0) {
  return detail::components(states, nullptr, device);
}
template <LifeStateLayout S, LifeStateLayout C>
std::vector<std::vector<S>> Components(std::span<const S> states, const C &corona, int device = 0) {
  return detail::components(states, words(&corona), device);
}

// ---- making LifeWelds and what a search derives from them ----
//
// welds[i] = LifeWeld::FromRequired(states[i], required)  (LifeWeld.hpp:133-159)
template <LifeWeldLayout W, LifeStateLayout S>
std::vector<W> WeldFromRequiredBatch(std::span<const S> states, const S &required, int device = 0) {
  std::vector<W> welds(states.size());
  check(lifeapi_weld_from_required_batch(words(states.data()), words(&required), 0, words(welds.data()),
                                         states.size(), device));
  return welds;
}
// ... with required[i] for states[i]
template <LifeWeldLayout W, LifeStateLayout S>
std::vector<W> WeldFromRequiredBatch(std::span<const S> states, std::span<const S> required, int device = 0) {
  if (required.size() != states.size()) throw Error(LIFEAPI_E_INVALID, "lifeapi: size mismatch");
  std::vector<W> welds(states.size());
  check(lifeapi_weld_from_required_batch(words(states.data()), words(required.data()), 1, words(welds.data()),
                                         states.size(), device));
  return welds;
}

// targets[i] = welds[i].ToTarget()  (LifeWeld.hpp:188-191)
template <LifeTargetLayout T, LifeWeldLayout W>
std::vector<T> WeldToTargetBatch(std::span<const W> welds, int device = 0) {
  const size_t n = welds.size();
  std::vector<uint64_t> wanted(n * 64), unwanted(n * 64);
  check(lifeapi_weld_to_target_batch(words(welds.data()), wanted.data(), unwanted.data(), n, device));
  std::vector<T> targets(n);
  for (size_t i = 0; i < n; ++i) {
    uint64_t *t = words(&targets[i]);
    std::copy_n(wanted.data() + i * 64, 64, t);
    std::copy_n(unwanted.data() + i * 64, 64, t + 64);
  }
  return targets;
}

namespace detail {
template <LifeStableLayout B, LifeWeldLayout W>
std::vector<B> weld_to_stable(std::span<const W> welds, const uint64_t *active, int per, const uint64_t *mask,
                              unsigned duration, int device) {
  std::vector<B> stables(welds.size());
  check(lifeapi_weld_to_stable_batch(words(welds.data()), active, per, mask, duration, words(stables.data()),
                                     welds.size(), device));
  return stables;
}
}  // namespace detail

// stables[i] = welds[i].ToStable()  (LifeWeld.hpp:279-325), ready for PropagateBatch
template <LifeStableLayout B, LifeWeldLayout W>
std::vector<B> WeldToStableBatch(std::span<const W> welds, int device = 0) {
  return detail::weld_to_stable<B>(welds, nullptr, 0, nullptr, 0, device);
}
// stables[i] = welds[i].ToStable(active, duration[, mask])  (LifeWeld.hpp:327-400)
template <LifeStableLayout B, LifeWeldLayout W, LifeStateLayout S>
std::vector<B> WeldToStableBatch(std::span<const W> welds, const S &active, unsigned duration, int device = 0) {
  return detail::weld_to_stable<B>(welds, words(&active), 0, nullptr, duration, device);
}
template <LifeStableLayout B, LifeWeldLayout W, LifeStateLayout S>
std::vector<B> WeldToStableBatch(std::span<const W> welds, const S &active, unsigned duration, const S &mask,
                                 int device = 0) {
  return detail::weld_to_stable<B>(welds, words(&active), 0, words(&mask), duration, device);
}
// ... with active[i] for welds[i]
template <LifeStableLayout B, LifeWeldLayout W, LifeStateLayout S>
std::vector<B> WeldToStableBatch(std::span<const W> welds, std::span<const S> active, unsigned duration,
                                 int device = 0) {
  if (active.size() != welds.size()) throw Error(LIFEAPI_E_INVALID, "lifeapi: size mismatch");
  return detail::weld_to_stable<B>(welds, words(active.data()), 1, nullptr, duration, device);
}
template <LifeStableLayout B, LifeWeldLayout W, LifeStateLayout S>
std::vector<B> WeldToStableBatch(std::span<const W> welds, std::span<const S> active, unsigned duration,
                                 const S &mask, int device = 0) {
  if (active.size() != welds.size()) throw Error(LIFEAPI_E_INVALID, "lifeapi: size mismatch");
  return detail::weld_to_stable<B>(welds, words(active.data()), 1, words(&mask), duration, device);
}

// out[i] = welds[i].InteractionOffsets(other)  (LifeWeld.hpp:206-245)
template <LifeStateLayout S, LifeWeldLayout W>
std::vector<S> WeldInteractionOffsetsBatch(std::span<const W> welds, const W &other, int device = 0) {
  std::vector<S> out(welds.size());
  check(lifeapi_weld_interaction_offsets_batch(words(welds.data()), words(&other), words(out.data()), welds.size(),
                                               device));
  return out;
}

// ---- completing still lifes ----
//
// LifeStable::CompletionResult (LifeStable.hpp:128-132) in the reference's
// order, then the two results only the batched search has: a search that
// needed more than max_depth frames, and useSeed with an empty seed.
enum class CompletionResult : uint8_t { COMPLETED = 0, INCONSISTENT = 1, TIMEOUT = 2, TOO_DEEP = 3, BAD_SEED = 4 };

template <LifeStateLayout L>
struct Completions {
  std::vector<CompletionResult> result;
  std::vector<L> best;          // LifeState() unless COMPLETED
  std::vector<uint64_t> nodes;  // entries of CompleteStableStep
};

namespace detail {
template <LifeStableLayout S, LifeStateLayout L>
Completions<L> complete_stable(std::span<const S> s, bool minimise, const uint64_t *seeds, int per, uint64_t node_budget,
                               uint32_t max_depth, int device) {
  const size_t n = s.size();
  Completions<L> c{std::vector<CompletionResult>(n), std::vector<L>(n), std::vector<uint64_t>(n)};
  static_assert(sizeof(CompletionResult) == 1);
  check(lifeapi_stable_complete_batch(words(s.data()), seeds, per,
                                      (minimise ? LIFEAPI_COMPLETE_MINIMISE : 0u) | (seeds ? LIFEAPI_COMPLETE_USE_SEED : 0u),
                                      node_budget, max_depth, words(c.best.data()),
                                      reinterpret_cast<uint8_t *>(c.result.data()), c.nodes.data(), n, device));
  return c;
}
}  // namespace detail

// s[i].CompleteStable(timeout, minimise[, true, seed]) (LifeStable.hpp:1414-1458)
// with a per-object node budget (0 = 65536) in place of the timeout: see
// lifeapi_stable_complete_batch_dev for where the budget is read, the quirks
// kept and the three cases defined.  s is not changed.
template <LifeStableLayout S, LifeStateLayout L>
Completions<L> CompleteStableBatch(std::span<const S> s, bool minimise = false, uint64_t node_budget = 0,
                                   uint32_t max_depth = 64) {
  return detail::complete_stable<S, L>(s, minimise, nullptr, 0, node_budget, max_depth, 0);
}
// ... useSeed, one seed for the batch
template <LifeStableLayout S, LifeStateLayout L>
Completions<L> CompleteStableBatch(std::span<const S> s, bool minimise, uint64_t node_budget, uint32_t max_depth,
                                   const L &seed) {
  return detail::complete_stable<S, L>(s, minimise, words(&seed), 0, node_budget, max_depth, 0);
}
// ... useSeed, seeds[i] for s[i]
template <LifeStableLayout S, LifeStateLayout L>
Completions<L> CompleteStableBatch(std::span<const S> s, bool minimise, uint64_t node_budget, uint32_t max_depth,
                                   std::span<const L> seeds) {
  if (seeds.size() != s.size()) throw Error(LIFEAPI_E_INVALID, "lifeapi: size mismatch");
  return detail::complete_stable<S, L>(s, minimise, words(seeds.data()), 1, node_budget, max_depth, 0);
}

// weld.UnweldableMask(other, startingGood, startingBad) (LifeWeld.hpp:247-277):
// the offsets at which `other` cannot be placed next to `weld` -- those that
// interact, startingBad, and of the rest (outside startingGood) those whose
// placement weld | other.Moved(cell) has no stable completion.  The reference
// gives each placement's CompleteStable 0.05 s; here it gets node_budget nodes
// (0 = 65536).  As there, only INCONSISTENT marks a cell: a placement whose
// search times out (or needs more than 64 frames) stays unmarked.  The
// placements are built here, and go through WeldToStable and CompleteStable
// as one batch of at most 4096.
template <LifeWeldLayout W, LifeStateLayout L>
L UnweldableMask(const W &weld, const W &other, const L &startingGood, const L &startingBad, uint64_t node_budget = 0) {
  L bad;
  uint64_t *kb = words(&bad);
  check(lifeapi_weld_interaction_offsets_batch(words(&weld), words(&other), kb, 1, 0));
  const uint64_t *good = words(&startingGood), *sb = words(&startingBad), *a = words(&weld), *b = words(&other);
  std::vector<std::pair<unsigned, unsigned>> cells;
  for (unsigned x = 0; x < 64; ++x) {
    kb[x] |= sb[x];
    for (uint64_t m = ~good[x] & ~kb[x]; m; m &= m - 1) cells.push_back({x, (unsigned)std::countr_zero(m)});
  }
  if (cells.empty()) return bad;
  std::vector<W> placed(cells.size());
  for (size_t i = 0; i < cells.size(); ++i) {
    uint64_t *p = words(&placed[i]);
    const auto [x, y] = cells[i];
    for (unsigned k = 0; k < 4 * 64; ++k)  // weld | other.Moved(cell), plane by plane
      p[(k & ~63u) | ((k + x) & 63u)] = a[(k & ~63u) | ((k + x) & 63u)] | std::rotl(b[k], (int)y);
  }
  struct alignas(64) Stable {
    uint64_t planes[10 * 64];
  };
  const std::vector<Stable> stables = WeldToStableBatch<Stable, W>(std::span<const W>(placed));
  const Completions<L> c = CompleteStableBatch<Stable, L>(std::span<const Stable>(stables), false, node_budget, 64);
  for (size_t i = 0; i < cells.size(); ++i)
    if (c.result[i] == CompletionResult::INCONSISTENT) kb[cells[i].first] |= 1ull << cells[i].second;
  return bad;
}

// The search-loop idiom over a batch, in place (LifeAPI.hpp:1196-1216,
// LifeTarget.hpp:44-51):
//     for (unsigned g = 1; g <= gens; ++g) { s.Step(); if (!first && s.Contains(target)) first = g; }
// returns first (0 = never) per state; the states end Stepped(gens).
template <LifeStateLayout S, LifeTargetLayout T>
std::vector<uint32_t> StepContainsBatch(std::span<S> states, const T &target, unsigned gens, int device = 0) {
  std::vector<uint32_t> first(states.size());
  const uint64_t *t = words(&target);
  check(lifeapi_step_contains_batch(words(states.data()), words(states.data()), t, t + 64, first.data(),
                                    states.size(), gens, device));
  return first;
}

// The search loop with the offset test s.Contains(target, dx, dy)
// (LifeTarget.hpp:38-42) in place of s.Contains(target).
template <LifeStateLayout S, LifeTargetLayout T>
std::vector<uint32_t> StepContainsBatch(std::span<S> states, const T &target, int dx, int dy, unsigned gens,
                                        int device = 0) {
  uint64_t t[128];
  std::vector<uint32_t> first(states.size());
  if (!detail::moved_target(words(&target), dx, dy, t)) {  // never contained: step only
    check(lifeapi_step_batch(words(states.data()), words(states.data()), states.size(), gens, device));
    return first;
  }
  check(lifeapi_step_contains_batch(words(states.data()), words(states.data()), t, t + 64, first.data(),
                                    states.size(), gens, device));
  return first;
}

// LifeState::Parse of every string (Parsing.hpp:143-198).  status (optional)
// gets lifeapi_parse_rle_batch's per-pattern bits: 1 = a live cell off the
// 64x64 board was dropped (the reference writes out of bounds there), 2 =
// stopped at a "$" count of 129.
template <LifeStateLayout S>
std::vector<S> ParseBatch(std::span<const std::string> rles, std::vector<uint8_t> *status = nullptr,
                          int device = 0) {
  std::vector<uint64_t> offs(rles.size() + 1, 0);
  std::string blob;
  for (size_t i = 0; i < rles.size(); ++i) {
    blob += rles[i];
    offs[i + 1] = blob.size();
  }
  std::vector<S> out(rles.size());
  std::vector<uint8_t> st(rles.size());
  check(lifeapi_parse_rle_batch(blob.c_str(), offs.data(), rles.size(), words(out.data()), st.data(),
                                device));
  if (status) *status = std::move(st);
  return out;
}

// s.RLE() for every state (Parsing.hpp:8-63,200-204)
template <LifeStateLayout S>
std::vector<std::string> RLEBatch(std::span<const S> states, int device = 0) {
  std::vector<uint64_t> offs(states.size() + 1, 0);
  check(lifeapi_rle_batch(words(states.data()), states.size(), nullptr, 0, offs.data(), device));
  std::string text(offs.back(), '\0');
  check(lifeapi_rle_batch(words(states.data()), states.size(), text.data(), text.size(), offs.data(),
                          device));
  std::vector<std::string> out(states.size());
  for (size_t i = 0; i < states.size(); ++i) out[i] = text.substr(offs[i], offs[i + 1] - offs[i]);
  return out;
}

inline int DeviceCount() { return lifeapi_device_count(); }

// Page-locks a caller-owned array for its lifetime (lifeapi_host_register).
// Calls moving 8 MiB or more pin pageable arrays themselves; a HostPin holds
// the pin across the calls of a search loop and covers smaller batches.
class HostPin {
 public:
  HostPin(void *p, size_t bytes) : p_(p) { check(lifeapi_host_register(p, bytes)); }
  template <class T>
  explicit HostPin(std::span<T> s) : HostPin(static_cast<void *>(s.data()), s.size_bytes()) {}
  HostPin(const HostPin &) = delete;
  HostPin &operator=(const HostPin &) = delete;
  ~HostPin() { (void)lifeapi_host_unregister(p_); }

 private:
  void *p_;
};

}  // namespace lifeapi
