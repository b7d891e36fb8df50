// pair_batch_test.cpp -- GPU: the batched templates of lifeapi/batch.hpp for
// IntersectingOffsets, ConvolvePair, Halve, Skew and the per-universe-offset
// overloads of TransformBatch / SymmetricizeBatch, against the reference's
// recorded answers and the facade's CPU members.
//
//   pair_batch_test CASES      (the file of pair_cases.hpp)
#include <lifeapi/batch.hpp>

#include "pair_cases.hpp"

#include <map>

using namespace lifeapi;

static int failures = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      ++failures;                                         \
      std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);                  \
      std::fprintf(stderr, "\n");                         \
    }                                                     \
  } while (0)

static bool same(const std::vector<LifeState> &x, const std::vector<LifeState> &y) {
  if (x.size() != y.size()) return false;
  for (size_t i = 0; i < x.size(); ++i)
    if (!(x[i] == y[i])) return false;
  return true;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  // one launch per (kind, arg): the cases of each, in file order
  struct Group {
    std::vector<LifeState> a, b, out;
  };
  std::map<std::pair<int64_t, int64_t>, Group> groups;
  for (const cases::Case &c : cases::read(argv[1])) {
    Group &g = groups[{c.kind, c.arg}];
    g.a.push_back(c.a);
    g.b.push_back(c.b);
    g.out.push_back(c.out);
  }
  size_t launches = 0;
  for (const auto &[key, g] : groups) {
    const auto [kind, arg] = key;
    std::vector<LifeState> got(g.a.size());
    const std::span<const LifeState> a(g.a), b(g.b);
    if (kind == 0) {
      IntersectingOffsetsBatch(a, b, StaticSymmetry(arg), std::span(got));
      CHECK(same(got, g.out), "IntersectingOffsetsBatch(%d)", int(arg));
    } else if (kind == 1) {
      ConvolvePairBatch(a, b, SymmetryTransform(arg), std::span(got));
      CHECK(same(got, g.out), "ConvolvePairBatch(%d)", int(arg));
      // the value form of the transform, and in place on b
      std::vector<LifeState> inplace = g.b;
      ConvolvePairBatch(a, std::span<const LifeState>(inplace), uint32_t(arg), std::span(inplace));
      CHECK(same(inplace, g.out), "ConvolvePairBatch(%d) in place", int(arg));
    } else if (kind == 2) {
      HalveBatch(a, std::span(got), HalveMode(arg));
      CHECK(same(got, g.out), "HalveBatch(%d)", int(arg));
    } else {
      SkewBatch(a, std::span(got), arg != 0);
      CHECK(same(got, g.out), "SkewBatch(%d)", int(arg));
    }
    ++launches;
  }
  // the self form: IntersectingOffsets(active, sym) of the first operands
  for (const auto &[key, g] : groups)
    if (key.first == 0) {
      std::vector<LifeState> got(g.a.size()), want;
      for (const LifeState &s : g.a) want.push_back(IntersectingOffsets(s, StaticSymmetry(key.second)));
      IntersectingOffsetsBatch(std::span<const LifeState>(g.a), StaticSymmetry(key.second), std::span(got));
      CHECK(same(got, want), "IntersectingOffsetsBatch(active, %d)", int(key.second));
      ++launches;
    }
  // an offset per universe, against the facade's CPU members
  const Group &any = groups.begin()->second;
  std::vector<std::pair<int, int>> offsets;
  for (size_t i = 0; i < any.a.size(); ++i) offsets.push_back({int(i * 7) - 70, 65 - int(i * 5)});
  for (uint32_t sym : {0u, 1u, 3u, 5u, 6u, 7u, 11u, 13u, 17u}) {
    std::vector<LifeState> got(any.a.size()), want;
    for (size_t i = 0; i < any.a.size(); ++i) want.push_back(Symmetricize(any.a[i], StaticSymmetry(sym), offsets[i]));
    SymmetricizeBatch(std::span<const LifeState>(any.a), std::span(got), StaticSymmetry(sym),
                      std::span<const std::pair<int, int>>(offsets));
    CHECK(same(got, want), "SymmetricizeBatch(%u, offsets)", sym);
    ++launches;
  }
  for (uint32_t t = 0; t < 16; ++t) {
    std::vector<LifeState> got(any.a.size()), want;
    for (size_t i = 0; i < any.a.size(); ++i) want.push_back(any.a[i].Transformed(SymmetryTransform(t)).Moved(offsets[i]));
    TransformBatch(std::span<const LifeState>(any.a), std::span(got), SymmetryTransform(t),
                   std::span<const std::pair<int, int>>(offsets));
    CHECK(same(got, want), "TransformBatch(%u, offsets)", t);
    ++launches;
  }
  // sizes must agree
  try {
    std::vector<LifeState> one(1), two(2);
    HalveBatch(std::span<const LifeState>(two), std::span(one));
    CHECK(false, "HalveBatch accepted a size mismatch");
  } catch (const Error &e) {
    CHECK(e.code == LIFEAPI_E_INVALID, "size mismatch code %d", e.code);
  }
  if (failures == 0) std::printf("pair_batch_test: ok (%zu launches)\n", launches);
  return failures ? 1 : 0;
}
