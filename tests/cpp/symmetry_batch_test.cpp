// symmetry_batch_test.cpp -- GPU: the batched symmetry templates of
// lifeapi/batch.hpp (TransformBatch in both forms, SymmetricizeBatch,
// XYBoundsBatch, SymmetryOrbitRepresentativesBatch, SymmetryOrbitBatch) on
// batches of 65 universes against the reference's recorded answers.
//
//   symmetry_batch_test CASES       (the file of symmetry_cases.hpp)
// Cases that share their parameters form one batch, repeated up to 65.
#include "symmetry_cases.hpp"

#include <map>
#include <tuple>

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

constexpr size_t kBatch = 65;
using Key = std::tuple<int64_t, int64_t, int64_t>;

static std::map<Key, std::vector<const cases::Mapped *>> grouped(const std::vector<cases::Mapped> &v) {
  std::map<Key, std::vector<const cases::Mapped *>> g;
  for (const cases::Mapped &m : v) g[{m.kind, m.dx, m.dy}].push_back(&m);
  return g;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  const cases::File c = cases::read(argv[1]);
  std::vector<LifeState> in(kBatch), out(kBatch);
  size_t launches = 0;
  try {
    for (const auto &[key, group] : grouped(c.transforms)) {
      const auto [kind, dx, dy] = key;
      const auto t = SymmetryTransform(kind);
      for (size_t u = 0; u < kBatch; ++u) in[u] = group[u % group.size()]->in;
      if (dx == 0 && dy == 0) {
        TransformBatch(std::span<const LifeState>(in), std::span(out), t);
        for (size_t u = 0; u < kBatch; ++u)
          CHECK(out[u] == group[u % group.size()]->out, "TransformBatch(%d) universe %zu", int(kind), u);
        // move first (LifeAPI.hpp:803-806): against the CPU member, and not the move-after answer
        TransformBatch(std::span<const LifeState>(in), std::span(out), 40, 25, t);
        for (size_t u = 0; u < kBatch; ++u) {
          LifeState want = in[u];
          want.Transform(40, 25, t);
          CHECK(out[u] == want, "TransformBatch(40, 25, %d) universe %zu", int(kind), u);
          CHECK(t == SymmetryTransform::Identity || !(out[u] == in[u].Transformed(t).Moved(40, 25)),
                "TransformBatch(40, 25, %d) moved after", int(kind));
        }
        // in place, the transform given by its value
        std::vector<LifeState> io = in;
        TransformBatch(std::span<const LifeState>(io), std::span(io), uint32_t(kind));
        for (size_t u = 0; u < kBatch; ++u)
          CHECK(io[u] == group[u % group.size()]->out, "TransformBatch in place (%d) universe %zu", int(kind), u);
        launches += 3;
      } else {
        // transform, then move: the C entry point's own form
        check(lifeapi_transform_batch(words(in.data()), words(out.data()), kBatch, uint32_t(kind), int(dx), int(dy), 0));
        for (size_t u = 0; u < kBatch; ++u)
          CHECK(out[u] == group[u % group.size()]->out, "lifeapi_transform_batch(%d, %d, %d) universe %zu", int(kind),
                int(dx), int(dy), u);
        ++launches;
      }
    }
    for (const auto &[key, group] : grouped(c.symmetries)) {
      const auto [kind, dx, dy] = key;
      for (size_t u = 0; u < kBatch; ++u) in[u] = group[u % group.size()]->in;
      SymmetricizeBatch(std::span<const LifeState>(in), std::span(out), StaticSymmetry(kind),
                        std::pair<int, int>(int(dx), int(dy)));
      for (size_t u = 0; u < kBatch; ++u)
        CHECK(out[u] == group[u % group.size()]->out, "SymmetricizeBatch(%d, {%d, %d}) universe %zu", int(kind),
              int(dx), int(dy), u);
      ++launches;
    }
    bool undefined_thrown = false;
    try {
      SymmetricizeBatch(std::span<const LifeState>(in), std::span(out), StaticSymmetry::D8, std::pair<int, int>(0, 0));
    } catch (const Error &e) {
      undefined_thrown = e.code == LIFEAPI_E_INVALID;
    }
    CHECK(undefined_thrown, "SymmetricizeBatch(D8) must throw LIFEAPI_E_INVALID");

    const size_t no = c.orbits.size();
    for (size_t u = 0; u < kBatch; ++u) in[u] = c.orbits[(u * 7) % no].in;
    const std::vector<std::array<int, 4>> bounds = XYBoundsBatch(std::span<const LifeState>(in));
    const std::vector<uint8_t> reps = SymmetryOrbitRepresentativesBatch(std::span<const LifeState>(in));
    std::vector<LifeState> images(8 * kBatch);
    const std::vector<uint8_t> masks = SymmetryOrbitBatch(std::span<const LifeState>(in), std::span(images));
    for (size_t u = 0; u < kBatch; ++u) {
      const cases::Orbit &o = c.orbits[(u * 7) % no];
      for (int k = 0; k < 4; ++k) CHECK(bounds[u][k] == o.bounds[k], "XYBoundsBatch universe %zu [%d]", u, k);
      CHECK(reps[u] == o.mask && masks[u] == o.mask, "orbit mask universe %zu: %02x %02x want %02x", u, reps[u],
            masks[u], unsigned(o.mask));
      for (int i = 0; i < 8; ++i) CHECK(images[8 * u + i] == o.images[i], "orbit image %d universe %zu", i, u);
      // and the CPU members agree with the masks' reading
      const std::vector<SymmetryTransform> kept = in[u].SymmetryOrbitRepresentatives();
      size_t next = 0;
      for (int i = 0; i < 8; ++i)
        if (masks[u] >> i & 1) {
          CHECK(next < kept.size() && uint32_t(kept[next]) == kOrbitTransforms[i], "representative %d universe %zu", i, u);
          ++next;
        }
      CHECK(next == kept.size(), "representatives universe %zu", u);
    }
    launches += 3;
  } catch (const Error &e) {
    std::fprintf(stderr, "lifeapi::Error %d: %s\n", e.code, e.what());
    return 1;
  }
  if (failures == 0) std::printf("symmetry_batch_test: ok (%zu launches of %zu universes)\n", launches, kBatch);
  return failures ? 1 : 0;
}
