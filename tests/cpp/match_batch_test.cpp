// match_batch_test.cpp -- the batched Match / Convolve / InteractionOffsets
// of lifeapi/batch.hpp against the facade's own single-universe CPU members
// (lifeapi/LifeState.hpp), every universe of a seeded batch.  The Python
// tests (tests/test_gpu_match.py) pin the GPU entry points to the reference's
// recorded outputs, so agreement here pins the CPU members too.  Needs a GPU;
// run by tests/test_gpu_match.py.  Exit status = number of failed checks.
#include <lifeapi/LifeState.hpp>

#include <cstdio>
#include <span>
#include <vector>

using lifeapi::LifeState;
using lifeapi::LifeTarget;

static int g_failures = 0, g_checks = 0;
#define EXPECT_TRUE(c)                                                          \
  do {                                                                          \
    ++g_checks;                                                                 \
    if (!(c)) {                                                                 \
      ++g_failures;                                                             \
      if (g_failures < 20) std::fprintf(stderr, "%s:%d: EXPECT_TRUE(%s) failed\n", __FILE__, __LINE__, #c); \
    }                                                                           \
  } while (0)
#define EXPECT_EQ(a, b) EXPECT_TRUE((a) == (b))

static constexpr size_t kN = 1000;

// full density and, every other universe, quarter density
static std::vector<LifeState> Seeded(uint64_t seed) {
  std::vector<LifeState> v(kN);
  for (size_t i = 0; i < kN; ++i) {
    v[i] = LifeState::RandomState(seed);
    if (i & 1) v[i] &= LifeState::RandomState(seed);
  }
  return v;
}

static std::vector<LifeTarget> Targets() {
  std::vector<LifeTarget> t;
  t.emplace_back(LifeState::Parse("2o$2o!").Moved(20, 30));        // block and ring
  t.emplace_back(LifeState::Parse("bo$2bo$3o!").Moved(62, 62));    // glider across both seams
  LifeState w, u;                                                  // 3 live + 5 dead care cells
  w.Set(63, 1), w.Set(0, 63), w.Set(2, 2);
  u.Set(62, 0), u.Set(1, 1), u.Set(1, 62), u.Set(0, 0), u.Set(63, 3);
  t.emplace_back(w, u);
  t.emplace_back(LifeState(), u);                                  // nothing wanted
  t.emplace_back(w, LifeState());                                  // nothing unwanted
  t.emplace_back(LifeState(), LifeState());                        // matches everywhere
  return t;
}

static void MatchBatch_EqualsCpu() {
  const std::vector<LifeState> in = Seeded(101);
  std::vector<LifeState> out(kN);
  for (const LifeTarget &t : Targets()) {
    lifeapi::MatchBatch(std::span<const LifeState>(in), t, std::span(out));
    const std::vector<uint32_t> counts = lifeapi::MatchCountBatch(std::span<const LifeState>(in), t);
    for (size_t i = 0; i < kN; ++i) {
      const LifeState want = in[i].Match(t);
      EXPECT_EQ(out[i], want);
      EXPECT_EQ(counts[i], want.GetPop());
    }
  }
  // the pattern forms: Match(pattern) is the target with its boundary dead
  const LifeState blk = LifeState::Parse("2o$2o!");
  EXPECT_EQ(in[0].Match(blk), in[0].Match(LifeTarget(blk)));
  EXPECT_EQ(in[0].MatchLive(blk), in[0].MatchLiveAndDead(blk, LifeState()));
  // in place
  std::vector<LifeState> io = in;
  lifeapi::MatchBatch(std::span<const LifeState>(io), Targets()[2], std::span(io));
  for (size_t i = 0; i < kN; ++i) EXPECT_EQ(io[i], in[i].Match(Targets()[2]));
}

static void ConvolveBatch_EqualsCpu() {
  const std::vector<LifeState> in = Seeded(202);
  std::vector<LifeState> sparse = in, out(kN);
  for (size_t i = 0; i < kN; ++i) sparse[i] &= in[(i + 1) % kN] & in[(i + 2) % kN] & in[(i + 3) % kN];
  LifeState zoi;
  for (int x = -1; x <= 1; ++x)
    for (int y = -1; y <= 1; ++y) zoi.SetSafe(x, y, true);
  LifeState runs;
  runs.state[9] = ((uint64_t(1) << 40) - 1) << 10;
  runs.state[63] = ~uint64_t(0);
  runs.state[0] = 0x8000000000000001ULL;
  for (const LifeState &p : {zoi, runs, LifeState::Parse("bo$2bo$3o!").Moved(62, 62), LifeState()}) {
    lifeapi::ConvolveBatch(std::span<const LifeState>(sparse), p, std::span(out));
    for (size_t i = 0; i < kN; ++i) EXPECT_EQ(out[i], sparse[i].Convolve(p));
  }
  // Convolve with the 3x3 block is ZOI (LifeAPI.hpp:521-529)
  lifeapi::ConvolveBatch(std::span<const LifeState>(sparse), zoi, std::span(out));
  for (size_t i = 0; i < kN; ++i) EXPECT_EQ(out[i], sparse[i].ZOI());
  // Mirrored twice is the identity, and cell (x, y) goes to (-x, -y)
  EXPECT_EQ(in[0].Mirrored().Mirrored(), in[0]);
  EXPECT_EQ(LifeState::Cell({3, 60}).Mirrored(), LifeState::Cell({61, 4}));
}

static void InteractionOffsetsBatch_EqualsCpu() {
  std::vector<LifeState> in = Seeded(303), out(kN);
  for (size_t i = 0; i < kN; i += 3) in[i] = LifeState::Parse("2o$2o!").Moved(int(i), int(7 * i));
  const LifeState eater = LifeState::Parse("2o$obo$2bo$2b2o!");
  for (const LifeState &o : {eater.Moved(30, 30), eater.Moved(62, 62), LifeState::Parse("bo$2bo$3o!"), LifeState()}) {
    lifeapi::InteractionOffsetsBatch(std::span<const LifeState>(in), o, std::span(out));
    for (size_t i = 0; i < kN; ++i) EXPECT_EQ(out[i], in[i].InteractionOffsets(o));
  }
}

int main() {
  try {
    MatchBatch_EqualsCpu();
    ConvolveBatch_EqualsCpu();
    InteractionOffsetsBatch_EqualsCpu();
  } catch (const lifeapi::Error &e) {
    std::fprintf(stderr, "lifeapi::Error %d: %s\n", e.code, e.what());
    return 100;
  }
  std::printf("%d checks, %d failures\n", g_checks, g_failures);
  return g_failures > 99 ? 99 : g_failures;
}
