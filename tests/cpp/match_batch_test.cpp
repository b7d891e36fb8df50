// match_batch_test.cpp -- the batched Match / Convolve / InteractionOffsets
// of lifeapi/batch.hpp against the facade's own single-universe CPU members
// (lifeapi/LifeState.hpp), every universe of a seeded batch.  The Python
// tests (tests/test_gpu_match.py) pin the GPU entry points to the reference's
// recorded outputs, so agreement here pins the CPU members too, on the inputs
// used here and as far as those inputs tell answers apart: Match on dense
// soups and on the near misses of two targets (one wrong care cell each),
// Convolve on sparse soups, InteractionOffsets on dense soups, whose masks
// are all but full and pin little, and on sparse soups with clusters, whose
// masks are between 5 % and 95 % full.  Needs a GPU; run by
// tests/test_gpu_match.py.  Exit status = number of failed checks.
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

// sparse with clusters: a soup of 1/128 density (seven RandomStates ANDed,
// without the row that RandomState always sets) and two 4 x 4 half-density
// boxes at seeded places, the first across both seams in every eighth universe
static std::vector<LifeState> SparseWithClusters(uint64_t seed) {
  std::vector<LifeState> v(kN);
  for (size_t i = 0; i < kN; ++i) {
    LifeState s = LifeState::RandomState(seed);
    for (int k = 0; k < 6; ++k) s &= LifeState::RandomState(seed);
    for (int x = 0; x < 64; ++x) s.state[x] &= (uint64_t(1) << 61) - 1;
    for (int box = 0; box < 2; ++box) {
      const LifeState r = LifeState::RandomState(seed);
      unsigned x0 = r.state[0] & 63, y0 = (r.state[0] >> 6) & 63;
      if (box == 0 && i % 8 == 0) x0 = 62, y0 = 61 + unsigned(i / 8 % 3);
      for (unsigned c = 0; c < 16; ++c)
        if ((r.state[1] >> c) & 1) s.Set((x0 + c / 4) & 63, (y0 + c % 4) & 63);
    }
    v[i] = s;
  }
  return v;
}

// t.wanted moved by (dx, dy) with all else dead, which matches at (dx, dy),
// then one universe per care cell of t with that cell alone flipped
static std::vector<LifeState> NearMisses(const LifeTarget &t, int dx, int dy) {
  const LifeState base = t.wanted.Moved(dx, dy), care = t.wanted | t.unwanted;
  std::vector<LifeState> v{base};
  for (unsigned x = 0; x < 64; ++x)
    for (unsigned y = 0; y < 64; ++y)
      if (care.Get(x, y)) {
        LifeState s = base;
        s.state[(x + dx) & 63] ^= uint64_t(1) << ((y + dy) & 63);
        v.push_back(s);
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
  // near misses of the block with its ring (moved across both seams) and of
  // the 3 + 5 care cells: only the first universe matches at the planted offset
  const int at[2][3] = {{0, 43, 33}, {2, 50, 9}};
  for (const auto &[k, dx, dy] : at) {
    const LifeTarget t = Targets()[k];
    const std::vector<LifeState> miss = NearMisses(t, dx, dy);
    EXPECT_EQ(miss.size(), size_t(1) + (t.wanted | t.unwanted).GetPop());
    std::vector<LifeState> got(miss.size());
    lifeapi::MatchBatch(std::span<const LifeState>(miss), t, std::span(got));
    for (size_t i = 0; i < miss.size(); ++i) {
      EXPECT_EQ(got[i], miss[i].Match(t));
      EXPECT_EQ(got[i].Get(dx, dy), i == 0);
      EXPECT_EQ(miss[i].Match(t).Get(dx, dy), i == 0);
    }
  }
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
  // sparse universes with clusters: masks that are neither empty nor full, so
  // that a lost term or a wrong threshold of either side would show.  The
  // R-pentomino has live cells of inclusive count 3, 4 and 5.
  in = SparseWithClusters(404);
  for (const LifeState &o : {eater.Moved(62, 62), LifeState::Parse("b2o$2o$bo!").Moved(62, 62)}) {
    lifeapi::InteractionOffsetsBatch(std::span<const LifeState>(in), o, std::span(out));
    size_t mixed = 0;
    for (size_t i = 0; i < kN; ++i) {
      const LifeState want = in[i].InteractionOffsets(o);
      EXPECT_EQ(out[i], want);
      mixed += want.GetPop() >= 4096 / 20 && want.GetPop() <= 4096 - 4096 / 20;
    }
    EXPECT_TRUE(mixed >= kN * 9 / 10);
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
