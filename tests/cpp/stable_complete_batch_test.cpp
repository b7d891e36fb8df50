// stable_complete_batch_test.cpp -- CompleteStableBatch and UnweldableMask of
// lifeapi/batch.hpp on the lifeapi:: structs.
//
//   stable_complete_batch_test          the checks that need no device: empty batches
//                                       succeed, mismatched sizes and bad arguments
//                                       throw LIFEAPI_E_INVALID
//   stable_complete_batch_test CASES    GPU: every recorded case of the file that
//                                       tests/test_stable_complete_facade.py writes --
//     uint64 objects, welds, weld budget; then per object, in words:
//       planes[640] seed[64] then for each of the four flag combinations
//       (minimise | use_seed << 1): result nodes best[64]
//     then per weld case: weld[256] other[256] good[64] bad[64] mask[64]
#include <lifeapi/LifeState.hpp>
#include <lifeapi/batch.hpp>

#include <cstdio>
#include <cstring>
#include <vector>

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

static_assert(sizeof(LifeStable) == 640 * 8 && sizeof(LifeState) == 64 * 8 && sizeof(LifeWeld) == 256 * 8);

struct Run {
  uint64_t result, nodes;
  LifeState best;
};
struct Case {
  LifeStable planes;
  LifeState seed;
  Run run[4];
};
struct WeldCase {
  LifeWeld weld, other;
  LifeState good, bad, mask;
};

static bool read_words(FILE *f, void *to, size_t words) { return std::fread(to, 8, words, f) == words; }

template <class F>
static bool invalid(F &&f) {
  try {
    f();
  } catch (const Error &e) {
    return e.code == LIFEAPI_E_INVALID;
  }
  return false;
}

static void without_a_device() {
  const std::vector<LifeStable> none;
  const std::vector<LifeState> no_seeds;
  const LifeState seed{};
  const std::span<const LifeStable> s(none);
  CHECK((CompleteStableBatch<LifeStable, LifeState>(s).result.empty()), "empty batch");
  CHECK((CompleteStableBatch<LifeStable, LifeState>(s, true, 100, 8, seed).best.empty()), "empty batch, one seed");
  CHECK((CompleteStableBatch<LifeStable, LifeState>(s, true, 100, 8, std::span<const LifeState>(no_seeds)).nodes.empty()),
        "empty batch, a seed per object");
  const std::vector<LifeStable> two(2);
  const std::vector<LifeState> three(3);
  const std::span<const LifeStable> t(two);
  CHECK(invalid([&] { (void)CompleteStableBatch<LifeStable, LifeState>(t, false, 0, 64, std::span<const LifeState>(three)); }),
        "2 objects, 3 seeds must throw LIFEAPI_E_INVALID");
  CHECK(invalid([&] { (void)CompleteStableBatch<LifeStable, LifeState>(t, false, 0, 0); }), "max_depth 0");
  CHECK(invalid([&] { (void)CompleteStableBatch<LifeStable, LifeState>(t, false, 0, 4097); }), "max_depth 4097");
  CHECK(invalid([&] { (void)CompleteStableBatch<LifeStable, LifeState>(t, false, (1ull << 24) + 1, 64); }),
        "a budget above 1 << 24");
  static_assert((int)CompletionResult::COMPLETED == 0 && (int)CompletionResult::INCONSISTENT == 1 &&
                (int)CompletionResult::TIMEOUT == 2 && (int)CompletionResult::TOO_DEEP == 3 &&
                (int)CompletionResult::BAD_SEED == 4);
}

int main(int argc, char **argv) {
  if (argc > 2) return 2;
  try {
    without_a_device();
    if (argc == 1) {
      if (failures == 0) std::printf("stable_complete_batch_test: ok (no device)\n");
      return failures ? 1 : 0;
    }
    FILE *f = std::fopen(argv[1], "rb");
    uint64_t head[3];
    if (!f || !read_words(f, head, 3)) throw std::runtime_error("cannot read the case file");
    std::vector<Case> c(head[0]);
    std::vector<WeldCase> w(head[1]);
    for (Case &k : c) {
      bool ok = read_words(f, &k.planes, 640) && read_words(f, &k.seed, 64);
      for (Run &r : k.run) ok = ok && read_words(f, &r.result, 1) && read_words(f, &r.nodes, 1) && read_words(f, &r.best, 64);
      if (!ok) throw std::runtime_error("short case file");
    }
    for (WeldCase &k : w)
      if (!(read_words(f, &k.weld, 256) && read_words(f, &k.other, 256) && read_words(f, &k.good, 64) &&
            read_words(f, &k.bad, 64) && read_words(f, &k.mask, 64)))
        throw std::runtime_error("short case file");
    std::fclose(f);

    const size_t n = c.size();
    std::vector<LifeStable> s(n);
    std::vector<LifeState> seeds(n);
    for (size_t k = 0; k < n; ++k) s[k] = c[k].planes, seeds[k] = c[k].seed;
    const std::span<const LifeStable> in(s);
    for (int fl = 0; fl < 4; ++fl) {
      const bool minimise = fl & 1;
      const Completions<LifeState> got = (fl & 2) ? CompleteStableBatch<LifeStable, LifeState>(
                                                        in, minimise, 0, 64, std::span<const LifeState>(seeds))
                                                  : CompleteStableBatch<LifeStable, LifeState>(in, minimise);
      for (size_t k = 0; k < n; ++k) {
        CHECK((uint64_t)got.result[k] == c[k].run[fl].result && got.nodes[k] == c[k].run[fl].nodes &&
                  got.best[k] == c[k].run[fl].best,
              "CompleteStableBatch flags %d object %zu", fl, k);
        CHECK(s[k] == c[k].planes, "object %zu was changed", k);
      }
    }
    // one seed for the batch: the object whose own seed it is gives its recorded answer
    for (size_t j = 0; j < n; j += n / 4 ? n / 4 : 1) {
      const Completions<LifeState> got = CompleteStableBatch<LifeStable, LifeState>(in, false, 0, 64, c[j].seed);
      CHECK((uint64_t)got.result[j] == c[j].run[2].result && got.nodes[j] == c[j].run[2].nodes &&
                got.best[j] == c[j].run[2].best,
            "CompleteStableBatch (one seed) %zu", j);
    }
    for (size_t k = 0; k < w.size(); ++k)
      CHECK(UnweldableMask(w[k].weld, w[k].other, w[k].good, w[k].bad, head[2]) == w[k].mask, "UnweldableMask %zu", k);
  } catch (const std::exception &e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 1;
  }
  if (failures == 0) std::printf("stable_complete_batch_test: ok\n");
  return failures ? 1 : 0;
}
