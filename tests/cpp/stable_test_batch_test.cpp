// stable_test_batch_test.cpp -- the batched LifeStable lookahead templates of
// lifeapi/batch.hpp (PropagateStripBatch, TestUnknownsBatch, PropagateAndTestBatch)
// on the lifeapi:: structs.
//
//   stable_test_batch_test          the checks that need no device: empty batches
//                                   succeed, mismatched sizes throw LIFEAPI_E_INVALID
//   stable_test_batch_test CASES    GPU: every recorded case of the file that
//                                   tests/test_stable_test_facade.py writes --
//     uint64 count; then per object, in words:
//       planes[640] column pat[640] pat_flags strip[640] strip_flags
//       tested[640] cells[64] tu[640] tu_flags
//     (PropagateAndTest of planes; PropagateStrip(column) of planes;
//      TestUnknowns(cells) of tested)
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

static_assert(sizeof(LifeStable) == 640 * 8 && sizeof(LifeState) == 64 * 8);

struct Case {
  LifeStable planes, pat, strip, tested, tu;
  LifeState cells;
  uint64_t column, pat_flags, strip_flags, tu_flags;
};

static bool read_words(FILE *f, void *to, size_t words) { return std::fread(to, 8, words, f) == words; }

static std::vector<Case> read_cases(const char *path) {
  FILE *f = std::fopen(path, "rb");
  uint64_t count = 0;
  if (!f || !read_words(f, &count, 1)) throw std::runtime_error("cannot read the case file");
  std::vector<Case> c(count);
  for (Case &k : c) {
    const bool ok = read_words(f, &k.planes, 640) && read_words(f, &k.column, 1) && read_words(f, &k.pat, 640) &&
                    read_words(f, &k.pat_flags, 1) && read_words(f, &k.strip, 640) && read_words(f, &k.strip_flags, 1) &&
                    read_words(f, &k.tested, 640) && read_words(f, &k.cells, 64) && read_words(f, &k.tu, 640) &&
                    read_words(f, &k.tu_flags, 1);
    if (!ok) throw std::runtime_error("short case file");
  }
  std::fclose(f);
  return c;
}

static uint64_t flags(PropagateResult r) { return (r.consistent ? 1u : 0u) | (r.changed ? 2u : 0u); }

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
  std::vector<LifeStable> none;
  std::vector<uint8_t> no_columns;
  std::vector<LifeState> no_cells;
  const LifeState empty{};
  CHECK(PropagateStripBatch(std::span<LifeStable>(none), std::span<const uint8_t>(no_columns)).empty(), "empty strip batch");
  CHECK(TestUnknownsBatch(std::span<LifeStable>(none), empty).empty(), "empty TestUnknowns batch, one mask");
  CHECK(TestUnknownsBatch(std::span<LifeStable>(none), std::span<const LifeState>(no_cells)).empty(),
        "empty TestUnknowns batch, a mask per object");
  CHECK(PropagateAndTestBatch(std::span<LifeStable>(none)).empty(), "empty PropagateAndTest batch");
  std::vector<LifeStable> two(2);
  const std::vector<uint8_t> three_columns(3);
  const std::vector<LifeState> three_cells(3);
  CHECK(invalid([&] { (void)PropagateStripBatch(std::span<LifeStable>(two), std::span<const uint8_t>(three_columns)); }),
        "2 objects, 3 columns must throw LIFEAPI_E_INVALID");
  CHECK(invalid([&] { (void)TestUnknownsBatch(std::span<LifeStable>(two), std::span<const LifeState>(three_cells)); }),
        "2 objects, 3 masks must throw LIFEAPI_E_INVALID");
}

int main(int argc, char **argv) {
  if (argc > 2) return 2;
  try {
    without_a_device();
    if (argc == 1) {
      if (failures == 0) std::printf("stable_test_batch_test: ok (no device)\n");
      return failures ? 1 : 0;
    }
    const std::vector<Case> c = read_cases(argv[1]);
    const size_t n = c.size();
    std::vector<LifeStable> s(n);
    std::vector<uint8_t> columns(n);
    std::vector<LifeState> cells(n);
    for (size_t k = 0; k < n; ++k) s[k] = c[k].planes, columns[k] = (uint8_t)c[k].column, cells[k] = c[k].cells;

    std::vector<PropagateResult> r = PropagateAndTestBatch(std::span<LifeStable>(s));
    for (size_t k = 0; k < n; ++k)
      CHECK(s[k] == c[k].pat && flags(r[k]) == c[k].pat_flags, "PropagateAndTestBatch %zu", k);

    for (size_t k = 0; k < n; ++k) s[k] = c[k].planes;
    r = PropagateStripBatch(std::span<LifeStable>(s), std::span<const uint8_t>(columns));
    for (size_t k = 0; k < n; ++k)
      CHECK(s[k] == c[k].strip && flags(r[k]) == c[k].strip_flags, "PropagateStripBatch %zu", k);

    for (size_t k = 0; k < n; ++k) s[k] = c[k].tested;
    r = TestUnknownsBatch(std::span<LifeStable>(s), std::span<const LifeState>(cells));
    for (size_t k = 0; k < n; ++k)
      CHECK(s[k] == c[k].tu && flags(r[k]) == c[k].tu_flags, "TestUnknownsBatch (a mask per object) %zu", k);

    // one mask for the batch: every object's own mask gives its recorded answer
    // there, and the others are at least left with a defined result
    for (size_t j = 0; j < n; j += n / 4 ? n / 4 : 1) {
      for (size_t k = 0; k < n; ++k) s[k] = c[k].tested;
      r = TestUnknownsBatch(std::span<LifeStable>(s), c[j].cells);
      CHECK(s[j] == c[j].tu && flags(r[j]) == c[j].tu_flags, "TestUnknownsBatch (one mask) %zu", j);
    }
  } catch (const std::exception &e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 1;
  }
  if (failures == 0) std::printf("stable_test_batch_test: ok\n");
  return failures ? 1 : 0;
}
