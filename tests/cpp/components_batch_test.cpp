// components_batch_test.cpp -- GPU: the batched component templates of
// lifeapi/batch.hpp (FirstOn, ComponentContaining with one seed and with a seed
// per universe, ComponentCounts, Components) on a type shaped like the
// reference's LifeState, against the reference's recorded answers.
//
//   components_batch_test CASES       (the file of components_cases.hpp)
#include "components_cases.hpp"

#include <lifeapi/batch.hpp>

#include <cstring>

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

// the reference's layout (LifeAPI.hpp:39-40) with none of its members
struct alignas(64) RefState {
  uint64_t state[64];
};
static RefState ref(const LifeState &s) {
  RefState r;
  std::memcpy(r.state, s.state, sizeof r.state);
  return r;
}
static bool same(const RefState &a, const LifeState &b) { return std::memcmp(a.state, b.state, sizeof a.state) == 0; }

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  const cases::File c = cases::read(argv[1]);
  const RefState dflt = ref(LifeState::DefaultCorona());
  size_t launches = 0;
  try {
    std::vector<RefState> in;
    for (const cases::First &f : c.firsts) in.push_back(ref(f.in));
    const std::vector<std::pair<int, int>> cells = FirstOn(std::span<const RefState>(in));
    for (size_t k = 0; k < in.size(); ++k)
      CHECK(cells[k].first == c.firsts[k].x && cells[k].second == c.firsts[k].y, "FirstOn universe %zu", k);
    ++launches;

    // seeds per universe: the cases of one corona form one batch
    for (size_t k = 0; k < c.containing.size();) {
      size_t e = k;
      std::vector<RefState> states, seeds;
      for (; e < c.containing.size() && c.containing[e].corona == c.containing[k].corona; ++e) {
        states.push_back(ref(c.containing[e].in));
        seeds.push_back(ref(c.containing[e].seed));
      }
      const RefState corona = ref(c.containing[k].corona);
      const bool is_default = same(dflt, c.containing[k].corona);
      const std::vector<RefState> got =
          is_default ? ComponentContaining(std::span<const RefState>(states), std::span<const RefState>(seeds))
                     : ComponentContaining(std::span<const RefState>(states), std::span<const RefState>(seeds), corona);
      for (size_t u = 0; u < got.size(); ++u) CHECK(same(got[u], c.containing[k + u].out), "ComponentContaining case %zu", k + u);
      // one seed for the batch: the first case's, against the CPU member
      const std::vector<RefState> one = ComponentContaining(std::span<const RefState>(states), seeds[0], corona);
      for (size_t u = 0; u < one.size(); ++u)
        CHECK(same(one[u], c.containing[k + u].in.ComponentContaining(c.containing[k].seed, c.containing[k].corona)),
              "ComponentContaining (one seed) case %zu", k + u);
      if (is_default) {
        const std::vector<RefState> d = ComponentContaining(std::span<const RefState>(states), seeds[0]);
        for (size_t u = 0; u < d.size(); ++u) CHECK(std::memcmp(&d[u], &one[u], sizeof d[u]) == 0, "default corona %zu", u);
        ++launches;
      }
      launches += 2;
      k = e;
    }

    // Components: the cases of one corona form one batch (counts, then the lists)
    for (size_t k = 0; k < c.parts.size();) {
      size_t e = k;
      std::vector<RefState> states;
      for (; e < c.parts.size() && c.parts[e].corona == c.parts[k].corona; ++e) states.push_back(ref(c.parts[e].in));
      const RefState corona = ref(c.parts[k].corona);
      const bool is_default = same(dflt, c.parts[k].corona);
      const std::vector<uint32_t> counts = is_default ? ComponentCounts(std::span<const RefState>(states))
                                                      : ComponentCounts(std::span<const RefState>(states), corona);
      const std::vector<std::vector<RefState>> lists = is_default ? Components(std::span<const RefState>(states))
                                                                  : Components(std::span<const RefState>(states), corona);
      for (size_t u = 0; u < states.size(); ++u) {
        const std::vector<LifeState> &want = c.parts[k + u].parts;
        bool ok = counts[u] == want.size() && lists[u].size() == want.size();
        for (size_t i = 0; ok && i < want.size(); ++i) ok = same(lists[u][i], want[i]);
        CHECK(ok, "Components case %zu: count %u, %zu listed, want %zu", k + u, counts[u], lists[u].size(), want.size());
      }
      launches += 3;
      k = e;
    }

    RefState hollow = dflt;
    hollow.state[0] &= ~uint64_t(1);
    bool thrown = false;
    try {
      (void)ComponentCounts(std::span<const RefState>(in), hollow);
    } catch (const Error &e) {
      thrown = e.code == LIFEAPI_E_INVALID;
    }
    CHECK(thrown, "ComponentCounts without (0, 0) must throw LIFEAPI_E_INVALID");
  } catch (const Error &e) {
    std::fprintf(stderr, "lifeapi::Error %d: %s\n", e.code, e.what());
    return 1;
  }
  if (failures == 0) std::printf("components_batch_test: ok (%zu launches)\n", launches);
  return failures ? 1 : 0;
}
