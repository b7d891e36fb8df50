// components_facade_test.cpp -- CPU: the facade's single-universe members
// FirstOn, FirstCell, ComponentContaining and Components
// (lifeapi/LifeState.hpp) against the reference's recorded answers.
//
//   components_facade_test CASES      (the file of components_cases.hpp)
// Needs no GPU and links nothing but the C++ runtime.
#include "components_cases.hpp"

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

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  const cases::File c = cases::read(argv[1]);
  const LifeState dflt = LifeState::DefaultCorona();
  CHECK(dflt.GetPop() == 21 && dflt.Get(0, 0) && dflt.Get(62, 1) && !dflt.Get(62, 2) && dflt.Get(1, 62),
        "DefaultCorona");

  for (size_t k = 0; k < c.firsts.size(); ++k) {
    const cases::First &f = c.firsts[k];
    const std::pair<int, int> got = f.in.FirstOn();
    CHECK(got.first == f.x && got.second == f.y, "FirstOn case %zu: (%d, %d), want (%d, %d)", k, got.first,
          got.second, int(f.x), int(f.y));
    const LifeState cell = f.in.FirstCell();
    CHECK(f.x < 0 ? cell.IsEmpty() : cell == LifeState::Cell({int(f.x), int(f.y)}), "FirstCell case %zu", k);
  }

  size_t defaults = 0;
  for (size_t k = 0; k < c.containing.size(); ++k) {
    const cases::Containing &m = c.containing[k];
    CHECK(m.in.ComponentContaining(m.seed, m.corona) == m.out, "ComponentContaining case %zu", k);
    if (m.corona == dflt) {
      CHECK(m.in.ComponentContaining(m.seed) == m.out, "ComponentContaining (default corona) case %zu", k);
      ++defaults;
    }
  }
  CHECK(defaults > 0, "no default-corona ComponentContaining case");

  defaults = 0;
  for (size_t k = 0; k < c.parts.size(); ++k) {
    const cases::Parts &m = c.parts[k];
    const std::vector<LifeState> got = m.in.Components(m.corona);
    bool same = got.size() == m.parts.size();
    for (size_t i = 0; same && i < got.size(); ++i) same = got[i] == m.parts[i];
    CHECK(same, "Components case %zu: %zu components, want %zu", k, got.size(), m.parts.size());
    if (m.corona == dflt) {
      CHECK(m.in.Components() == got, "Components() case %zu", k);
      ++defaults;
    }
  }
  CHECK(defaults > 0, "no default-corona Components case");

  // a corona without (0, 0): ComponentContaining runs, Components refuses
  LifeState hollow = dflt;
  hollow.Erase(0, 0);
  bool thrown = false;
  try {
    (void)c.parts[0].in.Components(hollow);
  } catch (const std::invalid_argument &) {
    thrown = true;
  }
  CHECK(thrown, "Components without (0, 0) must throw");

  if (failures == 0)
    std::printf("components_facade_test: ok (%zu cells, %zu seeds, %zu lists)\n", c.firsts.size(),
                c.containing.size(), c.parts.size());
  return failures ? 1 : 0;
}
