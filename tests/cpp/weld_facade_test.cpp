// weld_facade_test.cpp -- CPU: the facade's single-object LifeWeld members
// FromRequired, ToTarget, ToStable, InteractionOffsets, AllFrozen, operator|
// and Moved (lifeapi/LifeState.hpp) against the reference's recorded answers.
//
//   weld_facade_test CASES      (the file of weld_cases.hpp)
// Needs no GPU and links nothing but the C++ runtime.
#include "weld_cases.hpp"

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

  for (size_t k = 0; k < c.required.size(); ++k)
    CHECK(LifeWeld::FromRequired(c.required[k].state, c.required[k].required) == c.required[k].weld,
          "FromRequired case %zu", k);

  for (size_t k = 0; k < c.statics.size(); ++k) {
    const cases::Static &m = c.statics[k];
    const LifeTarget t = m.weld.ToTarget();
    CHECK(t.wanted == m.target.wanted && t.unwanted == m.target.unwanted, "ToTarget case %zu", k);
    CHECK(m.weld.ToStable() == m.stable, "ToStable() case %zu", k);
    CHECK(m.weld.ToStable(c.replays[0].active, 0, c.replays[0].mask) == m.stable, "ToStable(.., 0, ..) case %zu", k);
    CHECK(m.weld.AllFrozen() == (m.weld.frozen2 | m.weld.frozen1 | m.weld.frozen0), "AllFrozen case %zu", k);
    // Moved commutes with everything here, across both seams
    const std::pair<int, int> v{int(k * 7 % 64), int(k * 13 % 64)};
    const LifeTarget mt = m.weld.Moved(v).ToTarget();
    CHECK(mt.wanted == t.wanted.Moved(v) && mt.unwanted == t.unwanted.Moved(v), "Moved case %zu", k);
    CHECK((m.weld | m.weld) == m.weld && (m.weld | LifeWeld{}) == m.weld, "operator| case %zu", k);
  }
  const LifeWeld both = c.statics[0].weld | c.statics[1].weld;
  CHECK(both.state == (c.statics[0].weld.state | c.statics[1].weld.state) &&
            both.frozen0 == (c.statics[0].weld.frozen0 | c.statics[1].weld.frozen0),
        "operator| of two welds");

  size_t defaults = 0;
  for (size_t k = 0; k < c.replays.size(); ++k) {
    const cases::Replay &m = c.replays[k];
    CHECK(m.weld.ToStable(m.active, unsigned(m.duration), m.mask) == m.stable, "ToStable case %zu (duration %u)", k,
          unsigned(m.duration));
    if (m.mask == ~LifeState()) {
      CHECK(m.weld.ToStable(m.active, unsigned(m.duration)) == m.stable, "ToStable (default mask) case %zu", k);
      ++defaults;
    }
  }
  CHECK(defaults > 0, "no default-mask ToStable case");

  for (size_t k = 0; k < c.offsets.size(); ++k)
    CHECK(c.offsets[k].weld.InteractionOffsets(c.offsets[k].other) == c.offsets[k].out, "InteractionOffsets case %zu",
          k);

  if (failures == 0)
    std::printf("weld_facade_test: ok (%zu pairs, %zu welds, %zu replays, %zu offsets)\n", c.required.size(),
                c.statics.size(), c.replays.size(), c.offsets.size());
  return failures ? 1 : 0;
}
