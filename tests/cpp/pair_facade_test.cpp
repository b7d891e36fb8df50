// pair_facade_test.cpp -- CPU: the facade's IntersectingOffsets, Halve /
// HalveX / HalveY and Skew / InvSkew (lifeapi/LifeState.hpp) against the
// reference's recorded answers.
//
//   pair_facade_test CASES      (the file of pair_cases.hpp)
// Needs no GPU and links nothing but the C++ runtime.
#include "pair_cases.hpp"

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
  const std::vector<cases::Case> all = cases::read(argv[1]);
  size_t seen[4] = {0, 0, 0, 0}, selfs = 0;
  for (const cases::Case &c : all) {
    const int arg = int(c.arg);
    ++seen[c.kind & 3];
    switch (c.kind) {
    case 0:
      CHECK(IntersectingOffsets(c.a, c.b, StaticSymmetry(arg)) == c.out, "IntersectingOffsets(a, b, %d)", arg);
      if (c.a == c.b) {
        CHECK(IntersectingOffsets(c.a, StaticSymmetry(arg)) == c.out, "IntersectingOffsets(active, %d)", arg);
        ++selfs;
      }
      break;
    case 1:
      CHECK(c.a.Convolve(c.b.Transformed(SymmetryTransform(arg))) == c.out, "Convolve(Transformed(%d))", arg);
      // Convolve is symmetric in its operands
      CHECK(c.b.Transformed(SymmetryTransform(arg)).Convolve(c.a) == c.out, "Transformed(%d).Convolve", arg);
      break;
    case 2:
      CHECK((arg == 0 ? c.a.Halve() : arg == 1 ? c.a.HalveX() : c.a.HalveY()) == c.out, "Halve mode %d", arg);
      if (arg == 0) CHECK(c.a.HalveX().HalveY() == c.out && c.a.HalveY().HalveX() == c.out, "Halve = HalveX . HalveY");
      break;
    default:
      CHECK((arg == 0 ? c.a.Skew() : c.a.InvSkew()) == c.out, "Skew inverse %d", arg);
      CHECK((arg == 0 ? c.out.InvSkew() : c.out.Skew()) == c.a, "the other Skew undoes it (%d)", arg);
    }
  }
  CHECK(seen[0] && seen[1] && seen[2] && seen[3] && selfs, "a kind of case is missing");
  if (failures == 0)
    std::printf("pair_facade_test: ok (%zu offsets, %zu self, %zu convolutions, %zu halves, %zu skews)\n", seen[0], selfs,
                seen[1], seen[2], seen[3]);
  return failures ? 1 : 0;
}
