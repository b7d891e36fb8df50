// symmetry_facade_test.cpp -- CPU: the facade's single-universe symmetry
// members (lifeapi/LifeState.hpp) against the reference's recorded answers.
//
//   symmetry_facade_test CASES      (the file of symmetry_cases.hpp)
// Needs no GPU and links nothing but the C++ runtime.
#include "symmetry_cases.hpp"

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
  using enum SymmetryTransform;
  static_assert(uint32_t(ReflectAcrossYeqNegXP1) == 15 && uint32_t(Rotate180OddBoth) == 9);
  static_assert(uint32_t(StaticSymmetry::D4diag) == 17 && uint32_t(StaticSymmetry::D8even) == 20 &&
                uint32_t(StaticSymmetry::C2) == 7);

  for (const cases::Mapped &m : c.transforms) {
    const auto t = SymmetryTransform(m.kind);
    const int dx = int(m.dx), dy = int(m.dy);
    CHECK(m.in.Transformed(t).Moved(dx, dy) == m.out, "Transformed(%d).Moved(%d, %d)", int(m.kind), dx, dy);
    LifeState s = m.in;
    s.Transform(t);
    s.Move(dx, dy);
    CHECK(s == m.out, "Transform(%d); Move(%d, %d)", int(m.kind), dx, dy);
    // the inverse undoes it
    s.Move(-dx, -dy);
    s.Transform(TransformInverse(t));
    CHECK(s == m.in, "TransformInverse(%d)", int(m.kind));
    // Transform(dx, dy, t) moves FIRST: the recorded answer for (t, 0, 0) on the moved input
    if (dx == 0 && dy == 0) {
      LifeState a = m.in.Moved(-3, 11), b = a;
      a.Transform(3, -11, t);
      CHECK(a == m.out, "Transform(3, -11, %d)", int(m.kind));
      b.Transform(3, -10, t);
      CHECK(!(b == m.out), "Transform(3, -10, %d) must differ", int(m.kind));
      // the named primitives
      LifeState p = m.in;
      if (t == Identity) CHECK(p.Transformed(t) == m.in, "Identity");
      if (t == ReflectAcrossXEven) { p.FlipX(); CHECK(p == m.out, "FlipX"); p = m.in; p.BitReverse(); CHECK(p == m.out, "BitReverse"); }
      if (t == ReflectAcrossYEven) { p.FlipY(); CHECK(p == m.out, "FlipY"); }
      if (t == ReflectAcrossYeqX) { p.Transpose(false); CHECK(p == m.out, "Transpose(false)"); }
      if (t == ReflectAcrossYeqNegX) { p.Transpose(true); CHECK(p == m.out, "Transpose(true)"); p = m.in; p.Transpose(); CHECK(p == m.out, "Transpose()"); }
      if (t == Rotate180OddBoth) CHECK(m.in.Mirrored() == m.out, "Mirrored");
      // LifeTarget follows its planes
      LifeTarget target(m.in, ~m.in);
      const LifeTarget moved = target.Transformed(t);
      target.Transform(t);
      CHECK(moved.wanted == m.out && moved.unwanted == ~m.out, "LifeTarget::Transformed(%d)", int(m.kind));
      CHECK(target.wanted == m.out && target.unwanted == ~m.out, "LifeTarget::Transform(%d)", int(m.kind));
    }
  }

  for (const cases::Mapped &m : c.symmetries)
    CHECK(Symmetricize(m.in, StaticSymmetry(m.kind), {int(m.dx), int(m.dy)}) == m.out, "Symmetricize(%d, {%d, %d})",
          int(m.kind), int(m.dx), int(m.dy));
  // PerpComponent: the truncating halves (odd x - y), and offsets beyond one turn
  CHECK(PerpComponent(ReflectAcrossYeqX, {7, -3}) == std::make_pair(5, 59), "PerpComponent YeqX (7, -3)");
  CHECK(PerpComponent(ReflectAcrossYeqX, {-40, 13}) == std::make_pair(37, 26), "PerpComponent YeqX (-40, 13)");
  CHECK(PerpComponent(ReflectAcrossYeqNegXP1, {5, 6}) == std::make_pair(5, 5), "PerpComponent NegXP1 (5, 6)");
  CHECK(PerpComponent(ReflectAcrossX, {5, 6}) == std::make_pair(0, 6), "PerpComponent X");
  CHECK(PerpComponent(ReflectAcrossY, {5, 6}) == std::make_pair(5, 0), "PerpComponent Y");
  CHECK(PerpComponent(Rotate90, {5, 6}) == std::make_pair(5, 6), "PerpComponent default");

  size_t masks_seen = 0;
  for (const cases::Orbit &o : c.orbits) {
    const std::array<int, 4> b = o.in.XYBounds();
    for (int k = 0; k < 4; ++k) CHECK(b[k] == o.bounds[k], "XYBounds[%d] = %d, want %d", k, b[k], int(o.bounds[k]));
    const std::vector<LifeState> orbit = o.in.SymmetryOrbit();
    const std::vector<SymmetryTransform> reps = o.in.SymmetryOrbitRepresentatives();
    size_t next = 0;
    for (int i = 0; i < 8; ++i)
      if (o.mask >> i & 1) {
        CHECK(next < orbit.size() && next < reps.size() && orbit[next] == o.images[i] &&
                  reps[next] == detail::kOrbit[i],
              "orbit image %d of mask %02x", i, unsigned(o.mask));
        ++next;
      }
    CHECK(next == orbit.size() && next == reps.size(), "orbit size %zu, want %zu", orbit.size(), next);
    masks_seen |= size_t(1) << (o.mask & 63);
  }
  CHECK(masks_seen != 0, "no orbit case");
  if (failures == 0)
    std::printf("symmetry_facade_test: ok (%zu transforms, %zu symmetries, %zu orbits)\n", c.transforms.size(),
                c.symmetries.size(), c.orbits.size());
  return failures ? 1 : 0;
}
