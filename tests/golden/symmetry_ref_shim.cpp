// symmetry_ref_shim.cpp -- records the reference's own Transform / Move,
// Symmetricize, XYBounds, SymmetryOrbit and SymmetryOrbitRepresentatives for
// tests/golden/symmetry.npz.  Compiled by tests/golden/make_symmetry_golden.py
// against the reference headers where they lie (never committed or copied),
// into a temporary directory.
//
//   symmetry_ref_shim IN OUT
// IN:  uint64 count; then per operation int64 kind, a, b, c and state[64]
// OUT: per operation, in order:
//   kind 0  state.Transformed(a).Moved(b, c)                      64 words
//   kind 1  Symmetricize(state, a, {b, c})                        64 words
//   kind 2  s = state.Moved(b, c): s, then s.XYBounds() as 4 int64, the eight
//           images Transformed(t).Moved(-left, -top) of SymmetryOrbit's loop in
//           its order, and the mask of the transforms that
//           SymmetryOrbitRepresentatives() returns (bit i = the i-th of that
//           order); SymmetryOrbit() itself is checked to be the images of
//           the mask's bits                                   64 + 4 + 512 + 1
//
// The same translation unit instantiates the batched templates of
// lifeapi/batch.hpp on the reference's ::LifeState, so that they are compiled
// against the reference's types (never called here).
#include <lifeapi/batch.hpp>

#include "LifeAPI.hpp"
#include "Symmetry.hpp"

#include <cstdio>
#include <vector>

template void lifeapi::TransformBatch<::LifeState, ::SymmetryTransform>(std::span<const ::LifeState>,
                                                                        std::span<::LifeState>, ::SymmetryTransform,
                                                                        int);
template void lifeapi::TransformBatch<::LifeState, ::SymmetryTransform>(std::span<const ::LifeState>,
                                                                        std::span<::LifeState>, int, int,
                                                                        ::SymmetryTransform, int);
template void lifeapi::SymmetricizeBatch<::LifeState, ::StaticSymmetry>(std::span<const ::LifeState>,
                                                                        std::span<::LifeState>, ::StaticSymmetry,
                                                                        std::pair<int, int>, int);
template std::vector<std::array<int, 4>> lifeapi::XYBoundsBatch<::LifeState>(std::span<const ::LifeState>, int);
template std::vector<uint8_t> lifeapi::SymmetryOrbitRepresentativesBatch<::LifeState>(std::span<const ::LifeState>,
                                                                                      int);
template std::vector<uint8_t> lifeapi::SymmetryOrbitBatch<::LifeState>(std::span<const ::LifeState>,
                                                                       std::span<::LifeState>, int);

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  uint64_t count;
  if (!f || std::fread(&count, 8, 1, f) != 1) return 3;
  FILE *o = std::fopen(argv[2], "wb");
  if (!o) return 4;
  auto put = [&](const LifeState &r) { std::fwrite(r.state, 8, 64, o); };
  using enum SymmetryTransform;
  const SymmetryTransform order[8] = {Identity, ReflectAcrossX, ReflectAcrossYeqX, ReflectAcrossY,
                                      ReflectAcrossYeqNegXP1, Rotate90, Rotate270, Rotate180OddBoth};
  for (uint64_t k = 0; k < count; ++k) {
    int64_t h[4];
    LifeState s;
    if (std::fread(h, 8, 4, f) != 4 || std::fread(s.state, 8, 64, f) != 64) return 3;
    const int a = (int)h[1], b = (int)h[2], c = (int)h[3];
    if (h[0] == 0) {
      put(s.Transformed((SymmetryTransform)a).Moved(b, c));
    } else if (h[0] == 1) {
      put(Symmetricize(s, (StaticSymmetry)a, {b, c}));
    } else {
      s.Move(b, c);
      put(s);
      const std::array<int, 4> xy = s.XYBounds();
      for (int v : xy) {
        const int64_t w = v;
        std::fwrite(&w, 8, 1, o);
      }
      const std::vector<SymmetryTransform> reps = s.SymmetryOrbitRepresentatives();
      const std::vector<LifeState> orbit = s.SymmetryOrbit();
      if (orbit.size() != reps.size()) return 5;
      uint64_t mask = 0;
      size_t next = 0;
      for (int i = 0; i < 8; ++i) {
        LifeState t = s.Transformed(order[i]);
        const std::array<int, 4> bounds = t.XYBounds();
        t.Move(-bounds[0], -bounds[1]);
        put(t);
        if (next < reps.size() && reps[next] == order[i]) {
          if (!(orbit[next] == t)) return 5;
          mask |= 1u << i;
          ++next;
        }
      }
      if (next != reps.size()) return 5;
      std::fwrite(&mask, 8, 1, o);
    }
  }
  std::fclose(f);
  return std::fclose(o) == 0 ? 0 : 4;
}
