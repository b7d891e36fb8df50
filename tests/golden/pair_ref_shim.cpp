// pair_ref_shim.cpp -- records the reference's own IntersectingOffsets,
// Convolve of a transformed operand, Halve / HalveX / HalveY and Skew /
// InvSkew for tests/golden/pair.npz.  Compiled by
// tests/golden/make_pair_golden.py against the reference headers where they
// lie (never committed or copied), into a temporary directory.
//
//   pair_ref_shim IN OUT
// IN:  uint64 count; then per operation int64 kind, arg and a[64], b[64]
// OUT: per operation 64 words:
//   kind 0  IntersectingOffsets(a, b, StaticSymmetry(arg))
//   kind 1  a.Convolve(b.Transformed(SymmetryTransform(arg)))
//   kind 2  a.Halve() (arg 0), a.HalveX() (1), a.HalveY() (2)
//   kind 3  a.Skew() (arg 0), a.InvSkew() (1)
//
// The same translation unit instantiates the batched templates of
// lifeapi/batch.hpp on the reference's ::LifeState, so that they are compiled
// against the reference's types (never called here).
#include <lifeapi/batch.hpp>

#include "LifeAPI.hpp"
#include "Symmetry.hpp"

#include <cstdio>

using OffsetSpan = std::span<const std::pair<int, int>>;
template void lifeapi::TransformBatch<::LifeState, ::SymmetryTransform>(std::span<const ::LifeState>,
                                                                        std::span<::LifeState>, ::SymmetryTransform,
                                                                        OffsetSpan, int);
template void lifeapi::SymmetricizeBatch<::LifeState, ::StaticSymmetry>(std::span<const ::LifeState>,
                                                                        std::span<::LifeState>, ::StaticSymmetry,
                                                                        OffsetSpan, int);
template void lifeapi::ConvolvePairBatch<::LifeState, ::SymmetryTransform>(std::span<const ::LifeState>,
                                                                           std::span<const ::LifeState>,
                                                                           ::SymmetryTransform, std::span<::LifeState>,
                                                                           int);
template void lifeapi::IntersectingOffsetsBatch<::LifeState, ::StaticSymmetry>(std::span<const ::LifeState>,
                                                                               std::span<const ::LifeState>,
                                                                               ::StaticSymmetry, std::span<::LifeState>,
                                                                               int);
template void lifeapi::IntersectingOffsetsBatch<::LifeState, ::StaticSymmetry>(std::span<const ::LifeState>,
                                                                               ::StaticSymmetry, std::span<::LifeState>,
                                                                               int);
template void lifeapi::HalveBatch<::LifeState>(std::span<const ::LifeState>, std::span<::LifeState>, lifeapi::HalveMode,
                                               int);
template void lifeapi::SkewBatch<::LifeState>(std::span<const ::LifeState>, std::span<::LifeState>, bool, int);

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  uint64_t count;
  if (!f || std::fread(&count, 8, 1, f) != 1) return 3;
  FILE *o = std::fopen(argv[2], "wb");
  if (!o) return 4;
  auto put = [&](const LifeState &r) { std::fwrite(r.state, 8, 64, o); };
  for (uint64_t k = 0; k < count; ++k) {
    int64_t h[2];
    LifeState a, b;
    if (std::fread(h, 8, 2, f) != 2 || std::fread(a.state, 8, 64, f) != 64 || std::fread(b.state, 8, 64, f) != 64)
      return 3;
    const int arg = (int)h[1];
    if (h[0] == 0) {
      put(IntersectingOffsets(a, b, (StaticSymmetry)arg));
      if (a == b && !(IntersectingOffsets(a, (StaticSymmetry)arg) == IntersectingOffsets(a, b, (StaticSymmetry)arg)))
        return 5;
    } else if (h[0] == 1) {
      put(a.Convolve(b.Transformed((SymmetryTransform)arg)));
    } else if (h[0] == 2) {
      put(arg == 0 ? a.Halve() : arg == 1 ? a.HalveX() : a.HalveY());
    } else {
      put(arg == 0 ? a.Skew() : a.InvSkew());
    }
  }
  std::fclose(f);
  return std::fclose(o) == 0 ? 0 : 4;
}
