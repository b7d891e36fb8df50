// pair_cases.hpp -- the case file tests/test_pair_facade.py writes from
// tests/golden/pair.npz, read by pair_facade_test.cpp (CPU) and
// pair_batch_test.cpp (GPU).
//
//   uint64 count; then per case int64 kind, arg and a[64], b[64], out[64]:
//   kind 0  out = IntersectingOffsets(a, b, StaticSymmetry(arg))
//   kind 1  out = a.Convolve(b.Transformed(SymmetryTransform(arg)))
//   kind 2  out = a.Halve() (arg 0), a.HalveX() (1), a.HalveY() (2)
//   kind 3  out = a.Skew() (arg 0), a.InvSkew() (1)
#pragma once

#include <lifeapi/LifeState.hpp>

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace cases {

struct Case {
  int64_t kind, arg;
  lifeapi::LifeState a, b, out;
};

inline std::vector<Case> read(const char *path) {
  FILE *f = std::fopen(path, "rb");
  uint64_t count;
  if (!f || std::fread(&count, 8, 1, f) != 1) {
    std::fprintf(stderr, "cannot read %s\n", path);
    std::exit(2);
  }
  std::vector<Case> r(count);
  for (Case &c : r) {
    int64_t h[2];
    if (std::fread(h, 8, 2, f) != 2 || std::fread(c.a.state, 8, 64, f) != 64 || std::fread(c.b.state, 8, 64, f) != 64 ||
        std::fread(c.out.state, 8, 64, f) != 64) {
      std::fprintf(stderr, "%s is truncated\n", path);
      std::exit(2);
    }
    c.kind = h[0];
    c.arg = h[1];
  }
  std::fclose(f);
  return r;
}

}  // namespace cases
