// symmetry_cases.hpp -- reader of the case file tests/test_symmetry_facade.py
// writes from tests/golden/symmetry.npz (the reference's recorded answers),
// shared by symmetry_facade_test.cpp (CPU) and symmetry_batch_test.cpp (GPU).
//
// File: uint64 nt, ns, no; then
//   nt x { int64 transform, dx, dy; in[64]; out[64] }   out = in.Transformed(t).Moved(dx, dy)
//   ns x { int64 symmetry, dx, dy; in[64]; out[64] }    out = Symmetricize(in, symmetry, {dx, dy})
//   no x { in[64]; int64 bounds[4]; images[8][64]; uint64 mask }
#pragma once

#include <lifeapi/LifeState.hpp>

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace cases {

struct Mapped {
  int64_t kind, dx, dy;
  lifeapi::LifeState in, out;
};
struct Orbit {
  lifeapi::LifeState in;
  int64_t bounds[4];
  lifeapi::LifeState images[8];
  uint64_t mask;
};
struct File {
  std::vector<Mapped> transforms, symmetries;
  std::vector<Orbit> orbits;
};

inline void need(bool ok, const char *what) {
  if (!ok) {
    std::fprintf(stderr, "case file: %s\n", what);
    std::exit(2);
  }
}

inline File read(const char *path) {
  std::FILE *f = std::fopen(path, "rb");
  need(f != nullptr, "cannot open");
  uint64_t n[3];
  need(std::fread(n, 8, 3, f) == 3, "short header");
  File c;
  auto state = [&](lifeapi::LifeState &s) { need(std::fread(s.state, 8, 64, f) == 64, "short state"); };
  auto mapped = [&](std::vector<Mapped> &v, uint64_t count) {
    v.resize(count);
    for (Mapped &m : v) {
      need(std::fread(&m.kind, 8, 3, f) == 3, "short case");
      state(m.in);
      state(m.out);
    }
  };
  mapped(c.transforms, n[0]);
  mapped(c.symmetries, n[1]);
  c.orbits.resize(n[2]);
  for (Orbit &o : c.orbits) {
    state(o.in);
    need(std::fread(o.bounds, 8, 4, f) == 4, "short bounds");
    for (lifeapi::LifeState &img : o.images) state(img);
    need(std::fread(&o.mask, 8, 1, f) == 1, "short mask");
  }
  std::fclose(f);
  need(!c.transforms.empty() && !c.symmetries.empty() && !c.orbits.empty(), "empty section");
  return c;
}

}  // namespace cases
