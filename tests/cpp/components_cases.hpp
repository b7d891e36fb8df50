// components_cases.hpp -- reader of the case file tests/test_components_facade.py
// writes from tests/golden/components.npz (the reference's recorded answers),
// shared by components_facade_test.cpp (CPU) and components_batch_test.cpp (GPU).
//
// File: uint64 nf, nc, np; then
//   nf x { in[64]; int64 x, y }                                (x, y) = in.FirstOn()
//   nc x { in[64]; seed[64]; corona[64]; out[64] }             out = in.ComponentContaining(seed, corona)
//   np x { in[64]; corona[64]; uint64 count; parts[count][64] }  parts = in.Components(corona)
#pragma once

#include <lifeapi/LifeState.hpp>

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace cases {

struct First {
  lifeapi::LifeState in;
  int64_t x, y;
};
struct Containing {
  lifeapi::LifeState in, seed, corona, out;
};
struct Parts {
  lifeapi::LifeState in, corona;
  std::vector<lifeapi::LifeState> parts;
};
struct File {
  std::vector<First> firsts;
  std::vector<Containing> containing;
  std::vector<Parts> parts;
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
  c.firsts.resize(n[0]);
  for (First &k : c.firsts) {
    state(k.in);
    need(std::fread(&k.x, 8, 2, f) == 2, "short cell");
  }
  c.containing.resize(n[1]);
  for (Containing &k : c.containing) {
    state(k.in);
    state(k.seed);
    state(k.corona);
    state(k.out);
  }
  c.parts.resize(n[2]);
  for (Parts &k : c.parts) {
    state(k.in);
    state(k.corona);
    uint64_t count;
    need(std::fread(&count, 8, 1, f) == 1 && count <= 4096, "bad count");
    k.parts.resize(count);
    for (lifeapi::LifeState &p : k.parts) state(p);
  }
  std::fclose(f);
  need(!c.firsts.empty() && !c.containing.empty() && !c.parts.empty(), "empty section");
  return c;
}

}  // namespace cases
