// weld_cases.hpp -- reader of the case file tests/test_weld_facade.py writes
// from tests/golden/weld_family.npz (the reference's recorded answers), shared by
// weld_facade_test.cpp (CPU) and weld_batch_test.cpp (GPU).
//
// File: uint64 nr, nw, ns, no; then
//   nr x { state[64]; required[64]; weld[256] }        weld = FromRequired(state, required)
//   nw x { weld[256]; target[128]; stable[640] }       target = weld.ToTarget(), stable = weld.ToStable()
//   ns x { weld[256]; active[64]; mask[64]; uint64 duration; stable[640] }
//                                                      stable = weld.ToStable(active, duration, mask)
//   no x { weld[256]; other[256]; out[64] }            out = weld.InteractionOffsets(other)
#pragma once

#include <lifeapi/LifeState.hpp>

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace cases {

struct Required {
  lifeapi::LifeState state, required;
  lifeapi::LifeWeld weld;
};
struct Static {
  lifeapi::LifeWeld weld;
  lifeapi::LifeTarget target;
  lifeapi::LifeStable stable;
};
struct Replay {
  lifeapi::LifeWeld weld;
  lifeapi::LifeState active, mask;
  uint64_t duration;
  lifeapi::LifeStable stable;
};
struct Offsets {
  lifeapi::LifeWeld weld, other;
  lifeapi::LifeState out;
};
struct File {
  std::vector<Required> required;
  std::vector<Static> statics;
  std::vector<Replay> replays;
  std::vector<Offsets> offsets;
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
  uint64_t n[4];
  need(std::fread(n, 8, 4, f) == 4, "short header");
  File c;
  // every struct read here is N LifeStates in member order and nothing else
  static_assert(sizeof(lifeapi::LifeWeld) == 2048 && sizeof(lifeapi::LifeTarget) == 1024 &&
                sizeof(lifeapi::LifeStable) == 5120);
  auto get = [&](auto &s) { need(std::fread(static_cast<void *>(&s), sizeof s, 1, f) == 1, "short record"); };
  c.required.resize(n[0]);
  for (Required &k : c.required) get(k.state), get(k.required), get(k.weld);
  c.statics.resize(n[1]);
  for (Static &k : c.statics) get(k.weld), get(k.target), get(k.stable);
  c.replays.resize(n[2]);
  for (Replay &k : c.replays) get(k.weld), get(k.active), get(k.mask), get(k.duration), get(k.stable);
  c.offsets.resize(n[3]);
  for (Offsets &k : c.offsets) get(k.weld), get(k.other), get(k.out);
  std::fclose(f);
  need(!c.required.empty() && !c.statics.empty() && !c.replays.empty() && !c.offsets.empty(), "empty section");
  return c;
}

}  // namespace cases
