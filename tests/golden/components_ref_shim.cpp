// components_ref_shim.cpp -- records the reference's own FirstOn,
// ComponentContaining and Components for tests/golden/components.npz.  Compiled
// by tests/golden/make_components_golden.py against the reference headers where
// they lie (never committed or copied), into a temporary directory.
//
//   components_ref_shim IN OUT
// IN:  uint64 count; then per operation int64 kind and state[64], seed[64],
//      corona[64]
// OUT: per operation, in order:
//   kind 0  state.FirstOn() as 2 int64                            2 words
//   kind 1  state.ComponentContaining(seed, corona)              64 words
//   kind 2  state.ComponentContaining(seed)   (the default argument) 64 words
//   kind 3  state.Components(corona): the count, then each   1 + 64 k words
// (state.Components() is not offered: in this snapshot its default corona lacks
// (0, 0), see make_components_golden.py, and the loop does not terminate)
//
// The same translation unit instantiates the batched templates of
// lifeapi/batch.hpp on the reference's ::LifeState, so that they are compiled
// against the reference's types (never called here).
#include <lifeapi/batch.hpp>

#include "LifeAPI.hpp"

#include <cstdio>
#include <vector>

template std::vector<std::pair<int, int>> lifeapi::FirstOn<::LifeState>(std::span<const ::LifeState>, int);
template std::vector<::LifeState> lifeapi::ComponentContaining<::LifeState>(std::span<const ::LifeState>,
                                                                            const ::LifeState &, int);
template std::vector<::LifeState> lifeapi::ComponentContaining<::LifeState, ::LifeState>(
    std::span<const ::LifeState>, const ::LifeState &, const ::LifeState &, int);
template std::vector<::LifeState> lifeapi::ComponentContaining<::LifeState>(std::span<const ::LifeState>,
                                                                            std::span<const ::LifeState>, int);
template std::vector<::LifeState> lifeapi::ComponentContaining<::LifeState, ::LifeState>(
    std::span<const ::LifeState>, std::span<const ::LifeState>, const ::LifeState &, int);
template std::vector<uint32_t> lifeapi::ComponentCounts<::LifeState>(std::span<const ::LifeState>, int);
template std::vector<uint32_t> lifeapi::ComponentCounts<::LifeState, ::LifeState>(std::span<const ::LifeState>,
                                                                                  const ::LifeState &, int);
template std::vector<std::vector<::LifeState>> lifeapi::Components<::LifeState>(std::span<const ::LifeState>, int);
template std::vector<std::vector<::LifeState>> lifeapi::Components<::LifeState, ::LifeState>(
    std::span<const ::LifeState>, const ::LifeState &, int);

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  uint64_t count;
  if (!f || std::fread(&count, 8, 1, f) != 1) return 3;
  FILE *o = std::fopen(argv[2], "wb");
  if (!o) return 4;
  auto put = [&](const LifeState &r) { std::fwrite(r.state, 8, 64, o); };
  for (uint64_t k = 0; k < count; ++k) {
    int64_t kind;
    LifeState s, seed, corona;
    if (std::fread(&kind, 8, 1, f) != 1 || std::fread(s.state, 8, 64, f) != 64 ||
        std::fread(seed.state, 8, 64, f) != 64 || std::fread(corona.state, 8, 64, f) != 64)
      return 3;
    if (kind == 0) {
      const std::pair<int, int> c = s.FirstOn();
      const int64_t xy[2] = {c.first, c.second};
      std::fwrite(xy, 8, 2, o);
    } else if (kind == 1) {
      put(s.ComponentContaining(seed, corona));
    } else if (kind == 2) {
      put(s.ComponentContaining(seed));
    } else {
      const std::vector<LifeState> parts = s.Components(corona);
      const uint64_t n = parts.size();
      std::fwrite(&n, 8, 1, o);
      for (const LifeState &p : parts) put(p);
    }
  }
  std::fclose(f);
  return std::fclose(o) == 0 ? 0 : 4;
}
