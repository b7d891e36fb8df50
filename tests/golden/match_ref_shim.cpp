// match_ref_shim.cpp -- records the reference's own Match(const LifeTarget&),
// Convolve and InteractionOffsets for tests/golden/match.npz.  Compiled by
// tests/golden/make_match_golden.py against the reference headers where they
// lie (never committed or copied), into a temporary directory.
//
//   match_ref_shim IN OUT
// IN:  uint64 n, nt, np, no; states[n][64]; targets[nt][2][64];
//      patterns[np][64]; others[no][64]
// OUT: match[nt][n][64]; convolve[np][n][64]; interaction[no][n][64]
// Any of nt, np, no may be 0: for tests/golden/match_sharp.npz the generator
// runs this once per target on that target's own near misses, once for the
// patterns on the impulse states and once for the others on the sparse batch.
//
// The same translation unit instantiates the batched templates of
// lifeapi/batch.hpp on the reference's ::LifeState / ::LifeTarget, so that
// they are compiled against the reference's types (never called here).
#include <lifeapi/batch.hpp>

#include "LifeAPI.hpp"
#include "LifeTarget.hpp"

#include <chrono>
#include <cstdio>
#include <string>
#include <thread>
#include <vector>

template void lifeapi::MatchBatch<::LifeState, ::LifeTarget>(std::span<const ::LifeState>, const ::LifeTarget &,
                                                             std::span<::LifeState>, int);
template std::vector<uint32_t> lifeapi::MatchCountBatch<::LifeState, ::LifeTarget>(std::span<const ::LifeState>,
                                                                                   const ::LifeTarget &, int);
template void lifeapi::ConvolveBatch<::LifeState, ::LifeState>(std::span<const ::LifeState>, const ::LifeState &,
                                                               std::span<::LifeState>, int);
template void lifeapi::InteractionOffsetsBatch<::LifeState, ::LifeState>(std::span<const ::LifeState>,
                                                                         const ::LifeState &, std::span<::LifeState>,
                                                                         int);

static LifeState load(const uint64_t *w) {
  LifeState s;
  for (int i = 0; i < 64; ++i) s.state[i] = w[i];
  return s;
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  uint64_t h[4];
  if (!f || std::fread(h, 8, 4, f) != 4) return 3;
  const size_t n = h[0], nt = h[1], np = h[2], no = h[3], total = (n + 2 * nt + np + no) * 64;
  std::vector<uint64_t> in(total);
  if (std::fread(in.data(), 8, total, f) != total) return 3;
  std::fclose(f);
  const uint64_t *states = in.data(), *targets = states + n * 64, *patterns = targets + nt * 128,
                 *others = patterns + np * 64;
  if (std::string(argv[2]) == "--rate") {
    // for scale only: the reference's Match on every target, 16 threads,
    // states per second (make_match_golden.py --rate)
    for (size_t k = 0; k < nt; ++k) {
      const LifeTarget t(load(targets + k * 128), load(targets + k * 128 + 64));
      const size_t reps = 16 * 4096;
      std::vector<uint64_t> sink(16);
      const auto t0 = std::chrono::steady_clock::now();
      std::vector<std::thread> pool;
      for (int th = 0; th < 16; ++th)
        pool.emplace_back([&, th] {
          uint64_t acc = 0;
          for (size_t r = th; r < reps; r += 16) acc ^= load(states + (r % n) * 64).Match(t).state[r & 63];
          sink[th] = acc;
        });
      for (auto &p : pool) p.join();
      const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      std::printf("target %zu: %.0f states/s (16 threads, sink %llx)\n", k, reps / s, (unsigned long long)sink[0]);
    }
    return 0;
  }
  FILE *o = std::fopen(argv[2], "wb");
  if (!o) return 4;
  auto put = [&](const LifeState &r) { std::fwrite(r.state, 8, 64, o); };
  for (size_t k = 0; k < nt; ++k) {
    const LifeTarget t(load(targets + k * 128), load(targets + k * 128 + 64));
    for (size_t i = 0; i < n; ++i) put(load(states + i * 64).Match(t));
  }
  for (size_t k = 0; k < np; ++k) {
    const LifeState p = load(patterns + k * 64);
    for (size_t i = 0; i < n; ++i) put(load(states + i * 64).Convolve(p));
  }
  for (size_t k = 0; k < no; ++k) {
    const LifeState p = load(others + k * 64);
    for (size_t i = 0; i < n; ++i) put(load(states + i * 64).InteractionOffsets(p));
  }
  return std::fclose(o) == 0 ? 0 : 4;
}
