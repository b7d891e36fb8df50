// Host program for tests/test_step_chunk_order.py: lifeapi_amd/csrc/step_order.hpp
// (the index arithmetic k_step runs on the device) evaluated for every wave of
// a one-shot grid.  Arguments: MAX_BLOCKS.  For every grid of 1..MAX_BLOCKS
// blocks, every group count that needs exactly that grid (ragged against the
// 4 waves of a block), chunked and not, forward and reversed, and a plain tail
// of 0, 1, half and all of the groups (launch.hpp launch_order's plain_from),
// one line per wave:
//   nb groups chunk reverse plain_from b wib place index group plain
#include <cstdio>
#include <cstdlib>

#include "step_order.hpp"

using namespace lifeapi_impl;

int main(int argc, char **argv) {
  const unsigned max_blocks = argc > 1 ? (unsigned)std::atoi(argv[1]) : 40u;
  for (unsigned nb = 1; nb <= max_blocks; ++nb)
    for (uint64_t groups = (uint64_t)(nb - 1) * kWavesPerBlock + 1; groups <= (uint64_t)nb * kWavesPerBlock; ++groups)
      for (int chunk = 0; chunk < 2; ++chunk)
        for (int reverse = 0; reverse < 2; ++reverse) {
          const uint64_t tails[4] = {0, 1, (groups + 1) / 2, groups};
          for (int k = 0; k < 4; ++k) {
            if (k && tails[k] == tails[k - 1]) continue;
            const uint64_t plain_from = groups - tails[k];
            for (unsigned b = 0; b < nb; ++b)
              for (unsigned wib = 0; wib < (unsigned)kWavesPerBlock; ++wib) {
                const StepTake t = step_take(b, nb, wib, 0, groups, chunk != 0, reverse != 0, plain_from);
                std::printf("%u %llu %d %d %llu %u %u %llu %llu %lld %d\n", nb, (unsigned long long)groups, chunk,
                            reverse, (unsigned long long)plain_from, b, wib,
                            (unsigned long long)(chunk ? xcd_chunk_place(b, nb) : b), (unsigned long long)t.index,
                            t.index < groups ? (long long)t.group : -1ll, t.plain ? 1 : 0);
              }
          }
        }
  return 0;
}
