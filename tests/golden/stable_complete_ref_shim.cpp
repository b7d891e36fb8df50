// stable_complete_ref_shim.cpp -- records the reference's own
// LifeStable::CompleteStable (LifeStable.hpp:1340-1458) and
// LifeWeld::UnweldableMask (LifeWeld.hpp:247-277) for
// tests/golden/stable_complete.npz.  Compiled by
// tests/golden/make_stable_complete_golden.py against the reference headers
// where they lie (never committed or copied), into a temporary directory.
//
//   stable_complete_ref_shim 0 IN OUT
// IN:  uint64 count; then per run planes[640], seed[64], flags (1 minimise, 2
//      useSeed), node budget (0 = none), node cap
// OUT per run: result (0 COMPLETED, 1 INCONSISTENT, 2 TIMEOUT; 5 = the cap was
//      reached, nothing else is meaningful), nodes, deepest stack, search-area
//      rounds, population found by the rounds (before the minimise pass),
//      1 if the reference defines the call, frames popped for their on-branch,
//      most ZOI growths of the caller's seed at one node, best[64]
//
// The numbers come from the same search spelled out over the reference's own
// members (Propagate, PerturbedUnknowns, Vulnerable, NeighbourCount, FirstOn,
// ZOI, BigZOI, GetPop, SetOn / SetOff), with a node budget where the reference
// reads the clock: `nodes` counts the entries of the step, tail calls included,
// and "past the limit" is nodes >= budget.  Without a budget (and below the cap,
// which only keeps the recorder from running away on an object it will not
// keep) the spelled-out search must return what CompleteStable(1e9f, ...)
// returns, else the shim fails.  That comparison is skipped where the reference
// leaves the call undefined: unknown within state.ZOI() (no round runs and
// `result` is read uninitialised; the spelled-out search runs one step on the
// object as given) and useSeed with an empty seed (never passed in here).
//
//   stable_complete_ref_shim 1 IN OUT
// IN:  uint64 count; then per case state[64] and required[64] of the weld, the
//      same of the other catalyst, good[64], bad[64], node budget
// OUT per case: the two LifeWelds as LifeWeld::FromRequired makes them
//      (weld[256], other[256]), mask[64], tested[64] (the placements
//      searched), counts of COMPLETED / INCONSISTENT / TIMEOUT --
//      weld.UnweldableMask(other, good, bad) spelled out with the budgeted
//      search in place of CompleteStable(0.05, false)
//
// The same translation unit instantiates the batched templates of
// lifeapi/batch.hpp on the reference's own structs (never called here).
#include <lifeapi/batch.hpp>

#include "LifeAPI.hpp"
#include "LifeStable.hpp"
#include "LifeWeld.hpp"

#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

template lifeapi::Completions<::LifeState> lifeapi::CompleteStableBatch<::LifeStable, ::LifeState>(
    std::span<const ::LifeStable>, bool, uint64_t, uint32_t);
template lifeapi::Completions<::LifeState> lifeapi::CompleteStableBatch<::LifeStable, ::LifeState>(
    std::span<const ::LifeStable>, bool, uint64_t, uint32_t, const ::LifeState &);
template lifeapi::Completions<::LifeState> lifeapi::CompleteStableBatch<::LifeStable, ::LifeState>(
    std::span<const ::LifeStable>, bool, uint64_t, uint32_t, std::span<const ::LifeState>);
template ::LifeState lifeapi::UnweldableMask<::LifeWeld, ::LifeState>(const ::LifeWeld &, const ::LifeWeld &,
                                                                      const ::LifeState &, const ::LifeState &, uint64_t);

static_assert(sizeof(LifeStable) == 640 * 8 && sizeof(LifeWeld) == 256 * 8 && sizeof(LifeState) == 64 * 8);

enum : uint64_t { COMPLETED = 0, INCONSISTENT = 1, TIMEOUT = 2, CAPPED = 5 };

constexpr uint64_t kDepthCap = 256;  // a recursion this deep is no fixture either (the step's frames are 5 KiB)

struct Search {
  uint64_t budget = 0, cap = 0;  // budget 0 = none
  uint64_t nodes = 0, depth = 0, deepest = 0, rounds = 0, first_pop = 0, pops = 0, growths = 0;
  bool second = false;  // in the minimise pass
  bool capped = false;
  bool minimise = false;
  unsigned maxPop = std::numeric_limits<int>::max();
  LifeState best;

  bool late() const { return budget && nodes >= budget; }

  // CompleteStableStep, LifeStable.hpp:1340-1412 (the on-branch a loop, as the
  // reference's tail call)
  uint64_t step(LifeStable s, bool useSeed, const LifeState &seed) {
    for (;;) {
      if (capped) return TIMEOUT;
      if (late()) return TIMEOUT;
      if (nodes >= cap || depth >= kDepthCap) {
        capped = true;
        return TIMEOUT;
      }
      ++nodes;
      if (!s.Propagate().consistent) return INCONSISTENT;
      const unsigned currentPop = s.state.GetPop();
      if (currentPop >= maxPop) return COMPLETED;
      LifeState settable = s.PerturbedUnknowns() & s.dead0.ZOI();
      if (settable.IsEmpty()) {
        best = s.state;
        maxPop = s.state.GetPop();
        return COMPLETED;
      }
      if (useSeed) {
        LifeState seedZOI = seed;
        uint64_t grown = 0;
        for (; (settable & seedZOI).IsEmpty(); ++grown) seedZOI = seedZOI.ZOI();
        if (!second && grown > growths) growths = grown;
        settable &= seedZOI;
      }
      std::pair<int, int> cell = (s.Vulnerable() & settable).FirstOn();
      if (cell.first == -1) {
        NeighbourCount unknownCount(s.unknown);
        const LifeState low = settable & ~unknownCount.bit3 & ~unknownCount.bit2 & unknownCount.bit1;
        cell = (low & ~unknownCount.bit0).FirstOn();
        if (cell.first == -1) cell = (low & unknownCount.bit0).FirstOn();
        if (cell.first == -1) cell = settable.FirstOn();
        if (cell.first == -1) return INCONSISTENT;
      }
      {
        LifeStable next = s;
        next.SetOff(cell);
        ++depth;
        if (depth > deepest) deepest = depth;
        const uint64_t r = step(next, useSeed, seed);
        --depth;
        if (r == TIMEOUT) return TIMEOUT;
        if (!minimise && r == COMPLETED) return COMPLETED;
      }
      ++pops;
      s.SetOn(cell);
    }
  }

  // CompleteStable, LifeStable.hpp:1414-1458
  uint64_t run(const LifeStable &in, bool useSeed, const LifeState &seed, LifeState &out) {
    out = LifeState();
    if (in.state.IsEmpty()) return COMPLETED;
    if (in.unknown.IsEmpty()) {
      out = in.state;
      return COMPLETED;
    }
    uint64_t result;
    LifeState searchArea = in.state.ZOI();
    if ((in.unknown & ~searchArea).IsEmpty()) {
      result = step(in, useSeed, seed);  // the reference runs no round: defined here as one step
    } else {
      while (!(in.unknown & ~searchArea).IsEmpty()) {
        searchArea = searchArea.ZOI();
        LifeStable copy = in;
        copy.unknown &= searchArea;
        ++rounds;
        result = step(copy, useSeed, seed);
        if (best.GetPop() > 0 || late() || capped) break;
      }
    }
    first_pop = best.GetPop();
    if (capped) return CAPPED;
    if (result == TIMEOUT && best.IsEmpty()) return TIMEOUT;
    if (result == INCONSISTENT && best.IsEmpty()) return INCONSISTENT;
    if (minimise) {
      LifeStable copy = in;
      copy.unknown &= searchArea.BigZOI();
      second = true;
      step(copy, true, in.state | best);
      if (capped) return CAPPED;
    }
    out = best;
    return COMPLETED;
  }
};

static uint64_t code(LifeStable::CompletionResult r) {
  return r == LifeStable::CompletionResult::COMPLETED ? COMPLETED
         : r == LifeStable::CompletionResult::INCONSISTENT ? INCONSISTENT : TIMEOUT;
}

int main(int argc, char **argv) {
  if (argc != 4) return 2;
  const int mode = argv[1][0] - '0';
  FILE *f = std::fopen(argv[2], "rb");
  uint64_t count;
  if (!f || std::fread(&count, 8, 1, f) != 1) return 3;
  FILE *o = std::fopen(argv[3], "wb");
  if (!o) return 4;
  if (mode == 0) {
    std::vector<uint64_t> rec(640 + 64 + 3);
    for (uint64_t k = 0; k < count; ++k) {
      if (std::fread(rec.data(), 8, rec.size(), f) != rec.size()) return 3;
      LifeStable in;
      LifeState seed;
      std::memcpy((void *)&in, rec.data(), sizeof in);
      std::memcpy((void *)&seed, rec.data() + 640, sizeof seed);
      const bool minimise = rec[704] & 1, useSeed = rec[704] & 2;
      if (useSeed && seed.IsEmpty()) return 5;
      Search s;
      s.budget = rec[705];
      s.cap = rec[706];
      s.minimise = minimise;
      LifeState best;
      const uint64_t r = s.run(in, useSeed, seed, best);
      const bool defined = in.state.IsEmpty() || in.unknown.IsEmpty() || !(in.unknown & ~in.state.ZOI()).IsEmpty();
      if (defined && r != CAPPED && s.budget == 0) {
        LifeStable again = in;
        auto [rr, rbest] = again.CompleteStable(1e9f, minimise, useSeed, seed);
        if (code(rr) != r || !(rbest == best)) {
          std::fprintf(stderr, "run %llu: the spelled-out search differs from CompleteStable\n", (unsigned long long)k);
          return 6;
        }
      }
      const uint64_t head[8] = {r, s.nodes, s.deepest, s.rounds, s.first_pop, defined ? 1u : 0u, s.pops, s.growths};
      std::fwrite(head, 8, 8, o);
      std::fwrite((const void *)&best, 8, 64, o);
    }
  } else {
    std::vector<uint64_t> rec(6 * 64 + 1);
    for (uint64_t k = 0; k < count; ++k) {
      if (std::fread(rec.data(), 8, rec.size(), f) != rec.size()) return 3;
      LifeState in[6];
      std::memcpy((void *)in, rec.data(), sizeof in);
      const LifeWeld weld = LifeWeld::FromRequired(in[0], in[1]), other = LifeWeld::FromRequired(in[2], in[3]);
      const LifeState &good = in[4], &bad = in[5];
      // UnweldableMask, LifeWeld.hpp:247-277
      LifeState knownBad = weld.InteractionOffsets(other) | bad;
      LifeState toTest = ~good & ~knownBad;
      const LifeState tested = toTest;
      uint64_t counts[3] = {0, 0, 0};
      for (auto cell = toTest.FirstOn(); cell != std::make_pair(-1, -1); toTest.Erase(cell), cell = toTest.FirstOn()) {
        const LifeWeld placed = weld | other.Moved(cell);
        Search s;
        s.budget = rec[384];
        s.cap = ~0ull;
        LifeState best;
        const uint64_t r = s.run(placed.ToStable(), false, LifeState(), best);
        if (r == CAPPED) return 7;
        ++counts[r];
        if (r == INCONSISTENT) knownBad.Set(cell);
      }
      std::fwrite((const void *)&weld, 8, 256, o);
      std::fwrite((const void *)&other, 8, 256, o);
      std::fwrite((const void *)&knownBad, 8, 64, o);
      std::fwrite((const void *)&tested, 8, 64, o);
      std::fwrite(counts, 8, 3, o);
    }
  }
  std::fclose(f);
  return std::fclose(o) == 0 ? 0 : 4;
}
