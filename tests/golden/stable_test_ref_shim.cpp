// stable_test_ref_shim.cpp -- records the reference's own LifeStable strip
// passes, TestUnknowns and PropagateAndTest for tests/golden/stable_test.npz.
// Compiled by tests/golden/make_stable_test_golden.py against the reference
// headers where they lie (never committed or copied), into a temporary
// directory.
//
//   stable_test_ref_shim MODE IN OUT
// IN:  uint64 count; then per object planes[640], column
// OUT per object, MODE 0 (classification, on the reference's outputs alone):
//   8 words: PropagateAndTest's flags (consistent | changed << 1), cells tested,
//   cells forced on, cells forced off, Joins that changed the object, 1 if
//   TestUnknowns returned inconsistent, 1 if Propagate did, rounds of the outer
//   loop -- counted by a loop that calls the reference's Propagate, Vulnerable,
//   FirstOn and TestUnknown in PropagateAndTest's own order, and whose end state
//   must equal PropagateAndTest's (else the shim fails)
// MODE 1 (the recording):
//   PropagateAndTest: planes[640], flags
//   Propagate, then TestUnknowns(Vulnerable().ZOI()): planes[640], flags
//   the object after PropagateStep(), UpdateOptions() and SignalNeighbours(), its
//   state and unknown planes then replaced by PropagateAndTest's ("fresh":
//   options and cells that nothing has synchronised yet): planes[640], 0
//   for the object as given and then for the fresh one, for each of the 8
//   columns {0, 1, 2, 31, 61, 62, 63, column}, for each of the six strip passes
//   (SynchroniseStateKnownStrip, UpdateOptionsStrip, SignalNeighboursStrip,
//   PropagateStepStrip, PropagateStrip, StabiliseOptionsStrip): planes[640],
//   flags
//
// The same translation unit instantiates the batched templates of
// lifeapi/batch.hpp on the reference's own structs (never called here).
#include <lifeapi/batch.hpp>

#include "LifeAPI.hpp"
#include "LifeStable.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

template std::vector<lifeapi::PropagateResult> lifeapi::PropagateStripBatch<::LifeStable>(std::span<::LifeStable>,
                                                                                         std::span<const uint8_t>, int);
template std::vector<lifeapi::PropagateResult> lifeapi::TestUnknownsBatch<::LifeStable, ::LifeState>(
    std::span<::LifeStable>, const ::LifeState &, int);
template std::vector<lifeapi::PropagateResult> lifeapi::TestUnknownsBatch<::LifeStable, ::LifeState>(
    std::span<::LifeStable>, std::span<const ::LifeState>, int);
template std::vector<lifeapi::PropagateResult> lifeapi::PropagateAndTestBatch<::LifeStable>(std::span<::LifeStable>, int);

static_assert(sizeof(LifeStable) == 640 * 8);

static LifeStable load(const uint64_t *p) {
  LifeStable s;
  std::memcpy((void *)&s, p, sizeof s);
  return s;
}
static uint64_t flags(LifeStable::PropagateResult r) { return (r.consistent ? 1u : 0u) | (r.changed ? 2u : 0u); }

struct Counts {
  uint64_t tested = 0, forced_on = 0, forced_off = 0, joins = 0, bad_test = 0, bad_propagate = 0, rounds = 0;
};

// PropagateAndTest (and TestUnknowns inside it) spelled out over the
// reference's own members, counting what each TestUnknown did
static LifeStable::PropagateResult counted(LifeStable &s, Counts &c) {
  bool ever = false, any = true;
  while (any) {
    any = false;
    ++c.rounds;
    auto r = s.Propagate();
    if (!r.consistent) {
      c.bad_propagate = 1;
      return {false, false};
    }
    any = any || r.changed;
    LifeState remaining = s.Vulnerable().ZOI() & s.unknown;
    bool changed = false;
    while (!remaining.IsEmpty()) {
      auto cell = remaining.FirstOn();
      remaining.Erase(cell);
      LifeStable on = s, off = s;
      on.SetOn(cell);
      off.SetOff(cell);
      const auto ron = on.PropagateStrip(cell.first), roff = off.PropagateStrip(cell.first);
      const LifeStable before = s;
      const auto t = s.TestUnknown(cell);
      ++c.tested;
      if (!t.consistent) {
        c.bad_test = 1;
        return {false, false};
      }
      if (!ron.consistent) ++c.forced_off;
      else if (!roff.consistent) ++c.forced_on;
      else if (t.changed && !(s == before)) ++c.joins;
      changed = changed || t.changed;
      remaining &= s.unknown;
    }
    any = any || changed;
    ever = any || ever;
  }
  return {true, ever};
}

int main(int argc, char **argv) {
  if (argc != 4) return 2;
  const int mode = argv[1][0] - '0';
  FILE *f = std::fopen(argv[2], "rb");
  uint64_t count;
  if (!f || std::fread(&count, 8, 1, f) != 1) return 3;
  FILE *o = std::fopen(argv[3], "wb");
  if (!o) return 4;
  auto put = [&](const LifeStable &s, uint64_t fl) {
    std::fwrite((const void *)&s, 8, 640, o);
    std::fwrite(&fl, 8, 1, o);
  };
  std::vector<uint64_t> rec(641);
  for (uint64_t k = 0; k < count; ++k) {
    if (std::fread(rec.data(), 8, rec.size(), f) != rec.size()) return 3;
    const LifeStable in = load(rec.data());
    const unsigned column = (unsigned)rec[640];
    LifeStable pat = in;
    const auto rpat = pat.PropagateAndTest();
    if (mode == 0) {
      LifeStable again = in;
      Counts c;
      const auto r = counted(again, c);
      if (!(again == pat) || flags(r) != flags(rpat)) return 6;
      const uint64_t out[8] = {flags(rpat), c.tested, c.forced_on, c.forced_off, c.joins, c.bad_test, c.bad_propagate, c.rounds};
      std::fwrite(out, 8, 8, o);
      continue;
    }
    put(pat, flags(rpat));
    LifeStable tu = in;
    tu.Propagate();
    const auto rtu = tu.TestUnknowns(tu.Vulnerable().ZOI());
    put(tu, flags(rtu));
    const unsigned columns[8] = {0, 1, 2, 31, 61, 62, 63, column};
    LifeStable fresh = in;  // options and cells that nothing has synchronised yet
    fresh.PropagateStep();
    fresh.UpdateOptions();
    fresh.SignalNeighbours();
    fresh.state = pat.state;  // what the lookahead settled, its options not yet set
    fresh.unknown = pat.unknown;
    put(fresh, 0);
    for (const LifeStable *from : {&in, (const LifeStable *)&fresh})
    for (unsigned x : columns) {
      for (int pass = 0; pass < 6; ++pass) {
        LifeStable s = *from;
        LifeStable::PropagateResult r{};
        switch (pass) {
        case 0: r = s.SynchroniseStateKnownStrip(x); break;
        case 1: r = s.UpdateOptionsStrip(x); break;
        case 2: r = s.SignalNeighboursStrip(x); break;
        case 3: r = s.PropagateStepStrip(x); break;
        case 4: r = s.PropagateStrip(x); break;
        default: r = s.StabiliseOptionsStrip(x); break;
        }
        put(s, flags(r));
      }
    }
  }
  std::fclose(f);
  return std::fclose(o) == 0 ? 0 : 4;
}
