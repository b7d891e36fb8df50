// weld_ref_shim.cpp -- records the reference's own LifeWeld::FromRequired,
// ToTarget, ToStable, InteractionOffsets and Step for tests/golden/weld_family.npz.
// Compiled by tests/golden/make_weld_golden.py against the reference headers
// where they lie (never committed or copied), into a temporary directory.
//
//   weld_ref_shim IN OUT
// IN:  uint64 count; then per operation int64 kind, int64 duration and
//      weld[256], other[256], x[64], y[64]
// OUT: per operation, in order:
//   kind 0  LifeWeld::FromRequired(x, y)                          256 words
//   kind 1  weld.ToTarget(): wanted, unwanted                     128 words
//   kind 2  weld.ToStable()                                       640 words
//   kind 3  weld.ToStable(x, duration, y)                         640 words
//   kind 4  weld.ToStable(x, duration)   (the default mask)       640 words
//   kind 5  weld.InteractionOffsets(other)                         64 words
//   kind 6  weld.Stepped()                                        256 words
//   kind 7  weld.state.InteractionOffsets(other.state)             64 words
//   kind 8  the formula of kind 5 with every plane under its OWN side's mask
//           (what LifeWeld.hpp:238-239 would give without their oddity),
//           from the reference's own operations                    64 words
//
// The same translation unit instantiates the batched templates of
// lifeapi/batch.hpp on the reference's own structs, so that they are compiled
// against the reference's types (never called here).
#include <lifeapi/batch.hpp>

#include "LifeAPI.hpp"
#include "LifeWeld.hpp"

#include <cstdio>
#include <vector>

template std::vector<::LifeWeld> lifeapi::WeldFromRequiredBatch<::LifeWeld, ::LifeState>(std::span<const ::LifeState>,
                                                                                         const ::LifeState &, int);
template std::vector<::LifeWeld> lifeapi::WeldFromRequiredBatch<::LifeWeld, ::LifeState>(std::span<const ::LifeState>,
                                                                                         std::span<const ::LifeState>, int);
template std::vector<::LifeTarget> lifeapi::WeldToTargetBatch<::LifeTarget, ::LifeWeld>(std::span<const ::LifeWeld>, int);
template std::vector<::LifeStable> lifeapi::WeldToStableBatch<::LifeStable, ::LifeWeld>(std::span<const ::LifeWeld>, int);
template std::vector<::LifeStable> lifeapi::WeldToStableBatch<::LifeStable, ::LifeWeld, ::LifeState>(
    std::span<const ::LifeWeld>, const ::LifeState &, unsigned, int);
template std::vector<::LifeStable> lifeapi::WeldToStableBatch<::LifeStable, ::LifeWeld, ::LifeState>(
    std::span<const ::LifeWeld>, const ::LifeState &, unsigned, const ::LifeState &, int);
template std::vector<::LifeStable> lifeapi::WeldToStableBatch<::LifeStable, ::LifeWeld, ::LifeState>(
    std::span<const ::LifeWeld>, std::span<const ::LifeState>, unsigned, int);
template std::vector<::LifeStable> lifeapi::WeldToStableBatch<::LifeStable, ::LifeWeld, ::LifeState>(
    std::span<const ::LifeWeld>, std::span<const ::LifeState>, unsigned, const ::LifeState &, int);
template std::vector<::LifeState> lifeapi::WeldInteractionOffsetsBatch<::LifeState, ::LifeWeld>(
    std::span<const ::LifeWeld>, const ::LifeWeld &, int);

static LifeState load(const uint64_t *p) {
  LifeState s;
  for (int i = 0; i < 64; ++i) s.state[i] = p[i];
  return s;
}
static LifeWeld load_weld(const uint64_t *p) { return LifeWeld(load(p), load(p + 64), load(p + 128), load(p + 192)); }

// the seven planes of one side, from the reference's CountNeighbourhood
struct Planes {
  LifeState cells, dead1, dead2, live3, live4up, dead2up, dead1up;
  explicit Planes(const LifeState &s) {
    LifeState b3, b2, b1, b0;
    s.CountNeighbourhood(b3, b2, b1, b0);
    cells = s;
    dead1 = ~b3 & ~b2 & ~b1 & b0 & ~s;
    dead2 = ~b3 & ~b2 & b1 & ~b0 & ~s;
    live3 = ~b3 & ~b2 & b1 & b0 & s;
    live4up = (b2 | b3) & s;
    dead2up = (b3 | b2 | b1) & ~s;
    dead1up = (b3 | b2 | b1 | b0) & ~s;
  }
};
static LifeState own_side_formula(const LifeWeld &a, const LifeWeld &b) {
  const LifeState ak = (a.state & ~a.AllFrozen()).ZOI(), bk = (b.state & ~b.AllFrozen()).ZOI().Mirrored();
  const Planes p(a.state), q(b.state.Mirrored());
  return p.cells.Convolve(q.cells) | (p.dead1 & ak).Convolve(q.dead2 & bk) | (q.dead1 & bk).Convolve(p.dead2 & ak) |
         (p.live3 & ak).Convolve(q.dead2up & bk) | (p.live4up & ak).Convolve(q.dead1up & bk) |
         (q.live3 & bk).Convolve(p.dead2up & ak) | (q.live4up & bk).Convolve(p.dead1up & ak);
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  uint64_t count;
  if (!f || std::fread(&count, 8, 1, f) != 1) return 3;
  FILE *o = std::fopen(argv[2], "wb");
  if (!o) return 4;
  auto put = [&](const LifeState &r) { std::fwrite(r.state, 8, 64, o); };
  auto put_weld = [&](const LifeWeld &w) { put(w.state), put(w.frozen2), put(w.frozen1), put(w.frozen0); };
  auto put_stable = [&](const LifeStable &s) {
    for (const LifeState *p : {&s.state, &s.unknown, &s.live2, &s.live3, &s.dead0, &s.dead1, &s.dead2, &s.dead4,
                               &s.dead5, &s.dead6})
      put(*p);
  };
  std::vector<uint64_t> rec(2 + 256 + 256 + 64 + 64);
  for (uint64_t k = 0; k < count; ++k) {
    if (std::fread(rec.data(), 8, rec.size(), f) != rec.size()) return 3;
    const int64_t kind = (int64_t)rec[0];
    const unsigned duration = (unsigned)rec[1];
    const LifeWeld weld = load_weld(&rec[2]), other = load_weld(&rec[258]);
    const LifeState x = load(&rec[514]), y = load(&rec[578]);
    switch (kind) {
    case 0: put_weld(LifeWeld::FromRequired(x, y)); break;
    case 1: {
      const LifeTarget t = weld.ToTarget();
      put(t.wanted), put(t.unwanted);
      break;
    }
    case 2: put_stable(weld.ToStable()); break;
    case 3: put_stable(weld.ToStable(x, duration, y)); break;
    case 4: put_stable(weld.ToStable(x, duration)); break;
    case 5: put(weld.InteractionOffsets(other)); break;
    case 6: put_weld(weld.Stepped()); break;
    case 7: put(weld.state.InteractionOffsets(other.state)); break;
    case 8: put(own_side_formula(weld, other)); break;
    default: return 5;
    }
  }
  std::fclose(f);
  return std::fclose(o) == 0 ? 0 : 4;
}
