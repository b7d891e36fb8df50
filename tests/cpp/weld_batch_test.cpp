// weld_batch_test.cpp -- GPU: the batched LifeWeld templates of lifeapi/batch.hpp
// (WeldFromRequiredBatch, WeldToTargetBatch, WeldToStableBatch,
// WeldInteractionOffsetsBatch) on the lifeapi:: structs, against the facade's own
// CPU members on the inputs of the recorded cases, and straight on into
// PropagateBatch without leaving the batch.
//
//   weld_batch_test CASES       (the file of weld_cases.hpp)
#include "weld_cases.hpp"

#include <lifeapi/batch.hpp>

using namespace lifeapi;

static int failures = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      ++failures;                                         \
      std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);                  \
      std::fprintf(stderr, "\n");                         \
    }                                                     \
  } while (0)

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  const cases::File c = cases::read(argv[1]);
  size_t launches = 0;
  try {
    std::vector<LifeState> states, required;
    for (const cases::Required &k : c.required) states.push_back(k.state), required.push_back(k.required);
    const std::span<const LifeState> st(states), rq(required);
    const std::vector<LifeWeld> per = WeldFromRequiredBatch<LifeWeld>(st, rq);
    const std::vector<LifeWeld> one = WeldFromRequiredBatch<LifeWeld>(st, required[0]);
    for (size_t k = 0; k < states.size(); ++k) {
      CHECK(per[k] == LifeWeld::FromRequired(states[k], required[k]), "WeldFromRequiredBatch (per universe) %zu", k);
      CHECK(one[k] == LifeWeld::FromRequired(states[k], required[0]), "WeldFromRequiredBatch (one required) %zu", k);
    }
    launches += 2;

    std::vector<LifeWeld> welds;
    for (const cases::Static &k : c.statics) welds.push_back(k.weld);
    const std::span<const LifeWeld> ws(welds);
    const std::vector<LifeTarget> targets = WeldToTargetBatch<LifeTarget>(ws);
    std::vector<LifeStable> stables = WeldToStableBatch<LifeStable>(ws);
    for (size_t k = 0; k < welds.size(); ++k) {
      const LifeTarget t = welds[k].ToTarget();
      CHECK(targets[k].wanted == t.wanted && targets[k].unwanted == t.unwanted, "WeldToTargetBatch %zu", k);
      CHECK(stables[k] == welds[k].ToStable(), "WeldToStableBatch %zu", k);
    }
    launches += 2;
    // ... and on into the propagation passes without leaving the batch (what
    // Propagate makes of them is tests/test_gpu_weld.py's, against the oracle)
    const std::vector<PropagateResult> pr = PropagateBatch(std::span<LifeStable>(stables));
    CHECK(pr.size() == stables.size(), "PropagateBatch after WeldToStableBatch");
    ++launches;

    // one active / mask / duration for the batch, then an active per weld
    const cases::Replay &r = c.replays[c.replays.size() / 2];
    const unsigned d = 8;
    const std::vector<LifeStable> a = WeldToStableBatch<LifeStable>(ws, r.active, d);
    const std::vector<LifeStable> b = WeldToStableBatch<LifeStable>(ws, r.active, d, r.mask);
    std::vector<LifeState> actives;
    for (size_t k = 0; k < welds.size(); ++k) actives.push_back(c.replays[k % c.replays.size()].active);
    const std::vector<LifeStable> p = WeldToStableBatch<LifeStable>(ws, std::span<const LifeState>(actives), d);
    const std::vector<LifeStable> q = WeldToStableBatch<LifeStable>(ws, std::span<const LifeState>(actives), d, r.mask);
    for (size_t k = 0; k < welds.size(); ++k) {
      CHECK(a[k] == welds[k].ToStable(r.active, d), "WeldToStableBatch (active) %zu", k);
      CHECK(b[k] == welds[k].ToStable(r.active, d, r.mask), "WeldToStableBatch (active, mask) %zu", k);
      CHECK(p[k] == welds[k].ToStable(actives[k], d), "WeldToStableBatch (actives) %zu", k);
      CHECK(q[k] == welds[k].ToStable(actives[k], d, r.mask), "WeldToStableBatch (actives, mask) %zu", k);
    }
    launches += 4;

    for (const LifeWeld &other : {c.offsets.front().other, c.offsets.back().other}) {
      const std::vector<LifeState> got = WeldInteractionOffsetsBatch<LifeState>(ws, other);
      for (size_t k = 0; k < welds.size(); ++k)
        CHECK(got[k] == welds[k].InteractionOffsets(other), "WeldInteractionOffsetsBatch %zu", k);
      ++launches;
    }

    bool thrown = false;
    try {
      (void)WeldToStableBatch<LifeStable>(ws, r.active, 65537u);
    } catch (const Error &e) {
      thrown = e.code == LIFEAPI_E_INVALID;
    }
    CHECK(thrown, "duration 65537 must throw LIFEAPI_E_INVALID");
  } catch (const Error &e) {
    std::fprintf(stderr, "lifeapi::Error %d: %s\n", e.code, e.what());
    return 1;
  }
  if (failures == 0) std::printf("weld_batch_test: ok (%zu launches)\n", launches);
  return failures ? 1 : 0;
}
