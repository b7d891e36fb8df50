// weld.hip -- the LifeWeld construction entry points: FromRequired
// (LifeWeld.hpp:133-159), ToTarget (:188-191), ToStable (:279-400) and
// InteractionOffsets(const LifeWeld &) (:206-245) over a batch
// (weld_kernels.hpp).  Every argument is checked before a device is touched.
#include "launch.hpp"
#include "weld_kernels.hpp"

using namespace lifeapi_impl;

namespace {

// objects per wave (their loads issued first).  k_weld_to_stable takes one:
// its generation loop keeps about sixty registers per weld live
constexpr int kFromRequiredU = 2, kToTargetU = 4, kOffsetsU = 2;
constexpr size_t kState = 512, kWeld = 4 * 512, kStable = 10 * 512;
constexpr uint32_t kMaxDuration = 65536;

struct Arg {
  const char *name;
  const void *p;
  size_t bytes;  // in all
};

// non-null and 8-byte aligned
int check_ptr(const char *fn, const Arg &a) {
  if (!a.p) return fail(LIFEAPI_E_INVALID, (std::string(fn) + ": null " + a.name + "%s").c_str());
  if (!aligned8(a.p)) return fail(LIFEAPI_E_INVALID, (std::string(fn) + ": misaligned " + a.name + "%s").c_str());
  return LIFEAPI_OK;
}
// an output clear of every other array of the call
int check_clear(const char *fn, const Arg &out, std::initializer_list<Arg> others) {
  for (const Arg &o : others)
    if (o.p && ranges_overlap(out.p, out.bytes, o.p, o.bytes))
      return fail(LIFEAPI_E_INVALID, (std::string(fn) + ": " + out.name + " overlaps " + o.name + "%s").c_str());
  return LIFEAPI_OK;
}
int check_n(const char *fn, size_t n) {
  return n > SIZE_MAX / kStable ? fail(LIFEAPI_E_INVALID, "%s: n too large", fn) : LIFEAPI_OK;
}

}  // namespace

extern "C" {

int lifeapi_weld_from_required_batch_dev(const uint64_t *d_states, const uint64_t *d_required,
                                         int per_universe_required, uint64_t *d_welds, size_t n, void *stream) {
  static const char fn[] = "lifeapi_weld_from_required_batch_dev";
  if (n == 0) return LIFEAPI_OK;
  int rc = check_n(fn, n);
  const Arg st{"d_states", d_states, n * kState}, rq{"d_required", d_required, per_universe_required ? n * kState : kState},
      we{"d_welds", d_welds, n * kWeld};
  for (const Arg *a : {&st, &rq, &we})
    if (rc == LIFEAPI_OK) rc = check_ptr(fn, *a);
  if (rc == LIFEAPI_OK) rc = check_clear(fn, we, {st, rq});
  if (rc != LIFEAPI_OK) return rc;
  return launch(k_weld_from_required<kFromRequiredU>, "k_weld_from_required launch",
                Grid{(n + kFromRequiredU - 1) / kFromRequiredU}, stream, Written{d_welds, (uint64_t)n * kWeld},
                d_states, d_required, per_universe_required ? 1u : 0u, d_welds, n);
}

int lifeapi_weld_to_target_batch_dev(const uint64_t *d_welds, uint64_t *d_wanted, uint64_t *d_unwanted, size_t n,
                                     void *stream) {
  static const char fn[] = "lifeapi_weld_to_target_batch_dev";
  if (n == 0) return LIFEAPI_OK;
  int rc = check_n(fn, n);
  const Arg we{"d_welds", d_welds, n * kWeld}, wa{"d_wanted", d_wanted, n * kState},
      un{"d_unwanted", d_unwanted, n * kState};
  for (const Arg *a : {&we, &wa, &un})
    if (rc == LIFEAPI_OK) rc = check_ptr(fn, *a);
  if (rc == LIFEAPI_OK) rc = check_clear(fn, wa, {we, un});
  if (rc == LIFEAPI_OK) rc = check_clear(fn, un, {we});
  if (rc != LIFEAPI_OK) return rc;
  // (the wanted plane is the batch a later launch reads as states)
  return launch(k_weld_to_target<kToTargetU>, "k_weld_to_target launch", Grid{(n + kToTargetU - 1) / kToTargetU},
                stream, Written{d_wanted, (uint64_t)n * kState}, d_welds, d_wanted, d_unwanted, n);
}

int lifeapi_weld_to_stable_batch_dev(const uint64_t *d_welds, const uint64_t *d_active, int per_universe_active,
                                     const uint64_t *d_mask, uint32_t duration, uint64_t *d_stables, size_t n,
                                     void *stream) {
  static const char fn[] = "lifeapi_weld_to_stable_batch_dev";
  if (duration > kMaxDuration) return fail(LIFEAPI_E_INVALID, "%s: duration > 65536", fn);
  if (n == 0) return LIFEAPI_OK;
  int rc = check_n(fn, n);
  const Arg we{"d_welds", d_welds, n * kWeld},
      ac{"d_active", d_active, per_universe_active ? n * kState : kState}, ma{"d_mask", d_mask, kState},
      sb{"d_stables", d_stables, n * kStable};
  for (const Arg *a : {&we, &sb})
    if (rc == LIFEAPI_OK) rc = check_ptr(fn, *a);
  for (const Arg *a : {&ac, &ma})  // optional
    if (rc == LIFEAPI_OK && a->p) rc = check_ptr(fn, *a);
  if (rc == LIFEAPI_OK) rc = check_clear(fn, sb, {we, ac, ma});
  if (rc != LIFEAPI_OK) return rc;
  return launch(k_weld_to_stable, "k_weld_to_stable launch", Grid{n}, stream, Written{d_stables, (uint64_t)n * kStable},
                d_welds, d_active, per_universe_active ? 1u : 0u, d_mask, duration, d_stables, n);
}

int lifeapi_weld_interaction_offsets_batch_dev(const uint64_t *d_welds, const uint64_t *d_other, uint64_t *d_out,
                                               size_t n, void *stream) {
  static const char fn[] = "lifeapi_weld_interaction_offsets_batch_dev";
  if (n == 0) return LIFEAPI_OK;
  int rc = check_n(fn, n);
  const Arg we{"d_welds", d_welds, n * kWeld}, ot{"d_other", d_other, kWeld}, ou{"d_out", d_out, n * kState};
  for (const Arg *a : {&we, &ot, &ou})
    if (rc == LIFEAPI_OK) rc = check_ptr(fn, *a);
  if (rc == LIFEAPI_OK) rc = check_clear(fn, ou, {we, ot});
  if (rc != LIFEAPI_OK) return rc;
  return launch(k_weld_interaction_offsets<kOffsetsU>, "k_weld_interaction_offsets launch",
                Grid{(n + kOffsetsU - 1) / kOffsetsU}, stream, Written{d_out, (uint64_t)n * kState}, d_welds, d_other,
                d_out, n);
}

}  // extern "C"
