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
constexpr uint32_t kMaxDuration = 65536;

}  // namespace

extern "C" {

int lifeapi_weld_from_required_batch_dev(const uint64_t *d_states, const uint64_t *d_required,
                                         int per_universe_required, uint64_t *d_welds, size_t n, void *stream) {
  static const char fn[] = "lifeapi_weld_from_required_batch_dev";
  if (n == 0) return LIFEAPI_OK;
  int rc = check_n(fn, n);
  const Arg st{"d_states", d_states, n * kStateBytes}, rq{"d_required", d_required, per_universe_required ? n * kStateBytes : kStateBytes},
      we{"d_welds", d_welds, n * kWeldBytes};
  for (const Arg *a : {&st, &rq, &we})
    if (rc == LIFEAPI_OK) rc = check_ptr(fn, *a);
  if (rc == LIFEAPI_OK) rc = check_clear(fn, we, {st, rq});
  if (rc != LIFEAPI_OK) return rc;
  return launch_groups(k_weld_from_required<kFromRequiredU>, "k_weld_from_required launch", kFromRequiredU, stream,
                       d_welds, kWeldBytes, n, d_states, d_required, per_universe_required ? 1u : 0u, d_welds, n);
}

int lifeapi_weld_to_target_batch_dev(const uint64_t *d_welds, uint64_t *d_wanted, uint64_t *d_unwanted, size_t n,
                                     void *stream) {
  static const char fn[] = "lifeapi_weld_to_target_batch_dev";
  if (n == 0) return LIFEAPI_OK;
  int rc = check_n(fn, n);
  const Arg we{"d_welds", d_welds, n * kWeldBytes}, wa{"d_wanted", d_wanted, n * kStateBytes},
      un{"d_unwanted", d_unwanted, n * kStateBytes};
  for (const Arg *a : {&we, &wa, &un})
    if (rc == LIFEAPI_OK) rc = check_ptr(fn, *a);
  if (rc == LIFEAPI_OK) rc = check_clear(fn, wa, {we, un});
  if (rc == LIFEAPI_OK) rc = check_clear(fn, un, {we});
  if (rc != LIFEAPI_OK) return rc;
  // (the wanted plane is the batch a later launch reads as states)
  return launch_groups(k_weld_to_target<kToTargetU>, "k_weld_to_target launch", kToTargetU, stream, d_wanted,
                       kStateBytes, n, d_welds, d_wanted, d_unwanted, n);
}

int lifeapi_weld_to_stable_batch_dev(const uint64_t *d_welds, const uint64_t *d_active, int per_universe_active,
                                     const uint64_t *d_mask, uint32_t duration, uint64_t *d_stables, size_t n,
                                     void *stream) {
  static const char fn[] = "lifeapi_weld_to_stable_batch_dev";
  if (duration > kMaxDuration) return fail(LIFEAPI_E_INVALID, "%s: duration > 65536", fn);
  if (n == 0) return LIFEAPI_OK;
  int rc = check_n(fn, n);
  const Arg we{"d_welds", d_welds, n * kWeldBytes},
      ac{"d_active", d_active, per_universe_active ? n * kStateBytes : kStateBytes}, ma{"d_mask", d_mask, kStateBytes},
      sb{"d_stables", d_stables, n * kStableBytes};
  for (const Arg *a : {&we, &sb})
    if (rc == LIFEAPI_OK) rc = check_ptr(fn, *a);
  for (const Arg *a : {&ac, &ma})  // optional
    if (rc == LIFEAPI_OK && a->p) rc = check_ptr(fn, *a);
  if (rc == LIFEAPI_OK) rc = check_clear(fn, sb, {we, ac, ma});
  if (rc != LIFEAPI_OK) return rc;
  return launch_groups(k_weld_to_stable, "k_weld_to_stable launch", 1, stream, d_stables, kStableBytes, n, d_welds,
                       d_active, per_universe_active ? 1u : 0u, d_mask, duration, d_stables, n);
}

int lifeapi_weld_interaction_offsets_batch_dev(const uint64_t *d_welds, const uint64_t *d_other, uint64_t *d_out,
                                               size_t n, void *stream) {
  static const char fn[] = "lifeapi_weld_interaction_offsets_batch_dev";
  if (n == 0) return LIFEAPI_OK;
  int rc = check_n(fn, n);
  const Arg we{"d_welds", d_welds, n * kWeldBytes}, ot{"d_other", d_other, kWeldBytes}, ou{"d_out", d_out, n * kStateBytes};
  for (const Arg *a : {&we, &ot, &ou})
    if (rc == LIFEAPI_OK) rc = check_ptr(fn, *a);
  if (rc == LIFEAPI_OK) rc = check_clear(fn, ou, {we, ot});
  if (rc != LIFEAPI_OK) return rc;
  return launch_groups(k_weld_interaction_offsets<kOffsetsU>, "k_weld_interaction_offsets launch", kOffsetsU, stream,
                       d_out, kStateBytes, n, d_welds, d_other, d_out, n);
}

}  // extern "C"
