// match.hip -- the per-offset entry points: Match (LifeTarget.hpp:53-55,
// LifeAPI.hpp:432-435), Convolve (LifeAPI.hpp:1293-1370) and
// InteractionOffsets (LifeAPI.hpp:1066-1095) over a batch, one pattern per
// launch (match_kernels.hpp).
#include "launch.hpp"
#include "match_kernels.hpp"

using namespace lifeapi_impl;

namespace {

// universes per wave (their loads issued first)
constexpr int kMatchU = 4, kInteractionU = 2;

// the 64 device words of a pattern: non-null, aligned, not written by the call
int check_pattern(const void *pat, const void *d_out, size_t n, const char *what) {
  if (!pat || !aligned8(pat)) return fail(LIFEAPI_E_INVALID, "null or misaligned pattern pointer to %s", what);
  if (d_out && ranges_overlap(pat, kStateBytes, d_out, n * kStateBytes))
    return fail(LIFEAPI_E_INVALID, "the pattern overlaps the output batch of %s", what);
  return LIFEAPI_OK;
}

}  // namespace

extern "C" {

int lifeapi_match_batch_dev(const uint64_t *d_states, const uint64_t *d_wanted, const uint64_t *d_unwanted,
                            uint64_t *d_out, uint32_t *d_count, size_t n, void *stream) {
  if (n == 0) return LIFEAPI_OK;
  if (!d_out && !d_count) return fail(LIFEAPI_E_INVALID, "lifeapi_match_batch_dev: both d_out and d_count are null%s");
  int rc = d_out ? check_batch(d_states, d_out, n) : check_batch(d_states, d_states, n);
  if (rc == LIFEAPI_OK) rc = check_pattern(d_wanted, d_out, n, "lifeapi_match_batch_dev");
  if (rc == LIFEAPI_OK) rc = check_pattern(d_unwanted, d_out, n, "lifeapi_match_batch_dev");
  if (rc != LIFEAPI_OK) return rc;
  if (d_count) {
    if ((uintptr_t)d_count & 3u) return fail(LIFEAPI_E_INVALID, "lifeapi_match_batch_dev: misaligned d_count%s");
    if (ranges_overlap(d_count, n * 4, d_states, n * 512) || (d_out && ranges_overlap(d_count, n * 4, d_out, n * 512)) ||
        ranges_overlap(d_count, n * 4, d_wanted, 512) || ranges_overlap(d_count, n * 4, d_unwanted, 512))
      return fail(LIFEAPI_E_INVALID, "lifeapi_match_batch_dev: d_count overlaps another argument%s");
  }
  return launch_groups(k_match<kMatchU>, "k_match launch", kMatchU, stream, d_out, kStateBytes, n, d_states, d_out, d_wanted,
                       d_unwanted, d_count, n);
}

int lifeapi_convolve_batch_dev(const uint64_t *d_states, const uint64_t *d_pattern, uint64_t *d_out, size_t n,
                               void *stream) {
  if (n == 0) return LIFEAPI_OK;
  int rc = check_batch(d_states, d_out, n);
  if (rc == LIFEAPI_OK) rc = check_pattern(d_pattern, d_out, n, "lifeapi_convolve_batch_dev");
  if (rc != LIFEAPI_OK) return rc;
  return launch_groups(k_convolve<kMatchU>, "k_convolve launch", kMatchU, stream, d_out, kStateBytes, n, d_states, d_out,
                       d_pattern, n);
}

int lifeapi_interaction_offsets_batch_dev(const uint64_t *d_states, const uint64_t *d_other, uint64_t *d_out,
                                          size_t n, void *stream) {
  if (n == 0) return LIFEAPI_OK;
  int rc = check_batch(d_states, d_out, n);
  if (rc == LIFEAPI_OK) rc = check_pattern(d_other, d_out, n, "lifeapi_interaction_offsets_batch_dev");
  if (rc != LIFEAPI_OK) return rc;
  return launch_groups(k_interaction_offsets<kInteractionU>, "k_interaction_offsets launch", kInteractionU, stream,
                       d_out, kStateBytes, n, d_states, d_out, d_other, n);
}

}  // extern "C"
