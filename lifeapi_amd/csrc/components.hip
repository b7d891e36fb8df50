// components.hip -- the connected-component entry points: FirstOn
// (LifeAPI.hpp:301-323), ComponentContaining (LifeAPI.hpp:655-665, 1184-1188)
// and Components (LifeAPI.hpp:667-676, 1189-1193) over a batch, one corona per
// launch (components_kernels.hpp).  The corona is a host pointer: it is
// checked and classified here and handed to the kernel by value.
#include "launch.hpp"
#include "components_kernels.hpp"

using namespace lifeapi_impl;

namespace {

// universes per wave (their loads issued first; the flood runs until all of
// a wave's universes have converged)
constexpr int kFirstOnU = 4, kContainingU = 2;

void set_cell(Corona &c, int a, int b) { c.w[a & 63] |= uint64_t(1) << (b & 63); }

// the coronas with a fixed network (components_kernels.hpp), centred on (0, 0)
Corona fixed_corona(int kind) {
  Corona c{};
  for (int a = -2; a <= 2; ++a)
    for (int b = -2; b <= 2; ++b) {
      const int m = (a < 0 ? -a : a), k = (b < 0 ? -b : b);
      const bool in = kind == kDefault ? m + k < 4 : kind == k3x3 ? m <= 1 && k <= 1 : m + k <= 1;
      if (in) set_cell(c, a, b);
    }
  return c;
}

// the caller's corona (NULL = the reference's default, b3o$5o$5o$5o$b3o! at
// (-2, -2), LifeAPI.hpp:1185-1186) and the network that computes it
int classify(const uint64_t *corona, Corona &c) {
  if (!corona) {
    c = fixed_corona(kDefault);
    return kDefault;
  }
  for (int x = 0; x < kWave; ++x) c.w[x] = corona[x];
  for (int kind : {kDefault, k3x3, kPlus}) {
    const Corona f = fixed_corona(kind);
    bool same = true;
    for (int x = 0; x < kWave; ++x) same = same && f.w[x] == c.w[x];
    if (same) return kind;
  }
  return kGeneral;
}

template <int KIND>
int launch_containing(void *stream, const uint64_t *d_states, const uint64_t *d_seeds, int per, const Corona &c,
                      uint64_t *d_out, size_t n) {
  return launch_groups(k_component_containing<KIND, kContainingU>, "k_component_containing launch", kContainingU,
                       stream, d_out, kStateBytes, n, d_states, d_seeds, per ? 1u : 0u, c, d_out, n);
}

template <int KIND>
int launch_components(void *stream, const uint64_t *d_states, const Corona &c, uint32_t *d_count,
                      uint64_t *d_components, uint32_t max_components, size_t n) {
  return launch_groups(k_components<KIND>, "k_components launch", 1, stream, d_components,
                       (uint64_t)max_components * kStateBytes, n, d_states, c, d_count, d_components, max_components, n);
}

}  // namespace

extern "C" {

int lifeapi_first_on_batch_dev(const uint64_t *d_states, int32_t *d_cells, size_t n, void *stream) {
  if (n == 0) return LIFEAPI_OK;
  if (!d_cells) return fail(LIFEAPI_E_INVALID, "lifeapi_first_on_batch_dev: null d_cells%s");
  int rc = check_batch(d_states, d_states, n);
  if (rc == LIFEAPI_OK) rc = check_side(d_cells, 4, 8, d_states, n, "lifeapi_first_on_batch_dev");
  if (rc != LIFEAPI_OK) return rc;
  return launch_groups(k_first_on<kFirstOnU>, "k_first_on launch", kFirstOnU, stream, nullptr, 0, n, d_states, d_cells,
                       n);
}

int lifeapi_component_containing_batch_dev(const uint64_t *d_states, const uint64_t *d_seeds, int per_universe_seeds,
                                           const uint64_t *corona, uint64_t *d_out, size_t n, void *stream) {
  Corona c;
  const int kind = classify(corona, c);
  if (n == 0) return LIFEAPI_OK;
  int rc = check_batch(d_states, d_out, n);
  if (rc != LIFEAPI_OK) return rc;
  if (!d_seeds || !aligned8(d_seeds))
    return fail(LIFEAPI_E_INVALID, "lifeapi_component_containing_batch_dev: null or misaligned d_seeds%s");
  if (per_universe_seeds) {
    if ((rc = check_batch(d_seeds, d_out, n)) != LIFEAPI_OK) return rc;
  } else if (ranges_overlap(d_seeds, 512, d_out, n * 512)) {
    return fail(LIFEAPI_E_INVALID, "lifeapi_component_containing_batch_dev: the seed overlaps the output batch%s");
  }
  switch (kind) {
  case kDefault: return launch_containing<kDefault>(stream, d_states, d_seeds, per_universe_seeds, c, d_out, n);
  case k3x3: return launch_containing<k3x3>(stream, d_states, d_seeds, per_universe_seeds, c, d_out, n);
  case kPlus: return launch_containing<kPlus>(stream, d_states, d_seeds, per_universe_seeds, c, d_out, n);
  default: return launch_containing<kGeneral>(stream, d_states, d_seeds, per_universe_seeds, c, d_out, n);
  }
}

int lifeapi_components_batch_dev(const uint64_t *d_states, const uint64_t *corona, uint32_t *d_count,
                                 uint64_t *d_components, uint32_t max_components, size_t n, void *stream) {
  Corona c;
  const int kind = classify(corona, c);
  // without its centre the seed's component is empty and the reference's
  // loop (LifeAPI.hpp:670-674) never ends
  if (!(c.w[0] & 1u))
    return fail(LIFEAPI_E_INVALID,
                "lifeapi_components_batch_dev: the corona must contain cell (0, 0) (Components never ends without it)%s");
  if (n == 0) return LIFEAPI_OK;
  if (!d_count && !d_components)
    return fail(LIFEAPI_E_INVALID, "lifeapi_components_batch_dev: both d_count and d_components are null%s");
  if (d_components && max_components == 0)
    return fail(LIFEAPI_E_INVALID, "lifeapi_components_batch_dev: d_components with max_components == 0%s");
  int rc = check_batch(d_states, d_states, n);
  if (rc == LIFEAPI_OK && d_count) rc = check_side(d_count, 4, 4, d_states, n, "lifeapi_components_batch_dev");
  if (rc == LIFEAPI_OK && d_components)
    rc = check_side(d_components, 8, (size_t)max_components * 512, d_states, n, "lifeapi_components_batch_dev");
  if (rc == LIFEAPI_OK && d_count && d_components &&
      ranges_overlap(d_count, n * 4, d_components, n * max_components * 512))
    rc = fail(LIFEAPI_E_INVALID, "lifeapi_components_batch_dev: d_count overlaps d_components%s");
  if (rc != LIFEAPI_OK) return rc;
  switch (kind) {
  case kDefault: return launch_components<kDefault>(stream, d_states, c, d_count, d_components, max_components, n);
  case k3x3: return launch_components<k3x3>(stream, d_states, c, d_count, d_components, max_components, n);
  case kPlus: return launch_components<kPlus>(stream, d_states, c, d_count, d_components, max_components, n);
  default: return launch_components<kGeneral>(stream, d_states, c, d_count, d_components, max_components, n);
  }
}

}  // extern "C"
