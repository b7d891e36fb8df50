// stable_test.hip -- the LifeStable lookahead entry points: the strip passes
// (LifeStable.hpp:921-948, 995-1249), TestUnknowns (:1321-1338) and
// PropagateAndTest (:163-184) over a batch (stable_test_kernels.hpp).  Every
// argument is checked before a device is touched.
#include "launch.hpp"
#include "stable_test_kernels.hpp"

using namespace lifeapi_impl;

namespace {

// The strip passes' waves loop over the batch from a grid of at most this many
// blocks per CU (their work is bound by the 5 KiB they load).  The lookahead
// kernels take one wave per LifeStable instead (Grid{n}; their loop only serves
// a grid that launch() had to cap): an object costs them some hundred
// microseconds of VALU work that depends on its data, and a wave that walks a
// fixed stride through the batch takes whatever its objects cost -- on a batch
// that repeats with the grid's period the same wave took every slow object
// (1M objects, PropagateAndTest: 228 ms with 3 blocks per CU, 171 ms with 8).
constexpr int kBlocksPerCu = 8;

using StripFn = void (*)(uint64_t *, const uint8_t *, uint8_t *, uint64_t, uint32_t);
const StripFn kStripPasses[6] = {k_stable_strip<0>, k_stable_strip<1>, k_stable_strip<2>,
                                 k_stable_strip<3>, k_stable_strip<4>, k_stable_strip<5>};

int test_launch(const char *fn, bool test_unknowns, uint64_t *d_planes, const uint64_t *d_cells, int per_object_cells,
                uint8_t *d_flags, size_t n, uint32_t max_iters, void *stream) {
  if (n == 0) return LIFEAPI_OK;
  int rc = check_n(fn, n);
  const Arg pl{"d_planes", d_planes, n * kStableBytes, true}, fl{"d_flags", d_flags, n, false},
      ce{"d_cells", d_cells, per_object_cells ? n * kStateBytes : kStateBytes, true};
  if (rc == LIFEAPI_OK) rc = check_ptr(fn, pl);
  if (rc == LIFEAPI_OK) rc = check_ptr(fn, fl);
  if (rc == LIFEAPI_OK && test_unknowns) rc = check_ptr(fn, ce);
  if (rc == LIFEAPI_OK) rc = check_clear(fn, fl, {pl});
  if (rc == LIFEAPI_OK && test_unknowns) rc = check_clear(fn, ce, {pl});
  if (rc != LIFEAPI_OK) return rc;
  return launch(test_unknowns ? k_stable_test<0> : k_stable_test<1>,
                test_unknowns ? "k_stable_test<0> launch" : "k_stable_test<1> launch", Grid{n}, stream,
                Written{d_planes, (uint64_t)n * kStableBytes}, d_planes, d_cells, per_object_cells ? 1u : 0u, d_flags, n,
                max_iters ? max_iters : 1u << 20);
}

}  // namespace

extern "C" {

int lifeapi_stable_strip_pass_batch_dev(uint64_t *d_planes, const uint8_t *d_columns, uint8_t *d_flags, size_t n,
                                        int pass, uint32_t max_iters, void *stream) {
  static const char fn[] = "lifeapi_stable_strip_pass_batch_dev";
  if (pass < 0 || pass > 5) return fail(LIFEAPI_E_INVALID, "%s: pass outside 0..5", fn);
  if (n == 0) return LIFEAPI_OK;
  int rc = check_n(fn, n);
  const Arg pl{"d_planes", d_planes, n * kStableBytes, true}, co{"d_columns", d_columns, n, false},
      fl{"d_flags", d_flags, n, false};
  for (const Arg *a : {&pl, &co, &fl})
    if (rc == LIFEAPI_OK) rc = check_ptr(fn, *a);
  for (const Arg *a : {&co, &fl})
    if (rc == LIFEAPI_OK) rc = check_clear(fn, *a, {pl});
  if (rc != LIFEAPI_OK) return rc;
  return launch(kStripPasses[pass], "k_stable_strip launch", Grid{n, kBlocksPerCu}, stream,
                Written{d_planes, (uint64_t)n * kStableBytes}, d_planes, d_columns, d_flags, n,
                max_iters ? max_iters : 1u << 20);
}

int lifeapi_stable_test_unknowns_batch_dev(uint64_t *d_planes, const uint64_t *d_cells, int per_object_cells,
                                           uint8_t *d_flags, size_t n, uint32_t max_iters, void *stream) {
  return test_launch("lifeapi_stable_test_unknowns_batch_dev", true, d_planes, d_cells, per_object_cells, d_flags, n,
                     max_iters, stream);
}

int lifeapi_stable_propagate_and_test_batch_dev(uint64_t *d_planes, uint8_t *d_flags, size_t n, uint32_t max_iters,
                                                void *stream) {
  return test_launch("lifeapi_stable_propagate_and_test_batch_dev", false, d_planes, nullptr, 0, d_flags, n, max_iters,
                     stream);
}

}  // extern "C"
