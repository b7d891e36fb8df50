// symmetry.hip -- the symmetry layer's entry points: Transform then Move
// (Symmetry.hpp:105-173, LifeAPI.hpp:682-735), Symmetricize (Symmetry.hpp:
// 565-654), XYBounds (LifeAPI.hpp:446-484) and SymmetryOrbit[Representatives]
// (Symmetry.hpp:798-830) over a batch, one transform / symmetry per launch and one
// offset per launch or per universe (symmetry_kernels.hpp, where the
// descriptors that restate each as at most two affine maps of the torus are).
#include "launch.hpp"
#include "symmetry_kernels.hpp"

using namespace lifeapi_impl;

namespace {

// universes per wave (their loads issued first)
constexpr int kTransformU = 4, kSymmetricizeU = 4, kBoundsU = 4, kOrbitU = 2;

}  // namespace

extern "C" {

int lifeapi_transform_batch_dev(const uint64_t *d_in, uint64_t *d_out, size_t n, uint32_t transform, int dx, int dy,
                                void *stream) {
  if (transform > 15) return fail(LIFEAPI_E_INVALID, "lifeapi_transform_batch_dev: transform must be 0..15%s");
  if (n == 0) return LIFEAPI_OK;
  const int rc = check_batch(d_in, d_out, n);
  if (rc != LIFEAPI_OK) return rc;
  const Affine a = backwards(moved(kTransforms[transform], dx, dy));
  return a.transpose ? launch_groups(k_transform<true, kTransformU>, "k_transform launch", kTransformU, stream, d_out, kStateBytes,
                                     n, d_in, d_out, a, n)
                     : launch_groups(k_transform<false, kTransformU>, "k_transform launch", kTransformU, stream, d_out, kStateBytes,
                                     n, d_in, d_out, a, n);
}

int lifeapi_symmetricize_batch_dev(const uint64_t *d_in, uint64_t *d_out, size_t n, uint32_t symmetry, int dx, int dy,
                                   void *stream) {
  Forward m[2] = {kTransforms[0], kTransforms[0]};
  const int rounds = symmetricize_maps(symmetry, dx, dy, m);
  if (rounds < 0)
    return fail(LIFEAPI_E_INVALID, "lifeapi_symmetricize_batch_dev: Symmetricize is undefined for this symmetry%s");
  if (n == 0) return LIFEAPI_OK;
  const int rc = check_batch(d_in, d_out, n);
  if (rc != LIFEAPI_OK) return rc;
  const Affine2 maps{{backwards(m[0]), backwards(m[1])}};
  return launch_groups(k_symmetricize<kSymmetricizeU>, "k_symmetricize launch", kSymmetricizeU, stream, d_out, kStateBytes, n, d_in,
                       d_out, maps, (uint32_t)rounds, n);
}

// n x {dx, dy} int32 device words: non-null, aligned, not written by the call
static int check_offsets(const int32_t *d_offsets, const uint64_t *d_out, size_t n, const char *what) {
  if (!d_offsets || ((uintptr_t)d_offsets & 3u)) return fail(LIFEAPI_E_INVALID, "null or misaligned d_offsets to %s", what);
  if (n > SIZE_MAX / 512 || ranges_overlap(d_offsets, n * 8, d_out, n * 512))
    return fail(LIFEAPI_E_INVALID, "d_offsets overlaps the output batch of %s", what);
  return LIFEAPI_OK;
}

int lifeapi_transform_offsets_batch_dev(const uint64_t *d_in, uint64_t *d_out, size_t n, uint32_t transform,
                                        const int32_t *d_offsets, void *stream) {
  if (transform > 15) return fail(LIFEAPI_E_INVALID, "lifeapi_transform_offsets_batch_dev: transform must be 0..15%s");
  if (n == 0) return LIFEAPI_OK;
  int rc = check_batch(d_in, d_out, n);
  if (rc == LIFEAPI_OK) rc = check_offsets(d_offsets, d_out, n, "lifeapi_transform_offsets_batch_dev");
  if (rc != LIFEAPI_OK) return rc;
  const Forward base = kTransforms[transform];
  return base.swap ? launch_groups(k_transform_offsets<true, kTransformU>, "k_transform_offsets launch", kTransformU,
                                   stream, d_out, kStateBytes, n, d_in, d_out, base, d_offsets, n)
                   : launch_groups(k_transform_offsets<false, kTransformU>, "k_transform_offsets launch", kTransformU,
                                   stream, d_out, kStateBytes, n, d_in, d_out, base, d_offsets, n);
}

int lifeapi_symmetricize_offsets_batch_dev(const uint64_t *d_in, uint64_t *d_out, size_t n, uint32_t symmetry,
                                           const int32_t *d_offsets, void *stream) {
  Forward m[2] = {kTransforms[0], kTransforms[0]};
  if (symmetricize_maps(symmetry, 0, 0, m) < 0)
    return fail(LIFEAPI_E_INVALID,
                "lifeapi_symmetricize_offsets_batch_dev: Symmetricize is undefined for this symmetry%s");
  if (n == 0) return LIFEAPI_OK;
  int rc = check_batch(d_in, d_out, n);
  if (rc == LIFEAPI_OK) rc = check_offsets(d_offsets, d_out, n, "lifeapi_symmetricize_offsets_batch_dev");
  if (rc != LIFEAPI_OK) return rc;
  return launch_groups(k_symmetricize_offsets<kSymmetricizeU>, "k_symmetricize_offsets launch", kSymmetricizeU, stream,
                       d_out, kStateBytes, n, d_in, d_out, symmetry, d_offsets, n);
}

int lifeapi_bounds_batch_dev(const uint64_t *d_states, int32_t *d_bounds, size_t n, void *stream) {
  if (n == 0) return LIFEAPI_OK;
  if (!d_bounds) return fail(LIFEAPI_E_INVALID, "lifeapi_bounds_batch_dev: null d_bounds%s");
  int rc = check_batch(d_states, d_states, n);
  if (rc == LIFEAPI_OK) rc = check_side(d_bounds, 4, 16, d_states, n, "lifeapi_bounds_batch_dev");
  if (rc != LIFEAPI_OK) return rc;
  return launch_groups(k_bounds<kBoundsU>, "k_bounds launch", kBoundsU, stream, nullptr, 0, n, d_states, d_bounds, n);
}

int lifeapi_symmetry_orbit_batch_dev(const uint64_t *d_states, uint64_t *d_images, uint8_t *d_first, size_t n,
                                     void *stream) {
  if (n == 0) return LIFEAPI_OK;
  if (!d_images && !d_first)
    return fail(LIFEAPI_E_INVALID, "lifeapi_symmetry_orbit_batch_dev: both d_images and d_first are null%s");
  int rc = check_batch(d_states, d_states, n);
  if (rc == LIFEAPI_OK && d_images)
    rc = check_side(d_images, 8, 8 * 512, d_states, n, "lifeapi_symmetry_orbit_batch_dev");
  if (rc == LIFEAPI_OK && d_first) rc = check_side(d_first, 1, 1, d_states, n, "lifeapi_symmetry_orbit_batch_dev");
  if (rc == LIFEAPI_OK && d_images && d_first && ranges_overlap(d_first, n, d_images, n * 8 * 512))
    rc = fail(LIFEAPI_E_INVALID, "lifeapi_symmetry_orbit_batch_dev: d_first overlaps d_images%s");
  if (rc != LIFEAPI_OK) return rc;
  return launch_groups(k_symmetry_orbit<kOrbitU>, "k_symmetry_orbit launch", kOrbitU, stream, d_images, 8 * kStateBytes,
                       n, d_states, d_images, d_first, n);
}

}  // extern "C"
