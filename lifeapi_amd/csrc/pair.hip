// pair.hip -- the entry points with both operands per universe: Convolve of
// a universe with a transformed universe and IntersectingOffsets
// (Symmetry.hpp:729-772), and Halve / HalveX / HalveY / Skew / InvSkew
// (Symmetry.hpp:681-727) over a batch (pair_kernels.hpp).
#include "launch.hpp"
#include "pair_kernels.hpp"

using namespace lifeapi_impl;

namespace {

// universes per wave (their loads issued first)
constexpr int kPairU = 4, kHalveU = 4, kSkewU = 4;

// the transform IntersectingOffsets applies to pat1 (Symmetry.hpp:733-767),
// by StaticSymmetry value; -1 where the reference has none
int intersecting_transform(uint32_t symmetry) {
  switch (symmetry) {
  case kC2: return 0;             // Identity
  case kC4: return 8;             // Rotate270
  case kD2AcrossX: return 4;      // ReflectAcrossY
  case kD2AcrossY: return 2;      // ReflectAcrossX
  case kD2diagodd: return 15;     // ReflectAcrossYeqNegXP1
  case kD2negdiagodd: return 13;  // ReflectAcrossYeqX
  default: return -1;
  }
}

}  // namespace

extern "C" {

int lifeapi_convolve_pair_batch_dev(const uint64_t *d_a, const uint64_t *d_b, uint32_t transform, uint64_t *d_out,
                                    size_t n, void *stream) {
  if (transform > 15) return fail(LIFEAPI_E_INVALID, "lifeapi_convolve_pair_batch_dev: transform must be 0..15%s");
  if (n == 0) return LIFEAPI_OK;
  // each pair of the three batches equal or disjoint
  int rc = check_batch(d_a, d_out, n);
  if (rc == LIFEAPI_OK) rc = check_batch(d_b, d_out, n);
  if (rc == LIFEAPI_OK && d_a != d_b && ranges_overlap(d_a, n * 512, d_b, n * 512))
    rc = fail(LIFEAPI_E_INVALID, "lifeapi_convolve_pair_batch_dev: the operands overlap (only d_b == d_a is allowed)%s");
  if (rc != LIFEAPI_OK) return rc;
  const Affine t = backwards(kTransforms[transform]);
  const uint32_t plain = transform == 0;
  return d_a == d_b ? launch_groups(k_convolve_pair<true, kPairU>, "k_convolve_pair launch", kPairU, stream, d_out, kStateBytes, n,
                                    d_a, d_b, d_out, t, plain, n)
                    : launch_groups(k_convolve_pair<false, kPairU>, "k_convolve_pair launch", kPairU, stream, d_out, kStateBytes, n,
                                    d_a, d_b, d_out, t, plain, n);
}

int lifeapi_intersecting_offsets_batch_dev(const uint64_t *d_pat1, const uint64_t *d_pat2, uint32_t symmetry,
                                           uint64_t *d_out, size_t n, void *stream) {
  const int t = intersecting_transform(symmetry);
  if (t < 0)
    return fail(LIFEAPI_E_INVALID,
                "lifeapi_intersecting_offsets_batch_dev: IntersectingOffsets is undefined for this symmetry%s");
  // pat2.Convolve(pat1.Transformed(t)): pat1 is the transformed operand
  return lifeapi_convolve_pair_batch_dev(d_pat2, d_pat1, (uint32_t)t, d_out, n, stream);
}

int lifeapi_halve_batch_dev(const uint64_t *d_in, uint64_t *d_out, size_t n, uint32_t mode, void *stream) {
  if (mode > 2) return fail(LIFEAPI_E_INVALID, "lifeapi_halve_batch_dev: mode must be 0 (Halve), 1 (HalveX) or 2 (HalveY)%s");
  if (n == 0) return LIFEAPI_OK;
  const int rc = check_batch(d_in, d_out, n);
  if (rc != LIFEAPI_OK) return rc;
  return launch_groups(k_halve<kHalveU>, "k_halve launch", kHalveU, stream, d_out, kStateBytes, n, d_in, d_out, mode, n);
}

int lifeapi_skew_batch_dev(const uint64_t *d_in, uint64_t *d_out, size_t n, int inverse, void *stream) {
  if (n == 0) return LIFEAPI_OK;
  const int rc = check_batch(d_in, d_out, n);
  if (rc != LIFEAPI_OK) return rc;
  return launch_groups(k_skew<kSkewU>, "k_skew launch", kSkewU, stream, d_out, kStateBytes, n, d_in, d_out,
                       (uint32_t)(inverse != 0), n);
}

}  // extern "C"
