// symmetry.hip -- the symmetry layer's entry points: Transform then Move
// (Symmetry.hpp:105-173, LifeAPI.hpp:682-735), Symmetricize (Symmetry.hpp:
// 565-654), XYBounds (LifeAPI.hpp:446-484) and SymmetryOrbit[Representatives]
// (Symmetry.hpp:798-830) over a batch, one transform / symmetry and offset per
// launch (symmetry_kernels.hpp).  The host restates each as at most two
// affine maps of the torus.
#include "launch.hpp"
#include "symmetry_kernels.hpp"

using namespace lifeapi_impl;

namespace {

// universes per wave (their loads issued first)
constexpr int kTransformU = 4, kSymmetricizeU = 4, kBoundsU = 4, kOrbitU = 2;

// A forward affine map of the torus, (x, y) -> (sx x + bx, sy y + by), or
// with `swap` (sx y + bx, sy x + by): where the cell at (x, y) goes.
struct Forward {
  bool swap;
  int sx, sy;
  long long bx, by;
};

// The 16 SymmetryTransforms in the enum's order (Symmetry.hpp:7-26), read
// off Transform (Symmetry.hpp:105-173): FlipX is (x, -y - 1), FlipY
// (-x - 1, y), Transpose(false) (y, x), Transpose(true) (-y - 1, -x - 1),
// Move(a, b) adds (a, b).
constexpr Forward kTransforms[16] = {
    {false, 1, 1, 0, 0},     // Identity
    {false, 1, -1, 0, -1},   // ReflectAcrossXEven
    {false, 1, -1, 0, 0},    // ReflectAcrossX
    {false, -1, 1, -1, 0},   // ReflectAcrossYEven
    {false, -1, 1, 0, 0},    // ReflectAcrossY
    {true, -1, 1, -1, 0},    // Rotate90Even
    {true, -1, 1, 0, 0},     // Rotate90
    {true, 1, -1, 0, -1},    // Rotate270Even
    {true, 1, -1, 0, 0},     // Rotate270
    {false, -1, -1, 0, 0},   // Rotate180OddBoth
    {false, -1, -1, -1, 0},  // Rotate180EvenHorizontal
    {false, -1, -1, 0, -1},  // Rotate180EvenVertical
    {false, -1, -1, -1, -1}, // Rotate180EvenBoth
    {true, 1, 1, 0, 0},      // ReflectAcrossYeqX
    {true, -1, -1, -1, -1},  // ReflectAcrossYeqNegX
    {true, -1, -1, 0, 0},    // ReflectAcrossYeqNegXP1
};

Forward moved(Forward f, long long dx, long long dy) {
  f.bx += dx;
  f.by += dy;
  return f;
}

uint32_t mod64(long long v) { return (uint32_t)(((v % 64) + 64) % 64); }

// The map read backwards, as the kernels apply it (symmetry_kernels.hpp):
// out(X, Y) = in(sx (X - bx), sy (Y - by)); with swap out(X, Y) = g(Y, X),
// g(u, v) = in(sy (u - by), sx (v - bx)).
Affine backwards(const Forward &f) {
  const int cs = f.swap ? f.sy : f.sx, rs = f.swap ? f.sx : f.sy;
  const long long cb = f.swap ? f.by : f.bx, rb = f.swap ? f.bx : f.by;
  Affine a;
  a.colflip = cs < 0;
  a.coloff = mod64(-cs * cb);
  a.rowflip = rs < 0;
  const uint32_t r = mod64(-rs * rb);  // w'(y) = w(+-y + r)
  a.rowrot = a.rowflip ? (63u - r) & 63u : r;
  a.transpose = f.swap;
  return a;
}

// PerpComponent (Symmetry.hpp:540-563) for the two diagonal reflections, in
// the reference's own int arithmetic (truncating / and %): not a function of
// the offset mod 64 alone
void perp_diag(int ox, int oy, bool negative, int &px, int &py) {
  const int x = (ox + 32) % 64 - 32, y = (oy + 32) % 64 - 32;
  if (negative) {
    px = py = ((x + y + 128) / 2) % 64;
  } else {
    px = ((x - y + 128) / 2) % 64;
    py = ((-x + y + 128) / 2) % 64;
  }
}

// StaticSymmetry values (Symmetry.hpp:57-79) Symmetricize defines
enum : uint32_t { kC1 = 0, kD2AcrossX = 1, kD2AcrossY = 3, kD2negdiagodd = 5, kD2diagodd = 6, kC2 = 7, kC4 = 11,
                  kD4 = 13, kD4diag = 17 };

// Symmetricize(state, symmetry, {dx, dy}) as rounds of acc |= map(acc)
// (Symmetry.hpp:565-654); -1 for a symmetry the reference leaves undefined
int symmetricize_maps(uint32_t symmetry, int dx, int dy, Forward (&m)[2]) {
  const long long x = dx, y = dy;
  switch (symmetry) {
  case kC1: return 0;
  case kC2:  // FlipX, FlipY, Move(dx + 1, dy + 1)
    m[0] = moved(kTransforms[12], x + 1, y + 1);
    return 1;
  case kC4:  // Rotate90, Move(offset); then FlipX, FlipY, Move(dx - dy + 1, dy + dx + 1)
    m[0] = moved(kTransforms[6], x, y);
    m[1] = moved(kTransforms[12], x - y + 1, y + x + 1);
    return 2;
  case kD2AcrossX:  // FlipX, Move(dx, dy + 1)
    m[0] = moved(kTransforms[1], x, y + 1);
    return 1;
  case kD2AcrossY:  // FlipY, Move(dx + 1, dy)
    m[0] = moved(kTransforms[3], x + 1, y);
    return 1;
  case kD2diagodd:  // ReflectAcrossYeqX, Move(offset)
    m[0] = moved(kTransforms[13], x, y);
    return 1;
  case kD2negdiagodd:  // Transpose(true), Move(dx + 1, dy + 1)
    m[0] = moved(kTransforms[14], x + 1, y + 1);
    return 1;
  case kD4:  // PerpComponent(ReflectAcrossX) = (0, dy), PerpComponent(ReflectAcrossY) = (dx, 0)
    m[0] = moved(kTransforms[1], 0, y + 1);
    m[1] = moved(kTransforms[3], x + 1, 0);
    return 2;
  case kD4diag: {
    int px, py, qx, qy;
    perp_diag(dx, dy, false, px, py);
    perp_diag(dx, dy, true, qx, qy);
    m[0] = moved(kTransforms[13], px, py);
    m[1] = moved(kTransforms[14], (long long)qx + 1, (long long)qy + 1);
    return 2;
  }
  default: return -1;
  }
}

// one wave per group of U universes, a wave for every group (the kernels'
// loops only run again on a grid capped at 2^30 blocks)
template <class... P, class... A>
int launch_groups(void (*kernel)(P...), const char *what, int U, void *stream, uint64_t *d_out, size_t n, A... args) {
  return launch(kernel, what, Grid{(n + U - 1) / U}, stream,
                d_out ? Written{d_out, (uint64_t)n * 512} : kWritesNoBatch, args...);
}

// a per-universe output of `bytes` each: aligned, clear of the states
int check_side(const void *p, size_t align, size_t bytes, const void *d_states, size_t n, const char *what) {
  if ((uintptr_t)p & (align - 1)) return fail(LIFEAPI_E_INVALID, "misaligned output of %s", what);
  if (n > SIZE_MAX / bytes || ranges_overlap(p, n * bytes, d_states, n * 512))
    return fail(LIFEAPI_E_INVALID, "an output of %s overlaps the input batch", what);
  return LIFEAPI_OK;
}

}  // namespace

extern "C" {

int lifeapi_transform_batch_dev(const uint64_t *d_in, uint64_t *d_out, size_t n, uint32_t transform, int dx, int dy,
                                void *stream) {
  if (transform > 15) return fail(LIFEAPI_E_INVALID, "lifeapi_transform_batch_dev: transform must be 0..15%s");
  if (n == 0) return LIFEAPI_OK;
  const int rc = check_batch(d_in, d_out, n);
  if (rc != LIFEAPI_OK) return rc;
  const Affine a = backwards(moved(kTransforms[transform], dx, dy));
  return a.transpose ? launch_groups(k_transform<true, kTransformU>, "k_transform launch", kTransformU, stream, d_out,
                                     n, d_in, d_out, a, n)
                     : launch_groups(k_transform<false, kTransformU>, "k_transform launch", kTransformU, stream, d_out,
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
  return launch_groups(k_symmetricize<kSymmetricizeU>, "k_symmetricize launch", kSymmetricizeU, stream, d_out, n, d_in,
                       d_out, maps, (uint32_t)rounds, n);
}

int lifeapi_bounds_batch_dev(const uint64_t *d_states, int32_t *d_bounds, size_t n, void *stream) {
  if (n == 0) return LIFEAPI_OK;
  if (!d_bounds) return fail(LIFEAPI_E_INVALID, "lifeapi_bounds_batch_dev: null d_bounds%s");
  int rc = check_batch(d_states, d_states, n);
  if (rc == LIFEAPI_OK) rc = check_side(d_bounds, 4, 16, d_states, n, "lifeapi_bounds_batch_dev");
  if (rc != LIFEAPI_OK) return rc;
  return launch_groups(k_bounds<kBoundsU>, "k_bounds launch", kBoundsU, stream, nullptr, n, d_states, d_bounds, n);
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
  return launch(k_symmetry_orbit<kOrbitU>, "k_symmetry_orbit launch", Grid{(n + kOrbitU - 1) / kOrbitU}, stream,
                d_images ? Written{d_images, (uint64_t)n * 8 * 512} : kWritesNoBatch, d_states, d_images, d_first, n);
}

}  // extern "C"
