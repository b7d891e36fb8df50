// host.hpp -- host-side helpers shared by the kernel files (host.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <functional>
#include <initializer_list>
#include <string>

#include "common.hpp"
#include "lifeapi_hip.h"

namespace lifeapi_impl {

extern thread_local std::string g_err;  // lifeapi_last_error()

// set g_err (fmt has one %s for arg) and return code
int fail(int code, const char *fmt, const char *arg = nullptr);
// set g_err from a HIP error; missing code objects map to LIFEAPI_E_NOKERNEL
int fail_hip(hipError_t e, const char *what);
// CUs of the current device, which must be a gfx950
int device_cus(int &cus);
// unused dynamic LDS per block that leaves exactly min(blocks_per_cu, what
// the kernel's registers allow) blocks of `kernel` resident per CU of the
// current device (an occupancy cap), checked against the occupancy API
int occupancy_lds(const void *kernel, int blocks_per_cu, unsigned &bytes);
bool aligned8(const void *p);
inline bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }
// [a, a + abytes) and [b, b + bbytes) share a byte
inline bool ranges_overlap(const void *a, size_t abytes, const void *b, size_t bbytes) {
  return (uintptr_t)a < (uintptr_t)b + bbytes && (uintptr_t)b < (uintptr_t)a + abytes;
}
// n universes in / out: non-null, 8-byte aligned, equal or disjoint
int check_batch(const void *in, const void *out, size_t n);
// The argument checks of the entry points that name the offending argument
// (weld.hip, stable_test.hip): fn is the entry point, for the message.
struct Arg {
  const char *name;
  const void *p;
  size_t bytes;  // in all
  bool align8 = true;
};
// non-null and, with align8, 8-byte aligned
int check_ptr(const char *fn, const Arg &a);
// a clear of every non-null array of `others` ("<a> overlaps <other>")
int check_clear(const char *fn, const Arg &a, std::initializer_list<Arg> others);
// n objects of any kind (the largest, a LifeStable) fit a size_t
int check_n(const char *fn, size_t n);
// a per-universe output of `bytes` each: aligned, clear of the states
// (symmetry.hip, components.hip)
int check_side(const void *p, size_t align, size_t bytes, const void *d_states, size_t n, const char *what);
// blocks for `waves_needed` waves, capped at cus * blocks_per_cu (0 = no cap)
unsigned grid_for(uint64_t waves_needed, int cus, int blocks_per_cu);
// the launch's error state as a return code
int launched(const char *what);

struct DeviceGuard {  // restores the caller's current device
  int prev = -1;
  DeviceGuard() { (void)hipGetDevice(&prev); }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// One host array taking part in a host-pointer call: `bytes` per universe;
// src -> copied in before each chunk's launch, dst -> copied out after it
// (src == dst for in-place arrays).  whole: `bytes` in all, the same for
// every universe (a target): all of it is copied in before every chunk's
// launch, to a 256-byte-aligned device address; never a dst.
struct HostIO {
  const void *src;
  void *dst;
  size_t bytes;
  bool whole = false;
  size_t span(size_t m) const { return whole ? bytes : m * bytes; }  // bytes holding m universes
};
constexpr size_t kMaxHostArrays = 8;  // per call
// the stream-ordered *_dev call on one staged chunk: dev[k] is the device
// copy of array k, m the chunk's universes
using ChunkFn = std::function<int(void *const *dev, size_t m, hipStream_t s)>;

// Stages n universes through each device's reusable buffers in chunks that
// alternate between two streams: H2D, fn, D2H, all asynchronous, then one
// sync of both streams.  device >= 0: that device; -1: one contiguous shard
// per visible device, each on its own host thread (host.hip over_devices).
int host_batch(size_t n, int device, std::initializer_list<HostIO> io, const ChunkFn &fn);
// the device a host-pointer call runs on (-1 = device 0), or an error code
int host_device(int device);

}  // namespace lifeapi_impl
