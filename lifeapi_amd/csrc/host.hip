// host.hip -- host side of the C ABI: errors, device checks, launch
// geometry, the staging used by every host-pointer entry point, and those
// entry points that only stage data around a *_dev call.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "launch.hpp"

namespace lifeapi_impl {

thread_local std::string g_err;

int fail(int code, const char *fmt, const char *arg) {
  char buf[512];
  std::snprintf(buf, sizeof buf, fmt, arg ? arg : "");
  g_err = buf;
  return code;
}
int fail_hip(hipError_t e, const char *what) {
  // the error is reported through our return code: consume HIP's sticky
  // per-thread copy, or the next launch's hipGetLastError() would return it
  (void)hipGetLastError();
  char buf[512];
  std::snprintf(buf, sizeof buf, "%s: %s (hipError %d)", what, hipGetErrorString(e), (int)e);
  g_err = buf;
  if (e == hipErrorNoBinaryForGpu || e == hipErrorInvalidDeviceFunction ||
      e == hipErrorInvalidImage || e == hipErrorSharedObjectInitFailed)
    return LIFEAPI_E_NOKERNEL;
  return (int)e;
}

struct DevInfo {
  int cus = 0;
  size_t lds_per_cu = 0;
  bool ok = false;
};
std::mutex g_info_mu;
std::vector<DevInfo> g_info;

static int device_info(DevInfo &out) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return fail_hip(e, "hipGetDevice");
  std::lock_guard<std::mutex> lk(g_info_mu);
  if ((int)g_info.size() <= dev) g_info.resize(dev + 1);
  if (!g_info[dev].ok) {
    hipDeviceProp_t p;
    e = hipGetDeviceProperties(&p, dev);
    if (e != hipSuccess) return fail_hip(e, "hipGetDeviceProperties");
    if (std::strncmp(p.gcnArchName, "gfx950", 6) != 0)
      return fail(LIFEAPI_E_NODEVICE, "device is %s, this library is built for gfx950 only",
                  p.gcnArchName);
    g_info[dev].cus = p.multiProcessorCount;
    g_info[dev].lds_per_cu = p.maxSharedMemoryPerMultiProcessor;
    g_info[dev].ok = true;
  }
  out = g_info[dev];
  return LIFEAPI_OK;
}

int device_cus(int &cus) {
  DevInfo d;
  const int rc = device_info(d);
  cus = d.cus;
  return rc;
}

// occupancy_lds results per (device, kernel, blocks per CU): the answer
// depends on nothing else, and computing it takes several occupancy queries
struct OccKey {
  int dev;
  const void *kernel;
  int blocks;
  bool operator<(const OccKey &o) const {
    return std::tie(dev, kernel, blocks) < std::tie(o.dev, o.kernel, o.blocks);
  }
};
std::mutex g_occ_mu;
std::map<OccKey, unsigned> g_occ;

static int occupancy_lds_uncached(const void *kernel, int blocks_per_cu, unsigned &bytes);

int occupancy_lds(const void *kernel, int blocks_per_cu, unsigned &bytes) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return fail_hip(e, "hipGetDevice");
  const OccKey key{dev, kernel, blocks_per_cu};
  {
    std::lock_guard<std::mutex> lk(g_occ_mu);
    auto it = g_occ.find(key);
    if (it != g_occ.end()) {
      bytes = it->second;
      return LIFEAPI_OK;
    }
  }
  const int rc = occupancy_lds_uncached(kernel, blocks_per_cu, bytes);
  if (rc == LIFEAPI_OK) {
    std::lock_guard<std::mutex> lk(g_occ_mu);
    g_occ[key] = bytes;
  }
  return rc;
}

static int occupancy_lds_uncached(const void *kernel, int blocks_per_cu, unsigned &bytes) {
  DevInfo d;
  int rc = device_info(d);
  if (rc != LIFEAPI_OK) return rc;
  if (blocks_per_cu < 1) return fail(LIFEAPI_E_INVALID, "occupancy cap below one block per CU%s");
  hipFuncAttributes fa;
  hipError_t e = hipFuncGetAttributes(&fa, kernel);
  if (e != hipSuccess) return fail_hip(e, "hipFuncGetAttributes");
  int free_blocks = 0;  // what the kernel's registers and static LDS allow
  e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&free_blocks, kernel, kBlock, 0);
  if (e != hipSuccess) return fail_hip(e, "hipOccupancyMaxActiveBlocksPerMultiprocessor");
  if (free_blocks < 1) return fail(LIFEAPI_E_INVALID, "kernel cannot be resident%s");
  const int want = std::min(blocks_per_cu, free_blocks);
  // round DOWN: k blocks of (static + dynamic) LDS must fit in the CU's LDS
  // (rounding up to the granule allowed one block fewer whenever k does not
  // divide it: 6 -> 5, 3 -> 2)
  const size_t per_block = d.lds_per_cu / (size_t)want;
  size_t dyn = per_block > fa.sharedSizeBytes ? (per_block - fa.sharedSizeBytes) & ~(size_t)255 : 0;
  for (;; dyn -= 256) {
    int got = 0;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&got, kernel, kBlock, dyn);
    if (e != hipSuccess) return fail_hip(e, "hipOccupancyMaxActiveBlocksPerMultiprocessor");
    if (got >= want) break;  // the granule rounded us above the share: shrink
    if (dyn < 256) return fail(LIFEAPI_E_INVALID, "cannot set the occupancy cap%s");
  }
  bytes = (unsigned)dyn;
  return LIFEAPI_OK;
}

// ---- launch order keyed on the batch (launch.hpp launch_reverse) ----
namespace {
constexpr int kOrderDevices = 64, kOrderSlots = 8;
struct OrderSlot {
  uintptr_t ptr = 0;
  uint64_t bytes = 0, tick = 0;
  bool reverse = false;
};
struct OrderBook {
  std::mutex mu;
  OrderSlot slot[kOrderSlots];
  uint64_t tick = 0;
};
OrderBook g_order[kOrderDevices];

OrderBook *order_book() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kOrderDevices) return nullptr;
  return &g_order[dev];
}

// forget every batch overlapping [p, p + bytes), then remember it written in
// order `rev` (the least recently written slot makes room); mu held
void order_record(OrderBook &b, uintptr_t p, uint64_t bytes, bool rev) {
  OrderSlot *victim = &b.slot[0];
  for (OrderSlot &s : b.slot) {
    if (s.bytes && s.ptr < p + bytes && p < s.ptr + s.bytes) s = OrderSlot{};
    if (!s.bytes || (victim->bytes && s.tick < victim->tick)) victim = &s;
  }
  *victim = OrderSlot{p, bytes, ++b.tick, rev};
}
}  // namespace

bool launch_reverse(const void *d_in, const void *d_out, uint64_t bytes) {
  OrderBook *b = order_book();
  if (!b || bytes == 0) return false;
  std::lock_guard<std::mutex> lk(b->mu);
  bool rev = false;
  for (const OrderSlot &s : b->slot)
    if (s.bytes == bytes && s.ptr == (uintptr_t)d_in) rev = !s.reverse;
  order_record(*b, (uintptr_t)d_out, bytes, rev);
  return rev;
}

void note_forward_write(const void *d_out, uint64_t bytes) {
  OrderBook *b = order_book();
  if (!b || bytes == 0) return;
  std::lock_guard<std::mutex> lk(b->mu);
  order_record(*b, (uintptr_t)d_out, bytes, false);
}

bool aligned8(const void *p) { return ((uintptr_t)p & 7u) == 0; }

int check_batch(const void *in, const void *out, size_t n) {
  if (n == 0) return LIFEAPI_OK;
  if (!in || !out) return fail(LIFEAPI_E_INVALID, "null universe pointer%s");
  if (!aligned8(in) || !aligned8(out)) return fail(LIFEAPI_E_INVALID, "universe pointers must be 8-byte aligned%s");
  if (n > (SIZE_MAX / 512)) return fail(LIFEAPI_E_INVALID, "n too large%s");
  if (in != out && ranges_overlap(in, n * 512, out, n * 512))
    return fail(LIFEAPI_E_INVALID, "input and output batches overlap (only in == out is allowed)%s");
  return LIFEAPI_OK;
}

int check_ptr(const char *fn, const Arg &a) {
  if (!a.p) return fail(LIFEAPI_E_INVALID, (std::string(fn) + ": null " + a.name + "%s").c_str());
  if (a.align8 && !aligned8(a.p))
    return fail(LIFEAPI_E_INVALID, (std::string(fn) + ": misaligned " + a.name + "%s").c_str());
  return LIFEAPI_OK;
}
int check_clear(const char *fn, const Arg &a, std::initializer_list<Arg> others) {
  for (const Arg &o : others)
    if (o.p && ranges_overlap(a.p, a.bytes, o.p, o.bytes))
      return fail(LIFEAPI_E_INVALID, (std::string(fn) + ": " + a.name + " overlaps " + o.name + "%s").c_str());
  return LIFEAPI_OK;
}
int check_n(const char *fn, size_t n) {
  return n > SIZE_MAX / kStableBytes ? fail(LIFEAPI_E_INVALID, "%s: n too large", fn) : LIFEAPI_OK;
}
int check_side(const void *p, size_t align, size_t bytes, const void *d_states, size_t n, const char *what) {
  if ((uintptr_t)p & (align - 1)) return fail(LIFEAPI_E_INVALID, "misaligned output of %s", what);
  if (n > SIZE_MAX / bytes || ranges_overlap(p, n * bytes, d_states, n * kStateBytes))
    return fail(LIFEAPI_E_INVALID, "an output of %s overlaps the input batch", what);
  return LIFEAPI_OK;
}

unsigned grid_for(uint64_t waves_needed, int cus, int blocks_per_cu) {
  uint64_t blocks = (waves_needed + kWavesPerBlock - 1) / kWavesPerBlock;
  if (blocks_per_cu > 0) blocks = std::min<uint64_t>(blocks, (uint64_t)cus * blocks_per_cu);
  blocks = std::min<uint64_t>(blocks, 1u << 30);
  return (unsigned)std::max<uint64_t>(blocks, 1);
}

int launched(const char *what) {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? LIFEAPI_OK : fail_hip(e, what);
}

// ---- host-pointer staging: one context per device ----
// Chunks alternate between two streams, each with its own staging buffer,
// and everything is issued asynchronously before one final sync per call.
// Stream order alone protects a buffer's reuse (chunk k + 2 waits for chunk
// k's D2H on the same stream).  Chunk k's H2D also waits (event) for chunk
// k-1's H2D, so the two streams run one chunk apart and chunk k's D2H
// overlaps chunk k+1's H2D; without that they start in phase and both
// directions stay serialised.  That pays only for page-locked host arrays:
// the runtime serialises pageable copies in both directions.  So every call
// moving at least kPinMinBytes page-locks the caller's arrays itself for its
// duration (hipHostRegister, then hipHostUnregister): on MI355X that costs
// under 1 ms and takes 1M universes from 19.4 to 12.2-13.1 ms
// (profiles/r01/host_bench.jsonl).  Arrays the caller pinned already
// (lifeapi_host_register) or that cannot be pinned are used as they are.
// An array that is not per-universe data (HostIO::whole: the 512-byte halves
// of a Contains target) has a slot of its own in each lane's buffer and is
// copied in again ahead of every chunk's launch, on the chunk's stream: the
// call owns no other device memory, and stream order is all that keeps a
// launch behind its target.
constexpr int kLanes = 2;  // (the event chain below assumes two)
constexpr size_t kChunkBytes = size_t(64) << 20;  // staging per stream and pass
constexpr size_t kPinMinBytes = size_t(8) << 20;  // smaller calls stay pageable

// Ranges this library pinned, shared by every call in the process: a call
// whose array lies inside one takes a reference instead of registering again,
// so concurrent calls (other threads, the per-device shards of a device = -1
// call) never unpin memory another call is still copying.
struct PinRec {
  uintptr_t lo, hi;
  int refs;
};
std::mutex g_pin_mu;
std::vector<PinRec> g_pins;

// Adds to `keys` a reference on every range this library pinned that
// overlaps [p, p + bytes) -- whatever the call's size, so no other call can
// unpin memory this call's copies may DMA from, even where the ranges only
// partly overlap.  With no overlap, a call of at least kPinMinBytes pins the
// array itself (and references that); smaller calls, arrays the caller
// pinned and unpinnable memory are used as they are.  Each key goes back
// through pin_release.
void pin_acquire(const void *p, size_t bytes, std::vector<uintptr_t> &keys) {
  if (!p || !bytes) return;
  const uintptr_t lo = (uintptr_t)p, hi = lo + bytes;
  std::lock_guard<std::mutex> lk(g_pin_mu);
  bool overlap = false;
  for (PinRec &r : g_pins)
    if (lo < r.hi && r.lo < hi) {
      ++r.refs;
      keys.push_back(r.lo);
      overlap = true;
    }
  if (overlap || bytes < kPinMinBytes) return;
  // Leave ranges the caller pinned alone: the runtime accepts a second
  // registration without counting it, so our unregister would undo theirs
  // (tools/ab/pin_probe.cpp; hipHostGetFlags fails on registered memory, the
  // pointer attributes report it as host memory).
  for (uintptr_t q : {lo, hi - 1}) {
    hipPointerAttribute_t a{};
    const hipError_t e = hipPointerGetAttributes(&a, (const void *)q);
    (void)hipGetLastError();
    if (e != hipSuccess || a.type != hipMemoryTypeUnregistered) return;
  }
  if (hipHostRegister((void *)lo, bytes, hipHostRegisterPortable) != hipSuccess) {
    (void)hipGetLastError();
    return;
  }
  g_pins.push_back({lo, hi, 1});
  keys.push_back(lo);
}

void pin_release(uintptr_t key) {
  if (!key) return;
  std::lock_guard<std::mutex> lk(g_pin_mu);
  for (size_t k = 0; k < g_pins.size(); ++k)
    if (g_pins[k].lo == key) {
      if (--g_pins[k].refs == 0) {
        if (hipHostUnregister((void *)key) != hipSuccess) (void)hipGetLastError();
        g_pins.erase(g_pins.begin() + k);
      }
      return;
    }
}

// Holds pin_acquire references for one call.
struct CallPins {
  std::vector<uintptr_t> keys;
  void add(const void *p, size_t bytes) { pin_acquire(p, bytes, keys); }
  ~CallPins() {
    for (uintptr_t k : keys) pin_release(k);
  }
};

struct HostCtx {
  std::mutex mu;
  hipStream_t stream[kLanes] = {};
  hipEvent_t h2d_done[kLanes] = {};
  char *buf[kLanes] = {};
  size_t cap = 0;  // bytes per stream
};
std::mutex g_ctx_mu;
std::vector<HostCtx *> g_ctx;

HostCtx *ctx_for(int dev) {
  std::lock_guard<std::mutex> lk(g_ctx_mu);
  if ((int)g_ctx.size() <= dev) g_ctx.resize(dev + 1, nullptr);
  if (!g_ctx[dev]) g_ctx[dev] = new HostCtx();  // lives for the process
  return g_ctx[dev];
}

// n universes of io[0..nio) (nio <= kMaxHostArrays: host_batch) on device
// dev.  Chunks are disjoint ranges of every per-universe array, so in-place
// arrays (src == dst) are safe.
static int host_chunked(int dev, size_t n, const HostIO *io, size_t nio, const ChunkFn &fn) {
  DeviceGuard guard;
  hipError_t e = hipSetDevice(dev);
  if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
  HostCtx *c = ctx_for(dev);
  std::lock_guard<std::mutex> lk(c->mu);
  for (int l = 0; l < kLanes; ++l)
    if (!c->stream[l]) {
      e = hipStreamCreateWithFlags(&c->stream[l], hipStreamNonBlocking);
      if (e != hipSuccess) return fail_hip(e, "hipStreamCreate");
      e = hipEventCreateWithFlags(&c->h2d_done[l], hipEventDisableTiming);
      if (e != hipSuccess) return fail_hip(e, "hipEventCreate");
    }
  size_t per = 0;  // (whole arrays do not move the chunk boundaries)
  for (size_t k = 0; k < nio; ++k)
    if (!io[k].whole) per += (io[k].bytes + 255) & ~size_t(255);
  const size_t half = (n + kLanes - 1) / kLanes;
  const size_t chunk = std::max<size_t>(1, std::min(half, kChunkBytes / per));
  size_t need = 0;
  for (size_t k = 0; k < nio; ++k) need += (io[k].span(chunk) + 255) & ~size_t(255);
  if (c->cap < need) {
    for (int l = 0; l < kLanes; ++l) {
      if (c->buf[l]) (void)hipFree(c->buf[l]);
      c->buf[l] = nullptr;
    }
    c->cap = 0;
    for (int l = 0; l < kLanes; ++l) {
      e = hipMalloc(&c->buf[l], need);
      if (e != hipSuccess) return fail_hip(e, "hipMalloc(staging)");
    }
    c->cap = need;
  }
  // page-lock the caller's arrays for this call (see above)
  CallPins pins;
  for (size_t q = 0; q < nio; ++q) {
    pins.add(io[q].src, io[q].span(n));
    if (io[q].dst != io[q].src) pins.add(io[q].dst, io[q].span(n));
  }
  int rc = LIFEAPI_OK;
  void *d[kMaxHostArrays];
  for (size_t k = 0; k * chunk < n && rc == LIFEAPI_OK; ++k) {
    const int l = (int)(k % kLanes);
    hipStream_t st = c->stream[l];
    const size_t off = k * chunk, m = std::min(chunk, n - off);
    if (k > 0 && (e = hipStreamWaitEvent(st, c->h2d_done[1 - l], 0)) != hipSuccess) {
      rc = fail_hip(e, "hipStreamWaitEvent");
      break;
    }
    size_t pos = 0;
    for (size_t q = 0; q < nio && rc == LIFEAPI_OK; ++q) {
      d[q] = c->buf[l] + pos;
      pos += (io[q].span(chunk) + 255) & ~size_t(255);
      const size_t at = io[q].whole ? 0 : off * io[q].bytes;
      if (io[q].src && (e = hipMemcpyAsync(d[q], (const char *)io[q].src + at, io[q].span(m),
                                           hipMemcpyHostToDevice, st)) != hipSuccess)
        rc = fail_hip(e, "hipMemcpyAsync(H2D)");
    }
    if (rc == LIFEAPI_OK && (e = hipEventRecord(c->h2d_done[l], st)) != hipSuccess)
      rc = fail_hip(e, "hipEventRecord");
    if (rc == LIFEAPI_OK) rc = fn(d, m, st);
    for (size_t q = 0; q < nio && rc == LIFEAPI_OK; ++q)
      if (io[q].dst && !io[q].whole &&
          (e = hipMemcpyAsync((char *)io[q].dst + off * io[q].bytes, d[q], m * io[q].bytes,
                              hipMemcpyDeviceToHost, st)) != hipSuccess)
        rc = fail_hip(e, "hipMemcpyAsync(D2H)");
  }
  // drain both streams even after an error: nothing may still read or write
  // the caller's arrays once we return
  for (int l = 0; l < kLanes; ++l) {
    e = hipStreamSynchronize(c->stream[l]);
    if (e != hipSuccess && rc == LIFEAPI_OK) rc = fail_hip(e, "hipStreamSynchronize");
  }
  return rc;  // (both streams synchronised: the pins can go)
}

int host_device(int device) {
  const int ndev = lifeapi_device_count();
  if (ndev <= 0) return fail(LIFEAPI_E_NODEVICE, "no HIP device visible%s");
  if (device < 0) device = 0;
  if (device >= ndev) return fail(LIFEAPI_E_NODEVICE, "bad device index%s");
  return device;
}

// device >= 0: fn(0, n, device) on that device.  device -1: one contiguous
// shard per visible device, fn(lo, hi, dev) on one host thread each, with the
// host arrays page-locked once for all shards (shard boundaries share
// pages).  LIFEAPI_HOST_SHARDS=k (1 <= k <= 64, else LIFEAPI_E_INVALID; empty = unset)
// overrides the shard count (at most n shards), shard s
// running on device s mod ndev: a rehearsal knob that runs the threaded path
// on a machine with fewer GPUs (tests/test_host_multidev.py).  The first
// failing shard's code and message are returned.
constexpr long kMaxHostShards = 64;
template <class F>
static int over_devices(size_t n, int device, std::initializer_list<HostIO> io, F &&fn) {
  const int ndev = lifeapi_device_count();
  if (ndev <= 0) return fail(LIFEAPI_E_NODEVICE, "no HIP device visible%s");
  if (device >= ndev || device < -1) return fail(LIFEAPI_E_NODEVICE, "bad device index%s");
  int shards = ndev;
  if (device < 0) {
    const char *e = std::getenv("LIFEAPI_HOST_SHARDS");
    if (e && *e) {  // (set but empty = unset, as `export LIFEAPI_HOST_SHARDS=` leaves it)
      char *end = nullptr;
      const long k = std::strtol(e, &end, 10);
      if (end == e || *end != '\0' || k < 1 || k > kMaxHostShards)
        return fail(LIFEAPI_E_INVALID, "LIFEAPI_HOST_SHARDS must be an integer in 1..64, not '%s'", e);
      shards = (int)k;
    }
    shards = (int)std::min<size_t>((size_t)shards, std::max<size_t>(n, 1));  // no empty shards
  }
  if (device >= 0 || shards == 1) return fn(0, n, device < 0 ? 0 : device);
  CallPins pins;
  for (const HostIO &a : io) {
    pins.add(a.src, a.span(n));
    if (a.dst != a.src) pins.add(a.dst, a.span(n));
  }
  std::vector<int> rcs(shards, LIFEAPI_OK);
  std::vector<std::string> errs(shards);
  std::vector<std::thread> pool;
  for (int k = 0; k < shards; ++k) {
    const size_t lo = n * k / shards, hi = n * (k + 1) / shards;
    pool.emplace_back([&, k, lo, hi] {
      if (hi > lo) rcs[k] = fn(lo, hi, k % ndev);
      errs[k] = g_err;
    });
  }
  for (auto &t : pool) t.join();
  for (int k = 0; k < shards; ++k)
    if (rcs[k] != LIFEAPI_OK) {
      g_err = errs[k];
      return rcs[k];
    }
  return LIFEAPI_OK;
}

// host_chunked over device(s): device >= 0 one device, -1 every visible one
// (over_devices), each shard's per-universe arrays offset by its first
// universe, whole arrays as they are
int host_batch(size_t n, int device, std::initializer_list<HostIO> io, const ChunkFn &fn) {
  if (io.size() > kMaxHostArrays) return fail(LIFEAPI_E_INVALID, "too many arrays%s");
  return over_devices(n, device, io, [&](size_t lo, size_t hi, int dev) {
    HostIO sh[kMaxHostArrays];
    size_t k = 0;
    for (HostIO a : io) {
      if (a.src && !a.whole) a.src = (const char *)a.src + lo * a.bytes;
      if (a.dst && !a.whole) a.dst = (char *)a.dst + lo * a.bytes;
      sh[k++] = a;
    }
    return host_chunked(dev, hi - lo, sh, k, fn);
  });
}

}  // namespace lifeapi_impl

using namespace lifeapi_impl;

extern "C" {

int lifeapi_abi_version(void) { return LIFEAPI_ABI_VERSION; }

const char *lifeapi_last_error(void) { return g_err.c_str(); }

int lifeapi_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int lifeapi_step_batch(const uint64_t *in, uint64_t *out, size_t n, uint32_t generations,
                       int device) {
  int rc = check_batch(in, out, n);
  if (rc != LIFEAPI_OK || n == 0) return rc;
  return host_batch(n, device, {{in, out, 512}}, [=](void *const *d, size_t m, hipStream_t s) {
    return lifeapi_step_batch_dev((const uint64_t *)d[0], (uint64_t *)d[0], m, generations, s);
  });
}

int lifeapi_host_register(void *p, size_t bytes) {
  if (!p || bytes == 0) return fail(LIFEAPI_E_INVALID, "null or empty range to lifeapi_host_register%s");
  if (lifeapi_device_count() <= 0) return fail(LIFEAPI_E_NODEVICE, "no HIP device visible%s");
  const hipError_t e = hipHostRegister(p, bytes, hipHostRegisterPortable);
  return e == hipSuccess ? LIFEAPI_OK : fail_hip(e, "hipHostRegister");
}

int lifeapi_host_unregister(void *p) {
  if (!p) return fail(LIFEAPI_E_INVALID, "null pointer to lifeapi_host_unregister%s");
  if (lifeapi_device_count() <= 0) return fail(LIFEAPI_E_NODEVICE, "no HIP device visible%s");
  const hipError_t e = hipHostUnregister(p);
  return e == hipSuccess ? LIFEAPI_OK : fail_hip(e, "hipHostUnregister");
}

int lifeapi_pop_batch(const uint64_t *states, uint32_t *pop, size_t n, int device) {
  if (n == 0) return LIFEAPI_OK;
  if (!states || !pop || !aligned8(states)) return fail(LIFEAPI_E_INVALID, "bad pointer to lifeapi_pop_batch%s");
  return host_batch(n, device, {{states, nullptr, 512}, {nullptr, pop, 4}},
                    [](void *const *d, size_t m, hipStream_t s) {
                      return lifeapi_pop_batch_dev((const uint64_t *)d[0], (uint32_t *)d[1], m, s);
                    });
}

int lifeapi_weld_step_batch(uint64_t *welds, size_t n, uint32_t generations, int device) {
  if (n == 0) return LIFEAPI_OK;
  if (!welds || !aligned8(welds)) return fail(LIFEAPI_E_INVALID, "bad pointer to lifeapi_weld_step_batch%s");
  return host_batch(n, device, {{welds, welds, 4 * 512}}, [=](void *const *d, size_t m, hipStream_t s) {
    return lifeapi_weld_step_batch_dev((uint64_t *)d[0], m, generations, s);
  });
}

int lifeapi_stable_pass_batch(uint64_t *planes, uint8_t *flags, size_t n, int pass,
                              uint32_t max_iters, int device) {
  if (n == 0) return LIFEAPI_OK;
  if (!planes || !flags || !aligned8(planes) || pass < 0 || pass > 5)
    return fail(LIFEAPI_E_INVALID, "bad argument to lifeapi_stable_pass_batch%s");
  return host_batch(n, device, {{planes, planes, 10 * 512}, {nullptr, flags, 1}},
                    [=](void *const *d, size_t m, hipStream_t s) {
                      return lifeapi_stable_pass_batch_dev((uint64_t *)d[0], (uint8_t *)d[1], m, pass,
                                                           max_iters, s);
                    });
}

int lifeapi_stable_vulnerable_batch(const uint64_t *planes, uint64_t *out, size_t n, int device) {
  if (n == 0) return LIFEAPI_OK;
  if (!planes || !out || !aligned8(planes) || !aligned8(out))
    return fail(LIFEAPI_E_INVALID, "bad pointer to lifeapi_stable_vulnerable_batch%s");
  return host_batch(n, device, {{planes, nullptr, 10 * 512}, {nullptr, out, 512}},
                    [](void *const *d, size_t m, hipStream_t s) {
                      return lifeapi_stable_vulnerable_batch_dev((const uint64_t *)d[0], (uint64_t *)d[1], m, s);
                    });
}

int lifeapi_neighbour_count_batch(const uint64_t *in, uint64_t *out, size_t n, int device) {
  if (n == 0) return LIFEAPI_OK;
  if (!in || !out || !aligned8(in) || !aligned8(out))
    return fail(LIFEAPI_E_INVALID, "bad pointer to lifeapi_neighbour_count_batch%s");
  return host_batch(n, device, {{in, nullptr, 512}, {nullptr, out, 4 * 512}},
                    [](void *const *d, size_t m, hipStream_t s) {
                      return lifeapi_neighbour_count_batch_dev((const uint64_t *)d[0], (uint64_t *)d[1], m, s);
                    });
}

int lifeapi_interaction_counts_batch(const uint64_t *in, uint64_t *out, size_t n, int with_next,
                                     int device) {
  if (n == 0) return LIFEAPI_OK;
  if (!in || !out || !aligned8(in) || !aligned8(out))
    return fail(LIFEAPI_E_INVALID, "bad pointer to lifeapi_interaction_counts_batch%s");
  return host_batch(n, device, {{in, nullptr, 512}, {nullptr, out, (with_next ? 4u : 3u) * 512}},
                    [=](void *const *d, size_t m, hipStream_t s) {
                      return lifeapi_interaction_counts_batch_dev((const uint64_t *)d[0], (uint64_t *)d[1], m,
                                                                  with_next, s);
                    });
}

int lifeapi_refined_step_batch(const uint64_t *in, uint64_t *out, size_t n, int device) {
  if (n == 0) return LIFEAPI_OK;
  if (!in || !out || !aligned8(in) || !aligned8(out))
    return fail(LIFEAPI_E_INVALID, "bad pointer to lifeapi_refined_step_batch%s");
  return host_batch(n, device, {{in, nullptr, 11 * 512}, {nullptr, out, 3 * 512}},
                    [](void *const *d, size_t m, hipStream_t s) {
                      return lifeapi_refined_step_batch_dev((const uint64_t *)d[0], (uint64_t *)d[1], m, s);
                    });
}

int lifeapi_contains_batch(const uint64_t *states, const uint64_t *wanted, const uint64_t *unwanted,
                           uint8_t *out, size_t n, int device) {
  if (n == 0) return LIFEAPI_OK;
  if (!states || !wanted || !unwanted || !out || !aligned8(states))
    return fail(LIFEAPI_E_INVALID, "bad pointer to lifeapi_contains_batch%s");
  return host_batch(n, device,
                    {{states, nullptr, 512}, {nullptr, out, 1}, {wanted, nullptr, 512, true},
                     {unwanted, nullptr, 512, true}},
                    [](void *const *d, size_t m, hipStream_t s) {
                      return lifeapi_contains_batch_dev((const uint64_t *)d[0], (const uint64_t *)d[2],
                                                        (const uint64_t *)d[3], (uint8_t *)d[1], m, s);
                    });
}

int lifeapi_match_batch(const uint64_t *states, const uint64_t *wanted, const uint64_t *unwanted,
                        uint64_t *out, uint32_t *count, size_t n, int device) {
  if (n == 0) return LIFEAPI_OK;
  if (!states || !wanted || !unwanted || (!out && !count) || !aligned8(states) || (out && !aligned8(out)))
    return fail(LIFEAPI_E_INVALID, "bad pointer to lifeapi_match_batch%s");
  if (out) {
    const int rc = check_batch(states, out, n);
    if (rc != LIFEAPI_OK) return rc;
  }
  // the states' staging slot doubles as the device mask buffer (in place)
  const bool mask = out != nullptr, cnt = count != nullptr;
  return host_batch(n, device,
                    {{states, out, 512}, {nullptr, count, 4}, {wanted, nullptr, 512, true},
                     {unwanted, nullptr, 512, true}},
                    [=](void *const *d, size_t m, hipStream_t s) {
                      return lifeapi_match_batch_dev((const uint64_t *)d[0], (const uint64_t *)d[2],
                                                     (const uint64_t *)d[3], mask ? (uint64_t *)d[0] : nullptr,
                                                     cnt ? (uint32_t *)d[1] : nullptr, m, s);
                    });
}

// Convolve / InteractionOffsets with `pattern` the whole-array operand; the
// states' staging slot doubles as the device output (in place)
static int pattern_batch(const uint64_t *states, const uint64_t *pattern, uint64_t *out, size_t n, int device,
                         bool interaction, const char *what) {
  if (n == 0) return LIFEAPI_OK;
  if (!pattern) return fail(LIFEAPI_E_INVALID, "null pattern pointer to %s", what);
  const int rc = check_batch(states, out, n);
  if (rc != LIFEAPI_OK) return rc;
  return host_batch(n, device, {{states, out, 512}, {pattern, nullptr, 512, true}},
                    [=](void *const *d, size_t m, hipStream_t s) {
                      return interaction
                                 ? lifeapi_interaction_offsets_batch_dev((const uint64_t *)d[0], (const uint64_t *)d[1],
                                                                         (uint64_t *)d[0], m, s)
                                 : lifeapi_convolve_batch_dev((const uint64_t *)d[0], (const uint64_t *)d[1],
                                                              (uint64_t *)d[0], m, s);
                    });
}

int lifeapi_convolve_batch(const uint64_t *states, const uint64_t *pattern, uint64_t *out, size_t n, int device) {
  return pattern_batch(states, pattern, out, n, device, false, "lifeapi_convolve_batch");
}

int lifeapi_interaction_offsets_batch(const uint64_t *states, const uint64_t *other, uint64_t *out, size_t n,
                                      int device) {
  return pattern_batch(states, other, out, n, device, true, "lifeapi_interaction_offsets_batch");
}

// the symmetry layer; Transform and Symmetricize run in place on the states'
// staging slot
int lifeapi_transform_batch(const uint64_t *in, uint64_t *out, size_t n, uint32_t transform, int dx, int dy,
                            int device) {
  const int rc = check_batch(in, out, n);
  if (rc != LIFEAPI_OK || n == 0) return rc;
  return host_batch(n, device, {{in, out, 512}}, [=](void *const *d, size_t m, hipStream_t s) {
    return lifeapi_transform_batch_dev((const uint64_t *)d[0], (uint64_t *)d[0], m, transform, dx, dy, s);
  });
}

int lifeapi_symmetricize_batch(const uint64_t *in, uint64_t *out, size_t n, uint32_t symmetry, int dx, int dy,
                               int device) {
  const int rc = check_batch(in, out, n);
  if (rc != LIFEAPI_OK || n == 0) return rc;
  return host_batch(n, device, {{in, out, 512}}, [=](void *const *d, size_t m, hipStream_t s) {
    return lifeapi_symmetricize_batch_dev((const uint64_t *)d[0], (uint64_t *)d[0], m, symmetry, dx, dy, s);
  });
}

// the same with an offset per universe, staged beside the states
static int offsets_batch(const uint64_t *in, uint64_t *out, size_t n, const int32_t *offsets, int device,
                         const char *what, const std::function<int(const uint64_t *, uint64_t *, size_t,
                                                                   const int32_t *, hipStream_t)> &dev) {
  if (n == 0) return LIFEAPI_OK;
  const int rc = check_batch(in, out, n);
  if (rc != LIFEAPI_OK) return rc;
  if (!offsets || ((uintptr_t)offsets & 3u)) return fail(LIFEAPI_E_INVALID, "null or misaligned offsets to %s", what);
  if (ranges_overlap(offsets, n * 8, out, n * 512))
    return fail(LIFEAPI_E_INVALID, "offsets overlaps the output batch of %s", what);
  return host_batch(n, device, {{in, out, 512}, {offsets, nullptr, 8}}, [=](void *const *d, size_t m, hipStream_t s) {
    return dev((const uint64_t *)d[0], (uint64_t *)d[0], m, (const int32_t *)d[1], s);
  });
}

int lifeapi_transform_offsets_batch(const uint64_t *in, uint64_t *out, size_t n, uint32_t transform,
                                    const int32_t *offsets, int device) {
  if (transform > 15) return fail(LIFEAPI_E_INVALID, "lifeapi_transform_offsets_batch: transform must be 0..15%s");
  return offsets_batch(in, out, n, offsets, device, "lifeapi_transform_offsets_batch",
                       [=](const uint64_t *di, uint64_t *dout, size_t m, const int32_t *dofs, hipStream_t s) {
                         return lifeapi_transform_offsets_batch_dev(di, dout, m, transform, dofs, s);
                       });
}

int lifeapi_symmetricize_offsets_batch(const uint64_t *in, uint64_t *out, size_t n, uint32_t symmetry,
                                       const int32_t *offsets, int device) {
  // (the symmetry is checked before n, as in the *_dev call: no device is touched)
  const int rc = lifeapi_symmetricize_offsets_batch_dev(nullptr, nullptr, 0, symmetry, nullptr, nullptr);
  if (rc != LIFEAPI_OK) return rc;
  return offsets_batch(in, out, n, offsets, device, "lifeapi_symmetricize_offsets_batch",
                       [=](const uint64_t *di, uint64_t *dout, size_t m, const int32_t *dofs, hipStream_t s) {
                         return lifeapi_symmetricize_offsets_batch_dev(di, dout, m, symmetry, dofs, s);
                       });
}

// a.Convolve(b.Transformed(t)) / IntersectingOffsets: the first operand's
// staging slot doubles as the device output; b == a is staged once
static int pair_batch(const uint64_t *a, const uint64_t *b, uint32_t code, bool intersecting, uint64_t *out, size_t n,
                      int device) {
  // (the code is checked before n, as in the *_dev calls: no device is touched)
  int rc = intersecting ? lifeapi_intersecting_offsets_batch_dev(nullptr, nullptr, code, nullptr, 0, nullptr)
                        : lifeapi_convolve_pair_batch_dev(nullptr, nullptr, code, nullptr, 0, nullptr);
  if (rc != LIFEAPI_OK || n == 0) return rc;
  rc = check_batch(a, out, n);
  if (rc == LIFEAPI_OK) rc = check_batch(b, out, n);
  if (rc == LIFEAPI_OK && a != b && ranges_overlap(a, n * 512, b, n * 512))
    rc = fail(LIFEAPI_E_INVALID, "the operands overlap (only the same batch twice is allowed)%s");
  if (rc != LIFEAPI_OK) return rc;
  const auto dev = [=](const uint64_t *da, const uint64_t *db, size_t m, hipStream_t s) {
    return intersecting ? lifeapi_intersecting_offsets_batch_dev(da, db, code, (uint64_t *)da, m, s)
                        : lifeapi_convolve_pair_batch_dev(da, db, code, (uint64_t *)da, m, s);
  };
  if (a == b)
    return host_batch(n, device, {{a, out, 512}}, [=](void *const *d, size_t m, hipStream_t s) {
      return dev((const uint64_t *)d[0], (const uint64_t *)d[0], m, s);
    });
  return host_batch(n, device, {{a, out, 512}, {b, nullptr, 512}}, [=](void *const *d, size_t m, hipStream_t s) {
    return dev((const uint64_t *)d[0], (const uint64_t *)d[1], m, s);
  });
}

int lifeapi_convolve_pair_batch(const uint64_t *a, const uint64_t *b, uint32_t transform, uint64_t *out, size_t n,
                                int device) {
  return pair_batch(a, b, transform, false, out, n, device);
}

int lifeapi_intersecting_offsets_batch(const uint64_t *pat1, const uint64_t *pat2, uint32_t symmetry, uint64_t *out,
                                       size_t n, int device) {
  return pair_batch(pat1, pat2, symmetry, true, out, n, device);
}

int lifeapi_halve_batch(const uint64_t *in, uint64_t *out, size_t n, uint32_t mode, int device) {
  if (mode > 2) return fail(LIFEAPI_E_INVALID, "lifeapi_halve_batch: mode must be 0 (Halve), 1 (HalveX) or 2 (HalveY)%s");
  const int rc = check_batch(in, out, n);
  if (rc != LIFEAPI_OK || n == 0) return rc;
  return host_batch(n, device, {{in, out, 512}}, [=](void *const *d, size_t m, hipStream_t s) {
    return lifeapi_halve_batch_dev((const uint64_t *)d[0], (uint64_t *)d[0], m, mode, s);
  });
}

int lifeapi_skew_batch(const uint64_t *in, uint64_t *out, size_t n, int inverse, int device) {
  const int rc = check_batch(in, out, n);
  if (rc != LIFEAPI_OK || n == 0) return rc;
  return host_batch(n, device, {{in, out, 512}}, [=](void *const *d, size_t m, hipStream_t s) {
    return lifeapi_skew_batch_dev((const uint64_t *)d[0], (uint64_t *)d[0], m, inverse, s);
  });
}

int lifeapi_bounds_batch(const uint64_t *states, int32_t *bounds, size_t n, int device) {
  if (n == 0) return LIFEAPI_OK;
  if (!states || !bounds || !aligned8(states)) return fail(LIFEAPI_E_INVALID, "bad pointer to lifeapi_bounds_batch%s");
  return host_batch(n, device, {{states, nullptr, 512}, {nullptr, bounds, 16}},
                    [](void *const *d, size_t m, hipStream_t s) {
                      return lifeapi_bounds_batch_dev((const uint64_t *)d[0], (int32_t *)d[1], m, s);
                    });
}

int lifeapi_symmetry_orbit_batch(const uint64_t *states, uint64_t *images, uint8_t *first, size_t n, int device) {
  if (n == 0) return LIFEAPI_OK;
  if (!states || (!images && !first) || !aligned8(states) || (images && !aligned8(images)))
    return fail(LIFEAPI_E_INVALID, "bad pointer to lifeapi_symmetry_orbit_batch%s");
  // (an output the caller leaves out keeps a one-byte slot and is not copied)
  const bool img = images != nullptr, fst = first != nullptr;
  return host_batch(n, device, {{states, nullptr, 512}, {nullptr, images, img ? size_t(8 * 512) : size_t(1)}, {nullptr, first, 1}},
                    [=](void *const *d, size_t m, hipStream_t s) {
                      return lifeapi_symmetry_orbit_batch_dev((const uint64_t *)d[0],
                                                              img ? (uint64_t *)d[1] : nullptr,
                                                              fst ? (uint8_t *)d[2] : nullptr, m, s);
                    });
}

// the connected-component family; the corona stays a host pointer all the way
// to the *_dev call, which reads it before it returns
int lifeapi_first_on_batch(const uint64_t *states, int32_t *cells, size_t n, int device) {
  if (n == 0) return LIFEAPI_OK;
  if (!states || !cells || !aligned8(states)) return fail(LIFEAPI_E_INVALID, "bad pointer to lifeapi_first_on_batch%s");
  return host_batch(n, device, {{states, nullptr, 512}, {nullptr, cells, 8}},
                    [](void *const *d, size_t m, hipStream_t s) {
                      return lifeapi_first_on_batch_dev((const uint64_t *)d[0], (int32_t *)d[1], m, s);
                    });
}

int lifeapi_component_containing_batch(const uint64_t *states, const uint64_t *seeds, int per_universe_seeds,
                                       const uint64_t *corona, uint64_t *out, size_t n, int device) {
  if (n == 0) return LIFEAPI_OK;
  int rc = check_batch(states, out, n);
  if (rc != LIFEAPI_OK) return rc;
  if (!seeds || !aligned8(seeds))
    return fail(LIFEAPI_E_INVALID, "null or misaligned seeds pointer to %s", "lifeapi_component_containing_batch");
  if (per_universe_seeds) {
    if ((rc = check_batch(seeds, out, n)) != LIFEAPI_OK) return rc;
  } else if (ranges_overlap(seeds, 512, out, n * 512)) {
    return fail(LIFEAPI_E_INVALID, "lifeapi_component_containing_batch: the seed overlaps the output batch%s");
  }
  // the states' staging slot doubles as the device output (in place)
  const bool per = per_universe_seeds != 0;
  return host_batch(n, device, {{states, out, 512}, {seeds, nullptr, 512, !per}},
                    [=](void *const *d, size_t m, hipStream_t s) {
                      return lifeapi_component_containing_batch_dev((const uint64_t *)d[0], (const uint64_t *)d[1], per,
                                                                    corona, (uint64_t *)d[0], m, s);
                    });
}

int lifeapi_components_batch(const uint64_t *states, const uint64_t *corona, uint32_t *count, uint64_t *components,
                             uint32_t max_components, size_t n, int device) {
  // the argument checks that need no device, in the *_dev call's order
  const int rc = lifeapi_components_batch_dev(nullptr, corona, nullptr, nullptr, 0, 0, nullptr);
  if (rc != LIFEAPI_OK || n == 0) return rc;
  if (!states || (!count && !components) || !aligned8(states) || (components && !aligned8(components)) ||
      (components && max_components == 0))
    return fail(LIFEAPI_E_INVALID, "bad argument to lifeapi_components_batch%s");
  // (an output the caller leaves out keeps a one-byte slot and is not copied;
  // the components go in as well as out, so that the slots past a universe's
  // count come back as the caller left them)
  const bool cnt = count != nullptr, cmp = components != nullptr;
  return host_batch(n, device,
                    {{states, nullptr, 512}, {nullptr, count, cnt ? size_t(4) : size_t(1)},
                     {components, components, cmp ? size_t(max_components) * 512 : size_t(1)}},
                    [=](void *const *d, size_t m, hipStream_t s) {
                      return lifeapi_components_batch_dev((const uint64_t *)d[0], corona, cnt ? (uint32_t *)d[1] : nullptr,
                                                          cmp ? (uint64_t *)d[2] : nullptr, max_components, m, s);
                    });
}

// the LifeWeld construction family: the argument checks that need no device
// are the *_dev call's own, made on the host pointers before anything is staged
int lifeapi_weld_from_required_batch(const uint64_t *states, const uint64_t *required, int per_universe_required,
                                     uint64_t *welds, size_t n, int device) {
  if (n == 0) return LIFEAPI_OK;
  if (!states || !required || !welds || !aligned8(states) || !aligned8(required) || !aligned8(welds))
    return fail(LIFEAPI_E_INVALID, "null or misaligned pointer to lifeapi_weld_from_required_batch%s");
  const bool per = per_universe_required != 0;
  if (ranges_overlap(welds, n * 2048, states, n * 512) || ranges_overlap(welds, n * 2048, required, per ? n * 512 : 512))
    return fail(LIFEAPI_E_INVALID, "lifeapi_weld_from_required_batch: welds overlaps an input%s");
  return host_batch(n, device, {{states, nullptr, 512}, {required, nullptr, 512, !per}, {nullptr, welds, 2048}},
                    [=](void *const *d, size_t m, hipStream_t s) {
                      return lifeapi_weld_from_required_batch_dev((const uint64_t *)d[0], (const uint64_t *)d[1], per,
                                                                  (uint64_t *)d[2], m, s);
                    });
}

int lifeapi_weld_to_target_batch(const uint64_t *welds, uint64_t *wanted, uint64_t *unwanted, size_t n, int device) {
  if (n == 0) return LIFEAPI_OK;
  if (!welds || !wanted || !unwanted || !aligned8(welds) || !aligned8(wanted) || !aligned8(unwanted))
    return fail(LIFEAPI_E_INVALID, "null or misaligned pointer to lifeapi_weld_to_target_batch%s");
  if (ranges_overlap(wanted, n * 512, welds, n * 2048) || ranges_overlap(unwanted, n * 512, welds, n * 2048) ||
      ranges_overlap(wanted, n * 512, unwanted, n * 512))
    return fail(LIFEAPI_E_INVALID, "lifeapi_weld_to_target_batch: an output overlaps the welds or the other output%s");
  return host_batch(n, device, {{welds, nullptr, 2048}, {nullptr, wanted, 512}, {nullptr, unwanted, 512}},
                    [](void *const *d, size_t m, hipStream_t s) {
                      return lifeapi_weld_to_target_batch_dev((const uint64_t *)d[0], (uint64_t *)d[1],
                                                              (uint64_t *)d[2], m, s);
                    });
}

int lifeapi_weld_to_stable_batch(const uint64_t *welds, const uint64_t *active, int per_universe_active,
                                 const uint64_t *mask, uint32_t duration, uint64_t *stables, size_t n, int device) {
  const int rc = lifeapi_weld_to_stable_batch_dev(nullptr, nullptr, 0, nullptr, duration, nullptr, 0, nullptr);
  if (rc != LIFEAPI_OK || n == 0) return rc;
  if (!welds || !stables || !aligned8(welds) || !aligned8(stables) || !aligned8(active) || !aligned8(mask))
    return fail(LIFEAPI_E_INVALID, "null or misaligned pointer to lifeapi_weld_to_stable_batch%s");
  const bool act = active != nullptr, per = act && per_universe_active != 0, msk = mask != nullptr;
  if (ranges_overlap(stables, n * 5120, welds, n * 2048) ||
      (act && ranges_overlap(stables, n * 5120, active, per ? n * 512 : 512)) ||
      (msk && ranges_overlap(stables, n * 5120, mask, 512)))
    return fail(LIFEAPI_E_INVALID, "lifeapi_weld_to_stable_batch: stables overlaps an input%s");
  // (an input the caller leaves out keeps a one-byte slot and is not copied)
  return host_batch(n, device,
                    {{welds, nullptr, 2048}, {nullptr, stables, 5120}, {active, nullptr, act ? size_t(512) : size_t(1), act && !per},
                     {mask, nullptr, msk ? size_t(512) : size_t(1), msk}},
                    [=](void *const *d, size_t m, hipStream_t s) {
                      return lifeapi_weld_to_stable_batch_dev((const uint64_t *)d[0], act ? (const uint64_t *)d[2] : nullptr,
                                                              per, msk ? (const uint64_t *)d[3] : nullptr, duration,
                                                              (uint64_t *)d[1], m, s);
                    });
}

int lifeapi_weld_interaction_offsets_batch(const uint64_t *welds, const uint64_t *other, uint64_t *out, size_t n,
                                           int device) {
  if (n == 0) return LIFEAPI_OK;
  if (!welds || !other || !out || !aligned8(welds) || !aligned8(other) || !aligned8(out))
    return fail(LIFEAPI_E_INVALID, "null or misaligned pointer to lifeapi_weld_interaction_offsets_batch%s");
  if (ranges_overlap(out, n * 512, welds, n * 2048) || ranges_overlap(out, n * 512, other, 2048))
    return fail(LIFEAPI_E_INVALID, "lifeapi_weld_interaction_offsets_batch: out overlaps an input%s");
  return host_batch(n, device, {{welds, nullptr, 2048}, {nullptr, out, 512}, {other, nullptr, 2048, true}},
                    [](void *const *d, size_t m, hipStream_t s) {
                      return lifeapi_weld_interaction_offsets_batch_dev((const uint64_t *)d[0], (const uint64_t *)d[2],
                                                                        (uint64_t *)d[1], m, s);
                    });
}

// the LifeStable lookahead family: the argument checks that need no device
namespace {
int stable_test_check(const char *fn, const uint64_t *planes, const void *side, size_t side_bytes, bool side_align8,
                      const uint8_t *flags, size_t n) {
  if (!planes || !side || !flags) return fail(LIFEAPI_E_INVALID, "null pointer to %s", fn);
  if (!aligned8(planes) || (side_align8 && !aligned8(side))) return fail(LIFEAPI_E_INVALID, "misaligned pointer to %s", fn);
  if (ranges_overlap(planes, n * 5120, side, side_bytes) || ranges_overlap(planes, n * 5120, flags, n))
    return fail(LIFEAPI_E_INVALID, "%s: an array overlaps the planes", fn);
  return LIFEAPI_OK;
}
}  // namespace

int lifeapi_stable_strip_pass_batch(uint64_t *planes, const uint8_t *columns, uint8_t *flags, size_t n, int pass,
                                    uint32_t max_iters, int device) {
  if (pass < 0 || pass > 5) return fail(LIFEAPI_E_INVALID, "lifeapi_stable_strip_pass_batch: pass outside 0..5%s");
  if (n == 0) return LIFEAPI_OK;
  const int rc = stable_test_check("lifeapi_stable_strip_pass_batch", planes, columns, n, false, flags, n);
  if (rc != LIFEAPI_OK) return rc;
  return host_batch(n, device, {{planes, planes, 5120}, {columns, nullptr, 1}, {nullptr, flags, 1}},
                    [=](void *const *d, size_t m, hipStream_t s) {
                      return lifeapi_stable_strip_pass_batch_dev((uint64_t *)d[0], (const uint8_t *)d[1],
                                                                 (uint8_t *)d[2], m, pass, max_iters, s);
                    });
}

int lifeapi_stable_test_unknowns_batch(uint64_t *planes, const uint64_t *cells, int per_object_cells, uint8_t *flags,
                                       size_t n, uint32_t max_iters, int device) {
  if (n == 0) return LIFEAPI_OK;
  const bool per = per_object_cells != 0;
  const int rc = stable_test_check("lifeapi_stable_test_unknowns_batch", planes, cells, per ? n * 512 : 512, true, flags, n);
  if (rc != LIFEAPI_OK) return rc;
  return host_batch(n, device, {{planes, planes, 5120}, {nullptr, flags, 1}, {cells, nullptr, 512, !per}},
                    [=](void *const *d, size_t m, hipStream_t s) {
                      return lifeapi_stable_test_unknowns_batch_dev((uint64_t *)d[0], (const uint64_t *)d[2], per,
                                                                    (uint8_t *)d[1], m, max_iters, s);
                    });
}

int lifeapi_stable_propagate_and_test_batch(uint64_t *planes, uint8_t *flags, size_t n, uint32_t max_iters,
                                            int device) {
  if (n == 0) return LIFEAPI_OK;
  const int rc = stable_test_check("lifeapi_stable_propagate_and_test_batch", planes, flags, n, false, flags, n);
  if (rc != LIFEAPI_OK) return rc;
  return host_batch(n, device, {{planes, planes, 5120}, {nullptr, flags, 1}},
                    [=](void *const *d, size_t m, hipStream_t s) {
                      return lifeapi_stable_propagate_and_test_batch_dev((uint64_t *)d[0], (uint8_t *)d[1], m,
                                                                         max_iters, s);
                    });
}

int lifeapi_step_contains_batch(const uint64_t *in, uint64_t *final_states, const uint64_t *wanted,
                                const uint64_t *unwanted, uint32_t *first_gen, size_t n,
                                uint32_t generations, int device) {
  if (n == 0) return LIFEAPI_OK;
  if (!in || !wanted || !unwanted || !first_gen || !aligned8(in))
    return fail(LIFEAPI_E_INVALID, "bad pointer to lifeapi_step_contains_batch%s");
  if (final_states) {
    const int rc = check_batch(in, final_states, n);
    if (rc != LIFEAPI_OK) return rc;
  }
  // the states' staging slot doubles as the device final buffer (in place)
  const bool keep = final_states != nullptr;
  return host_batch(n, device,
                    {{in, final_states, 512}, {nullptr, first_gen, 4}, {wanted, nullptr, 512, true},
                     {unwanted, nullptr, 512, true}},
                    [=](void *const *d, size_t m, hipStream_t s) {
                      return lifeapi_step_contains_batch_dev(
                          (const uint64_t *)d[0], keep ? (uint64_t *)d[0] : nullptr, (const uint64_t *)d[2],
                          (const uint64_t *)d[3], (uint32_t *)d[1], m, generations, s);
                    });
}

}  // extern "C"
