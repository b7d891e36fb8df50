// launch.hpp -- host only: the one way a *_dev entry point launches a kernel
// (launch), with the batch it writes stated for the order book (Written), the
// order-keyed store policy (launch_order), and launch as the kernels with one
// wave per group of objects take it (launch_groups).  The book is in host.hip.
#pragma once

#include <type_traits>

#include "host.hpp"

namespace lifeapi_impl {

// Launch order keyed on the batch (the order never changes a result): true
// = take the groups in reverse.  Reverse exactly when d_in is a batch of
// `bytes` that an earlier order-keyed launch on this device wrote in forward
// order (and forward when it wrote it in reverse), so that each launch starts
// on what the launch that wrote its input wrote last, which the memory-side
// Infinity Cache may still hold; any other input runs forward.  Records d_out
// as written in the order returned.  A few batches are remembered per device,
// so interleaved loops over several batches keep the alternation.
bool launch_reverse(const void *d_in, const void *d_out, uint64_t bytes);
// Records d_out (bytes) as written in forward order by a launch that does not
// alternate (so a stale entry for that range cannot reverse a later reader).
void note_forward_write(const void *d_out, uint64_t bytes);
// (Both are for the two functions below and the tuning build's order_probe /
// order_note; no entry point calls them.)

// The batch a launch writes: launch() records it as written forward, unless
// launch_order has recorded it already.
struct Written {
  const void *out = nullptr;
  uint64_t bytes = 0;
  bool recorded = false;
};
// no batch a later order-keyed launch could read: counts, hashes, hits, text
constexpr Written kWritesNoBatch{};

// The order-keyed store policy (step.hip, "Launch order and store policy") of
// a launch of `groups` groups of bytes_per_group each that reads d_in and
// writes d_out (`bytes` both).  keyed: the book decides the order and holds
// d_out as written in it; else the launch runs forward.  The groups from
// plain_from on, in the launch's order, store the last plain_bytes (rounded
// up to groups) with plain stores.
struct LaunchOrder {
  bool reverse;  // the kernel's kReverse / kWeldReverse bit
  uint64_t plain_from;
  Written written;
};
inline LaunchOrder launch_order(const void *d_in, const void *d_out, uint64_t bytes, uint64_t groups,
                                uint64_t bytes_per_group, bool keyed, uint64_t plain_bytes) {
  const uint64_t plain = (plain_bytes + bytes_per_group - 1) / bytes_per_group;
  return {keyed && launch_reverse(d_in, d_out, bytes), plain < groups ? groups - plain : 0, {d_out, bytes, keyed}};
}

struct Grid {
  uint64_t waves;               // waves (or groups) the batch needs
  int blocks_per_cu = 0;        // at most this many per CU, the waves looping over the batch; 0 = one-shot
  int resident_blocks = 0;      // at most this many resident per CU (occupancy_lds); 0 = as many as fit
  int cus = 0;                  // the device's CUs where the caller has asked already (device_cus); 0 = ask
  bool wave_per_group = false;  // the kernel loops nowhere: the grid must hold every wave
};

// Launches `kernel` (blocks of kBlock threads) on `stream` with `args`,
// converted to its parameter types; `what` names the launch in an error.
template <class... P>
int launch(void (*kernel)(P...), const char *what, Grid g, void *stream, const Written &w,
           std::common_type_t<P>... args) {
  int rc = g.cus ? LIFEAPI_OK : device_cus(g.cus);
  if (rc != LIFEAPI_OK) return rc;
  unsigned lds = 0;
  if (g.resident_blocks) rc = occupancy_lds(reinterpret_cast<const void *>(kernel), g.resident_blocks, lds);
  if (rc != LIFEAPI_OK) return rc;
  if (w.bytes && !w.recorded) note_forward_write(w.out, w.bytes);
  const unsigned grid = grid_for(g.waves, g.cus, g.blocks_per_cu);
  if (g.wave_per_group && (uint64_t)grid * kWavesPerBlock < g.waves)
    return fail(LIFEAPI_E_INVALID, "batch too large for one grid%s");
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), lds, (hipStream_t)stream, args...);
  return launched(what);
}

// The launch of the kernels with one wave per group of U objects
// (wave_groups.hpp): a wave for every group, so the kernels' loops only run
// again on a grid capped at 2^30 blocks.  d_out is the batch written, of
// bytes_per_object each, or null where the launch writes none (counts, cells,
// bounds).
template <class... P, class... A>
int launch_groups(void (*kernel)(P...), const char *what, int U, void *stream, const void *d_out,
                  uint64_t bytes_per_object, size_t n, A... args) {
  return launch(kernel, what, Grid{(n + U - 1) / U}, stream,
                d_out ? Written{d_out, (uint64_t)n * bytes_per_object} : kWritesNoBatch, args...);
}

}  // namespace lifeapi_impl
