// stable_complete.hip -- the LifeStable::CompleteStable entry points
// (LifeStable.hpp:1340-1458 over a batch, stable_complete_kernels.hpp), device
// and host forms.  Every argument is checked before a device is touched.
#include <map>
#include <mutex>

#include "launch.hpp"
#include "stable_complete_kernels.hpp"

using namespace lifeapi_impl;

namespace {

// A full grid: this many blocks per CU (what the kernel's 156 VGPRs leave resident),
// each wave with a stack of its own.  The
// waves claim their objects, so a smaller grid (a smaller workspace) only
// lowers the number of concurrent searches.
constexpr int kCompleteBlocksPerCu = 3;
constexpr uint64_t kMaxBudget = 1ull << 24, kDefaultBudget = 1ull << 16;
constexpr uint32_t kMaxDepth = 4096;
// what the host form allocates per stream at most
constexpr size_t kHostWorkspaceCap = (size_t)1 << 30;

size_t stack_bytes(uint32_t max_depth) { return (size_t)max_depth * kCompleteFrameBytes; }

struct Args {
  const uint64_t *planes, *seeds;
  int per_object_seeds;
  uint32_t flags;
  uint64_t node_budget;
  uint32_t max_depth;
  uint64_t *best;
  uint8_t *result;
  uint64_t *nodes;
  size_t n;
};

// the checks the device and the host form share (n > 0)
int check_args(const char *fn, const Args &a) {
  const std::string f(fn);
  auto bad = [&](const char *what) { return fail(LIFEAPI_E_INVALID, (f + ": " + what + "%s").c_str()); };
  if (a.n > SIZE_MAX / kStableBytes) return bad("n too large");
  if (a.flags & ~(kCompleteFlagMinimise | kCompleteFlagUseSeed)) return bad("unknown flag bits");
  if (a.max_depth == 0 || a.max_depth > kMaxDepth) return bad("max_depth outside 1..4096");
  if (a.node_budget > kMaxBudget) return bad("node_budget above 1 << 24");
  const bool seeded = (a.flags & kCompleteFlagUseSeed) != 0u;
  if (!a.planes || !a.best || !a.result || (seeded && !a.seeds)) return bad("null pointer");
  if (!aligned8(a.planes) || !aligned8(a.best) || (seeded && !aligned8(a.seeds)) || (a.nodes && !aligned8(a.nodes)))
    return bad("misaligned pointer");
  struct Range {
    const void *p;
    size_t bytes;
  };
  const Range in[2] = {{a.planes, a.n * kStableBytes}, {a.seeds, seeded ? (a.per_object_seeds ? a.n * kStateBytes : kStateBytes) : 0}};
  const Range out[3] = {{a.best, a.n * kStateBytes}, {a.result, a.n}, {a.nodes, a.nodes ? a.n * 8 : 0}};
  for (const Range &o : out)
    for (const Range &i : in)
      if (o.bytes && i.bytes && ranges_overlap(o.p, o.bytes, i.p, i.bytes)) return bad("an output overlaps an input");
  for (int i = 0; i < 3; ++i)
    for (int j = i + 1; j < 3; ++j)
      if (out[i].bytes && out[j].bytes && ranges_overlap(out[i].p, out[i].bytes, out[j].p, out[j].bytes))
        return bad("outputs overlap");
  return LIFEAPI_OK;
}

// the host form's workspaces, one per staging stream, kept for the process
std::mutex g_ws_mu;
std::map<hipStream_t, std::pair<void *, size_t>> g_ws;

int host_workspace(hipStream_t s, size_t want, void *&ws, size_t &bytes) {
  std::lock_guard<std::mutex> lock(g_ws_mu);
  auto &slot = g_ws[s];
  if (slot.second < want) {
    // (stream order: the launches that used the old one were issued on s)
    hipError_t e = hipStreamSynchronize(s);
    if (e == hipSuccess && slot.first) e = hipFree(slot.first);
    slot = {nullptr, 0};
    if (e == hipSuccess) e = hipMalloc(&slot.first, want);
    if (e != hipSuccess) return fail_hip(e, "the CompleteStable workspace");
    slot.second = want;
  }
  ws = slot.first;
  bytes = slot.second;
  return LIFEAPI_OK;
}

}  // namespace

extern "C" {

size_t lifeapi_stable_complete_workspace_bytes(size_t n, uint32_t max_depth) {
  if (max_depth == 0 || max_depth > kMaxDepth) {
    fail(LIFEAPI_E_INVALID, "lifeapi_stable_complete_workspace_bytes: max_depth outside 1..4096%s");
    return 0;
  }
  if (n == 0) return kCompleteHeaderBytes + stack_bytes(max_depth);
  int cus = 0;
  if (device_cus(cus) != LIFEAPI_OK) return 0;
  const uint64_t waves = std::min<uint64_t>(n, (uint64_t)grid_for(n, cus, kCompleteBlocksPerCu) * kWavesPerBlock);
  return kCompleteHeaderBytes + (size_t)waves * stack_bytes(max_depth);
}

int lifeapi_stable_complete_batch_dev(const uint64_t *d_planes, const uint64_t *d_seeds, int per_object_seeds,
                                      uint32_t flags, uint64_t node_budget, uint32_t max_depth, uint64_t *d_best,
                                      uint8_t *d_result, uint64_t *d_nodes, size_t n, void *d_workspace,
                                      size_t workspace_bytes, void *stream) {
  static const char fn[] = "lifeapi_stable_complete_batch_dev";
  if (n == 0) return LIFEAPI_OK;
  const Args a{d_planes, d_seeds, per_object_seeds, flags, node_budget, max_depth, d_best, d_result, d_nodes, n};
  int rc = check_args(fn, a);
  if (rc != LIFEAPI_OK) return rc;
  if (!d_workspace) return fail(LIFEAPI_E_INVALID, "%s: null d_workspace", fn);
  if ((uintptr_t)d_workspace & 127u) return fail(LIFEAPI_E_INVALID, "%s: d_workspace not 128-byte aligned", fn);
  if (workspace_bytes < kCompleteHeaderBytes + stack_bytes(max_depth))
    return fail(LIFEAPI_E_INVALID, "%s: workspace below one wave's stack", fn);
  const bool seeded = (flags & kCompleteFlagUseSeed) != 0u;
  const std::pair<const void *, size_t> arrays[5] = {{d_planes, n * kStableBytes},
                                                    {d_seeds, seeded ? (per_object_seeds ? n * kStateBytes : kStateBytes) : 0},
                                                    {d_best, n * kStateBytes},
                                                    {d_result, n},
                                                    {d_nodes, d_nodes ? n * 8 : 0}};
  for (const auto &r : arrays)
    if (r.second && ranges_overlap(d_workspace, workspace_bytes, r.first, r.second))
      return fail(LIFEAPI_E_INVALID, "%s: the workspace overlaps an array", fn);
  int cus = 0;
  rc = device_cus(cus);
  if (rc != LIFEAPI_OK) return rc;
  const uint64_t fit = (workspace_bytes - kCompleteHeaderBytes) / stack_bytes(max_depth);
  const uint64_t waves =
      std::min<uint64_t>({(uint64_t)n, fit, (uint64_t)grid_for(n, cus, kCompleteBlocksPerCu) * kWavesPerBlock});
  const hipError_t e = hipMemsetAsync(d_workspace, 0, kCompleteHeaderBytes, (hipStream_t)stream);
  if (e != hipSuccess) return fail_hip(e, "lifeapi_stable_complete_batch_dev: clearing the claim counter");
  Grid g{waves};
  g.cus = cus;
  return launch(k_stable_complete, "k_stable_complete launch", g, stream, Written{d_best, (uint64_t)n * kStateBytes},
                d_planes, seeded ? d_seeds : nullptr, per_object_seeds ? 1u : 0u, flags,
                (uint32_t)(node_budget ? node_budget : kDefaultBudget), max_depth, d_best, d_result, d_nodes,
                (unsigned long long *)d_workspace, (char *)d_workspace + kCompleteHeaderBytes, waves, (uint64_t)n);
}

int lifeapi_stable_complete_batch(const uint64_t *planes, const uint64_t *seeds, int per_object_seeds, uint32_t flags,
                                  uint64_t node_budget, uint32_t max_depth, uint64_t *best, uint8_t *result,
                                  uint64_t *nodes, size_t n, int device) {
  if (n == 0) return LIFEAPI_OK;
  const Args a{planes, seeds, per_object_seeds, flags, node_budget, max_depth, best, result, nodes, n};
  const int rc = check_args("lifeapi_stable_complete_batch", a);
  if (rc != LIFEAPI_OK) return rc;
  const bool seeded = (flags & kCompleteFlagUseSeed) != 0u, per = per_object_seeds != 0, counted = nodes != nullptr;
  // (without USE_SEED one empty universe is staged in the seed's place, so that the arrays keep theirs)
  static const uint64_t kNoSeed[64] = {};
  const ChunkFn fn = [=](void *const *d, size_t m, hipStream_t s) {
    size_t want = lifeapi_stable_complete_workspace_bytes(m, max_depth);
    if (want == 0) return (int)LIFEAPI_E_NODEVICE;  // (device_cus has said why)
    want = std::max(std::min(want, kHostWorkspaceCap), kCompleteHeaderBytes + stack_bytes(max_depth));
    void *ws = nullptr;
    size_t bytes = 0;
    const int r = host_workspace(s, want, ws, bytes);
    if (r != LIFEAPI_OK) return r;
    return lifeapi_stable_complete_batch_dev((const uint64_t *)d[0], (const uint64_t *)d[3], per, flags, node_budget,
                                             max_depth, (uint64_t *)d[1], (uint8_t *)d[2],
                                             counted ? (uint64_t *)d[4] : nullptr, m, ws, bytes, s);
  };
  const HostIO in{planes, nullptr, kStableBytes}, b{nullptr, best, kStateBytes}, r{nullptr, result, 1},
      sd{seeded ? seeds : kNoSeed, nullptr, kStateBytes, !(seeded && per)};
  if (counted) return host_batch(n, device, {in, b, r, sd, {nullptr, nodes, 8}}, fn);
  return host_batch(n, device, {in, b, r, sd}, fn);
}

}  // extern "C"
