// Library-owned device memory behind the C ABI (workspace.h): the per-device BatchNorm accumulator replicas and
// tile-claim ring, the per-(device, stream) scratch buffers and deferral arena, and the fixed-order slab reduce whose
// launches the arena defers. One mutex guards both maps; the static helpers below expect it held.
#include "workspace.h"
#include <map>
#include <mutex>
#include <vector>

namespace {

// Fixed-order sum of G partial slabs into dW (dW[i] += sum_g part[g][i]): a 256-thread block takes 32 float4
// elements; its 8 thread groups sum consecutive slab ranges [g0, g1) in order, and group 0 adds the 8 range sums in
// order. The association depends only on G, so two runs give the same bits (unlike f32 atomics).
__device__ __forceinline__ void slab_reduce_block(int G, size_t n4, const float4* __restrict__ part,
                                                  float4* __restrict__ dW, int blk, float4 (&ps)[8][32]) {
  const int e = threadIdx.x & 31, j = threadIdx.x >> 5;
  const size_t i = (size_t)blk * 32 + e;
  const int per = (G + 7) / 8, g0 = min(G, j * per), g1 = min(G, g0 + per);
  float4 acc = {0.f, 0.f, 0.f, 0.f};
  if (i < n4) {
    int g = g0;
    for (; g + 4 <= g1; g += 4) {   // four loads in flight, added in order
      const float4 v0 = part[(size_t)g * n4 + i], v1 = part[(size_t)(g + 1) * n4 + i];
      const float4 v2 = part[(size_t)(g + 2) * n4 + i], v3 = part[(size_t)(g + 3) * n4 + i];
      acc.x += v0.x; acc.y += v0.y; acc.z += v0.z; acc.w += v0.w;
      acc.x += v1.x; acc.y += v1.y; acc.z += v1.z; acc.w += v1.w;
      acc.x += v2.x; acc.y += v2.y; acc.z += v2.z; acc.w += v2.w;
      acc.x += v3.x; acc.y += v3.y; acc.z += v3.z; acc.w += v3.w;
    }
    for (; g < g1; ++g) {
      const float4 v = part[(size_t)g * n4 + i];
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
  }
  ps[j][e] = acc;
  __syncthreads();
  if (j == 0 && i < n4) {
    float4 s = ps[0][e];
#pragma unroll
    for (int q = 1; q < 8; ++q) {
      const float4 v = ps[q][e];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    float4 d = dW[i];
    d.x += s.x; d.y += s.y; d.z += s.z; d.w += s.w;
    dW[i] = d;
  }
}
__global__ __launch_bounds__(256) void wgrad_slab_reduce_kernel(int G, size_t n4, const float4* __restrict__ part,
                                                                float4* __restrict__ dW) {
  __shared__ float4 ps[8][32];
  slab_reduce_block(G, n4, part, dW, blockIdx.x, ps);
}
// the deferred reductions of a backward in one launch (adp_wgrad_defer / adp_wgrad_flush): segment j takes blocks
// [blk0[j], blk0[j + 1]), each block the same arithmetic as wgrad_slab_reduce_kernel (bit-identical sums)
constexpr int SEG_MAX = 32;
struct SegTable {
  int n;
  int blk0[SEG_MAX + 1];
  int G[SEG_MAX];
  unsigned long long n4[SEG_MAX];
  const float4* part[SEG_MAX];
  float4* dst[SEG_MAX];
};
__global__ __launch_bounds__(256) void wgrad_slab_reduce_batched_kernel(SegTable t) {
  __shared__ float4 ps[8][32];
  const int b = blockIdx.x;
  int j = 0;
  while (j + 1 < t.n && b >= t.blk0[j + 1]) ++j;
  slab_reduce_block(t.G[j], (size_t)t.n4[j], t.part[j], t.dst[j], b - t.blk0[j], ps);
}

// a conv launch with bn_defer_fold leaves its BatchNorm sums in the replicas; until the matching
// adp_bn_finalize_fold (same channel count, sum vector and stream) runs, no other launch may use them
struct PendingFold { bool on = false; int C = 0; const float* sum = nullptr; hipStream_t s = nullptr; };
struct DeviceState {
  double* stat = nullptr;    // BatchNorm accumulator replicas
  PendingFold fold;
  int* claim = nullptr;      // tile-claim ring
  unsigned claim_next = 0;
};
// ---- deferred slab reductions (adp_wgrad_defer / adp_wgrad_flush). Every deterministic weight / bias gradient launch
// is followed by a small reduce launch (~10 us) and, like every launch, a ~5.8 us dependency gap: 21 per training
// step, ~0.34 ms (profiles/r05a: tools/kstats.py, gap analysis in DESIGN.md §3 (30)). Deferred, the slabs go to the
// stream's arena (chunks kept across steps) and the reductions are recorded; adp_wgrad_flush launches them all as one
// kernel (up to SEG_MAX segments per launch), in the same fixed order: bit-identical gradients.
struct StreamState {
  std::pair<void*, size_t> scratch[(int)adp::Slot::Count] = {};   // (base, bytes)
  bool defer = false;
  std::vector<std::pair<char*, size_t>> chunks;   // arena: (base, bytes), reused across steps
  size_t ci = 0, used = 0;                          // current chunk, bytes used in it
  size_t pending = 0;                               // slab bytes recorded since the last launch of the tables
  std::vector<SegTable> tables;                     // (built as the segments are recorded)
};
// a stream's state lives on the device whose launches write it, and the default stream is handle 0 on every device
using StreamKey = std::pair<int, hipStream_t>;
std::mutex g_mu;
std::map<int, DeviceState> g_dev;
std::map<StreamKey, StreamState> g_stream;

StreamKey stream_key(hipStream_t s) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  return {dev, s};
}
void launch_tables(std::vector<SegTable>& tables, hipStream_t s) {
  for (const SegTable& t : tables)
    if (t.n > 0) hipLaunchKernelGGL(wgrad_slab_reduce_batched_kernel, dim3((unsigned)t.blk0[t.n]), dim3(256), 0, s, t);
  tables.clear();
}
double* stat_locked(DeviceState& d) {
  if (d.stat) return d.stat;
  const size_t bytes = sizeof(double) * adp::STAT_REPL * 2 * adp::STAT_CMAX;
  if (hipMalloc(&d.stat, bytes) != hipSuccess || hipMemset(d.stat, 0, bytes) != hipSuccess ||
      hipDeviceSynchronize() != hipSuccess) {
    d.stat = nullptr;
    adp::set_error("stat_scratch: allocation of the BatchNorm accumulator replicas failed");
  }
  return d.stat;
}
double* stat_take(bool fold, int C, const float* sum, hipStream_t s) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { adp::set_error("stat_scratch: hipGetDevice failed"); return nullptr; }
  std::lock_guard<std::mutex> lk(g_mu);
  DeviceState& d = g_dev[dev];
  PendingFold& pf = d.fold;
  if (fold) {
    if (!pf.on || pf.C != C || pf.sum != sum || pf.s != s) {
      adp::set_error(pf.on ? "adp_bn_finalize_fold: does not match the pending deferred fold (channel count, sum "
                             "vector or stream differ)"
                           : "adp_bn_finalize_fold: no conv launch with bn_defer_fold is pending");
      return nullptr;
    }
    pf.on = false;
  } else if (pf.on) {
    adp::set_error("BatchNorm accumulator replicas hold the sums of a bn_defer_fold launch: adp_bn_finalize_fold "
                   "must run first");
    return nullptr;
  }
  return stat_locked(d);
}
void* scratch_locked(StreamState& st, adp::Slot slot, size_t bytes) {
  auto& e = st.scratch[(int)slot];
  if (e.second >= bytes) return e.first;
  if (e.first) {   // kernels queued on any stream may still use the old buffer
    if (hipDeviceSynchronize() != hipSuccess || hipFree(e.first) != hipSuccess) {
      adp::set_error("scratch: releasing the old buffer failed");
      return nullptr;
    }
    e = {nullptr, 0};
  }
  const size_t want = bytes + bytes / 4;   // grow with headroom
  if (hipMalloc(&e.first, want) != hipSuccess) {
    e = {nullptr, 0};
    adp::set_error("scratch: hipMalloc failed");
    return nullptr;
  }
  e.second = want;
  return e.first;
}

}  // namespace

namespace adp {
int defer_fold_begin(int C, const float* sum, hipStream_t s) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { set_error("defer_fold: hipGetDevice failed"); return -2; }
  std::lock_guard<std::mutex> lk(g_mu);
  g_dev[dev].fold = PendingFold{true, C, sum, s};
  return 0;
}
double* stat_scratch() { return stat_take(false, 0, nullptr, nullptr); }
double* stat_scratch_fold(int C, const float* sum, hipStream_t s) { return stat_take(true, C, sum, s); }
// drop a deferred fold that never reached its adp_bn_finalize_fold (an error or exception between the two) and
// re-zero the replicas it left its sums in, stream-ordered on s; a no-op when nothing is pending -- and when the
// pending fold was left on another stream: that one belongs to another caller (engine handle, thread) whose launch
// may still be in flight, and a memset on s would neither be ordered after it nor be ours to make
int bn_fold_reset(hipStream_t s) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { set_error("adp_bn_fold_reset: hipGetDevice failed"); return -2; }
  std::lock_guard<std::mutex> lk(g_mu);
  DeviceState& d = g_dev[dev];
  if (!d.fold.on || d.fold.s != s) return 0;
  d.fold.on = false;
  double* p = stat_locked(d);
  if (!p) return -2;
  if (hipMemsetAsync(p, 0, sizeof(double) * STAT_REPL * 2 * STAT_CMAX, s) != hipSuccess) {
    set_error("adp_bn_fold_reset: clearing the accumulator replicas failed");
    return -2;
  }
  return 0;
}
int* claim_slot() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { set_error("claim_slot: hipGetDevice failed"); return nullptr; }
  std::lock_guard<std::mutex> lk(g_mu);
  DeviceState& d = g_dev[dev];
  if (!d.claim) {
    const size_t bytes = sizeof(int) * CLAIM_SLOTS * CLAIM_INTS;
    if (hipMalloc(&d.claim, bytes) != hipSuccess || hipMemset(d.claim, 0, bytes) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {
      d.claim = nullptr;
      set_error("claim_slot: allocation of the tile-claiming counters failed");
      return nullptr;
    }
  }
  return d.claim + (size_t)(d.claim_next++ % CLAIM_SLOTS) * CLAIM_INTS;
}
void* scratch(Slot slot, size_t bytes, hipStream_t s) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { set_error("scratch: hipGetDevice failed"); return nullptr; }
  std::lock_guard<std::mutex> lk(g_mu);
  return scratch_locked(g_stream[{dev, s}], slot, bytes);
}
Slabs reduce_part(Slot slot, size_t bytes, hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_mu);
  StreamState& d = g_stream[stream_key(s)];
  if (!d.defer) return {static_cast<float*>(scratch_locked(d, slot, bytes)), false};
  bytes = (bytes + 255) / 256 * 256;
  // (option wgrad_defer_mb: once the recorded slabs would pass this many MB, the recorded reductions are
  //  launched first and the arena starts over: the slabs are re-read while they still sit in the MALL, and the
  //  arena's first chunk stays resident)
  const size_t lim = (size_t)std::max(0, option("wgrad_defer_mb", 64)) << 20;
  if (lim && d.pending + bytes > lim && !d.tables.empty()) {
    launch_tables(d.tables, s);
    d.ci = 0;
    d.used = 0;
    d.pending = 0;
  }
  while (d.ci < d.chunks.size() && d.used + bytes > d.chunks[d.ci].second) { ++d.ci; d.used = 0; }
  if (d.ci == d.chunks.size()) {   // (first steps only: a new chunk, kept until adp_wgrad_release)
    // (option wgrad_arena_max_kb: the most the arena may hold in total, 0 = no limit)
    const size_t cap = (size_t)std::max(0, option("wgrad_arena_max_kb", 0)) << 10;
    size_t held = 0;
    for (const auto& c : d.chunks) held += c.second;
    const size_t room = !cap ? SIZE_MAX : cap > held ? cap - held : 0;
    const size_t sz = std::max(bytes, std::min((size_t)256 << 20, room));
    void* p = nullptr;
    if (bytes > room || hipMalloc(&p, sz) != hipSuccess) {
      // no arena: this launch's slabs go to the scratch slot and its reduction runs at once (slab_reduce), still
      // in a fixed order
      if (bytes <= room) (void)hipGetLastError();   // (the failed hipMalloc's)
      return {static_cast<float*>(scratch_locked(d, slot, bytes)), false};
    }
    d.chunks.push_back({static_cast<char*>(p), sz});
    d.used = 0;
  }
  d.pending += bytes;
  float* r = reinterpret_cast<float*>(d.chunks[d.ci].first + d.used);
  d.used += bytes;
  return {r, true};
}
void slab_reduce(int G, size_t n4, Slabs part, float* dst, hipStream_t s) {
  if (!part.deferred) {
    hipLaunchKernelGGL(wgrad_slab_reduce_kernel, dim3((unsigned)((n4 + 31) / 32)), dim3(256), 0, s, G, n4,
                       reinterpret_cast<const float4*>(part.p), reinterpret_cast<float4*>(dst));
    return;
  }
  std::lock_guard<std::mutex> lk(g_mu);
  StreamState& d = g_stream[stream_key(s)];
  // segments of one launch run concurrently: a destination already in the open table (the same gradient
  // accumulated twice) starts a new table, launched after it
  bool clash = false;
  if (!d.tables.empty()) {
    const SegTable& o = d.tables.back();
    const float4* lo = reinterpret_cast<const float4*>(dst);
    for (int j = 0; j < o.n && !clash; ++j) clash = lo < o.dst[j] + o.n4[j] && o.dst[j] < lo + n4;
  }
  if (d.tables.empty() || d.tables.back().n == SEG_MAX || clash) {
    d.tables.emplace_back();
    d.tables.back().n = 0;
    d.tables.back().blk0[0] = 0;
  }
  SegTable& t = d.tables.back();
  const int j = t.n++;
  t.G[j] = G;
  t.n4[j] = n4;
  t.part[j] = reinterpret_cast<const float4*>(part.p);
  t.dst[j] = reinterpret_cast<float4*>(dst);
  t.blk0[j + 1] = t.blk0[j] + (int)((n4 + 31) / 32);
}
int wgrad_defer(hipStream_t s, int on) {
  std::lock_guard<std::mutex> lk(g_mu);
  StreamState& d = g_stream[stream_key(s)];
  if (!on && !d.tables.empty()) { set_error("adp_wgrad_defer: reductions pending (adp_wgrad_flush first)"); return -1; }
  d.defer = on != 0 && option("wgrad_defer", 1);   // (option wgrad_defer = 0: every reduction launched at once)
  return 0;
}
// launch the pending reductions of stream s (stream-ordered after the launches that wrote their slabs) and end the
// deferral; the arena is reused by the next deferred launches, which are ordered after these reductions
int wgrad_flush(hipStream_t s) {
  std::vector<SegTable> tables;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_stream.find(stream_key(s));
    if (it == g_stream.end()) return 0;
    StreamState& d = it->second;
    tables.swap(d.tables);
    d.defer = false;
    d.ci = 0;
    d.used = 0;
    d.pending = 0;
  }
  launch_tables(tables, s);
  return 0;
}
// free everything (current device, stream s) holds -- arena chunks and scratch buffers -- and forget the stream: a
// workspace per stream that is never freed leaks with every destroyed stream, and a reused handle would inherit it.
// Synchronises s first; an error with reductions pending (flush first).
int wgrad_release(hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_stream.find(stream_key(s));
  if (it == g_stream.end()) return 0;
  StreamState& d = it->second;
  if (!d.tables.empty()) { set_error("adp_wgrad_release: reductions pending (adp_wgrad_flush first)"); return -1; }
  bool holds = !d.chunks.empty();
  for (const auto& e : d.scratch) holds = holds || e.first;
  if (holds && hipStreamSynchronize(s) != hipSuccess) {
    set_error("adp_wgrad_release: stream synchronisation failed");
    return -1;
  }
  for (auto& c : d.chunks) (void)hipFree(c.first);
  for (auto& e : d.scratch) (void)hipFree(e.first);
  g_stream.erase(it);
  return 0;
}
// (test hook) the number of arena chunks of (current device, stream s)
int wgrad_arena_chunks(hipStream_t s) {
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_stream.find(stream_key(s));
  return it == g_stream.end() ? 0 : (int)it->second.chunks.size();
}
}  // namespace adp
