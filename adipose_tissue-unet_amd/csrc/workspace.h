// Library-owned device memory (workspace.hip): everything the library allocates behind its C ABI, in two maps under one
// mutex. Per device: the BatchNorm accumulator replicas with their pending-fold record, and the tile-claim ring. Per
// (device, stream): the growable scratch buffers, and the arena and record of the deferred slab reductions. Only the
// first use of a (device, stream) and the growth of its scratch or arena allocate; adp_wgrad_release frees a stream's.
#pragma once
#include "common.h"

namespace adp {
// Replicated per-channel accumulators for the BatchNorm sums (statistics of a conv output, or the
// BN-backward dbeta/dgamma reductions). Atomics execute at the memory side and serialise per
// address, so thousands of blocks adding into the same C values queue behind each other (measured:
// ~17 ns per add per address, 1.75 ms per training step); blocks add into replica (block & 63)
// instead and stat_fold() sums the replicas into the caller's accumulators and re-zeroes them.
// The replicas are f64: each producer adds f32 partials summed in a fixed order, and f64 sums
// of them in the atomics' run-dependent order round to the same f32 (deterministic BatchNorm statistics).
// Per device, lazily allocated and zeroed; launches that use it must be ordered on one stream.
constexpr int STAT_REPL = 64, STAT_CMAX = 2048;
double* stat_scratch();   // [STAT_REPL][2][STAT_CMAX] f64, or nullptr (error set) if allocation failed or a
                         // deferred fold is pending
// bn_defer_fold bookkeeping: a launch that leaves its sums in the replicas records (C, sum, stream); only the
// adp_bn_finalize_fold with the same three may take the replicas next (stat_scratch_fold clears the record)
int defer_fold_begin(int C, const float* sum, hipStream_t s);
double* stat_scratch_fold(int C, const float* sum, hipStream_t s);
int bn_fold_reset(hipStream_t s);   // adp_bn_fold_reset
// dynamic tile claiming: a zeroed slot of CLAIM_INTS counters for one persistent launch (a ring of CLAIM_SLOTS per
// device, handed out in turn; a launch leaves its slot zeroed again), or nullptr (error set)
constexpr int CLAIM_SLOTS = 64, CLAIM_INTS = 512;
int* claim_slot();

// growable scratch of (current device, stream s), one buffer per user; launches that use a buffer are ordered on s.
// Grows with 25 % headroom; growing synchronises the device. nullptr (error set) if the allocation failed.
enum class Slot {
  WgradPart,     // weight-gradient split partials / slabs reduced at once
  UnfusedDz,     // dz of the unfused BatchNorm-backward weight gradient
  BiasRows,      // bias-gradient block rows reduced at once
  KsplitPart,    // split-K partial tiles of the tap64 forward
  AucSort,       // adp_auc_metrics: keys, values and the sort's temporary
  DistField,     // adp_distance_transform: the two passes' fields
  BoundaryDist,  // adp_boundary_metrics: the four distance fields
  BoundarySort,  // adp_boundary_metrics: surface distances and the sort's temporary
  StainPart,     // adp_stain_lab_stats: one row of six f64 sums per block
  TileQcPart,    // adp_tile_qc: one row of three int64 sums per block
  CcScan,        // adp_cc_table / adp_cc_relabel: the ranks of the roots and the scan's temporary
  ResampleTables,   // adp_resample_u8 / adp_resample_nearest_u8: the axes' bounds and taps, or index tables
  Count
};
void* scratch(Slot slot, size_t bytes, hipStream_t s);

// The slabs of one deterministic reduction. While s defers (adp_wgrad_defer) they come from the stream's arena and
// `deferred` is set; otherwise, or when the arena may not grow (allocation failure, option wgrad_arena_max_kb), from
// scratch `slot`. p is nullptr (error set) if that allocation failed too.
struct Slabs {
  float* p = nullptr;
  bool deferred = false;
};
Slabs reduce_part(Slot slot, size_t bytes, hipStream_t s);
// dst[i] += sum_g part.p[g][i] over G slabs of n4 float4 each, in an order fixed by G alone (deterministic): arena slabs
// are recorded and launched batched by adp_wgrad_flush, scratch slabs are reduced at once
void slab_reduce(int G, size_t n4, Slabs part, float* dst, hipStream_t s);
// deferred slab reductions of a stream (adp_wgrad_defer / adp_wgrad_flush / adp_wgrad_release)
int wgrad_defer(hipStream_t s, int on);
int wgrad_flush(hipStream_t s);
int wgrad_release(hipStream_t s);   // frees the whole workspace of (current device, s): arena and scratch
int wgrad_arena_chunks(hipStream_t s);
}  // namespace adp
