// Connected-component labelling of binary maps on the GPU, with component areas, small-object removal and a table of
// per-component statistics: the reference's remove_small_components (Segmentation/build_dataset.py:1122-1131,
// build_test_dataset.py:374: cv2.connectedComponentsWithStats(connectivity=8), keep area >= min_px) and the labelling
// behind analyze_cell_characteristics (pre-post-processing_tools/analysis/morphology parameter_analysis/
// analyze_training_data.py:76-130).
//
// Labels are canonical: background 0, foreground 1 + the raster index (y*W + x, within the pixel's own image) of the
// first pixel of its component. `labels` doubles as the union-find forest: parent(i) = labels[i] - 1.
//
// INVARIANT: parent(i) <= i at every moment, in LDS and in global memory. Every value ever written to labels[i] is
// 1 + the index of a pixel of i's own component that is <= i, and it only ever decreases (every write of the merge
// stage is an atomicMin). So every find / union chain strictly decreases and every loop below terminates whatever any
// other thread or block is doing; no block waits for another block's progress (no flags, no spinning). A stale read
// of a parent yields an older, larger ancestor: still a member of the component and still < i.
//
// adp_cc_label, three launches (each kernel boundary makes the previous stage's plain stores visible across XCDs):
//   1. cc_local_kernel    one block per region of R x C = 32 x 64 pixels of one image. A wave takes a row: the ballot of
//                         the foreground gives every pixel the start of its row run as parent (in LDS); then unions
//                         between adjacent rows, one per pair of touching runs (LDS atomicMin); then every pixel finds
//                         its local root and stores 1 + the root's global index. Local raster order agrees with global
//                         raster order inside a region, so the local minimum is the global minimum of the local piece.
//   2. cc_merge_kernel    one thread per pixel of the first row of a region (against the row above) and of the first
//                         column of a region (against the column to the left), corners included. Reads are agent-scope
//                         relaxed atomic loads, writes agent-scope atomicMin. union(a, b): find both roots (halving the
//                         path on the way), atomicMin(&labels[hi], lo + 1), and the result is confirmed from the value
//                         the atomicMin returns: if hi was no longer a root, the loop goes on with (lo, old parent of hi).
//   3. cc_jump_kernel     every foreground pixel sets parent(i) = parent(parent(i)) until its parent is a root, and
//                         publishes each step (a relaxed agent-scope store of its own word, which no other thread
//                         writes in this launch). All pixels jump at once, so chains halve together: O(log depth)
//                         rounds where the others have kept up, and never more than the chain's length. Most
//                         pixels point at their former local root, which points at the root: two loads and a store.
//                         A classification "former local root or not" would save the others' store, but after stage 2
//                         a former local root may point into its own region (two arms joined elsewhere), so it
//                         cannot be told from the pixel's position; all pixels take the same path instead.
//
// adp_cc_areas / adp_cc_table: sums per component, integers, hence exact in any order. Atomics serialise per address at
// the memory side (workspace.h: ~17 ns each), and an all-foreground map is one component, so sums are pre-aggregated on
// chip. One block takes a tile of AR x AC = 64 x 256 pixels. A wave reads 64 consecutive pixels of a row; a run of equal
// labels within the wave is summed in closed form by its first lane (length from the ballot of label changes). The
// run's sums go into an LDS hash table of HT = 1024 labels (LDS atomics); after a barrier each occupied entry issues
// its global atomics once. A run that finds no slot within PROBES probes goes to memory directly: that needs more than
// HT / 2 or so distinct labels in one tile, so those components are small ones.
// Worst-case atomics per address (area of one component) = tiles of the image that the component touches, when the
// table does not overflow:
//   all-foreground 1024^2:  (1024 / 64) * (1024 / 256)  =   64 adds to area[0]   (~1 us at 17 ns)
//   all-foreground 8192^2:  (8192 / 64) * (8192 / 256)  = 4096 adds to area[0]   (~70 us)
// against 2^20 and 2^26 unaggregated. Neither depends on the length of a run: a longer run is a longer closed form.
// With overflow the bound is the number of wave runs of the label in the tile (at most 64 * 128).
// adp_cc_table ranks the roots (labels[i] == i + 1) with an exclusive scan (hipcub) and accumulates straight into the
// caller's rows {first, area, x_min, y_min, x_max, y_max, sum_x, sum_y}; a root's rank is its row.
//
// adp_cc_shape: the integer sums behind perimeter, axes and eccentricity, rows {first, S_xx, S_yy, S_xy, p_straight,
// p_diag, p_mixed, border_px} in the table's order (the same scan). One launch of cc_shape_kernel, one block per tile
// of ST_R x ST_C = 64 x 128 pixels:
//   1. the tile's labels with a two-pixel halo go to LDS (0 outside the image): a pixel's perimeter code depends on the
//      border flags of its eight neighbours, and each flag on that neighbour's four edge neighbours.
//   2. every pixel of the tile and of the first halo ring whose label differs from one of its edge neighbours' gets
//      the border flag, kept in bit 31 of its LDS word (labels are at most 2^31 - 1). The comparisons mask that bit, so
//      the pass needs no second buffer and no barrier of its own.
//   3. a wave takes 64 consecutive pixels of a row from LDS. A border pixel counts the neighbours whose word equals its
//      own (same label and flagged): code = 1 + 2 * n4 + 10 * nd, classified by three bit masks. Runs of equal labels
//      are aggregated by their first lane as in cc_accum_kernel: moments in closed form, relative to the tile, and the
//      four perimeter counts as popcount(ballot(class) & run mask). The sums go into an LDS hash table of SHT = 512
//      labels; after a barrier every occupied entry translates its moments to image coordinates in 64 bit and issues
//      its global atomics once (zero counts are skipped). A run without a slot after PROBES probes goes to memory.
//      The root pixel of a component stores `first`.
// LDS: labels (64 + 4) * (128 + 4) * 4 = 35904 B, keys 2048 B, values 512 * 10 * 4 = 20480 B: 58432 B, two blocks
// of 512 threads (16 waves) per CU of 160 KiB; a thread's 18 staging loads are issued together. The 64 x 256 tile of
// the areas would need 70720 B for the labels alone.
// Worst-case atomics per address (S_xx of one component) = tiles the component touches:
//   all-foreground 1024^2:  (1024 / 64) * (1024 / 128)  =   128 adds   (~2 us at 17 ns)
//   all-foreground 8192^2:  (8192 / 64) * (8192 / 128)  =  8192 adds   (~140 us)
// twice the areas' count, the price of the smaller tile.
#include <hipcub/hipcub.hpp>

#include <climits>

#include "common.h"
#include "workspace.h"
#include "../../include/adipose_hip.h"

namespace {

constexpr int TPB = 256, WAVES = TPB / 64;
constexpr int R = ADP_CC_REGION_ROWS, C = ADP_CC_REGION_COLS;   // region of the local labelling; C = one wave
static_assert(C == 64 && R % WAVES == 0, "a wave takes a row of a region");
constexpr int AR = 64, AC = 256;           // tile of the sums
constexpr int HT_BITS = 10, HT = 1 << HT_BITS, PROBES = 16;
constexpr int SEGS = AR * (AC / 64);       // wave segments of a tile
typedef unsigned long long u64;

#define RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
#define RLX_WG __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP

// Which of the three neighbours in the previous line (l, c, r = at offsets -1, 0, +1) the pixel unites with, given its
// own line's neighbours cl / cr: one union per pair of touching runs. With c present the pair was already united by the
// pixel before if that one is foreground and touches too; l and r matter only at connectivity 8 and only when c is
// absent (otherwise they belong to c's run), and not when the own neighbour below them is foreground (it has them as c).
struct Contact { bool c, l, r; };
ADP_DEV Contact contact(bool cl, bool cr, bool ul, bool uc, bool ur, bool conn8) {
  Contact k;
  k.c = uc && !(cl && ul);
  k.l = conn8 && !uc && ul && !cl;
  k.r = conn8 && !uc && ur && !cr;
  return k;
}

// ---------------------------------------------------------------- stage 1: a region in LDS
ADP_DEV int lds_find(int* P, int i) {
  int p;
  while ((p = __hip_atomic_load(&P[i], RLX_WG)) != i) i = p;
  return i;
}
ADP_DEV void lds_union(int* P, int a, int b) {
  while (true) {
    a = lds_find(P, a);
    b = lds_find(P, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(&P[b], a, RLX_WG);
    if (old == b) return;   // b was a root: linked
    b = old;                // b had a parent already: go on with (a, that parent)
  }
}

template <bool F32>
__global__ __launch_bounds__(TPB) void cc_local_kernel(int H, int W, int nbr, int nbc, const void* src, float thr,
                                                       int conn8, int* labels) {
  __shared__ int P[R * C];
  __shared__ u64 M[R];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int per = nbr * nbc;
  const int n = blockIdx.x / per, rem = blockIdx.x - n * per;
  const int y0 = (rem / nbc) * R, x0 = (rem % nbc) * C;
  const size_t img = (size_t)n * H * W;
  const int x = x0 + lane;
#pragma unroll
  for (int i = 0; i < R / WAVES; ++i) {
    const int r = wave + i * WAVES, y = y0 + r;
    bool fg = false;
    if (x < W && y < H) {
      const size_t g = img + (size_t)y * W + x;
      fg = F32 ? static_cast<const float*>(src)[g] > thr : static_cast<const uint8_t*>(src)[g] != 0;
    }
    const u64 m = __ballot(fg);
    const u64 below = ~m & ((1ull << lane) - 1);          // background pixels left of this one
    const int start = below ? 64 - __clzll((long long)below) : 0;
    P[r * C + lane] = fg ? r * C + start : -1;
    if (lane == 0) M[r] = m;
  }
  __syncthreads();
  for (int i = 0; i < R / WAVES; ++i) {
    const int r = wave + i * WAVES;
    if (r == 0) continue;
    const u64 cur = M[r], up = M[r - 1];
    if (!((cur >> lane) & 1)) continue;
    auto bit = [lane](u64 m, int d) { const int b = lane + d; return b >= 0 && b < 64 && ((m >> b) & 1); };
    const Contact k = contact(bit(cur, -1), bit(cur, 1), bit(up, -1), bit(up, 0), bit(up, 1), conn8 != 0);
    const int me = r * C + lane, ab = (r - 1) * C + lane;
    if (k.c) lds_union(P, me, ab);
    if (k.l) lds_union(P, me, ab - 1);
    if (k.r) lds_union(P, me, ab + 1);
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < R / WAVES; ++i) {
    const int r = wave + i * WAVES, y = y0 + r;
    if (x < W && y < H) {
      const int p = P[r * C + lane];
      int out = 0;
      if (p >= 0) {
        const int root = lds_find(P, p);
        out = (y0 + root / C) * W + x0 + root % C + 1;
      }
      labels[img + (size_t)y * W + x] = out;
    }
  }
}

// ---------------------------------------------------------------- stage 2: region borders in global memory
ADP_DEV int g_load(int* L, int i) { return __hip_atomic_load(&L[i], RLX_AGENT); }

// root of i (0-based index; L[i] != 0), halving the path: parent(i) = parent(parent(i)) by atomicMin
ADP_DEV int g_find(int* L, int i) {
  while (true) {
    const int p = g_load(L, i) - 1;
    if (p == i) return i;
    const int gp = g_load(L, p) - 1;
    if (gp == p) return p;
    __hip_atomic_fetch_min(&L[i], gp + 1, RLX_AGENT);
    i = gp;
  }
}
ADP_DEV void g_union(int* L, int a, int b) {
  while (true) {
    a = g_find(L, a);
    b = g_find(L, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(&L[b], a + 1, RLX_AGENT);
    if (old == b + 1) return;   // confirmed by the returned value: b was a root and now points at a
    b = old - 1;                // b had the parent old - 1 < b (kept, or replaced by a): unite a with it
  }
}

// items of one image: nhb * W pixels of the rows y = R, 2R, ... then nvb * H pixels of the columns x = C, 2C, ...
__global__ __launch_bounds__(TPB) void cc_merge_kernel(int H, int W, int nhb, int nvb, long long per, long long total,
                                                       int conn8, int* labels) {
  const long long gid = (long long)blockIdx.x * TPB + threadIdx.x;
  if (gid >= total) return;
  const long long n = gid / per;
  long long it = gid - n * per;
  int* L = labels + (size_t)n * H * W;
  const long long nh = (long long)nhb * W;
  int me, prev_base, step;   // the pixel, its centre neighbour in the previous line, index step along the line
  bool has_l, has_r;         // neighbours at -1 / +1 along the line exist
  bool in_l, in_r;           // ... and lie in the pixel's own region: only then stage 1 has united them with it
  if (it < nh) {
    const int b = (int)(it / W), x = (int)(it - (long long)b * W), y = (b + 1) * R;   // y <= (nbr - 1) * R < H
    me = y * W + x; prev_base = me - W; step = 1;
    has_l = x > 0; has_r = x + 1 < W;
    in_l = x % C != 0; in_r = has_r && (x + 1) % C != 0;
  } else {
    it -= nh;
    const int b = (int)(it / H), y = (int)(it - (long long)b * H), x = (b + 1) * C;   // x <= (nbc - 1) * C < W
    me = y * W + x; prev_base = me - 1; step = W;
    has_l = y > 0; has_r = y + 1 < H;
    in_l = y % R != 0; in_r = has_r && (y + 1) % R != 0;
  }
  if (g_load(L, me) == 0) return;
  // cl / cr only spare unions that a neighbour makes, given that it is already united with this pixel: across a
  // region border that would rest on the other pass sparing nothing there, and at a corner with all four pixels set
  // each pass would leave the union to the other
  const bool cl = in_l && g_load(L, me - step) != 0, cr = in_r && g_load(L, me + step) != 0;
  const bool ul = has_l && g_load(L, prev_base - step) != 0, uc = g_load(L, prev_base) != 0;
  const bool ur = has_r && g_load(L, prev_base + step) != 0;
  const Contact k = contact(cl, cr, ul, uc, ur, conn8 != 0);
  if (k.c) g_union(L, me, prev_base);
  if (k.l) g_union(L, me, prev_base - step);
  if (k.r) g_union(L, me, prev_base + step);
}

// ---------------------------------------------------------------- stage 3
__global__ __launch_bounds__(TPB) void cc_jump_kernel(size_t hw, size_t total, int* labels) {
  for (size_t g = (size_t)blockIdx.x * TPB + threadIdx.x; g < total; g += (size_t)gridDim.x * TPB) {
    const int v = labels[g];   // its own word: only this thread writes it in this launch
    if (v == 0) continue;
    int* L = labels + (g / hw) * hw;
    const int i = (int)(g % hw);
    int p = v - 1;
    while (true) {
      const int gp = g_load(L, p) - 1;
      if (gp == p) break;                                // the parent is a root: done
      __hip_atomic_store(&L[i], gp + 1, RLX_AGENT);      // seen by the pixels that pass through i
      p = gp;
    }
  }
}

// ---------------------------------------------------------------- sums per component
// NV ints per LDS entry: {area} or {area, x_min, y_min, x_max, y_max, sum (x - x0), sum (y - y0)}
template <bool TABLE>
struct Emit {
  int* area;             // areas: this image's plane
  const int* rank;       // table: this image's ranks; rank[0] is the image's base
  int max_rows;
  long long* rows;       // table: this image's rows
  ADP_DEV void operator()(int lab, int a, int xmin, int ymin, int xmax, int ymax, long long sx, long long sy) const {
    if (!TABLE) {
      atomicAdd(&area[lab - 1], a);
    } else {
      const int k = rank[lab - 1] - rank[0];
      if (k >= max_rows) return;
      u64* row = reinterpret_cast<u64*>(rows + (size_t)k * 8);
      atomicAdd(&row[1], (u64)a);
      atomicMin(&row[2], (u64)xmin);
      atomicMin(&row[3], (u64)ymin);
      atomicMax(&row[4], (u64)xmax);
      atomicMax(&row[5], (u64)ymax);
      atomicAdd(&row[6], (u64)sx);
      atomicAdd(&row[7], (u64)sy);
    }
  }
};

template <bool TABLE>
__global__ __launch_bounds__(TPB) void cc_accum_kernel(int H, int W, int ntr, int ntc, const int* __restrict__ labels,
                                                       int* area, const int* __restrict__ rank, int max_rows,
                                                       long long* table) {
  constexpr int NV = TABLE ? 7 : 1;
  __shared__ int keys[HT];
  __shared__ int vals[HT * NV];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int per = ntr * ntc;
  const int n = blockIdx.x / per, rem = blockIdx.x - n * per;
  const int y0 = (rem / ntc) * AR, x0 = (rem % ntc) * AC;
  const size_t hw = (size_t)H * W;
  const int* L = labels + n * hw;
  Emit<TABLE> emit{TABLE ? nullptr : area + n * hw, TABLE ? rank + n * hw : nullptr, max_rows,
                   TABLE ? table + (size_t)n * max_rows * 8 : nullptr};
  for (int e = threadIdx.x; e < HT; e += TPB) {
    keys[e] = 0;
    vals[e * NV] = 0;
    if (TABLE) {
      vals[e * NV + 1] = INT_MAX; vals[e * NV + 2] = INT_MAX;
      vals[e * NV + 3] = -1; vals[e * NV + 4] = -1;
      vals[e * NV + 5] = 0; vals[e * NV + 6] = 0;
    }
  }
  __syncthreads();

  for (int s0 = wave; s0 < SEGS; s0 += WAVES * 4) {
    int lab[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {   // four rows' requests in flight
      const int s = s0 + u * WAVES, y = y0 + s / (AC / 64), x = x0 + (s % (AC / 64)) * 64 + lane;
      lab[u] = (y < H && x < W) ? L[(size_t)y * W + x] : 0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int s = s0 + u * WAVES, y = y0 + s / (AC / 64), x = x0 + (s % (AC / 64)) * 64 + lane;
      const int v = lab[u];
      if (__ballot(v != 0) == 0) continue;
      const int prev = __shfl_up(v, 1, 64);
      const bool change = lane == 0 || prev != v;
      const u64 cb = __ballot(change);
      if (!change || v == 0) continue;
      const u64 nx = lane == 63 ? 0ull : cb >> (lane + 1);
      const int len = nx ? __ffsll((long long)nx) : 64 - lane;   // up to the next change or the end of the wave
      const int rx = x - x0, ry = y - y0;
      const int sx = len * rx + len * (len - 1) / 2, sy = len * ry;   // relative to the tile: at most 64 * 255 each
      uint32_t h = ((uint32_t)v * 2654435761u) >> (32 - HT_BITS);
      int slot = -1;
      for (int p = 0; p < PROBES; ++p) {
        const int old = atomicCAS(&keys[h], 0, v);
        if (old == 0 || old == v) { slot = (int)h; break; }
        h = (h + 1) & (HT - 1);
      }
      if (slot >= 0) {
        int* e = &vals[slot * NV];
        atomicAdd(&e[0], len);
        if (TABLE) {
          atomicMin(&e[1], x); atomicMin(&e[2], y);
          atomicMax(&e[3], x + len - 1); atomicMax(&e[4], y);
          atomicAdd(&e[5], sx); atomicAdd(&e[6], sy);
        }
      } else {
        emit(v, len, x, y, x + len - 1, y, (long long)sx + (long long)len * x0, (long long)sy + (long long)len * y0);
      }
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < HT; e += TPB) {
    const int v = keys[e];
    if (v == 0) continue;
    const int* q = &vals[e * NV];
    if (TABLE)
      emit(v, q[0], q[1], q[2], q[3], q[4], (long long)q[5] + (long long)q[0] * x0, (long long)q[6] + (long long)q[0] * y0);
    else
      emit(v, q[0], 0, 0, 0, 0, 0, 0);
  }
}

// ---------------------------------------------------------------- shape sums per component
constexpr int ST_R = ADP_CC_SHAPE_TILE_ROWS, ST_C = ADP_CC_SHAPE_TILE_COLS;   // tile of the shape sums
constexpr int SP = ST_C + 4, SROWS = ST_R + 4;                               // the staged labels: pitch and rows
constexpr int RING_C = ST_C + 2, RING = (ST_R + 2) * RING_C;                 // the tile and the first halo ring
constexpr int SHT_BITS = 9, SHT = 1 << SHT_BITS;
constexpr int SNV = 10;   // ints per LDS entry: {area, sum rx, sum ry, sum rx^2, sum ry^2, sum rx*ry, p_straight, p_diag, p_mixed, border_px}
constexpr int SSEGS = ST_R * (ST_C / 64);
constexpr int STPB = 512, SWAVES = STPB / 64;                   // eight waves a block: two blocks a CU by LDS, 16 waves
constexpr int STAGE = (SROWS * SP + STPB - 1) / STPB;          // labels a thread stages: all its loads are in flight at once
static_assert(ST_C % 64 == 0 && SSEGS % SWAVES == 0, "a wave takes 64 consecutive pixels of a tile row");
// rx <= ST_C - 1 and ry <= ST_R - 1 are relative to the tile, so an entry's largest sum over all ST_R * ST_C pixels is
// below 64 * 128 * 127^2 = 132'128'768 < 2^31: the LDS entries are 32 bit
static_assert((long long)ST_R * ST_C * (ST_C - 1) * (ST_C - 1) < INT_MAX && (long long)ST_R * ST_C * (ST_R - 1) * (ST_R - 1) < INT_MAX,
              "tile-relative moments must fit an int");
constexpr int BORDER_BIT = INT_MIN;
constexpr u64 code_mask(std::initializer_list<int> codes) {
  u64 m = 0;
  for (int c : codes) m |= 1ull << c;
  return m;
}
constexpr u64 CODES_STRAIGHT = code_mask({5, 7, 15, 17, 25, 27}), CODES_DIAG = code_mask({21, 33}), CODES_MIXED = code_mask({13, 23});

// q: an entry's SNV sums, relative to the tile at (x0, y0)
ADP_DEV void shape_emit(const int* rank, int max_rows, long long* rows, int lab, int x0, int y0, const int* q) {
  const int k = rank[lab - 1] - rank[0];
  if (k >= max_rows) return;
  u64* row = reinterpret_cast<u64*>(rows + (size_t)k * 8);
  const long long a = q[0], sx = q[1], sy = q[2], X = x0, Y = y0;
  // sum (X + rx)^2 = sum rx^2 + 2 X sum rx + X^2 a, and likewise: every term is at most the image's sum, which fits
  atomicAdd(&row[1], (u64)(q[3] + 2 * X * sx + X * X * a));
  atomicAdd(&row[2], (u64)(q[4] + 2 * Y * sy + Y * Y * a));
  atomicAdd(&row[3], (u64)(q[5] + X * sy + Y * sx + X * Y * a));
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (q[6 + j]) atomicAdd(&row[4 + j], (u64)q[6 + j]);
}

__global__ __launch_bounds__(STPB) void cc_shape_kernel(int H, int W, int ntr, int ntc, const int* __restrict__ labels,
                                                       const int* __restrict__ rank, int max_rows, long long* shape) {
  __shared__ int S[SROWS * SP];
  __shared__ int keys[SHT];
  __shared__ int vals[SHT * SNV];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int per = ntr * ntc;
  const int n = blockIdx.x / per, rem = blockIdx.x - n * per;
  const int y0 = (rem / ntc) * ST_R, x0 = (rem % ntc) * ST_C;
  const size_t hw = (size_t)H * W;
  const int* L = labels + n * hw;
  const int* rk = rank + n * hw;
  long long* rows = shape + (size_t)n * max_rows * 8;
  int staged[STAGE];
#pragma unroll
  for (int i = 0; i < STAGE; ++i) {
    const int e = threadIdx.x + i * STPB, y = y0 - 2 + e / SP, x = x0 - 2 + e % SP;
    // an unconditional load from the clamped position and no control flow (&, not &&): under a branch per load each
    // load waits for the one before
    const int v = L[(size_t)min(max(y, 0), H - 1) * W + min(max(x, 0), W - 1)];
    const bool inside = (e < SROWS * SP) & (y >= 0) & (y < H) & (x >= 0) & (x < W);
    staged[i] = inside ? v : 0;
  }
  for (int e = threadIdx.x; e < SHT; e += STPB) keys[e] = 0;
  for (int e = threadIdx.x; e < SHT * SNV; e += STPB) vals[e] = 0;
#pragma unroll
  for (int i = 0; i < STAGE; ++i) {
    const int e = threadIdx.x + i * STPB;
    if (e < SROWS * SP) S[e] = staged[i];
  }
  __syncthreads();

  // border flags of the tile and the first ring. Another thread may set the bit of a word while this one compares it:
  // the comparison masks the bit, so either value gives the same answer
  for (int e = threadIdx.x; e < RING; e += STPB) {
    int* c = &S[(e / RING_C + 1) * SP + e % RING_C + 1];
    const int v = __hip_atomic_load(c, RLX_WG) & INT_MAX;
    if (v == 0) continue;
    auto differs = [v](const int* p) { return (__hip_atomic_load(p, RLX_WG) & INT_MAX) != v; };
    if (differs(c - SP) || differs(c + SP) || differs(c - 1) || differs(c + 1)) __hip_atomic_store(c, v | BORDER_BIT, RLX_WG);
  }
  __syncthreads();

  for (int s = wave; s < SSEGS; s += SWAVES) {
    const int ry = s / (ST_C / 64), rx = (s % (ST_C / 64)) * 64 + lane;
    const int* c = &S[(ry + 2) * SP + rx + 2];
    const int w = c[0], v = w & INT_MAX;   // 0 outside the image
    if (__ballot(v != 0) == 0) continue;
    const bool border = w < 0;
    u64 cls = 0;
    if (border) {
      const int n4 = (c[-SP] == w) + (c[SP] == w) + (c[-1] == w) + (c[1] == w);
      const int nd = (c[-SP - 1] == w) + (c[-SP + 1] == w) + (c[SP - 1] == w) + (c[SP + 1] == w);
      cls = 1ull << (1 + 2 * n4 + 10 * nd);
    }
    const u64 bb = __ballot(border), bs = __ballot((cls & CODES_STRAIGHT) != 0), bd = __ballot((cls & CODES_DIAG) != 0),
              bm = __ballot((cls & CODES_MIXED) != 0);
    const int prev = __shfl_up(v, 1, 64);
    const bool change = lane == 0 || prev != v;
    const u64 cb = __ballot(change);
    if (v == 0) continue;
    const int idx = (y0 + ry) * W + x0 + rx;   // inside the image, as v != 0
    if (v == idx + 1) {                        // the component's first pixel: its row's constant part
      const int k = rk[idx] - rk[0];
      if (k < max_rows) rows[(size_t)k * 8] = idx;
    }
    if (!change) continue;
    const u64 nx = lane == 63 ? 0ull : cb >> (lane + 1);
    const int len = nx ? __ffsll((long long)nx) : 64 - lane;   // up to the next change or the end of the wave
    const u64 run = (len == 64 ? ~0ull : (1ull << len) - 1) << lane;
    const int t = len * (len - 1) / 2;                          // sum of 0 .. len - 1
    int q[SNV];
    q[0] = len;
    q[1] = len * rx + t;
    q[2] = len * ry;
    q[3] = len * rx * rx + 2 * rx * t + t * (2 * len - 1) / 3;   // sum of squares of 0 .. len - 1 = t (2 len - 1) / 3
    q[4] = len * ry * ry;
    q[5] = ry * q[1];
    q[6] = __popcll(bs & run);
    q[7] = __popcll(bd & run);
    q[8] = __popcll(bm & run);
    q[9] = __popcll(bb & run);
    uint32_t h = ((uint32_t)v * 2654435761u) >> (32 - SHT_BITS);
    int slot = -1;
    for (int p = 0; p < PROBES; ++p) {
      const int old = atomicCAS(&keys[h], 0, v);
      if (old == 0 || old == v) { slot = (int)h; break; }
      h = (h + 1) & (SHT - 1);
    }
    if (slot >= 0) {
      int* e = &vals[slot * SNV];
#pragma unroll
      for (int j = 0; j < SNV; ++j)
        if (q[j]) atomicAdd(&e[j], q[j]);
    } else {
      shape_emit(rk, max_rows, rows, v, x0, y0, q);
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < SHT; e += STPB) {
    const int v = keys[e];
    if (v != 0) shape_emit(rk, max_rows, rows, v, x0, y0, &vals[e * SNV]);
  }
}

__global__ __launch_bounds__(TPB) void cc_filter_kernel(size_t hw, size_t total, const int* __restrict__ labels,
                                                        const int* __restrict__ area, int min_px, uint8_t* out_u8,
                                                        float* out_f32) {
  for (size_t g = (size_t)blockIdx.x * TPB + threadIdx.x; g < total; g += (size_t)gridDim.x * TPB) {
    const int v = labels[g];
    const bool keep = v != 0 && area[(g / hw) * hw + (size_t)(v - 1)] >= min_px;
    if (out_u8) out_u8[g] = keep ? 1 : 0;
    if (out_f32) out_f32[g] = keep ? 1.f : 0.f;
  }
}

// the flag "pixel i of a run of whole images is the first pixel of its component"
struct RootFlag {
  const int* L;
  int hw;
  __host__ __device__ int operator()(int i) const { return L[i] == i % hw + 1 ? 1 : 0; }
};

// roots write their rows' constant part; the last pixel of an image writes its count. rank: exclusive scan of the flags
__global__ __launch_bounds__(TPB) void cc_table_init_kernel(int W, size_t hw, size_t total, const int* __restrict__ labels,
                                                            const int* __restrict__ rank, int max_rows, long long* table,
                                                            int* counts) {
  for (size_t g = (size_t)blockIdx.x * TPB + threadIdx.x; g < total; g += (size_t)gridDim.x * TPB) {
    const size_t n = g / hw;
    const int i = (int)(g - n * hw);
    const bool root = labels[g] == i + 1;
    const int k = rank[g] - rank[n * hw];
    if (root && k < max_rows) {
      long long* row = table + (n * (size_t)max_rows + (size_t)k) * 8;
      row[0] = i;
      row[2] = LLONG_MAX;   // x_min, y_min: lowered by the accumulation (a component has at least its first pixel)
      row[3] = LLONG_MAX;
    }
    if ((size_t)i + 1 == hw) counts[n] = k + (root ? 1 : 0);
  }
}

__global__ __launch_bounds__(TPB) void cc_relabel_kernel(size_t hw, size_t total, const int* __restrict__ labels,
                                                         const int* __restrict__ rank, int* dense) {
  for (size_t g = (size_t)blockIdx.x * TPB + threadIdx.x; g < total; g += (size_t)gridDim.x * TPB) {
    const int v = labels[g];
    const size_t base = (g / hw) * hw;
    dense[g] = v ? rank[base + (size_t)(v - 1)] - rank[base] + 1 : 0;
  }
}

int stride_grid(size_t total) { return (int)std::min<size_t>((total + TPB - 1) / TPB, 1 << 16); }

bool shape_ok(const char* who, int N, int H, int W) {
  if (N < 1 || H < 1 || W < 1) {
    adp::set_error(std::string(who) + ": N, H and W must be at least 1");
    return false;
  }
  if ((long long)H * W > 0x7FFFFFFFll - 2) {
    adp::set_error(std::string(who) + ": H * W is above 2^31 - 2 (labels are int32)");
    return false;
  }
  return true;
}

// images per launch of the scan-based calls: the scan's item count is an int
int scan_group(int N, int H, int W) { return (int)std::min<long long>(N, std::max<long long>(1, 0x7FFFFFFFll / ((long long)H * W))); }

// exclusive scan of the root flags of `g` whole images into Slot::CcScan; nullptr (error set) on failure
int* scan_roots(const char* who, int g, size_t hw, const int* labels, hipStream_t s) {
  const int num = (int)(g * hw);
  hipcub::CountingInputIterator<int> idx(0);
  hipcub::TransformInputIterator<int, RootFlag, hipcub::CountingInputIterator<int>> flags(idx, RootFlag{labels, (int)hw});
  size_t tmp_b = 0;
  if (hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_b, flags, (int*)nullptr, num, s) != hipSuccess) {
    adp::set_error(std::string(who) + ": temporary-storage query failed");
    return nullptr;
  }
  const size_t rank_b = ((size_t)num * 4 + 255) / 256 * 256;
  char* w = static_cast<char*>(adp::scratch(adp::Slot::CcScan, rank_b + tmp_b + 256, s));
  if (!w) return nullptr;
  int* rank = reinterpret_cast<int*>(w);
  if (hipcub::DeviceScan::ExclusiveSum(w + rank_b, tmp_b, flags, rank, num, s) != hipSuccess) {
    adp::set_error(std::string(who) + ": scan failed");
    return nullptr;
  }
  return rank;
}

}  // namespace

extern "C" int adp_cc_label(int N, int H, int W, const void* src, int src_dtype, float thr, int connectivity, int* labels,
                            adp_stream_t st) {
  ADP_REQUIRE(src && labels, "adp_cc_label: src and labels must be non-null");
  if (!shape_ok("adp_cc_label", N, H, W)) return -1;
  ADP_REQUIRE(connectivity == 4 || connectivity == 8, "adp_cc_label: connectivity must be 4 or 8");
  ADP_REQUIRE(src_dtype == ADP_CC_SRC_U8 || src_dtype == ADP_CC_SRC_F32, "adp_cc_label: unknown src_dtype");
  const int nbr = (H + R - 1) / R, nbc = (W + C - 1) / C;
  const long long blocks = (long long)N * nbr * nbc;
  const long long per = (long long)(nbr - 1) * W + (long long)(nbc - 1) * H;   // border items of an image
  const long long mblocks = ((long long)N * per + TPB - 1) / TPB;
  ADP_REQUIRE(blocks <= 0x7FFFFFFFll && mblocks <= 0x7FFFFFFFll, "adp_cc_label: too many blocks (N * H * W too large for one launch)");
  hipStream_t s = (hipStream_t)st;
  const int conn8 = connectivity == 8;
  const size_t total = (size_t)N * H * W;
  if (src_dtype == ADP_CC_SRC_F32)
    hipLaunchKernelGGL(cc_local_kernel<true>, dim3((unsigned)blocks), dim3(TPB), 0, s, H, W, nbr, nbc, src, thr, conn8, labels);
  else
    hipLaunchKernelGGL(cc_local_kernel<false>, dim3((unsigned)blocks), dim3(TPB), 0, s, H, W, nbr, nbc, src, thr, conn8, labels);
  if (per > 0) {
    hipLaunchKernelGGL(cc_merge_kernel, dim3((unsigned)mblocks), dim3(TPB), 0, s, H, W, nbr - 1, nbc - 1, per,
                       (long long)N * per, conn8, labels);
    hipLaunchKernelGGL(cc_jump_kernel, dim3(stride_grid(total)), dim3(TPB), 0, s, (size_t)H * W, total, labels);
  }
  return adp::check_launch("adp_cc_label");
}

extern "C" int adp_cc_areas(int N, int H, int W, const int* labels, int* area, adp_stream_t st) {
  ADP_REQUIRE(labels && area, "adp_cc_areas: labels and area must be non-null");
  if (!shape_ok("adp_cc_areas", N, H, W)) return -1;
  const int ntr = (H + AR - 1) / AR, ntc = (W + AC - 1) / AC;
  const long long blocks = (long long)N * ntr * ntc;
  ADP_REQUIRE(blocks <= 0x7FFFFFFFll, "adp_cc_areas: too many blocks (N * H * W too large for one launch)");
  hipStream_t s = (hipStream_t)st;
  ADP_REQUIRE(hipMemsetAsync(area, 0, (size_t)N * H * W * sizeof(int), s) == hipSuccess, "adp_cc_areas: memset failed");
  hipLaunchKernelGGL(cc_accum_kernel<false>, dim3((unsigned)blocks), dim3(TPB), 0, s, H, W, ntr, ntc, labels, area,
                     (const int*)nullptr, 0, (long long*)nullptr);
  return adp::check_launch("adp_cc_areas");
}

extern "C" int adp_cc_filter(int N, int H, int W, const int* labels, const int* area, int min_px, uint8_t* out_u8,
                             float* out_f32, adp_stream_t st) {
  ADP_REQUIRE(labels && area, "adp_cc_filter: labels and area must be non-null");
  ADP_REQUIRE(out_u8 || out_f32, "adp_cc_filter: out_u8 and out_f32 are both NULL");
  if (!shape_ok("adp_cc_filter", N, H, W)) return -1;
  const size_t total = (size_t)N * H * W;
  hipLaunchKernelGGL(cc_filter_kernel, dim3(stride_grid(total)), dim3(TPB), 0, (hipStream_t)st, (size_t)H * W, total,
                     labels, area, min_px, out_u8, out_f32);
  return adp::check_launch("adp_cc_filter");
}

extern "C" int adp_cc_table(int N, int H, int W, const int* labels, int max_rows, long long* table, int* counts,
                            adp_stream_t st) {
  ADP_REQUIRE(labels && counts, "adp_cc_table: labels and counts must be non-null");
  ADP_REQUIRE(max_rows >= 0 && (table || max_rows == 0), "adp_cc_table: max_rows rows need a table");
  if (!shape_ok("adp_cc_table", N, H, W)) return -1;
  const int ntr = (H + AR - 1) / AR, ntc = (W + AC - 1) / AC;
  const int G = scan_group(N, H, W);
  ADP_REQUIRE((long long)G * ntr * ntc <= 0x7FFFFFFFll, "adp_cc_table: too many blocks (H * W too large for one launch)");
  hipStream_t s = (hipStream_t)st;
  const size_t hw = (size_t)H * W;
  if (max_rows > 0)
    ADP_REQUIRE(hipMemsetAsync(table, 0, (size_t)N * max_rows * 8 * sizeof(long long), s) == hipSuccess,
                "adp_cc_table: memset failed");
  for (int n0 = 0; n0 < N; n0 += G) {
    const int g = std::min(G, N - n0);
    const int* lab = labels + (size_t)n0 * hw;
    long long* tab = max_rows > 0 ? table + (size_t)n0 * max_rows * 8 : nullptr;
    const int* rank = scan_roots("adp_cc_table", g, hw, lab, s);
    if (!rank) return -2;
    hipLaunchKernelGGL(cc_table_init_kernel, dim3(stride_grid(g * hw)), dim3(TPB), 0, s, W, hw, g * hw, lab, rank, max_rows,
                       tab, counts + n0);
    if (max_rows > 0)
      hipLaunchKernelGGL(cc_accum_kernel<true>, dim3((unsigned)(g * ntr * ntc)), dim3(TPB), 0, s, H, W, ntr, ntc, lab,
                         (int*)nullptr, rank, max_rows, tab);
  }
  return adp::check_launch("adp_cc_table");
}

extern "C" int adp_cc_shape(int N, int H, int W, const int* labels, int max_rows, long long* shape, adp_stream_t st) {
  ADP_REQUIRE(labels, "adp_cc_shape: labels must be non-null");
  ADP_REQUIRE(max_rows >= 0 && (shape || max_rows == 0), "adp_cc_shape: max_rows rows need a shape table");
  if (!shape_ok("adp_cc_shape", N, H, W)) return -1;
  // sum x^2 <= H * W * (W - 1)^2 and the like must fit int64; (max - 1)^2 < 2^62 as max < 2^31
  const long long last = (long long)std::max(H, W) - 1, last2 = last * last;
  ADP_REQUIRE(last2 == 0 || (long long)H * W <= LLONG_MAX / last2,
              "adp_cc_shape: H * W * (max(H, W) - 1)^2 is 2^63 or more (the moment sums are int64)");
  if (max_rows == 0) return 0;
  const int ntr = (H + ST_R - 1) / ST_R, ntc = (W + ST_C - 1) / ST_C;
  const int G = scan_group(N, H, W);
  ADP_REQUIRE((long long)G * ntr * ntc <= 0x7FFFFFFFll, "adp_cc_shape: too many blocks (H * W too large for one launch)");
  hipStream_t s = (hipStream_t)st;
  const size_t hw = (size_t)H * W;
  ADP_REQUIRE(hipMemsetAsync(shape, 0, (size_t)N * max_rows * 8 * sizeof(long long), s) == hipSuccess,
              "adp_cc_shape: memset failed");
  for (int n0 = 0; n0 < N; n0 += G) {
    const int g = std::min(G, N - n0);
    const int* lab = labels + (size_t)n0 * hw;
    const int* rank = scan_roots("adp_cc_shape", g, hw, lab, s);
    if (!rank) return -2;
    hipLaunchKernelGGL(cc_shape_kernel, dim3((unsigned)(g * ntr * ntc)), dim3(STPB), 0, s, H, W, ntr, ntc, lab, rank, max_rows,
                       shape + (size_t)n0 * max_rows * 8);
  }
  return adp::check_launch("adp_cc_shape");
}

extern "C" int adp_cc_relabel(int N, int H, int W, const int* labels, int* dense, adp_stream_t st) {
  ADP_REQUIRE(labels && dense, "adp_cc_relabel: labels and dense must be non-null");
  if (!shape_ok("adp_cc_relabel", N, H, W)) return -1;
  hipStream_t s = (hipStream_t)st;
  const size_t hw = (size_t)H * W;
  const int G = scan_group(N, H, W);
  for (int n0 = 0; n0 < N; n0 += G) {
    const int g = std::min(G, N - n0);
    const int* rank = scan_roots("adp_cc_relabel", g, hw, labels + (size_t)n0 * hw, s);
    if (!rank) return -2;
    hipLaunchKernelGGL(cc_relabel_kernel, dim3(stride_grid(g * hw)), dim3(TPB), 0, s, hw, g * hw, labels + (size_t)n0 * hw,
                       rank, dense + (size_t)n0 * hw);
  }
  return adp::check_launch("adp_cc_relabel");
}
