// Per-tile fat counts for the tile-level "Has Fat / No Fat" evaluation (Segmentation/tile_classification_evaluation.py:
// calculate_fat_percentage :211-226 of the prediction and of the ground truth after its "smart normalisation" :478-489).
// N probability maps (float32) and their N ground-truth masks (uint8) become N x 4 integers; the definition is in
// tile_classification.py's docstring and its numpy path fat_counts_ref.
//
// The ground truth's float arithmetic never reaches the device: g.astype(float32) > thr and g.astype(float32) / 255 > thr
// are monotone in the byte g, so the host hands over the two smallest bytes that pass (cut_raw, cut_scaled; 256 when none
// does) and the kernel compares integers. Which of the two counts holds is decided by the image's maximum (column 1),
// which is only known at the end, so both are counted.
//
// counts_kernel: grid (blocks per image, N), 1024 threads; a block counts ADP_FAT_BLOCK_PX pixels of one image in both
// planes. Image i starts at element i * n_px, so with an odd n_px the float plane and the byte plane leave 16-byte
// alignment at different images: each plane's range is split on its own into a scalar head (up to the first aligned
// address), 16-byte loads (4 floats / 16 bytes a lane) and a scalar tail. A thread issues a whole round of its loads (8
// of the float plane, 2 of the byte plane) before it counts any. Counters are per lane (at most ADP_FAT_BLOCK_PX, 32
// bits), reduced by __shfl_down across the 64 lanes of a wave, across the block's sixteen waves through LDS, and thread
// 0 issues at most three 64-bit atomicAdd and one atomicMax. Integer sums and a maximum: the result does not depend on
// the grid, the order of arrival or the run.
//
// The block is as large as a block can be because the atomics are what the kernel waits for: an image's four counters
// share one 32-byte row, every block of the image adds into it, and adds into one row are taken one after the other.
// With 8192 pixels and 256 threads a block (128 blocks and up to 512 atomics per 1024^2 image) eight tiles took 32.3 us
// whether a thread had one load in flight or eight; with 32768 pixels and 1024 threads (32 blocks, 128 atomics, the same
// loads in flight per CU) they take 17.6 us, and the maps alone, one atomic a block, run at the copy rate (DESIGN.md §3
// (64)). A block skips the atomicMax when the maximum it reads is already as large as its own.
#include "common.h"
#include "../../include/adipose_hip.h"

namespace {

constexpr int TPB = 1024, WAVES = TPB / 64;
constexpr int BPX = ADP_FAT_BLOCK_PX;
// 16-byte loads a thread issues before it counts any of them: a full block's share of either plane in one round
constexpr int UF = BPX / 4 / TPB, UB = BPX / 16 / TPB;
static_assert(BPX % (TPB * 16) == 0 && UF >= 1 && UF <= 8 && UB >= 1, "whole rounds; the float round fits the registers");
static_assert(TPB <= 1024 && WAVES <= 64, "one block; its waves' partial counts are summed by one thread");

struct Lane { uint32_t pred, mx, raw, scaled; };

ADP_DEV void count_f(Lane& c, float v, float thr) { c.pred += v > thr ? 1u : 0u; }   // IEEE: false with a NaN on either side
ADP_DEV void count_b(Lane& c, uint32_t g, uint32_t cut_raw, uint32_t cut_scaled) {
  c.mx = max(c.mx, g);
  c.raw += g >= cut_raw ? 1u : 0u;
  c.scaled += g >= cut_scaled ? 1u : 0u;
}

// elements of `len` before the first 16-byte aligned address from p on (ESZ bytes each); everything if p is not even
// aligned to its element
template <int ESZ>
ADP_DEV uint32_t head_of(const void* p, uint32_t len) {
  const uintptr_t a = (uintptr_t)p;
  if (a % ESZ) return len;
  const uint32_t h = (uint32_t)((16 - (a & 15)) & 15) / ESZ;
  return min(h, len);
}

__global__ __launch_bounds__(TPB) void counts_kernel(size_t n_px, const float* __restrict__ pred, float thr,
                                                     const uint8_t* __restrict__ gt, uint32_t cut_raw, uint32_t cut_scaled,
                                                     unsigned long long* __restrict__ out) {
  __shared__ uint32_t part[WAVES][4];
  const int img = blockIdx.y, tid = threadIdx.x;
  const size_t start = (size_t)blockIdx.x * BPX;   // (the grid covers n_px: start < n_px)
  const uint32_t len = (uint32_t)min((size_t)BPX, n_px - start);
  Lane c = {0u, 0u, 0u, 0u};
  if (pred) {
    const float* p = pred + (size_t)img * n_px + start;
    const uint32_t head = head_of<4>(p, len), nvec = (len - head) / 4, tail0 = head + nvec * 4;
    for (uint32_t k = tid; k < head; k += TPB) count_f(c, p[k], thr);   // fewer than 4 elements, if p is aligned at all
    const float4* q = reinterpret_cast<const float4*>(p + head);
    for (uint32_t k0 = tid; k0 - tid < nvec; k0 += UF * TPB) {   // UF loads in flight; one past the end re-reads the last
      float4 v[UF];
#pragma unroll
      for (int j = 0; j < UF; ++j) v[j] = q[min(k0 + j * TPB, nvec - 1)];
#pragma unroll
      for (int j = 0; j < UF; ++j)
        if (k0 + j * TPB < nvec) {
          count_f(c, v[j].x, thr); count_f(c, v[j].y, thr); count_f(c, v[j].z, thr); count_f(c, v[j].w, thr);
        }
    }
    if (tail0 + tid < len) count_f(c, p[tail0 + tid], thr);   // fewer than 4 elements
  }
  if (gt) {
    const uint8_t* p = gt + (size_t)img * n_px + start;
    const uint32_t head = head_of<1>(p, len), nvec = (len - head) / 16, tail0 = head + nvec * 16;
    if ((uint32_t)tid < head) count_b(c, p[tid], cut_raw, cut_scaled);   // fewer than 16 elements
    const uint4* q = reinterpret_cast<const uint4*>(p + head);
    for (uint32_t k0 = tid; k0 - tid < nvec; k0 += UB * TPB) {
      uint4 v[UB];
#pragma unroll
      for (int j = 0; j < UB; ++j) v[j] = q[min(k0 + j * TPB, nvec - 1)];
#pragma unroll
      for (int j = 0; j < UB; ++j)
        if (k0 + j * TPB < nvec) {
          const uint32_t w[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
          for (int d = 0; d < 4; ++d)
#pragma unroll
            for (int e = 0; e < 4; ++e) count_b(c, (w[d] >> (8 * e)) & 255u, cut_raw, cut_scaled);
        }
    }
    if (tail0 + tid < len) count_b(c, p[tail0 + tid], cut_raw, cut_scaled);   // fewer than 16 elements
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    c.pred += __shfl_down(c.pred, o, 64);
    c.mx = max(c.mx, __shfl_down(c.mx, o, 64));
    c.raw += __shfl_down(c.raw, o, 64);
    c.scaled += __shfl_down(c.scaled, o, 64);
  }
  if ((tid & 63) == 0) {
    uint32_t* w = part[tid >> 6];
    w[0] = c.pred; w[1] = c.mx; w[2] = c.raw; w[3] = c.scaled;
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t s0 = 0, mx = 0, s2 = 0, s3 = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      s0 += part[w][0]; mx = max(mx, part[w][1]); s2 += part[w][2]; s3 += part[w][3];
    }
    unsigned long long* o = out + 4 * (size_t)img;   // zeroed by the call: a zero adds nothing
    if (s0) atomicAdd(o + 0, (unsigned long long)s0);
    // (the maximum only grows: a block that reads one as large as its own has nothing to add; a stale read costs an atomic)
    if (mx > __hip_atomic_load(o + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(o + 1, (unsigned long long)mx);
    if (s2) atomicAdd(o + 2, (unsigned long long)s2);
    if (s3) atomicAdd(o + 3, (unsigned long long)s3);
  }
}

}  // namespace

extern "C" int adp_fat_counts(int N, size_t n_px, const float* pred, float pred_thr, const uint8_t* gt, int cut_raw,
                              int cut_scaled, unsigned long long* out, adp_stream_t st) {
  ADP_REQUIRE(N >= 0 && N <= 65535, "adp_fat_counts: N must be in 0 .. 65535");
  ADP_REQUIRE(n_px >= 1 && n_px <= ((size_t)1 << 36), "adp_fat_counts: n_px must be in 1 .. 2^36");
  ADP_REQUIRE(pred || gt, "adp_fat_counts: pred and gt must not both be null");
  ADP_REQUIRE(out, "adp_fat_counts: out must be non-null");
  ADP_REQUIRE(cut_raw >= 0 && cut_raw <= 256 && cut_scaled >= 0 && cut_scaled <= 256,
              "adp_fat_counts: cut_raw and cut_scaled must be in 0 .. 256");
  if (N == 0) return 0;
  hipStream_t s = (hipStream_t)st;
  if (hipMemsetAsync(out, 0, (size_t)N * 4 * sizeof(unsigned long long), s) != hipSuccess) {
    (void)hipGetLastError();
    adp::set_error("adp_fat_counts: zeroing out failed");
    return -1;
  }
  const dim3 grid((unsigned)((n_px + BPX - 1) / BPX), (unsigned)N), block(TPB);
  hipLaunchKernelGGL(counts_kernel, grid, block, 0, s, n_px, pred, pred_thr, gt, (uint32_t)cut_raw, (uint32_t)cut_scaled, out);
  return adp::check_launch("adp_fat_counts");
}
