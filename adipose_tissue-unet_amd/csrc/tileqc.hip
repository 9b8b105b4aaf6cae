// Tile quality control sums of packed uint8 RGB tiles on the GPU: the measurements behind the reference's
// classify_tiles_batch (Segmentation/build_dataset.py:1253-1284, build_test_dataset.py:634-660), which sorts a tile into
// empty (white_ratio > 0.70), blurry (variance of the Laplacian < 7.5) or tissue. Per tile the call returns four
// integers {white, S1, S2, H*W}; the ratios and the variance are formed from them on the host (quality.py measures()).
//
// All arithmetic is on integers:
//   white  pixels with R, G and B all >= white_threshold (compared as ints: any threshold is valid)
//   gray   (R*9798 + G*19235 + B*3735 + 16384) >> 15: OpenCV 4's 8-bit COLOR_BGR2GRAY, restated (cv2 is not installed
//          here: "parity unpinned" in the tests). Deliberately not the PIL mode-L formula of stain.hip's gray plane:
//          the reference calls cv2 for this measurement.
//   lap    g(y-1,x) + g(y+1,x) + g(y,x-1) + g(y,x+1) - 4 g(y,x) with reflect-101 borders within the tile (index -1 -> 1,
//          H -> H-2): cv2.Laplacian(gray, CV_64F) with its default ksize=1 and border. A window of a larger image
//          reflects at its own edge and never reads its neighbours in the image.
//   S1 = sum lap, S2 = sum lap^2. |lap| <= 1020, so lap^2 <= 1 040 400 and a 32-bit sum holds 4128 worst-case pixels.
//
// One block takes a region of up to BR rows x BC columns of one tile. Wave w converts rows w, w + 4, ... of the region
// and of its one-row halo to gray, 4 pixels = 12 bytes per lane, packs the four grays into one dword in LDS and counts
// the white pixels of the region's own rows. The two halo columns of every row go into a 65th dword. After one barrier
// each lane forms the Laplacian of its 4 pixels from five LDS dwords. No gray plane goes to HBM. A thread sums at most
// BR / 4 * 4 = 32 pixels, so its S2 fits 32 bits; from the wave reduction on, every sum is 64-bit.
// Loads: a row's alignment is its own (origins and 3*W are often no multiples of 4), so a lane loads the three or four
// aligned dwords that hold its 12 bytes and shifts the bytes into place (no shift and three dwords where the row
// starts on a dword). Only dwords that hold at least one byte of the lane's pixels are loaded, so a load never leaves
// the 4-byte word (let alone the page) of a byte the caller passed; the up to 3 foreign bytes at either end are shifted
// out or never used. All of a wave's rows (at most 9) and the halo pixels are requested before the first is converted,
// so a wave has its whole share of the region in flight at once instead of one row.
//
// The sums: every block writes its three 64-bit partial sums to its own row of the stream's workspace
// (Slot::TileQcPart) and a finaliser, one block per tile, adds the tile's rows: the pattern of the stain statistics.
// Integer sums are exact whatever the order, so 64-bit atomics into a zeroed `sums` would give the same bits, and that
// was the first form of this kernel: one add per block per sum. But atomics serialise per address at the memory side,
// and a tile has three addresses whatever its size: 128 blocks per address at 1024^2, 8192 at 8192^2, where the queue
// of adds nearly doubled the pass (2 x 8192^2: 228 us with atomics, 127 us with rows, measured on an MI355X; 841
// windows of 1024^2 with their 2523 addresses ran at the same rate either way). The rows cost a second small launch in
// place of the memset and have no such cliff.
#include "common.h"
#include "workspace.h"
#include "../../include/adipose_hip.h"

namespace {

constexpr int TPB = 256, WAVES = TPB / 64;
constexpr int BR = 32;              // rows of a region
constexpr int BC = 256;             // columns of a region: one wave instruction covers a row (64 lanes x 4 pixels)
constexpr int RS = BC / 4 + 1;      // dwords of an LDS row: 64 of packed grays, then {left halo, right halo, -, -}
constexpr int RPW = (BR + 2 + WAVES - 1) / WAVES;   // rows of a region and its halo per wave
struct u32x3 { uint32_t a, b, c; };

ADP_DEV uint32_t gray_of(uint32_t r, uint32_t g, uint32_t b) { return (r * 9798u + g * 19235u + b * 3735u + 16384u) >> 15; }
ADP_DEV int reflect101(int i, int n) { return i < 0 ? -i : i >= n ? 2 * n - 2 - i : i; }

// the aligned dwords that hold bytes p[0 .. nbytes) (nbytes <= 12); those that hold none of them are not loaded (0)
struct Raw { uint32_t d[4]; };
ADP_DEV Raw load12(const uint8_t* p, int nbytes) {
  const int sh = (int)(reinterpret_cast<uintptr_t>(p) & 3);
  const uint32_t* q = reinterpret_cast<const uint32_t*>(p - sh);
  Raw r;
#pragma unroll
  for (int k = 0; k < 4; ++k) r.d[k] = (nbytes > 0 && 4 * k < sh + nbytes) ? q[k] : 0u;   // nbytes = 12: k < 3 || sh > 0
  return r;
}
// p[0 .. 12) of load12(p, .) as three dwords; sh = p & 3. Bytes past nbytes are unspecified
ADP_DEV u32x3 align12(const Raw& r, int sh) {
  // v_alignbyte_b32: ({hi, lo} >> 8 * sh) & 0xFFFFFFFF on two separate registers (a 64-bit shift would want the loaded
  // dwords in register pairs, and the copy into a pair waits for the load: one row in flight again)
  auto join = [sh](uint32_t lo, uint32_t hi) { return __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)sh); };
  return u32x3{join(r.d[0], r.d[1]), join(r.d[1], r.d[2]), join(r.d[2], r.d[3])};
}

// FULL: H is a multiple of BR and W of BC, so every region is whole and the per-lane and per-row guards compile away
template <bool FULL>
__global__ __launch_bounds__(TPB) void tile_qc_kernel(int H, int W, int nbr, int nbc, const uint8_t* rgb, long long pitch,
                                                      const long long* origins, int thr, long long* part) {
  __shared__ uint32_t L[(BR + 2) * RS];
  __shared__ long long red[WAVES][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int per = nbr * nbc;
  const int n = blockIdx.x / per, rem = blockIdx.x - n * per;
  const int y0 = (rem / nbc) * BR, x0 = (rem % nbc) * BC;
  const int rows = FULL ? BR : min(BR, H - y0), cols = FULL ? BC : min(BC, W - x0);   // the region's own (both >= 1)
  const uint8_t* tile = rgb + (origins ? origins[n] : (long long)n * H * pitch);
  const int cnt = FULL ? 4 : max(0, min(4, cols - 4 * lane));   // pixels of this lane in a row
  int white = 0;

  // requests first: this wave's rows of y0 - 1 .. y0 + rows (reflected at the tile's edge), then the halo columns
  // x0 - 1 and x0 + cols of every row (reflected likewise), one pixel per thread
  Raw raw[RPW];
  int shift[RPW];
#pragma unroll
  for (int i = 0; i < RPW; ++i) {
    const int lr = wave + i * WAVES;
    const uint8_t* p = tile + (long long)reflect101(min(y0 - 1 + lr, H), H) * pitch + 3ll * x0 + 12 * lane;
    shift[i] = (int)(reinterpret_cast<uintptr_t>(p) & 3);
    raw[i] = load12(p, lr < rows + 2 ? 3 * cnt : 0);
  }
  const bool halo_thread = threadIdx.x < 2 * (rows + 2);
  uint32_t hr = 0, hg = 0, hb = 0;
  if (halo_thread) {
    const int lr = threadIdx.x >> 1, side = threadIdx.x & 1;
    const uint8_t* p = tile + (long long)reflect101(y0 - 1 + lr, H) * pitch + 3ll * reflect101(side ? x0 + cols : x0 - 1, W);
    hr = p[0]; hg = p[1]; hb = p[2];
  }
  // gray -> L[lr][lane]
#pragma unroll
  for (int i = 0; i < RPW; ++i) {
    const int lr = wave + i * WAVES;
    if (lr >= rows + 2) break;
    const u32x3 w = align12(raw[i], shift[i]);
    const uint32_t px[4] = {w.a & 0xFFFFFFu, (w.a >> 24) | (w.b & 0xFFFFu) << 8, (w.b >> 16) | (w.c & 0xFFu) << 16,
                            w.c >> 8};   // r | g << 8 | b << 16; pixels >= cnt are unspecified and unused
    const bool own = lr >= 1 && lr <= rows;
    uint32_t packed = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = px[j] & 255u, g = (px[j] >> 8) & 255u, b = px[j] >> 16;
      packed |= gray_of(r, g, b) << (8 * j);
      white += (own && j < cnt && r >= thr && g >= thr && b >= thr) ? 1 : 0;
    }
    L[lr * RS + lane] = packed;
  }
  if (halo_thread)
    reinterpret_cast<uint8_t*>(&L[(threadIdx.x >> 1) * RS + BC / 4])[threadIdx.x & 1] = (uint8_t)gray_of(hr, hg, hb);
  __syncthreads();

  int s1 = 0;
  uint32_t s2 = 0;
  if (cnt > 0) {
    for (int lr = 1 + wave; lr <= rows; lr += WAVES) {
      const uint32_t* row = &L[lr * RS];
      const uint32_t c = row[lane], u = row[lane - RS], d = row[lane + RS], halo = row[BC / 4];
      const uint32_t lw = lane > 0 ? row[lane - 1] : halo << 24;   // its top byte: the pixel left of this lane's first
      const uint32_t lf = c << 8 | lw >> 24;                       // byte j: gray of pixel j - 1
      uint32_t rt = c >> 8 | row[lane + 1] << 24;                  // byte j: gray of pixel j + 1
      if (4 * lane + cnt == cols) {                                // this lane holds the row's last pixel
        const int sh = 8 * (cnt - 1);
        rt = (rt & ~(255u << sh)) | ((halo >> 8) & 255u) << sh;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < cnt) {
          const int sh = 8 * j;
          const int lap = (int)(((u >> sh) & 255u) + ((d >> sh) & 255u) + ((lf >> sh) & 255u) + ((rt >> sh) & 255u)) -
                          4 * (int)((c >> sh) & 255u);
          s1 += lap;
          s2 += (uint32_t)(lap * lap);
        }
      }
    }
  }

  long long v[3] = {white, s1, (long long)s2};
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < 3; ++k) red[wave][k] = v[k];
  __syncthreads();
  if (threadIdx.x < 3) {
    long long t = 0;
    for (int w = 0; w < WAVES; ++w) t += red[w][threadIdx.x];
    part[(size_t)blockIdx.x * 3 + threadIdx.x] = t;   // row `rem` of tile n: (N, per, 3)
  }
}

// one block per tile: sums[n] = {sum of the tile's `per` rows of part, H * W}
__global__ __launch_bounds__(TPB) void tile_qc_final_kernel(int per, long long hw, const long long* part, long long* sums) {
  __shared__ long long red[WAVES][3];
  const int n = blockIdx.x;
  const long long* rows = part + (size_t)n * per * 3;
  long long v[3] = {0, 0, 0};
  for (int r = threadIdx.x; r < per; r += TPB)
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] += rows[(size_t)r * 3 + k];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < 3; ++k) red[threadIdx.x >> 6][k] = v[k];
  __syncthreads();
  if (threadIdx.x < 3) {
    long long t = 0;
    for (int w = 0; w < WAVES; ++w) t += red[w][threadIdx.x];
    sums[4 * (size_t)n + threadIdx.x] = t;
  }
  if (threadIdx.x == 3) sums[4 * (size_t)n + 3] = hw;
}

}  // namespace

extern "C" int adp_tile_qc(int N, int H, int W, const uint8_t* rgb, long long row_pitch, const long long* origins,
                           int white_threshold, long long* sums, adp_stream_t st) {
  ADP_REQUIRE(rgb && sums, "adp_tile_qc: rgb and sums must be non-null");
  ADP_REQUIRE(N >= 1, "adp_tile_qc: N must be at least 1");
  ADP_REQUIRE(H >= 2 && W >= 2, "adp_tile_qc: H and W must be at least 2 (reflect-101 borders)");
  ADP_REQUIRE(row_pitch == 0 || row_pitch >= 3ll * W, "adp_tile_qc: row_pitch is below 3 * W");
  const long long pitch = row_pitch ? row_pitch : 3ll * W;
  const int nbr = (H + BR - 1) / BR, nbc = (W + BC - 1) / BC;
  const long long blocks = (long long)N * nbr * nbc;
  ADP_REQUIRE((long long)nbr * nbc <= 0x7FFFFFFFll && blocks <= 0x7FFFFFFFll, "adp_tile_qc: too many blocks (N * H * W too large for one launch)");
  hipStream_t s = (hipStream_t)st;
  long long* part = static_cast<long long*>(adp::scratch(adp::Slot::TileQcPart, (size_t)blocks * 3 * sizeof(long long), s));
  if (!part) return -1;
  if (H % BR == 0 && W % BC == 0)
    hipLaunchKernelGGL(tile_qc_kernel<true>, dim3((unsigned)blocks), dim3(TPB), 0, s, H, W, nbr, nbc, rgb, pitch, origins,
                       white_threshold, part);
  else
    hipLaunchKernelGGL(tile_qc_kernel<false>, dim3((unsigned)blocks), dim3(TPB), 0, s, H, W, nbr, nbc, rgb, pitch, origins,
                       white_threshold, part);
  hipLaunchKernelGGL(tile_qc_final_kernel, dim3((unsigned)N), dim3(TPB), 0, s, nbr * nbc, (long long)H * W, part, sums);
  return adp::check_launch("adp_tile_qc");
}
