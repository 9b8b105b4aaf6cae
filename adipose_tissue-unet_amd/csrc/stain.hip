// Reinhard stain normalisation of packed uint8 RGB tiles (N, H, W, 3) on the GPU
// (src/utils/stain_normalization.py:32-146: _calculate_lab_stats :76-92, normalize_image :94-146; the dataset builders
// apply it tile by tile, build_dataset.py:1234-1238, so every tile is normalised with its own statistics).
//
// Colour maths: skimage's documented rgb2lab / lab2rgb (D65 white, 2-degree observer), restated:
//   decode   c > 0.04045 ? ((c + 0.055) / 1.055)^2.4 : c / 12.92      (a 256-entry table: the input is 8-bit)
//   XYZ      M rgb, M = (0.412453 0.357580 0.180423 / 0.212671 0.715160 0.072169 / 0.019334 0.119193 0.950227),
//            divided by the white point (0.95047, 1, 1.08883)
//   f(t)     t > 0.008856 ? cbrt(t) : 7.787 t + 16/116;   L = 116 fy - 16, a = 500 (fx - fy), b = 200 (fy - fz)
//   inverse  fy = (L + 16) / 116, fx = a / 500 + fy, fz = max(fy - b / 200, 0);
//            t = f > 0.2068966 ? f^3 : (f - 16/116) / 7.787, times the white point; rgb = M^-1 xyz
//   encode   c > 0.0031308 ? 1.055 c^(1/2.4) - 0.055 : 12.92 c, clipped to [0, 1]; byte = trunc(255 c) (astype(uint8))
// (skimage is not installed here: a restatement, "parity unpinned" in the tests.)
//
// Two passes, LAB recomputed in the second instead of a 12-byte-per-pixel LAB image between them:
//   1. stats: conversions in f32, sums in f64 of the deviations from the tile's first pixel (a constant tile has std
//      exactly 0 and the sums stay well conditioned). Deterministic and independent of N and of the grid: a tile is cut
//      into R = rows(H*W) fixed row sets of pixel chunks, each row is reduced in a fixed order (thread, wave butterfly,
//      LDS) into one row of the partial buffer, and a per-tile finaliser sums the rows in a fixed order. No atomics.
//   2. apply: (lab - src_mean) * (tgt_std / src_std) + tgt_mean on the f64 statistics, back to sRGB bytes, and / or the
//      fused gray plane (R*19595 + G*38470 + B*7471 + 0x8000) >> 16 of those bytes (PIL mode L).
// Memory access: 4 pixels = 12 bytes = 3 dwords per thread where the tile is dword-aligned (float4 for the gray plane),
// bytes otherwise and for the last H*W % 4 pixels.
#include "common.h"
#include "workspace.h"
#include "../../include/adipose_hip.h"

namespace {

constexpr int TPB = 256;
constexpr int CH = 2;             // 4-pixel groups per thread and chunk of the stats pass (chunk = 2048 pixels)
constexpr int MAX_ROWS = 2048;    // partial rows per tile
constexpr int MAX_BLOCKS = 2048;  // blocks per launch (all tiles)

struct Lut { float v[256]; };       // sRGB decode of every byte value, f64 on the host rounded to f32
struct Mat3 { float m[9]; };        // M^-1 (inverted in f64 on the host)
struct Target { double mean[3], std[3]; };
struct u32x3 { uint32_t a, b, c; };

ADP_DEV void rgb2lab(float r, float g, float b, float& L, float& A, float& B) {
  const float x = (0.412453f * r + 0.357580f * g + 0.180423f * b) / 0.95047f;
  const float y = 0.212671f * r + 0.715160f * g + 0.072169f * b;
  const float z = (0.019334f * r + 0.119193f * g + 0.950227f * b) / 1.08883f;
  auto f = [](float t) { return t > 0.008856f ? cbrtf(t) : 7.787f * t + 16.f / 116.f; };
  const float fx = f(x), fy = f(y), fz = f(z);
  L = 116.f * fy - 16.f;
  A = 500.f * (fx - fy);
  B = 200.f * (fy - fz);
}

ADP_DEV float srgb_encode(float c) {
  c = c > 0.0031308f ? 1.055f * powf(c, 1.f / 2.4f) - 0.055f : 12.92f * c;
  return fminf(fmaxf(c, 0.f), 1.f);
}

// -> the three output bytes packed as r | g << 8 | b << 16
ADP_DEV uint32_t lab2rgb_bytes(float L, float A, float B, const Mat3& mi) {
  const float fy = (L + 16.f) / 116.f;
  const float fx = A / 500.f + fy;
  const float fz = fmaxf(fy - B / 200.f, 0.f);
  auto t = [](float f) { return f > 0.2068966f ? f * f * f : (f - 16.f / 116.f) / 7.787f; };
  const float x = t(fx) * 0.95047f, y = t(fy), z = t(fz) * 1.08883f;
  const float r = srgb_encode(mi.m[0] * x + mi.m[1] * y + mi.m[2] * z);
  const float g = srgb_encode(mi.m[3] * x + mi.m[4] * y + mi.m[5] * z);
  const float b = srgb_encode(mi.m[6] * x + mi.m[7] * y + mi.m[8] * z);
  return (uint32_t)(r * 255.f) | (uint32_t)(g * 255.f) << 8 | (uint32_t)(b * 255.f) << 16;
}

// pixels 4g .. 4g + cnt - 1 of a tile as px[j] = r | g << 8 | b << 16
ADP_DEV void load_group(const uint8_t* tile, size_t g, int cnt, bool vec, uint32_t* px) {
  if (vec && cnt == 4) {
    const u32x3 w = *reinterpret_cast<const u32x3*>(tile + 12 * g);
    px[0] = w.a & 0xFFFFFFu;
    px[1] = (w.a >> 24) | (w.b & 0xFFFFu) << 8;
    px[2] = (w.b >> 16) | (w.c & 0xFFu) << 16;
    px[3] = w.c >> 8;
  } else {
    for (int j = 0; j < cnt; ++j) {
      const uint8_t* p = tile + 12 * g + 3 * j;
      px[j] = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
    }
  }
}

// sum over the block of v[0..6) in a fixed order; valid in threads 0..5 (thread k returns the sum of v[k])
ADP_DEV double block_sum6(double* v, double (*red)[6]) {
#pragma unroll
  for (int k = 0; k < 6; ++k)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
  __syncthreads();   // the previous use of red has been read
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < 6; ++k) red[threadIdx.x >> 6][k] = v[k];
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x < 6)
    for (int w = 0; w < TPB / 64; ++w) t += red[w][threadIdx.x];
  return t;
}

// part: (N, R + 1, 6) f64. Row r < R of tile n: {sum dL, sum dA, sum dB, sum dL^2, sum dA^2, sum dB^2} over the chunks
// r, r + R, ... of the tile, d = lab - lab(first pixel); row R: lab(first pixel).
__global__ __launch_bounds__(TPB) void stain_stats_kernel(size_t HW, int R, const uint8_t* rgb, double* part, Lut lut_arg) {
  __shared__ float lut[256];
  __shared__ double red[TPB / 64][6];
  lut[threadIdx.x] = lut_arg.v[threadIdx.x];
  __syncthreads();
  const int n = blockIdx.y;
  const uint8_t* tile = rgb + (size_t)n * HW * 3;
  const bool vec = (reinterpret_cast<uintptr_t>(tile) & 3) == 0;
  const size_t ngroups = (HW + 3) / 4, nchunks = (ngroups + (size_t)CH * TPB - 1) / ((size_t)CH * TPB);
  float L0, A0, B0;
  rgb2lab(lut[tile[0]], lut[tile[1]], lut[tile[2]], L0, A0, B0);
  double* rows = part + (size_t)n * (R + 1) * 6;
  if (blockIdx.x == 0 && threadIdx.x < 3) rows[(size_t)R * 6 + threadIdx.x] = threadIdx.x == 0 ? L0 : threadIdx.x == 1 ? A0 : B0;
  for (int r = blockIdx.x; r < R; r += gridDim.x) {
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (size_t c = r; c < nchunks; c += R) {
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const size_t g = (c * CH + j) * TPB + threadIdx.x;
        if (g >= ngroups) continue;
        const int cnt = (int)std::min<size_t>(4, HW - 4 * g);
        uint32_t px[4];
        load_group(tile, g, cnt, vec, px);
        for (int q = 0; q < cnt; ++q) {
          float L, A, B;
          rgb2lab(lut[px[q] & 255u], lut[(px[q] >> 8) & 255u], lut[px[q] >> 16], L, A, B);
          const double dl = (double)L - (double)L0, da = (double)A - (double)A0, db = (double)B - (double)B0;
          acc[0] += dl; acc[1] += da; acc[2] += db;
          acc[3] += dl * dl; acc[4] += da * da; acc[5] += db * db;
        }
      }
    }
    const double t = block_sum6(acc, red);
    if (threadIdx.x < 6) rows[(size_t)r * 6 + threadIdx.x] = t;
  }
}

// one block per tile: thread t sums rows t, t + 256, ... in index order, then the block's fixed-order sum
__global__ __launch_bounds__(TPB) void stain_stats_final_kernel(size_t HW, int R, const double* part, double* stats) {
  __shared__ double red[TPB / 64][6];
  __shared__ double tot[6];
  const int n = blockIdx.x;
  const double* rows = part + (size_t)n * (R + 1) * 6;
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int r = threadIdx.x; r < R; r += TPB)
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[k] += rows[(size_t)r * 6 + k];
  const double t = block_sum6(acc, red);
  if (threadIdx.x < 6) tot[threadIdx.x] = t;
  __syncthreads();
  if (threadIdx.x < 3) {
    const int k = threadIdx.x;
    const double cnt = (double)HW, m = tot[k] / cnt;
    const double var = tot[3 + k] / cnt - m * m;
    stats[(size_t)n * 6 + k] = rows[(size_t)R * 6 + k] + m;
    stats[(size_t)n * 6 + 3 + k] = sqrt(fmax(var, 0.0));
  }
}

__global__ __launch_bounds__(TPB) void stain_apply_kernel(size_t HW, const uint8_t* rgb, const double* src_stats, Target tgt,
                                                          Mat3 mi, uint8_t* rgb_out, float* gray_out, Lut lut_arg) {
  __shared__ float lut[256];
  lut[threadIdx.x] = lut_arg.v[threadIdx.x];
  __syncthreads();
  const int n = blockIdx.y;
  const uint8_t* tile = rgb + (size_t)n * HW * 3;
  uint8_t* out = rgb_out ? rgb_out + (size_t)n * HW * 3 : nullptr;
  float* gray = gray_out ? gray_out + (size_t)n * HW : nullptr;
  const bool vec = (reinterpret_cast<uintptr_t>(tile) & 3) == 0;
  const bool vec_out = (reinterpret_cast<uintptr_t>(out) & 3) == 0, vec_gray = (reinterpret_cast<uintptr_t>(gray) & 15) == 0;
  double sm[3], k[3], tm[3];   // v' = (v - sm) * k + tm; a channel without spread becomes the target mean
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double sd = src_stats[(size_t)n * 6 + 3 + c];
    sm[c] = src_stats[(size_t)n * 6 + c];
    k[c] = sd == 0.0 ? 0.0 : tgt.std[c] / sd;
    tm[c] = tgt.mean[c];
  }
  const size_t ngroups = (HW + 3) / 4;
  for (size_t g = blockIdx.x * (size_t)TPB + threadIdx.x; g < ngroups; g += (size_t)gridDim.x * TPB) {
    const int cnt = (int)std::min<size_t>(4, HW - 4 * g);
    uint32_t px[4] = {0, 0, 0, 0};
    load_group(tile, g, cnt, vec, px);
    float gr[4] = {0.f, 0.f, 0.f, 0.f};
    for (int q = 0; q < cnt; ++q) {
      float L, A, B;
      rgb2lab(lut[px[q] & 255u], lut[(px[q] >> 8) & 255u], lut[px[q] >> 16], L, A, B);
      L = (float)(((double)L - sm[0]) * k[0] + tm[0]);
      A = (float)(((double)A - sm[1]) * k[1] + tm[1]);
      B = (float)(((double)B - sm[2]) * k[2] + tm[2]);
      const uint32_t o = lab2rgb_bytes(L, A, B, mi);
      px[q] = o;
      gr[q] = (float)(((o & 255u) * 19595u + ((o >> 8) & 255u) * 38470u + (o >> 16) * 7471u + 0x8000u) >> 16);
    }
    if (out) {
      if (vec_out && cnt == 4) {
        u32x3 w;
        w.a = px[0] | px[1] << 24;
        w.b = px[1] >> 8 | px[2] << 16;
        w.c = px[2] >> 16 | px[3] << 8;
        *reinterpret_cast<u32x3*>(out + 12 * g) = w;
      } else {
        for (int q = 0; q < cnt; ++q) {
          uint8_t* p = out + 12 * g + 3 * q;
          p[0] = (uint8_t)px[q]; p[1] = (uint8_t)(px[q] >> 8); p[2] = (uint8_t)(px[q] >> 16);
        }
      }
    }
    if (gray) {
      if (vec_gray && cnt == 4) {
        *reinterpret_cast<float4*>(gray + 4 * g) = make_float4(gr[0], gr[1], gr[2], gr[3]);
      } else {
        for (int q = 0; q < cnt; ++q) gray[4 * g + q] = gr[q];
      }
    }
  }
}

const Lut& decode_lut() {
  static const Lut lut = [] {
    Lut l;
    for (int i = 0; i < 256; ++i) {
      const double c = i / 255.0;
      l.v[i] = (float)(c > 0.04045 ? std::pow((c + 0.055) / 1.055, 2.4) : c / 12.92);
    }
    return l;
  }();
  return lut;
}

const Mat3& rgb_from_xyz() {   // inverse of M in f64 (adjugate / determinant), rounded to f32
  static const Mat3 inv = [] {
    const double a[9] = {0.412453, 0.357580, 0.180423, 0.212671, 0.715160, 0.072169, 0.019334, 0.119193, 0.950227};
    const double det = a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) +
                       a[2] * (a[3] * a[7] - a[4] * a[6]);
    const double adj[9] = {a[4] * a[8] - a[5] * a[7], a[2] * a[7] - a[1] * a[8], a[1] * a[5] - a[2] * a[4],
                           a[5] * a[6] - a[3] * a[8], a[0] * a[8] - a[2] * a[6], a[2] * a[3] - a[0] * a[5],
                           a[3] * a[7] - a[4] * a[6], a[1] * a[6] - a[0] * a[7], a[0] * a[4] - a[1] * a[3]};
    Mat3 r;
    for (int i = 0; i < 9; ++i) r.m[i] = (float)(adj[i] / det);
    return r;
  }();
  return inv;
}

inline int grid_x(size_t want, int N) {
  return (int)std::min<size_t>(std::max<size_t>(want, 1), (size_t)std::max(1, MAX_BLOCKS / N));
}

}  // namespace

extern "C" int adp_stain_lab_stats(int N, int H, int W, const uint8_t* rgb, double* stats, adp_stream_t st) {
  ADP_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0 && rgb && stats,
              "adp_stain_lab_stats: bad arguments (N in 1..65535, H*W > 0, rgb and stats non-null)");
  hipStream_t s = (hipStream_t)st;
  const size_t HW = (size_t)H * W, ngroups = (HW + 3) / 4;
  const size_t nchunks = (ngroups + (size_t)CH * TPB - 1) / ((size_t)CH * TPB);
  const int R = (int)std::min<size_t>(nchunks, MAX_ROWS);   // a function of H*W alone: the sums do not depend on N
  double* part = static_cast<double*>(adp::scratch(adp::Slot::StainPart, (size_t)N * (R + 1) * 6 * sizeof(double), s));
  if (!part) return -1;
  hipLaunchKernelGGL(stain_stats_kernel, dim3(grid_x(R, N), N), dim3(TPB), 0, s, HW, R, rgb, part, decode_lut());
  hipLaunchKernelGGL(stain_stats_final_kernel, dim3(N), dim3(TPB), 0, s, HW, R, part, stats);
  return adp::check_launch("adp_stain_lab_stats");
}

extern "C" int adp_stain_reinhard_apply(int N, int H, int W, const uint8_t* rgb, const double* src_stats,
                                        const double* tgt, uint8_t* rgb_out, float* gray_out, adp_stream_t st) {
  ADP_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0 && rgb && src_stats && tgt,
              "adp_stain_reinhard_apply: bad arguments (N in 1..65535, H*W > 0, rgb, src_stats and tgt non-null)");
  ADP_REQUIRE(rgb_out || gray_out, "adp_stain_reinhard_apply: rgb_out and gray_out are both NULL");
  Target t;
  for (int c = 0; c < 3; ++c) { t.mean[c] = tgt[c]; t.std[c] = tgt[3 + c]; }
  const size_t HW = (size_t)H * W, ngroups = (HW + 3) / 4;
  hipLaunchKernelGGL(stain_apply_kernel, dim3(grid_x((ngroups + TPB - 1) / TPB, N), N), dim3(TPB), 0, (hipStream_t)st, HW,
                     rgb, src_stats, t, rgb_from_xyz(), rgb_out, gray_out, decode_lut());
  return adp::check_launch("adp_stain_reinhard_apply");
}
