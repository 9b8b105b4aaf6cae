// Contrast-limited adaptive histogram equalisation of 8-bit gray planes (cv2.createCLAHE(clip, (tx, ty)).apply), the
// contrast step of the reference's tile pipeline (pre-post-processing_tools/preprocess_small_MS_SIMs.py:393-431, flag
// --enhance-contrast; large_wsi_to_small_wsi_MS.py:202-210 enhance_clahe; adaptive_clahe_function.py), and the two
// helpers of the adaptive normalisation (gray statistics, percentile stretch). The definition (OpenCV 4's clahe.cpp for
// 8-bit input, restated) is in contrast.py's docstring; contrast.py's numpy path is the same arithmetic, bit for bit.
//
// Geometry: the image is extended by reflect-101 at the bottom and right to (He, We) = (ty * th, tx * tw); the extension
// is index arithmetic (row ey >= H reads row 2H - 2 - ey), never a padded copy. The entry points recompute the geometry
// from (H, W, ty, tx) and refuse an extension beyond dim - 1, so no reflected index leaves the image.
//
// adp_clahe_hist: a block counts a slab of one tile, up to SLAB_ROWS rows x SLAB_COLS columns, so that a grid of few
// large tiles still fills the chip (6144^2 at 16 x 16: 256 tiles of 384 x 384 = 1536 blocks; a 1 x 1 grid, the global
// histogram of adp_u8_stretch: 96 x 6 blocks). A lane takes 16 pixels at a 16-aligned x: one 16-byte load where the row
// is 16-byte aligned (W % 16 == 0, aligned base, uint8), byte or float loads otherwise (edges of a tile, the reflected
// columns, float32 planes). Every wave has its own 256-bin histogram in LDS (ds_add_u32, no return). Histology is
// mostly near-white, and LDS atomics serialise per address, so equal values are merged before the atomic: a lane adds
// one count per run of equal neighbouring values of its 16, and when all 64 lanes of a wave hold one and the same value
// (the constant image, the background of a slide) lane 0 adds the wave's whole count once. The block's four histograms
// are summed and the non-zero bins are added to the tile's global histogram with integer atomicAdd: integer sums do not
// depend on order, so the result is the same for every grid, N and run.
//
// adp_clahe_lut: one wave per tile, 4 bins per lane: clip, excess by a wave reduction, redistribution in closed form
// (bin i gets batch + [resid > 0 and i % step == 0 and i / step < resid]), inclusive scan (4 in the lane, shuffles
// across), one float multiply per bin, 256 bytes out.
//
// adp_clahe_apply: the rows of the image fall into ty + 1 bands with constant (y1, y2): band k holds the rows with
// floor(tyf) = k - 1. The bands' first rows are found on the host with the same float32 expression the kernel uses (the
// product y * (1 / th) is rounded, so integer arithmetic would not find the same boundary), a block takes APPLY_ROWS rows
// of one band and stages only its two LUT rows in LDS, interleaved: S[x][v] = {lut[y1][x][v], lut[y2][x][v]}, 2 * tx *
// 256 bytes, so a pixel gathers two 16-bit words. 16 pixels per lane where W % 16 == 0 and the planes are 16-byte
// aligned: a thread keeps its 16 columns down the block's rows, so their two tile columns and weights are formed once
// (6144^2 at 16 x 16: 44 us with them formed per pixel, 35 us so; 144 VGPRs, which the 3 blocks per CU of that grid do
// not miss). One pixel per lane otherwise. Contraction is off for the whole file (and the float helpers are plain
// operators of this file, not the __f*_rn intrinsics, which compile under the header's setting and fuse): every
// multiply and add rounds on its own.
//
// adp_gray_stats: {sum g, sum g^2, sum lap, sum lap^2, H * W} per image, lap the 4-neighbour Laplacian with reflect-101
// borders as in tileqc.hip; at most STAT_BLOCKS blocks per image, one 64-bit integer atomicAdd per block and sum.
// adp_u8_stretch: every block rebuilds its image's 256-entry float32 table from the 256-bin histogram (scan in LDS, the
// two order statistics with numpy's linear interpolation, all float64) and maps 16 pixels per lane through it.
#include "common.h"
#include "../../include/adipose_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256, WAVES = TPB / 64;
constexpr int SLAB_ROWS = ADP_CLAHE_SLAB_ROWS, SLAB_COLS = ADP_CLAHE_SLAB_COLS;
constexpr int MAXG = ADP_CLAHE_MAX_GRID;
constexpr int APPLY_ROWS = 8;
constexpr int STAT_BLOCKS = 256;
static_assert(SLAB_COLS % 16 == 0, "a slab starts at a multiple of 16 columns of its tile only if its width is one");

struct Geo { int He, We, th, tw; };

// the geometry, or false with the error set
bool geometry(const char* who, int H, int W, int ty, int tx, Geo* g) {
  if (ty < 1 || ty > MAXG || tx < 1 || tx > MAXG) {
    adp::set_error(std::string(who) + ": the tile grid must be 1 .. 64 both ways");
    return false;
  }
  if (H < 1 || W < 1 || (long long)H * W > 0x7FFFFFFFll - 2 * MAXG * (long long)(H + W)) {
    adp::set_error(std::string(who) + ": H and W must be at least 1 and H * W below 2^31");
    return false;
  }
  int He = H, We = W;
  if (H % ty != 0 || W % tx != 0) {
    He = H + (ty - H % ty);
    We = W + (tx - W % tx);
    if (He - H > H - 1 || We - W > W - 1) {
      adp::set_error(std::string(who) + ": the image is too small for the grid (reflect-101 extension beyond dim - 1)");
      return false;
    }
  }
  *g = Geo{He, We, He / ty, We / tx};
  return true;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// single float32 operations (compiled under contract(off) above; the __f*_rn intrinsics are plain operators compiled
// under the header's setting, and fuse)
ADP_DEV float mulf(float a, float b) { return a * b; }
ADP_DEV float addf(float a, float b) { return a + b; }
ADP_DEV float subf(float a, float b) { return a - b; }
ADP_DEV unsigned to_u8(float f) { return (unsigned)fminf(fmaxf(rintf(f), 0.f), 255.f); }

// ---------------------------------------------------------------- histogram
// VEC: uint8 rows that start on 16 bytes (W % 16 == 0, aligned base)
template <bool VEC>
__global__ __launch_bounds__(TPB) void clahe_hist_kernel(int H, int W, int ty, int tx, int th, int tw, int nsr, int nsc,
                                                         const void* __restrict__ src, int f32, unsigned* __restrict__ hist) {
  __shared__ unsigned h[WAVES][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < WAVES * 256; i += TPB) (&h[0][0])[i] = 0;
  __syncthreads();
  // block -> (image, tile, slab)
  int b = blockIdx.x;
  const int sc = b % nsc; b /= nsc;
  const int sr = b % nsr; b /= nsr;
  const int ix = b % tx; b /= tx;
  const int iy = b % ty;
  const int n = b / ty;
  const int ey0 = iy * th + sr * SLAB_ROWS, rows = min(SLAB_ROWS, th - sr * SLAB_ROWS);
  const int xa = ix * tw + sc * SLAB_COLS, xb = min(xa + SLAB_COLS, ix * tw + tw);   // extended columns [xa, xb)
  const int c0 = xa >> 4, nc = ((xb + 15) >> 4) - c0;                                 // 16-aligned chunks that meet them
  const int units = rows * nc;
  const size_t img = (size_t)n * H * W;
  const uint8_t* s8 = static_cast<const uint8_t*>(src) + img;
  const float* s32 = static_cast<const float*>(src) + img;
  unsigned* mine = h[wave];

  for (int ub = threadIdx.x - lane; ub < units; ub += TPB) {   // the bound is the wave's: __all below sees whole waves
    const int u = ub + lane;
    const bool act = u < units;
    unsigned v[16] = {};
    unsigned valid = 0;
    if (act) {
      const int r = u / nc, xs = (c0 + (u - r * nc)) << 4;
      const int ey = ey0 + r, y = ey < H ? ey : 2 * H - 2 - ey;
      const size_t row = (size_t)y * W;
      if (VEC && xs >= xa && xs + 16 <= xb && xs + 16 <= W) {
        const uint4 q = *reinterpret_cast<const uint4*>(s8 + row + xs);
        const unsigned d[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = (d[j >> 2] >> (8 * (j & 3))) & 255u;
        valid = 0xFFFFu;
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int ex = xs + j;
          v[j] = 0;
          if (ex >= xa && ex < xb) {
            const int x = ex < W ? ex : 2 * W - 2 - ex;
            v[j] = f32 ? to_u8(s32[row + x]) : s8[row + x];
            valid |= 1u << j;
          }
        }
      }
    }
    bool one = valid == 0xFFFFu;
#pragma unroll
    for (int j = 1; j < 16; ++j) one = one && v[j] == v[0];
    const unsigned v0 = (unsigned)__builtin_amdgcn_readfirstlane((int)v[0]);   // lane 0 is active: ub < units
    const unsigned long long active = __ballot(act);   // by every lane, before lane 0 goes on alone
    if (__all(!act || (one && v[0] == v0))) {
      if (lane == 0) atomicAdd(&mine[v0], 16u * (unsigned)__popcll(active));
      continue;
    }
    // runs of equal neighbouring values among the valid pixels
    unsigned cur = 0, cnt = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (!((valid >> j) & 1u)) continue;
      if (cnt && v[j] != cur) {
        atomicAdd(&mine[cur], cnt);
        cnt = 0;
      }
      cur = v[j];
      ++cnt;
    }
    if (cnt) atomicAdd(&mine[cur], cnt);
  }
  __syncthreads();
  unsigned t = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) t += h[w][threadIdx.x];
  if (t) atomicAdd(&hist[(((size_t)n * ty + iy) * tx + ix) * 256 + threadIdx.x], t);
}

// ---------------------------------------------------------------- look-up tables
__global__ __launch_bounds__(TPB) void clahe_lut_kernel(int tiles, unsigned clip, float scale, const unsigned* __restrict__ hist,
                                                        uint8_t* __restrict__ lut) {
  const int lane = threadIdx.x & 63;
  const int tile = blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (tile >= tiles) return;   // whole waves leave
  const uint4 q = reinterpret_cast<const uint4*>(hist + (size_t)tile * 256)[lane];
  unsigned hb[4] = {q.x, q.y, q.z, q.w};
  if (clip > 0) {
    unsigned excess = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      excess += hb[j] > clip ? hb[j] - clip : 0u;
      hb[j] = min(hb[j], clip);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) excess += __shfl_xor(excess, o, 64);
    const unsigned batch = excess >> 8, resid = excess & 255u;
    const unsigned step = resid ? max(256u / resid, 1u) : 1u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned i = 4u * lane + j;
      hb[j] += batch + ((resid > 0 && i % step == 0 && i / step < resid) ? 1u : 0u);
    }
  }
  hb[1] += hb[0];
  hb[2] += hb[1];
  hb[3] += hb[2];
  unsigned incl = hb[3];   // inclusive scan of the lanes' totals
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  const unsigned before = incl - hb[3];
  unsigned packed = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float f = rintf(mulf((float)(before + hb[j]), scale));
    packed |= (unsigned)fminf(f, 255.f) << (8 * j);
  }
  reinterpret_cast<unsigned*>(lut + (size_t)tile * 256)[lane] = packed;
}

// ---------------------------------------------------------------- interpolation
struct Bands {
  int first[MAXG + 2];   // band k = rows [first[k], first[k + 1]): floor(tyf) = k - 1
  int block[MAXG + 2];   // blocks of the bands before k (per image)
};

// floor(float(i) * inv - 0.5f) and the weight of the upper neighbour, as the definition rounds them
ADP_DEV float axis_pos(int i, float inv, float* a) {
  const float f = subf(mulf((float)i, inv), 0.5f);
  const float fl = floorf(f);
  *a = subf(f, fl);
  return fl;
}

// the two columns of a pixel as LDS indices (x1 * 256 | x2 * 256 << 16) and the weight of the second
ADP_DEV unsigned columns(int x, float inv_tw, int tx, float* xa) {
  const int fl = (int)axis_pos(x, inv_tw, xa);
  const int x1 = min(max(fl, 0), tx - 1), x2 = min(fl + 1, tx - 1);
  return (unsigned)(x1 << 8) | (unsigned)(x2 << 8) << 16;
}

ADP_DEV unsigned interp(const unsigned short* __restrict__ S, unsigned v, unsigned cols, float xa, float ya, float ya1) {
  const float xa1 = subf(1.f, xa);
  const unsigned p1 = S[(cols & 0xFFFFu) + v], p2 = S[(cols >> 16) + v];   // {lut[y1], lut[y2]} of the two columns
  const float top = addf(mulf((float)(p1 & 255u), xa1), mulf((float)(p2 & 255u), xa));
  const float bot = addf(mulf((float)(p1 >> 8), xa1), mulf((float)(p2 >> 8), xa));
  return to_u8(addf(mulf(top, ya1), mulf(bot, ya)));
}

template <bool VEC>
__global__ __launch_bounds__(TPB) void clahe_apply_kernel(int H, int W, int ty, int tx, float inv_th, float inv_tw,
                                                          int per_image, Bands bands, const void* __restrict__ src, int f32,
                                                          const uint8_t* __restrict__ lut, void* __restrict__ dst, int dst_f32) {
  extern __shared__ __attribute__((aligned(16))) unsigned short S[];   // [tx][256] of {lut[y1], lut[y2]}
  const int n = blockIdx.x / per_image, rem = blockIdx.x - n * per_image;
  int k = 0;
  while (k < ty && bands.block[k + 1] <= rem) ++k;   // the same in every lane
  const int r0 = bands.first[k] + (rem - bands.block[k]) * APPLY_ROWS, r1 = min(r0 + APPLY_ROWS, bands.first[k + 1]);
  const int y1 = max(k - 1, 0), y2 = min(k, ty - 1);
  {
    const uint4* a = reinterpret_cast<const uint4*>(lut + ((size_t)n * ty + y1) * tx * 256);
    const uint4* b = reinterpret_cast<const uint4*>(lut + ((size_t)n * ty + y2) * tx * 256);
    uint4* out = reinterpret_cast<uint4*>(S);
    for (int i = threadIdx.x; i < tx * 16; i += TPB) {   // 16 bytes of either row -> 32 bytes
      const uint4 p = a[i], q = b[i];
      const unsigned pa[4] = {p.x, p.y, p.z, p.w}, qa[4] = {q.x, q.y, q.z, q.w};
      unsigned o[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        o[2 * j] = (pa[j] & 255u) | (qa[j] & 255u) << 8 | (pa[j] & 0xFF00u) << 8 | (qa[j] & 0xFF00u) << 16;
        o[2 * j + 1] = ((pa[j] >> 16) & 255u) | ((qa[j] >> 16) & 255u) << 8 | (pa[j] >> 24) << 16 | (qa[j] >> 24) << 24;
      }
      out[2 * i] = make_uint4(o[0], o[1], o[2], o[3]);
      out[2 * i + 1] = make_uint4(o[4], o[5], o[6], o[7]);
    }
  }
  __syncthreads();
  const size_t img = (size_t)n * H * W;
  const uint8_t* s8 = static_cast<const uint8_t*>(src) + img;
  const float* s32 = static_cast<const float*>(src) + img;
  uint8_t* d8 = static_cast<uint8_t*>(dst) + img;
  float* d32 = static_cast<float*>(dst) + img;
  if (VEC) {
    // a thread keeps 16 columns and walks down the block's rows: the columns' indices and weights are formed once.
    // Where a row has fewer than TPB chunks the threads split the rows among groups of `per_row`
    const int cw = W >> 4, per_row = min(cw, TPB), groups = TPB / per_row;
    const int cg = threadIdx.x % per_row, rg = threadIdx.x / per_row;
    for (int c = cg; c < cw && rg < groups; c += per_row) {
      const int x0 = c << 4;
      float xa[16];
      unsigned cols[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) cols[j] = columns(x0 + j, inv_tw, tx, &xa[j]);
      for (int y = r0 + rg; y < r1; y += groups) {
        float ya;
        axis_pos(y, inv_th, &ya);
        const float ya1 = subf(1.f, ya);
        const size_t at = (size_t)y * W + x0;
        unsigned v[16];
        if (f32) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float4 q = reinterpret_cast<const float4*>(s32 + at)[j];
            v[4 * j] = to_u8(q.x); v[4 * j + 1] = to_u8(q.y); v[4 * j + 2] = to_u8(q.z); v[4 * j + 3] = to_u8(q.w);
          }
        } else {
          const uint4 q = *reinterpret_cast<const uint4*>(s8 + at);
          const unsigned d[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
          for (int j = 0; j < 16; ++j) v[j] = (d[j >> 2] >> (8 * (j & 3))) & 255u;
        }
        unsigned o[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) o[j] = interp(S, v[j], cols[j], xa[j], ya, ya1);
        if (dst_f32) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            reinterpret_cast<float4*>(d32 + at)[j] = make_float4((float)o[4 * j], (float)o[4 * j + 1], (float)o[4 * j + 2], (float)o[4 * j + 3]);
        } else {
          unsigned w[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) w[j] = o[4 * j] | o[4 * j + 1] << 8 | o[4 * j + 2] << 16 | o[4 * j + 3] << 24;
          *reinterpret_cast<uint4*>(d8 + at) = make_uint4(w[0], w[1], w[2], w[3]);
        }
      }
    }
  } else {
    const int units = (r1 - r0) * W;
    for (int u = threadIdx.x; u < units; u += TPB) {
      const int r = u / W, x = u - r * W, y = r0 + r;
      float ya;
      axis_pos(y, inv_th, &ya);
      const size_t at = (size_t)y * W + x;
      float xa;
      const unsigned cols = columns(x, inv_tw, tx, &xa);
      const unsigned o = interp(S, f32 ? to_u8(s32[at]) : s8[at], cols, xa, ya, subf(1.f, ya));
      if (dst_f32) d32[at] = (float)o;
      else d8[at] = (uint8_t)o;
    }
  }
}

// ---------------------------------------------------------------- gray statistics
ADP_DEV int reflect101(int i, int n) { return i < 0 ? -i : i >= n ? 2 * n - 2 - i : i; }

__global__ __launch_bounds__(TPB) void gray_stats_kernel(int H, int W, int per_image, const void* __restrict__ src, int f32,
                                                         unsigned long long* __restrict__ sums) {
  __shared__ long long red[WAVES][4];
  const int n = blockIdx.x / per_image, rem = blockIdx.x - n * per_image;
  const size_t img = (size_t)n * H * W;
  const uint8_t* s8 = static_cast<const uint8_t*>(src) + img;
  const float* s32 = static_cast<const float*>(src) + img;
  auto px = [&](int y, int x) -> int { const size_t at = (size_t)y * W + x; return f32 ? (int)to_u8(s32[at]) : (int)s8[at]; };
  long long v[4] = {0, 0, 0, 0};
  const int total = H * W;
  for (int p = rem * TPB + threadIdx.x; p < total; p += per_image * TPB) {
    const int y = p / W, x = p - y * W;
    const int g = px(y, x);
    const int lap = px(reflect101(y - 1, H), x) + px(reflect101(y + 1, H), x) + px(y, reflect101(x - 1, W)) +
                    px(y, reflect101(x + 1, W)) - 4 * g;
    v[0] += g;
    v[1] += g * g;
    v[2] += lap;
    v[3] += lap * lap;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < 4; ++k) red[threadIdx.x >> 6][k] = v[k];
  __syncthreads();
  if (threadIdx.x < 4) {
    long long t = 0;
    for (int w = 0; w < WAVES; ++w) t += red[w][threadIdx.x];
    if (t) atomicAdd(&sums[5 * (size_t)n + threadIdx.x], (unsigned long long)t);   // two's complement: the sign survives
  }
  if (threadIdx.x == 4 && rem == 0) sums[5 * (size_t)n + 4] = (unsigned long long)total;
}

// ---------------------------------------------------------------- percentile stretch
// VEC: n_px % 16 == 0 and aligned planes
template <bool VEC>
__global__ __launch_bounds__(TPB) void u8_stretch_kernel(size_t n_px, int per_image, const uint8_t* __restrict__ src,
                                                         const unsigned* __restrict__ hist, double p_low, double p_high, int mode,
                                                         float* __restrict__ dst) {
  __shared__ unsigned long long cum[256];
  __shared__ double lohi[2];
  __shared__ float table[256];
  const int n = blockIdx.x / per_image, rem = blockIdx.x - n * per_image;
  cum[threadIdx.x] = hist[(size_t)n * 256 + threadIdx.x];
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {   // inclusive scan
    const unsigned long long add = threadIdx.x >= o ? cum[threadIdx.x - o] : 0ull;
    __syncthreads();
    cum[threadIdx.x] += add;
    __syncthreads();
  }
  if (threadIdx.x < 2) {
    const unsigned long long cnt = cum[255] ? cum[255] : 1ull;   // (an all-zero histogram: lo = hi = 255, nothing reads past it)
    const double q = (threadIdx.x ? p_high : p_low) / 100.0;
    const double pos = (double)(cnt - 1) * q;
    const double kf = floor(pos), t = pos - kf;
    const unsigned long long k = (unsigned long long)kf, k1 = k + 1 < cnt ? k + 1 : cnt - 1;
    int a = 0, b = 0;   // the k-th and (k + 1)-th smallest values: the first bins whose running count passes k, k1
    while (a < 255 && cum[a] <= k) ++a;
    while (b < 255 && cum[b] <= k1) ++b;
    const double d = (double)b - (double)a;
    lohi[threadIdx.x] = t >= 0.5 ? (double)b - d * (1.0 - t) : (double)a + d * t;   // numpy's _lerp
  }
  __syncthreads();
  {
    const double lo = lohi[0], hi = lohi[1];
    const double den = mode == 0 ? (hi - lo) + 1e-3 : fmax(hi - lo, 1e-3);
    table[threadIdx.x] = (float)fmin(fmax(((double)threadIdx.x - lo) / den, 0.0), 1.0);
  }
  __syncthreads();
  const uint8_t* s = src + (size_t)n * n_px;
  float* d = dst + (size_t)n * n_px;
  if (VEC) {
    const size_t chunks = n_px >> 4;
    for (size_t c = (size_t)rem * TPB + threadIdx.x; c < chunks; c += (size_t)per_image * TPB) {
      const uint4 q = reinterpret_cast<const uint4*>(s)[c];
      const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        reinterpret_cast<float4*>(d)[4 * c + j] = make_float4(table[w[j] & 255u], table[(w[j] >> 8) & 255u],
                                                              table[(w[j] >> 16) & 255u], table[w[j] >> 24]);
    }
  } else {
    for (size_t p = (size_t)rem * TPB + threadIdx.x; p < n_px; p += (size_t)per_image * TPB) d[p] = table[s[p]];
  }
}

}  // namespace

extern "C" int adp_clahe_hist(int N, int H, int W, const void* src, int src_f32, int ty, int tx, unsigned* hist,
                              adp_stream_t st) {
  Geo g;
  if (!geometry("adp_clahe_hist", H, W, ty, tx, &g)) return -1;
  ADP_REQUIRE(N >= 1, "adp_clahe_hist: N must be at least 1");
  ADP_REQUIRE(src && hist, "adp_clahe_hist: src and hist must be non-null");
  const int nsr = (g.th + SLAB_ROWS - 1) / SLAB_ROWS, nsc = (g.tw + SLAB_COLS - 1) / SLAB_COLS;
  const long long blocks = (long long)N * ty * tx * nsr * nsc;
  ADP_REQUIRE(blocks <= 0x7FFFFFFFll, "adp_clahe_hist: too many blocks (N * H * W too large for one launch)");
  hipStream_t s = (hipStream_t)st;
  if (hipMemsetAsync(hist, 0, (size_t)N * ty * tx * 256 * sizeof(unsigned), s) != hipSuccess) {
    adp::set_error("adp_clahe_hist: hipMemsetAsync failed");
    return -1;
  }
  if (!src_f32 && W % 16 == 0 && aligned16(src))
    hipLaunchKernelGGL(clahe_hist_kernel<true>, dim3((unsigned)blocks), dim3(TPB), 0, s, H, W, ty, tx, g.th, g.tw, nsr, nsc,
                       src, 0, hist);
  else
    hipLaunchKernelGGL(clahe_hist_kernel<false>, dim3((unsigned)blocks), dim3(TPB), 0, s, H, W, ty, tx, g.th, g.tw, nsr, nsc,
                       src, src_f32 ? 1 : 0, hist);
  return adp::check_launch("adp_clahe_hist");
}

extern "C" int adp_clahe_lut(int N, int ty, int tx, int area, double clip_limit, const unsigned* hist, uint8_t* lut,
                             adp_stream_t st) {
  ADP_REQUIRE(ty >= 1 && ty <= MAXG && tx >= 1 && tx <= MAXG, "adp_clahe_lut: the tile grid must be 1 .. 64 both ways");
  ADP_REQUIRE(N >= 1, "adp_clahe_lut: N must be at least 1");
  ADP_REQUIRE(area >= 1, "adp_clahe_lut: area must be at least 1");
  ADP_REQUIRE(hist && lut, "adp_clahe_lut: hist and lut must be non-null");
  ADP_REQUIRE(!(clip_limit > 0) || std::isfinite(clip_limit), "adp_clahe_lut: clip_limit must be finite");
  const long long tiles = (long long)N * ty * tx;
  ADP_REQUIRE(tiles <= 0x7FFFFFFFll - WAVES, "adp_clahe_lut: too many tiles");
  unsigned clip = 0;
  if (clip_limit > 0) {
    // max(int(clip_limit * area / 256), 1); a limit of `area` or more clips nothing, as any larger one
    const double c = clip_limit * (double)area / 256.0;
    clip = c >= (double)area ? (unsigned)area : std::max((unsigned)(long long)c, 1u);
  }
  const float scale = 255.f / (float)area;
  hipLaunchKernelGGL(clahe_lut_kernel, dim3((unsigned)((tiles + WAVES - 1) / WAVES)), dim3(TPB), 0, (hipStream_t)st,
                     (int)tiles, clip, scale, hist, lut);
  return adp::check_launch("adp_clahe_lut");
}

extern "C" int adp_clahe_apply(int N, int H, int W, const void* src, int src_f32, int ty, int tx, const uint8_t* lut,
                               void* dst, int dst_f32, adp_stream_t st) {
  Geo g;
  if (!geometry("adp_clahe_apply", H, W, ty, tx, &g)) return -1;
  ADP_REQUIRE(N >= 1, "adp_clahe_apply: N must be at least 1");
  ADP_REQUIRE(src && lut && dst, "adp_clahe_apply: src, lut and dst must be non-null");
  ADP_REQUIRE(aligned16(lut), "adp_clahe_apply: lut must be 16-byte aligned");
  const float inv_th = 1.f / (float)g.th, inv_tw = 1.f / (float)g.tw;
  // the bands' first rows, by the kernel's own float32 expression (floor is monotone in y)
  Bands bands;
  int y = 0;
  for (int k = 0; k <= ty + 1; ++k) {
    bands.first[k] = y;
    if (k == ty + 1) break;
    while (y < H) {
      volatile float prod = (float)y * inv_th;   // rounded to float32 before the subtraction
      volatile float f = prod - 0.5f;
      if (k <= ty - 1 && (int)floorf(f) > k - 1) break;   // the last band takes whatever is left
      ++y;
    }
  }
  bands.first[ty + 1] = H;
  int nb = 0;
  for (int k = 0; k <= ty; ++k) {
    bands.block[k] = nb;
    nb += (bands.first[k + 1] - bands.first[k] + APPLY_ROWS - 1) / APPLY_ROWS;
  }
  bands.block[ty + 1] = nb;
  const long long blocks = (long long)N * nb;
  ADP_REQUIRE(blocks <= 0x7FFFFFFFll, "adp_clahe_apply: too many blocks (N * H too large for one launch)");
  const size_t lds = (size_t)tx * 256 * 2;
  const bool vec = W % 16 == 0 && aligned16(src) && aligned16(dst);
  if (vec)
    hipLaunchKernelGGL(clahe_apply_kernel<true>, dim3((unsigned)blocks), dim3(TPB), lds, (hipStream_t)st, H, W, ty, tx, inv_th,
                       inv_tw, nb, bands, src, src_f32 ? 1 : 0, lut, dst, dst_f32 ? 1 : 0);
  else
    hipLaunchKernelGGL(clahe_apply_kernel<false>, dim3((unsigned)blocks), dim3(TPB), lds, (hipStream_t)st, H, W, ty, tx, inv_th,
                       inv_tw, nb, bands, src, src_f32 ? 1 : 0, lut, dst, dst_f32 ? 1 : 0);
  return adp::check_launch("adp_clahe_apply");
}

extern "C" int adp_gray_stats(int N, int H, int W, const void* src, int src_f32, long long* sums, adp_stream_t st) {
  ADP_REQUIRE(src && sums, "adp_gray_stats: src and sums must be non-null");
  ADP_REQUIRE(N >= 1, "adp_gray_stats: N must be at least 1");
  ADP_REQUIRE(H >= 2 && W >= 2, "adp_gray_stats: H and W must be at least 2 (reflect-101 borders)");
  ADP_REQUIRE((long long)H * W <= 0x7FFFFFFFll - (long long)STAT_BLOCKS * TPB, "adp_gray_stats: H * W must be below 2^31");
  const int per = (int)std::min<long long>(((long long)H * W + TPB * 16 - 1) / (TPB * 16), STAT_BLOCKS);
  ADP_REQUIRE((long long)N * per <= 0x7FFFFFFFll, "adp_gray_stats: too many blocks");
  hipStream_t s = (hipStream_t)st;
  if (hipMemsetAsync(sums, 0, (size_t)N * 5 * sizeof(long long), s) != hipSuccess) {
    adp::set_error("adp_gray_stats: hipMemsetAsync failed");
    return -1;
  }
  hipLaunchKernelGGL(gray_stats_kernel, dim3((unsigned)(N * per)), dim3(TPB), 0, s, H, W, per, src, src_f32 ? 1 : 0,
                     reinterpret_cast<unsigned long long*>(sums));
  return adp::check_launch("adp_gray_stats");
}

extern "C" int adp_u8_stretch(int N, size_t n_px, const uint8_t* src, const unsigned* hist, double p_low, double p_high,
                              int mode, float* dst, adp_stream_t st) {
  ADP_REQUIRE(src && hist && dst, "adp_u8_stretch: src, hist and dst must be non-null");
  ADP_REQUIRE(N >= 1 && n_px >= 1, "adp_u8_stretch: N and n_px must be at least 1");
  ADP_REQUIRE(n_px <= 0xFFFFFFFFull, "adp_u8_stretch: n_px must fit the histogram's 32-bit counts");
  ADP_REQUIRE(p_low >= 0 && p_low <= 100 && p_high >= 0 && p_high <= 100, "adp_u8_stretch: percentiles must be in 0 .. 100");
  ADP_REQUIRE(mode == 0 || mode == 1, "adp_u8_stretch: mode must be 0 ((hi - lo) + 1e-3) or 1 (max(hi - lo, 1e-3))");
  const int per = (int)std::min<size_t>((n_px + TPB * 64 - 1) / (TPB * 64), 1024);
  ADP_REQUIRE((long long)N * per <= 0x7FFFFFFFll, "adp_u8_stretch: too many blocks");
  if (n_px % 16 == 0 && aligned16(src) && aligned16(dst))
    hipLaunchKernelGGL(u8_stretch_kernel<true>, dim3((unsigned)(N * per)), dim3(TPB), 0, (hipStream_t)st, n_px, per, src, hist,
                       p_low, p_high, mode, dst);
  else
    hipLaunchKernelGGL(u8_stretch_kernel<false>, dim3((unsigned)(N * per)), dim3(TPB), 0, (hipStream_t)st, n_px, per, src, hist,
                       p_low, p_high, mode, dst);
  return adp::check_launch("adp_u8_stretch");
}
