// The statistical steps of the reference's gray-image preparation (pre-post-processing_tools/preprocess_small_MS_SIMs.py):
// remove_banding_column_normalize :249-286 (--banding-method column), normalize_zscore :92-114 and normalize_percentile
// :117-138 (--normalization-method). The definitions are in normalization.py's docstring; its numpy path is the same
// arithmetic, bit for bit: exact integer sums, histograms and minima / maxima first, then a few float64 operations, each
// rounded on its own (contraction is off for the whole file) in the order the definition writes them.
//
// adp_gray_colstats: the column reduction of a row-major plane, read once. A block takes a band of BAND_ROWS rows x
// BAND_COLS columns. VEC (uint8, W % 16 == 0, 16-byte aligned base): a lane reads 16 B = 16 adjacent columns of a row
// and keeps 16 x {S1, S2, min, max} in 32-bit registers (64 rows of 255^2 stay far below 2^32); 16 lanes cover the
// band's columns, so a wave holds 4 rows at a time and the block 16. The wave's 4 row groups are combined by two
// shuffles, the 4 waves through LDS, and thread x of the block then issues the band's contribution to column x: two
// 64-bit integer atomicAdd, one atomicMin, one atomicMax. Scalar (any W, unaligned planes, float32 planes): thread x
// walks down column x of the band (a row of the block is one coalesced read) and issues the same four atomics. Integer
// atomics are exact in any order, so the result does not depend on the grid or the run. The outputs are initialised by
// a small kernel of the same call ({0, 0} and {0xFFFFFFFF, 0}). Four atomics per column and band are what a large plane
// pays for (6144^2: 2.4 M of them, 32 us; a fifth of that with four times the rows, 19 us), while a small one needs the
// blocks (1024^2: 7.5 us with 64 rows, 10.4 with 256): a VEC block takes TALL_FACTOR bands of rows once the plane has
// more than TALL_BLOCKS blocks of one band. The scalar path keeps one band: its thread walks its column row by row and
// wants the blocks more than it minds the atomics (6144^2 float32: 129 us so, 163 us with 256 rows).
//
// adp_gray_colparams: one block per image: (cm, d) of every column, the exact totals of S1 and S2 (64-bit integers),
// and the minimum / maximum of the normalised value over the image, which the increasing map of a column takes at the
// column's minimum / maximum. min and max of doubles do not depend on the order either.
//
// adp_gray_colnorm: the element-wise end. VEC4 (W % 4 == 0, planes aligned to 4 pixels): a lane keeps 4 columns' (cm, d)
// in registers and walks down the band's rows, 4 pixels per load and store; one column per thread otherwise.
//
// adp_gray_normalize: every block rebuilds its image's 256-entry uint8 table in LDS from the image's histogram
// (adp_clahe_hist on a 1 x 1 grid): the z-score's mean and deviation from S1 = sum i h[i], S2 = sum i^2 h[i], or the two
// order statistics by the search of adp_u8_stretch, as a count over the bins; then 16 pixels per lane through the table.
#include "common.h"
#include "../../include/adipose_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256, WAVES = TPB / 64;
constexpr int BAND_ROWS = ADP_GNORM_BAND_ROWS, BAND_COLS = ADP_GNORM_BAND_COLS;
constexpr int TALL_BLOCKS = ADP_GNORM_TALL_BLOCKS, TALL_FACTOR = ADP_GNORM_TALL_FACTOR;
static_assert(BAND_COLS == TPB, "thread x of a block owns column x of its band");
static_assert(TALL_FACTOR * BAND_ROWS * 255ll * 255ll < 0xFFFFFFFFll, "a block's sums are 32-bit");

ADP_DEV unsigned to_u8(float f) { return (unsigned)fminf(fmaxf(rintf(f), 0.f), 255.f); }

// mean and population deviation of n values from their exact sums
ADP_DEV void stats(unsigned long long S1, unsigned long long S2, double n, double* mean, double* sd) {
  const double m = (double)S1 / n;
  const double ex2 = (double)S2 / n;
  const double mm = m * m;
  *mean = m;
  *sd = sqrt(fmax(ex2 - mm, 0.0));
}

ADP_DEV unsigned clip_trunc(double t) { return (unsigned)fmin(fmax(t, 0.0), 255.0); }

// ---------------------------------------------------------------- column statistics
__global__ __launch_bounds__(TPB) void colstats_init_kernel(size_t cols, unsigned long long* __restrict__ colsums,
                                                            unsigned* __restrict__ colminmax) {
  for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < cols; i += (size_t)gridDim.x * TPB) {
    colsums[2 * i] = 0ull;
    colsums[2 * i + 1] = 0ull;
    colminmax[2 * i] = 0xFFFFFFFFu;
    colminmax[2 * i + 1] = 0u;
  }
}

template <bool VEC>
__global__ __launch_bounds__(TPB) void colstats_kernel(int H, int W, int rows, int nbr, int nbc, const void* __restrict__ src,
                                                       int f32, unsigned long long* __restrict__ colsums,
                                                       unsigned* __restrict__ colminmax) {
  int b = blockIdx.x;
  const int bc = b % nbc; b /= nbc;
  const int br = b % nbr;
  const int n = b / nbr;
  const int y0 = br * rows, y1 = min(y0 + rows, H);   // rows = BAND_ROWS or TALL_FACTOR * BAND_ROWS
  const int x0 = bc * BAND_COLS;
  const size_t img = (size_t)n * H * W;
  const uint8_t* s8 = static_cast<const uint8_t*>(src) + img;
  const float* s32 = static_cast<const float*>(src) + img;
  unsigned s1 = 0, s2 = 0, mn = 0xFFFFFFFFu, mx = 0;   // of column x0 + threadIdx.x
  if (VEC) {
    __shared__ unsigned part[WAVES][4][BAND_COLS];
    const int cl = threadIdx.x & 15, rg = threadIdx.x >> 4;   // 16 columns x0 + 16 cl .., rows y0 + rg, + 16, ..
    const int xs = x0 + (cl << 4);
    unsigned a1[16], a2[16], lo[16], hi[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) { a1[j] = 0; a2[j] = 0; lo[j] = 0xFFFFFFFFu; hi[j] = 0; }
    if (xs < W) {   // W % 16 == 0: the whole chunk is inside
      for (int y = y0 + rg; y < y1; y += TPB / 16) {
        const uint4 q = *reinterpret_cast<const uint4*>(s8 + (size_t)y * W + xs);
        const unsigned d[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const unsigned v = (d[j >> 2] >> (8 * (j & 3))) & 255u;
          a1[j] += v;
          a2[j] += v * v;
          lo[j] = min(lo[j], v);
          hi[j] = max(hi[j], v);
        }
      }
    }
    // the wave's 4 row groups (lanes cl, cl + 16, cl + 32, cl + 48), then the 4 waves
#pragma unroll
    for (int j = 0; j < 16; ++j) {
#pragma unroll
      for (int o = 16; o < 64; o <<= 1) {
        a1[j] += __shfl_xor(a1[j], o, 64);
        a2[j] += __shfl_xor(a2[j], o, 64);
        lo[j] = min(lo[j], (unsigned)__shfl_xor(lo[j], o, 64));
        hi[j] = max(hi[j], (unsigned)__shfl_xor(hi[j], o, 64));
      }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane < 16) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        part[wave][0][(lane << 4) + j] = a1[j];
        part[wave][1][(lane << 4) + j] = a2[j];
        part[wave][2][(lane << 4) + j] = lo[j];
        part[wave][3][(lane << 4) + j] = hi[j];
      }
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      s1 += part[w][0][threadIdx.x];
      s2 += part[w][1][threadIdx.x];
      mn = min(mn, part[w][2][threadIdx.x]);
      mx = max(mx, part[w][3][threadIdx.x]);
    }
  } else {
    const int x = x0 + threadIdx.x;
    if (x < W) {
      for (int y = y0; y < y1; ++y) {
        const size_t at = (size_t)y * W + x;
        const unsigned v = f32 ? to_u8(s32[at]) : (unsigned)s8[at];
        s1 += v;
        s2 += v * v;
        mn = min(mn, v);
        mx = max(mx, v);
      }
    }
  }
  const int x = x0 + threadIdx.x;
  if (x < W) {   // the band has at least one row, so mn <= mx are values of the column
    const size_t c = (size_t)n * W + x;
    if (s1) atomicAdd(&colsums[2 * c], (unsigned long long)s1);
    if (s2) atomicAdd(&colsums[2 * c + 1], (unsigned long long)s2);
    atomicMin(&colminmax[2 * c], mn);
    if (mx) atomicMax(&colminmax[2 * c + 1], mx);
  }
}

// ---------------------------------------------------------------- column parameters
__global__ __launch_bounds__(TPB) void colparams_kernel(int H, int W, const unsigned long long* __restrict__ colsums,
                                                        const unsigned* __restrict__ colminmax, double* __restrict__ col,
                                                        double* __restrict__ glob) {
  __shared__ unsigned long long r1[WAVES], r2[WAVES];
  __shared__ double rlo[WAVES], rhi[WAVES];
  const int n = blockIdx.x;
  const size_t base = (size_t)n * W;
  unsigned long long t1 = 0, t2 = 0;
  double lo = INFINITY, hi = -INFINITY;
  for (int x = threadIdx.x; x < W; x += TPB) {
    const unsigned long long S1 = colsums[2 * (base + x)], S2 = colsums[2 * (base + x) + 1];
    double cm, cs;
    stats(S1, S2, (double)H, &cm, &cs);
    const double d = cs + 1e-10;
    col[2 * (base + x)] = cm;
    col[2 * (base + x) + 1] = d;
    t1 += S1;
    t2 += S2;
    lo = fmin(lo, ((double)colminmax[2 * (base + x)] - cm) / d);
    hi = fmax(hi, ((double)colminmax[2 * (base + x) + 1] - cm) / d);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    t1 += __shfl_xor(t1, o, 64);
    t2 += __shfl_xor(t2, o, 64);
    lo = fmin(lo, __shfl_xor(lo, o, 64));
    hi = fmax(hi, __shfl_xor(hi, o, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    r1[w] = t1; r2[w] = t2; rlo[w] = lo; rhi[w] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < WAVES; ++w) {
      t1 += r1[w];
      t2 += r2[w];
      lo = fmin(lo, rlo[w]);
      hi = fmax(hi, rhi[w]);
    }
    double gm, gs;
    stats(t1, t2, (double)((long long)H * W), &gm, &gs);
    glob[4 * (size_t)n] = gm;
    glob[4 * (size_t)n + 1] = gs;
    glob[4 * (size_t)n + 2] = lo;
    glob[4 * (size_t)n + 3] = hi;
  }
}

// ---------------------------------------------------------------- column normalisation
ADP_DEV unsigned colnorm_px(unsigned v, double cm, double d, bool preserve, double a, double b) {
  double t = ((double)v - cm) / d;
  if (preserve) {
    t = t * a;   // gs
    t = t + b;   // gm
  } else {
    t = (t - a) / b;   // lo, (hi - lo) + 1e-10
    t = t * 255.0;
  }
  return clip_trunc(t);
}

// PER columns per thread: 4 (W % 4 == 0, planes aligned to 4 pixels) or 1
template <int PER>
__global__ __launch_bounds__(TPB) void colnorm_kernel(int H, int W, int nbr, int nbc, const void* __restrict__ src, int f32,
                                                      const double* __restrict__ col, const double* __restrict__ glob,
                                                      int preserve, void* __restrict__ dst, int dst_f32) {
  constexpr int TPR = BAND_COLS / PER, STEP = TPB / TPR;
  int b = blockIdx.x;
  const int bc = b % nbc; b /= nbc;
  const int br = b % nbr;
  const int n = b / nbr;
  const int y0 = br * BAND_ROWS, y1 = min(y0 + BAND_ROWS, H);
  const int x = bc * BAND_COLS + (threadIdx.x % TPR) * PER;
  if (x >= W) return;   // W % PER == 0: the thread's columns are all inside or all outside
  const size_t img = (size_t)n * H * W;
  const uint8_t* s8 = static_cast<const uint8_t*>(src) + img;
  const float* s32 = static_cast<const float*>(src) + img;
  uint8_t* d8 = static_cast<uint8_t*>(dst) + img;
  float* d32 = static_cast<float*>(dst) + img;
  double cm[PER], d[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    cm[j] = col[2 * ((size_t)n * W + x + j)];
    d[j] = col[2 * ((size_t)n * W + x + j) + 1];
  }
  const double gm = glob[4 * (size_t)n], gs = glob[4 * (size_t)n + 1], lo = glob[4 * (size_t)n + 2], hi = glob[4 * (size_t)n + 3];
  const double a = preserve ? gs : lo, bb = preserve ? gm : (hi - lo) + 1e-10;
  for (int y = y0 + threadIdx.x / TPR; y < y1; y += STEP) {
    const size_t at = (size_t)y * W + x;
    unsigned v[PER], o[PER];
    if (PER == 4) {
      if (f32) {
        const float4 q = *reinterpret_cast<const float4*>(s32 + at);
        v[0] = to_u8(q.x); v[1 % PER] = to_u8(q.y); v[2 % PER] = to_u8(q.z); v[3 % PER] = to_u8(q.w);
      } else {
        const unsigned q = *reinterpret_cast<const unsigned*>(s8 + at);
#pragma unroll
        for (int j = 0; j < PER; ++j) v[j] = (q >> (8 * j)) & 255u;
      }
    } else {
      v[0] = f32 ? to_u8(s32[at]) : (unsigned)s8[at];
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) o[j] = colnorm_px(v[j], cm[j], d[j], preserve != 0, a, bb);
    if (PER == 4) {
      if (dst_f32) *reinterpret_cast<float4*>(d32 + at) = make_float4((float)o[0], (float)o[1 % PER], (float)o[2 % PER], (float)o[3 % PER]);
      else *reinterpret_cast<unsigned*>(d8 + at) = o[0] | o[1 % PER] << 8 | o[2 % PER] << 16 | o[3 % PER] << 24;
    } else {
      if (dst_f32) d32[at] = (float)o[0];
      else d8[at] = (uint8_t)o[0];
    }
  }
}

// ---------------------------------------------------------------- z-score / percentile stretch
// VEC: n_px % 16 == 0 and aligned planes
template <bool VEC>
__global__ __launch_bounds__(TPB) void normalize_kernel(size_t n_px, int per_image, const void* __restrict__ src, int f32,
                                                        const unsigned* __restrict__ hist, int method, double p_low,
                                                        double p_high, void* __restrict__ dst, int dst_f32) {
  __shared__ unsigned long long cum[256], m1[256], m2[256];
  __shared__ double par[2];   // (mean, std) or (lo, hi)
  __shared__ unsigned table[256];
  const int n = blockIdx.x / per_image, rem = blockIdx.x - n * per_image;
  const unsigned i = threadIdx.x;
  {
    const unsigned long long h = hist[(size_t)n * 256 + i];
    cum[i] = h;
    m1[i] = h * i;
    m2[i] = h * i * i;
  }
  __syncthreads();
  if (method == ADP_GNORM_ZSCORE) {
    for (int o = 128; o > 0; o >>= 1) {   // integer sums: any order
      if ((int)i < o) { cum[i] += cum[i + o]; m1[i] += m1[i + o]; m2[i] += m2[i + o]; }
      __syncthreads();
    }
    if (i == 0) {
      const unsigned long long cnt = cum[0] ? cum[0] : 1ull;   // (an all-zero histogram: nothing reads the table)
      stats(m1[0], m2[0], (double)cnt, &par[0], &par[1]);
    }
    __syncthreads();
    const double mean = par[0], sd = par[1];
    double t = ((double)i - mean) / (sd + 1e-10);
    t = t + 3.0;
    t = t / 6.0;
    t = t * 255.0;
    table[i] = clip_trunc(t);
  } else {
    for (int o = 1; o < 256; o <<= 1) {   // inclusive scan
      const unsigned long long add = (int)i >= o ? cum[i - o] : 0ull;
      __syncthreads();
      cum[i] += add;
      __syncthreads();
    }
    const unsigned long long cnt = cum[255] ? cum[255] : 1ull, mine = cum[i];
#pragma unroll
    for (int e = 0; e < 2; ++e) {   // every thread forms both positions; the search is a count over the 256 bins
      const double q = (e ? p_high : p_low) / 100.0;
      const double pos = (double)(cnt - 1) * q;
      const double kf = floor(pos), t = pos - kf;
      const unsigned long long k = (unsigned long long)kf, k1 = k + 1 < cnt ? k + 1 : cnt - 1;
      // the k-th and (k + 1)-th smallest values: the first bins whose running count passes k, k1; the running count
      // does not fall, so that bin's index is the number of bins that have not passed it (adp_u8_stretch's search)
      const int a = min(__syncthreads_count(mine <= k), 255), b = min(__syncthreads_count(mine <= k1), 255);
      const double d = (double)b - (double)a;
      if (i == 0) par[e] = t >= 0.5 ? (double)b - d * (1.0 - t) : (double)a + d * t;   // numpy's _lerp
    }
    __syncthreads();
    const double lo = par[0], hi = par[1];
    const double scale = fmax(hi - lo, 1e-3);
    const double t = fmin(fmax(((double)i - lo) / scale, 0.0), 1.0);
    table[i] = (unsigned)(t * 255.0);
  }
  __syncthreads();
  const size_t img = (size_t)n * n_px;
  const uint8_t* s8 = static_cast<const uint8_t*>(src) + img;
  const float* s32 = static_cast<const float*>(src) + img;
  uint8_t* d8 = static_cast<uint8_t*>(dst) + img;
  float* d32 = static_cast<float*>(dst) + img;
  if (VEC) {
    const size_t chunks = n_px >> 4;
    for (size_t c = (size_t)rem * TPB + threadIdx.x; c < chunks; c += (size_t)per_image * TPB) {
      unsigned o[16];
      if (f32) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float4 q = reinterpret_cast<const float4*>(s32)[4 * c + j];
          o[4 * j] = table[to_u8(q.x)]; o[4 * j + 1] = table[to_u8(q.y)];
          o[4 * j + 2] = table[to_u8(q.z)]; o[4 * j + 3] = table[to_u8(q.w)];
        }
      } else {
        const uint4 q = reinterpret_cast<const uint4*>(s8)[c];
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 16; ++j) o[j] = table[(w[j >> 2] >> (8 * (j & 3))) & 255u];
      }
      if (dst_f32) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          reinterpret_cast<float4*>(d32)[4 * c + j] = make_float4((float)o[4 * j], (float)o[4 * j + 1], (float)o[4 * j + 2], (float)o[4 * j + 3]);
      } else {
        unsigned w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = o[4 * j] | o[4 * j + 1] << 8 | o[4 * j + 2] << 16 | o[4 * j + 3] << 24;
        reinterpret_cast<uint4*>(d8)[c] = make_uint4(w[0], w[1], w[2], w[3]);
      }
    }
  } else {
    for (size_t p = (size_t)rem * TPB + threadIdx.x; p < n_px; p += (size_t)per_image * TPB) {
      const unsigned o = table[f32 ? to_u8(s32[p]) : (unsigned)s8[p]];
      if (dst_f32) d32[p] = (float)o;
      else d8[p] = (uint8_t)o;
    }
  }
}

bool shape_ok(const char* who, int N, int H, int W) {
  if (N < 0 || N > 65535 || H < 1 || W < 1 || (long long)H * W > 0x7FFFFFFFll) {
    adp::set_error(std::string(who) + ": N must be in 0 .. 65535, H and W at least 1 and H * W below 2^31");
    return false;
  }
  return true;
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return !(pa + na <= pb || pb + nb <= pa);
}

bool aligned(const void* p, uintptr_t to) { return ((uintptr_t)p & (to - 1)) == 0; }

// the bands of an (N, H, W) plane as a 1-D grid, or false with the error set
bool bands(const char* who, int N, int H, int W, int* nbr, int* nbc, unsigned* blocks) {
  *nbr = (H + BAND_ROWS - 1) / BAND_ROWS;
  *nbc = (W + BAND_COLS - 1) / BAND_COLS;
  const long long nb = (long long)N * *nbr * *nbc;
  if (nb > 0x7FFFFFFFll) {
    adp::set_error(std::string(who) + ": too many blocks (N * H * W too large for one launch)");
    return false;
  }
  *blocks = (unsigned)nb;
  return true;
}

}  // namespace

extern "C" int adp_gray_colstats(int N, int H, int W, const void* src, int src_f32, long long* colsums, uint32_t* colminmax,
                                 adp_stream_t st) {
  if (!shape_ok("adp_gray_colstats", N, H, W)) return -1;
  ADP_REQUIRE(src && colsums && colminmax, "adp_gray_colstats: src, colsums and colminmax must be non-null");
  const size_t px = (size_t)N * H * W * (src_f32 ? 4 : 1), cols = (size_t)N * W;
  ADP_REQUIRE(!overlap(src, px, colsums, cols * 16) && !overlap(src, px, colminmax, cols * 8) &&
                  !overlap(colsums, cols * 16, colminmax, cols * 8),
              "adp_gray_colstats: the outputs must not overlap src or each other");
  int nbr, nbc;
  unsigned blocks;
  if (!bands("adp_gray_colstats", N, H, W, &nbr, &nbc, &blocks)) return -1;
  if (N == 0) return 0;
  const bool vec = !src_f32 && W % 16 == 0 && aligned(src, 16);
  int rows = BAND_ROWS;
  if (vec && blocks > (unsigned)TALL_BLOCKS) {   // fewer, taller blocks: a quarter of the atomics
    rows = TALL_FACTOR * BAND_ROWS;
    nbr = (H + rows - 1) / rows;
    blocks = (unsigned)N * nbr * nbc;
  }
  hipStream_t s = (hipStream_t)st;
  unsigned long long* sums = reinterpret_cast<unsigned long long*>(colsums);
  hipLaunchKernelGGL(colstats_init_kernel, dim3((unsigned)std::min<size_t>((cols + TPB - 1) / TPB, 1024)), dim3(TPB), 0, s, cols,
                     sums, colminmax);
  if (vec)
    hipLaunchKernelGGL(colstats_kernel<true>, dim3(blocks), dim3(TPB), 0, s, H, W, rows, nbr, nbc, src, 0, sums, colminmax);
  else
    hipLaunchKernelGGL(colstats_kernel<false>, dim3(blocks), dim3(TPB), 0, s, H, W, rows, nbr, nbc, src, src_f32 ? 1 : 0, sums,
                       colminmax);
  return adp::check_launch("adp_gray_colstats");
}

extern "C" int adp_gray_colparams(int N, int H, int W, const long long* colsums, const uint32_t* colminmax, double* col,
                                  double* glob, adp_stream_t st) {
  if (!shape_ok("adp_gray_colparams", N, H, W)) return -1;
  ADP_REQUIRE(colsums && colminmax && col && glob, "adp_gray_colparams: colsums, colminmax, col and glob must be non-null");
  const size_t cols = (size_t)N * W;
  ADP_REQUIRE(!overlap(colsums, cols * 16, col, cols * 16) && !overlap(colminmax, cols * 8, col, cols * 16) &&
                  !overlap(colsums, cols * 16, glob, (size_t)N * 32) && !overlap(colminmax, cols * 8, glob, (size_t)N * 32) &&
                  !overlap(col, cols * 16, glob, (size_t)N * 32),
              "adp_gray_colparams: the outputs must not overlap the inputs or each other");
  if (N == 0) return 0;
  hipLaunchKernelGGL(colparams_kernel, dim3((unsigned)N), dim3(TPB), 0, (hipStream_t)st, H, W,
                     reinterpret_cast<const unsigned long long*>(colsums), colminmax, col, glob);
  return adp::check_launch("adp_gray_colparams");
}

extern "C" int adp_gray_colnorm(int N, int H, int W, const void* src, int src_f32, const double* col, const double* glob,
                                int preserve_global, void* dst, int dst_f32, adp_stream_t st) {
  if (!shape_ok("adp_gray_colnorm", N, H, W)) return -1;
  ADP_REQUIRE(src && col && glob && dst, "adp_gray_colnorm: src, col, glob and dst must be non-null");
  const size_t px = (size_t)N * H * W, nsrc = px * (src_f32 ? 4 : 1), ndst = px * (dst_f32 ? 4 : 1);
  ADP_REQUIRE(!overlap(src, nsrc, dst, ndst) && !overlap(col, (size_t)N * W * 16, dst, ndst) &&
                  !overlap(glob, (size_t)N * 32, dst, ndst),
              "adp_gray_colnorm: dst must not overlap src, col or glob");
  int nbr, nbc;
  unsigned blocks;
  if (!bands("adp_gray_colnorm", N, H, W, &nbr, &nbc, &blocks)) return -1;
  if (N == 0) return 0;
  if (W % 4 == 0 && aligned(src, src_f32 ? 16 : 4) && aligned(dst, dst_f32 ? 16 : 4))
    hipLaunchKernelGGL(colnorm_kernel<4>, dim3(blocks), dim3(TPB), 0, (hipStream_t)st, H, W, nbr, nbc, src, src_f32 ? 1 : 0, col,
                       glob, preserve_global ? 1 : 0, dst, dst_f32 ? 1 : 0);
  else
    hipLaunchKernelGGL(colnorm_kernel<1>, dim3(blocks), dim3(TPB), 0, (hipStream_t)st, H, W, nbr, nbc, src, src_f32 ? 1 : 0, col,
                       glob, preserve_global ? 1 : 0, dst, dst_f32 ? 1 : 0);
  return adp::check_launch("adp_gray_colnorm");
}

extern "C" int adp_gray_normalize(int N, size_t n_px, const void* src, int src_f32, const uint32_t* hist, int method,
                                  double p_low, double p_high, void* dst, int dst_f32, adp_stream_t st) {
  ADP_REQUIRE(N >= 0 && N <= 65535, "adp_gray_normalize: N must be in 0 .. 65535");
  ADP_REQUIRE(n_px >= 1 && n_px <= 0x7FFFFFFFull, "adp_gray_normalize: n_px must be at least 1 and below 2^31");
  ADP_REQUIRE(method == ADP_GNORM_ZSCORE || method == ADP_GNORM_PERCENTILE,
              "adp_gray_normalize: method must be ADP_GNORM_ZSCORE or ADP_GNORM_PERCENTILE");
  ADP_REQUIRE(method != ADP_GNORM_PERCENTILE || (p_low >= 0 && p_low <= p_high && p_high <= 100),
              "adp_gray_normalize: percentiles need 0 <= p_low <= p_high <= 100");
  ADP_REQUIRE(src && hist && dst, "adp_gray_normalize: src, hist and dst must be non-null");
  const size_t px = (size_t)N * n_px, nsrc = px * (src_f32 ? 4 : 1), ndst = px * (dst_f32 ? 4 : 1);
  ADP_REQUIRE(!overlap(src, nsrc, dst, ndst) && !overlap(hist, (size_t)N * 1024, dst, ndst),
              "adp_gray_normalize: dst must not overlap src or hist");
  if (N == 0) return 0;
  const int per = (int)std::min<size_t>((n_px + TPB * 64 - 1) / (TPB * 64), 1024);
  if (n_px % 16 == 0 && aligned(src, 16) && aligned(dst, 16))
    hipLaunchKernelGGL(normalize_kernel<true>, dim3((unsigned)(N * per)), dim3(TPB), 0, (hipStream_t)st, n_px, per, src,
                       src_f32 ? 1 : 0, hist, method, p_low, p_high, dst, dst_f32 ? 1 : 0);
  else
    hipLaunchKernelGGL(normalize_kernel<false>, dim3((unsigned)(N * per)), dim3(TPB), 0, (hipStream_t)st, n_px, per, src,
                       src_f32 ? 1 : 0, hist, method, p_low, p_high, dst, dst_f32 ? 1 : 0);
  return adp::check_launch("adp_gray_normalize");
}
