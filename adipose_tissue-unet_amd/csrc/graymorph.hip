// Gray-scale (flat) morphology of 8-bit planes and the background corrections built on it: the reference's
// remove_banding_morphological, correct_illumination_rolling_ball and correct_illumination_tophat
// (pre-post-processing_tools/preprocess_small_MS_SIMs.py:217-246, 293-326, 357-390). The definitions are in
// illumination.py; in short, for a footprint of kh rows of column extents [lo[a], hi[a]) in a box kw wide, anchor
// (cy, cx) = (kh / 2, kw / 2):
//   erode(M)(y, x)  = min over rows a, lo[a] <= b < hi[a], of M(y + a - cy, x + b - cx)
//   dilate(M)(y, x) = max over the same offsets (not the reflected ones)
// positions outside the image take no part (OpenCV's default morphology border); an empty footprint gives 255 / 0.
//
// gray_morph_kernel. The footprint is decomposed by rows: erode(y, x) = min over a of the horizontal window minimum of
// input row y + a - cy over the columns [x + lo[a] - cx, x + hi[a] - cx). A window minimum of any length L is two reads
// of a table of power-of-two windows, P_0 = the row, P_e[j] = min(P_{e-1}[j], P_{e-1}[j + 2^(e-1)]):
// min(P_e[s], P_e[s + L - 2^e]) with e = floor(log2 L). So a pixel costs 2 kh LDS byte reads whatever the footprint's width
// (the 301 ellipse: 602 reads for its 70 000 offsets).
//
// A block of 256 threads produces TR x TC = 64 x 256 pixels, one column per thread, the column's 64 running minima in
// registers. It streams the input rows y0 - cy .. y0 + TR - 1 + (kh - 1 - cy) that lie inside the image through LDS,
// GR = 4 at a time: the columns x0 - cx .. x0 + TC - 1 + (kw - 1 - cx) of each (identity outside the image: 255 for
// the minimum, 0 for the maximum) as level 0, then the levels 1 .. emax (emax = floor(log2 of the longest row)), built
// four pixels per lane and step: two dword reads, a byte alignment for the steps 1 and 2, and a byte-wise minimum made of
// two packed 16-bit minima. A staged row with its levels then serves every output row of the block it reaches (up to
// TR of them): row r is footprint row a = r - y + cy of output row y. The footprint's rows are a table in LDS, packed
// by the host and passed by value: the two byte offsets {e * 768 + lo, e * 768 + hi - 2^e} of a row's reads inside a
// staged row's levels. The window reads carry no branch: an empty row, and a row index up to 7 outside the footprint,
// has both offsets point into an eleventh pseudo-level that holds the identity, so the eight output rows of a group
// issue their table reads, then their sixteen window reads, together (with a branch per row the two LDS latencies of
// every row came one after the other: 2.6 ms for the 301 ellipse on 8 x 1024^2); a group of eight
// whose rows all lie outside the footprint is skipped by a uniform branch.
// LDS: 4 rows x 11 levels x 768 B + the table = 35.9 KB. Barriers: 2 + emax per four input rows.
// A staged row is read TC + kw - 1 wide for TC outputs and TR + kh - 1 rows are staged for TR output rows, each with its
// levels: the price of a footprint larger than the tile. Runs of rows with equal extents (rectangles) are not merged
// into a vertical pass; each row costs its two reads.
// No atomics and no communication between blocks: every output byte is written once by one thread.
//
// gray_bgsum_kernel: per-image sum of a u8 plane, 64-bit integer atomics (the value does not depend on block order).
// illum_finish_kernel: the element-wise end of the corrections; reads the sum from device memory, nothing synchronises
// with the host. Single float32 operations (contraction off), exact for these integer inputs.
#include "common.h"
#include "../../include/adipose_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr int KMAX = ADP_GMORPH_KMAX;
constexpr int TR = ADP_GMORPH_TILE_ROWS, TC = ADP_GMORPH_TILE_COLS;
constexpr int GR = 4;                        // input rows staged per round
constexpr int NLEV = 10;                     // levels 0 .. 9: 2^9 <= KMAX < 2^10
constexpr int SWD = (TC + KMAX - 1) / 4;     // dwords of a staged row at the widest footprint
constexpr int JG = 8, FPAD = JG - 1;         // output rows per branch-free group; table entries outside the footprint
constexpr unsigned IDENT_OFF = NLEV * SWD * 4;                       // byte offset of the identity pseudo-level
constexpr unsigned IDENT_ROW = IDENT_OFF | IDENT_OFF << 16;
static_assert(TR % JG == 0, "whole groups of output rows");
static_assert((NLEV + 1) * SWD * 4 < 65536, "the table packs two 16-bit byte offsets");
static_assert(TC <= SWD * 4, "the identity pseudo-level covers every thread's read");
static_assert(TC == TPB, "one thread per output column");
static_assert((TC + KMAX - 1) % 4 == 0, "a staged row is whole dwords");
static_assert((1 << (NLEV - 1)) <= KMAX && KMAX < (1 << NLEV), "levels cover the longest row");

// row a of the footprint: bits 0 .. 15 = e * SWD * 4 + lo, bits 16 .. 31 = e * SWD * 4 + hi - 2^e, e = floor(log2 len);
// IDENT_ROW for an empty row
struct Foot {
  int kh, kw, emax;
  unsigned row[KMAX];
};

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

template <bool MAXOP>
ADP_DEV unsigned op1(unsigned a, unsigned b) { return MAXOP ? max(a, b) : min(a, b); }

// byte-wise minimum / maximum of two dwords: the even and the odd bytes as pairs of 16-bit values
template <bool MAXOP>
ADP_DEV unsigned op4(unsigned a, unsigned b) {
  const unsigned ae = a & 0x00FF00FFu, ao = (a >> 8) & 0x00FF00FFu, be = b & 0x00FF00FFu, bo = (b >> 8) & 0x00FF00FFu;
  u16x2 xe = __builtin_bit_cast(u16x2, ae), ye = __builtin_bit_cast(u16x2, be);
  u16x2 xo = __builtin_bit_cast(u16x2, ao), yo = __builtin_bit_cast(u16x2, bo);
  const u16x2 re = MAXOP ? __builtin_elementwise_max(xe, ye) : __builtin_elementwise_min(xe, ye);
  const u16x2 ro = MAXOP ? __builtin_elementwise_max(xo, yo) : __builtin_elementwise_min(xo, yo);
  return __builtin_bit_cast(unsigned, re) | (__builtin_bit_cast(unsigned, ro) << 8);
}

// a pixel as the plane holds it: u8, or f32 rounded to nearest (half to even) and clamped to 0 .. 255
ADP_DEV unsigned load_px(const void* src, int f32, size_t i) {
  if (f32) return (unsigned)fminf(fmaxf(rintf(static_cast<const float*>(src)[i]), 0.f), 255.f);
  return static_cast<const uint8_t*>(src)[i];
}

template <bool MAXOP>
__global__ __launch_bounds__(TPB) void gray_morph_kernel(int H, int W, int ntr, int ntc, const void* __restrict__ src,
                                                         int src_f32, uint8_t* __restrict__ dst, Foot fp) {
  __shared__ unsigned lev[GR][NLEV + 1][SWD];
  __shared__ unsigned ftab[KMAX + 2 * FPAD];
  constexpr unsigned ID = MAXOP ? 0u : 255u, ID4 = MAXOP ? 0u : 0xFFFFFFFFu;
  const int tid = threadIdx.x;
  const int per = ntr * ntc;
  const int n = blockIdx.x / per, rem = blockIdx.x - n * per;
  const int y0 = (rem / ntc) * TR, x0 = (rem % ntc) * TC;
  const int kh = fp.kh, cy = kh / 2, cx = fp.kw / 2;
  const size_t img = (size_t)n * H * W;
  for (int i = tid; i < kh + 2 * FPAD; i += TPB) {
    const int a = i - FPAD;
    ftab[i] = a >= 0 && a < kh ? fp.row[a] : IDENT_ROW;
  }
  for (int i = tid; i < GR * (TC / 4); i += TPB) lev[i / (TC / 4)][NLEV][i % (TC / 4)] = ID4;
  unsigned acc[TR];
#pragma unroll
  for (int j = 0; j < TR; ++j) acc[j] = ID;
  const int r_lo = max(y0 - cy, 0), r_hi = min(y0 + TR - 1 + (kh - 1 - cy), H - 1);
  const int sw = TC + fp.kw - 1;        // staged pixels of a row: columns x0 - cx .. x0 - cx + sw - 1
  const int swd = (sw + 3) >> 2;        // <= SWD
  for (int r0 = r_lo; r0 <= r_hi; r0 += GR) {
    __syncthreads();   // the round before has been read (the first time: the table is written)
    for (int i = tid; i < GR * swd; i += TPB) {
      const int rr = i / swd, q = i - rr * swd;
      const int y = r0 + rr;
      unsigned v = ID4;
      if (y <= r_hi) {
        v = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int j = 4 * q + b, x = x0 - cx + j;
          unsigned p = ID;
          if (j < sw && x >= 0 && x < W) p = load_px(src, src_f32, img + (size_t)y * W + x);
          v |= p << (8 * b);
        }
      }
      lev[rr][0][q] = v;
    }
    __syncthreads();
    for (int e = 1; e <= fp.emax; ++e) {
      const int h = 1 << (e - 1);
      for (int i = tid; i < GR * swd; i += TPB) {
        const int rr = i / swd, q = i - rr * swd;
        const unsigned a = lev[rr][e - 1][q];
        unsigned b;
        if (h >= 4) {
          const int q2 = q + (h >> 2);
          b = q2 < swd ? lev[rr][e - 1][q2] : ID4;
        } else {
          const unsigned nx = q + 1 < swd ? lev[rr][e - 1][q + 1] : ID4;
          b = __builtin_amdgcn_alignbyte(nx, a, (unsigned)h);   // the bytes 4 q + h .. 4 q + h + 3
        }
        lev[rr][e][q] = op4<MAXOP>(a, b);
      }
      __syncthreads();
    }
    const int nrr = min(GR, r_hi - r0 + 1);
#pragma unroll 1
    for (int rr = 0; rr < nrr; ++rr) {
      const uint8_t* base = reinterpret_cast<const uint8_t*>(&lev[rr][0][0]) + tid;
      const int a0 = r0 + rr - y0 + cy;   // the footprint row of output row y0
#pragma unroll
      for (int jb = 0; jb < TR / JG; ++jb) {
        const int a_hi = a0 - jb * JG, a_lo = a_hi - (JG - 1);   // the footprint rows of output rows jb * JG .. + JG - 1
        if (a_hi < 0 || a_lo >= kh) continue;
        const unsigned* ft = &ftab[a_lo + FPAD];                 // a_lo >= -FPAD, a_hi <= kh - 1 + FPAD
        unsigned f[JG];
#pragma unroll
        for (int u = 0; u < JG; ++u) f[u] = ft[JG - 1 - u];      // row a_hi - u
#pragma unroll
        for (int u = 0; u < JG; ++u)
          acc[jb * JG + u] = op1<MAXOP>(acc[jb * JG + u], op1<MAXOP>(base[f[u] & 0xFFFFu], base[f[u] >> 16]));
      }
    }
  }
  const int x = x0 + tid;
  if (x < W) {
#pragma unroll
    for (int j = 0; j < TR; ++j)
      if (y0 + j < H) dst[img + (size_t)(y0 + j) * W + x] = (uint8_t)acc[j];
  }
}

// sums[n] += the block's part of image n (blockIdx.y); a thread's 32-bit partial sum holds: with n_px < 2^31 and the
// grid of ew_grid() it adds at most 4096 values of at most 255
__global__ __launch_bounds__(TPB) void gray_bgsum_kernel(size_t n_px, const uint8_t* __restrict__ src,
                                                         unsigned long long* __restrict__ sums) {
  __shared__ unsigned long long part[TPB / 64];
  const uint8_t* s = src + (size_t)blockIdx.y * n_px;
  unsigned t = 0;
  for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n_px; i += (size_t)gridDim.x * TPB) t += s[i];
  unsigned long long v = t;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long b = 0;
#pragma unroll
    for (int w = 0; w < TPB / 64; ++w) b += part[w];
    atomicAdd(&sums[blockIdx.y], b);
  }
}

ADP_DEV void store_px(void* dst, int f32, size_t i, float clipped) {   // clipped is in 0 .. 255: the cast truncates
  const unsigned u = (unsigned)clipped;
  if (f32) static_cast<float*>(dst)[i] = (float)u;
  else static_cast<uint8_t*>(dst)[i] = (uint8_t)u;
}

__global__ __launch_bounds__(TPB) void illum_finish_kernel(size_t n_px, const void* __restrict__ v, int v_f32,
                                                           const uint8_t* __restrict__ b, const long long* __restrict__ sums,
                                                           int mode, void* __restrict__ dst, int dst_f32) {
  const size_t img = (size_t)blockIdx.y * n_px;
  float mean32 = 0.f;
  if (mode == ADP_ILLUM_SUBTRACT_MEAN) mean32 = (float)((double)sums[blockIdx.y] / (double)n_px);
  for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n_px; i += (size_t)gridDim.x * TPB) {
    const int pv = (int)load_px(v, v_f32, img + i), pb = (int)b[img + i];
    float r;
    if (mode == ADP_ILLUM_SUBTRACT_MEAN) {
      r = (float)(pv - pb) + mean32;
    } else if (mode == ADP_ILLUM_TOPHAT_HALF) {
      r = (float)pv + (float)max(pv - pb, 0) * 0.5f;
    } else {   // ADP_ILLUM_DIFF
      r = (float)(pv - pb);
    }
    store_px(dst, dst_f32, img + i, fminf(fmaxf(r, 0.f), 255.f));
  }
}

bool shape_ok(const char* who, int N, int H, int W) {
  if (N < 0 || H < 1 || W < 1) {
    adp::set_error(std::string(who) + ": N must be at least 0, H and W at least 1");
    return false;
  }
  return true;
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return !(pa + na <= pb || pb + nb <= pa);
}

int ew_grid(size_t n_px) { return (int)std::min<size_t>((n_px + TPB * 16 - 1) / (TPB * 16), 2048); }

}  // namespace

extern "C" int adp_gray_morph(int N, int H, int W, const void* src, int src_f32, uint8_t* dst, int kh, int kw,
                              const int* row_lo, const int* row_hi, int op, adp_stream_t st) {
  if (!shape_ok("adp_gray_morph", N, H, W)) return -1;
  ADP_REQUIRE(kh >= 1 && kh <= KMAX && kw >= 1 && kw <= KMAX, "adp_gray_morph: kh and kw must be in 1 .. 513");
  ADP_REQUIRE(op == ADP_GMORPH_ERODE || op == ADP_GMORPH_DILATE, "adp_gray_morph: op must be ADP_GMORPH_ERODE or ADP_GMORPH_DILATE");
  ADP_REQUIRE(row_lo && row_hi, "adp_gray_morph: the footprint rows must be non-null");
  Foot fp{};
  fp.kh = kh;
  fp.kw = kw;
  for (int a = 0; a < kh; ++a) {
    ADP_REQUIRE(row_lo[a] >= 0 && row_hi[a] <= kw && row_lo[a] <= row_hi[a], "adp_gray_morph: bad footprint row");
    const int len = row_hi[a] - row_lo[a];
    fp.row[a] = IDENT_ROW;
    if (len == 0) continue;   // an empty row has no offsets
    int e = 0;
    while ((2 << e) <= len) ++e;
    fp.emax = std::max(fp.emax, e);
    const unsigned lvl = (unsigned)e * SWD * 4;
    fp.row[a] = (lvl + (unsigned)row_lo[a]) | (lvl + (unsigned)(row_hi[a] - (1 << e))) << 16;
  }
  ADP_REQUIRE(src && dst, "adp_gray_morph: src and dst must be non-null");
  const size_t px = (size_t)N * H * W;
  ADP_REQUIRE(!overlap(src, px * (src_f32 ? 4 : 1), dst, px), "adp_gray_morph: src must not overlap dst");
  if (N == 0) return 0;
  const int ntr = (H + TR - 1) / TR, ntc = (W + TC - 1) / TC;
  const long long blocks = (long long)N * ntr * ntc;
  ADP_REQUIRE(blocks <= 0x7FFFFFFFll, "adp_gray_morph: too many blocks (N * H * W too large for one launch)");
  if (op == ADP_GMORPH_DILATE)
    hipLaunchKernelGGL(gray_morph_kernel<true>, dim3((unsigned)blocks), dim3(TPB), 0, (hipStream_t)st, H, W, ntr, ntc, src,
                       src_f32 ? 1 : 0, dst, fp);
  else
    hipLaunchKernelGGL(gray_morph_kernel<false>, dim3((unsigned)blocks), dim3(TPB), 0, (hipStream_t)st, H, W, ntr, ntc, src,
                       src_f32 ? 1 : 0, dst, fp);
  return adp::check_launch("adp_gray_morph");
}

extern "C" int adp_gray_bgsum(int N, int H, int W, const uint8_t* src, long long* sums, adp_stream_t st) {
  if (!shape_ok("adp_gray_bgsum", N, H, W)) return -1;
  ADP_REQUIRE(src && sums, "adp_gray_bgsum: src and sums must be non-null");
  ADP_REQUIRE(N <= 65535, "adp_gray_bgsum: N must be at most 65535");
  ADP_REQUIRE((long long)H * W <= 0x7FFFFFFFll, "adp_gray_bgsum: H * W must be below 2^31");
  if (N == 0) return 0;
  hipStream_t s = (hipStream_t)st;
  if (hipMemsetAsync(sums, 0, (size_t)N * sizeof(long long), s) != hipSuccess) {
    adp::set_error("adp_gray_bgsum: hipMemsetAsync failed");
    return -1;
  }
  const size_t n_px = (size_t)H * W;
  hipLaunchKernelGGL(gray_bgsum_kernel, dim3(ew_grid(n_px), N), dim3(TPB), 0, s, n_px, src,
                     reinterpret_cast<unsigned long long*>(sums));
  return adp::check_launch("adp_gray_bgsum");
}

extern "C" int adp_illum_finish(int N, int H, int W, const void* v, int v_f32, const uint8_t* b, const long long* sums,
                                int mode, void* dst, int dst_f32, adp_stream_t st) {
  if (!shape_ok("adp_illum_finish", N, H, W)) return -1;
  ADP_REQUIRE(mode == ADP_ILLUM_SUBTRACT_MEAN || mode == ADP_ILLUM_TOPHAT_HALF || mode == ADP_ILLUM_DIFF,
              "adp_illum_finish: mode must be ADP_ILLUM_SUBTRACT_MEAN, ADP_ILLUM_TOPHAT_HALF or ADP_ILLUM_DIFF");
  ADP_REQUIRE(v && b && dst, "adp_illum_finish: v, b and dst must be non-null");
  ADP_REQUIRE(mode != ADP_ILLUM_SUBTRACT_MEAN || sums, "adp_illum_finish: ADP_ILLUM_SUBTRACT_MEAN needs sums");
  ADP_REQUIRE(N <= 65535, "adp_illum_finish: N must be at most 65535");
  const size_t px = (size_t)N * H * W;
  ADP_REQUIRE(!overlap(v, px * (v_f32 ? 4 : 1), dst, px * (dst_f32 ? 4 : 1)) && !overlap(b, px, dst, px * (dst_f32 ? 4 : 1)),
              "adp_illum_finish: dst must not overlap v or b");
  if (N == 0) return 0;
  const size_t n_px = (size_t)H * W;
  hipLaunchKernelGGL(illum_finish_kernel, dim3(ew_grid(n_px), N), dim3(TPB), 0, (hipStream_t)st, n_px, v, v_f32 ? 1 : 0, b,
                     sums, mode, dst, dst_f32 ? 1 : 0);
  return adp::check_launch("adp_illum_finish");
}
