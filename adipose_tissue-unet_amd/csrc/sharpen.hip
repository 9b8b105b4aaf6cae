// The last step of the reference's gray-image preparation (pre-post-processing_tools/preprocess_small_MS_SIMs.py):
// sharpen_image :434-455 (--sharpen --sharpen-sigma 1.0 --sharpen-amount 0.5), an unsharp mask over a Gaussian blur.
// The definition is in sharpen.py's docstring; its numpy path is the same arithmetic, bit for bit: integer taps that
// sum to 2^24 (formed on the host; nothing here evaluates exp), exact integer sums S = sum_j q|j| sum_i q|i| v over the
// reflect-101 border, then three float64 operations, each rounded on its own (contraction is off for the whole file).
//
// Radius classes. A kernel is compiled for a radius R, so that its taps sit in scalar registers, every loop over them
// is unrolled and a thread keeps a sliding window in registers. A call with radius r runs the smallest class R >= r
// with the taps r + 1 .. R set to zero: a zero tap adds nothing to an integer sum, and the fold takes any index, so
// the result is that of radius r exactly. Classes 4, 8, 12, 16 are fused; 24, 32, 48, 64 take two launches.
//
// fused_kernel<R> (r <= ADP_SHARP_FUSED_RMAX): a block of 256 threads makes a TR x TC tile of the output.
//   1. stage: the (TR + 2R) x (TC + 2R) bytes around the tile into LDS, border indices folded here. A block whose halo
//      lies inside the image (the interior) takes a path without the fold, 4 pixels per load where the plane allows it
//      (W % 4 == 0 and an aligned base; R % 4 == 0 in every class).
//   2. row pass: R[sy][x] = q0 v[x] + sum_i qi (v[x - i] + v[x + i]) for the TR + 2R staged rows, 32-bit, into LDS; a
//      thread reads the 4 + 2R bytes of 4 adjacent sums as words. The two mirrored bytes are added before the multiply
//      (510 * 2^23 < 2^32: a 24-bit multiply-add, as 2 qi <= 2^24); R <= 255 * 2^24 < 2^32.
//   3. column pass: S = sum_j q|j| R[y + j][x], one 32 x 32 + 64 multiply-add per tap (two mirrored row sums need 33
//      bits, so they are not added first). A thread makes TR / 4 consecutive rows of one column from the TR / 4 + 2R row
//      sums it reads once; a wave's reads are 64 adjacent words.
//   4. finish in registers: D = v 2^48 - S, d = f64(D) 2^-48, t = f64(v) + amount d, out = trunc(clip(t, 0, 255)).
//   5. one byte (or float) store per pixel.
//   LDS: (TR + 2R)(TC + 2R) bytes + (TR + 2R) TC words: 13 KiB at R = 4, 22 KiB at R = 16, seven blocks and more of a
//   CU's 160 KiB. What bounds the resident blocks is the waves at R = 4 (eight blocks, 56 registers) and the registers
//   of the unrolled window at R = 16 (126: four blocks).
//
// Larger r (up to ADP_SHARP_RMAX) takes two launches through the caller's uint32 (N, H, W) plane of row sums:
// rows_kernel<R> stages TR rows x (TC + 2R) bytes and writes R (step 2); cols_kernel<R> loads (TR + 2R) x TC row sums,
// rows folded once through a table in LDS, into LDS (40 KiB at R = 64: three blocks per CU) and runs steps 3 to 5.
//
// adp_gray_blur writes S itself (int64) instead of the finish: it is what the tests hold to Python integers.
#include "common.h"
#include "../../include/adipose_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr int TR = ADP_SHARP_TILE_ROWS, TC = ADP_SHARP_TILE_COLS;
constexpr int F = ADP_SHARP_FUSED_RMAX, RMAX = ADP_SHARP_RMAX;
constexpr int PER = TR / (TPB / TC);   // consecutive rows of a column that one thread makes
static_assert(TC == 64 && TPB % TC == 0 && TR % (TPB / TC) == 0, "a wave is one row of the tile");
static_assert(F == 16 && RMAX == 64, "run() lists the radius classes");
static_assert((TR + 2 * F) * (TC + 2 * F) + (TR + 2 * F) * TC * 4 <= 80 * 1024, "two fused blocks per CU at least");
static_assert((TR + 2 * RMAX) * (TC + 1) * 4 <= 64 * 1024, "the column pass' row sums fit a block's LDS");
static_assert(TR + 2 * RMAX <= TPB, "a thread per staged row of the column pass");

struct Taps { uint32_t q[RMAX + 1]; };   // q0 .. qR of the class, by value: zero beyond the call's radius

ADP_DEV unsigned to_u8(float f) { return (unsigned)fminf(fmaxf(rintf(f), 0.f), 255.f); }

// BORDER_REFLECT_101 folded as often as needed; index 0 when the extent is 1
ADP_DEV int fold(int p, int n) {
  if (n == 1) return 0;
  long long q = p;
  const long long top = 2ll * (n - 1);
  while (q < 0 || q >= n) q = q < 0 ? -q : top - q;
  return (int)q;
}

ADP_DEV unsigned load_px(const void* src, int f32, size_t at) {
  return f32 ? to_u8(static_cast<const float*>(src)[at]) : (unsigned)static_cast<const uint8_t*>(src)[at];
}

struct Tile { int n, y0, x0; };
ADP_DEV Tile tile_of(int nty, int ntx) {
  int b = blockIdx.x;
  Tile t;
  t.x0 = (b % ntx) * TC; b /= ntx;
  t.y0 = (b % nty) * TR;
  t.n = b / nty;
  return t;
}

// step 1 without the fold, 4 pixels per load: rows x COLS pixels from `at` on (4-pixel aligned; W % 4 == 0) into
// st[.][SW]. (Issuing a thread's loads together, ahead of the first LDS write, was tried and changed no time.)
template <int COLS, int SW>
ADP_DEV void stage_quads(uint8_t (*st)[SW], const void* __restrict__ src, int f32, size_t at, int W, int rows) {
  static_assert(COLS % 4 == 0, "whole quads");
  constexpr int QPR = COLS / 4;
  for (int k = threadIdx.x; k < rows * QPR; k += TPB) {
    const int sy = k / QPR, sx = (k % QPR) * 4;
    const size_t p = at + (size_t)sy * W + sx;
    uint32_t v;
    if (f32) {
      const float4 q = *reinterpret_cast<const float4*>(static_cast<const float*>(src) + p);
      v = to_u8(q.x) | to_u8(q.y) << 8 | to_u8(q.z) << 16 | to_u8(q.w) << 24;
    } else {
      v = *reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(src) + p);
    }
    *reinterpret_cast<uint32_t*>(&st[sy][sx]) = v;
  }
}

// step 1 pixel by pixel: staged (sy, sx) is image (fold(ya + sy), fold(xa + sx)), or (ya + sy, xa + sx) without FOLD
template <int COLS, int SW, bool FOLD>
ADP_DEV void stage_pixels(uint8_t (*st)[SW], const void* __restrict__ src, int f32, size_t img, int H, int W, int ya, int xa,
                          int rows) {
  for (int k = threadIdx.x; k < rows * COLS; k += TPB) {
    const int sy = k / COLS, sx = k % COLS;
    const int gy = FOLD ? fold(ya + sy, H) : ya + sy, gx = FOLD ? fold(xa + sx, W) : xa + sx;
    st[sy][sx] = (uint8_t)load_px(src, f32, img + (size_t)gy * W + gx);
  }
}

// step 2 for 4 adjacent sums: w points at the staged byte of the first one's left-most tap (word aligned)
template <int R>
ADP_DEV uint4 row_quad(const uint32_t* w, const Taps& taps) {
  constexpr int ND = (4 + 2 * R) / 4;   // R % 4 == 0: the 4 + 2R bytes are whole words
  unsigned b[4 * ND];
#pragma unroll
  for (int d = 0; d < ND; ++d) {
    const uint32_t v = w[d];
#pragma unroll
    for (int j = 0; j < 4; ++j) b[4 * d + j] = (v >> (8 * j)) & 255u;
  }
  uint32_t o[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    uint32_t a = taps.q[0] * b[e + R];   // q0 may be 2^24 itself: a full multiply
#pragma unroll
    for (int i = 1; i <= R; ++i) a += __umul24(taps.q[i], b[e + R - i] + b[e + R + i]);
    o[e] = a;
  }
  return make_uint4(o[0], o[1], o[2], o[3]);
}

// step 3 for PER consecutive rows of column x: rows[k0 + k][x], k = 0 .. PER + 2R - 1, is the thread's window
template <int R>
ADP_DEV void column_sums(const uint32_t (*rows)[TC], int k0, int x, const Taps& taps, unsigned long long* S) {
#pragma unroll
  for (int e = 0; e < PER; ++e) S[e] = 0;
#pragma unroll
  for (int k = 0; k < PER + 2 * R; ++k) {   // row sum k enters output e with tap |k - e - R|
    const uint32_t v = rows[k0 + k][x];
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      const int j = k - e - R;
      if (j >= -R && j <= R) S[e] += (unsigned long long)taps.q[j < 0 ? -j : j] * v;
    }
  }
}

// steps 4 and 5 for one pixel
ADP_DEV void finish(unsigned long long S, unsigned px, double amount, size_t at, long long* __restrict__ S_out,
                    void* __restrict__ dst, int dst_f32) {
  if (S_out) {
    S_out[at] = (long long)S;
    return;
  }
  const long long D = ((long long)px << 48) - (long long)S;
  const double d = (double)D * 0x1p-48;
  const double ad = amount * d;
  const double tt = (double)px + ad;
  const unsigned o = (unsigned)fmin(fmax(tt, 0.0), 255.0);
  if (dst_f32) static_cast<float*>(dst)[at] = (float)o;
  else static_cast<uint8_t*>(dst)[at] = (uint8_t)o;
}

template <int R>
__global__ __launch_bounds__(TPB) void fused_kernel(int H, int W, int nty, int ntx, const void* __restrict__ src, int f32,
                                                    int quads, Taps taps, double amount, long long* __restrict__ S_out,
                                                    void* __restrict__ dst, int dst_f32) {
  static_assert(R % 4 == 0 && R >= 4 && R <= F, "a fused radius class");
  constexpr int SH = TR + 2 * R, SW = TC + 2 * R;   // the staged rows and bytes per row (whole words)
  __shared__ __attribute__((aligned(16))) uint8_t st[SH][SW];
  __shared__ __attribute__((aligned(16))) uint32_t rows[SH][TC];
  const Tile t = tile_of(nty, ntx);
  const size_t img = (size_t)t.n * H * W;
  const int ya = t.y0 - R, xa = t.x0 - R;
  if (ya >= 0 && ya + SH <= H && xa >= 0 && xa + SW <= W) {   // interior: no fold
    if (quads) stage_quads<SW, SW>(st, src, f32, img + (size_t)ya * W + xa, W, SH);
    else stage_pixels<SW, SW, false>(st, src, f32, img, H, W, ya, xa, SH);
  } else {
    stage_pixels<SW, SW, true>(st, src, f32, img, H, W, ya, xa, SH);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < SH * (TC / 4); k += TPB) {
    const int sy = k / (TC / 4), xq = (k % (TC / 4)) * 4;
    *reinterpret_cast<uint4*>(&rows[sy][xq]) = row_quad<R>(reinterpret_cast<const uint32_t*>(&st[sy][xq]), taps);
  }
  __syncthreads();
  const int x = threadIdx.x % TC, gx = t.x0 + x, oy0 = (threadIdx.x / TC) * PER;
  if (gx >= W) return;
  unsigned long long S[PER];
  column_sums<R>(rows, oy0, x, taps, S);
  const size_t at = img + (size_t)(t.y0 + oy0) * W + gx;
#pragma unroll
  for (int e = 0; e < PER; ++e)
    if (t.y0 + oy0 + e < H) finish(S[e], st[oy0 + e + R][x + R], amount, at + (size_t)e * W, S_out, dst, dst_f32);
}

template <int R>
__global__ __launch_bounds__(TPB) void rows_kernel(int H, int W, int nty, int ntx, const void* __restrict__ src, int f32,
                                                   int quads, Taps taps, uint32_t* __restrict__ rowbuf) {
  static_assert(R % 4 == 0 && R <= RMAX, "a radius class");
  constexpr int SW = TC + 2 * R;
  __shared__ __attribute__((aligned(16))) uint8_t st[TR][SW];
  const Tile t = tile_of(nty, ntx);
  const size_t img = (size_t)t.n * H * W;
  const int xa = t.x0 - R;
  const int th = min(TR, H - t.y0);   // the tile's rows inside the image
  if (xa >= 0 && xa + SW <= W) {
    if (quads) stage_quads<SW, SW>(st, src, f32, img + (size_t)t.y0 * W + xa, W, th);
    else stage_pixels<SW, SW, false>(st, src, f32, img, H, W, t.y0, xa, th);
  } else {
    stage_pixels<SW, SW, true>(st, src, f32, img, H, W, t.y0, xa, th);   // (rows t.y0 .. are inside: their fold is the identity)
  }
  __syncthreads();
  for (int k = threadIdx.x; k < th * (TC / 4); k += TPB) {
    const int sy = k / (TC / 4), xq = (k % (TC / 4)) * 4;
    const uint4 o = row_quad<R>(reinterpret_cast<const uint32_t*>(&st[sy][xq]), taps);
    uint32_t* out = rowbuf + img + (size_t)(t.y0 + sy) * W + t.x0 + xq;
    if (quads && t.x0 + xq + 3 < W) {
      *reinterpret_cast<uint4*>(out) = o;
    } else {
      const uint32_t v[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (t.x0 + xq + e < W) out[e] = v[e];
    }
  }
}

template <int R>
__global__ __launch_bounds__(TPB) void cols_kernel(int H, int W, int nty, int ntx, const void* __restrict__ src, int f32,
                                                   const uint32_t* __restrict__ rowbuf, Taps taps, double amount,
                                                   long long* __restrict__ S_out, void* __restrict__ dst, int dst_f32) {
  static_assert(R % 4 == 0 && R <= RMAX, "a radius class");
  constexpr int SH = TR + 2 * R;
  __shared__ uint32_t rows[SH][TC];
  __shared__ int gyof[SH];   // the folded image row of every staged row
  const Tile t = tile_of(nty, ntx);
  const size_t img = (size_t)t.n * H * W;
  const int x = threadIdx.x % TC, gx = t.x0 + x, ty = threadIdx.x / TC;
  if ((int)threadIdx.x < SH) gyof[threadIdx.x] = fold(t.y0 - R + (int)threadIdx.x, H);
  __syncthreads();
  if (gx < W) {   // (rows past the image's end fold to rows inside it: every staged row is loaded)
#pragma unroll 8
    for (int it = 0; it < SH / (TPB / TC); ++it) {
      const int sy = ty + it * (TPB / TC);
      rows[sy][x] = rowbuf[img + (size_t)gyof[sy] * W + gx];
    }
  }
  __syncthreads();
  const int oy0 = ty * PER;
  if (gx >= W || t.y0 + oy0 >= H) return;
  unsigned long long S[PER];
  column_sums<R>(rows, oy0, x, taps, S);
  const size_t at = img + (size_t)(t.y0 + oy0) * W + gx;
#pragma unroll
  for (int e = 0; e < PER; ++e)
    if (t.y0 + oy0 + e < H)
      finish(S[e], S_out ? 0u : load_px(src, f32, at + (size_t)e * W), amount, at + (size_t)e * W, S_out, dst, dst_f32);
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return !(pa + na <= pb || pb + nb <= pa);
}

// the checks both entry points share, then the launches; exactly one of S_out and dst is set
int run(const char* who, int N, int H, int W, const void* src, int src_f32, const uint32_t* taps, int r, double amount,
        uint32_t* rowbuf, long long* S_out, void* dst, int dst_f32, adp_stream_t st) {
  const std::string w(who);
  ADP_REQUIRE(N >= 0 && N <= 65535 && H >= 1 && W >= 1 && (long long)H * W <= 0x7FFFFFFFll,
              w + ": N must be in 0 .. 65535, H and W at least 1 and H * W below 2^31");
  ADP_REQUIRE(r >= 0 && r <= RMAX, w + ": r must be in 0 .. " + std::to_string(RMAX) + " (ADP_SHARP_RMAX)");
  ADP_REQUIRE(src && taps && (S_out || dst), w + ": src, taps and the output must be non-null");
  unsigned long long sum = taps[0];
  for (int i = 1; i <= r; ++i) sum += 2ull * taps[i];
  ADP_REQUIRE(sum == (1ull << 24), w + ": the taps must sum to 2^24 (q0 + 2 sum qi)");
  ADP_REQUIRE(std::isfinite(amount), w + ": amount must be finite");
  ADP_REQUIRE(r <= F || rowbuf, w + ": rowbuf must be non-null when r exceeds " + std::to_string(F) + " (ADP_SHARP_FUSED_RMAX)");
  const size_t px = (size_t)N * H * W, nsrc = px * (src_f32 ? 4 : 1);
  const void* out = S_out ? (const void*)S_out : dst;
  const size_t nout = px * (S_out ? 8 : dst_f32 ? 4 : 1);
  ADP_REQUIRE(!overlap(src, nsrc, out, nout), w + ": the output must not overlap src");
  ADP_REQUIRE(r <= F || (!overlap(rowbuf, px * 4, src, nsrc) && !overlap(rowbuf, px * 4, out, nout)),
              w + ": rowbuf must not overlap src or the output");
  const int nty = (H + TR - 1) / TR, ntx = (W + TC - 1) / TC;
  const long long blocks = (long long)N * nty * ntx;
  ADP_REQUIRE(blocks <= 0x7FFFFFFFll, w + ": too many blocks (N * H * W too large for one launch)");
  if (N == 0) return 0;
  Taps t = {};   // the class' taps beyond r stay zero
  for (int i = 0; i <= r; ++i) t.q[i] = taps[i];
  hipStream_t s = (hipStream_t)st;
  const dim3 grid((unsigned)blocks), block(TPB);
  const int f32 = src_f32 ? 1 : 0, o32 = dst_f32 ? 1 : 0;
  // 4 pixels per load (and 4 row sums per store): W % 4 == 0 and bases aligned to 4 pixels
  const int quads = W % 4 == 0 && ((uintptr_t)src & (src_f32 ? 15 : 3)) == 0 && (r <= F || ((uintptr_t)rowbuf & 15) == 0);
#define ADP_SHARP_FUSED(R_) \
  hipLaunchKernelGGL(fused_kernel<R_>, grid, block, 0, s, H, W, nty, ntx, src, f32, quads, t, amount, S_out, dst, o32)
#define ADP_SHARP_TWO(R_)                                                                                  \
  do {                                                                                                     \
    hipLaunchKernelGGL(rows_kernel<R_>, grid, block, 0, s, H, W, nty, ntx, src, f32, quads, t, rowbuf);    \
    hipLaunchKernelGGL(cols_kernel<R_>, grid, block, 0, s, H, W, nty, ntx, src, f32, rowbuf, t, amount, S_out, dst, o32); \
  } while (0)
  if (r <= 4) ADP_SHARP_FUSED(4);
  else if (r <= 8) ADP_SHARP_FUSED(8);
  else if (r <= 12) ADP_SHARP_FUSED(12);
  else if (r <= 16) ADP_SHARP_FUSED(16);
  else if (r <= 24) ADP_SHARP_TWO(24);
  else if (r <= 32) ADP_SHARP_TWO(32);
  else if (r <= 48) ADP_SHARP_TWO(48);
  else ADP_SHARP_TWO(64);
#undef ADP_SHARP_FUSED
#undef ADP_SHARP_TWO
  return adp::check_launch(who);
}

}  // namespace

extern "C" int adp_gray_blur(int N, int H, int W, const void* src, int src_f32, const uint32_t* taps, int r, uint32_t* rowbuf,
                             long long* S_out, adp_stream_t st) {
  ADP_REQUIRE(S_out, "adp_gray_blur: src, taps and the output must be non-null");
  return run("adp_gray_blur", N, H, W, src, src_f32, taps, r, 0.0, rowbuf, S_out, nullptr, 0, st);
}

extern "C" int adp_gray_sharpen(int N, int H, int W, const void* src, int src_f32, const uint32_t* taps, int r, double amount,
                                uint32_t* rowbuf, void* dst, int dst_f32, adp_stream_t st) {
  ADP_REQUIRE(dst, "adp_gray_sharpen: src, taps and the output must be non-null");
  return run("adp_gray_sharpen", N, H, W, src, src_f32, taps, r, amount, rowbuf, nullptr, dst, dst_f32, st);
}
