// Pillow-exact resampling of 8-bit images (pre-post-processing_tools/ECM_scaling.py:175 and :184: every ECM image is
// brought to its Pseudocolored counterpart's size with PIL.Image.resize(size, Image.LANCZOS)). The definition is in
// resample.py's docstring; its numpy path is the same arithmetic, bit for bit. The host makes the tables in float64
// (nothing here evaluates sin); a pass is out = clamp((2^21 + sum_j k_j v[lo + j]) >> 22, 0, 255) in int32, the
// horizontal pass first, through a uint8 image, then the vertical one. A pass whose extent does not change is skipped.
//
// Images are (N, H, W, C) uint8, C in 1 .. 4, channels interleaved: a row is W * C bytes, and the vertical pass does not
// see channels at all. The tables of an axis with m outputs are bounds [m][2] = {lo, cnt} and taps [m][ksize] int32; the
// entry point checks them on the host (0 <= lo, 0 <= cnt <= ksize, lo + cnt <= n, lo and lo + cnt never descending, the
// int32 bound of a sum) and copies them into the stream's workspace, so no kernel reads outside its image.
//
// General form: two launches through the caller's intermediate (N, H, Wo, C).
//   hpass_kernel: a block makes a run of TC outputs of up to RH rows. The outputs' taps overlap (at a down-scale
//     neighbours share most of them), so the run's input span, lo of its first output to lo + cnt of its last, is staged
//     in LDS once, RH rows of it; RH is what ADP_RESAMPLE_LDS_BYTES holds of the widest span of the call. A span wider
//     than that budget (the box filter far down) is read from global memory instead.
//   vpass_kernel: a thread owns 4 adjacent bytes of a row (1 where the row bytes or a base are not a multiple of 4) and
//     walks TR output rows; a wave reads 256 adjacent bytes per tap, and the bounds and taps of a row are wave-uniform.
// Fused form: one launch, used when both extents change and the tile fits. A block makes a TR x TC output tile: the
//   horizontal pass of the input rows the tile needs (lo of its first row to lo + cnt of its last) goes into LDS as
//   uint8, TC * C bytes a row, and the vertical pass runs out of LDS. The intermediate never reaches memory; the image is
//   read about once (the taps of neighbouring outputs come from the vector cache) and written once. It fits when the most
//   rows any tile needs, times TC * C, is at most ADP_RESAMPLE_LDS_BYTES = 32 KiB: five blocks of a CU's 160 KiB, 20 of
//   its 32 waves. Neighbouring tiles of a column repeat the horizontal pass of the rows they share: 2 support / TR of
//   it, 19 % for Lanczos.
// Library option resample_fused: -1 (default) and 1 take the fused form whenever it fits, 0 never.
//
// Nearest: gather_kernel, through the two index tables.
#include "common.h"
#include "workspace.h"
#include "../../include/adipose_hip.h"

#include <cstdlib>

namespace {

constexpr int TPB = 256;
constexpr int TR = ADP_RESAMPLE_TILE_ROWS, TC = ADP_RESAMPLE_TILE_COLS;
constexpr int KMAX = ADP_RESAMPLE_KMAX, LDS_BYTES = ADP_RESAMPLE_LDS_BYTES;
constexpr int BITS = 22;
static_assert(LDS_BYTES <= 64 * 1024 && TR * TC * 4 <= LDS_BYTES, "an up-scale's tile (about TR rows) fits at C = 4");
static_assert(KMAX >= 193, "Lanczos down to 1 / 32");

// the tables of one axis on the device: bounds [m][2] {lo, cnt}, taps [m][ks]
struct Axis {
  const int* b;
  const int* k;
  int ks;
};

// clamp(acc >> 22, 0, 255), clamped before the shift (the same value: 2^30 - 1 >> 22 = 255). Written the other way
// round, two results packed into a word become one v_ashr_pk_u8_i32, whose upper 16 bits the compiler takes for zero
// and the MI355X does not clear: bytes 2 and 3 of the word then came out with stray bits set.
ADP_DEV uint32_t sat8(int acc) { return (uint32_t)(min(max(acc, 0), 0x3FFFFFFF) >> BITS); }

// one output: p[0], p[step], .. are the cnt input bytes under the taps kk
ADP_DEV uint8_t conv(const uint8_t* p, int step, const int* __restrict__ kk, int cnt) {
  int acc = 1 << (BITS - 1);
  for (int j = 0; j < cnt; ++j) acc += kk[j] * (int)p[(size_t)j * step];
  return (uint8_t)sat8(acc);
}

// four adjacent outputs of a vertical pass: the words p, p + step, .. (4-byte aligned) hold the input bytes of all four
ADP_DEV uint32_t conv4(const uint8_t* p, size_t step, const int* __restrict__ kk, int cnt) {
  int a0 = 1 << (BITS - 1), a1 = a0, a2 = a0, a3 = a0;
  for (int j = 0; j < cnt; ++j) {
    const uint32_t v = *reinterpret_cast<const uint32_t*>(p + j * step);
    const int q = kk[j];
    a0 += q * (int)(v & 255u);
    a1 += q * (int)((v >> 8) & 255u);
    a2 += q * (int)((v >> 16) & 255u);
    a3 += q * (int)(v >> 24);
  }
  return sat8(a0) | sat8(a1) << 8 | sat8(a2) << 16 | sat8(a3) << 24;
}

// blockIdx.x -> (image, row tile, column tile)
struct Tile { int n, rt, ct; };
ADP_DEV Tile tile_of(int nrt, int nct) {
  int b = blockIdx.x;
  Tile t;
  t.ct = b % nct; b /= nct;
  t.rt = b % nrt;
  t.n = b / nrt;
  return t;
}

// dst (N, H, Wo, C) = the horizontal pass of src (N, H, W, C). Dynamic LDS: RH * spanB bytes when staged (spanB = the
// widest run's span in bytes), none otherwise
__global__ __launch_bounds__(TPB) void hpass_kernel(int H, int W, int C, int Wo, int RH, int spanB, int staged, int nrt,
                                                    int nct, const uint8_t* __restrict__ src, Axis ax,
                                                    uint8_t* __restrict__ dst) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const Tile t = tile_of(nrt, nct);
  const int x0 = t.ct * TC, x1 = min(x0 + TC, Wo), y0 = t.rt * RH, rows = min(RH, H - y0);
  const int s0 = ax.b[2 * x0];                                        // the run's span: input columns s0 .. s1 - 1
  const int s1 = ax.b[2 * (x1 - 1)] + ax.b[2 * (x1 - 1) + 1];
  const int span = (s1 - s0) * C;                                     // at most spanB when staged
  const size_t row0 = (size_t)t.n * H + y0;
  if (staged) {
    for (int k = threadIdx.x; k < rows * span; k += TPB) {
      const int r = k / span, e = k - r * span;
      lds[r * spanB + e] = src[((row0 + r) * W + s0) * C + e];
    }
    __syncthreads();
  }
  const int wC = (x1 - x0) * C;
  for (int k = threadIdx.x; k < rows * wC; k += TPB) {
    const int r = k / wC, e = k - r * wC, xe = e / C, c = e - xe * C, x = x0 + xe;
    const int lo = ax.b[2 * x], cnt = ax.b[2 * x + 1];
    const uint8_t* p = staged ? lds + r * spanB + (lo - s0) * C + c : src + ((row0 + r) * W + lo) * C + c;
    dst[((row0 + r) * Wo + x0) * C + e] = conv(p, C, ax.k + (size_t)x * ax.ks, cnt);
  }
}

// dst (N, Ho, RB) = the vertical pass of src (N, H, RB), rows of RB bytes; V bytes of a row per thread
template <int V>
__global__ __launch_bounds__(TPB) void vpass_kernel(int H, int Ho, int RB, int nrt, int nct,
                                                    const uint8_t* __restrict__ src, Axis ax, uint8_t* __restrict__ dst) {
  const Tile t = tile_of(nrt, nct);
  const long long e = ((long long)t.ct * TPB + threadIdx.x) * V;
  if (e >= RB) return;   // (V = 4 runs only where RB % 4 == 0: e + 3 < RB)
  const int y0 = t.rt * TR, y1 = min(y0 + TR, Ho);
  const uint8_t* in = src + (size_t)t.n * H * RB + e;
  uint8_t* out = dst + (size_t)t.n * Ho * RB + e;
  for (int y = y0; y < y1; ++y) {
    const int lo = ax.b[2 * y], cnt = ax.b[2 * y + 1];
    const int* __restrict__ kk = ax.k + (size_t)y * ax.ks;
    if (V == 4) {
      *reinterpret_cast<uint32_t*>(out + (size_t)y * RB) = conv4(in + (size_t)lo * RB, RB, kk, cnt);
    } else {
      out[(size_t)y * RB] = conv(in + (size_t)lo * RB, RB, kk, cnt);
    }
  }
}

// both passes of a TR x TC output tile through LDS. Dynamic LDS: rows_max * TC * C bytes, rows_max the most input rows
// any row tile of the call needs
__global__ __launch_bounds__(TPB) void fused_kernel(int H, int W, int C, int Ho, int Wo, int nrt, int nct, int quads,
                                                    const uint8_t* __restrict__ src, Axis ax, Axis ay,
                                                    uint8_t* __restrict__ dst) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const Tile t = tile_of(nrt, nct);
  const int x0 = t.ct * TC, x1 = min(x0 + TC, Wo), y0 = t.rt * TR, y1 = min(y0 + TR, Ho);
  const int r0 = ay.b[2 * y0];                                        // the tile's input rows r0 .. r0 + rows - 1
  const int rows = ay.b[2 * (y1 - 1)] + ay.b[2 * (y1 - 1) + 1] - r0;  // at most rows_max
  const int wC = (x1 - x0) * C, LW = TC * C;
  for (int k = threadIdx.x; k < rows * wC; k += TPB) {
    const int r = k / wC, e = k - r * wC, xe = e / C, c = e - xe * C, x = x0 + xe;
    const int lo = ax.b[2 * x], cnt = ax.b[2 * x + 1];
    lds[r * LW + e] = conv(src + (((size_t)t.n * H + r0 + r) * W + lo) * C + c, C, ax.k + (size_t)x * ax.ks, cnt);
  }
  __syncthreads();
  if (quads) {   // Wo * C % 4 == 0 and dst word aligned: so is every tile's row (x0 * C and wC are multiples of 4)
    const int wQ = wC / 4;
    for (int k = threadIdx.x; k < (y1 - y0) * wQ; k += TPB) {
      const int yy = k / wQ, e = (k - yy * wQ) * 4, y = y0 + yy;
      const int lo = ay.b[2 * y], cnt = ay.b[2 * y + 1];
      *reinterpret_cast<uint32_t*>(dst + (((size_t)t.n * Ho + y) * Wo + x0) * C + e) =
          conv4(lds + (lo - r0) * LW + e, LW, ay.k + (size_t)y * ay.ks, cnt);
    }
    return;
  }
  for (int k = threadIdx.x; k < (y1 - y0) * wC; k += TPB) {
    const int yy = k / wC, e = k - yy * wC, y = y0 + yy;
    const int lo = ay.b[2 * y], cnt = ay.b[2 * y + 1];
    dst[(((size_t)t.n * Ho + y) * Wo + x0) * C + e] = conv(lds + (lo - r0) * LW + e, LW, ay.k + (size_t)y * ay.ks, cnt);
  }
}

// dst (N, Ho, Wo, C) = src (N, H, W, C) at rows yi and columns xi
__global__ __launch_bounds__(TPB) void gather_kernel(int H, int W, int C, int Ho, int Wo, int nct,
                                                     const uint8_t* __restrict__ src, const int* __restrict__ xi,
                                                     const int* __restrict__ yi, uint8_t* __restrict__ dst) {
  int b = blockIdx.x;
  const int ct = b % nct; b /= nct;
  const int y = b % Ho, n = b / Ho;
  const long long e = (long long)ct * TPB + threadIdx.x;
  if (e >= (long long)Wo * C) return;
  const int x = (int)(e / C), c = (int)(e - (long long)x * C);
  dst[((size_t)n * Ho + y) * Wo * C + e] = src[(((size_t)n * H + yi[y]) * W + xi[x]) * C + c];
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return !(pa + na <= pb || pb + nb <= pa);
}

// the checks both entry points share
int check_shape(const std::string& w, int N, int H, int W, int C, int Ho, int Wo) {
  ADP_REQUIRE(N >= 0 && N <= 65535, w + ": N must be in 0 .. 65535");
  ADP_REQUIRE(C >= 1 && C <= 4, w + ": C must be in 1 .. 4");
  ADP_REQUIRE(H >= 1 && W >= 1 && Ho >= 1 && Wo >= 1, w + ": every extent must be at least 1");
  const long long lim = 0x7FFFFFFFll;
  ADP_REQUIRE((long long)H * W * C <= lim && (long long)Ho * Wo * C <= lim && (long long)H * Wo * C <= lim,
              w + ": H * W * C must be below 2^31 for the input, the output and the intermediate");
  return 0;
}

// one axis' host tables, n inputs -> m outputs; *widest = the most inputs a run of `run` outputs spans
int check_axis(const std::string& w, const char* axis, const int* b, const int* k, int ks, int n, int m, int run, int* widest) {
  const std::string a = w + ": " + axis;
  ADP_REQUIRE(b && k, a + " bounds and taps must be non-null where the extent changes");
  ADP_REQUIRE(ks >= 1 && ks <= KMAX, a + " ksize must be in 1 .. " + std::to_string(KMAX) + " (ADP_RESAMPLE_KMAX)");
  int plo = 0, phi = 0;
  *widest = 0;
  for (int i = 0; i < m; ++i) {
    const int lo = b[2 * i], cnt = b[2 * i + 1];
    ADP_REQUIRE(lo >= 0 && cnt >= 0 && cnt <= ks && (long long)lo + cnt <= n,
                a + " bounds must hold 0 <= lo, 0 <= cnt <= ksize and lo + cnt <= the input extent");
    ADP_REQUIRE(lo >= plo && lo + cnt >= phi, a + " bounds must not descend");
    plo = lo;
    phi = lo + cnt;
    long long mag = 0;
    for (int j = 0; j < cnt; ++j) mag += std::llabs((long long)k[(size_t)i * ks + j]);
    ADP_REQUIRE((1ll << (BITS - 1)) + 255 * mag < (1ll << 31), a + " taps: 2^21 + 255 sum |k_j| must stay below 2^31");
    const int first = i - i % run;   // lo never descends: the run's span starts at its first output's lo
    *widest = std::max(*widest, lo + cnt - b[2 * first]);
  }
  return 0;
}

// host ints -> the stream's workspace at word offset `at`; the copy reads `p` before it returns
const int* upload(int* base, size_t& at, const int* p, size_t n, hipStream_t s, bool& ok) {
  int* d = base + at;
  at += (n + 3) & ~(size_t)3;
  if (hipMemcpyAsync(d, p, n * sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess) ok = false;
  return d;
}

}  // namespace

extern "C" int adp_resample_u8(int N, int H, int W, int C, int Ho, int Wo, const uint8_t* src, const int* xb, const int* xk,
                               int xks, const int* yb, const int* yk, int yks, uint8_t* tmp, uint8_t* dst, adp_stream_t st) {
  const std::string w("adp_resample_u8");
  if (int rc = check_shape(w, N, H, W, C, Ho, Wo)) return rc;
  ADP_REQUIRE(src && dst, w + ": src and dst must be non-null");
  const bool horiz = W != Wo, vert = H != Ho;
  int span_max = 0, rows_max = 0;
  if (horiz)
    if (int rc = check_axis(w, "horizontal", xb, xk, xks, W, Wo, TC, &span_max)) return rc;
  if (vert)
    if (int rc = check_axis(w, "vertical", yb, yk, yks, H, Ho, TR, &rows_max)) return rc;
  const size_t nsrc = (size_t)N * H * W * C, ndst = (size_t)N * Ho * Wo * C, ntmp = (size_t)N * H * Wo * C;
  ADP_REQUIRE(!overlap(src, nsrc, dst, ndst), w + ": dst must not overlap src");
  const int opt = adp::option("resample_fused", -1);
  ADP_REQUIRE(opt >= -1 && opt <= 1, w + ": option resample_fused must be -1 (auto), 0 (never) or 1 (whenever it fits)");
  const bool fused = horiz && vert && opt != 0 && (long long)rows_max * TC * C <= LDS_BYTES;
  const bool two = horiz && vert && !fused;
  ADP_REQUIRE(!two || tmp, w + ": tmp must be non-null when both extents change and the fused form is off or does not fit");
  ADP_REQUIRE(!two || (!overlap(tmp, ntmp, src, nsrc) && !overlap(tmp, ntmp, dst, ndst)), w + ": tmp must not overlap src or dst");
  const int nct = (Wo + TC - 1) / TC, nrt = (Ho + TR - 1) / TR;
  // the horizontal pass' rows per block: what the budget holds of the widest span (unstaged beyond it)
  const long long spanB = std::max(4ll, ((long long)span_max * C + 3) & ~3ll);
  const bool staged = horiz && spanB <= LDS_BYTES;
  const int RH = staged ? (int)std::min<long long>(TR, LDS_BYTES / spanB) : TR;
  const int hrt = (H + RH - 1) / RH;
  const long long RB = (long long)Wo * C, vct = (RB + TPB * 4 - 1) / (TPB * 4), vct1 = (RB + TPB - 1) / TPB;
  const long long most = std::max({(long long)N * nrt * nct, (long long)N * hrt * nct, (long long)N * nrt * vct1});
  ADP_REQUIRE(most <= 0x7FFFFFFFll, w + ": too many blocks (N * H * W too large for one launch)");
  if (N == 0) return 0;
  hipStream_t s = (hipStream_t)st;
  if (!horiz && !vert) {
    if (hipMemcpyAsync(dst, src, nsrc, hipMemcpyDeviceToDevice, s) != hipSuccess) {
      adp::set_error(w + ": the copy of an unchanged image failed");
      return -2;
    }
    return 0;
  }
  // the tables, in the stream's workspace
  auto pad4 = [](size_t n) { return (n + 3) & ~(size_t)3; };
  const size_t words = (horiz ? pad4(2 * (size_t)Wo) + pad4((size_t)Wo * xks) : 0) + (vert ? pad4(2 * (size_t)Ho) + pad4((size_t)Ho * yks) : 0);
  int* base = static_cast<int*>(adp::scratch(adp::Slot::ResampleTables, words * sizeof(int), s));
  if (!base) return -3;
  size_t at = 0;
  bool ok = true;
  Axis ax = {nullptr, nullptr, xks}, ay = {nullptr, nullptr, yks};
  if (horiz) {
    ax.b = upload(base, at, xb, 2 * (size_t)Wo, s, ok);
    ax.k = upload(base, at, xk, (size_t)Wo * xks, s, ok);
  }
  if (vert) {
    ay.b = upload(base, at, yb, 2 * (size_t)Ho, s, ok);
    ay.k = upload(base, at, yk, (size_t)Ho * yks, s, ok);
  }
  if (!ok) {
    adp::set_error(w + ": the upload of the tables failed");
    return -2;
  }
  const dim3 block(TPB);
  auto hpass = [&](uint8_t* out) {
    hipLaunchKernelGGL(hpass_kernel, dim3((unsigned)((long long)N * hrt * nct)), block, staged ? (size_t)RH * spanB : 0, s, H, W,
                       C, Wo, RH, (int)spanB, staged ? 1 : 0, hrt, nct, src, ax, out);
  };
  auto vpass = [&](const uint8_t* in, int rb) {   // rows of rb bytes
    const bool quads = rb % 4 == 0 && ((uintptr_t)in & 3) == 0 && ((uintptr_t)dst & 3) == 0;
    if (quads)
      hipLaunchKernelGGL(vpass_kernel<4>, dim3((unsigned)((long long)N * nrt * vct)), block, 0, s, H, Ho, rb, nrt, (int)vct, in, ay, dst);
    else
      hipLaunchKernelGGL(vpass_kernel<1>, dim3((unsigned)((long long)N * nrt * vct1)), block, 0, s, H, Ho, rb, nrt, (int)vct1, in, ay, dst);
  };
  if (fused) {
    const int quads = RB % 4 == 0 && ((uintptr_t)dst & 3) == 0;
    hipLaunchKernelGGL(fused_kernel, dim3((unsigned)((long long)N * nrt * nct)), block, (size_t)rows_max * TC * C, s, H, W, C, Ho,
                       Wo, nrt, nct, quads, src, ax, ay, dst);
  } else if (two) {
    hpass(tmp);
    vpass(tmp, (int)RB);
  } else if (horiz) {
    hpass(dst);
  } else {
    vpass(src, (int)RB);   // (W == Wo)
  }
  return adp::check_launch("adp_resample_u8");
}

extern "C" int adp_resample_nearest_u8(int N, int H, int W, int C, int Ho, int Wo, const uint8_t* src, const int* xi,
                                       const int* yi, uint8_t* dst, adp_stream_t st) {
  const std::string w("adp_resample_nearest_u8");
  if (int rc = check_shape(w, N, H, W, C, Ho, Wo)) return rc;
  ADP_REQUIRE(src && dst && xi && yi, w + ": src, dst and both index tables must be non-null");
  for (int x = 0; x < Wo; ++x) ADP_REQUIRE(xi[x] >= 0 && xi[x] < W, w + ": a column index lies outside 0 .. W - 1");
  for (int y = 0; y < Ho; ++y) ADP_REQUIRE(yi[y] >= 0 && yi[y] < H, w + ": a row index lies outside 0 .. H - 1");
  ADP_REQUIRE(!overlap(src, (size_t)N * H * W * C, dst, (size_t)N * Ho * Wo * C), w + ": dst must not overlap src");
  const long long nct = ((long long)Wo * C + TPB - 1) / TPB, blocks = (long long)N * Ho * nct;
  ADP_REQUIRE(blocks <= 0x7FFFFFFFll, w + ": too many blocks (N * H * W too large for one launch)");
  if (N == 0) return 0;
  hipStream_t s = (hipStream_t)st;
  auto pad4 = [](size_t n) { return (n + 3) & ~(size_t)3; };
  int* base = static_cast<int*>(adp::scratch(adp::Slot::ResampleTables, (pad4(Wo) + pad4(Ho)) * sizeof(int), s));
  if (!base) return -3;
  size_t at = 0;
  bool ok = true;
  const int* dx = upload(base, at, xi, Wo, s, ok);
  const int* dy = upload(base, at, yi, Ho, s, ok);
  if (!ok) {
    adp::set_error(w + ": the upload of the tables failed");
    return -2;
  }
  hipLaunchKernelGGL(gather_kernel, dim3((unsigned)blocks), dim3(TPB), 0, s, H, W, C, Ho, Wo, (int)nct, src, dx, dy, dst);
  return adp::check_launch("adp_resample_nearest_u8");
}
