// Annotation polygons -> ground-truth masks: create_binary_mask (Segmentation/build_dataset.py:903-911,
// build_test_dataset.py:357-365: one cv2.fillPoly over all polygons of an image), the step before the subtraction of
// the bubbles class, morph_close (morph.hip) and remove_small_components (components.hip). The output is a plane in
// morph.hip's format: (N, H, WW) 64-bit words, WW = ceil(W / 64), bit b of word w of a row is pixel 64 w + b, the bits
// past W are 0. The definition (annotations.py's docstring, its numpy path rasterize_np) restates OpenCV's construction;
// cv2 is not installed, so parity with cv2.fillPoly itself is unpinned.
//
//   mask = interior | boundary
//   interior(y, x) = parity over every non-horizontal edge of every polygon of the image of [ylo <= y < yhi and X(y) <= x],
//                    X(y) = xlo + (y - ylo)(xhi - xlo) / (yhi - ylo) exactly: each (edge, row) toggles column ceil(X(y)),
//                    clamped up to 0 and dropped at >= W, and a row is the prefix-XOR of its toggles (even-odd filling)
//   boundary       = the pixels of every edge's 8-connected line: LineIterator's integer error walk from the endpoint
//                    with the smaller x, in closed form (a pixel per step of the major axis, the minor coordinate
//                    floor((2 minor k + major - 1) / (2 major)) steps on); only pixels inside the raster count
//
// Vertex v starts the edge to the next vertex of its polygon (the last one to the first); a thread finds its polygon and
// image by bisecting the two offset arrays, and takes no edge where they do not bracket it (offsets that do not ascend
// cost pixels, never an access outside xy or the plane: every index is checked against V, N, H and W where it is used).
// Coordinates beyond ADP_POLY_COORD_MAX take no part (the products below then stay under 2^51 in int64).
//
// Four steps on the stream: the plane is zeroed; toggle_kernel XORs one bit per (edge, row); scan_kernel turns every row
// into its prefix parity in place; boundary_kernel ORs the lines in. Integer atomics commute, so the words do not depend
// on the grid, the order of arrival or the run.
//   * An edge's rows (its steps, for the line) are cut to the raster first, so a vertex 2^24 pixels away costs nothing.
//     A lane walks up to SOLO rows of its own edge alone; a longer edge is walked by the whole wave, one after the other
//     (ballot, the edge broadcast by shuffles, a contiguous share of the rows per lane): a slide-high edge does not
//     serialise in one lane and the short edges of an annotator's outline do not leave 63 lanes idle.
//   * A walk divides once, at its first row, and steps quotient and remainder from there (64-bit division is a
//     subroutine on this hardware).
//   * The line pass gathers the bits of one word before it issues the atomic: a flat edge is one atomic a word, not one
//     a pixel.
//   * scan_kernel: a word's prefix parity in six shift-XORs; the words' parities cross the wave in one ballot, a lane
//     flips its word when an odd number of set words precede it in its row; rows wider than ADP_POLY_SCAN_WORDS words
//     carry one bit from chunk to chunk. A row narrower than 64 words shares its wave with other rows (G lanes a row, G
//     the power of two that holds WW). The last word is masked to W: a row whose dropped toggles leave odd parity would
//     otherwise set the bits past W.
#include "common.h"
#include "../../include/adipose_hip.h"

namespace {

typedef unsigned long long u64;
typedef long long i64;
constexpr int TPB = 256;
constexpr int CW = ADP_POLY_SCAN_WORDS;
constexpr i64 CMAX = ADP_POLY_COORD_MAX;
constexpr int SOLO = 32;   // rows (line steps) up to which a lane walks its edge alone
static_assert(CW == 64, "a chunk of the scan is one word per lane of a wave");
static_assert(CMAX <= (1 << 24), "(2 CMAX)^2 and 2 (2 CMAX)^2 must stay far below 2^63");

struct Edge {
  int x0, y0, x1, y1;
  int img;   // -1: no edge
};

ADP_DEV i64 floordiv(i64 a, i64 b) {   // b > 0
  i64 q = a / b;
  return (a - q * b < 0) ? q - 1 : q;
}

// the last i in [0, n) with off[i] <= v (0 when there is none); n >= 1
ADP_DEV int last_le(const int* __restrict__ off, int n, i64 v) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= v) lo = mid; else hi = mid;
  }
  return lo;
}

ADP_DEV Edge load_edge(i64 v, i64 V, int P, int N, const int* __restrict__ xy, const int* __restrict__ poly_off,
                       const int* __restrict__ img_off) {
  Edge e = {0, 0, 0, 0, -1};
  if (v >= V) return e;
  const int p = last_le(poly_off, P, v);
  const i64 start = poly_off[p], end = poly_off[p + 1];
  if (!(start >= 0 && start <= v && v < end && end <= V)) return e;
  const int n = last_le(img_off, N, p);
  if (!(img_off[n] <= p && p < img_off[n + 1])) return e;
  const i64 nxt = v + 1 < end ? v + 1 : start;
  e.x0 = xy[2 * v]; e.y0 = xy[2 * v + 1];
  e.x1 = xy[2 * nxt]; e.y1 = xy[2 * nxt + 1];
  const bool ok = e.x0 >= -CMAX && e.x0 <= CMAX && e.y0 >= -CMAX && e.y0 <= CMAX && e.x1 >= -CMAX && e.x1 <= CMAX &&
                  e.y1 >= -CMAX && e.y1 <= CMAX;
  e.img = ok ? n : -1;
  return e;
}

ADP_DEV Edge edge_from(const Edge& e, int src) {
  Edge s;
  s.x0 = __shfl(e.x0, src, 64); s.y0 = __shfl(e.y0, src, 64);
  s.x1 = __shfl(e.x1, src, 64); s.y1 = __shfl(e.y1, src, 64);
  s.img = __shfl(e.img, src, 64);
  return s;
}

// ---- interior: the rows [r0, r1) of an edge inside the raster, and the toggles of rows [a, b) of them
ADP_DEV void toggle_range(const Edge& e, int H, i64& r0, i64& r1) {
  const i64 ylo = min(e.y0, e.y1), yhi = max(e.y0, e.y1);
  r0 = max(ylo, (i64)0);
  r1 = e.img < 0 ? r0 : min(yhi, (i64)H);   // (a horizontal edge has ylo == yhi: no rows)
}

ADP_DEV void toggle_rows(const Edge& e, i64 a, i64 b, int W, int WW, u64* __restrict__ plane) {
  if (a >= b) return;
  const bool up = e.y0 <= e.y1;
  const i64 xlo = up ? e.x0 : e.x1, ylo = up ? e.y0 : e.y1, xhi = up ? e.x1 : e.x0, yhi = up ? e.y1 : e.y0;
  const i64 D = yhi - ylo, dxs = xhi - xlo;   // D > 0: a >= ylo, b <= yhi, a < b
  const i64 qs = floordiv(dxs, D), rs = dxs - qs * D;
  i64 q = floordiv((a - ylo) * dxs, D), r = (a - ylo) * dxs - q * D;   // X(y) - xlo = q + r / D, 0 <= r < D
  for (i64 y = a; y < b; ++y) {
    i64 c = xlo + q + (r > 0 ? 1 : 0);
    if (c < 0) c = 0;
    if (c < W) atomicXor(plane + (size_t)y * WW + (size_t)(c >> 6), 1ull << (c & 63));
    q += qs;
    r += rs;
    if (r >= D) { r -= D; ++q; }
  }
}

__global__ __launch_bounds__(TPB) void toggle_kernel(i64 V, int P, int N, int H, int W, int WW,
                                                     const int* __restrict__ xy, const int* __restrict__ poly_off,
                                                     const int* __restrict__ img_off, u64* __restrict__ bits) {
  const int lane = threadIdx.x & 63;
  const i64 v = (i64)blockIdx.x * TPB + threadIdx.x;
  const Edge e = load_edge(v, V, P, N, xy, poly_off, img_off);   // (no thread leaves before the ballot)
  i64 r0, r1;
  toggle_range(e, H, r0, r1);
  const size_t img_words = (size_t)H * WW;
  if (r1 - r0 <= SOLO) toggle_rows(e, r0, r1, W, WW, bits + (size_t)max(e.img, 0) * img_words);
  u64 todo = __ballot(r1 - r0 > SOLO);
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const Edge s = edge_from(e, src);
    i64 s0, s1;
    toggle_range(s, H, s0, s1);
    const i64 share = (s1 - s0 + 63) / 64, a = s0 + lane * share;
    toggle_rows(s, a, min(a + share, s1), W, WW, bits + (size_t)s.img * img_words);
  }
}

// ---- boundary: the line from the endpoint with the smaller x, steps k = 0 .. L of its major axis
struct Line {
  i64 xa, ya, s, den, step;   // den = 2 L, step = 2 * the minor extent (den = 1, step = 0 for a point)
  bool ymajor;
  i64 k0, k1;                 // the steps [k0, k1) whose major coordinate is inside the raster
};

ADP_DEV Line line_of(const Edge& e, int H, int W) {
  Line l;
  const bool fwd = e.x0 <= e.x1;
  l.xa = fwd ? e.x0 : e.x1; l.ya = fwd ? e.y0 : e.y1;
  const i64 xb = fwd ? e.x1 : e.x0, yb = fwd ? e.y1 : e.y0;
  const i64 dx = xb - l.xa, dy = yb - l.ya, ady = dy < 0 ? -dy : dy;
  l.s = dy > 0 ? 1 : dy < 0 ? -1 : 0;
  l.ymajor = ady > dx;
  const i64 L = l.ymajor ? ady : dx;
  l.den = L ? 2 * L : 1;
  l.step = L ? 2 * (l.ymajor ? dx : ady) : 0;
  i64 lo, hi;   // inclusive
  if (!l.ymajor) { lo = -l.xa; hi = (i64)W - 1 - l.xa; }
  else if (l.s > 0) { lo = -l.ya; hi = (i64)H - 1 - l.ya; }
  else { lo = l.ya - ((i64)H - 1); hi = l.ya; }
  l.k0 = max(lo, (i64)0);
  l.k1 = e.img < 0 ? l.k0 : max(min(hi, L) + 1, l.k0);
  return l;
}

ADP_DEV void walk(const Line& l, i64 a, i64 b, int H, int W, int WW, u64* __restrict__ plane) {
  if (a >= b) return;
  const i64 num = l.step * a + l.den / 2 - (l.den > 1 ? 1 : 0);   // >= 0
  i64 q = num / l.den, r = num - q * l.den;
  u64 acc = 0;
  i64 cur = -1;
  for (i64 k = a; k < b; ++k) {
    const i64 x = l.ymajor ? l.xa + q : l.xa + k, y = l.ymajor ? l.ya + l.s * k : l.ya + l.s * q;
    if (x >= 0 && x < W && y >= 0 && y < H) {
      const i64 idx = y * WW + (x >> 6);
      if (idx != cur) {
        if (acc) atomicOr(plane + cur, acc);
        cur = idx;
        acc = 0;
      }
      acc |= 1ull << (x & 63);
    }
    r += l.step;   // step <= den: at most one carry
    if (r >= l.den) { r -= l.den; ++q; }
  }
  if (acc) atomicOr(plane + cur, acc);
}

__global__ __launch_bounds__(TPB) void boundary_kernel(i64 V, int P, int N, int H, int W, int WW,
                                                       const int* __restrict__ xy, const int* __restrict__ poly_off,
                                                       const int* __restrict__ img_off, u64* __restrict__ bits) {
  const int lane = threadIdx.x & 63;
  const i64 v = (i64)blockIdx.x * TPB + threadIdx.x;
  const Edge e = load_edge(v, V, P, N, xy, poly_off, img_off);
  const Line l = line_of(e, H, W);
  const size_t img_words = (size_t)H * WW;
  if (l.k1 - l.k0 <= SOLO) walk(l, l.k0, l.k1, H, W, WW, bits + (size_t)max(e.img, 0) * img_words);
  u64 todo = __ballot(l.k1 - l.k0 > SOLO);
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const Edge s = edge_from(e, src);
    const Line m = line_of(s, H, W);
    const i64 share = (m.k1 - m.k0 + 63) / 64, a = m.k0 + lane * share;
    walk(m, a, min(a + share, m.k1), H, W, WW, bits + (size_t)s.img * img_words);
  }
}

// ---- rows -> their prefix parity, in place. lg = log2(G), G lanes a row
__global__ __launch_bounds__(TPB) void scan_kernel(size_t rows, int WW, int lg, u64 tail, u64* __restrict__ bits) {
  const int lane = threadIdx.x & 63;
  const int G = 1 << lg, seg = lane >> lg, pos = lane & (G - 1);
  const u64 segmask = (G == 64 ? ~0ull : (1ull << G) - 1) << (seg * G);
  const u64 before = segmask & ((1ull << lane) - 1);   // the lanes of my row left of me
  const size_t wave = ((size_t)blockIdx.x * TPB + threadIdx.x) >> 6, nwaves = ((size_t)gridDim.x * TPB) >> 6;
  const size_t per = (size_t)(64 >> lg);
  for (size_t r0 = wave * per; r0 < rows; r0 += nwaves * per) {   // (wave-uniform: every lane reaches the ballot)
    const size_t row = r0 + seg;
    unsigned carry = 0;
    for (int w0 = 0; w0 < WW; w0 += G) {
      const int w = w0 + pos;
      const bool ok = row < rows && w < WW;
      u64* p = bits + row * WW + w;
      u64 v = ok ? *p : 0;
      v ^= v << 1; v ^= v << 2; v ^= v << 4; v ^= v << 8; v ^= v << 16; v ^= v << 32;
      const u64 odd = __ballot((int)(v >> 63));
      if ((__popcll(odd & before) & 1u) ^ carry) v = ~v;
      if (ok) *p = (w == WW - 1) ? v & tail : v;
      carry ^= __popcll(odd & segmask) & 1u;
    }
  }
}

}  // namespace

extern "C" int adp_poly_raster(int N, int H, int W, const int* xy, const int* poly_off, const int* img_off, int P,
                               long long V, unsigned long long* bits, adp_stream_t st) {
  ADP_REQUIRE(N >= 0 && H >= 1 && W >= 1, "adp_poly_raster: N must be at least 0, H and W at least 1");
  ADP_REQUIRE(P >= 0 && V >= 0 && V <= 0x7FFFFFFFll, "adp_poly_raster: P must be at least 0, V in 0 .. 2^31 - 1");
  if (N == 0) return 0;
  ADP_REQUIRE(xy && poly_off && img_off && bits, "adp_poly_raster: xy, poly_off, img_off and bits must be non-null");
  hipStream_t s = (hipStream_t)st;
  const int WW = (W + 63) / 64;
  const size_t rows = (size_t)N * H;
  if (hipMemsetAsync(bits, 0, rows * WW * sizeof(u64), s) != hipSuccess) {
    (void)hipGetLastError();
    adp::set_error("adp_poly_raster: zeroing the plane failed");
    return -1;
  }
  if (P == 0 || V == 0) return 0;
  const unsigned blocks = (unsigned)((V + TPB - 1) / TPB);
  hipLaunchKernelGGL(toggle_kernel, dim3(blocks), dim3(TPB), 0, s, (i64)V, P, N, H, W, WW, xy, poly_off, img_off, bits);
  if (adp::check_launch("adp_poly_raster (toggle)")) return -1;
  int lg = 0;
  while ((1 << lg) < std::min(WW, CW)) ++lg;
  const size_t waves = (rows + (64 >> lg) - 1) / (64 >> lg);
  const unsigned sblocks = (unsigned)std::min<size_t>((waves + TPB / 64 - 1) / (TPB / 64), 1u << 20);
  const u64 tail = (W & 63) ? (1ull << (W & 63)) - 1 : ~0ull;
  hipLaunchKernelGGL(scan_kernel, dim3(sblocks), dim3(TPB), 0, s, rows, WW, lg, tail, bits);
  if (adp::check_launch("adp_poly_raster (scan)")) return -1;
  hipLaunchKernelGGL(boundary_kernel, dim3(blocks), dim3(TPB), 0, s, (i64)V, P, N, H, W, WW, xy, poly_off, img_off, bits);
  return adp::check_launch("adp_poly_raster");
}
