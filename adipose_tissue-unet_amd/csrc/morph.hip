// Binary mask morphology on bit-packed planes: morph_close (Segmentation/build_dataset.py:1190, build_test_dataset.py:596,
// flag --morph-close-k: cv2.morphologyEx(MORPH_CLOSE, getStructuringElement(MORPH_ELLIPSE, (k, k)))), the step the
// reference applies one line above remove_small_components (components.hip).
//
// A plane is (N, H, WW) 64-bit words, WW = ceil(W / 64); bit b of word w of a row is pixel x = 64 w + b. The bits past W
// in a row's last word are 0: every kernel that writes a plane keeps that.
//
// A footprint is k rows of column extents [lo[a], hi[a]) in a k x k box, anchor c = k / 2 both ways:
//   dilate(M)(y, x) = OR  over lo[a] <= b < hi[a] of M(y + a - c, x + b - c)    positions outside the image take no part
//   erode(M)(y, x)  = AND over the same offsets (not the reflected ones)        likewise: OpenCV's default border
// so erode(M) = ~dilate'(~M) where dilate' sees 0 outside the image: ERODE is the same kernel on the complement
// (complemented on load, with out-of-image words and tail bits 0 after complementing; complemented and masked to W on
// store).
//
// morph_bits_kernel: a block produces TR x TW words (one thread per word) from an LDS copy of the tile with c rows above,
// k - 1 - c below and one word on each side (k <= 63 keeps the horizontal reach below 64 bits); words outside the image
// are staged as 0. The host groups the footprint's rows by extent (the ellipse has 5 distinct extents at k = 15, 10 at
// 31, 19 at 63). Per group a thread ORs its three words (left, middle, right) of the group's rows, cuts the 128 bits
// that start at the group's first column offset out of the three (a funnel shift that takes the left word's top bits
// along: for a negative offset the pixels left of the word come from there), ORs the window with itself shifted by
// 1, 2, 4, ... until `len` neighbours are covered, and ORs the low word into the accumulator: 3 LDS words and 6 ORs per
// footprint row, one span OR of ~log2(len) steps per distinct extent, no loop over taps.
// LDS (TR + 62) * (TW + 2) * 8 = 7520 B at 32 x 8. A 32-lane half reads 4 rows x 8 words at a row stride of 20 dwords:
// the fourth row wraps onto the first row's banks for 12 of its 16 dwords (2-way there). A conflict-free stride would be
// 16 (mod 64) dwords, 80 for this tile; the kernel is bound by its 64-bit shifts, not by LDS.
// No atomics, no communication between blocks, every output word written once by one thread: the result does not depend
// on N, the grid or the run.
#include "common.h"
#include "../../include/adipose_hip.h"

namespace {

constexpr int TPB = 256;
constexpr int KMAX = ADP_MORPH_KMAX;
constexpr int TR = ADP_MORPH_TILE_ROWS, TW = ADP_MORPH_TILE_WORDS;
constexpr int SW = TW + 2;                 // staged words per row
constexpr int SR = TR + KMAX - 1;          // staged rows at the largest footprint
static_assert(TR * TW == TPB, "one thread per output word");
static_assert(KMAX <= 63, "one halo word per side");
typedef unsigned long long u64;

// rows[start[g] .. start[g + 1]) are the footprint rows whose columns are [off[g] + c, off[g] + c + len[g])
struct Groups {
  int k, n;
  signed char off[KMAX];
  unsigned char len[KMAX], start[KMAX + 1], rows[KMAX];
};

template <bool F32>
__global__ __launch_bounds__(TPB) void morph_pack_kernel(size_t nrows, int W, int WW, const void* __restrict__ src,
                                                         float thr, u64* __restrict__ bits) {
  const int lane = threadIdx.x & 63;
  const size_t words = nrows * WW;
  const size_t wave = ((size_t)blockIdx.x * TPB + threadIdx.x) >> 6, nwaves = ((size_t)gridDim.x * TPB) >> 6;
  for (size_t w0 = wave * 4; w0 < words; w0 += nwaves * 4) {   // four words of a wave: their loads are issued together
    bool fg[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const size_t wi = w0 + j;
      fg[j] = false;
      if (wi < words) {
        const size_t row = wi / WW;
        const int x = (int)(wi - row * WW) * 64 + lane;
        if (x < W) {
          const size_t g = row * W + x;
          fg[j] = F32 ? static_cast<const float*>(src)[g] > thr : static_cast<const uint8_t*>(src)[g] != 0;
        }
      }
    }
    u64 m[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) m[j] = __ballot(fg[j]);
    const u64 mine = lane == 0 ? m[0] : lane == 1 ? m[1] : lane == 2 ? m[2] : m[3];
    if (lane < 4 && w0 + lane < words) bits[w0 + lane] = mine;
  }
}

__global__ __launch_bounds__(TPB) void morph_unpack_kernel(size_t nrows, int W, int WW, const u64* __restrict__ bits,
                                                           uint8_t* __restrict__ out_u8, float* __restrict__ out_f32) {
  const int lane = threadIdx.x & 63;
  const size_t words = nrows * WW;
  const size_t wave = ((size_t)blockIdx.x * TPB + threadIdx.x) >> 6, nwaves = ((size_t)gridDim.x * TPB) >> 6;
  for (size_t wi = wave; wi < words; wi += nwaves) {
    const size_t row = wi / WW;
    const int x = (int)(wi - row * WW) * 64 + lane;
    if (x >= W) continue;
    const unsigned b = (unsigned)(bits[wi] >> lane) & 1u;
    const size_t g = row * W + x;
    if (out_u8) out_u8[g] = (uint8_t)b;
    if (out_f32) out_f32[g] = (float)b;
  }
}

// W % 64 == 0 and 16-byte aligned maps: rows are whole words, so the map is one run of P / 16 chunks of 16 pixels and
// four neighbouring lanes make a word. Packing, a lane loads its 16 pixels in 16-byte accesses (one for u8, four for f32) and
// the lanes of a quad exchange their 16 bits in two shuffles; unpacking, a lane stores 16 bytes (16 pixels of u8, 4 of f32). Any other map takes the wave-per-word kernels above.
// bit i of the result = byte i of d is non-zero
ADP_DEV unsigned nonzero_bytes(unsigned d) {
  const unsigned t = (((d & 0x7f7f7f7fu) + 0x7f7f7f7fu) | d) & 0x80808080u;   // bit 7 of every non-zero byte
  return (((t >> 7) * 0x00204081u) >> 21) & 0xFu;                              // bits 0, 8, 16, 24 -> 21 .. 24, no carries
}
// byte i of the result = bit i of nib
ADP_DEV unsigned bytes_of_bits(unsigned nib) { return ((nib & 0xFu) * 0x00204081u) & 0x01010101u; }

template <bool F32>
__global__ __launch_bounds__(TPB) void morph_pack16_kernel(size_t chunks, const void* __restrict__ src, float thr,
                                                           u64* __restrict__ bits) {
  // chunks % 4 == 0 and the stride is a multiple of 4: the lanes of a quad leave the loop together
  for (size_t c = (size_t)blockIdx.x * TPB + threadIdx.x; c < chunks; c += (size_t)gridDim.x * TPB) {
    unsigned m16 = 0;
    if (F32) {
      const float4* p = static_cast<const float4*>(src) + c * 4;
      float4 v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = p[j];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        m16 |= ((unsigned)(v[j].x > thr) | (unsigned)(v[j].y > thr) << 1 | (unsigned)(v[j].z > thr) << 2 |
                (unsigned)(v[j].w > thr) << 3) << (4 * j);
    } else {
      const uint4 v = static_cast<const uint4*>(src)[c];
      m16 = nonzero_bytes(v.x) | nonzero_bytes(v.y) << 4 | nonzero_bytes(v.z) << 8 | nonzero_bytes(v.w) << 12;
    }
    u64 m = (u64)m16 << (16 * (int)(c & 3));
    m |= __shfl_xor(m, 1);
    m |= __shfl_xor(m, 2);
    if ((c & 3) == 0) bits[c >> 2] = m;
  }
}

__global__ __launch_bounds__(TPB) void morph_unpack16_kernel(size_t chunks, const u64* __restrict__ bits,
                                                             uint8_t* __restrict__ out_u8, float* __restrict__ out_f32) {
  if (out_u8)
    for (size_t c = (size_t)blockIdx.x * TPB + threadIdx.x; c < chunks; c += (size_t)gridDim.x * TPB) {
      const unsigned m16 = (unsigned)(bits[c >> 2] >> (16 * (int)(c & 3))) & 0xFFFFu;
      reinterpret_cast<uint4*>(out_u8)[c] = make_uint4(bytes_of_bits(m16), bytes_of_bits(m16 >> 4), bytes_of_bits(m16 >> 8),
                                                       bytes_of_bits(m16 >> 12));
    }
  // f32: one float4 per lane and step, neighbouring lanes store neighbouring float4s (a word is 16 of them)
  if (out_f32)
    for (size_t f = (size_t)blockIdx.x * TPB + threadIdx.x; f < chunks * 4; f += (size_t)gridDim.x * TPB) {
      const unsigned n = (unsigned)(bits[f >> 4] >> (4 * (int)(f & 15)));
      reinterpret_cast<float4*>(out_f32)[f] =
          make_float4((float)(n & 1u), (float)((n >> 1) & 1u), (float)((n >> 2) & 1u), (float)((n >> 3) & 1u));
    }
}

// the low word of OR_{t < len} (v >> t) of the 128-bit v = (hi, lo)
ADP_DEV u64 span_or(u64 lo, u64 hi, int len) {
  int cur = 1;
  while (cur * 2 <= len) {
    lo |= (lo >> cur) | (hi << (64 - cur));
    hi |= hi >> cur;
    cur *= 2;
  }
  if (cur < len) {
    const int t = len - cur;
    lo |= (lo >> t) | (hi << (64 - t));
  }
  return lo;
}

template <bool ERODE>
__global__ __launch_bounds__(TPB) void morph_bits_kernel(int H, int WW, int ntr, int ntw, u64 tail,
                                                         const u64* __restrict__ src, u64* __restrict__ dst, Groups fp) {
  __shared__ u64 S[SR * SW];
  const int per = ntr * ntw;
  const int n = blockIdx.x / per, rem = blockIdx.x - n * per;
  const int y0 = (rem / ntw) * TR, w0 = (rem % ntw) * TW;
  const int c = fp.k / 2;
  const size_t img = (size_t)n * H * WW;
  const int staged = (TR + fp.k - 1) * SW;
  for (int i = threadIdx.x; i < staged; i += TPB) {
    const int r = i / SW, cw = i - r * SW;
    const int y = y0 - c + r, w = w0 - 1 + cw;
    u64 v = 0;
    if (y >= 0 && y < H && w >= 0 && w < WW) {
      v = src[img + (size_t)y * WW + w];
      if (ERODE) {
        v = ~v;
        if (w == WW - 1) v &= tail;
      }
    }
    S[i] = v;
  }
  __syncthreads();
  const int ty = threadIdx.x / TW, tw = threadIdx.x - ty * TW;
  u64 acc = 0;
  for (int g = 0; g < fp.n; ++g) {
    u64 L = 0, M = 0, R = 0;
    for (int j = fp.start[g]; j < fp.start[g + 1]; ++j) {
      const u64* p = &S[(ty + fp.rows[j]) * SW + tw];
      L |= p[0];
      M |= p[1];
      R |= p[2];
    }
    // bits [sh, sh + 128) of the 192-bit (R, M, L): bit 64 + x + off of it is the first neighbour of pixel x
    const int sh = 64 + fp.off[g];   // 33 .. 95
    u64 lo, hi;
    if (sh < 64) {
      lo = (L >> sh) | (M << (64 - sh));
      hi = (M >> sh) | (R << (64 - sh));
    } else if (sh == 64) {
      lo = M;
      hi = R;
    } else {
      lo = (M >> (sh - 64)) | (R << (128 - sh));
      hi = R >> (sh - 64);
    }
    acc |= span_or(lo, hi, fp.len[g]);
  }
  const int y = y0 + ty, w = w0 + tw;
  if (y < H && w < WW) {
    if (ERODE) acc = ~acc;
    if (w == WW - 1) acc &= tail;   // a dilation reaches past W too
    dst[img + (size_t)y * WW + w] = acc;
  }
}

int wave_grid(size_t waves) { return (int)std::min<size_t>((waves + TPB / 64 - 1) / (TPB / 64), 1 << 16); }

int chunk_grid(size_t chunks) { return (int)std::min<size_t>((chunks + TPB - 1) / TPB, 1 << 16); }
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }   // NULL counts as aligned

bool shape_ok(const char* who, int N, int H, int W) {
  if (N < 0 || H < 1 || W < 1) {
    adp::set_error(std::string(who) + ": N must be at least 0, H and W at least 1");
    return false;
  }
  return true;
}

}  // namespace

extern "C" int adp_morph_pack(int N, int H, int W, const void* src, int src_dtype, float thr, unsigned long long* bits,
                              adp_stream_t st) {
  if (!shape_ok("adp_morph_pack", N, H, W)) return -1;
  ADP_REQUIRE(src_dtype == ADP_CC_SRC_U8 || src_dtype == ADP_CC_SRC_F32, "adp_morph_pack: unknown src_dtype");
  if (N == 0) return 0;
  ADP_REQUIRE(src && bits, "adp_morph_pack: src and bits must be non-null");
  const int WW = (W + 63) / 64;
  const size_t nrows = (size_t)N * H, words = nrows * WW;
  if (W % 64 == 0 && aligned16(src)) {
    const size_t chunks = words * 4;
    if (src_dtype == ADP_CC_SRC_F32)
      hipLaunchKernelGGL(morph_pack16_kernel<true>, dim3(chunk_grid(chunks)), dim3(TPB), 0, (hipStream_t)st, chunks, src, thr, bits);
    else
      hipLaunchKernelGGL(morph_pack16_kernel<false>, dim3(chunk_grid(chunks)), dim3(TPB), 0, (hipStream_t)st, chunks, src, thr, bits);
    return adp::check_launch("adp_morph_pack");
  }
  const int grid = wave_grid((words + 3) / 4);
  if (src_dtype == ADP_CC_SRC_F32)
    hipLaunchKernelGGL(morph_pack_kernel<true>, dim3(grid), dim3(TPB), 0, (hipStream_t)st, nrows, W, WW, src, thr, bits);
  else
    hipLaunchKernelGGL(morph_pack_kernel<false>, dim3(grid), dim3(TPB), 0, (hipStream_t)st, nrows, W, WW, src, thr, bits);
  return adp::check_launch("adp_morph_pack");
}

extern "C" int adp_morph_bits(int N, int H, int W, const unsigned long long* src, unsigned long long* dst, int ksize,
                              const int* row_lo, const int* row_hi, int op, adp_stream_t st) {
  if (!shape_ok("adp_morph_bits", N, H, W)) return -1;
  ADP_REQUIRE(ksize >= 1 && ksize <= KMAX, "adp_morph_bits: ksize must be in 1 .. 63");
  ADP_REQUIRE(op == ADP_MORPH_DILATE || op == ADP_MORPH_ERODE, "adp_morph_bits: op must be ADP_MORPH_DILATE or ADP_MORPH_ERODE");
  ADP_REQUIRE(row_lo && row_hi, "adp_morph_bits: the footprint rows must be non-null");
  Groups fp{};
  fp.k = ksize;
  int nrow = 0;
  for (int a = 0; a < ksize; ++a) {
    ADP_REQUIRE(row_lo[a] >= 0 && row_hi[a] <= ksize && row_lo[a] <= row_hi[a], "adp_morph_bits: bad footprint row");
    if (row_lo[a] == row_hi[a]) continue;   // an empty row has no offsets
    bool seen = false;
    for (int b = 0; b < a; ++b) seen = seen || (row_lo[b] == row_lo[a] && row_hi[b] == row_hi[a]);
    if (seen) continue;
    fp.off[fp.n] = (signed char)(row_lo[a] - ksize / 2);
    fp.len[fp.n] = (unsigned char)(row_hi[a] - row_lo[a]);
    fp.start[fp.n] = (unsigned char)nrow;
    for (int b = a; b < ksize; ++b)
      if (row_lo[b] == row_lo[a] && row_hi[b] == row_hi[a]) fp.rows[nrow++] = (unsigned char)b;
    fp.start[++fp.n] = (unsigned char)nrow;
  }
  if (N == 0) return 0;
  ADP_REQUIRE(src && dst, "adp_morph_bits: src and dst must be non-null");
  const int WW = (W + 63) / 64;
  const size_t words = (size_t)N * H * WW;
  const uintptr_t sa = (uintptr_t)src, da = (uintptr_t)dst, bytes = words * sizeof(u64);
  ADP_REQUIRE(sa + bytes <= da || da + bytes <= sa, "adp_morph_bits: src must not alias dst");
  const int ntr = (H + TR - 1) / TR, ntw = (WW + TW - 1) / TW;
  const long long blocks = (long long)N * ntr * ntw;
  ADP_REQUIRE(blocks <= 0x7FFFFFFFll, "adp_morph_bits: too many blocks (N * H * W too large for one launch)");
  const u64 tail = (W & 63) ? (1ull << (W & 63)) - 1 : ~0ull;
  if (op == ADP_MORPH_ERODE)
    hipLaunchKernelGGL(morph_bits_kernel<true>, dim3((unsigned)blocks), dim3(TPB), 0, (hipStream_t)st, H, WW, ntr, ntw,
                       tail, src, dst, fp);
  else
    hipLaunchKernelGGL(morph_bits_kernel<false>, dim3((unsigned)blocks), dim3(TPB), 0, (hipStream_t)st, H, WW, ntr, ntw,
                       tail, src, dst, fp);
  return adp::check_launch("adp_morph_bits");
}

extern "C" int adp_morph_unpack(int N, int H, int W, const unsigned long long* bits, uint8_t* out_u8, float* out_f32,
                                adp_stream_t st) {
  if (!shape_ok("adp_morph_unpack", N, H, W)) return -1;
  if (N == 0) return 0;
  ADP_REQUIRE(bits, "adp_morph_unpack: bits must be non-null");
  ADP_REQUIRE(out_u8 || out_f32, "adp_morph_unpack: out_u8 and out_f32 are both NULL");
  const int WW = (W + 63) / 64;
  const size_t nrows = (size_t)N * H;
  if (W % 64 == 0 && aligned16(out_u8) && aligned16(out_f32)) {
    const size_t chunks = nrows * WW * 4;
    hipLaunchKernelGGL(morph_unpack16_kernel, dim3(chunk_grid(out_f32 ? chunks * 4 : chunks)), dim3(TPB), 0,
                       (hipStream_t)st, chunks, bits, out_u8, out_f32);
    return adp::check_launch("adp_morph_unpack");
  }
  hipLaunchKernelGGL(morph_unpack_kernel, dim3(wave_grid(nrows * WW)), dim3(TPB), 0, (hipStream_t)st, nrows, W, WW, bits,
                     out_u8, out_f32);
  return adp::check_launch("adp_morph_unpack");
}
