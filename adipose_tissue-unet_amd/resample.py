"""Pillow-exact resampling of 8-bit images: the ECM-channel scaling step, on the device.

The annotations are drawn on the Pseudocolored slides; an ECM slide of the same section has slightly different pixel
dimensions. The reference lines the two up in pre-post-processing_tools/ECM_scaling.py: every ECM image is resampled to
the exact width and height of its Pseudocolored counterpart with PIL.Image.resize(size, Image.LANCZOS) (:175, :184).
Its docstring (:17-42) also promises bilinear, bicubic and nearest, which its argparse never got; cli/ecm_scaling.py
has the flag. This module has

  get_image_size / build_reference_dict / resample_image   :66-192   the script's host helpers (all I/O through PIL)
  resize_np / resize / resample_image_array / Resampler              PIL.Image.resize of an 8-bit image, restated

The definition is Pillow's (src/libImaging/Resample.c for 8-bit images, Geometry.c for nearest), and Pillow is a
dependency: tests/test_resample.py holds resize_np to live PIL.Image.resize and to tests/golden/resample.npz on every
pixel, with no tolerance. The host computes a coefficient table in float64; everything after it is integer arithmetic.

Input. (H, W, C) or (N, H, W, C) uint8 with C in 1 .. 4, or (H, W) / (N, H, W) with C = 1. A 3-D array is (H, W, C)
when its last extent is 1 .. 4 and (N, H, W) otherwise; `channels=` (True / False) says it outright. Every channel and
every image is treated on its own: Pillow's behaviour for modes L and RGB. Pillow premultiplies RGBA / LA by alpha
before it resamples: that is out of scope (a 4-channel array is resampled here as four independent planes, which is
Pillow's RGBX, not its RGBA; resample_image hands RGBA / LA files to Pillow on the host and says so). Float input is
not accepted.

Filters (FILTERS: name -> support, f), f evaluated in float64 with math.sin / math.cos (the C library's):
      box       0.5   1 for -0.5 < x <= 0.5, else 0
      bilinear  1     1 - |x| for |x| < 1, else 0
      hamming   1     1 at 0; 0 for |x| >= 1; else sin(pi x) / (pi x) * (0.54 + 0.46 cos(pi x))
      bicubic   2     a = -0.5: ((a + 2)|x| - (a + 3)) x^2 + 1 for |x| < 1; (((|x| - 5)|x| + 8)|x| - 4) a for |x| < 2; else 0
      lanczos   3     sinc(x) sinc(x / 3) for -3 <= x < 3, else 0; sinc(0) = 1, sinc(x) = sin(pi x) / (pi x)

Coefficients of one axis, input extent n, output extent m (coefficients(); the device never evaluates sin):
      scale = n / m, fs = max(scale, 1), ss = 1 / fs, support = filter support * fs, ksize = 2 ceil(support) + 1
    for output index i:
      c   = (i + 0.5) scale
      lo  = max(int(c - support + 0.5), 0),  hi = min(int(c + support + 0.5), n),  cnt = hi - lo
      w_j = f((j + lo - c + 0.5) * ss) for j < cnt       (Pillow multiplies by the reciprocal ss; it does not divide by
                                                          fs. The two can round differently in the last place; this
                                                          module does what Pillow does)
      ww  = the sum of the w_j in ascending j;  w_j /= ww when ww != 0
      k_j = int(w_j 2^22 + 0.5) for w_j >= 0, else int(w_j 2^22 - 0.5)
    int is C truncation throughout. lo and hi never descend with i; taps beyond cnt are zero.

One pass along an axis: out = clamp((2^21 + sum_j k_j v[lo + j]) >> 22, 0, 255), the shift arithmetic. Pillow
accumulates in int32; pass_np accumulates in int64 and raises OverflowError unless every partial sum's bound
2^21 + 255 sum_j |k_j| stays below 2^31 (it does for every table coefficients() makes), so the device uses int32.

Two passes. The horizontal pass runs first and writes a uint8 image; the vertical pass runs on that image: the rounding
between the two is part of the definition. A pass whose extent does not change is skipped, not run with identity taps.

Nearest (nearest_table()). No convolution. Per axis a = n / m, and a double x0 = a * 0.5 is accumulated (x0 += a after
each output index); the source index is int(x0), clamped to n - 1. (The closed form int((i + 0.5) n / m) is not the
same table.) The table is built on the host; the device gathers.

Limits. Extents >= 1; H * W * C < 2^31 on both sides (and for the intermediate); N <= 65535; ksize <= KMAX = 193 (Lanczos
down to 1 / 32, bicubic to 1 / 48, bilinear and Hamming to 1 / 96, box to 1 / 192). Beyond them resize_np and resize
raise ValueError. coefficients() and pass_np() themselves have no ksize limit.

The device path (csrc/resample.hip: adp_resample_u8 / adp_resample_nearest_u8) and the numpy path below (hosts without
a GPU, and the tests' reference) agree bit for bit, in both of the device's forms (one fused launch where the tile's
intermediate fits LDS, otherwise two launches through an intermediate image; library option resample_fused).
"""
from __future__ import annotations

import math
import os
import re

import numpy as np

from .components import _is_tensor, _to_device
from .contrast import _dispatch

KMAX = 193                       # include/adipose_hip.h ADP_RESAMPLE_KMAX
TILE_ROWS, TILE_COLS = 32, 64    # ADP_RESAMPLE_TILE_ROWS / _COLS: the output tile of one block of the fused form
LDS_BYTES = 32768                # ADP_RESAMPLE_LDS_BYTES: what a block may hold (five blocks per CU)
PRECISION_BITS = 22
NMAX = 65535
_WHAT = "resampling"
IMAGE_EXTS = (".jpg", ".jpeg", ".png", ".tif", ".tiff")


# ---------------------------------------------------------------- definition: filters
def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _hamming(x):
    x = abs(x)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    x = x * math.pi
    return math.sin(x) / x * (0.54 + 0.46 * math.cos(x))


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


FILTERS = {"box": (0.5, _box), "bilinear": (1.0, _bilinear), "hamming": (1.0, _hamming), "bicubic": (2.0, _bicubic),
           "lanczos": (3.0, _lanczos)}
METHODS = tuple(FILTERS) + ("nearest",)


def _filter(name):
    if name not in FILTERS:
        raise ValueError(f"unknown filter {name!r}: one of {', '.join(FILTERS)} (or nearest)")
    return FILTERS[name]


def _extent(v, what):
    if isinstance(v, bool) or int(v) != v or int(v) < 1:
        raise ValueError(f"{what} must be an integer of at least 1")
    return int(v)


def ksize_of(n, m, filter):
    """ksize of the module's definition for one axis."""
    support = _filter(filter)[0] * max(_extent(n, "n") / _extent(m, "m"), 1.0)
    return int(math.ceil(support)) * 2 + 1


def coefficients(n, m, filter):
    """The table of one axis: (bounds (m, 2) int32 rows {lo, cnt}, taps (m, ksize) int32, zero beyond cnt, ksize)."""
    support0, f = _filter(filter)
    n, m = _extent(n, "n"), _extent(m, "m")
    scale = n / m
    fs = max(scale, 1.0)
    support = support0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    c = (np.arange(m, dtype=np.float64) + 0.5) * scale
    lo = np.maximum(np.trunc(c - support + 0.5).astype(np.int64), 0)
    hi = np.minimum(np.trunc(c + support + 0.5).astype(np.int64), n)
    cnt = hi - lo
    j = np.arange(ksize, dtype=np.int64)
    live = j[None, :] < cnt[:, None]
    x = ((j[None, :] + lo[:, None]).astype(np.float64) - c[:, None] + 0.5) * ss
    w = np.zeros((m, ksize), np.float64)
    w[live] = [f(v) for v in x[live].tolist()]
    ww = np.cumsum(w, axis=1)[:, -1:]          # a sequential sum in ascending j (the zeros beyond cnt add nothing)
    w = np.divide(w, ww, out=w, where=ww != 0.0)
    k = np.where(w < 0.0, np.trunc(w * float(1 << PRECISION_BITS) - 0.5), np.trunc(w * float(1 << PRECISION_BITS) + 0.5))
    k = np.where(live, k, 0.0)
    return np.stack([lo, cnt], axis=1).astype(np.int32), np.ascontiguousarray(k.astype(np.int32)), ksize


def nearest_table(n, m):
    """(m,) int32: the source index of every output index of one axis."""
    n, m = _extent(n, "n"), _extent(m, "m")
    a = n / m
    x0 = a * 0.5
    out = np.empty(m, np.int32)
    for i in range(m):
        out[i] = min(int(x0), n - 1)
        x0 += a
    return out


# ---------------------------------------------------------------- numpy path
def pass_np(a, bounds, taps, axis):
    """One pass of the module's definition along `axis` of the uint8 array a (extent n there -> len(bounds))."""
    a = np.asarray(a)
    if a.dtype != np.uint8:
        raise TypeError(f"{_WHAT} takes uint8")
    bounds, taps = np.asarray(bounds, np.int64), np.asarray(taps, np.int64)
    n, m, ks = a.shape[axis], bounds.shape[0], taps.shape[1]
    lo, cnt = bounds[:, 0], bounds[:, 1]
    if bounds.shape != (m, 2) or taps.shape[0] != m or lo.min(initial=0) < 0 or cnt.min(initial=0) < 0 \
            or cnt.max(initial=0) > ks or (lo + cnt).max(initial=0) > n:
        raise ValueError("bounds must hold 0 <= lo, 0 <= cnt <= ksize and lo + cnt <= n")
    if (1 << (PRECISION_BITS - 1)) + 255 * int(np.abs(taps).sum(axis=1).max(initial=0)) >= 1 << 31:
        raise OverflowError("a pass' sum may leave int32: 2^21 + 255 sum |k_j| must stay below 2^31")
    v = np.moveaxis(a, axis, 0)
    flat = v.reshape(n, -1)
    out = np.empty((m, flat.shape[1]), np.uint8)
    step = max(1, (1 << 22) // max(m, 1))      # columns per chunk: the int64 accumulator stays near 32 MiB
    for c0 in range(0, flat.shape[1], step):
        blk = flat[:, c0:c0 + step]
        acc = np.full((m, blk.shape[1]), 1 << (PRECISION_BITS - 1), np.int64)
        for j in range(int(cnt.max(initial=0))):
            on = j < cnt
            acc[on] += taps[on, j, None] * blk[lo[on] + j].astype(np.int64)
        out[:, c0:c0 + step] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.ascontiguousarray(np.moveaxis(out.reshape((m,) + v.shape[1:]), 0, axis))


def _layout(shape, channels):
    """The shape of an input -> (N, H, W, C) and a function that gives an (N, Ho, Wo, C) result the input's layout."""
    nd = len(shape)
    if nd not in (2, 3, 4):
        raise ValueError(f"{_WHAT} takes (H, W), (N, H, W), (H, W, C) or (N, H, W, C)")
    if nd == 4:
        if channels is False:
            raise ValueError("a 4-D input has channels")
        chan = True
    elif nd == 2:
        if channels:
            raise ValueError("a 2-D input has no channels")
        chan = False
    else:
        chan = (1 <= shape[-1] <= 4) if channels is None else bool(channels)
    batch = nd == 4 or (nd == 3 and not chan)
    N = int(shape[0]) if batch else 1
    C = int(shape[-1]) if chan else 1
    H, W = (int(s) for s in (shape[-3:-1] if chan else shape[-2:]))
    if not 1 <= C <= 4:
        raise ValueError(f"{_WHAT} takes 1 .. 4 channels")
    if H < 1 or W < 1:
        raise ValueError(f"{_WHAT} takes an image of at least 1 x 1")

    def back(ho, wo):
        return ((N,) if batch else ()) + (ho, wo) + ((C,) if chan else ())
    return N, H, W, C, back


def _size(size):
    try:
        wo, ho = size
    except (TypeError, ValueError):
        raise ValueError("size is (width, height)") from None
    return _extent(wo, "the width"), _extent(ho, "the height")


def _limits(N, H, W, C, Ho, Wo, filter):
    """ValueError for what neither path accepts; the two axes' ksize (0 for nearest)."""
    if N > NMAX:
        raise ValueError(f"{_WHAT} takes at most {NMAX} images")
    for h, w in ((H, W), (Ho, Wo), (H, Wo)):
        if h * w * C >= 1 << 31:
            raise ValueError(f"{_WHAT} takes images of H * W * C below 2^31 (input, output and the intermediate)")
    if filter == "nearest":
        return 0, 0
    ks = ksize_of(W, Wo, filter), ksize_of(H, Ho, filter)
    for k, n, m in ((ks[0], W, Wo), (ks[1], H, Ho)):
        if n != m and k > KMAX:
            raise ValueError(f"{n} -> {m} needs {k} taps per output; the limit is {KMAX} ({filter} down to 1 / "
                             f"{int((KMAX - 1) / 2 / FILTERS[filter][0])})")
    return ks


def resize_np(img, size, filter="lanczos", channels=None):
    """PIL.Image.resize(size, filter) of every image and channel of a uint8 array, size = (width, height), by the
    module's definition: the numpy path."""
    a = np.asarray(img)
    if a.dtype != np.uint8:
        raise TypeError(f"{_WHAT} takes uint8")
    N, H, W, C, back = _layout(a.shape, channels)
    Wo, Ho = _size(size)
    if filter != "nearest":
        _filter(filter)
    _limits(N, H, W, C, Ho, Wo, filter)
    v = a.reshape(N, H, W, C)
    if filter == "nearest":
        v = v[:, nearest_table(H, Ho)][:, :, nearest_table(W, Wo)]
    else:
        if Wo != W:
            b, k, _ = coefficients(W, Wo, filter)
            v = pass_np(v, b, k, 2)
        if Ho != H:
            b, k, _ = coefficients(H, Ho, filter)
            v = pass_np(v, b, k, 1)
    return np.ascontiguousarray(v).reshape(back(Ho, Wo))


# ---------------------------------------------------------------- device path
def _host_ptr(a):
    import ctypes as C
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _tile_rows(yb, Ho):
    """The most input rows any TILE_ROWS output rows span, from the vertical bounds."""
    b = np.asarray(yb, np.int64)
    y0 = np.arange(0, Ho, TILE_ROWS)
    y1 = np.minimum(y0 + TILE_ROWS, Ho) - 1
    return int((b[y1, 0] + b[y1, 1] - b[y0, 0]).max())


def fused_fits(H, W, C, Ho, Wo, filter):
    """Whether the fused form's footprint admits this resize (both extents change and the intermediate rows of every
    TILE_ROWS x TILE_COLS output tile fit LDS_BYTES): what adp_resample_u8 computes from the vertical bounds."""
    if filter == "nearest" or H == Ho or W == Wo:
        return False
    return _tile_rows(coefficients(H, Ho, filter)[0], Ho) * TILE_COLS * C <= LDS_BYTES


def resize(t, size, filter="lanczos", channels=None, tmp=None):
    """resize_np on the device: a uint8 array (uploaded) or tensor -> a uint8 device tensor in the input's layout. The
    two-launch form runs through `tmp`, a uint8 tensor of at least N * H * Wo * C elements (allocated here when None and
    needed). Runs on the current stream; the tables are read on the host before the call returns."""
    import torch

    from ._lib import call, ptr, stream_ptr
    m = _to_device(t)
    if m.dtype != torch.uint8:
        raise TypeError(f"{_WHAT} takes uint8")
    N, H, W, C, back = _layout(tuple(m.shape), channels)
    Wo, Ho = _size(size)
    if filter != "nearest":
        _filter(filter)
    _limits(N, H, W, C, Ho, Wo, filter)
    m = m.contiguous()
    out = torch.empty(back(Ho, Wo), dtype=torch.uint8, device=m.device)
    if N == 0:
        return out
    with torch.cuda.device(m.device):
        if filter == "nearest":
            xi, yi = nearest_table(W, Wo), nearest_table(H, Ho)
            call("adp_resample_nearest_u8", N, H, W, C, Ho, Wo, ptr(m), _host_ptr(xi), _host_ptr(yi), ptr(out), stream_ptr())
            return out
        xb = xk = yb = yk = None
        xks = yks = 0
        if Wo != W:
            xb, xk, xks = coefficients(W, Wo, filter)
        if Ho != H:
            yb, yk, yks = coefficients(H, Ho, filter)
        if tmp is None:
            from .ops import get_option
            if xb is not None and yb is not None and (get_option("resample_fused") == 0
                                                      or _tile_rows(yb, Ho) * TILE_COLS * C > LDS_BYTES):
                tmp = torch.empty(N * H * Wo * C, dtype=torch.uint8, device=m.device)
        elif not (_is_tensor(tmp) and tmp.is_cuda and tmp.device == m.device and tmp.dtype == torch.uint8
                  and tmp.is_contiguous() and tmp.numel() >= N * H * Wo * C):
            raise ValueError("tmp must be a contiguous uint8 tensor of at least N * H * Wo * C elements on the image's device")
        call("adp_resample_u8", N, H, W, C, Ho, Wo, ptr(m), _host_ptr(xb), _host_ptr(xk), xks, _host_ptr(yb), _host_ptr(yk),
             yks, ptr(tmp), ptr(out), stream_ptr())
    return out


# ---------------------------------------------------------------- the public surface
def resample_image_array(img, size, filter="lanczos", channels=None):
    """resize in the input's container: array in, array out; tensor in, tensor out on the same device; the device where
    there is one, the numpy path otherwise."""
    Wo, Ho = _size(size)
    if filter not in METHODS:
        _filter(filter)
    return _dispatch(img, lambda a: resize_np(a, (Wo, Ho), filter, channels), lambda v: resize(v, (Wo, Ho), filter, channels))


class Resampler:
    """resample_image_array to a fixed size = (width, height): call it on an image or a batch. The size and the filter
    are checked here."""

    def __init__(self, size, filter="lanczos"):
        self.size = _size(size)
        if filter not in METHODS:
            _filter(filter)
        self.filter = filter

    def __call__(self, img):
        return resample_image_array(img, self.size, self.filter)

    def __repr__(self):
        return f"Resampler(size={self.size}, filter={self.filter!r})"


# ---------------------------------------------------------------- the script's host helpers
def _pil():
    from PIL import Image
    Image.MAX_IMAGE_PIXELS = None   # the script's setting: slides are larger than Pillow's default limit
    return Image


def get_image_size(image_path):
    """ECM_scaling.py:66-81: (width, height) of an image file."""
    with _pil().open(image_path) as img:
        return tuple(img.size)


def build_reference_dict(reference_dir, log=print):
    """ECM_scaling.py:84-111: {stem: (width, height)} of the image files of a directory; a file that cannot be read is
    reported and left out."""
    sizes = {}
    for name in os.listdir(reference_dir):
        path = os.path.join(reference_dir, name)
        stem, ext = os.path.splitext(name)
        if not os.path.isfile(path) or ext.lower() not in IMAGE_EXTS:
            continue
        try:
            sizes[stem] = get_image_size(path)
            log(f"Reference: {stem} → {sizes[stem][0]}×{sizes[stem][1]}")
        except Exception as e:   # the script goes on with the other files
            log(f"⚠️  Failed to read {name}: {e}")
    return sizes


def match_reference(stem, ref_sizes):
    """ECM_scaling.py:263-276: the reference stem of a target stem: itself, else without a trailing -ddd, else None."""
    if stem in ref_sizes:
        return stem
    stripped = re.sub(r"-\d{3}$", "", stem)
    return stripped if stripped in ref_sizes else None


def to_uint8_minmax(a):
    """ECM_scaling.py:132-139: a 16-bit array to 8 bits, ((a - min) / (max - min) * 255) in float32, truncated; zeros for
    a flat image. (max - min is taken in Python integers: the script's int16 difference can wrap.)"""
    a = np.asarray(a)
    lo, hi = int(a.min()), int(a.max())
    if hi <= lo:
        return np.zeros(a.shape, np.uint8)
    return ((a.astype(np.float32) - np.float32(lo)) / np.float32(hi - lo) * np.float32(255)).astype(np.uint8)


def _save(img, output_path, ext):
    """The script's save settings per format (:178, :187-192)."""
    if ext in (".tif", ".tiff"):
        img.save(output_path, format="TIFF", compression="tiff_deflate")
    elif ext in (".jpg", ".jpeg"):
        img.save(output_path, format="JPEG", quality=95, optimize=True)
    elif ext == ".png":
        img.save(output_path, format="PNG", optimize=True)
    else:
        img.save(output_path)


def resample_image(input_path, target_size, output_path, filter="lanczos", log=print):
    """ECM_scaling.py:114-192: the image file resampled to target_size = (width, height) and saved in its own format.
    A 16-bit gray TIFF is brought to 8 bits first (to_uint8_minmax). Modes L and RGB go through resample_image_array
    (the device where there is one); any other mode (RGBA and LA, which Pillow premultiplies; palette, 1-bit, 32-bit) is
    resampled by Pillow on the host, and `log` says so."""
    Image = _pil()
    if filter not in METHODS:
        _filter(filter)
    size = _size(target_size)
    ext = os.path.splitext(str(input_path))[1].lower()
    with Image.open(input_path) as src:
        img = src.copy()
    if ext in (".tif", ".tiff") and img.mode in ("I;16", "I;16L", "I;16B", "I;16N"):
        img = Image.fromarray(to_uint8_minmax(np.asarray(img)))
    if img.mode in ("L", "RGB"):
        out = Image.fromarray(resample_image_array(np.asarray(img), size, filter, channels=img.mode == "RGB"))
    else:
        log(f"   mode {img.mode}: resampled by Pillow on the host")
        out = img.resize(size, getattr(Image.Resampling, filter.upper()))
    _save(out, output_path, ext)
