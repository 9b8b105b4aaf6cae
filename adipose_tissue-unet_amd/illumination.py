"""Gray-scale (flat) morphology of 8-bit gray images, and the background corrections built on it.

The reference prepares a gray image before --enhance-contrast (contrast.py) in three functions of
pre-post-processing_tools/preprocess_small_MS_SIMs.py, all called from preprocess_ecm_image:

  remove_banding_morphological        :217-246   opening by a kernel_height x kernel_width rectangle (512 x 1), then
                                                 img - background + mean(background)      (--banding-method morphological)
  correct_illumination_rolling_ball   :293-326   opening by a disc of `radius` (100), the same subtraction
                                                                                          (--illumination-method rolling-ball)
  correct_illumination_tophat         :357-390   white top-hat by cv2's ellipse of kernel_size (301), then
                                                 img + 0.5 * tophat                       (--illumination-method tophat)

cv2 is not a dependency, so parity with cv2 itself is unpinned; both paths of this module are built to the definitions
below, and the tests pin them to oracle/numpy_ref.py's cv_ellipse_rows / cv_morph and, where it is installed, scipy.

Footprint. kh rows of column extents [lo[a], hi[a]) in a box kw wide, written (lo, hi) for a square box (kw = kh) or
(lo, hi, kw). The anchor is (cy, cx) = (kh // 2, kw // 2), cv2's default. 0 <= lo[a] <= hi[a] <= kw; a row may be
empty. 1 <= kh, kw <= KMAX = 513: the reference's defaults and documented ranges fit (the 512 x 1 line, the 301
ellipse, a 401 disc).

  erode(M)(y, x)  = min over rows a, lo[a] <= b < hi[a], of M(y + a - cy, x + b - cx)
  dilate(M)(y, x) = max over the same offsets (not the reflected ones)
  open = dilate(erode(M))        close = erode(dilate(M))
  tophat = saturate_u8(M - open(M))      blackhat = saturate_u8(close(M) - M)

Positions outside the image take no part (OpenCV's default morphology border, as in morphology.py and cv_morph). An
empty footprint erodes to 255 and dilates to 0. For even sizes the offsets are asymmetric, so opening is not
anti-extensive; that is cv2's behaviour and is kept, hence the saturation in the two hats. A footprint may be larger
than the image: a 301 ellipse on a 256 x 256 tile is an ordinary call.

Constructors. ellipse_rows(k): cv2.getStructuringElement(MORPH_ELLIPSE, (k, k)), the formula of
morphology.footprint_rows without that module's limit of 63. rect_rows(kh, kw). disc_rows(radius): kh = kw = 2 r + 1 and
row a spans r +- isqrt(r^2 - (a - r)^2), which equals the reference's np.sqrt(x**2 + y**2) <= radius.

Corrections, for a u8 plane v:

  subtract_background(v, bg): S = the exact integer sum of bg over the image, n = H * W,
      mean32 = float32(float64(S) / float64(n)),
      out = uint8(trunc(clip(float32(int(v) - int(bg)) + mean32, 0, 255)))
    one float32 addition; the integer difference is exact. The reference's bg_float.mean() is numpy's pairwise float32
    sum, which is inexact once the sum passes 2^24 (beyond about 65 793 pixels of 255); this is the correctly rounded
    mean instead.
  rolling_ball(v, radius=100)                                      = subtract_background(v, open(v, disc_rows(radius)))
  remove_banding_morphological(v, kernel_width=1, kernel_height=512) = the same with rect_rows(kernel_height, kernel_width)
  tophat_correction(v, kernel_size=301): an even size is bumped to the next odd, as the reference does;
      out = uint8(trunc(clip(float32(v) + float32(tophat(v, ellipse_rows(k))) * 0.5f, 0, 255)))
    every step is exact in float32.

Input conversion. A float32 plane is rounded to nearest (half to even) and clamped to 0 .. 255 on load, the rule
contrast.py uses. The output is uint8, or float32 holding the same integers.

Everything is integers or single exact float32 operations, so the device path (csrc/graymorph.hip: adp_gray_morph /
adp_gray_bgsum / adp_illum_finish) and the numpy path below (hosts without a GPU, and the tests' reference) agree bit
for bit. Both decompose the footprint by rows: erode(y, x) = min over a of the horizontal window minimum of row
y + a - cy over [x + lo[a] - cx, x + hi[a] - cx), and a window minimum of length L is two reads of a table of
power-of-two windows, min(P_e[s], P_e[s + L - 2^e]) with e = floor(log2 L).

Applied per tile (the predictor on single tiles), a correction differs from the correction of the whole image within a
footprint radius of the tile's edges, and its background mean is the tile's; the sliding window corrects a gray image
once as a whole, as the reference does before it tiles.
"""
from __future__ import annotations

import math

import numpy as np

from .components import _is_tensor, _on_device, _to_device
from .contrast import _dispatch

ERODE, DILATE = 0, 1
KMAX = 513
# pixels a block of adp_gray_morph produces (include/adipose_hip.h ADP_GMORPH_TILE_ROWS / _COLS): the GPU tests place
# their shapes around them
TILE_ROWS, TILE_COLS = 64, 256
SUBTRACT_MEAN, TOPHAT_HALF, DIFF = 0, 1, 2
METHODS = (None, "rolling-ball", "tophat")
_F = np.float32


# ---------------------------------------------------------------- footprints
def _size(k, what="the footprint size"):
    k = int(k)
    if not 1 <= k <= KMAX:
        raise ValueError(f"{what} must be in 1 .. {KMAX}")
    return k


def ellipse_rows(k):
    """cv2.getStructuringElement(MORPH_ELLIPSE, (k, k)) as (lo, hi): r = c = k // 2, row a spans c +- rint(c * sqrt((r^2 -
    (a - r)^2) / r^2)) (saturate_cast rounds half to even), clipped to the box."""
    k = _size(k)
    r = c = k // 2
    inv_r2 = 1.0 / (r * r) if r else 0.0
    lo, hi = [], []
    for a in range(k):
        dy = a - r
        dx = int(np.rint(c * math.sqrt((r * r - dy * dy) * inv_r2)))
        lo.append(max(c - dx, 0))
        hi.append(min(c + dx + 1, k))
    return lo, hi


def rect_rows(kh, kw):
    """The kh x kw rectangle as (lo, hi, kw)."""
    kh, kw = _size(kh, "the footprint height"), _size(kw, "the footprint width")
    return [0] * kh, [kw] * kh, kw


def disc_rows(radius):
    """The disc x^2 + y^2 <= radius^2 in its (2 r + 1)-box as (lo, hi)."""
    r = int(radius)
    if r < 0:
        raise ValueError("the radius must be at least 0")
    _size(2 * r + 1, "the disc's size 2 * radius + 1")
    d = [math.isqrt(r * r - (a - r) * (a - r)) for a in range(2 * r + 1)]
    return [r - v for v in d], [r + v + 1 for v in d]


def footprint_array(rows):
    """A footprint -> its kh x kw uint8 array."""
    lo, hi, kw = _check_rows(rows)
    se = np.zeros((len(lo), kw), np.uint8)
    for a in range(len(lo)):
        se[a, lo[a]:hi[a]] = 1
    return se


def _check_rows(rows):
    if len(rows) not in (2, 3):
        raise ValueError("a footprint is (lo, hi) or (lo, hi, kw)")
    lo, hi = [int(v) for v in rows[0]], [int(v) for v in rows[1]]
    kh = len(lo)
    kw = int(rows[2]) if len(rows) == 3 else kh
    if len(hi) != kh or not (1 <= kh <= KMAX and 1 <= kw <= KMAX):
        raise ValueError(f"a footprint has 1 .. {KMAX} rows of (lo, hi) in a box 1 .. {KMAX} wide")
    if any(not 0 <= l <= h <= kw for l, h in zip(lo, hi)):
        raise ValueError("a footprint row needs 0 <= lo <= hi <= kw")
    return lo, hi, kw


# ---------------------------------------------------------------- numpy path
def _u8_np(img):
    a = np.asarray(img)
    if a.ndim not in (2, 3):
        raise ValueError("gray morphology takes an (H, W) or (N, H, W) gray image")
    if a.dtype == np.uint8:
        return a
    if a.dtype.kind == "f":
        return np.clip(np.rint(a), 0, 255).astype(np.uint8)
    raise TypeError("gray morphology takes uint8, or float holding 0 .. 255")


def _morph_u8(b, rows, maxop):
    """Erosion (dilation if maxop) of (N, H, W) uint8 by the checked footprint, by rows: the levels P_e of the padded
    image once, then two shifted views per footprint row."""
    lo, hi, kw = rows
    kh = len(lo)
    N, H, W = b.shape
    ident = 0 if maxop else 255
    f = np.maximum if maxop else np.minimum
    out = np.full(b.shape, ident, np.uint8)
    lens = [h - l for l, h in zip(lo, hi)]
    if N == 0 or max(lens) == 0:
        return out
    pad = np.full((N, H + kh - 1, W + kw - 1), ident, np.uint8)   # padded row y + a, column x + b: offset (a, b) of (y, x)
    pad[:, kh // 2:kh // 2 + H, kw // 2:kw // 2 + W] = b
    levels = [pad]
    for e in range(1, max(lens).bit_length()):
        h = 1 << (e - 1)
        nxt = levels[-1].copy()
        f(nxt[..., :-h], levels[-1][..., h:], out=nxt[..., :-h])
        levels.append(nxt)
    tmp = np.empty_like(out)
    for a in range(kh):
        if lens[a] == 0:
            continue
        e = lens[a].bit_length() - 1
        p = levels[e][:, a:a + H]
        s2 = hi[a] - (1 << e)
        f(p[..., lo[a]:lo[a] + W], p[..., s2:s2 + W], out=tmp)
        f(out, tmp, out=out)
    return out


def _np_steps(img, rows, steps, dtype):
    rows = _check_rows(rows)
    a = _u8_np(img)
    b = a.reshape((-1,) + a.shape[-2:])
    for maxop in steps:
        b = _morph_u8(b, rows, maxop)
    return b.reshape(a.shape).astype(dtype, copy=False)


def erode_np(img, rows, dtype=np.uint8):
    """Erosion of an (H, W) or (N, H, W) gray image (uint8, or float rounded and clamped on load) by the footprint
    `rows`, in `dtype`."""
    return _np_steps(img, rows, (False,), dtype)


def dilate_np(img, rows, dtype=np.uint8):
    return _np_steps(img, rows, (True,), dtype)


def open_np(img, rows, dtype=np.uint8):
    return _np_steps(img, rows, (False, True), dtype)


def close_np(img, rows, dtype=np.uint8):
    return _np_steps(img, rows, (True, False), dtype)


def tophat_np(img, rows, dtype=np.uint8):
    a = _u8_np(img)
    return np.maximum(a.astype(np.int16) - open_np(a, rows), 0).astype(dtype)


def blackhat_np(img, rows, dtype=np.uint8):
    a = _u8_np(img)
    return np.maximum(close_np(a, rows).astype(np.int16) - a, 0).astype(dtype)


def subtract_background_np(img, bg, dtype=np.uint8):
    """img - bg + mean(bg) per image by the module's definition; bg uint8 of img's shape."""
    a, g = _u8_np(img), np.asarray(bg)
    if g.dtype != np.uint8 or g.shape != a.shape:
        raise ValueError("the background is a uint8 plane of the image's shape")
    v, b = a.reshape((-1,) + a.shape[-2:]), g.reshape((-1,) + a.shape[-2:])
    out = np.empty(v.shape, dtype)
    n = v.shape[1] * v.shape[2]
    for i in range(v.shape[0]):
        mean32 = _F(np.float64(int(b[i].sum(dtype=np.int64))) / np.float64(n))
        out[i] = np.clip((v[i].astype(np.int32) - b[i]).astype(_F) + mean32, _F(0), _F(255)).astype(np.uint8)   # truncates
    return out.reshape(a.shape)


def _odd(kernel_size):
    k = int(kernel_size)
    return k + 1 if k % 2 == 0 else k


def rolling_ball_np(img, radius=100, dtype=np.uint8):
    a = _u8_np(img)
    return subtract_background_np(a, open_np(a, disc_rows(radius)), dtype)


def remove_banding_morphological_np(img, kernel_width=1, kernel_height=512, dtype=np.uint8):
    a = _u8_np(img)
    return subtract_background_np(a, open_np(a, rect_rows(kernel_height, kernel_width)), dtype)


def tophat_correction_np(img, kernel_size=301, dtype=np.uint8):
    a = _u8_np(img)
    th = tophat_np(a, ellipse_rows(_odd(kernel_size)))
    return np.clip(a.astype(_F) + th.astype(_F) * _F(0.5), _F(0), _F(255)).astype(np.uint8).astype(dtype)   # truncates


# ---------------------------------------------------------------- device path
def _src(t):
    """A host array or a tensor -> (contiguous device tensor uint8 | float32, its f32 flag, N, H, W)."""
    import torch
    m = _to_device(t)
    if m.dim() not in (2, 3):
        raise ValueError("gray morphology takes an (H, W) or (N, H, W) gray image")
    if m.dtype not in (torch.uint8, torch.float32):
        if not m.dtype.is_floating_point:
            raise TypeError("gray morphology takes uint8, or float holding 0 .. 255")
        m = m.to(torch.float32)
    m = m.contiguous()
    N = 1 if m.dim() == 2 else int(m.shape[0])
    return m, int(m.dtype == torch.float32), N, int(m.shape[-2]), int(m.shape[-1])


def _out_dtype(dtype, m):
    import torch
    dtype = dtype or m.dtype
    if dtype not in (torch.uint8, torch.float32):
        raise TypeError("gray morphology writes uint8 or float32")
    return dtype


def _u8(m, f32):
    """The uint8 plane a float32 plane is loaded as."""
    import torch
    return m.round().clamp_(0, 255).to(torch.uint8) if f32 else m


def _gray_morph(m, f32, rows, op):
    """One adp_gray_morph launch on the current stream: (N, H, W) or (H, W) device plane -> a new uint8 plane."""
    import ctypes as C

    import torch

    from ._lib import call, ptr, stream_ptr
    lo, hi, kw = rows
    kh = len(lo)
    out = torch.empty(m.shape, dtype=torch.uint8, device=m.device)
    if m.numel():
        N = 1 if m.dim() == 2 else int(m.shape[0])
        with torch.cuda.device(m.device):
            call("adp_gray_morph", N, int(m.shape[-2]), int(m.shape[-1]), ptr(m), f32, ptr(out), kh, kw,
                 (C.c_int * kh)(*lo), (C.c_int * kh)(*hi), op, stream_ptr())
    return out


def _dev_steps(t, rows, steps):
    rows = _check_rows(rows)
    m, f32, _, _, _ = _src(t)
    for op in steps:
        m, f32 = _gray_morph(m, f32, rows, op), 0
    return m


def _finish(v, v_f32, b, sums, mode, dtype):
    import torch

    from ._lib import call, ptr, stream_ptr
    out = torch.empty(v.shape, dtype=dtype, device=v.device)
    if v.numel():
        N = 1 if v.dim() == 2 else int(v.shape[0])
        with torch.cuda.device(v.device):
            call("adp_illum_finish", N, int(v.shape[-2]), int(v.shape[-1]), ptr(v), v_f32, ptr(b), ptr(sums), mode, ptr(out),
                 int(dtype == torch.float32), stream_ptr())
    return out


def _as(out, dtype):
    return out if out.dtype == dtype else out.to(dtype)


def erode(t, rows, dtype=None):
    """erode_np on the device: (H, W) or (N, H, W) uint8 or float32 (rounded and clamped on load) -> a device tensor of
    the same shape, uint8 or float32 (default: the input's dtype) holding the same integers. A host array is uploaded.
    One launch per morphological step on the current stream, no synchronisation."""
    m = _src(t)[0]
    return _as(_dev_steps(m, rows, (ERODE,)), _out_dtype(dtype, m))


def dilate(t, rows, dtype=None):
    m = _src(t)[0]
    return _as(_dev_steps(m, rows, (DILATE,)), _out_dtype(dtype, m))


def open(t, rows, dtype=None):   # noqa: A001 (the operation's name)
    m = _src(t)[0]
    return _as(_dev_steps(m, rows, (ERODE, DILATE)), _out_dtype(dtype, m))


def close(t, rows, dtype=None):
    m = _src(t)[0]
    return _as(_dev_steps(m, rows, (DILATE, ERODE)), _out_dtype(dtype, m))


def tophat(t, rows, dtype=None):
    m, f32, _, _, _ = _src(t)
    return _finish(m, f32, _dev_steps(m, rows, (ERODE, DILATE)), None, DIFF, _out_dtype(dtype, m))


def blackhat(t, rows, dtype=None):
    m, f32, _, _, _ = _src(t)
    return _finish(_dev_steps(m, rows, (DILATE, ERODE)), 0, _u8(m, f32), None, DIFF, _out_dtype(dtype, m))


def background_sum(bg):
    """(N,) int64 device tensor: the exact sum of every image of the uint8 device plane bg (adp_gray_bgsum)."""
    import torch

    from ._lib import call, ptr, stream_ptr
    if not (_is_tensor(bg) and bg.is_cuda and bg.dtype == torch.uint8 and bg.dim() in (2, 3)):
        raise TypeError("the background is a uint8 device plane (H, W) or (N, H, W)")
    g = bg.contiguous()
    N = 1 if g.dim() == 2 else int(g.shape[0])
    sums = torch.empty((N,), dtype=torch.int64, device=g.device)
    if g.numel():
        with torch.cuda.device(g.device):
            call("adp_gray_bgsum", N, int(g.shape[-2]), int(g.shape[-1]), ptr(g), ptr(sums), stream_ptr())
    return sums


def subtract_background(t, bg, dtype=None):
    """subtract_background_np on the device; the mean is formed on the device from the integer sum (no host sync)."""
    import torch
    m, f32, _, _, _ = _src(t)
    g = _to_device(bg)
    if g.dtype != torch.uint8 or g.shape != m.shape:
        raise ValueError("the background is a uint8 plane of the image's shape")
    g = g.contiguous()
    return _finish(m, f32, g, background_sum(g), SUBTRACT_MEAN, _out_dtype(dtype, m))


def rolling_ball(t, radius=100, dtype=None):
    m = _src(t)[0]
    return subtract_background(m, _dev_steps(m, disc_rows(radius), (ERODE, DILATE)), dtype)


def remove_banding_morphological(t, kernel_width=1, kernel_height=512, dtype=None):
    m = _src(t)[0]
    return subtract_background(m, _dev_steps(m, rect_rows(kernel_height, kernel_width), (ERODE, DILATE)), dtype)


def tophat_correction(t, kernel_size=301, dtype=None):
    m, f32, _, _, _ = _src(t)
    opened = _dev_steps(m, ellipse_rows(_odd(kernel_size)), (ERODE, DILATE))
    return _finish(m, f32, opened, None, TOPHAT_HALF, _out_dtype(dtype, m))


# ---------------------------------------------------------------- the reference's surface
def _apply(img, np_fn, dev_fn):
    """A correction in the input's dtype (uint8, or float holding the integers) and container: array in, array out;
    tensor in, tensor out on the same device; the device where there is one."""
    if _is_tensor(img):
        return _dispatch(img, lambda a: np_fn(a, a.dtype), dev_fn)
    a = np.asarray(img)
    dt = a.dtype if a.dtype.kind == "f" else np.uint8
    return _dispatch(a, lambda v: np_fn(v, dt),
                     lambda v: dev_fn(v.astype(np.float32) if dt != np.uint8 else v)).astype(dt, copy=False)


def correct_illumination_rolling_ball(img, radius=100):
    """preprocess_small_MS_SIMs.py:293-326 on an (H, W) or (N, H, W) gray image, array or tensor."""
    disc_rows(radius)
    return _apply(img, lambda a, dt: rolling_ball_np(a, radius, dt), lambda t: rolling_ball(t, radius))


def correct_illumination_tophat(img, kernel_size=301):
    """preprocess_small_MS_SIMs.py:357-390."""
    ellipse_rows(_odd(kernel_size))
    return _apply(img, lambda a, dt: tophat_correction_np(a, kernel_size, dt), lambda t: tophat_correction(t, kernel_size))


def remove_banding(img, kernel_width=1, kernel_height=512):
    """preprocess_small_MS_SIMs.py:217-246 (remove_banding_morphological)."""
    rect_rows(kernel_height, kernel_width)
    return _apply(img, lambda a, dt: remove_banding_morphological_np(a, kernel_width, kernel_height, dt),
                  lambda t: remove_banding_morphological(t, kernel_width, kernel_height))


class IlluminationCorrection:
    """preprocess_ecm_image's background steps in its order: banding removal (banding = (width, height) of the opening's
    rectangle, or None), then the illumination method (None, "rolling-ball" with `radius`, or "tophat" with
    `kernel_size`). Call it on a gray image or a batch, array or tensor."""

    def __init__(self, banding=None, method=None, radius=100, kernel_size=301):
        if method in ("none", ""):
            method = None
        if method not in METHODS:
            raise ValueError("method must be None, 'rolling-ball' or 'tophat'")
        self.banding = None if banding is None else (int(banding[0]), int(banding[1]))
        self.method = method
        self.radius = int(radius)
        self.kernel_size = int(kernel_size)
        if self.banding is not None:
            rect_rows(self.banding[1], self.banding[0])
        if method == "rolling-ball":
            disc_rows(self.radius)
        if method == "tophat":
            if self.kernel_size < 1:
                raise ValueError("kernel_size must be at least 1")
            ellipse_rows(_odd(self.kernel_size))

    def remove_banding(self, img):
        """The banding step alone (the reference normalises between it and the illumination step: normalization.py)."""
        if self.banding is not None:
            img = remove_banding(img, self.banding[0], self.banding[1])
        return img

    def correct(self, img):
        """The illumination step alone."""
        if self.method == "rolling-ball":
            img = correct_illumination_rolling_ball(img, self.radius)
        elif self.method == "tophat":
            img = correct_illumination_tophat(img, self.kernel_size)
        return img

    def __call__(self, img):
        return self.correct(self.remove_banding(img))

    def __repr__(self):
        return (f"IlluminationCorrection(banding={self.banding}, method={self.method!r}, radius={self.radius}, "
                f"kernel_size={self.kernel_size})")
