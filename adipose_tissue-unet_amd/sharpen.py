"""The last step of the gray-image preparation: unsharp-mask sharpening.

The reference prepares a gray image in preprocess_ecm_image (pre-post-processing_tools/preprocess_small_MS_SIMs.py:
462-537): banding removal, normalisation, illumination correction, CLAHE, sharpening. illumination.py, normalization.py
and contrast.py have the first four; this module has

  sharpen_image   :434-455   img + amount * (img - GaussianBlur(img, (0, 0), sigma)), clipped and truncated to uint8
                             (--sharpen --sharpen-sigma 1.0 --sharpen-amount 0.5)

cv2 is not a dependency, so parity with cv2.GaussianBlur itself is unpinned; both paths of this module are built to the
definition below, which is exact integer arithmetic up to three float64 operations.

Input. A plane is (H, W) or (N, H, W) uint8. A float plane is rounded to nearest (half to even) and clamped to 0 .. 255
on load, the rule of contrast.py, illumination.py and normalization.py. The output is uint8, or float32 holding the same
integers. Every image of a batch is treated on its own.

Radius. n = rint(8 sigma + 1) | 1 in float64, rint half to even (cv2's ksize rule for a float image with ksize (0, 0));
r = n >> 1. sigma must be finite and > 0, and r <= RMAX = 64 (sigma up to about 16): a larger sigma is a ValueError.
r = 0 (sigma below 0.0625) makes the blur the identity.

Taps, on the host only (the device never evaluates exp):
      w_i = exp(-(i * i) / (2 sigma^2)) in float64 (math.exp), i = 0 .. r
      T   = math.fsum of the 2r + 1 symmetric values
      q_i = int(rint(w_i / T * 2^24)) for i >= 1,   q_0 = 2^24 - 2 sum_{i >= 1} q_i
    so the taps sum to exactly 2^24 and a flat image is a fixed point.

Border. BORDER_REFLECT_101 folded as often as needed: fold(p, n) = m if m < n else P - m, with the period P = 2 (n - 1)
and m = p mod P (non-negative); index 0 when the extent is 1. Images smaller than r are legal.

Blur. S(y, x) = sum_j q_|j| * sum_i q_|i| * v(fold(y + j, H), fold(x + i, W)). A row sum is at most 255 * 2^24 < 2^32
and S <= 255 * 2^48 < 2^56: exact in integers in any order.

Finish, in float64, each line one correctly rounded IEEE operation, with no contraction:
      D = v * 2^48 - S                                    (int64, exact)
      d = f64(D) * 2^-48                                  (the conversion rounds to nearest even; the scaling is exact)
      a = amount * d
      t = f64(v) + a
      out = uint8(trunc(clip(t, 0, 255)))
    amount is any finite float64; a negative amount blurs.

Deviation from the reference, stated. Its float32 taps sum to 1 +- 2^-24, so where the blur returns the pixel itself
(flat regions, sigma below about 0.3) its truncation can drop a pixel by one level; here such pixels are unchanged.
Elsewhere the two differ by float32 rounding next to an integer boundary: tests/test_sharpen.py holds this module to a
float32 restatement of the reference to within one level on at most 0.2 % of the pixels of textured images.

The device path (csrc/sharpen.hip: adp_gray_blur / adp_gray_sharpen) and the numpy path below (hosts without a GPU, and
the tests' reference) agree bit for bit.

Applied per tile (the predictor on single tiles) the border is the tile's; the sliding window sharpens a gray image
once as a whole, as the reference does before it tiles.
"""
from __future__ import annotations

import math

import numpy as np

from .components import _is_tensor, _to_device
from .contrast import _dispatch

RMAX = 64          # include/adipose_hip.h ADP_SHARP_RMAX
FUSED_RMAX = 16    # ADP_SHARP_FUSED_RMAX: up to here one launch; beyond it two, through a uint32 plane of row sums
# rows x columns of the output tile one block makes (ADP_SHARP_TILE_ROWS / _COLS): the GPU tests place their shapes
# around them
TILE_ROWS, TILE_COLS = 32, 64
ONE = 1 << 24      # the taps' sum
_D = np.float64
_WHAT = "sharpening"


# ---------------------------------------------------------------- definition: radius, taps, border
def _sigma(sigma):
    sigma = float(sigma)
    if not (math.isfinite(sigma) and sigma > 0):
        raise ValueError("sigma must be finite and > 0")
    return sigma


def _amount(amount):
    amount = float(amount)
    if not math.isfinite(amount):
        raise ValueError("amount must be finite")
    return amount


def radius(sigma):
    """r of the (2r + 1)-tap Gaussian cv2.GaussianBlur(float image, (0, 0), sigma) uses; ValueError beyond RMAX."""
    sigma = _sigma(sigma)
    r = (int(np.rint(_D(8.0) * _D(sigma) + _D(1.0))) | 1) >> 1
    if r > RMAX:
        raise ValueError(f"sigma {sigma:g} needs a blur radius of {r}; the limit is {RMAX} (sigma up to about {RMAX / 4:g})")
    return r


def taps(sigma):
    """[q_0, .., q_r]: the integer taps of the module's definition; q_0 + 2 sum q_i = 2^24."""
    sigma = _sigma(sigma)
    r = radius(sigma)
    w = [math.exp(-(i * i) / (2.0 * sigma * sigma)) for i in range(r + 1)]
    T = math.fsum(w[::-1][:-1] + w)
    q = [0] + [int(np.rint(_D(w[i]) / _D(T) * _D(ONE))) for i in range(1, r + 1)]
    q[0] = ONE - 2 * sum(q)
    return q


def fold(p, n):
    """BORDER_REFLECT_101 of index p (an int or an integer array) into 0 .. n - 1, folded as often as needed."""
    n = int(n)
    if n < 1:
        raise ValueError("fold needs an extent of at least 1")
    if n == 1:
        return p * 0
    P = 2 * (n - 1)
    m = p % P
    return np.where(m < n, m, P - m) if isinstance(m, np.ndarray) else (m if m < n else P - m)


# ---------------------------------------------------------------- numpy path
def _u8_np(img):
    a = np.asarray(img)
    if a.ndim not in (2, 3):
        raise ValueError(f"{_WHAT} takes an (H, W) or (N, H, W) gray image")
    if a.shape[-1] < 1 or a.shape[-2] < 1:
        raise ValueError(f"{_WHAT} takes an image of at least 1 x 1")
    if a.dtype == np.uint8:
        return a
    if a.dtype.kind == "f":
        return np.clip(np.rint(a), 0, 255).astype(np.uint8)
    raise TypeError(f"{_WHAT} takes uint8, or float holding 0 .. 255")


def _pass(b, q, axis):
    """sum_i q_|i| b[.. fold(k + i) ..] along `axis`, in int64."""
    r, n = len(q) - 1, b.shape[axis]
    p = np.take(b, fold(np.arange(-r, n + r), n), axis=axis)
    out = q[0] * np.take(p, np.arange(r, r + n), axis=axis)
    for i in range(1, r + 1):
        out += q[i] * (np.take(p, np.arange(r - i, r - i + n), axis=axis) + np.take(p, np.arange(r + i, r + i + n), axis=axis))
    return out


def blur_sum_np(img, sigma):
    """(H, W) or (N, H, W) -> S of the module's definition, int64 of the same shape."""
    a = _u8_np(img)
    q = taps(sigma)
    return _pass(_pass(a.astype(np.int64), q, a.ndim - 1), q, a.ndim - 2)


def sharpen_np(img, sigma=1.0, amount=0.5, dtype=np.uint8):
    """sharpen_image by the module's definition, in `dtype`."""
    a = _u8_np(img)
    amount = _D(_amount(amount))
    v = a.astype(np.int64)
    D = v * (1 << 48) - blur_sum_np(a, sigma)
    d = D.astype(_D) * _D(2.0 ** -48)
    t = amount * d
    t = v.astype(_D) + t
    return np.clip(t, 0.0, 255.0).astype(np.uint8).astype(dtype, copy=False)   # truncates


# ---------------------------------------------------------------- device path
def _src(t):
    """A host array or a tensor -> (contiguous device tensor uint8 | float32, its f32 flag, N, H, W)."""
    import torch
    m = _to_device(t)
    if m.dim() not in (2, 3):
        raise ValueError(f"{_WHAT} takes an (H, W) or (N, H, W) gray image")
    if m.shape[-1] < 1 or m.shape[-2] < 1:
        raise ValueError(f"{_WHAT} takes an image of at least 1 x 1")
    if m.dtype not in (torch.uint8, torch.float32):
        if not m.dtype.is_floating_point:
            raise TypeError(f"{_WHAT} takes uint8, or float holding 0 .. 255")
        m = m.to(torch.float32)
    m = m.contiguous()
    N = 1 if m.dim() == 2 else int(m.shape[0])
    return m, int(m.dtype == torch.float32), N, int(m.shape[-2]), int(m.shape[-1])


def _rowbuf(rowbuf, r, m, N, H, W):
    """The uint32 (N, H, W) plane of row sums the two-launch form needs (an int32 tensor: the same bits), or None."""
    import torch
    if r <= FUSED_RMAX or N == 0:
        return None
    if rowbuf is None:
        return torch.empty((N, H, W), dtype=torch.int32, device=m.device)
    if not (_is_tensor(rowbuf) and rowbuf.is_cuda and rowbuf.device == m.device and rowbuf.dtype == torch.int32
            and rowbuf.is_contiguous() and rowbuf.numel() >= N * H * W):
        raise ValueError("rowbuf must be a contiguous int32 tensor of at least N * H * W elements on the image's device")
    return rowbuf


def _taps_arg(q):
    import ctypes as C
    return (C.c_uint32 * len(q))(*q)


def blur_sum(t, sigma, rowbuf=None):
    """blur_sum_np on the device: an int64 device tensor of the input's shape. Runs on the current stream, no
    synchronisation; `rowbuf` as in sharpen()."""
    import torch

    from ._lib import call, ptr, stream_ptr
    q = taps(sigma)
    m, f32, N, H, W = _src(t)
    out = torch.empty(m.shape, dtype=torch.int64, device=m.device)
    if N:
        rb = _rowbuf(rowbuf, len(q) - 1, m, N, H, W)
        with torch.cuda.device(m.device):
            call("adp_gray_blur", N, H, W, ptr(m), f32, _taps_arg(q), len(q) - 1, ptr(rb), ptr(out), stream_ptr())
    return out


def sharpen(t, sigma=1.0, amount=0.5, dtype=None, rowbuf=None):
    """sharpen_np on the device: (H, W) or (N, H, W) uint8 or float32 (rounded and clamped on load) -> a device tensor of
    the same shape, uint8 or float32 (default: the input's dtype) holding the same integers. A host array is uploaded.
    One launch for a radius up to FUSED_RMAX; two beyond it, through `rowbuf`, an int32 tensor of N * H * W elements
    (allocated here when None). Runs on the current stream, no synchronisation."""
    import torch

    from ._lib import call, ptr, stream_ptr
    q = taps(sigma)
    amount = _amount(amount)
    m, f32, N, H, W = _src(t)
    dtype = dtype or m.dtype
    if dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"{_WHAT} writes uint8 or float32")
    out = torch.empty(m.shape, dtype=dtype, device=m.device)
    if N:
        rb = _rowbuf(rowbuf, len(q) - 1, m, N, H, W)
        with torch.cuda.device(m.device):
            call("adp_gray_sharpen", N, H, W, ptr(m), f32, _taps_arg(q), len(q) - 1, amount, ptr(rb), ptr(out),
                 int(dtype == torch.float32), stream_ptr())
    return out


# ---------------------------------------------------------------- the reference's surface
def sharpen_image(img, sigma=1.0, amount=0.5):
    """preprocess_small_MS_SIMs.py:434-455 on an (H, W) or (N, H, W) gray image, in the input's dtype (uint8, or float
    holding the integers) and container: array in, array out; tensor in, tensor out on the same device; the device
    where there is one."""
    radius(sigma)
    amount = _amount(amount)
    if _is_tensor(img):
        return _dispatch(img, lambda a: sharpen_np(a, sigma, amount, a.dtype), lambda t: sharpen(t, sigma, amount))
    a = np.asarray(img)
    dt = a.dtype if a.dtype.kind == "f" else np.uint8
    return _dispatch(a, lambda v: sharpen_np(v, sigma, amount, dt),
                     lambda v: sharpen(v.astype(np.float32) if dt != np.uint8 else v, sigma, amount)).astype(dt, copy=False)


class UnsharpMask:
    """sharpen_image with preprocess_small_MS_SIMs.py's defaults (--sharpen-sigma 1.0, --sharpen-amount 0.5); call it on
    a gray image or a batch. sigma and amount are checked here."""

    def __init__(self, sigma=1.0, amount=0.5):
        self.sigma = _sigma(sigma)
        self.amount = _amount(amount)
        self.radius = radius(self.sigma)

    def __call__(self, img):
        return sharpen_image(img, self.sigma, self.amount)

    def __repr__(self):
        return f"UnsharpMask(sigma={self.sigma}, amount={self.amount})"
