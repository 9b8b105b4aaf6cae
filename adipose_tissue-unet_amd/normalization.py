"""The statistical steps of the gray-image preparation: column de-banding, z-score and percentile stretch.

The reference prepares a gray image in preprocess_ecm_image (pre-post-processing_tools/preprocess_small_MS_SIMs.py:
462-537): banding removal, normalisation, illumination correction, CLAHE, sharpening. illumination.py has the
morphological banding removal and the illumination step, contrast.py has CLAHE, sharpen.py the sharpening; this module has

  remove_banding_column_normalize   :249-286   every column to zero mean and unit deviation, then back to the image's
                                               mean and deviation, or to 0 .. 255          (--banding-method column)
  normalize_zscore                  :92-114    (v - mean) / std, +-3 deviations to 0 .. 255  (--normalization-method zscore)
  normalize_percentile              :117-138   the p_low .. p_high percentiles to 0 .. 255   (--normalization-method percentile)

Input. A plane is (H, W) or (N, H, W) uint8. A float32 plane is rounded to nearest (half to even) and clamped to
0 .. 255 on load, the rule of contrast.py and illumination.py. The output is uint8, or float32 holding the same
integers. Every image of a batch is treated on its own.

Arithmetic. All floating-point arithmetic is float64; every operation written below is one correctly rounded IEEE
operation in the order written, with no contraction.

  stats(S1, S2, n), for the exact integer sums S1 = sum v, S2 = sum v^2 over n values:
      mean = f64(S1) / f64(n),  ex2 = f64(S2) / f64(n),  std = sqrt(max(ex2 - mean * mean, 0))
    the population deviation (numpy's .std()). S2 < 2^53 for any image with H * W < 2^31, so the conversions are exact.

  column_normalize(v, preserve_global=True). Per column x: S1_x, S2_x, vmin_x, vmax_x over the H rows;
      (cm_x, cs_x) = stats(S1_x, S2_x, H),  d_x = cs_x + 1e-10,  (gm, gs) = stats(sum S1_x, sum S2_x, H * W)
      t = (f64(v) - cm_x) / d_x
      preserve_global:  t = t * gs + gm                                  (two operations)
      otherwise:        lo = min over x of (f64(vmin_x) - cm_x) / d_x,  hi = max over x of (f64(vmax_x) - cm_x) / d_x
                        (the image's minimum and maximum of t: the map is increasing in v within a column)
                        t = ((t - lo) / ((hi - lo) + 1e-10)) * 255.0
      out = uint8(trunc(clip(t, 0, 255)))
    A constant column gives t = 0 before the rescale.

  zscore(v). From the image's 256-bin histogram h: S1 = sum i h[i], S2 = sum i^2 h[i], n = sum h[i];
      (mean, std) = stats(S1, S2, n)
      table[i] = uint8(trunc(clip((((f64(i) - mean) / (std + 1e-10)) + 3.0) / 6.0 * 255.0, 0, 255))),  out = table[v]

  percentile(v, p_low=1.0, p_high=99.0), 0 <= p_low <= p_high <= 100:
      (lo, hi) = contrast.hist_percentiles(h, p_low, p_high)   (np.percentile's "linear" method, exactly, from h)
      scale = max(hi - lo, 1e-3)
      table[i] = uint8(trunc(clip((f64(i) - lo) / scale, 0, 1) * 255.0)),  out = table[v]

The reference computes the same formulas in float32, and its numpy float32 means are inexact on large images, so parity
with it is to within one gray level, not bit for bit (tests/test_normalization.py holds both to one level on at most
0.2 % of the pixels). The device path (csrc/graynorm.hip: adp_gray_colstats / adp_gray_colparams / adp_gray_colnorm /
adp_gray_normalize, and adp_clahe_hist for the histogram) and the numpy path below (hosts without a GPU, and the tests'
reference) agree bit for bit.

augment.py has normalize_zscore / normalize_percentile too: those are the training feed's, which return float images
(zero mean and unit deviation; 0 .. 1). The functions of those names here are the preparation script's, which return
8-bit images in the input's dtype.

Applied per tile (the predictor on single tiles) the statistics are the tile's; the sliding window normalises a gray
image once as a whole, as the reference does before it tiles.
"""
from __future__ import annotations

import numpy as np

from .components import _is_tensor, _to_device
from .contrast import _dispatch, hist_percentiles

# rows x columns of the plane that one block of adp_gray_colstats reduces (include/adipose_hip.h ADP_GNORM_BAND_ROWS /
# _COLS): the GPU tests place their shapes around them
BAND_ROWS, BAND_COLS = 64, 256
# beyond TALL_BLOCKS such blocks per call a block of the 16-byte path takes TALL_FACTOR bands of rows
# (ADP_GNORM_TALL_BLOCKS / _FACTOR)
TALL_BLOCKS, TALL_FACTOR = 1024, 4
ZSCORE, PERCENTILE = 0, 1
METHODS = (None, "percentile", "zscore")
_D = np.float64
_WHAT = "gray normalisation"


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


def _percentiles(p_low, p_high):
    p_low, p_high = float(p_low), float(p_high)
    if not 0.0 <= p_low <= p_high <= 100.0:
        raise ValueError("the percentiles need 0 <= p_low <= p_high <= 100")
    return p_low, p_high


def _stats(S1, S2, n):
    """(mean, std) float64 from exact integer sums (int64 arrays or ints below 2^53) over n values."""
    n = _D(n)
    mean = np.asarray(S1).astype(_D) / n
    ex2 = np.asarray(S2).astype(_D) / n
    return mean, np.sqrt(np.maximum(ex2 - mean * mean, _D(0)))


def column_stats_np(img):
    """(H, W) or (N, H, W) -> (col, glob): col (W, 2) or (N, W, 2) float64 {cm, d} per column and glob (4,) or (N, 4)
    float64 {gm, gs, lo, hi} per image, by the module's definition."""
    a = _u8_np(img)
    b = a.reshape((-1,) + a.shape[-2:]).astype(np.int64)
    N, H, W = b.shape
    S1, S2 = b.sum(axis=1), (b * b).sum(axis=1)
    cm, cs = _stats(S1, S2, H)
    d = cs + _D(1e-10)
    gm, gs = _stats(S1.sum(axis=1), S2.sum(axis=1), H * W)
    if N:
        lo = ((b.min(axis=1).astype(_D) - cm) / d).min(axis=1)
        hi = ((b.max(axis=1).astype(_D) - cm) / d).max(axis=1)
    else:
        lo = hi = np.zeros((0,), _D)
    col, glob = np.stack([cm, d], axis=-1), np.stack([gm, gs, lo, hi], axis=-1)
    return (col[0], glob[0]) if a.ndim == 2 else (col, glob)


def column_normalize_np(img, preserve_global=True, dtype=np.uint8):
    """remove_banding_column_normalize by the module's definition, in `dtype`."""
    a = _u8_np(img)
    b = a.reshape((-1,) + a.shape[-2:])
    col, glob = column_stats_np(b)
    out = np.empty(b.shape, dtype)
    for n in range(b.shape[0]):
        t = (b[n].astype(_D) - col[n, :, 0][None, :]) / col[n, :, 1][None, :]
        gm, gs, lo, hi = glob[n]
        if preserve_global:
            t = t * gs
            t = t + gm
        else:
            t = ((t - lo) / ((hi - lo) + _D(1e-10))) * _D(255)
        out[n] = np.clip(t, 0.0, 255.0).astype(np.uint8)   # truncates
    return out.reshape(a.shape)


def zscore_table(hist):
    """The 256-entry uint8 table of the z-score stretch from a 256-bin histogram."""
    h = [int(v) for v in np.asarray(hist).ravel()]
    n = sum(h)
    mean, std = _stats(sum(i * c for i, c in enumerate(h)), sum(i * i * c for i, c in enumerate(h)), max(n, 1))
    t = (np.arange(256, dtype=_D) - mean) / (std + _D(1e-10))
    t = t + _D(3)
    t = t / _D(6)
    t = t * _D(255)
    return np.clip(t, 0.0, 255.0).astype(np.uint8)


def percentile_table(hist, p_low=1.0, p_high=99.0):
    """The 256-entry uint8 table of the percentile stretch from a 256-bin histogram."""
    lo, hi = hist_percentiles(hist, p_low, p_high)
    scale = max(hi - lo, _D(1e-3))
    return (np.clip((np.arange(256, dtype=_D) - lo) / scale, 0.0, 1.0) * _D(255)).astype(np.uint8)


def _table_np(img, table_of, dtype):
    a = _u8_np(img)
    b = a.reshape((-1,) + a.shape[-2:])
    out = np.empty(b.shape, dtype)
    for n in range(b.shape[0]):
        out[n] = table_of(np.bincount(b[n].ravel(), minlength=256))[b[n]]
    return out.reshape(a.shape)


def normalize_zscore_np(img, dtype=np.uint8):
    return _table_np(img, zscore_table, dtype)


def normalize_percentile_np(img, p_low=1.0, p_high=99.0, dtype=np.uint8):
    p_low, p_high = _percentiles(p_low, p_high)
    return _table_np(img, lambda h: percentile_table(h, p_low, p_high), dtype)


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


def _out_dtype(dtype, m):
    import torch
    dtype = dtype or m.dtype
    if dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"{_WHAT} writes uint8 or float32")
    return dtype


def _column_stats(m, f32, N, H, W):
    import torch

    from ._lib import call, ptr, stream_ptr
    lead = tuple(m.shape[:-2])
    col = torch.empty(lead + (W, 2), dtype=torch.float64, device=m.device)
    glob = torch.empty(lead + (4,), dtype=torch.float64, device=m.device)
    if N:
        sums = torch.empty((N, W, 2), dtype=torch.int64, device=m.device)
        minmax = torch.empty((N, W, 2), dtype=torch.int32, device=m.device)   # uint32 bits
        with torch.cuda.device(m.device):
            call("adp_gray_colstats", N, H, W, ptr(m), f32, ptr(sums), ptr(minmax), stream_ptr())
            call("adp_gray_colparams", N, H, W, ptr(sums), ptr(minmax), ptr(col), ptr(glob), stream_ptr())
    return col, glob


def column_stats(t):
    """column_stats_np on the device: the two float64 device tensors (col, glob). Two launches (and the small one that
    initialises the integer sums) on the current stream, no synchronisation."""
    return _column_stats(*_src(t))


def column_normalize(t, preserve_global=True, dtype=None):
    """column_normalize_np on the device: (H, W) or (N, H, W) uint8 or float32 (rounded and clamped on load) -> a device
    tensor of the same shape, uint8 or float32 (default: the input's dtype) holding the same integers. A host array is
    uploaded. Runs on the current stream, no synchronisation."""
    import torch

    from ._lib import call, ptr, stream_ptr
    m, f32, N, H, W = _src(t)
    dtype = _out_dtype(dtype, m)
    col, glob = _column_stats(m, f32, N, H, W)
    out = torch.empty(m.shape, dtype=dtype, device=m.device)
    if N:
        with torch.cuda.device(m.device):
            call("adp_gray_colnorm", N, H, W, ptr(m), f32, ptr(col), ptr(glob), int(bool(preserve_global)), ptr(out),
                 int(dtype == torch.float32), stream_ptr())
    return out


def _normalize(t, method, p_low, p_high, dtype):
    import torch

    from ._lib import call, ptr, stream_ptr
    m, f32, N, H, W = _src(t)
    dtype = _out_dtype(dtype, m)
    out = torch.empty(m.shape, dtype=dtype, device=m.device)
    if N:
        hist = torch.empty((N, 256), dtype=torch.int32, device=m.device)
        with torch.cuda.device(m.device):
            call("adp_clahe_hist", N, H, W, ptr(m), f32, 1, 1, ptr(hist), stream_ptr())
            call("adp_gray_normalize", N, H * W, ptr(m), f32, ptr(hist), method, float(p_low), float(p_high), ptr(out),
                 int(dtype == torch.float32), stream_ptr())
    return out


def zscore(t, dtype=None):
    """normalize_zscore_np on the device (the histogram by adp_clahe_hist on a 1 x 1 grid, then adp_gray_normalize)."""
    return _normalize(t, ZSCORE, 0.0, 100.0, dtype)


def percentile(t, p_low=1.0, p_high=99.0, dtype=None):
    """normalize_percentile_np on the device."""
    p_low, p_high = _percentiles(p_low, p_high)
    return _normalize(t, PERCENTILE, p_low, p_high, dtype)


# ---------------------------------------------------------------- the reference's surface
def _apply(img, np_fn, dev_fn):
    """In the input's dtype (uint8, or float holding the integers) and container: array in, array out; tensor in, tensor
    out on the same device; the device where there is one."""
    if _is_tensor(img):
        return _dispatch(img, lambda a: np_fn(a, a.dtype), dev_fn)
    a = np.asarray(img)
    dt = a.dtype if a.dtype.kind == "f" else np.uint8
    return _dispatch(a, lambda v: np_fn(v, dt),
                     lambda v: dev_fn(v.astype(np.float32) if dt != np.uint8 else v)).astype(dt, copy=False)


def remove_banding_column_normalize(img, preserve_global=True):
    """preprocess_small_MS_SIMs.py:249-286 on an (H, W) or (N, H, W) gray image, array or tensor."""
    return _apply(img, lambda a, dt: column_normalize_np(a, preserve_global, dt),
                  lambda t: column_normalize(t, preserve_global))


def normalize_zscore(img):
    """preprocess_small_MS_SIMs.py:92-114: an 8-bit image in the input's dtype (augment.normalize_zscore is the training
    feed's and returns the float z-scores)."""
    return _apply(img, normalize_zscore_np, zscore)


def normalize_percentile(img, p_low=1.0, p_high=99.0):
    """preprocess_small_MS_SIMs.py:117-138: an 8-bit image in the input's dtype (augment.normalize_percentile is the
    training feed's and returns floats in 0 .. 1)."""
    p_low, p_high = _percentiles(p_low, p_high)
    return _apply(img, lambda a, dt: normalize_percentile_np(a, p_low, p_high, dt), lambda t: percentile(t, p_low, p_high))


class GrayNormalization:
    """preprocess_ecm_image's statistical steps: column de-banding (column_banding, with preserve_global) and the
    normalisation method (None, "percentile" with p_low / p_high, or "zscore"). remove_banding() and normalize() are the
    two steps; calling the object does both in that order. The reference runs the morphological banding removal and the
    illumination correction between and after them (IlluminationCorrection.remove_banding / .correct)."""

    def __init__(self, column_banding=False, preserve_global=True, method=None, p_low=1.0, p_high=99.0):
        if method in ("none", ""):
            method = None
        if method not in METHODS:
            raise ValueError("method must be None, 'percentile' or 'zscore'")
        self.column_banding = bool(column_banding)
        self.preserve_global = bool(preserve_global)
        self.method = method
        self.p_low, self.p_high = _percentiles(p_low, p_high)

    def remove_banding(self, img):
        return remove_banding_column_normalize(img, self.preserve_global) if self.column_banding else img

    def normalize(self, img):
        if self.method == "percentile":
            return normalize_percentile(img, self.p_low, self.p_high)
        if self.method == "zscore":
            return normalize_zscore(img)
        return img

    def __call__(self, img):
        return self.normalize(self.remove_banding(img))

    def __repr__(self):
        return (f"GrayNormalization(column_banding={self.column_banding}, preserve_global={self.preserve_global}, "
                f"method={self.method!r}, p_low={self.p_low}, p_high={self.p_high})")
