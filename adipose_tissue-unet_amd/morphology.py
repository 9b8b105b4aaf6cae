"""Binary mask morphology: dilation, erosion, opening and closing by an ellipse, a rectangle or a cross.

The reference cleans every ground-truth mask in two steps (Segmentation/build_dataset.py:1190-1191,
build_test_dataset.py:596-597):

  target_mask = morph_close(target_mask, args.morph_close_k)     cv2.morphologyEx(MORPH_CLOSE) with
                                                                 getStructuringElement(MORPH_ELLIPSE, (k, k))
  target_mask = remove_small_components(target_mask, args.min_cc_px)

The second step is components.remove_small_components; this module is the first, so that a predicted mask can have the
treatment of the masks it is scored against without leaving the device.

A footprint is k rows of column extents [lo[a], hi[a]) in a k x k box (footprint_rows), anchor c = k // 2 both ways:

  dilate(M)(y, x) = OR  over lo[a] <= b < hi[a] of M(y + a - c, x + b - c)
  erode(M)(y, x)  = AND over the same offsets (not the reflected ones)
  close = erode(dilate(M)), open = dilate(erode(M)), same footprint and anchor

Positions outside the image take no part in either (OpenCV's default morphology border: an all-ones mask erodes to all
ones). For even k the offsets are not symmetric and closing is not extensive; that is OpenCV's behaviour and is kept.

The device path (csrc/morph.hip: adp_morph_pack / adp_morph_bits / adp_morph_unpack) works on bit-packed planes: (N, H,
WW) 64-bit words, WW = ceil(W / 64), bit b of word w of a row is pixel 64 w + b, the bits past W are 0. The numpy path
below (hosts without a GPU, and the tests' reference) agrees with it bit for bit: everything is integers.

cv2 is not a dependency, so parity with cv2.morphologyEx itself is unpinned; the tests pin both paths to
oracle/numpy_ref.py's cv_ellipse_rows / cv_morph (the statement of OpenCV's construction the boundary refiner is pinned
to) and, for odd k and where scipy is installed, to scipy.ndimage.binary_dilation(border_value=0) followed by
binary_erosion(border_value=1).
"""
from __future__ import annotations

import math

import numpy as np

from .components import SRC_F32, SRC_U8, _is_tensor, _on_device, _to_device

DILATE, ERODE = 0, 1
KMAX = 63
# words a block of adp_morph_bits produces (include/adipose_hip.h ADP_MORPH_TILE_ROWS / _WORDS): the GPU tests place
# their shapes around it
TILE_ROWS, TILE_WORDS = 32, 8
SHAPES = ("ellipse", "rect", "cross")


# ---------------------------------------------------------------- footprints
def footprint_rows(k, shape="ellipse"):
    """The footprint of size k as (lo, hi): row a covers the columns [lo[a], hi[a]) of the k x k box.
    ellipse: cv2.getStructuringElement(MORPH_ELLIPSE, (k, k)): r = c = k // 2, row a spans c +- rint(c * sqrt((r^2 -
    (a - r)^2) / r^2)) (saturate_cast rounds half to even), clipped to the box. rect: every row [0, k). cross: row
    k // 2 is [0, k), every other row [k // 2, k // 2 + 1)."""
    k = int(k)
    if not 1 <= k <= KMAX:
        raise ValueError(f"the footprint size must be in 1 .. {KMAX}")
    c = k // 2
    if shape == "rect":
        return [0] * k, [k] * k
    if shape == "cross":
        return [0 if a == c else c for a in range(k)], [k if a == c else c + 1 for a in range(k)]
    if shape != "ellipse":
        raise ValueError(f"shape must be one of {', '.join(SHAPES)}")
    r = c
    inv_r2 = 1.0 / (r * r) if r else 0.0
    lo, hi = [], []
    for a in range(k):
        dy = a - r
        dx = int(np.rint(c * math.sqrt((r * r - dy * dy) * inv_r2)))
        lo.append(max(c - dx, 0))
        hi.append(min(c + dx + 1, k))
    return lo, hi


def footprint_array(rows):
    """(lo, hi) -> the k x k uint8 array of the footprint."""
    lo, hi = rows
    k = len(lo)
    se = np.zeros((k, k), np.uint8)
    for a in range(k):
        se[a, lo[a]:hi[a]] = 1
    return se


def _check_rows(rows):
    lo, hi = [int(v) for v in rows[0]], [int(v) for v in rows[1]]
    k = len(lo)
    if len(hi) != k or not 1 <= k <= KMAX:
        raise ValueError(f"a footprint has 1 .. {KMAX} rows of (lo, hi)")
    if any(not 0 <= l <= h <= k for l, h in zip(lo, hi)):
        raise ValueError("a footprint row needs 0 <= lo <= hi <= k")
    return lo, hi


# ---------------------------------------------------------------- numpy path
def _fg_np(mask, threshold=None):
    m = np.asarray(mask)
    if threshold is not None:
        return m > threshold
    if m.dtype.kind == "f":
        raise TypeError("a float mask needs a threshold")
    return m != 0


def _check_ndim(a):
    if a.ndim not in (2, 3):
        raise ValueError("morphology takes an (H, W) or (N, H, W) mask")


def pack_np(mask, threshold=None):
    """(H, W) or (N, H, W) mask -> (H, WW) or (N, H, WW) uint64 words of its foreground (non-zero, or > threshold)."""
    fg = _fg_np(mask, threshold)
    _check_ndim(fg)
    W = fg.shape[-1]
    WW = (W + 63) // 64
    pad = np.zeros(fg.shape[:-1] + (WW * 64,), np.uint8)
    pad[..., :W] = fg
    by = np.packbits(pad, axis=-1, bitorder="little")
    return np.ascontiguousarray(by).view("<u8").astype(np.uint64, copy=False).reshape(fg.shape[:-1] + (WW,))


def unpack_np(bits, W, dtype=np.uint8):
    """(H, WW) or (N, H, WW) words -> the 0 / 1 mask of width W in `dtype`."""
    b = np.ascontiguousarray(np.asarray(bits)).view(np.uint64).astype("<u8", copy=False)
    _check_ndim(b)
    if b.shape[-1] != (W + 63) // 64:
        raise ValueError("the plane's words do not match W")
    px = np.unpackbits(b.view(np.uint8).reshape(b.shape[:-1] + (b.shape[-1] * 8,)), axis=-1, bitorder="little")
    return px[..., :W].astype(dtype)


def _dilate_bool(fg, rows):
    """Dilation of an (N, H, W) bool array with zeros outside: per footprint row one span OR (a difference of running
    sums along x), shifted to the row's place."""
    lo, hi = rows
    k = len(lo)
    c = k // 2
    N, H, W = fg.shape
    cs = np.zeros((N, H + 2 * k, W + 2 * k + 1), np.int32)
    np.cumsum(fg, axis=2, dtype=np.int32, out=cs[:, k:k + H, k + 1:k + W + 1])
    cs[:, k:k + H, k + W + 1:] = cs[:, k:k + H, k + W:k + W + 1]
    out = np.zeros(fg.shape, bool)
    for a in range(k):
        if lo[a] == hi[a]:
            continue
        r = cs[:, k + a - c:k + a - c + H]
        out |= r[:, :, k + hi[a] - c:k + hi[a] - c + W] > r[:, :, k + lo[a] - c:k + lo[a] - c + W]
    return out


def _np_op(mask, rows, threshold, dtype, steps):
    rows = _check_rows(rows)
    fg = _fg_np(mask, threshold)
    _check_ndim(fg)
    m = fg[None] if fg.ndim == 2 else fg
    for erode in steps:
        m = ~_dilate_bool(~m, rows) if erode else _dilate_bool(m, rows)
    m = m[0] if fg.ndim == 2 else m
    return m.astype(dtype)


def _rows_arg(k, shape):
    return footprint_rows(k, shape) if np.isscalar(k) else _check_rows(k)


def dilate_np(mask, k, shape="ellipse", threshold=None, dtype=np.uint8):
    """Dilation of an (H, W) or (N, H, W) mask (foreground non-zero, or > threshold) as 0 / 1 in `dtype`. k is a size
    (with `shape`) or a footprint (lo, hi)."""
    return _np_op(mask, _rows_arg(k, shape), threshold, dtype, (False,))


def erode_np(mask, k, shape="ellipse", threshold=None, dtype=np.uint8):
    return _np_op(mask, _rows_arg(k, shape), threshold, dtype, (True,))


def close_np(mask, k, shape="ellipse", threshold=None, dtype=np.uint8):
    return _np_op(mask, _rows_arg(k, shape), threshold, dtype, (False, True))


def open_np(mask, k, shape="ellipse", threshold=None, dtype=np.uint8):
    return _np_op(mask, _rows_arg(k, shape), threshold, dtype, (True, False))


# ---------------------------------------------------------------- device path
def _nhw(t):
    if t.dim() == 2:
        return 1, int(t.shape[0]), int(t.shape[1])
    if t.dim() == 3:
        return int(t.shape[0]), int(t.shape[1]), int(t.shape[2])
    raise ValueError("morphology takes an (H, W) or (N, H, W) mask")


def pack(mask, threshold=None):
    """The packed foreground of an (H, W) or (N, H, W) mask on the device: uint8 / bool (foreground non-zero), or float32
    together with `threshold` (foreground > threshold, fused into the load) -> int64 device tensor (H, WW) or (N, H,
    WW), WW = ceil(W / 64) (torch has no usable uint64: the words are the same bits). A host array is uploaded. Runs on
    the current stream."""
    import torch

    from ._lib import call, ptr, stream_ptr
    m = _to_device(mask)
    if m.dtype == torch.bool:
        m = m.view(torch.uint8)
    if m.dtype == torch.uint8:
        if threshold is not None:
            m, kind = m.to(torch.float32), SRC_F32
        else:
            kind = SRC_U8
    elif m.dtype == torch.float32:
        if threshold is None:
            raise TypeError("a float32 mask needs a threshold")
        kind = SRC_F32
    else:
        raise TypeError("morphology takes a uint8 / bool mask, or float32 with a threshold")
    m = m.contiguous()
    N, H, W = _nhw(m)
    bits = torch.empty(tuple(m.shape[:-1]) + ((W + 63) // 64,), dtype=torch.int64, device=m.device)
    if N and H and W:
        with torch.cuda.device(m.device):
            call("adp_morph_pack", N, H, W, ptr(m), kind, float(threshold if threshold is not None else 0.0), ptr(bits),
                 stream_ptr())
    return bits


def _bits_arg(bits, W):
    import torch
    if not (_is_tensor(bits) and bits.is_cuda and bits.dtype == torch.int64):
        raise TypeError("expected the int64 device tensor that pack() returns")
    b = bits.contiguous()
    N, H, WW = _nhw(b)
    if WW != (int(W) + 63) // 64:
        raise ValueError("the plane's words do not match W")
    return b, N, H


def unpack(bits, W, dtype=None):
    """A packed plane -> its 0 / 1 mask of width W: uint8 (default) or float32 device tensor."""
    import torch

    from ._lib import call, ptr, stream_ptr
    b, N, H = _bits_arg(bits, W)
    dtype = dtype or torch.uint8
    if dtype not in (torch.uint8, torch.float32):
        raise TypeError("unpack writes uint8 or float32")
    out = torch.empty(tuple(b.shape[:-1]) + (int(W),), dtype=dtype, device=b.device)
    if N and H and W:
        with torch.cuda.device(b.device):
            call("adp_morph_unpack", N, H, int(W), ptr(b), ptr(out) if dtype == torch.uint8 else None,
                 ptr(out) if dtype == torch.float32 else None, stream_ptr())
    return out


def _bits_op(bits, W, rows, op):
    import ctypes as C

    import torch

    from ._lib import call, ptr, stream_ptr
    lo, hi = _check_rows(rows)
    b, N, H = _bits_arg(bits, W)
    out = torch.empty_like(b)
    if N and H and W:
        k = len(lo)
        with torch.cuda.device(b.device):
            call("adp_morph_bits", N, H, int(W), ptr(b), ptr(out), k, (C.c_int * k)(*lo), (C.c_int * k)(*hi), op,
                 stream_ptr())
    return out


def dilate_bits(bits, W, rows):
    """Dilation of a packed plane of width W by the footprint rows (lo, hi): a new plane."""
    return _bits_op(bits, W, rows, DILATE)


def erode_bits(bits, W, rows):
    """Erosion of a packed plane of width W by the footprint rows (lo, hi): a new plane."""
    return _bits_op(bits, W, rows, ERODE)


def _dev_op(mask, rows, threshold, dtype, steps):
    rows = _check_rows(rows)
    W = int(mask.shape[-1])
    bits = pack(mask, threshold)
    for op in steps:
        bits = _bits_op(bits, W, rows, op)
    return unpack(bits, W, dtype)


def dilate(mask, k, shape="ellipse", threshold=None, dtype=None):
    """Dilation on the device: (H, W) or (N, H, W) uint8 / bool, or float32 with `threshold` -> 0 / 1 device tensor of
    the same shape, uint8 (default) or float32. k is a size (with `shape`: ellipse, rect or cross) or a footprint
    (lo, hi). A host array is uploaded. Runs on the current stream: pack, one pass per step, unpack."""
    return _dev_op(mask, _rows_arg(k, shape), threshold, dtype, (DILATE,))


def erode(mask, k, shape="ellipse", threshold=None, dtype=None):
    return _dev_op(mask, _rows_arg(k, shape), threshold, dtype, (ERODE,))


def close(mask, k, shape="ellipse", threshold=None, dtype=None):
    return _dev_op(mask, _rows_arg(k, shape), threshold, dtype, (DILATE, ERODE))


def open(mask, k, shape="ellipse", threshold=None, dtype=None):   # noqa: A001 (the operation's name)
    return _dev_op(mask, _rows_arg(k, shape), threshold, dtype, (ERODE, DILATE))


# ---------------------------------------------------------------- the reference's surface
def morph_close(mask, k):
    """The reference's morph_close (build_dataset.py:1115-1119): `mask` (non-zero pixels) closed with the k x k ellipse, as 0 / 1 in
    the input's dtype and container: numpy in, numpy out; tensor in, tensor out on the same device. k <= 0 returns
    `mask` itself. Uses the device where there is one (a device tensor always), the numpy path otherwise."""
    if k <= 0:
        return mask
    rows = footprint_rows(k, "ellipse")
    if not _is_tensor(mask):
        mask = np.asarray(mask)
    if not _on_device(mask):
        m = mask.numpy() if _is_tensor(mask) else mask
        out = close_np(m != 0, rows, dtype=m.dtype)
        if _is_tensor(mask):
            import torch
            return torch.from_numpy(out)
        return out
    import torch
    src = _to_device(mask)
    if src.dtype == torch.float32:
        out = close(src.abs(), rows, threshold=0.0, dtype=torch.float32)   # non-zero of a float mask: |x| > 0
    else:
        out = close(src if src.dtype in (torch.uint8, torch.bool) else src != 0, rows)
        if src.dtype != torch.uint8:
            out = out.to(src.dtype)
    if _is_tensor(mask):
        return out if mask.is_cuda else out.cpu()
    return out.cpu().numpy().astype(mask.dtype, copy=False)
