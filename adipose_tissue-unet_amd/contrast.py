"""Contrast-limited adaptive histogram equalisation (CLAHE) of 8-bit gray images, and the adaptive normalisation built on it.

The reference enhances contrast on the way into the network in three places:

  pre-post-processing_tools/preprocess_small_MS_SIMs.py:393-431, 526-531, 919-923   --enhance-contrast, --clahe-tile-size 16,
                                                                                     --clahe-clip-limit 3.0, on the whole image
  pre-post-processing_tools/large_wsi_to_small_wsi_MS.py:202-210, 266-292           enhance_clahe(arr, 2.0, 8), per channel
  .../contrast_and_normalization_analysis/adaptive_clahe_function.py                adaptive_clahe_normalization(img)

all through cv2.createCLAHE(clipLimit, tileGridSize).apply. cv2 is not a dependency, so parity with cv2 itself is
unpinned; both paths of this module are built to the definition below, OpenCV 4's clahe.cpp for 8-bit input, restated.

Input: src (H, W) uint8, clip_limit (double), a grid of tx x ty tiles (cv2's tileGridSize is (tx, ty)).

1. Geometry. If H % ty == 0 and W % tx == 0 the extended size (He, We) is (H, W). Otherwise BOTH axes are extended:
   He = H + (ty - H % ty), We = W + (tx - W % tx); an axis that divides evenly still grows by a full ty or tx when the
   other does not (cv2's quirk, kept). The extension is reflect-101 at the bottom and right (index H + i -> H - 2 - i).
   Tile size th = He // ty, tw = We // tx, area = th * tw. ValueError if an extension exceeds dim - 1, or if tx or ty is
   outside 1 .. 64.
2. Clip. clip = max(int(clip_limit * area / 256), 1) in IEEE double if clip_limit > 0, else 0 = no clipping.
3. Per tile: the integer histogram h[256] of the extended image's tile. If clip > 0: excess = sum max(h - clip, 0),
   h = min(h, clip), batch = excess // 256, resid = excess - 256 * batch, every bin += batch; if resid > 0,
   step = max(256 // resid, 1) and bins 0, step, 2 step, ... get 1 more, stopping after resid bins or at index 256,
   whichever comes first (resid < 256 and (resid - 1) * (256 // resid) < 256, so it is always after resid bins and the
   histogram's sum is kept).
4. LUT. scale = float32(255) / float32(area); lut[i] = saturate_u8(rint(float32(cumsum(h)[i]) * scale)), half to even.
5. Interpolation per output pixel (y, x) in float32, every multiply and add rounded on its own (no fused multiply-add):
   tyf = float32(y) * (1f / float32(th)) - 0.5f, y1 = floor(tyf), ya = tyf - y1, ya1 = 1f - ya, then y1 = max(y1, 0),
   y2 = min(floor(tyf) + 1, ty - 1); the same in x. With v = src[y, x]:
   res = (lut[y1,x1][v] * xa1 + lut[y1,x2][v] * xa) * ya1 + (lut[y2,x1][v] * xa1 + lut[y2,x2][v] * xa) * ya
   dst = saturate_u8(rint(res)).

Everything up to the LUT is integers, and the float32 steps are single IEEE operations, so the device path
(csrc/clahe.hip: adp_clahe_hist / adp_clahe_lut / adp_clahe_apply) and the numpy path below (hosts without a GPU, and the
tests' reference) agree bit for bit. A float32 plane is rounded to nearest and clamped to 0 .. 255 on load: the identity
for the gray planes data.read_gray and the predictor's PIL gray produce.

adaptive_clahe_normalization sorts an image into poor / medium / good from its contrast ratio std / (mean + 1e-6) and
the variance of its Laplacian (4 neighbours, reflect-101: cv2.Laplacian's default), formed on the host from five
integer sums {sum g, sum g^2, sum lap, sum lap^2, H * W} (adp_gray_stats), then applies CLAHE (2.0, 8 x 8), CLAHE
(1.5, 12 x 12) or none, and a 5-95 or 2-98 percentile stretch clip((v - lo) / (hi - lo + 1e-3), 0, 1). The order
statistics come exactly from the image's 256-bin histogram with numpy's linear interpolation in float64
(adp_u8_stretch does that on the device, no host sync); the result is float32.
"""
from __future__ import annotations

import math

import numpy as np

from .components import _is_tensor, _on_device, _to_device

MAX_GRID = 64
# rows / columns of a tile that one block of adp_clahe_hist counts (include/adipose_hip.h ADP_CLAHE_SLAB_ROWS / _COLS):
# the GPU tests place their shapes around them
SLAB_ROWS, SLAB_COLS = 64, 1024
QUALITY_CLASSES = ("poor", "medium", "good")
POOR_CONTRAST, GOOD_CONTRAST, GOOD_SHARPNESS = 0.183, 0.267, 38.2
STRETCH_ADD, STRETCH_MAX = 0, 1   # den = (hi - lo) + 1e-3 (the adaptive function's) | max(hi - lo, 1e-3)
_F = np.float32


# ---------------------------------------------------------------- definition: geometry and clip
def _grid(tile_grid):
    tx, ty = (int(tile_grid), int(tile_grid)) if np.isscalar(tile_grid) else (int(tile_grid[0]), int(tile_grid[1]))
    if not (1 <= tx <= MAX_GRID and 1 <= ty <= MAX_GRID):
        raise ValueError(f"the tile grid must be 1 .. {MAX_GRID} both ways")
    return tx, ty


def clahe_geometry(H, W, tile_grid=(8, 8)):
    """(He, We, th, tw) of an (H, W) image on the grid tile_grid = (tx, ty) (cv2's order)."""
    tx, ty = _grid(tile_grid)
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError("CLAHE takes an image of at least 1 x 1")
    if H % ty == 0 and W % tx == 0:
        He, We = H, W
    else:
        He, We = H + (ty - H % ty), W + (tx - W % tx)
        if He - H > H - 1 or We - W > W - 1:
            raise ValueError(f"a {H} x {W} image is too small for a {tx} x {ty} grid (reflect-101 extension)")
    return He, We, He // ty, We // tx


def clahe_clip(clip_limit, area):
    """The per-bin limit of a tile of `area` pixels; 0 = no clipping."""
    clip_limit = float(clip_limit)
    if not clip_limit > 0:
        return 0
    if not math.isfinite(clip_limit):
        raise ValueError("clip_limit must be finite")
    return max(int(clip_limit * area / 256), 1)


# ---------------------------------------------------------------- numpy path
def _u8_np(img):
    a = np.asarray(img)
    if a.ndim not in (2, 3):
        raise ValueError("CLAHE takes an (H, W) or (N, H, W) gray image")
    if a.dtype == np.uint8:
        return a
    if a.dtype.kind == "f":
        return np.clip(np.rint(a), 0, 255).astype(np.uint8)
    raise TypeError("CLAHE takes uint8, or float holding 0 .. 255")


def clahe_hist_np(img, tile_grid=(8, 8)):
    """(H, W) or (N, H, W) -> (ty, tx, 256) or (N, ty, tx, 256) uint32: the histograms of the extended image's tiles."""
    a = _u8_np(img)
    tx, ty = _grid(tile_grid)
    H, W = a.shape[-2:]
    He, We, th, tw = clahe_geometry(H, W, (tx, ty))
    b = a.reshape((-1, H, W))
    e = np.pad(b, ((0, 0), (0, He - H), (0, We - W)), mode="reflect")
    t = e.reshape(-1, ty, th, tx, tw).transpose(0, 1, 3, 2, 4).reshape(-1, th * tw)
    idx = (np.arange(t.shape[0], dtype=np.int64)[:, None] * 256 + t).ravel()
    h = np.bincount(idx, minlength=t.shape[0] * 256).astype(np.uint32)
    return h.reshape(a.shape[:-2] + (ty, tx, 256))


def clahe_lut_np(hist, area, clip_limit):
    """(..., 256) histograms of tiles of `area` pixels -> (..., 256) uint8 look-up tables."""
    h = np.asarray(hist).astype(np.int64)
    clip = clahe_clip(clip_limit, area)
    if clip > 0:
        excess = np.maximum(h - clip, 0).sum(axis=-1, keepdims=True)
        h = np.minimum(h, clip)
        batch = excess // 256
        resid = excess - 256 * batch
        step = np.maximum(256 // np.maximum(resid, 1), 1)
        i = np.arange(256)
        h = h + batch + ((resid > 0) & (i % step == 0) & (i // step < resid))
    scale = _F(255) / _F(area)
    return np.clip(np.rint(np.cumsum(h, axis=-1).astype(_F) * scale), 0, 255).astype(np.uint8)


def _axis_weights(n, t, cells):
    """Per position 0 .. n-1 of an axis with tiles of t and `cells` tiles: (i1, i2, a, a1)."""
    f = np.arange(n, dtype=_F) * (_F(1) / _F(t)) - _F(0.5)
    fl = np.floor(f)
    a = f - fl
    return np.maximum(fl, 0).astype(np.intp), np.minimum(fl + 1, cells - 1).astype(np.intp), a, _F(1) - a


def clahe_apply_np(img, lut, tile_grid=(8, 8), dtype=np.uint8):
    """The interpolation step: img (H, W) or (N, H, W), lut (ty, tx, 256) or (N, ty, tx, 256) -> the image in `dtype`."""
    a = _u8_np(img)
    tx, ty = _grid(tile_grid)
    H, W = a.shape[-2:]
    _, _, th, tw = clahe_geometry(H, W, (tx, ty))
    b = a.reshape((-1, H, W))
    L = np.asarray(lut).reshape((-1, ty, tx, 256))
    if L.shape[0] != b.shape[0] or L.dtype != np.uint8:
        raise ValueError("the look-up tables do not match the image")
    y1, y2, ya, ya1 = (v[:, None] for v in _axis_weights(H, th, ty))
    x1, x2, xa, xa1 = (v[None, :] for v in _axis_weights(W, tw, tx))
    out = np.empty(b.shape, dtype)
    for n in range(b.shape[0]):
        v, T = b[n], L[n]
        top = T[y1, x1, v].astype(_F) * xa1 + T[y1, x2, v].astype(_F) * xa
        bot = T[y2, x1, v].astype(_F) * xa1 + T[y2, x2, v].astype(_F) * xa
        out[n] = np.clip(np.rint(top * ya1 + bot * ya), 0, 255).astype(dtype)
    return out.reshape(a.shape)


def clahe_np(img, clip_limit=2.0, tile_grid=(8, 8), dtype=np.uint8):
    """cv2.createCLAHE(clip_limit, tile_grid).apply(img) by the module's definition, in numpy."""
    a = _u8_np(img)
    _, _, th, tw = clahe_geometry(a.shape[-2], a.shape[-1], tile_grid)
    return clahe_apply_np(a, clahe_lut_np(clahe_hist_np(a, tile_grid), th * tw, clip_limit), tile_grid, dtype)


def gray_stats_np(img):
    """(H, W) or (N, H, W) -> (N, 5) int64 {sum g, sum g^2, sum lap, sum lap^2, H * W}; lap as in quality.py."""
    a = _u8_np(img)
    g = a.reshape((-1,) + a.shape[-2:]).astype(np.int64)
    N, H, W = g.shape
    if H < 2 or W < 2:
        raise ValueError("the Laplacian needs H and W of at least 2 (reflect-101 borders)")
    p = np.pad(g, ((0, 0), (1, 1), (1, 1)), mode="reflect")
    lap = p[:, :-2, 1:-1] + p[:, 2:, 1:-1] + p[:, 1:-1, :-2] + p[:, 1:-1, 2:] - 4 * g
    return np.stack([g.sum(axis=(1, 2)), (g * g).sum(axis=(1, 2)), lap.sum(axis=(1, 2)), (lap * lap).sum(axis=(1, 2)),
                     np.full(N, H * W, np.int64)], axis=1).astype(np.int64)


def quality_measures(sums):
    """(N, 5) sums (array or tensor) -> (contrast_ratio, sharpness) float64 arrays: population std / (mean + 1e-6) and
    the population variance of the Laplacian, numerators in Python ints (n * S2 passes 2^63 on large images)."""
    s = sums.cpu().numpy() if hasattr(sums, "cpu") else np.asarray(sums)
    ratio, sharp = [], []
    for s1, s2, l1, l2, n in ([int(v) for v in r] for r in s.reshape(-1, 5)):
        mean = s1 / n
        std = math.sqrt((n * s2 - s1 * s1) / (n * n))
        ratio.append(std / (mean + 1e-6))
        sharp.append((n * l2 - l1 * l1) / (n * n))
    return np.array(ratio, np.float64), np.array(sharp, np.float64)


def quality_class(sums):
    """(N, 5) sums -> a list of "poor" | "medium" | "good" (adaptive_clahe_function.py's cut-offs)."""
    return ["poor" if r < POOR_CONTRAST else "good" if r > GOOD_CONTRAST and s > GOOD_SHARPNESS else "medium"
            for r, s in zip(*quality_measures(sums))]


def hist_percentiles(hist, p_low, p_high):
    """np.percentile(values, (p_low, p_high)) (method "linear", float64) of the values a 256-bin histogram counts."""
    cum = np.cumsum(np.asarray(hist).astype(np.int64))
    n = int(cum[-1])
    out = []
    for p in (p_low, p_high):
        pos = (n - 1) * (np.float64(p) / np.float64(100))
        k = int(np.floor(pos))
        t = pos - np.float64(k)
        a = np.float64(np.searchsorted(cum, k, side="right"))                # the k-th smallest value (0-based)
        b = np.float64(np.searchsorted(cum, min(k + 1, n - 1), side="right"))
        d = b - a
        out.append(b - d * (np.float64(1) - t) if t >= 0.5 else a + d * t)   # numpy's _lerp
    return out[0], out[1]


def u8_stretch_np(img, p_low, p_high, mode=STRETCH_ADD):
    """Per image clip((v - lo) / den, 0, 1) as float32, lo / hi its p_low / p_high percentiles; den = (hi - lo) + 1e-3
    (mode STRETCH_ADD) or max(hi - lo, 1e-3) (STRETCH_MAX). The arithmetic is float64, rounded to float32 once."""
    a = _u8_np(img)
    b = a.reshape((-1,) + a.shape[-2:])
    out = np.empty(b.shape, np.float32)
    for n in range(b.shape[0]):
        lo, hi = hist_percentiles(np.bincount(b[n].ravel(), minlength=256), p_low, p_high)
        den = (hi - lo) + 1e-3 if mode == STRETCH_ADD else max(hi - lo, 1e-3)
        table = np.clip((np.arange(256, dtype=np.float64) - lo) / den, 0.0, 1.0).astype(np.float32)
        out[n] = table[b[n]]
    return out.reshape(a.shape)


_ADAPTIVE = {"poor": (2.0, 8, 5.0, 95.0), "medium": (1.5, 12, 5.0, 95.0), "good": (None, None, 2.0, 98.0)}


def adaptive_clahe_normalization_np(img):
    a = _u8_np(img)
    b = a.reshape((-1,) + a.shape[-2:])
    out = np.empty(b.shape, np.float32)
    for n, cls in enumerate(quality_class(gray_stats_np(b))):
        clip, grid, lo, hi = _ADAPTIVE[cls]
        e = b[n] if clip is None else clahe_np(b[n], clip, (grid, grid))
        out[n] = u8_stretch_np(e, lo, hi, STRETCH_ADD)
    return out.reshape(a.shape)


# ---------------------------------------------------------------- device path
def _src(t):
    """A host array or a tensor -> (contiguous device tensor uint8 | float32, its f32 flag, N, H, W)."""
    import torch
    m = _to_device(t)
    if m.dim() not in (2, 3):
        raise ValueError("CLAHE takes an (H, W) or (N, H, W) gray image")
    if m.dtype not in (torch.uint8, torch.float32):
        if not m.dtype.is_floating_point:
            raise TypeError("CLAHE takes uint8, or float holding 0 .. 255")
        m = m.to(torch.float32)
    m = m.contiguous()
    N = 1 if m.dim() == 2 else int(m.shape[0])
    return m, int(m.dtype == torch.float32), N, int(m.shape[-2]), int(m.shape[-1])


def clahe_hist(t, tile_grid=(8, 8)):
    """clahe_hist_np on the device: (ty, tx, 256) or (N, ty, tx, 256) int32 tensor (torch has no usable uint32: the same
    bits, and no count reaches 2^31). Runs on the current stream."""
    import torch

    from ._lib import call, ptr, stream_ptr
    m, f32, N, H, W = _src(t)
    tx, ty = _grid(tile_grid)
    clahe_geometry(H, W, (tx, ty))
    hist = torch.empty(tuple(m.shape[:-2]) + (ty, tx, 256), dtype=torch.int32, device=m.device)
    if N:
        with torch.cuda.device(m.device):
            call("adp_clahe_hist", N, H, W, ptr(m), f32, ty, tx, ptr(hist), stream_ptr())
    return hist


def clahe_lut(hist, area, clip_limit):
    """clahe_lut_np on the device: (..., ty, tx, 256) int32 histograms -> uint8 tables of the same shape."""
    import torch

    from ._lib import call, ptr, stream_ptr
    if not (_is_tensor(hist) and hist.is_cuda and hist.dtype == torch.int32 and hist.dim() in (3, 4) and hist.shape[-1] == 256):
        raise TypeError("expected the int32 device tensor that clahe_hist() returns")
    clahe_clip(clip_limit, area)
    h = hist.contiguous()
    ty, tx = int(h.shape[-3]), int(h.shape[-2])
    N = 1 if h.dim() == 3 else int(h.shape[0])
    lut = torch.empty(h.shape, dtype=torch.uint8, device=h.device)
    if N:
        with torch.cuda.device(h.device):
            call("adp_clahe_lut", N, ty, tx, int(area), float(clip_limit), ptr(h), ptr(lut), stream_ptr())
    return lut


def clahe_apply(t, lut, tile_grid=(8, 8), dtype=None):
    """clahe_apply_np on the device; `dtype` torch.uint8 or torch.float32 (default: the input's)."""
    import torch

    from ._lib import call, ptr, stream_ptr
    m, f32, N, H, W = _src(t)
    tx, ty = _grid(tile_grid)
    clahe_geometry(H, W, (tx, ty))
    dtype = dtype or m.dtype
    if dtype not in (torch.uint8, torch.float32):
        raise TypeError("CLAHE writes uint8 or float32")
    if not (_is_tensor(lut) and lut.is_cuda and lut.dtype == torch.uint8
            and tuple(lut.shape) == tuple(m.shape[:-2]) + (ty, tx, 256)):
        raise ValueError("the look-up tables do not match the image")
    out = torch.empty(m.shape, dtype=dtype, device=m.device)
    if N:
        with torch.cuda.device(m.device):
            call("adp_clahe_apply", N, H, W, ptr(m), f32, ty, tx, ptr(lut.contiguous()), ptr(out),
                 int(dtype == torch.float32), stream_ptr())
    return out


def clahe(t, clip_limit=2.0, tile_grid=(8, 8), dtype=None):
    """CLAHE on the device: (H, W) or (N, H, W) uint8 or float32 (rounded and clamped to 0 .. 255 on load), every image
    on its own -> a device tensor of the same shape, uint8 or float32 (default: the input's dtype) holding the same
    integers. A host array is uploaded. Three launches on the current stream, no synchronisation."""
    m, _, _, H, W = _src(t)
    _, _, th, tw = clahe_geometry(H, W, tile_grid)
    return clahe_apply(m, clahe_lut(clahe_hist(m, tile_grid), th * tw, clip_limit), tile_grid, dtype)


def gray_stats(t):
    """gray_stats_np on the device: (N, 5) int64 device tensor."""
    import torch

    from ._lib import call, ptr, stream_ptr
    m, f32, N, H, W = _src(t)
    if H < 2 or W < 2:
        raise ValueError("the Laplacian needs H and W of at least 2 (reflect-101 borders)")
    sums = torch.empty((N, 5), dtype=torch.int64, device=m.device)
    if N:
        with torch.cuda.device(m.device):
            call("adp_gray_stats", N, H, W, ptr(m), f32, ptr(sums), stream_ptr())
    return sums


def u8_stretch(t, p_low, p_high, mode=STRETCH_ADD):
    """u8_stretch_np on the device (uint8 in, float32 out): the image's global histogram (adp_clahe_hist on a 1 x 1
    grid), then adp_u8_stretch, which finds the order statistics from it on the device."""
    import torch

    from ._lib import call, ptr, stream_ptr
    m, f32, N, H, W = _src(t)
    if f32:
        m = m.round().clamp_(0, 255).to(torch.uint8)
    hist = clahe_hist(m, (1, 1))
    out = torch.empty(m.shape, dtype=torch.float32, device=m.device)
    if N:
        with torch.cuda.device(m.device):
            call("adp_u8_stretch", N, H * W, ptr(m), ptr(hist), float(p_low), float(p_high), int(mode), ptr(out),
                 stream_ptr())
    return out


def _adaptive_device(t):
    import torch
    m, _, N, H, W = _src(t)
    b = m.reshape(N, H, W)
    classes = quality_class(gray_stats(b))   # the one host sync: the (N, 5) sums decide the branch
    out = torch.empty((N, H, W), dtype=torch.float32, device=m.device)
    for cls in QUALITY_CLASSES:
        sel = [i for i, c in enumerate(classes) if c == cls]
        if not sel:
            continue
        clip, grid, lo, hi = _ADAPTIVE[cls]
        g = b if len(sel) == N else b[torch.tensor(sel, device=m.device)]
        if clip is not None:
            g = clahe(g, clip, (grid, grid), torch.uint8)
        r = u8_stretch(g, lo, hi, STRETCH_ADD)
        if len(sel) == N:
            out = r
        else:
            out[torch.tensor(sel, device=m.device)] = r
    return out.reshape(m.shape)


# ---------------------------------------------------------------- the reference's surface
def _dispatch(img, np_fn, dev_fn):
    """numpy in, numpy out; tensor in, tensor out on the same device. The device where there is one (a device tensor
    always), the numpy path otherwise."""
    if not _is_tensor(img):
        img = np.asarray(img)
    if not _on_device(img):
        if _is_tensor(img):
            import torch
            return torch.from_numpy(np_fn(img.numpy()))
        return np_fn(img)
    out = dev_fn(img)
    if _is_tensor(img):
        return out if img.is_cuda else out.cpu()
    return out.cpu().numpy()


def apply_clahe(img, clip_limit=2.0, tile_grid=(8, 8)):
    """CLAHE of an (H, W) or (N, H, W) gray image, array or tensor, in the input's dtype (uint8, or float32 holding the
    integers) and container."""
    if _is_tensor(img):
        return _dispatch(img, lambda a: clahe_np(a, clip_limit, tile_grid, a.dtype), lambda t: clahe(t, clip_limit, tile_grid))
    a = np.asarray(img)
    dt = a.dtype if a.dtype.kind == "f" else np.uint8
    return _dispatch(a, lambda v: clahe_np(v, clip_limit, tile_grid, dt),
                     lambda v: clahe(v.astype(np.float32) if dt != np.uint8 else v, clip_limit, tile_grid)).astype(dt, copy=False)


def enhance_clahe(arr, clip_limit=2.0, tile_size=8):
    """large_wsi_to_small_wsi_MS.py:202-210: CLAHE on a tile_size x tile_size grid; an (H, W, C) image channel by
    channel (one batch of C planes on the device)."""
    grid = (int(tile_size), int(tile_size))
    if arr.ndim == 2:
        return apply_clahe(arr, clip_limit, grid)
    if arr.ndim != 3:
        raise ValueError("enhance_clahe takes (H, W) or (H, W, C)")
    if _is_tensor(arr):
        return apply_clahe(arr.permute(2, 0, 1).contiguous(), clip_limit, grid).permute(1, 2, 0).contiguous()
    planes = apply_clahe(np.ascontiguousarray(np.moveaxis(np.asarray(arr), 2, 0)), clip_limit, grid)
    return np.ascontiguousarray(np.moveaxis(planes, 0, 2))


def adaptive_clahe_normalization(img):
    """adaptive_clahe_function.py: (H, W) or (N, H, W) gray (array or tensor) -> float32 in [0, 1], every image by its
    own class. On the device a batch is grouped by class; the only host sync is the read of the (N, 5) sums."""
    return _dispatch(img, adaptive_clahe_normalization_np, _adaptive_device)


class Clahe:
    """cv2.createCLAHE(clipLimit, (tile_size, tile_size)) with preprocess_small_MS_SIMs.py's defaults
    (--clahe-clip-limit 3.0, --clahe-tile-size 16); call it on a gray image or a batch."""

    def __init__(self, clip_limit=3.0, tile_size=16):
        self.clip_limit = float(clip_limit)
        self.tile_size = int(tile_size)
        self.tile_grid = _grid(self.tile_size)
        clahe_clip(self.clip_limit, 1)

    def __call__(self, img):
        return apply_clahe(img, self.clip_limit, self.tile_grid)

    def __repr__(self):
        return f"Clahe(clip_limit={self.clip_limit}, tile_size={self.tile_size})"
