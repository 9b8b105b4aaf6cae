"""Annotation polygons -> ground-truth masks: the reference's JSON readers and create_binary_mask, on the device.

The reference builds every ground-truth mask in four steps (Segmentation/build_dataset.py, build_test_dataset.py):
  create_binary_mask       cv2.fillPoly of the annotators' polygon JSON              :903-911
  fat minus bubbles        target & ~subtract                                        :1183-1187
  morph_close              morphology.py                                             :1190
  remove_small_components  components.py                                             :1191
This module is the first two, and target_mask_bits chains all four on the device on bit-packed planes.

The reference's names and behaviour: parse_image_stem_from_json (:494-503), load_json_annotations (:738-800),
slide_has_valid_annotations (:803-837), get_tile_annotations (:840-900), create_binary_mask (:903-911). A JSON payload
is a list of annotation records or a single record; only elements of type "polyline" with at least 3 points are used;
a vertex is int(round(v)) with Python's round-half-to-even; a record without confidenceScore is included (and flagged).

What the raster is. cv2 is not a dependency, so, like the CLAHE and the morphology, the operation is defined here by a
restatement of OpenCV's construction; parity with cv2.fillPoly itself is UNPINNED.
  An image has polygons; a polygon is a cyclic list of integer vertices (x, y), x the column and y the row; edges join
  consecutive vertices and the last to the first. The raster is H x W; vertices may lie outside it on any side. All
  polygons of an image are filled together (the reference's single fillPoly call).
  interior(y, x) = the parity, over every non-horizontal edge of every polygon of the image, of
                   [ylo <= y < yhi and X(y) <= x], (xlo, ylo), (xhi, yhi) the edge's endpoints sorted by y and
                   X(y) = xlo + (y - ylo)(xhi - xlo) / (yhi - ylo) the exact rational. Each such (edge, row) toggles
                   column ceil(X(y)), clamped up to 0 and dropped when >= W; a row is the prefix-XOR of its toggles.
                   Even-odd filling: where two polygons overlap the interior cancels (OpenCV's behaviour, kept).
  boundary(y, x) = the pixels of every edge's 8-connected line: LineIterator's integer error walk from the endpoint
                   (xa, ya) with the smaller x, in closed form. dx = xb - xa >= 0, dy = yb - ya, s = sign(dy):
                   |dy| > dx:  (xa + floor((2 dx k + |dy| - 1) / (2 |dy|)), ya + s k)   k = 0 .. |dy|
                   otherwise:  (xa + k, ya + s floor((2 |dy| k + dx - 1) / (2 dx)))     k = 0 .. dx   (a point if 0)
                   Only pixels inside the raster count. OpenCV clips a line to the image before it walks it, so it can
                   differ by a pixel where a boundary leaves the raster: unpinned as well.
  mask = interior | boundary.
Coordinates are accepted in |x|, |y| <= COORD_MAX = 2^24 (products stay below 2^51 in int64); beyond it ValueError,
before anything is launched.

rasterize_np is the host path and the tests' reference (vectorised numpy, exact). rasterize_bits / rasterize are the
device path (csrc/polyraster.hip: adp_poly_raster): planes in morphology.py's packed format, (N, H, WW) 64-bit words,
WW = ceil(W / 64), bit b of word w is pixel 64 w + b, the bits past W zero. Both agree bit for bit: integers only.
"""
from __future__ import annotations

import json
from pathlib import Path
from typing import List, Tuple

import numpy as np

from .components import _gpu

# include/adipose_hip.h ADP_POLY_COORD_MAX / ADP_POLY_SCAN_WORDS (the GPU tests place their widths around the latter)
COORD_MAX = 1 << 24
SCAN_WORDS = 64

__all__ = ["parse_image_stem_from_json", "load_json_annotations", "slide_has_valid_annotations",
           "get_tile_annotations", "create_binary_mask", "rasterize_np", "rasterize_bits", "rasterize",
           "target_mask_bits", "target_mask_np", "COORD_MAX", "SCAN_WORDS"]


# ------------------------------------------------------------------------------ the reference's JSON surface
def parse_image_stem_from_json(json_path, cls: str) -> str:
    """:494-503 — the image stem of "<stem>_<cls>_annotations*.json" / "<stem>_<cls>_*.json", else the file's stem."""
    stem = Path(json_path).stem
    for token in (f"_{cls}_annotations", f"_{cls}_"):
        if token in stem:
            return stem.split(token)[0]
    return stem


def _records(json_path):
    with open(json_path, "r", encoding="utf-8") as f:
        return json.load(f)


def _elements(record):
    return record.get("annotation", {}).get("elements", [])


def _coords(pts):
    return np.array([[int(round(p[0])), int(round(p[1]))] for p in pts], dtype=np.int32)


def load_json_annotations(json_path, min_confidence: int = 1) -> Tuple[List[np.ndarray], bool]:
    """:738-800 -> (polygons as (n, 2) int32 arrays, whether a record lacked confidenceScore). Records below
    min_confidence are left out; one without a score is included."""
    data = _records(json_path)
    if isinstance(data, list):
        records = [r for r in data if isinstance(r, dict)]
    elif isinstance(data, dict):
        records = [data]
    else:
        records = []
    elements, missing = [], False
    for rec in records:
        score = rec.get("confidenceScore")
        if score is None:
            missing = True
        elif not score >= min_confidence:
            continue
        elems = _elements(rec)
        if isinstance(elems, list):
            elements.extend(elems)
    polys = []
    for elem in elements:
        if not isinstance(elem, dict) or elem.get("type") != "polyline":
            continue
        pts = elem.get("points", [])
        if pts and len(pts) >= 3:
            polys.append(_coords(pts))
    return polys, missing


def slide_has_valid_annotations(json_path, min_confidence: int) -> bool:
    """:803-837 — whether any record at or above min_confidence (or without a score) has a polyline of >= 3 points."""
    payload = _records(json_path)
    for rec in payload if isinstance(payload, list) else [payload]:
        if not isinstance(rec, dict):
            continue
        score = rec.get("confidenceScore")
        if score is None or score >= min_confidence:
            for elem in _elements(rec):
                if isinstance(elem, dict) and elem.get("type") == "polyline":
                    pts = elem.get("points", [])
                    if pts and len(pts) >= 3:
                        return True
    return False


def get_tile_annotations(json_path, tile_bbox, min_confidence: int) -> Tuple[List[np.ndarray], bool]:
    """:840-900 -> (polygons whose bounding box meets tile_bbox = (x1, y1, x2, y2), shifted to tile coordinates;
    whether the tile met only polygons below min_confidence)."""
    payload = _records(json_path)
    x1, y1, x2, y2 = tile_bbox
    polys, low, high = [], False, False
    for rec in payload if isinstance(payload, list) else [payload]:
        if not isinstance(rec, dict):
            continue
        score = rec.get("confidenceScore")
        for elem in _elements(rec):
            if not isinstance(elem, dict) or elem.get("type") != "polyline":
                continue
            pts = elem.get("points", [])
            if not pts or len(pts) < 3:
                continue
            c = _coords(pts)
            xs, ys = c[:, 0], c[:, 1]
            if xs.max() < x1 or xs.min() > x2 or ys.max() < y1 or ys.min() > y2:
                continue
            if score is not None and score < min_confidence:
                low = True
                continue
            polys.append(c - np.array([x1, y1]))
            high = True
    return polys, (low and not high)


# ------------------------------------------------------------------------------ polygons -> flat arrays
def _flatten(polys_per_image):
    """-> xy (V, 2) int64, poly_off (P + 1), img_off (N + 1): the arrays adp_poly_raster takes. Empty polygons are
    dropped. Raises ValueError on a vertex that is not integral or lies beyond COORD_MAX."""
    xy, poly_off, img_off = [], [0], [0]
    for polys in polys_per_image:
        for p in polys:
            a = np.asarray(p)
            if a.size == 0:
                continue
            if a.dtype.kind not in "iu":
                if not np.all(a == np.rint(a)):
                    raise ValueError("polygon vertices must be integers (the reference rounds them when it loads the JSON)")
            a = a.astype(np.int64).reshape(-1, 2)
            xy.append(a)
            poly_off.append(poly_off[-1] + len(a))
        img_off.append(len(poly_off) - 1)
    xy = np.concatenate(xy) if xy else np.zeros((0, 2), np.int64)
    if xy.size and np.abs(xy).max() > COORD_MAX:
        raise ValueError(f"polygon coordinates must lie in -{COORD_MAX} .. {COORD_MAX}")
    return xy, np.asarray(poly_off, np.int64), np.asarray(img_off, np.int64)


def _check_hw(H, W):
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError("the raster needs H and W of at least 1")
    return H, W


# ------------------------------------------------------------------------------ numpy path
def _expand(count):
    """For counts c[i] >= 0: (the index i of every item, its rank 0 .. c[i] - 1), items in order."""
    idx = np.repeat(np.arange(len(count)), count)
    start = np.cumsum(count) - count
    return idx, np.arange(int(count.sum()), dtype=np.int64) - start[idx]


def _raster_flat(xy, poly_off, img_off, H, W):
    N = len(img_off) - 1
    out = np.zeros((N, H, W), np.uint8)
    V = len(xy)
    if V == 0:
        return out
    npoly = np.diff(poly_off)
    pid = np.repeat(np.arange(len(npoly)), npoly)
    img = np.repeat(np.arange(N), np.diff(img_off))[pid]
    nxt = np.arange(V) + 1
    last = poly_off[1:][pid] - 1
    nxt[np.arange(V) == last] = poly_off[:-1][pid][np.arange(V) == last]
    x0, y0, x1, y1 = xy[:, 0], xy[:, 1], xy[nxt, 0], xy[nxt, 1]
    flat = out.reshape(-1)
    # interior: one toggle per (non-horizontal edge, row inside the raster), then the rows' prefix parity
    up = y0 <= y1
    xlo, ylo, xhi, yhi = np.where(up, x0, x1), np.where(up, y0, y1), np.where(up, x1, x0), np.where(up, y1, y0)
    r0, r1 = np.maximum(ylo, 0), np.minimum(yhi, H)
    e, k = _expand(np.maximum(r1 - r0, 0))
    if len(e):
        y = r0[e] + k
        D = (yhi - ylo)[e]
        col = xlo[e] - ((-(y - ylo[e]) * (xhi - xlo)[e]) // D)   # xlo + ceil(num / D), floor division of integers
        col = np.maximum(col, 0)
        keep = col < W
        pos, cnt = np.unique((img[e][keep] * H + y[keep]) * W + col[keep], return_counts=True)
        flat[pos[(cnt & 1) == 1]] = 1
        np.bitwise_xor.accumulate(out, axis=2, out=out)
    # boundary: every edge's line, the steps whose major coordinate is inside the raster
    fwd = x0 <= x1
    xa, ya, xb, yb = np.where(fwd, x0, x1), np.where(fwd, y0, y1), np.where(fwd, x1, x0), np.where(fwd, y1, y0)
    dx, dy = xb - xa, yb - ya
    ady, s = np.abs(dy), np.sign(dy)
    ymaj = ady > dx
    L = np.where(ymaj, ady, dx)
    lo = np.where(ymaj, np.where(s > 0, -ya, ya - (H - 1)), -xa)
    hi = np.where(ymaj, np.where(s > 0, H - 1 - ya, ya), W - 1 - xa)
    k0 = np.maximum(lo, 0)
    e, k = _expand(np.maximum(np.minimum(hi, L) + 1 - k0, 0))
    if len(e):
        k = k + k0[e]
        Le, minor = L[e], np.where(ymaj, dx, ady)[e]
        q = np.where(Le > 0, (2 * minor * k + Le - 1) // np.maximum(2 * Le, 1), 0)
        x = np.where(ymaj[e], xa[e] + q, xa[e] + k)
        y = np.where(ymaj[e], ya[e] + s[e] * k, ya[e] + s[e] * q)
        keep = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        flat[(img[e][keep] * H + y[keep]) * W + x[keep]] = 1
    return out


def rasterize_np(polys_per_image, H, W):
    """The raster on the host: a list (one entry per image) of lists of polygons -> (N, H, W) uint8 0 / 1. A polygon is
    an (n, 2) integer array of (x, y). Exact."""
    H, W = _check_hw(H, W)
    return _raster_flat(*_flatten(polys_per_image), H, W)


# ------------------------------------------------------------------------------ device path
def rasterize_bits(polys_per_image, H, W):
    """The raster on the device, packed: int64 device tensor (N, H, WW), WW = ceil(W / 64), in morphology.pack's format
    (one entry of polys_per_image per image). Runs on the current stream."""
    import torch

    from ._lib import call, ptr, stream_ptr
    H, W = _check_hw(H, W)
    xy, poly_off, img_off = _flatten(polys_per_image)   # (raises before anything is launched)
    N, P, V = len(img_off) - 1, len(poly_off) - 1, len(xy)
    dev = torch.device("cuda", torch.cuda.current_device())
    bits = torch.empty((N, H, (W + 63) // 64), dtype=torch.int64, device=dev)
    if N:
        # one upload: the vertices (at least one slot, so that the pointer is never null) and the two offset arrays
        host = np.concatenate([xy.reshape(-1), np.zeros(2 if V == 0 else 0, np.int64), poly_off, img_off]).astype(np.int32)
        buf = torch.from_numpy(host).to(dev)
        nxy = max(2 * V, 2)
        with torch.cuda.device(dev):
            call("adp_poly_raster", N, H, W, ptr(buf), ptr(buf[nxy:]), ptr(buf[nxy + P + 1:]), P, V, ptr(bits),
                 stream_ptr())
    return bits


def rasterize(polys_per_image, H, W, dtype=None):
    """The raster on the device as a 0 / 1 mask: uint8 (default) or float32 device tensor (N, H, W)."""
    from . import morphology
    return morphology.unpack(rasterize_bits(polys_per_image, H, W), int(W), dtype)


def create_binary_mask(polygons, width: int, height: int) -> np.ndarray:
    """:903-911 — many polygons into one (height, width) uint8 0 / 1 mask; polygons of fewer than 3 vertices are
    dropped. Uses the device where there is one, the numpy path otherwise (the same bits)."""
    polys = [np.asarray(p).reshape(-1, 2) for p in (polygons or []) if len(p) >= 3]
    if not polys:
        return np.zeros((int(height), int(width)), np.uint8)
    if _gpu():
        return rasterize([polys], height, width)[0].cpu().numpy()
    return rasterize_np([polys], height, width)[0]


# ------------------------------------------------------------------------------ the reference's whole chain
def target_mask_bits(target_polys, subtract_polys, H, W, morph_close_k=0, min_cc_px=0):
    """The reference's ground truth of one image on the device, as a packed (H, WW) plane: the raster of target_polys,
    minus the raster of subtract_polys (None or empty: nothing is subtracted), closed with the morph_close_k ellipse
    (0: off), without its 8-connected components below min_cc_px pixels (0: off). Nothing leaves the device."""
    from . import components as cc
    from . import morphology as mo
    bits = rasterize_bits([list(target_polys)], H, W)
    if subtract_polys is not None and len(subtract_polys):
        bits = bits & ~rasterize_bits([list(subtract_polys)], H, W)   # (the tail bits stay 0: bits' are)
    if morph_close_k > 0:
        rows = mo.footprint_rows(morph_close_k, "ellipse")
        bits = mo.erode_bits(mo.dilate_bits(bits, W, rows), W, rows)
    if min_cc_px > 0:
        lab = cc.label(mo.unpack(bits, W), 8)
        bits = mo.pack(cc.filter_small(lab, cc.areas(lab), min_cc_px))
    return bits[0]


def target_mask_np(target_polys, subtract_polys, H, W, morph_close_k=0, min_cc_px=0):
    """target_mask_bits on the host: the (H, W) uint8 0 / 1 mask."""
    from . import components as cc
    from . import morphology as mo
    m = rasterize_np([list(target_polys)], H, W)[0]
    if subtract_polys is not None and len(subtract_polys):
        m = m & (1 - rasterize_np([list(subtract_polys)], H, W)[0])
    if morph_close_k > 0:
        m = mo.close_np(m, morph_close_k)
    if min_cc_px > 0:
        lab = cc.label_np(m, 8)
        m = cc.filter_np(lab, cc.areas_np(lab), min_cc_px)
    return m
