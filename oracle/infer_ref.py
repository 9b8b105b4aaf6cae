"""Plain references of the inference- and evaluation-side kernels -- TEST INFRASTRUCTURE ONLY.

The pieces oracle/numpy_ref.py does not already restate, for csrc/infer.hip and csrc/metrics.hip, written from the
definitions (not from any library's code) in numpy / Python integers, and the input families the CPU tests
(tests/test_infer_ref.py, against scipy / scikit-learn) and the GPU tests (tests/test_gpu_infer_side.py) share:

  prep_input          (view(img) - f32(mean)) / f32(std + 1e-10) in float32, channel-padded with zeros
  tta_merge_seq/_f64  de-augmented views summed in float32 in view order, divided by f32(nv); the float64 mean
  blend_accumulate    acc += tile * w, wsum += w in float32 over a row band of the canvas (w = None: 1)
  blend_finalize      acc / max(wsum, f32(floor)) in float32
  edt_brute           min over all zero pixels of (sy dy)^2 + (sx dx)^2 in float64, then sqrt: O(n^2)
  auc_exact           Mann-Whitney with ties from integer counts, float(Fraction(num2, 2 P N))
  average_precision   sum_g (pos_g / P) * precision_g over the groups of equal score, float64
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from . import numpy_ref as NR

F32 = np.float32
NAN = float("nan")


# --------------------------------------------------------------------------------------- input preparation
def prep_input(img, mean, std, view, Cs):
    """img (N, H, W) or (N, H, W, Cin) float32 -> (N, H', W', Cs) float32: TTA view `view` of every image, then
    (x - f32(mean)) / f32(std + 1e-10) in float32, channels Cin..Cs zero."""
    img = np.asarray(img, F32)
    if img.ndim == 3:
        img = img[..., None]
    aug = NR.TTA_TRANSFORMS[view][0]
    den = F32(float(std) + 1e-10)
    v = np.stack([aug(a) for a in img])                       # the transforms act on axes 0 and 1 of (H, W, C)
    out = np.zeros(v.shape[:3] + (Cs,), F32)
    out[..., :v.shape[3]] = (v - F32(mean)) / den
    return out


# --------------------------------------------------------------------------------------- TTA merge
def _deaugmented(per_view, views):
    return [np.ascontiguousarray(NR.TTA_TRANSFORMS[v][1](p)) for p, v in zip(per_view, views)]


def tta_merge_seq(per_view, views):
    """Sum of the de-augmented views in float32, in view order, divided by float32(nv)."""
    acc = np.zeros(np.asarray(per_view[0]).shape, F32)
    for p in _deaugmented(np.asarray(per_view, F32), views):
        acc = acc + p
    return acc / F32(len(views))


def tta_merge_f64(per_view, views):
    return np.mean(np.stack(_deaugmented(np.asarray(per_view, F32), views)).astype(np.float64), axis=0)


# --------------------------------------------------------------------------------------- blending
def blend_accumulate(tiles, positions, shape, weight=None, rows=None):
    """(acc, wsum) float32 over the canvas rows [rows[0], rows[1]) (default: all): for every tile in order
    acc += tile * weight, wsum += weight, each product and sum rounded to float32; weight None is 1 (linear)."""
    H, W = shape
    y0, y1 = (0, H) if rows is None else rows
    acc = np.zeros((y1 - y0, W), F32)
    ws = np.zeros((y1 - y0, W), F32)
    for t, (y, x) in zip(tiles, positions):
        t = np.asarray(t, F32)
        T = t.shape[0]
        w = np.ones((T, T), F32) if weight is None else np.asarray(weight, F32)[:T, :T]
        assert y0 <= y and y + T <= y1 and 0 <= x and x + T <= W, "tile outside the band"
        acc[y - y0:y - y0 + T, x:x + T] += t * w
        ws[y - y0:y - y0 + T, x:x + T] += w
    return acc, ws


def blend_finalize(acc, ws, floor):
    return (np.asarray(acc, F32) / np.maximum(np.asarray(ws, F32), F32(floor))).astype(F32)


# --------------------------------------------------------------------------------------- distance transform
def edt_brute(mask, sampling=(1.0, 1.0), chunk=256):
    """Distance of every pixel to the nearest zero pixel of `mask`, by trying every zero pixel: the minimum of
    (sy dy)^2 + (sx dx)^2 in float64, then sqrt. O(pixels x zeros); a mask without a zero is refused."""
    m = np.asarray(mask) != 0
    H, W = m.shape
    zy, zx = np.nonzero(~m)
    if zy.size == 0:
        raise ValueError("edt_brute: the mask has no zero pixel (the transform is undefined)")
    sy, sx = float(sampling[0]), float(sampling[1])
    yy, xx = (a.ravel().astype(np.float64) for a in np.mgrid[0:H, 0:W])
    zy, zx = zy.astype(np.float64), zx.astype(np.float64)
    d2 = np.empty(H * W, np.float64)
    for s in range(0, H * W, chunk):
        dy = (yy[s:s + chunk, None] - zy[None, :]) * sy
        dx = (xx[s:s + chunk, None] - zx[None, :]) * sx
        d2[s:s + chunk] = (dy * dy + dx * dx).min(axis=1)
    return np.sqrt(d2).reshape(H, W)


EDT_SHAPES = [(1, 1), (1, 130), (130, 1), (63, 65), (64, 64), (65, 63), (3, 130), (48, 40)]
EDT_EXACT_SAMPLINGS = [(1.0, 1.0), (2.0, 3.0), (0.5, 2.0)]   # every square and sum is exact in float64
EDT_INEXACT_SAMPLING = (0.7, 1.3)
EDT_BRUTE_BUDGET = 3000 * 3000                                # pixels x zeros the brute force is used up to


def edt_masks(H, W):
    """[(name, mask)] of the mask families at one shape; mask is bool, False = a zero pixel (a site). Every mask
    has at least one zero: scipy's transform (and the kernel's) of a mask without one is undefined."""
    rng = np.random.default_rng(1000 * H + W)
    out = []
    for name, (y, x) in {"corner00": (0, 0), "corner0W": (0, W - 1), "cornerH0": (H - 1, 0),
                         "cornerHW": (H - 1, W - 1)}.items():
        m = np.ones((H, W), bool)
        m[y, x] = False
        out.append((name, m))
    m = np.ones((H, W), bool)
    m[:, W // 3] = False
    out.append(("column", m))
    m = np.ones((H, W), bool)
    m[(2 * H) // 3, :] = False
    out.append(("row", m))
    yy, xx = np.mgrid[0:H, 0:W]
    out.append(("checker", ((yy + xx) % 2).astype(bool)))
    out.append(("allzero", np.zeros((H, W), bool)))
    for name, frac in (("rand0.3pct", 0.003), ("rand50pct", 0.5)):
        m = rng.random((H, W)) >= frac
        m[rng.integers(0, H), rng.integers(0, W)] = False
        out.append((name, m))
    return out


# --------------------------------------------------------------------------------------- ROC AUC / AP
def _groups(scores, truth):
    """Per group of equal score (ascending; -0 equal to +0): (positives, negatives) as Python integers."""
    s = np.asarray(scores, F32).ravel()
    y = (np.asarray(truth).ravel() > 0.5)
    assert not np.isnan(s).any()
    _, inv = np.unique(s, return_inverse=True)                 # compares by value: -0 == +0
    inv = inv.ravel()
    pos = np.bincount(inv, weights=y).astype(np.int64)
    cnt = np.bincount(inv).astype(np.int64)
    return [int(p) for p in pos], [int(c - p) for c, p in zip(cnt, pos)]


def auc_exact(scores, truth):
    """ROC AUC with ties (Mann-Whitney U / (P N), a tied pair counting one half) from integer counts:
    num2 = sum_g pos_g (2 neg_below_g + neg_g), result float(Fraction(num2, 2 P N)); NaN with one class."""
    pos, neg = _groups(scores, truth)
    P, N = sum(pos), sum(neg)
    if P == 0 or N == 0:
        return NAN
    num2, below = 0, 0
    for p, q in zip(pos, neg):
        num2 += p * (2 * below + q)
        below += q
    return float(Fraction(num2, 2 * P * N))


def average_precision(scores, truth):
    """sum_g (pos_g / P) * precision_g in float64, precision_g = positives / pixels with score >= the group's;
    NaN with one class (the reference's early return)."""
    pos, neg = _groups(scores, truth)
    P, N = sum(pos), sum(neg)
    if P == 0 or N == 0:
        return NAN
    ap, pa, ca = 0.0, 0, 0
    for p, q in zip(reversed(pos), reversed(neg)):             # descending thresholds
        pa += p
        ca += p + q
        ap += (p / P) * (pa / ca)
    return ap


AUC_N = [1, 2, 3, 255, 257, 3000]
_FLT_MIN = np.float32(np.finfo(np.float32).tiny)


def auc_cases(n):
    """[(name, scores f32 (n,), truth f32 (n,))] of the score families at one n. The random families carry both
    classes from n = 2 on (the first pixel positive, the last negative); at n = 1 every case is single-class."""
    rng = np.random.default_rng(77 + n)
    y = (rng.random(n) > 0.7).astype(F32)
    if n >= 2:
        y[0], y[-1] = 1.0, 0.0
    u = np.clip(0.35 * y + 0.65 * rng.random(n), 0, 1).astype(F32)
    out = [("continuous", u, y)]
    for lv in (3, 17):
        out.append((f"levels{lv}", (np.round(u * lv) / lv).astype(F32), y))
    out.append(("allequal", np.full(n, 0.625, F32), y))
    z = np.where(rng.random(n) < 0.5, F32(0.0), F32(-0.0)).astype(F32)
    out.append(("signedzeros", z, y))
    # -0 and +0 beside a positive and a negative score: one group between two others
    zz = np.choose(rng.integers(0, 4, n), [F32(-0.0), F32(0.0), F32(-0.25), F32(0.25)]).astype(F32)
    out.append(("zerosmixed", zz, y))
    out.append(("range-2to3", (u * 5 - 2).astype(F32), y))
    # subnormals (both signs, the smallest included) and the neighbours of FLT_MIN on both sides
    tiny = np.array([1, 2, 3, 0x7FFFFE, 0x7FFFFF, 0x800000, 0x800001, 0x800002], np.uint32)
    bits = tiny[rng.integers(0, tiny.size, n)] | (rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31))
    out.append(("subnormal", bits.astype(np.uint32).view(F32), y))
    if n >= 2:
        k = int(rng.integers(0, n))
        one = np.zeros(n, F32)
        one[k] = 1.0
        out.append(("onepositive", u, one))
        out.append(("onenegative", u, 1 - one))
    out.append(("allnegative", u, np.zeros(n, F32)))
    out.append(("allpositive", u, np.ones(n, F32)))
    return out
