"""CLAHE and the adaptive normalisation of adipose_amd.contrast: the numpy path against the module's definition.

cv2 is not installed, so parity with cv2.createCLAHE itself is unpinned. What is pinned: the vectorised numpy path equals
an independent transcription of the definition (plain per-tile and per-pixel loops, below) on histograms, tables and
output; the properties the definition implies (global equalisation on a 1 x 1 grid, monotone tables, a redistribution
that keeps the histogram's sum, the geometry quirk, half-to-even rounding); and the float32 interpolation stays within
one grey level of the same formula in float64. The device path is held to this numpy path bit for bit in
tests/test_gpu_contrast.py.
"""
import math

import numpy as np
import pytest

from adipose_amd import contrast as C

F = np.float32


# ---------------------------------------------------------------- the definition again, in loops
def loop_geometry(H, W, tx, ty):
    if H % ty == 0 and W % tx == 0:
        return H, W
    return H + (ty - H % ty), W + (tx - W % tx)


def loop_clahe(img, clip_limit, tx, ty):
    """(hist, lut, out) of one (H, W) uint8 image: every step of the definition as a loop over tiles, bins or pixels."""
    H, W = img.shape
    He, We = loop_geometry(H, W, tx, ty)
    th, tw = He // ty, We // tx
    area = th * tw
    ext = np.zeros((He, We), np.int64)
    for y in range(He):
        for x in range(We):
            ext[y, x] = img[y if y < H else 2 * H - 2 - y, x if x < W else 2 * W - 2 - x]
    clip = max(int(clip_limit * area / 256), 1) if clip_limit > 0 else 0
    hist = np.zeros((ty, tx, 256), np.int64)
    lut = np.zeros((ty, tx, 256), np.int64)
    scale = F(255) / F(area)
    for iy in range(ty):
        for ix in range(tx):
            h = [0] * 256
            for y in range(iy * th, (iy + 1) * th):
                for x in range(ix * tw, (ix + 1) * tw):
                    h[ext[y, x]] += 1
            hist[iy, ix] = h
            if clip > 0:
                excess = 0
                for i in range(256):
                    if h[i] > clip:
                        excess += h[i] - clip
                        h[i] = clip
                batch = excess // 256
                resid = excess - 256 * batch
                for i in range(256):
                    h[i] += batch
                if resid > 0:
                    step = max(256 // resid, 1)
                    i = 0
                    while i < 256 and resid > 0:
                        h[i] += 1
                        i += step
                        resid -= 1
            s = 0
            for i in range(256):
                s += h[i]
                lut[iy, ix, i] = min(max(int(np.rint(F(s) * scale)), 0), 255)
    out = np.zeros((H, W), np.uint8)
    inv_th, inv_tw = F(1) / F(th), F(1) / F(tw)
    for y in range(H):
        tyf = F(y) * inv_th - F(0.5)
        fy = int(math.floor(tyf))
        ya = tyf - F(fy)
        ya1 = F(1) - ya
        y1, y2 = max(fy, 0), min(fy + 1, ty - 1)
        for x in range(W):
            txf = F(x) * inv_tw - F(0.5)
            fx = int(math.floor(txf))
            xa = txf - F(fx)
            xa1 = F(1) - xa
            x1, x2 = max(fx, 0), min(fx + 1, tx - 1)
            v = img[y, x]
            res = (F(lut[y1, x1, v]) * xa1 + F(lut[y1, x2, v]) * xa) * ya1 + \
                  (F(lut[y2, x1, v]) * xa1 + F(lut[y2, x2, v]) * xa) * ya
            assert res.dtype == np.float32
            out[y, x] = min(max(int(np.rint(res)), 0), 255)
    return hist, lut, out


def random_image(shape, seed):
    """Half noise, half a near-white plateau: bins that exceed any clip beside bins that do not."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, shape, dtype=np.uint8)
    img[rng.random(shape) < 0.5] = 240
    return img


@pytest.mark.parametrize("shape,grid", [((9, 11), (2, 3)), ((16, 16), (4, 4)), ((33, 17), (4, 2)), ((40, 48), (1, 1))],
                         ids=str)
@pytest.mark.parametrize("clip_limit", [0.0, 2.0, 40.0])
def test_numpy_path_equals_the_loops(shape, grid, clip_limit):
    tx, ty = grid
    img = random_image(shape, shape[0] * 100 + shape[1])
    hist, lut, out = loop_clahe(img, clip_limit, tx, ty)
    _, _, th, tw = C.clahe_geometry(shape[0], shape[1], grid)
    got_hist = C.clahe_hist_np(img, grid)
    assert got_hist.dtype == np.uint32 and np.array_equal(got_hist, hist)
    got_lut = C.clahe_lut_np(got_hist, th * tw, clip_limit)
    assert got_lut.dtype == np.uint8 and np.array_equal(got_lut, lut)
    assert np.array_equal(C.clahe_apply_np(img, got_lut, grid), out)
    assert np.array_equal(C.clahe_np(img, clip_limit, grid), out)
    # a batch is its images one by one; a float32 plane holding the integers is the same image
    both = np.stack([img, img[::-1]])
    got = C.clahe_np(both, clip_limit, grid)
    assert np.array_equal(got[0], out) and np.array_equal(got[1], C.clahe_np(np.ascontiguousarray(img[::-1]), clip_limit, grid))
    assert np.array_equal(C.clahe_np(img.astype(np.float32), clip_limit, grid, np.float32), out.astype(np.float32))


def test_global_equalisation():
    img = random_image((40, 48), 3)
    cdf = np.cumsum(np.bincount(img.ravel(), minlength=256))
    want = np.rint(cdf * 255 / img.size)[img].astype(np.uint8)
    assert np.array_equal(C.clahe_np(img, 0.0, (1, 1)), want)


def test_constant_image():
    assert np.array_equal(C.clahe_np(np.full((64, 64), 77, np.uint8), 2.0, (8, 8)), np.full((64, 64), 84, np.uint8))


@pytest.mark.parametrize("clip_limit", [0.0, 0.01, 1.5, 3.0, 40.0])
def test_lut_rows_are_monotone_and_end_at_255(clip_limit):
    img = random_image((3, 67, 64), 5)
    _, _, th, tw = C.clahe_geometry(67, 64, (8, 8))
    lut = C.clahe_lut_np(C.clahe_hist_np(img, (8, 8)), th * tw, clip_limit).astype(np.int64)
    assert lut.shape == (3, 8, 8, 256)
    assert (np.diff(lut, axis=-1) >= 0).all() and (lut[..., -1] == 255).all()


# ---------------------------------------------------------------- redistribution
def redistributed(h, clip):
    """(the clipped and redistributed histogram, resid): the definition's step 3 on integers."""
    h = np.asarray(h, np.int64).copy()
    excess = int(np.maximum(h - clip, 0).sum())
    h = np.minimum(h, clip)
    batch, resid = divmod(excess, 256)
    h += batch
    if resid:
        step = max(256 // resid, 1)
        idx = np.arange(0, 256, step)[:resid]
        h[idx] += 1
    return h, resid


def test_residual_steps_never_run_off_the_end():
    """The definition stops at index 256 or after resid bins, whichever comes first. resid = excess mod 256 < 256 and
    step = 256 // resid, so the last bin touched is (resid - 1) * step <= 256 - step < 256: for every possible resid it
    is always "after resid bins", exactly resid bins get one more, and the sum is kept. The exact condition:"""
    for resid in range(1, 256):
        step = max(256 // resid, 1)
        assert (resid - 1) * step < 256
        assert len(np.arange(0, 256, step)[:resid]) == resid


def test_redistribution_conserves_the_sum():
    """Every bin at the clip but the last, one bin `add` above it: excess = add, so resid == 0 (512), resid > 128 with
    step 1 (200), and resid with 256 // resid > 1 (50: step 5)."""
    area, clip = 4096, 16
    assert C.clahe_clip(1.0, area) == clip
    for add, want in ((512, "resid0"), (200, "step1"), (50, "step_gt1")):
        h = np.zeros(256, np.int64)
        h[:200] = clip
        h[10] += add
        rest = area - int(h.sum())          # over bins 200 .., none above the clip
        for i in range(200, 256):
            h[i] = min(clip, rest)
            rest -= h[i]
        assert rest == 0 and h.sum() == area and (np.delete(h, 10) <= clip).all()
        _, resid = redistributed(h, clip)
        assert resid == add % 256
        assert {"resid0": resid == 0, "step1": resid > 128, "step_gt1": 0 < resid <= 128 and 256 // resid > 1}[want]
        lut = C.clahe_lut_np(h, area, 1.0)
        ref, _ = redistributed(h, clip)
        assert ref.sum() == area
        assert np.array_equal(lut, np.clip(np.rint(np.cumsum(ref).astype(F) * (F(255) / F(area))), 0, 255).astype(np.uint8))


def test_clip_floors_to_one():
    assert C.clahe_clip(0.01, 64) == 1 and C.clahe_clip(1e-9, 4096) == 1
    assert C.clahe_clip(0.0, 64) == 0 and C.clahe_clip(-1.0, 64) == 0
    assert C.clahe_clip(2.0, 64) == 1 and C.clahe_clip(2.0, 1024) == 8
    assert C.clahe_clip(3.0, 147456) == 1728
    # with clip 1 every occupied bin is cut to 1 and the rest is spread over all bins
    img = random_image((16, 16), 1)
    h = np.bincount(img.ravel(), minlength=256)
    ref, _ = redistributed(h, 1)
    assert ref.sum() == 256 and ref.max() - ref.min() <= 2
    lut = C.clahe_lut_np(h, 256, 0.01)
    assert np.array_equal(lut, np.clip(np.rint(np.cumsum(ref).astype(F) * (F(255) / F(256))), 0, 255).astype(np.uint8))


# ---------------------------------------------------------------- geometry
def test_geometry_quirk():
    assert C.clahe_geometry(67, 64, (8, 8)) == (72, 72, 9, 9)      # W divides, and still grows by a full tx
    assert C.clahe_geometry(64, 67, (8, 8)) == (72, 72, 9, 9)
    assert C.clahe_geometry(64, 64, (8, 8)) == (64, 64, 8, 8)
    assert C.clahe_geometry(33, 17, (4, 2)) == (34, 20, 17, 5)     # tile_grid = (tx, ty)
    assert C.clahe_geometry(8, 8, (8, 8)) == (8, 8, 1, 1)


def test_geometry_errors():
    with pytest.raises(ValueError):
        C.clahe_geometry(3, 64, (8, 8))       # He - H = 5 > H - 1
    with pytest.raises(ValueError):
        C.clahe_geometry(64, 4, (8, 8))       # W divides... not by 8: We - W = 4 > W - 1
    with pytest.raises(ValueError):
        C.clahe_geometry(1, 3, (2, 1))        # H = 1 cannot be reflected
    for grid in ((0, 8), (8, 0), (65, 8), (8, 65)):
        with pytest.raises(ValueError):
            C.clahe_geometry(640, 640, grid)
    with pytest.raises(ValueError):
        C.clahe_np(np.zeros((3, 64), np.uint8), 2.0, (8, 8))
    with pytest.raises(ValueError):
        C.Clahe(3.0, 65)


# ---------------------------------------------------------------- float32 against float64
def apply_f64(img, lut, tx, ty, th, tw):
    """The interpolation with float64 weights and sums: (res, rounded output)."""
    H, W = img.shape

    def axis(n, t, cells):
        f = np.arange(n, dtype=np.float64) / t - 0.5
        fl = np.floor(f)
        return np.maximum(fl, 0).astype(int), np.minimum(fl + 1, cells - 1).astype(int), f - fl

    y1, y2, ya = (v[:, None] for v in axis(H, th, ty))
    x1, x2, xa = (v[None, :] for v in axis(W, tw, tx))
    L = lut.astype(np.float64)
    res = (L[y1, x1, img] * (1 - xa) + L[y1, x2, img] * xa) * (1 - ya) + (L[y2, x1, img] * (1 - xa) + L[y2, x2, img] * xa) * ya
    return res, np.clip(np.rint(res), 0, 255).astype(np.uint8)


def smooth_image(shape, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    g = 128 + 60 * np.sin(yy / 7.0 + seed) * np.cos(xx / 5.0) + rng.normal(0, 25, shape)
    return np.clip(g, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("shape,grid", [((96, 96), (8, 8)), ((67, 64), (8, 8)), ((129, 95), (12, 12)), ((120, 200), (5, 3)),
                                        ((33, 17), (4, 2)), ((256, 192), (16, 16))], ids=str)
def test_f32_interpolation_against_f64(shape, grid):
    """float32 weights carry a relative error of a few 2^-24 and res <= 255, so res moves by well under 1e-3 and the
    rounded value can change only where res sits within that of a half: by one level, on a small share of pixels (a
    restatement on six shapes of Gaussian plus sine images measured at most 0.63 %; the cap is 2 %)."""
    tx, ty = grid
    img = smooth_image(shape, shape[0] + shape[1])
    _, _, th, tw = C.clahe_geometry(shape[0], shape[1], grid)
    lut = C.clahe_lut_np(C.clahe_hist_np(img, grid), th * tw, 2.0)
    got = C.clahe_apply_np(img, lut, grid).astype(int)
    _, want = apply_f64(img, lut, tx, ty, th, tw)
    diff = np.abs(got - want.astype(int))
    share = (diff > 0).mean()
    print(f"{shape} {grid}: max diff {diff.max()}, differing {100 * share:.3f} %")
    assert diff.max() <= 1
    assert share <= 0.02


def test_exact_halves_round_to_even():
    """Power-of-two tiles: the weights are dyadic, res is exact in float32 and in float64, and lands on exact halves."""
    grid = (8, 8)
    img = smooth_image((64, 64), 11)   # 8 x 8 tiles of 8 x 8
    lut = C.clahe_lut_np(C.clahe_hist_np(img, grid), 64, 2.0)
    res, want = apply_f64(img, lut, 8, 8, 8, 8)
    got = C.clahe_apply_np(img, lut, grid)
    assert np.array_equal(got, want)           # exact arithmetic both ways: no pixel differs
    halves = res - np.floor(res) == 0.5
    assert halves.sum() > 0
    assert (got[halves] % 2 == 0).all()
    up = np.floor(res[halves]).astype(int) % 2 == 1
    assert up.any() and (~up).any()            # some halves round up, some down: to even, not away from zero


# ---------------------------------------------------------------- helpers
def sums_for(mean, var, n, lap_var=0.0):
    s1 = int(round(mean * n))
    s2 = int(round((var + (s1 / n) ** 2) * n))
    return [s1, s2, 0, int(round(lap_var * n)), n]


def test_quality_class_thresholds():
    n = 1000000
    # contrast ratio = std / (mean + 1e-6) around 0.183 (mean 100: std 18.3 gives 0.18299999817 < 0.183)
    below = sums_for(100, 18.3 ** 2, n)
    above = sums_for(100, 18.3001 ** 2, n)
    (r0, r1), _ = C.quality_measures(np.array([below, above]))
    assert r0 < 0.183 < r1 and r1 - r0 < 2e-6
    assert C.quality_class(np.array([below, above])) == ["poor", "medium"]
    # around 0.267 with a sharp Laplacian: medium up to the cut, good past it
    lo = sums_for(100, 26.7 ** 2, n, 50.0)
    hi = sums_for(100, 26.7001 ** 2, n, 50.0)
    (r0, r1), (s0, s1) = C.quality_measures(np.array([lo, hi]))
    assert r0 <= 0.267 < r1 and s0 == s1 == 50.0
    assert C.quality_class(np.array([lo, hi])) == ["medium", "good"]
    # sharpness at, below and above 38.2 (n = 10: 382 / 10 is the double 38.2): "good" needs strictly more
    base = [1000, 100000 + 10 * 900, 0]   # mean 100, var 900: ratio 0.3
    at, under, over = base + [382, 10], base + [381, 10], base + [383, 10]
    _, sh = C.quality_measures(np.array([at, under, over]))
    assert sh[0] == 38.2 and sh[1] < 38.2 < sh[2]
    assert C.quality_class(np.array([at, under, over])) == ["medium", "medium", "good"]
    # the Laplacian's mean enters: var = E[lap^2] - E[lap]^2
    _, sh = C.quality_measures(np.array([[1000, 109000, 20, 382, 10]]))
    assert sh[0] == 38.2 - 4.0


def class_images():
    rng = np.random.default_rng(17)
    yy, xx = np.mgrid[0:96, 0:96]
    poor = np.clip(200 + rng.normal(0, 8, (96, 96)), 0, 255).astype(np.uint8)                 # low contrast
    medium = np.clip(40 + 2.0 * xx + 0.2 * yy, 0, 255).astype(np.uint8)                        # wide range, smooth
    good = rng.integers(0, 256, (96, 96), dtype=np.uint8)                                      # wide range, sharp
    return {"poor": poor, "medium": medium, "good": good}


def reference_adaptive(img):
    """adaptive_clahe_function.py with the module's CLAHE in place of cv2's: (class, float64 result, den)."""
    mean, std = np.mean(img), np.std(img)
    ratio = std / (mean + 1e-6)
    g = np.pad(img.astype(np.float64), 1, mode="reflect")
    sharp = (g[:-2, 1:-1] + g[2:, 1:-1] + g[1:-1, :-2] + g[1:-1, 2:] - 4 * g[1:-1, 1:-1]).var()
    if ratio < 0.183:
        cls, e, p = "poor", C.clahe_np(img, 2.0, (8, 8)).astype(np.float64), (5, 95)
    elif ratio > 0.267 and sharp > 38.2:
        cls, e, p = "good", img.astype(np.float64), (2, 98)
    else:
        cls, e, p = "medium", C.clahe_np(img, 1.5, (12, 12)).astype(np.float64), (5, 95)
    lo, hi = np.percentile(e, p)
    return cls, np.clip((e - lo) / (hi - lo + 1e-3), 0, 1), hi - lo + 1e-3


@pytest.mark.parametrize("cls", ["poor", "medium", "good"])
def test_adaptive_normalization_against_the_reference_formula(cls):
    img = class_images()[cls]
    assert C.quality_class(C.gray_stats_np(img)) == [cls]
    want_cls, want, den = reference_adaptive(img)
    assert want_cls == cls
    got = C.adaptive_clahe_normalization_np(img)
    assert got.dtype == np.float32 and got.min() >= 0 and got.max() <= 1
    # the quotient is formed in float64 from the same numbers (a few ulp of 255 / den) and rounded to float32 once
    # (half an ulp of a value below 1)
    bound = 2.0 ** -25 + 8 * 2.0 ** -53 * 255 / den
    err = np.abs(got.astype(np.float64) - want).max()
    print(f"{cls}: den {den:.4f}, max err {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert 0 < (got > 0).mean() and (got == 1).any() and (got == 0).any()
    batch = np.stack(list(class_images().values()))
    assert np.array_equal(C.adaptive_clahe_normalization_np(batch)[list(class_images()).index(cls)], got)


def test_hist_percentiles_equal_numpy():
    rng = np.random.default_rng(2)
    for shape in ((2, 2), (7, 9), (30, 31)):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        img[0, 0] = 255
        h = np.bincount(img.ravel(), minlength=256)
        for p in ((5, 95), (2, 98), (1, 99), (0, 100), (33.3, 66.6)):
            lo, hi = C.hist_percentiles(h, *p)
            want = np.percentile(img.astype(np.float64), p)
            assert lo == want[0] and hi == want[1]
    flat = np.full((5, 5), 9, np.uint8)
    out = C.u8_stretch_np(flat, 5, 95)
    assert (out == 0).all()                 # hi == lo: (v - lo) / 1e-3 = 0


def test_gray_stats_np_against_quality():
    from adipose_amd import quality
    rng = np.random.default_rng(4)
    g = rng.integers(0, 256, (3, 7, 9), dtype=np.uint8)
    s = C.gray_stats_np(g)
    assert s.shape == (3, 5) and s.dtype == np.int64
    assert np.array_equal(s[:, 0], g.astype(np.int64).sum(axis=(1, 2)))
    assert np.array_equal(s[:, 1], (g.astype(np.int64) ** 2).sum(axis=(1, 2)))
    # an RGB tile with R = G = B = g has OpenCV's gray g: the Laplacian sums are quality.py's
    q = quality.qc_sums_np(np.repeat(g[..., None], 3, axis=-1))
    assert np.array_equal(s[:, 2:], q[:, 1:])
    with pytest.raises(ValueError):
        C.gray_stats_np(np.zeros((1, 5), np.uint8))


def test_enhance_clahe_channel_by_channel():
    rng = np.random.default_rng(6)
    rgb = rng.integers(0, 256, (40, 48, 3), dtype=np.uint8)
    rgb[..., 1] //= 3
    got = C.clahe_np(np.ascontiguousarray(np.moveaxis(rgb, 2, 0)), 2.0, (8, 8))
    want = [C.clahe_np(np.ascontiguousarray(rgb[..., c]), 2.0, (8, 8)) for c in range(3)]
    for c in range(3):
        assert np.array_equal(got[c], want[c])
    out = C.enhance_clahe(rgb)   # (on the device where there is one, the numpy path otherwise: the same bits)
    assert isinstance(out, np.ndarray) and out.shape == rgb.shape and out.dtype == np.uint8
    assert all(np.array_equal(out[..., c], want[c]) for c in range(3))
    assert np.array_equal(C.enhance_clahe(np.ascontiguousarray(rgb[..., 0])), want[0])
    assert np.array_equal(C.Clahe(2.0, 8)(np.ascontiguousarray(rgb[..., 0])), want[0])


def test_cli_flags():
    from cli import segmentation_inference
    base = ["--images-dir", "i", "--output-dir", "o", "--weights", "w"]
    a = segmentation_inference.build_parser().parse_args(base)
    assert a.enhance_contrast is False and a.clahe_tile_size == 16 and a.clahe_clip_limit == 3.0
    a = segmentation_inference.build_parser().parse_args(base + ["--enhance-contrast", "--clahe-tile-size", "8",
                                                                 "--clahe-clip-limit", "2.5"])
    assert a.enhance_contrast is True and a.clahe_tile_size == 8 and a.clahe_clip_limit == 2.5
    c = C.Clahe()
    assert (c.clip_limit, c.tile_size, c.tile_grid) == (3.0, 16, (16, 16))
