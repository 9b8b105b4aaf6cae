"""Gray-scale morphology and the background corrections of adipose_amd.illumination: the numpy path against the module's
definition.

cv2 is not installed, so parity with cv2 itself is unpinned. What is pinned: the footprint constructors (the ellipse to
oracle/numpy_ref.py's cv_ellipse_rows, the disc to the reference's float construction); the row-decomposed numpy path to
cv_morph (a loop over every offset), to scipy where it is installed, and to a brute-force loop written here for
footprints that are not square; the properties the definition implies; and the three corrections to their formulas,
written out a second time with numpy scalars. Every comparison is array_equal. The device path is held to this numpy
path bit for bit in tests/test_gpu_illumination.py.
"""
import numpy as np
import pytest

from adipose_amd import illumination as I
from oracle.numpy_ref import cv_ellipse_rows, cv_morph

F = np.float32


def random_image(shape, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=shape, dtype=np.uint8)
    flat = img.reshape(-1)
    flat[rng.integers(0, flat.size)] = 0
    flat[rng.integers(0, flat.size)] = 255
    return img


def brute(img, rows, is_max):
    """The definition as a loop over output rows and offsets; footprint (lo, hi, kw)."""
    lo, hi, kw = rows
    kh = len(lo)
    cy, cx = kh // 2, kw // 2
    H, W = img.shape
    out = np.full((H, W), 0 if is_max else 255, np.uint8)
    for y in range(H):
        for a in range(kh):
            yy = y + a - cy
            if not 0 <= yy < H:
                continue
            for b in range(lo[a], hi[a]):
                d = b - cx                      # out[y, x] takes img[yy, x + d] where that is inside
                x1, x2 = max(0, -d), min(W, W - d)
                if x1 < x2:
                    seg = img[yy, x1 + d:x2 + d]
                    out[y, x1:x2] = np.maximum(out[y, x1:x2], seg) if is_max else np.minimum(out[y, x1:x2], seg)
    return out


# ---------------------------------------------------------------- footprints
def test_ellipse_rows_equal_the_oracle():
    for k in list(range(1, 66)) + [301]:
        assert I.ellipse_rows(k) == cv_ellipse_rows(k), k


@pytest.mark.parametrize("r", [1, 2, 7, 50, 100, 200])
def test_disc_rows_equal_the_float_construction(r):
    y, x = np.ogrid[-r:r + 1, -r:r + 1]
    se = (np.sqrt(x ** 2 + y ** 2) <= r).astype(np.uint8)   # the reference's kernel
    assert np.array_equal(I.footprint_array(I.disc_rows(r)), se)


def test_rect_rows():
    lo, hi, kw = I.rect_rows(3, 5)
    assert (lo, hi, kw) == ([0, 0, 0], [5, 5, 5], 5)
    assert I.footprint_array(I.rect_rows(512, 1)).shape == (512, 1)


# ---------------------------------------------------------------- erode / dilate
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 16, 31, 64, 65])
def test_ellipses_equal_cv_morph(k):
    img = random_image((37, 53), k)
    rows = I.ellipse_rows(k)
    assert np.array_equal(I.erode_np(img, rows), cv_morph(img, rows, False))
    assert np.array_equal(I.dilate_np(img, rows), cv_morph(img, rows, True))


def test_ellipse_301_equals_cv_morph():
    img = random_image((70, 333), 301)
    rows = I.ellipse_rows(301)
    assert np.array_equal(I.erode_np(img, rows), cv_morph(img, rows, False))
    assert np.array_equal(I.dilate_np(img, rows), cv_morph(img, rows, True))


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 16, 31])
def test_against_scipy(k):
    ndi = pytest.importorskip("scipy.ndimage")
    img = random_image((37, 53), 100 + k)
    rows = I.ellipse_rows(k)
    se = I.footprint_array(rows).astype(bool)
    # scipy centres a footprint at k // 2 as cv2 does; its erosion takes the offsets as they are
    assert np.array_equal(I.erode_np(img, rows), ndi.grey_erosion(img, footprint=se, mode="constant", cval=255))
    if k % 2 == 1:   # scipy's dilation reflects the footprint: the same set of offsets only for odd, symmetric ones
        assert np.array_equal(I.dilate_np(img, rows), ndi.grey_dilation(img, footprint=se, mode="constant", cval=0))


@pytest.mark.parametrize("kh,kw,shape", [(9, 1, (37, 53)), (8, 1, (37, 53)), (1, 6, (37, 53)), (3, 5, (37, 53)),
                                         (512, 1, (300, 9))])
def test_rectangles_equal_brute_force(kh, kw, shape):
    img = random_image(shape, kh * 7 + kw)
    rows = I.rect_rows(kh, kw)
    assert np.array_equal(I.erode_np(img, rows), brute(img, rows, False))
    assert np.array_equal(I.dilate_np(img, rows), brute(img, rows, True))


def test_rows_that_are_no_shape_equal_brute_force():
    # empty rows, rows off centre, a box wider than it is high
    rows = ([0, 3, 0, 6, 2], [2, 3, 7, 7, 2], 7)
    img = random_image((23, 31), 5)
    assert np.array_equal(I.erode_np(img, rows), brute(img, rows, False))
    assert np.array_equal(I.dilate_np(img, rows), brute(img, rows, True))


def test_empty_footprint():
    img = random_image((9, 11), 3)
    rows = ([1, 0, 2], [1, 0, 2])
    assert np.array_equal(I.erode_np(img, rows), np.full(img.shape, 255, np.uint8))
    assert np.array_equal(I.dilate_np(img, rows), np.zeros(img.shape, np.uint8))


@pytest.mark.parametrize("rows", [I.ellipse_rows(5), I.ellipse_rows(64), I.rect_rows(8, 3), I.disc_rows(7)])
def test_constant_planes_keep_their_borders(rows):
    assert np.array_equal(I.erode_np(np.full((19, 23), 255, np.uint8), rows), np.full((19, 23), 255, np.uint8))
    assert np.array_equal(I.dilate_np(np.zeros((19, 23), np.uint8), rows), np.zeros((19, 23), np.uint8))


@pytest.mark.parametrize("rows", [I.ellipse_rows(5), I.ellipse_rows(31), I.disc_rows(7), I.rect_rows(9, 1)])
def test_opening_is_anti_extensive_and_idempotent(rows):
    img = random_image((2, 37, 53), 11)
    o = I.open_np(img, rows)
    assert (o <= img).all()
    assert np.array_equal(I.open_np(o, rows), o)
    c = I.close_np(img, rows)
    assert (c >= img).all()
    assert np.array_equal(I.tophat_np(img, rows), img - o)
    assert np.array_equal(I.blackhat_np(img, rows), c - img)


def test_even_footprints_saturate_the_hats():
    img = random_image((37, 53), 12)
    rows = I.ellipse_rows(4)
    o, c = I.open_np(img, rows).astype(np.int32), I.close_np(img, rows).astype(np.int32)
    assert (o > img).any()   # asymmetric offsets: not anti-extensive
    assert np.array_equal(I.tophat_np(img, rows), np.clip(img - o, 0, 255).astype(np.uint8))
    assert np.array_equal(I.blackhat_np(img, rows), np.clip(c - img, 0, 255).astype(np.uint8))


def test_batch_is_image_by_image():
    img = random_image((3, 20, 33), 13)
    rows = I.ellipse_rows(7)
    got = I.open_np(img, rows)
    for n in range(3):
        assert np.array_equal(got[n], I.open_np(img[n], rows))


# ---------------------------------------------------------------- corrections
def formula_subtract(v, bg):
    S = sum(int(t) for t in bg.ravel())
    mean32 = np.float32(np.float64(S) / np.float64(bg.size))
    out = np.empty(v.shape, np.uint8)
    for i, (a, b) in enumerate(zip(v.ravel().tolist(), bg.ravel().tolist())):
        f = np.float32(a - b) + mean32
        out.flat[i] = int(min(max(f, np.float32(0)), np.float32(255)))
    return out


def formula_tophat(v, th):
    out = np.empty(v.shape, np.uint8)
    for i, (a, t) in enumerate(zip(v.ravel().tolist(), th.ravel().tolist())):
        f = np.float32(a) + np.float32(t) * np.float32(0.5)
        out.flat[i] = int(min(max(f, np.float32(0)), np.float32(255)))
    return out


def test_subtract_background_formula():
    v, bg = random_image((29, 31), 21), random_image((29, 31), 22)
    assert np.array_equal(I.subtract_background_np(v, bg), formula_subtract(v, bg))
    got = I.subtract_background_np(v, bg, np.float32)
    assert got.dtype == np.float32 and np.array_equal(got, formula_subtract(v, bg).astype(np.float32))


def test_subtract_background_sum_beyond_2_24():
    # 257 x 257 of 255: the sum 16 842 495 is past 2^24; one darker pixel makes the mean 255 - 1 / 66049, which a float32
    # running sum does not give
    bg = np.full((257, 257), 255, np.uint8)
    bg[5, 7] = 254
    v = random_image((257, 257), 23)
    S = 255 * 257 * 257 - 1
    assert S > 1 << 24
    mean32 = np.float32(np.float64(S) / np.float64(257 * 257))
    want = np.clip((v.astype(np.int32) - bg).astype(np.float32) + mean32, 0, 255).astype(np.uint8)
    assert np.array_equal(I.subtract_background_np(v, bg), want)
    assert np.array_equal(I.subtract_background_np(v[:40, :40], bg[:40, :40]), formula_subtract(v[:40, :40], bg[:40, :40]))
    # per image in a batch
    both = I.subtract_background_np(np.stack([v, v]), np.stack([bg, np.zeros_like(bg)]))
    assert np.array_equal(both[0], want) and np.array_equal(both[1], v)


def test_the_three_corrections():
    v = random_image((41, 47), 24)
    v[10:20, 10:30] //= 4
    assert np.array_equal(I.rolling_ball_np(v, 7), formula_subtract(v, I.open_np(v, I.disc_rows(7))))
    assert np.array_equal(I.remove_banding_morphological_np(v, 1, 12), formula_subtract(v, I.open_np(v, I.rect_rows(12, 1))))
    assert np.array_equal(I.remove_banding_morphological_np(v), formula_subtract(v, I.open_np(v, I.rect_rows(512, 1))))
    th = I.tophat_np(v, I.ellipse_rows(9))
    assert np.array_equal(I.tophat_correction_np(v, 9), formula_tophat(v, th))
    assert np.array_equal(I.tophat_correction_np(v, 8), I.tophat_correction_np(v, 9))   # even: the next odd
    assert np.array_equal(I.tophat_correction_np(v), formula_tophat(v, I.tophat_np(v, I.ellipse_rows(301))))
    # the surface: arrays in, arrays out, the input's dtype
    c = I.IlluminationCorrection(banding=(1, 12), method="rolling-ball", radius=7)
    want = I.rolling_ball_np(I.remove_banding_morphological_np(v, 1, 12), 7)
    if not I._on_device(v):
        got = c(v)
        assert got.dtype == np.uint8 and np.array_equal(got, want)
        got = c(v.astype(np.float32))
        assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32))
        assert np.array_equal(I.IlluminationCorrection(method="tophat", kernel_size=9)(v), I.tophat_correction_np(v, 9))
        assert I.IlluminationCorrection()(v) is v


def test_float_input_is_rounded_and_clamped():
    f = np.array([[0.5, 1.5, 2.5, -3.0, 254.5, 255.5, 300.0, 17.49, 17.51]], np.float32)
    u = np.array([[0, 2, 2, 0, 254, 255, 255, 17, 18]], np.uint8)
    rows = I.ellipse_rows(3)
    assert np.array_equal(I.erode_np(f, ([0], [1])), u)
    for fn in (I.erode_np, I.dilate_np, I.open_np, I.close_np, I.tophat_np, I.blackhat_np):
        assert np.array_equal(fn(f, rows), fn(u, rows))
        assert fn(f, rows, np.float32).dtype == np.float32
    assert np.array_equal(I.rolling_ball_np(f, 1), I.rolling_ball_np(u, 1))
    assert np.array_equal(I.tophat_correction_np(f, 3), I.tophat_correction_np(u, 3))


# ---------------------------------------------------------------- errors
def test_argument_errors():
    img = np.zeros((5, 5), np.uint8)
    for bad in (0, -1, I.KMAX + 1):
        with pytest.raises(ValueError):
            I.ellipse_rows(bad)
        with pytest.raises(ValueError):
            I.rect_rows(bad, 1)
        with pytest.raises(ValueError):
            I.rect_rows(1, bad)
    with pytest.raises(ValueError):
        I.disc_rows(-1)
    with pytest.raises(ValueError):
        I.disc_rows(I.KMAX // 2 + 1)
    assert len(I.disc_rows(200)[0]) == 401 and len(I.rect_rows(512, 1)[0]) == 512 and I.KMAX >= 513
    for rows in (([0], [2]), ([-1], [1]), ([1], [0]), ([0, 0], [1]), ([0], [1], 0), ([0], [3], 2), ([0] * 514, [1] * 514)):
        with pytest.raises(ValueError):
            I.erode_np(img, rows)
    with pytest.raises(ValueError):
        I.erode_np(np.zeros((2, 2, 2, 2), np.uint8), I.ellipse_rows(3))
    with pytest.raises(TypeError):
        I.erode_np(np.zeros((5, 5), np.int32), I.ellipse_rows(3))
    with pytest.raises(ValueError):
        I.subtract_background_np(img, np.zeros((5, 4), np.uint8))
    with pytest.raises(ValueError):
        I.subtract_background_np(img, np.zeros((5, 5), np.float32))
    with pytest.raises(ValueError):
        I.IlluminationCorrection(method="polynomial")
    with pytest.raises(ValueError):
        I.IlluminationCorrection(method="rolling-ball", radius=257)
    with pytest.raises(ValueError):
        I.IlluminationCorrection(method="tophat", kernel_size=514)
    with pytest.raises(ValueError):
        I.IlluminationCorrection(banding=(1, 514))
    assert I.IlluminationCorrection(method="tophat", kernel_size=512).kernel_size == 512   # bumped to 513 when applied


def test_tile_constants_and_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "adipose_hip.h")).read()
    val = {k: int(v) for k, v in re.findall(r"#define (ADP_(?:GMORPH|ILLUM)_\w+) (\d+)", hdr)}
    assert val["ADP_GMORPH_KMAX"] == I.KMAX
    assert (val["ADP_GMORPH_TILE_ROWS"], val["ADP_GMORPH_TILE_COLS"]) == (I.TILE_ROWS, I.TILE_COLS)
    assert (val["ADP_GMORPH_ERODE"], val["ADP_GMORPH_DILATE"]) == (I.ERODE, I.DILATE)
    assert (val["ADP_ILLUM_SUBTRACT_MEAN"], val["ADP_ILLUM_TOPHAT_HALF"], val["ADP_ILLUM_DIFF"]) == \
        (I.SUBTRACT_MEAN, I.TOPHAT_HALF, I.DIFF)


# ---------------------------------------------------------------- CLI
def test_cli_flags():
    from cli import segmentation_inference as S
    base = ["--images-dir", "i", "--output-dir", "o", "--weights", "w"]
    a = S.build_parser().parse_args(base)
    assert (a.illumination_method, a.rolling_ball_radius, a.tophat_kernel) == ("none", 100, 301)
    assert (a.banding_method, a.morph_width, a.morph_height) == ("none", 1, 512)
    assert S.build_illumination(a) is None
    a = S.build_parser().parse_args(base + ["--illumination-method", "rolling-ball", "--rolling-ball-radius", "50",
                                            "--banding-method", "morphological", "--morph-width", "3", "--morph-height", "256"])
    c = S.build_illumination(a)
    assert (c.banding, c.method, c.radius) == ((3, 256), "rolling-ball", 50)
    a = S.build_parser().parse_args(base + ["--illumination-method", "tophat", "--tophat-kernel", "151"])
    c = S.build_illumination(a)
    assert (c.banding, c.method, c.kernel_size) == (None, "tophat", 151)
    with pytest.raises(SystemExit):
        S.build_parser().parse_args(base + ["--illumination-method", "polynomial"])
    for bad in (["--illumination-method", "rolling-ball", "--rolling-ball-radius", "300"],
                ["--illumination-method", "tophat", "--tophat-kernel", "601"],
                ["--illumination-method", "tophat", "--tophat-kernel", "0"],
                ["--banding-method", "morphological", "--morph-height", "1024"],
                ["--banding-method", "morphological", "--morph-width", "0"]):
        with pytest.raises(ValueError):
            S.build_illumination(S.build_parser().parse_args(base + bad))


def test_cli_refuses_a_size_before_a_model_is_loaded(tmp_path, capsys):
    from cli import segmentation_inference as S
    (tmp_path / "img").mkdir()
    rc = S.main(["--images-dir", str(tmp_path / "img"), "--output-dir", str(tmp_path / "out"), "--weights",
                 str(tmp_path / "no_such_weights"), "--illumination-method", "rolling-ball", "--rolling-ball-radius", "300"])
    out = capsys.readouterr().out
    assert rc == 1 and "513" in out and "Loading model" not in out
