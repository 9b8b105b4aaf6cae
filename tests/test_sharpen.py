"""The unsharp mask of adipose_amd.sharpen: the numpy path against the module's definition (radius, taps, border and
the integer blur sum, restated here in Python ints) and against the reference's formula.

The reference (pre-post-processing_tools/preprocess_small_MS_SIMs.py:434-455) blurs a float32 image with
cv2.GaussianBlur(img, (0, 0), sigma): float32 taps by cv2's rule (exp in float64, normalised, stored as float32), a row
pass then a column pass in float32, reflect-101 borders; then img + amount * (img - blurred), clipped and truncated. It
is restated here in float32 numpy, and the module is held to it to within one gray level on at most 0.2 % of the pixels
of textured images (the cap tests/test_normalization.py uses). Flat images and sigma below 0.5 are left out of that
comparison: there the reference's taps, which sum to 1 +- 2^-24, can drop an unchanged pixel by one level, and the
module states that it does not. The device path is held to this numpy path bit for bit in tests/test_gpu_sharpen.py.
"""
import math
import os
import re

import numpy as np
import pytest

from adipose_amd import sharpen as SH

D = np.float64
F = np.float32


def textured(shape, seed=0):
    """A sinusoid plus noise of deviation 25 around 110: no flat run."""
    rng = np.random.default_rng([seed, *shape])
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    g = 110 + 40 * np.sin(yy / 5.0) * np.cos(xx / 7.0) + rng.normal(0, 25, shape)
    return np.clip(np.rint(g), 0, 255).astype(np.uint8)


# ---------------------------------------------------------------- definition
def test_radius_table():
    for sigma, r in ((0.0624, 0), (0.0626, 1), (1.0, 4), (2.3, 9), (16.0, 64)):
        assert SH.radius(sigma) == r
    for r in range(1, 65):
        assert SH.radius(r / 4) == r                       # 8 sigma + 1 = 2r + 1: what the GPU tests use
    assert SH.radius(0.01) == 0
    with pytest.raises(ValueError, match="64"):
        SH.radius(16.25)                                   # r = 65
    with pytest.raises(ValueError, match="64"):
        SH.radius(1e6)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            SH.radius(bad)


def test_taps_sum_and_sign():
    for sigma in (0.01, 0.0626, 0.3, 0.5, 1.0, 2.3, 4.0, 4.25, 7.7, 16.0):
        q = SH.taps(sigma)
        assert len(q) == SH.radius(sigma) + 1
        assert all(isinstance(v, int) and v >= 0 for v in q)
        assert q[0] + 2 * sum(q[1:]) == 1 << 24 == SH.ONE
        assert all(a >= b for a, b in zip(q, q[1:]))
        # the taps are the definition's
        w = [math.exp(-(i * i) / (2.0 * sigma * sigma)) for i in range(len(q))]
        T = math.fsum(w[:0:-1] + w)
        assert q[1:] == [int(np.rint(D(v) / D(T) * D(1 << 24))) for v in w[1:]]
    assert SH.taps(0.01) == [1 << 24]


def fold_slow(p, n):
    """Reflect at the two ends one step at a time."""
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * (n - 1) - p
    return p


def test_fold():
    assert [SH.fold(p, 5) for p in range(-9, 14)] == [1, 0, 1, 2, 3, 4, 3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1, 0, 1, 2, 3, 4, 3]
    assert [SH.fold(p, 2) for p in range(-5, 6)] == [1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1]
    for n in (1, 2, 5):
        period = max(2 * (n - 1), 1)
        ps = np.arange(-3 * period - 2, 3 * period + n + 3)        # beyond two periods both ways
        want = [fold_slow(int(p), n) for p in ps]
        assert [SH.fold(int(p), n) for p in ps] == want
        assert np.array_equal(SH.fold(ps, n), want)
    with pytest.raises(ValueError):
        SH.fold(0, 0)


def int_blur(img, q):
    """S from Python ints, pixel by pixel."""
    H, W = img.shape
    r = len(q) - 1
    v = [[int(x) for x in row] for row in img]
    S = np.empty((H, W), object)
    for y in range(H):
        for x in range(W):
            S[y, x] = sum(q[abs(j)] * sum(q[abs(i)] * v[fold_slow(y + j, H)][fold_slow(x + i, W)] for i in range(-r, r + 1))
                          for j in range(-r, r + 1))
    return S


def test_blur_sum_against_python_ints():
    img = np.random.default_rng(1).integers(0, 256, (3, 5), dtype=np.uint8)
    q = SH.taps(2.0)
    assert len(q) - 1 == 8                                         # r exceeds both extents
    want = int_blur(img, q)
    S = SH.blur_sum_np(img, 2.0)
    assert S.dtype == np.int64 and [int(v) for v in S.ravel()] == list(want.ravel())
    # and the finish, written out with numpy scalars
    for amount in (0.5, -0.7, 3.0):
        out = SH.sharpen_np(img, 2.0, amount)
        for y in range(3):
            for x in range(5):
                Dv = int(img[y, x]) * (1 << 48) - want[y, x]
                d = D(Dv) * D(2.0 ** -48)
                t = D(int(img[y, x])) + D(amount) * d
                assert out[y, x] == int(min(max(t, D(0)), D(255)))
    # the maximum of S: all 255 at the largest radius
    big = np.full((4, 3), 255, np.uint8)
    assert (SH.blur_sum_np(big, 16.0) == 255 * (1 << 48)).all()


def test_flat_images_are_fixed_points():
    for level in (0, 37, 255):
        img = np.full((9, 13), level, np.uint8)
        for sigma in (0.01, 0.3, 1.0, 2.3, 16.0):
            assert (SH.blur_sum_np(img, sigma) == level * (1 << 48)).all()
            for amount in (0.5, -2.0, 1e6, -1e6):
                assert (SH.sharpen_np(img, sigma, amount) == level).all()


def test_identity_cases():
    img = textured((21, 34))
    for sigma in (0.5, 1.0, 4.0):
        assert np.array_equal(SH.sharpen_np(img, sigma, 0.0), img)           # amount 0
    for amount in (0.5, -3.0, 100.0):
        assert np.array_equal(SH.sharpen_np(img, 0.05, amount), img)         # r = 0
    assert np.array_equal(SH.blur_sum_np(img, 0.05), img.astype(np.int64) << 48)
    # it does something otherwise: sharpening raises the deviation, a negative amount blurs
    assert SH.sharpen_np(img, 1.0, 0.5).astype(D).std() > img.astype(D).std() > SH.sharpen_np(img, 1.0, -0.5).astype(D).std()
    one = np.array([[200]], np.uint8)
    assert SH.sharpen_np(one, 16.0, 0.5)[0, 0] == 200


def test_float_input_is_rounded_and_clamped():
    f = np.array([[-3.0, 0.4, 0.5, 1.5], [2.5, 3.5, 255.5, 300.0], [17.2, 99.9, 128.0, 64.49]], np.float32)
    u = np.array([[0, 0, 0, 2], [2, 4, 255, 255], [17, 100, 128, 64]], np.uint8)
    assert np.array_equal(SH.sharpen_np(f, 0.05, 0.5), u)                    # the load itself
    assert np.array_equal(SH.blur_sum_np(f, 1.0), SH.blur_sum_np(u, 1.0))
    want = SH.sharpen_np(u, 1.0, 0.5)
    assert np.array_equal(SH.sharpen_np(f, 1.0, 0.5), want)
    out = SH.sharpen_np(f, 1.0, 0.5, np.float32)
    assert out.dtype == np.float32 and np.array_equal(out, want.astype(np.float32))
    # the surface keeps the input's dtype and container (on a host with a device it goes through it: the same bits)
    assert SH.sharpen_image(f).dtype == np.float32 and SH.sharpen_image(u).dtype == np.uint8
    assert np.array_equal(SH.sharpen_image(f, 1.0, 0.5), want.astype(np.float32))
    assert np.array_equal(SH.sharpen_image(u, 2.3, 0.7), SH.sharpen_np(u, 2.3, 0.7))
    import torch
    t = SH.sharpen_image(torch.from_numpy(u), 1.0, 0.5)
    assert isinstance(t, torch.Tensor) and not t.is_cuda and t.dtype == torch.uint8 and np.array_equal(t.numpy(), want)


def test_batch_is_image_by_image():
    b = np.stack([textured((37, 53), 1), np.full((37, 53), 200, np.uint8), textured((37, 53), 2)])
    out = SH.sharpen_np(b, 2.3, 0.7)
    S = SH.blur_sum_np(b, 2.3)
    assert out.shape == b.shape and S.shape == b.shape
    for i in range(3):
        assert np.array_equal(out[i], SH.sharpen_np(b[i], 2.3, 0.7)) and np.array_equal(S[i], SH.blur_sum_np(b[i], 2.3))


def test_argument_errors():
    img = textured((8, 8))
    for sigma in (0.0, -1.0, float("nan"), float("inf"), 16.25):
        for fn in (lambda: SH.sharpen_np(img, sigma, 0.5), lambda: SH.sharpen_image(img, sigma, 0.5),
                   lambda: SH.blur_sum_np(img, sigma), lambda: SH.taps(sigma), lambda: SH.UnsharpMask(sigma)):
            with pytest.raises(ValueError):
                fn()
    for amount in (float("nan"), float("inf"), -float("inf")):
        for fn in (lambda: SH.sharpen_np(img, 1.0, amount), lambda: SH.sharpen_image(img, 1.0, amount),
                   lambda: SH.UnsharpMask(1.0, amount)):
            with pytest.raises(ValueError):
                fn()
    with pytest.raises(ValueError):
        SH.sharpen_np(img[None, None])                 # 4-D
    with pytest.raises(ValueError):
        SH.sharpen_np(img[0])                          # 1-D
    with pytest.raises(ValueError):
        SH.sharpen_np(np.zeros((0, 4), np.uint8))
    with pytest.raises(TypeError):
        SH.sharpen_np(img.astype(np.int32))


def test_unsharp_mask_object():
    u = SH.UnsharpMask()
    assert (u.sigma, u.amount, u.radius) == (1.0, 0.5, 4)
    assert repr(u) == "UnsharpMask(sigma=1.0, amount=0.5)"
    assert repr(SH.UnsharpMask(2.3, -0.25)) == "UnsharpMask(sigma=2.3, amount=-0.25)"
    img = textured((30, 41))
    assert np.array_equal(u(img), SH.sharpen_np(img, 1.0, 0.5))
    assert np.array_equal(SH.UnsharpMask(4, 0.3)(img.astype(np.float32)), SH.sharpen_np(img, 4.0, 0.3, np.float32))


# ---------------------------------------------------------------- the reference's formula
def ref_sharpen(img, sigma, amount):
    """sharpen_image restated: cv2.GaussianBlur of a float32 image with ksize (0, 0), in float32 numpy."""
    n = int(np.rint(sigma * 8 + 1)) | 1
    r = n >> 1
    k = np.exp(-(np.arange(n, dtype=D) - r) ** 2 / (2.0 * sigma * sigma))
    k = (k / k.sum()).astype(F)                                     # cv2.getGaussianKernel(n, sigma, CV_32F)
    f = img.astype(F)
    H, W = f.shape
    p = np.take(f, SH.fold(np.arange(-r, W + r), W), axis=1)
    rows = np.zeros((H, W), F)
    for i in range(n):
        rows = rows + k[i] * p[:, i:i + W]
    p = np.take(rows, SH.fold(np.arange(-r, H + r), H), axis=0)
    blur = np.zeros((H, W), F)
    for i in range(n):
        blur = blur + k[i] * p[i:i + H, :]
    s = f + F(amount) * (f - blur)
    assert s.dtype == F
    return np.clip(s, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("shape", [(67, 131), (65, 257), (200, 513)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("sigma,amount", [(1, 0.5), (0.5, 1), (2.3, 0.7), (4, 0.3), (16, 0.5), (1, 2.5)])
def test_numpy_path_against_the_reference_formula(shape, sigma, amount):
    img = textured(shape)
    got, want = SH.sharpen_np(img, sigma, amount), ref_sharpen(img, sigma, amount)
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print(f"max difference {d.max()}, pixels that differ {(d > 0).sum()} of {d.size}")
    assert d.max() <= 1 and (d > 0).mean() <= 0.002
    assert (got != img).mean() > 0.5                                # the comparison is not of two identities


# ---------------------------------------------------------------- header and CLI
def test_constants_and_header():
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "adipose_hip.h")).read()
    val = {k: int(v) for k, v in re.findall(r"#define (ADP_SHARP_\w+) (\d+)", hdr)}
    assert (val["ADP_SHARP_RMAX"], val["ADP_SHARP_FUSED_RMAX"]) == (SH.RMAX, SH.FUSED_RMAX) == (64, SH.FUSED_RMAX)
    assert (val["ADP_SHARP_TILE_ROWS"], val["ADP_SHARP_TILE_COLS"]) == (SH.TILE_ROWS, SH.TILE_COLS)
    assert 4 <= SH.FUSED_RMAX < SH.RMAX                             # the default radius is fused; both forms exist
    assert int(re.search(r"#define ADP_ABI_VERSION (\d+)", hdr).group(1)) == 21


BASE = ["--images-dir", "i", "--output-dir", "o", "--weights", "w"]


def test_cli_flags():
    from cli import segmentation_inference as S
    a = S.build_parser().parse_args(BASE)
    assert (a.sharpen, a.sharpen_sigma, a.sharpen_amount) == (False, 1.0, 0.5)
    assert S.build_sharpen(a) is None
    a = S.build_parser().parse_args(BASE + ["--sharpen-sigma", "3", "--sharpen-amount", "2"])
    assert S.build_sharpen(a) is None                               # the values alone switch nothing on
    u = S.build_sharpen(S.build_parser().parse_args(BASE + ["--sharpen"]))
    assert (u.sigma, u.amount, u.radius) == (1.0, 0.5, 4)
    u = S.build_sharpen(S.build_parser().parse_args(BASE + ["--sharpen", "--sharpen-sigma", "2.3", "--sharpen-amount", "-0.5"]))
    assert (u.sigma, u.amount, u.radius) == (2.3, -0.5, 9)
    for bad in (["--sharpen-sigma", "16.25"], ["--sharpen-sigma", "0"], ["--sharpen-sigma", "nan"], ["--sharpen-amount", "inf"]):
        with pytest.raises(ValueError):
            S.build_sharpen(S.build_parser().parse_args(BASE + ["--sharpen"] + bad))
    # the other steps' flags are as they were
    assert S.build_illumination(a) is None and S.build_normalization(a) is None


def test_cli_refuses_sigma_before_a_model_is_loaded(tmp_path, capsys):
    from cli import segmentation_inference as S
    (tmp_path / "img").mkdir()
    rc = S.main(["--images-dir", str(tmp_path / "img"), "--output-dir", str(tmp_path / "out"), "--weights",
                 str(tmp_path / "no_such_weights"), "--sharpen", "--sharpen-sigma", "40"])
    out = capsys.readouterr().out
    assert rc == 1 and "limit is 64" in out and "Loading model" not in out


def test_predictor_takes_the_keyword():
    from adipose_amd.predictor import AdiposeUNet
    u = SH.UnsharpMask()
    m = AdiposeUNet(tile_size=64, sharpen=u)
    assert m.sharpen is u and AdiposeUNet(tile_size=64).sharpen is None
