"""Column de-banding and the z-score / percentile stretch of adipose_amd.normalization: the numpy path against the
reference's formulas and the module's definition.

The reference (pre-post-processing_tools/preprocess_small_MS_SIMs.py:92-138, 249-286) computes in float32, and numpy's
float32 means are inexact on large images, so the numpy path is held to the formulas, restated here in float64 and in
the reference's float32, to within one gray level on at most 0.2 % of the pixels; the statistics themselves are held to
Python-int arithmetic exactly. The device path is held to this numpy path bit for bit in
tests/test_gpu_normalization.py.
"""
import math
import os
import re

import numpy as np
import pytest

from adipose_amd import normalization as NM

D = np.float64


def banded(H, W):
    rng = np.random.default_rng(0)
    a = np.clip((rng.integers(0, 256, (H, W)) * 0.5 + 60) * (1 + 0.3 * np.sin(np.arange(W) / 7)), 0, 255).astype(np.uint8)
    a[:, W // 3] = 77
    return a


def tissue():
    from adipose_amd.data import synthetic_tile
    return np.ascontiguousarray(synthetic_tile(np.random.default_rng(3), size=128, channels=3)[0][..., 0])


IMAGES = {"37x53": lambda: banded(37, 53), "257x300": lambda: banded(257, 300), "tissue": tissue}


# the reference's three functions, in the float type `F`
def ref_column(img, preserve_global, F):
    f = img.astype(F)
    gm, gs = f.mean(), f.std()
    cm = f.mean(axis=0, keepdims=True)
    cs = f.std(axis=0, keepdims=True) + 1e-10
    n = (f - cm) / cs
    if preserve_global:
        n = n * gs + gm
    else:
        n = ((n - n.min()) / (n.max() - n.min() + 1e-10) * 255)
    return np.clip(n, 0, 255).astype(np.uint8)


def ref_zscore(arr, F):
    f = arr.astype(F)
    n = (f - f.mean()) / (f.std() + 1e-10)
    return np.clip((n + 3) / 6 * 255, 0, 255).astype(np.uint8)


def ref_percentile(arr, p_low, p_high, F):
    f = arr.astype(F)
    lo, hi = np.percentile(f, (p_low, p_high))
    return (np.clip((f - lo) / max(hi - lo, 1e-3), 0, 1) * 255).astype(np.uint8)


def close_enough(got, want):
    """Every pixel within 1 gray level and at most 0.2 % of the pixels different."""
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print(f"max difference {d.max()}, share of pixels that differ {(d > 0).mean():.3g}")
    return d.max() <= 1 and (d > 0).mean() <= 0.002


@pytest.mark.parametrize("F", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("name", list(IMAGES))
def test_numpy_path_against_the_reference_formulas(name, F):
    img = IMAGES[name]()
    for pg in (True, False):
        assert close_enough(NM.column_normalize_np(img, pg), ref_column(img, pg, F))
    assert close_enough(NM.normalize_zscore_np(img), ref_zscore(img, F))
    for pl, ph in ((1.0, 99.0), (2.5, 97.5), (0.0, 100.0)):
        assert close_enough(NM.normalize_percentile_np(img, pl, ph), ref_percentile(img, pl, ph, F))


def int_stats(S1, S2, n):
    mean = D(S1) / D(n)
    ex2 = D(S2) / D(n)
    return mean, D(math.sqrt(max(ex2 - mean * mean, D(0))))


def expected_stats(img):
    """The definition from Python ints, column by column."""
    H, W = img.shape
    v = [[int(x) for x in img[:, c]] for c in range(W)]
    col = np.empty((W, 2), D)
    T1 = T2 = 0
    lo, hi = D(np.inf), D(-np.inf)
    for c in range(W):
        S1, S2 = sum(v[c]), sum(x * x for x in v[c])
        cm, cs = int_stats(S1, S2, H)
        col[c] = cm, cs + D(1e-10)
        T1, T2 = T1 + S1, T2 + S2
        lo = min(lo, (D(min(v[c])) - cm) / col[c, 1])
        hi = max(hi, (D(max(v[c])) - cm) / col[c, 1])
    gm, gs = int_stats(T1, T2, H * W)
    return col, np.array([gm, gs, lo, hi], D)


def test_statistics_are_exact():
    a = np.random.default_rng(1).integers(0, 256, (4099, 3), dtype=np.uint8)
    a[:, 1] = 255
    a[1234, 1] = 254                                  # one 254 among 255s: a deviation float32 sums lose
    col, glob = NM.column_stats_np(a)
    wc, wg = expected_stats(a)
    assert np.array_equal(col.view(np.int64), wc.view(np.int64)) and np.array_equal(glob.view(np.int64), wg.view(np.int64))
    assert col[1, 0] == D(255 * 4099 - 1) / D(4099) and 0 < col[1, 1] < 0.02
    # all 255 at 2048 x 2048: the sums pass 2^24, where a float32 sum is inexact
    b = np.full((2048, 2048), 255, np.uint8)
    col, glob = NM.column_stats_np(b)
    assert (col[:, 0] == 255).all() and (col[:, 1] == D(1e-10)).all()
    assert glob[0] == 255 and glob[1] == 0 and glob[2] == 0 and glob[3] == 0
    assert (NM.column_normalize_np(b, True) == 255).all() and (NM.column_normalize_np(b, False) == 0).all()
    assert (NM.normalize_zscore_np(b) == 127).all()


def test_column_normalize_written_out():
    """The element-wise end a second time, pixel by pixel with numpy scalars."""
    img = banded(9, 11)
    col, glob = expected_stats(img)
    gm, gs, lo, hi = glob
    for pg in (True, False):
        want = np.empty(img.shape, np.uint8)
        for y in range(9):
            for x in range(11):
                t = (D(img[y, x]) - col[x, 0]) / col[x, 1]
                t = t * gs + gm if pg else ((t - lo) / ((hi - lo) + D(1e-10))) * D(255)
                want[y, x] = int(min(max(t, D(0)), D(255)))
        assert np.array_equal(NM.column_normalize_np(img, pg), want)


def test_tables_written_out():
    img = banded(37, 53)
    h = np.bincount(img.ravel(), minlength=256)
    S1, S2 = sum(i * int(c) for i, c in enumerate(h)), sum(i * i * int(c) for i, c in enumerate(h))
    mean, std = int_stats(S1, S2, img.size)
    assert mean == D(int(img.astype(np.int64).sum())) / D(img.size)
    want = [int(min(max((((D(i) - mean) / (std + D(1e-10))) + D(3)) / D(6) * D(255), D(0)), D(255))) for i in range(256)]
    assert np.array_equal(NM.zscore_table(h), np.array(want, np.uint8))
    lo, hi = np.percentile(img.astype(D), (2.5, 97.5))
    scale = max(hi - lo, D(1e-3))
    want = [int(min(max((D(i) - lo) / scale, D(0)), D(1)) * D(255)) for i in range(256)]
    assert np.array_equal(NM.percentile_table(h, 2.5, 97.5), np.array(want, np.uint8))
    assert np.array_equal(NM.normalize_percentile_np(img, 2.5, 97.5), np.array(want, np.uint8)[img])


def test_degenerate_cases():
    const = np.full((12, 17), 93, np.uint8)
    assert (NM.normalize_zscore_np(const) == 127).all()
    assert (NM.normalize_percentile_np(const) == 0).all()          # (v - lo) / 1e-3 = 0
    assert (NM.column_normalize_np(const, True) == 93).all() and (NM.column_normalize_np(const, False) == 0).all()
    # a constant column gives t = 0 before the rescale: the image's mean with preserve_global
    a = banded(20, 9)
    col, glob = NM.column_stats_np(a)
    assert col[3, 0] == 77 and col[3, 1] == D(1e-10)
    assert (NM.column_normalize_np(a, True)[:, 3] == int(glob[0])).all()
    t0 = ((D(0) - glob[2]) / ((glob[3] - glob[2]) + D(1e-10))) * D(255)
    assert (NM.column_normalize_np(a, False)[:, 3] == int(t0)).all()
    # H = 1: every column is constant; W = 1: one column
    row = np.arange(40, dtype=np.uint8)[None, :] * 5
    assert (NM.column_normalize_np(row, True) == int(D(int(row.sum())) / D(40))).all()
    assert (NM.column_normalize_np(row, False) == 0).all()
    colimg = (np.arange(40, dtype=np.uint8) * 5)[:, None]
    out = NM.column_normalize_np(colimg, False)
    assert out[0, 0] == 0 and out[-1, 0] == 254 and (np.diff(out[:, 0].astype(int)) >= 0).all()   # 255 * (1 - 1e-10 / ..)
    one = np.array([[200]], np.uint8)
    assert NM.column_normalize_np(one, True)[0, 0] == 200 and NM.normalize_zscore_np(one)[0, 0] == 127
    assert NM.normalize_percentile_np(one)[0, 0] == 0
    for shape in ((1, 40), (40, 1)):
        v = np.random.default_rng(2).integers(0, 256, shape, dtype=np.uint8)
        assert close_enough(NM.normalize_zscore_np(v), ref_zscore(v, D))
        assert close_enough(NM.normalize_percentile_np(v), ref_percentile(v, 1.0, 99.0, D))
    # p_low = p_high: a step at the percentile; (0, 100): minimum to 0 and maximum to 255
    img = banded(37, 53)
    med = np.percentile(img.astype(D), 50.0)
    out = NM.normalize_percentile_np(img, 50.0, 50.0)
    assert (out[img <= med] == 0).all() and (out[img >= med + 1e-3] == 255).all()
    out = NM.normalize_percentile_np(img, 0.0, 100.0)
    assert out.min() == 0 and out.max() == 255
    assert np.array_equal(out, ref_percentile(img, 0.0, 100.0, D))


def test_float_input_is_rounded_and_clamped():
    f = np.array([[-3.0, 0.4, 0.5, 1.5], [2.5, 254.5, 255.5, 300.0], [17.2, 99.9, 128.0, 64.49]], np.float32)
    u = np.array([[0, 0, 0, 2], [2, 254, 255, 255], [17, 100, 128, 64]], np.uint8)
    for fn in (lambda a, dt: NM.column_normalize_np(a, True, dt), lambda a, dt: NM.column_normalize_np(a, False, dt),
               NM.normalize_zscore_np, lambda a, dt: NM.normalize_percentile_np(a, 1.0, 99.0, dt)):
        want = fn(u, np.uint8)
        assert np.array_equal(fn(f, np.uint8), want)
        out = fn(f, np.float32)
        assert out.dtype == np.float32 and np.array_equal(out, want.astype(np.float32))
    # the surface keeps the input's dtype and container
    assert NM.normalize_zscore(f).dtype == np.float32 and NM.normalize_zscore(u).dtype == np.uint8
    assert np.array_equal(NM.normalize_percentile(f, 5, 95), NM.normalize_percentile_np(u, 5, 95).astype(np.float32))
    assert np.array_equal(NM.remove_banding_column_normalize(u, False), NM.column_normalize_np(u, False))


def test_batch_is_image_by_image():
    b = np.stack([banded(37, 53), np.full((37, 53), 200, np.uint8),
                  np.random.default_rng(4).integers(0, 256, (37, 53), dtype=np.uint8)])
    col, glob = NM.column_stats_np(b)
    assert col.shape == (3, 53, 2) and glob.shape == (3, 4)
    for i in range(3):
        c1, g1 = NM.column_stats_np(b[i])
        assert c1.shape == (53, 2) and g1.shape == (4,)
        assert np.array_equal(col[i], c1) and np.array_equal(glob[i], g1)
        for pg in (True, False):
            assert np.array_equal(NM.column_normalize_np(b, pg)[i], NM.column_normalize_np(b[i], pg))
        assert np.array_equal(NM.normalize_zscore_np(b)[i], NM.normalize_zscore_np(b[i]))
        assert np.array_equal(NM.normalize_percentile_np(b, 2.0, 98.0)[i], NM.normalize_percentile_np(b[i], 2.0, 98.0))
    # a neighbour changes nothing
    b2 = b.copy()
    b2[1] = 3
    assert np.array_equal(NM.column_normalize_np(b2)[0], NM.column_normalize_np(b)[0])


def test_argument_errors():
    img = banded(8, 8)
    for lo, hi in ((60, 40), (-1, 99), (1, 100.5), (float("nan"), 99)):
        with pytest.raises(ValueError):
            NM.normalize_percentile_np(img, lo, hi)
        with pytest.raises(ValueError):
            NM.normalize_percentile(img, lo, hi)
        with pytest.raises(ValueError):
            NM.GrayNormalization(method="percentile", p_low=lo, p_high=hi)
    with pytest.raises(ValueError):
        NM.GrayNormalization(method="minmax")
    with pytest.raises(ValueError):
        NM.normalize_zscore_np(img[None, None])            # 4-D
    with pytest.raises(ValueError):
        NM.column_normalize_np(img[0])                     # 1-D
    with pytest.raises(ValueError):
        NM.column_normalize_np(np.zeros((0, 4), np.uint8))
    with pytest.raises(TypeError):
        NM.normalize_zscore_np(img.astype(np.int32))


def test_gray_normalization_object():
    img = banded(37, 53)
    g = NM.GrayNormalization()
    assert g.remove_banding(img) is img and g.normalize(img) is img and g(img) is img
    assert NM.GrayNormalization(method="none").method is None
    g = NM.GrayNormalization(column_banding=True, preserve_global=False, method="percentile", p_low=2, p_high=98)
    assert "column_banding=True" in repr(g) and "'percentile'" in repr(g) and "p_low=2.0" in repr(g)
    # (on a host with a device these go through it; the device equals the numpy path bit for bit)
    assert np.array_equal(g.remove_banding(img), NM.column_normalize_np(img, False))
    assert np.array_equal(g.normalize(img), NM.normalize_percentile_np(img, 2, 98))
    assert np.array_equal(g(img), NM.normalize_percentile_np(NM.column_normalize_np(img, False), 2, 98))
    z = NM.GrayNormalization(method="zscore")
    assert np.array_equal(z(img), NM.normalize_zscore_np(img))


def test_band_constants_and_header():
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "adipose_hip.h")).read()
    val = {k: int(v) for k, v in re.findall(r"#define (ADP_GNORM_\w+) (\d+)", hdr)}
    assert (val["ADP_GNORM_BAND_ROWS"], val["ADP_GNORM_BAND_COLS"]) == (NM.BAND_ROWS, NM.BAND_COLS)
    assert (val["ADP_GNORM_TALL_BLOCKS"], val["ADP_GNORM_TALL_FACTOR"]) == (NM.TALL_BLOCKS, NM.TALL_FACTOR)
    assert (val["ADP_GNORM_ZSCORE"], val["ADP_GNORM_PERCENTILE"]) == (NM.ZSCORE, NM.PERCENTILE)
    assert int(re.search(r"#define ADP_ABI_VERSION (\d+)", hdr).group(1)) == 21


def test_illumination_call_is_its_two_steps():
    from adipose_amd.illumination import IlluminationCorrection
    img = banded(60, 70)
    for ic in (IlluminationCorrection(banding=(1, 12), method="rolling-ball", radius=7),
               IlluminationCorrection(banding=(3, 9), method="tophat", kernel_size=15),
               IlluminationCorrection(banding=(1, 12)), IlluminationCorrection(method="rolling-ball", radius=5),
               IlluminationCorrection()):
        assert np.array_equal(ic(img), ic.correct(ic.remove_banding(img)))
    ic = IlluminationCorrection(banding=(1, 12), method="rolling-ball", radius=7)
    assert not np.array_equal(ic.remove_banding(img), img) and not np.array_equal(ic.correct(img), ic(img))
    none = IlluminationCorrection()
    assert none.remove_banding(img) is img and none.correct(img) is img


# ---------------------------------------------------------------- CLI
def test_cli_flags():
    from cli import segmentation_inference as S
    base = ["--images-dir", "i", "--output-dir", "o", "--weights", "w"]
    a = S.build_parser().parse_args(base)
    assert (a.normalization_method, a.percentile_low, a.percentile_high, a.column_preserve_global) == ("none", 1.0, 99.0, True)
    assert a.banding_method == "none"
    assert S.build_normalization(a) is None and S.build_illumination(a) is None
    a = S.build_parser().parse_args(base + ["--banding-method", "column"])
    g = S.build_normalization(a)
    assert (g.column_banding, g.preserve_global, g.method) == (True, True, None)
    assert S.build_illumination(a) is None                       # column is no morphological banding
    a = S.build_parser().parse_args(base + ["--banding-method", "column", "--column-preserve-global",
                                            "--illumination-method", "rolling-ball"])
    assert S.build_normalization(a).preserve_global is True
    c = S.build_illumination(a)
    assert (c.banding, c.method) == (None, "rolling-ball")
    a = S.build_parser().parse_args(base + ["--normalization-method", "percentile", "--percentile-low", "2.5",
                                            "--percentile-high", "97.5", "--banding-method", "morphological"])
    g = S.build_normalization(a)
    assert (g.column_banding, g.method, g.p_low, g.p_high) == (False, "percentile", 2.5, 97.5)
    assert S.build_illumination(a).banding == (1, 512)
    a = S.build_parser().parse_args(base + ["--normalization-method", "zscore"])
    g = S.build_normalization(a)
    assert (g.column_banding, g.method) == (False, "zscore")
    with pytest.raises(SystemExit):
        S.build_parser().parse_args(base + ["--illumination-method", "polynomial"])
    with pytest.raises(SystemExit):
        S.build_parser().parse_args(base + ["--normalization-method", "minmax"])
    with pytest.raises(SystemExit):
        S.build_parser().parse_args(base + ["--banding-method", "fft"])
    for bad in (["--normalization-method", "percentile", "--percentile-low", "60", "--percentile-high", "40"],
                ["--normalization-method", "zscore", "--percentile-high", "101"],
                ["--banding-method", "column", "--percentile-low", "-1"]):
        with pytest.raises(ValueError):
            S.build_normalization(S.build_parser().parse_args(base + bad))


def test_cli_refuses_percentiles_before_a_model_is_loaded(tmp_path, capsys):
    from cli import segmentation_inference as S
    (tmp_path / "img").mkdir()
    rc = S.main(["--images-dir", str(tmp_path / "img"), "--output-dir", str(tmp_path / "out"), "--weights",
                 str(tmp_path / "no_such_weights"), "--normalization-method", "percentile", "--percentile-low", "60",
                 "--percentile-high", "40"])
    out = capsys.readouterr().out
    assert rc == 1 and "p_low <= p_high" in out and "Loading model" not in out
