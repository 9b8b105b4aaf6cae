"""Tile quality control on the host (adipose_amd.quality: qc_sums_np, measures, TileQC) and the inference CLI's flags.

qc_sums_np restates OpenCV 4's 8-bit BGR2GRAY and cv2.Laplacian (ksize 1, reflect-101 borders); cv2 is not installed, so
parity with cv2 itself is unpinned. The reference here is an independent float64 restatement written below: the same
gray formula and the Laplacian by explicit index arithmetic. Every value is an integer far below 2^53, so the float64
sums are exact and must equal the integer ones.
"""
import numpy as np
import pytest

from adipose_amd import quality as Q

PINK, WHITE = (226, 168, 202), (245, 244, 246)


def histology_tile(seed, h, w, base, amp=28.0, noise=5.0):
    """A seeded histology-like uint8 RGB tile (the generator of test_gpu_stain.py)."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    p = rng.rand(3)
    s = 0.5 * np.sin(2 * np.pi * (x / (7 + w / 3) + p[0])) * np.cos(2 * np.pi * (y / (5 + h / 2.5) + p[1])) \
        + 0.5 * np.sin(2 * np.pi * ((x + y) / (11 + (h + w) / 5) + p[2]))
    img = np.asarray(base, np.float64) + amp * s[..., None] * np.array([0.6, 1.0, 0.7]) + noise * rng.randn(h, w, 3)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


TISSUE = histology_tile(5, 64, 96, PINK)
BLURRY = histology_tile(5, 64, 96, PINK, noise=0.0)
EMPTY = histology_tile(5, 64, 96, WHITE, amp=4.0, noise=2.0)


def float_reference(tile, thr=235):
    """{white, S1, S2, n} of one (H, W, 3) tile in float64, index by index."""
    t = tile.astype(np.float64)
    H, W = t.shape[:2]
    gray = np.floor((t[..., 0] * 9798.0 + t[..., 1] * 19235.0 + t[..., 2] * 3735.0 + 16384.0) / 32768.0)

    def r101(i, n):
        return -i if i < 0 else 2 * n - 2 - i if i >= n else i

    s1 = s2 = 0.0
    for y in range(H):
        for x in range(W):
            lap = gray[r101(y - 1, H), x] + gray[r101(y + 1, H), x] + gray[y, r101(x - 1, W)] + gray[y, r101(x + 1, W)] \
                - 4.0 * gray[y, x]
            s1 += lap
            s2 += lap * lap
    white = float(((t[..., 0] >= thr) & (t[..., 1] >= thr) & (t[..., 2] >= thr)).sum())
    return [white, s1, s2, float(H * W)]


@pytest.mark.parametrize("shape", [(2, 2), (2, 5), (7, 9), (33, 20)], ids=str)
def test_sums_against_float_restatement(shape):
    tiles = np.stack([histology_tile(3 + k, *shape, base, amp, noise)
                      for k, (base, amp, noise) in enumerate([(PINK, 28.0, 5.0), (WHITE, 4.0, 2.0), (PINK, 28.0, 0.0)])])
    got = Q.qc_sums_np(tiles)
    assert got.dtype == np.int64 and got.shape == (3, 4)
    for k in range(3):
        assert [float(v) for v in got[k]] == float_reference(tiles[k])
    assert [float(v) for v in Q.qc_sums_np(tiles[1], 246)[0]] == float_reference(tiles[1], 246)   # one tile, another threshold


def test_sums_against_scipy_mirror():
    ndimage = pytest.importorskip("scipy.ndimage")
    for tile in (TISSUE, EMPTY):
        lap = ndimage.laplace(Q.gray_cv_np(tile).astype(np.float64), mode="mirror")
        s = Q.qc_sums_np(tile)[0]
        assert float(s[1]) == lap.sum() and float(s[2]) == (lap * lap).sum()


def test_measures_against_numpy():
    for tile in (TISSUE, BLURRY, EMPTY):
        g = np.pad(Q.gray_cv_np(tile), 1, mode="reflect").astype(np.float64)
        lap = g[:-2, 1:-1] + g[2:, 1:-1] + g[1:-1, :-2] + g[1:-1, 2:] - 4 * g[1:-1, 1:-1]
        ratio, var = Q.measures(Q.qc_sums_np(tile))
        assert ratio.dtype == np.float64 and var.dtype == np.float64
        assert abs(var[0] - np.var(lap)) <= 1e-12 * np.var(lap)
        want = (tile >= 235).all(axis=-1).mean()
        assert abs(ratio[0] - want) <= 1e-12 * max(want, 1.0)


def test_three_classes_and_their_order():
    qc = Q.TileQC()
    assert (qc.white_threshold, qc.white_ratio_limit, qc.blurry_threshold) == (235, 0.70, 7.5)
    ratio, var = qc.measure(np.stack([TISSUE, BLURRY, EMPTY]))
    print("white_ratio", ratio, "lap_var", var)
    assert ratio[0] == 0 and ratio[2] == 1.0 and var[0] > 100 and var[1] < 5
    assert qc.classify(np.stack([TISSUE, BLURRY, EMPTY])) == ["tissue", "blurry", "empty"]
    assert qc.classify([EMPTY, TISSUE]) == ["empty", "tissue"]     # a list of tiles
    assert qc.classify(TISSUE) == ["tissue"]                       # one tile
    # white and smooth: the white test comes first
    flat = np.full((16, 16, 3), 250, np.uint8)
    assert Q.measures(Q.qc_sums_np(flat))[1][0] == 0.0
    assert qc.classify(flat) == ["empty"]
    assert Q.TileQC(white_threshold=251).classify(flat) == ["blurry"]


def test_thresholds_at_equality():
    qc = Q.TileQC()
    # white_ratio = 7 / 10 = 0.70 exactly: not above the limit; lap_var = (2 * 15 - 0) / 4 = 7.5 exactly: not below
    assert Q.measures(np.array([[7, 0, 750, 10]]))[0][0] == 0.70 and Q.measures(np.array([[0, 0, 15, 2]]))[1][0] == 7.5
    assert qc.classes_from_sums(np.array([[7, 0, 750, 10], [8, 0, 750, 10]])) == ["tissue", "empty"]
    assert qc.classes_from_sums(np.array([[7, 0, 75, 10], [7, 0, 74, 10]])) == ["tissue", "blurry"]   # both at equality
    assert qc.classes_from_sums(np.array([[0, 0, 15, 2], [0, 0, 14, 2]])) == ["tissue", "blurry"]


def test_checkerboard():
    y, x = np.mgrid[0:12, 0:10]
    board = np.repeat((((y + x) & 1) * 255).astype(np.uint8)[..., None], 3, axis=-1)
    s = Q.qc_sums_np(board)[0]
    assert s.tolist() == [60, 0, 120 * 1040400, 120]
    assert Q.measures(s)[1][0] == 1040400.0


def test_n_times_s2_beyond_int64():
    n = 2048 * 2048
    assert n * (n * 1040400) > 2 ** 63
    ratio, var = Q.measures(np.array([[n // 2, 0, n * 1040400, n], [0, 10 * n, n * 1040400, n]], np.int64))
    assert var.tolist() == [1040400.0, 1040300.0] and ratio.tolist() == [0.5, 0.0]


def test_window_classes_on_the_host_or_the_device():
    img = np.concatenate([TISSUE[:, :64], EMPTY[:, :64]], axis=1)
    qc = Q.TileQC()
    assert qc.classify_windows(img, [(0, 0), (0, 64), (0, 48)], 64) == ["tissue", "empty", "empty"]
    assert qc.classify_windows(img, [], 64) == []


def test_bad_input():
    with pytest.raises(TypeError):
        Q.qc_sums_np(np.zeros((4, 4, 3), np.float32))
    with pytest.raises(ValueError):
        Q.qc_sums_np(np.zeros((1, 4, 3), np.uint8))


def test_inference_cli_tile_qc_flags():
    from cli.segmentation_inference import build_parser
    base = ["--images-dir", "i", "--output-dir", "o", "--weights", "w"]
    a = build_parser().parse_args(base)
    assert (a.tile_qc, a.white_threshold, a.white_ratio_limit, a.blurry_threshold, a.skip_blurry) == (
        False, 235, 0.70, 7.5, False)
    a = build_parser().parse_args(base + ["--tile-qc", "--white-threshold", "240", "--white-ratio-limit", "0.5",
                                          "--blurry-threshold", "12", "--skip-blurry"])
    assert (a.tile_qc, a.white_threshold, a.white_ratio_limit, a.blurry_threshold, a.skip_blurry) == (
        True, 240, 0.5, 12.0, True)
    # the flags of the rest of the parser are what they were
    assert (a.threshold, a.use_tta, a.tile, a.dtype, a.batch, a.stain_reference) == (0.5, False, 1024, "f32", 8, None)
