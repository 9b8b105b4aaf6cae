"""The numpy path of adipose_amd.components (no GPU): canonical labels against scipy.ndimage.label, the pure-numpy
fallback against the same, known answers, and the reference's remove_small_components / connectedComponentsWithStats /
cell statistics surface. cv2 and skimage are not installed: parity with them is unpinned; scipy's labelling stands in.
"""
import numpy as np
import pytest

from adipose_amd import components as cc

SHAPES = [(1, 1), (1, 17), (13, 1), (7, 9), (64, 96), (257, 131)]
DENSITIES = [0.1, 0.45, 0.6, 0.9]
S8 = np.ones((3, 3), int)


@pytest.fixture(autouse=True)
def host_only(monkeypatch):
    """The host path, also where a GPU is present."""
    monkeypatch.setattr(cc, "_gpu", lambda: False)


def bernoulli(shape, density, seed=0):
    return np.random.default_rng(seed + int(density * 100) + 7 * shape[0] + shape[1]).random(shape) < density


def renumber_by_first(lab):
    """scipy's labels -> 1 + raster index of each component's first pixel."""
    out = np.zeros(lab.shape, np.int32)
    flat, o = lab.ravel(), out.ravel()
    for v in range(1, int(lab.max()) + 1):
        idx = np.flatnonzero(flat == v)
        o[idx] = idx[0] + 1
    return out


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_label_np_against_scipy(shape, density, connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    m = bernoulli(shape, density)
    want = renumber_by_first(ndi.label(m, structure=S8 if connectivity == 8 else None)[0])
    got = cc.label_np(m, connectivity)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(cc.label_np(m, connectivity, force_pure=True), want)   # the fallback of hosts without scipy
    assert np.array_equal(cc.label_np(m.astype(np.float32) * 0.5 + 0.25, connectivity, threshold=0.5), want)


def test_fallback_is_taken_without_scipy(monkeypatch):
    m = bernoulli((40, 50), 0.5)
    want = cc.label_np(m, 8)
    monkeypatch.setattr(cc, "_scipy_ndimage", lambda: None)
    monkeypatch.setattr(cc, "_label2d_scipy", None)
    assert np.array_equal(cc.label_np(m, 8), want)
    batch = np.stack([m, ~m])
    assert np.array_equal(cc.label_np(batch, 4)[1], cc.label_np(~m, 4))


def n_components(lab):
    return len(np.unique(lab)) - (1 if (lab == 0).any() else 0)


def serpentine(h, w):
    m = np.zeros((h, w), np.uint8)
    m[0::2] = 1
    m[1::4, -1] = 1
    m[3::4, 0] = 1
    return m


@pytest.mark.parametrize("pure", [False, True], ids=["scipy", "numpy"])
def test_known_answers(pure):
    L = lambda m, c: cc.label_np(m, c, force_pure=pure)   # noqa: E731
    z = np.zeros((5, 6), np.uint8)
    assert not L(z, 8).any() and not L(z, 4).any()
    assert (L(np.ones((5, 6), np.uint8), 4) == 1).all()
    d = np.zeros((3, 3), np.uint8)
    d[0, 1] = d[1, 2] = 1
    assert L(d, 8).tolist() == [[0, 2, 0], [0, 0, 2], [0, 0, 0]]
    assert L(d, 4).tolist() == [[0, 2, 0], [0, 0, 6], [0, 0, 0]]
    yy, xx = np.mgrid[0:7, 0:9]
    board = (yy + xx) % 2 == 0
    assert n_components(L(board, 8)) == 1 and n_components(L(board, 4)) == (7 * 9 + 1) // 2
    assert np.array_equal(L(board, 4), np.where(board, np.arange(1, 64).reshape(7, 9), 0))
    u = np.zeros((9, 7), np.uint8)
    u[:, 1] = u[:, 5] = 1
    u[8, 1:6] = 1
    for c in (4, 8):
        assert np.array_equal(L(u, c), u * 2)   # both arms carry the left arm's first pixel
    s = serpentine(17, 12)
    for c in (4, 8):
        assert np.array_equal(L(s, c), s)       # one component whose first pixel is pixel 0
    rings = np.zeros((11, 11), np.uint8)
    rings[0, :] = rings[-1, :] = rings[:, 0] = rings[:, -1] = 1
    rings[2, 2:9] = rings[8, 2:9] = rings[2:9, 2] = rings[2:9, 8] = 1
    rings[4:7, 4:7] = 1
    for c in (4, 8):
        lab = L(rings, c)
        assert sorted(np.unique(lab)) == [0, 1, 2 * 11 + 2 + 1, 4 * 11 + 4 + 1]
        assert cc.areas_np(lab).ravel()[[0, 24, 48]].tolist() == [40, 24, 9]


def reference_remove_small_components(mask, min_px, ndi):
    """build_dataset.py:1122-1131 transcribed, scipy's 8-connected labels standing in for cv2's."""
    if min_px <= 0:
        return mask
    labels, num = ndi.label(mask.astype(np.uint8), structure=S8)
    out = np.zeros_like(mask)
    for lbl in range(1, num + 1):
        if (labels == lbl).sum() >= min_px:
            out[labels == lbl] = 1
    return out


def test_remove_small_components():
    ndi = pytest.importorskip("scipy.ndimage")
    m = np.zeros((12, 20), np.uint8)
    m[1, 1:6] = 1        # 5 pixels
    m[4, 2:6] = 1        # 4 pixels
    m[7:9, 10:13] = 1    # 6 pixels
    m[10, 19] = 1
    assert cc.remove_small_components(m, 0) is m and cc.remove_small_components(m, -3) is m
    got = cc.remove_small_components(m, 5)   # exactly min_px is kept, min_px - 1 is dropped
    assert got[1, 1:6].all() and not got[4].any() and got[7:9, 10:13].all() and not got[10].any()
    for dtype in (np.uint8, np.float32, np.int32, bool):
        x = bernoulli((64, 96), 0.3, seed=3).astype(dtype)
        for min_px in (1, 2, 4, 9, 10 ** 6):
            got = cc.remove_small_components(x, min_px)
            assert got.dtype == x.dtype and got.shape == x.shape
            assert np.array_equal(got, reference_remove_small_components(x, min_px, ndi))
    with pytest.raises(ValueError):
        cc.remove_small_components(m, 3, connectivity=6)
    import torch
    t = torch.from_numpy(m)
    assert cc.remove_small_components(t, 0) is t
    gt = cc.remove_small_components(t, 5)
    assert isinstance(gt, torch.Tensor) and gt.dtype == torch.uint8 and np.array_equal(gt.numpy(), cc.remove_small_components(m, 5))


def test_connected_components_with_stats():
    ndi = pytest.importorskip("scipy.ndimage")
    m = bernoulli((37, 53), 0.4, seed=5).astype(np.uint8)
    n, labels, stats, cent = cc.connected_components_with_stats(m)
    sl, k = ndi.label(m, structure=S8)
    assert n == k + 1 and stats.shape == (n, 5) and stats.dtype == np.int32 and cent.shape == (n, 2) and cent.dtype == np.float64
    assert labels.dtype == np.int32 and np.array_equal(labels > 0, m > 0) and labels.max() == k
    assert stats[:, 4].sum() == m.size
    # dense labels follow the raster order of first pixels, which is scipy's order too
    assert np.array_equal(labels, sl)
    objs = ndi.find_objects(sl)
    com = ndi.center_of_mass(m, sl, range(1, k + 1))
    for i in range(1, n):
        ys, xs = objs[i - 1]
        assert stats[i].tolist() == [xs.start, ys.start, xs.stop - xs.start, ys.stop - ys.start, int((sl == i).sum())]
        assert abs(cent[i, 0] - com[i - 1][1]) < 1e-9 and abs(cent[i, 1] - com[i - 1][0]) < 1e-9
    yy, xx = np.nonzero(m == 0)
    assert stats[0].tolist() == [xx.min(), yy.min(), xx.max() - xx.min() + 1, yy.max() - yy.min() + 1, len(yy)]
    assert abs(cent[0, 0] - xx.mean()) < 1e-9 and abs(cent[0, 1] - yy.mean()) < 1e-9
    n1, l1, s1, c1 = cc.connected_components_with_stats(np.ones((4, 5), np.uint8), 4)
    assert n1 == 2 and s1.tolist() == [[0, 0, 0, 0, 0], [0, 0, 5, 4, 20]] and c1[1].tolist() == [2.0, 1.5]
    n0, l0, s0, _ = cc.connected_components_with_stats(np.zeros((4, 5), np.uint8))
    assert n0 == 1 and not l0.any() and s0.tolist() == [[0, 0, 5, 4, 20]]


def test_table_np_rows_limit():
    m = bernoulli((20, 30), 0.3, seed=8)
    lab = cc.label_np(m, 8)
    full, k = cc.table_np(lab, 1000)
    assert 5 < k < 1000 and not full[k:].any()
    assert np.array_equal(full[:k, 0], np.flatnonzero(lab.ravel() == np.arange(1, 601)))
    part, k2 = cc.table_np(lab, 5)
    assert k2 == k and np.array_equal(part, full[:5])
    assert np.array_equal(cc.areas_np(lab).ravel()[full[:k, 0]], full[:k, 1])


def test_cell_statistics():
    from adipose_amd.data import synthetic_tile
    _, mask = synthetic_tile(np.random.default_rng(4), size=256, channels=1)
    mask[::9, ::11] = 1.0   # specks: below 10 px unless they touch a cell
    st = cc.cell_statistics(mask)
    assert set(st) == {"num_cells", "areas", "tissue_coverage"}
    lab = cc.label_np(mask > 0.5, 8)
    a = cc.areas_np(lab).ravel()
    a = a[a > 0]
    assert (a < 10).any() and (a >= 10).any()
    assert st["num_cells"] == int((a >= 10).sum()) == len(st["areas"])
    assert st["areas"] == [float(v) for v in a[a >= 10]] and all(isinstance(v, float) for v in st["areas"])
    assert st["tissue_coverage"] == float((mask > 0.5).sum() / mask.size)
    assert cc.cell_statistics(mask, min_area=1)["num_cells"] == len(a)
    assert cc.cell_statistics(np.zeros((8, 8), np.float32)) == {"num_cells": 0, "areas": [], "tissue_coverage": 0.0}
    row = cc.cell_stats_row("t.png", st)
    assert len(row) == len(cc.CELL_STATS_HEADER) and row[1] == st["num_cells"]
    assert cc.cell_stats_row("t.png")[1:] == [0, "0.000", "0.000", "0.000", "0.000", "0.000000"]


def test_region_constants_match_the_header():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "adipose_hip.h")).read()
    vals = {k: int(v) for k, v in re.findall(r"#define (ADP_CC_[A-Z0-9_]+) (\d+)", src)}
    assert (vals["ADP_CC_REGION_ROWS"], vals["ADP_CC_REGION_COLS"]) == (cc.REGION_ROWS, cc.REGION_COLS)
    assert (vals["ADP_CC_SRC_U8"], vals["ADP_CC_SRC_F32"]) == (cc.SRC_U8, cc.SRC_F32)


def test_cli_parsers():
    from cli import full_evaluation_enhanced, reconstruct_full_images, segmentation_inference
    a = segmentation_inference.build_parser().parse_args(["--images-dir", "i", "--output-dir", "o", "--weights", "w"])
    assert a.min_cc_px == 0 and a.cell_stats is False and a.cell_min_area == 10
    a = segmentation_inference.build_parser().parse_args(
        ["--images-dir", "i", "--output-dir", "o", "--weights", "w", "--min-cc-px", "64", "--cell-stats", "--cell-min-area", "25"])
    assert (a.min_cc_px, a.cell_stats, a.cell_min_area) == (64, True, 25)
    base = ["--weights", "w", "--data-root", "d", "--output-dir", "o"]
    a = reconstruct_full_images.parse_args(base)
    assert a.min_cc_px == 0 and a.cell_stats is False and a.cell_min_area == 10
    a = reconstruct_full_images.parse_args(base + ["--min-cc-px", "300", "--cell-stats"])
    assert (a.min_cc_px, a.cell_stats) == (300, True)
    a = full_evaluation_enhanced.build_parser().parse_args(["--weights", "w", "--test-dataset", "d"])
    assert a.min_cc_px == 0
    from adipose_amd.reconstruct import _component_settings
    assert _component_settings(reconstruct_full_images.parse_args(base)) == {}
    assert _component_settings(a) == {}
    assert _component_settings(reconstruct_full_images.parse_args(base + ["--min-cc-px", "300"])) == {
        "min_cc_px": 300, "cell_stats": False, "cell_min_area": None}
