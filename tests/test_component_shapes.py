"""The numpy path of the per-component shape measures (adipose_amd.components, no GPU): shape_table_np's integer
sums, region_shapes' floats, cell_shapes, its CSV row and the CLI flags.

skimage is not installed, so the measures are defined by the formulas in region_shapes' docstring; the fixtures below
were worked out by hand from them. Where scipy imports, the label-equality form that shape_table_np evaluates over the
whole map is compared with the per-region form (binary_erosion + convolve on each component's own mask), which is how
skimage's perimeter(neighborhood=4) is written.
"""
import math
from fractions import Fraction

import numpy as np
import pytest

from adipose_amd import components as cc

RTOL = 1e-12
SQ2 = math.sqrt(2.0)


@pytest.fixture(autouse=True)
def host_only(monkeypatch):
    """The host path, also where a GPU is present."""
    monkeypatch.setattr(cc, "_gpu", lambda: False)


def close(got, want):
    return abs(got - want) <= RTOL * max(abs(want), 1e-300) if want else got == 0


def measure(mask, connectivity=8):
    """(shape rows, region_shapes' dict) of every component of a small mask placed away from the image edge."""
    m = np.pad(np.asarray(mask, np.uint8), 3)
    lab = cc.label_np(m, connectivity)
    tab, k = cc.table_np(lab, 64)
    shp = cc.shape_table_np(lab, 64)
    assert np.array_equal(shp[:, 0], tab[:, 0]) and not shp[k:].any()
    return shp[:k], {key: v[:k] for key, v in cc.region_shapes(tab, shp).items()}


def disc(r):
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    return xx * xx + yy * yy <= r * r


# mask, connectivity, (p_straight, p_diag, p_mixed) or None, perimeter, major, minor, eccentricity (None: not pinned)
FIXTURES = {
    "pixel": (np.ones((1, 1)), 8, (0, 0, 0), 0.0, 0.0, 0.0, 0.0),
    "square2": (np.ones((2, 2)), 8, (4, 0, 0), 4.0, None, None, None),
    "square3": (np.ones((3, 3)), 8, (8, 0, 0), 8.0, 4 * math.sqrt(2 / 3), 4 * math.sqrt(2 / 3), 0.0),
    "square5": (np.ones((5, 5)), 8, None, 16.0, None, None, None),
    "row5": (np.ones((1, 5)), 8, (3, 0, 0), 3.0, 4 * SQ2, 0.0, 1.0),
    "diagonal3": (np.eye(3), 8, (0, 1, 0), SQ2, None, None, None),
    "rect2x4": (np.ones((2, 4)), 8, None, None, 4 * math.sqrt(1.25), 2.0, math.sqrt(0.8)),
    "disc15": (disc(15), 8, (24, 12, 48), 24 + 12 * SQ2 + 48 * (1 + SQ2) / 2, None, None, 0.0),
}


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_hand_fixtures(name):
    mask, conn, counts, perimeter, major, minor, ecc = FIXTURES[name]
    shp, r = measure(mask, conn)
    assert len(shp) == 1
    if counts is not None:
        assert tuple(shp[0, 4:7]) == counts
    area = float(np.count_nonzero(mask))
    assert r["area"][0] == area
    if perimeter is not None:
        assert close(r["perimeter"][0], perimeter)
        assert close(r["circularity"][0], 4 * math.pi * area / (perimeter ** 2 + 1e-10))
    if major is not None:
        assert close(r["major_axis_length"][0], major) and close(r["minor_axis_length"][0], minor)
        assert close(r["aspect_ratio"][0], major / (minor + 1e-10))
    if ecc is not None:
        assert close(r["eccentricity"][0], ecc)
    if name == "disc15":
        assert r["major_axis_length"][0] == r["minor_axis_length"][0]
        assert (r["centroid_x"][0], r["centroid_y"][0]) == (18.0, 18.0)
    if name == "pixel":
        assert shp[0].tolist() == [3 * 7 + 3, 9, 9, 9, 0, 0, 0, 1]   # at (3, 3) of a 7 x 7 map


def bernoulli(shape, density, seed):
    return np.random.default_rng(seed + int(density * 100)).random(shape) < density


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("density", [0.3, 0.5, 0.7])
def test_counts_against_the_per_region_form(density, connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    m = bernoulli((40, 53), density, 11)
    lab = cc.label_np(m, connectivity)
    tab, k = cc.table_np(lab, 40 * 53)
    shp = cc.shape_table_np(lab, 40 * 53)
    assert k >= 1 and not shp[k:].any()
    cross = ndi.generate_binary_structure(2, 1)
    weights = np.array([[10, 2, 10], [2, 1, 2], [10, 2, 10]])
    for row in range(k):
        own = lab == tab[row, 0] + 1
        border = own & ~ndi.binary_erosion(own, cross, border_value=0)
        hist = np.bincount(ndi.convolve(border.astype(np.uint8), weights, mode="constant", cval=0)[border], minlength=50)
        want = [sum(int(hist[c]) for c in codes) for codes in cc.PERIMETER_CODES] + [int(border.sum())]
        assert shp[row, 4:8].tolist() == want, row
        yy, xx = np.nonzero(own)
        assert shp[row, :4].tolist() == [tab[row, 0], int((xx * xx).sum()), int((yy * yy).sum()), int((xx * yy).sum())]


def test_diagonal_touch_at_connectivity_4():
    """Two squares that meet at a corner are two components at connectivity 4, each measured as if alone."""
    m = np.zeros((8, 8), np.uint8)
    m[1:4, 1:4] = 1
    m[4:7, 4:7] = 1
    shp, r = measure(m, 4)
    assert len(shp) == 2
    for i in range(2):
        assert tuple(shp[i, 4:8]) == (8, 0, 0, 8) and close(r["perimeter"][i], 8.0) and r["eccentricity"][i] == 0.0
    shp8, _ = measure(m, 8)
    assert len(shp8) == 1 and shp8[0, 7] == 16   # joined: one component with both squares' border pixels


def test_row_limit_and_order():
    yy, xx = np.mgrid[0:9, 0:11]
    board = ((yy + xx) % 2 == 0).astype(np.uint8)
    lab = cc.label_np(board, 4)
    K = (9 * 11 + 1) // 2
    tab, k = cc.table_np(lab, K + 5)
    full = cc.shape_table_np(lab, K + 5)
    assert k == K and full.shape == (K + 5, 8) and not full[K:].any()
    assert np.array_equal(full[:, 0], tab[:, 0]) and (np.diff(full[:K, 0]) > 0).all()
    assert np.array_equal(cc.shape_table_np(lab, 7), full[:7])
    assert cc.shape_table_np(lab, 0).shape == (0, 8)
    assert full[3].tolist() == [6, 36, 0, 0, 0, 0, 0, 1]   # the single pixel at (0, 6)
    batch = cc.shape_table_np(np.stack([lab, np.zeros_like(lab), lab]), 7)
    assert batch.shape == (3, 7, 8) and np.array_equal(batch[0], full[:7]) and not batch[1].any()
    assert np.array_equal(batch[2], full[:7])
    with pytest.raises(ValueError):
        cc.shape_table_np(np.zeros((1, 2 ** 22), np.int32), 1)   # H * W * (W - 1)^2 = 2^66


def test_region_shapes_large_values():
    """A S_xx above 2^63: the numerators are exact integers, so the floats equal the same computation in Fractions."""
    H = W = 30000
    A = H * W   # the full 30000^2 image as one component
    Sx = H * (W * (W - 1) // 2)
    Sy = W * (H * (H - 1) // 2)
    Sxx = H * ((W - 1) * W * (2 * W - 1) // 6)
    Syy = W * ((H - 1) * H * (2 * H - 1) // 6)
    Sxy = (W * (W - 1) // 2) * (H * (H - 1) // 2) + 12345   # not quite symmetric: c != 0
    assert A * Sxx > 2 ** 63 and Sxx < 2 ** 63
    tab = np.array([[0, A, 0, 0, W - 1, H - 1, Sx, Sy]], np.int64)
    shp = np.array([[0, Sxx, Syy, Sxy, 4 * W - 8, 0, 4, 4 * W - 4]], np.int64)
    r = cc.region_shapes(tab, shp)
    a, b, c = (Fraction(A * Sxx - Sx * Sx, A * A), Fraction(A * Syy - Sy * Sy, A * A), Fraction(A * Sxy - Sx * Sy, A * A))
    d = math.sqrt(float(((a - b) / 2) ** 2 + c ** 2))
    l1, l2 = float((a + b) / 2) + d, max(float((a + b) / 2) - d, 0.0)
    assert close(r["major_axis_length"][0], 4 * math.sqrt(l1)) and close(r["minor_axis_length"][0], 4 * math.sqrt(l2))
    assert close(r["eccentricity"][0], math.sqrt(1 - l2 / l1))
    assert close(r["centroid_x"][0], (W - 1) / 2) and close(r["centroid_y"][0], (H - 1) / 2)
    # with int64 wrap-around instead, A * Sxx would be off by multiples of 2^64 / A^2 ~ 2e1: far outside 1e-12
    z = cc.region_shapes(np.zeros((2, 3, 8), np.int64), np.zeros((2, 3, 8), np.int64))
    assert all(v.shape == (2, 3) and not v.any() for v in z.values())
    assert set(z) == {"area", "perimeter", "circularity", "major_axis_length", "minor_axis_length", "aspect_ratio",
                      "eccentricity", "centroid_x", "centroid_y"}


def test_cell_shapes():
    from adipose_amd.data import synthetic_tile
    _, mask = synthetic_tile(np.random.default_rng(4), size=256, channels=1)
    mask[::9, ::11] = 1.0   # specks: below 10 px unless they touch a cell
    sh = cc.cell_shapes(mask)
    assert set(sh) == {"num_cells", "areas", "perimeters", "circularities", "aspect_ratios", "eccentricities",
                       "tissue_coverage"}
    st = cc.cell_statistics(mask)
    assert sh["num_cells"] == st["num_cells"] > 0 and sh["areas"] == st["areas"]
    assert sh["tissue_coverage"] == st["tissue_coverage"] and cc.stats_from_shapes(sh) == st
    st3 = cc.cell_statistics(mask, min_area=3, threshold=0.25)
    assert cc.stats_from_shapes(cc.cell_shapes(mask, min_area=3, threshold=0.25)) == st3
    for key in ("perimeters", "circularities", "aspect_ratios", "eccentricities"):
        assert len(sh[key]) == sh["num_cells"] and all(isinstance(v, float) for v in sh[key])
    assert all(0.0 <= e <= 1.0 for e in sh["eccentricities"]) and all(a >= 1.0 - 1e-9 for a in sh["aspect_ratios"])
    # the same numbers from the tables directly
    lab = cc.label_np(mask > 0.5, 8)
    tab, k = cc.table_np(lab, 10 ** 4)
    r = cc.region_shapes(tab[:k], cc.shape_table_np(lab, 10 ** 4)[:k])
    keep = r["area"] >= 10
    assert sh["perimeters"] == r["perimeter"][keep].tolist() and sh["eccentricities"] == r["eccentricity"][keep].tolist()
    assert sh["circularities"] == (4 * np.pi * r["area"] / (r["perimeter"] ** 2 + 1e-10))[keep].tolist()
    assert sh["aspect_ratios"] == (r["major_axis_length"] / (r["minor_axis_length"] + 1e-10))[keep].tolist()
    empty = cc.cell_shapes(np.zeros((8, 8), np.float32))
    assert empty == {"num_cells": 0, "areas": [], "perimeters": [], "circularities": [], "aspect_ratios": [],
                     "eccentricities": [], "tissue_coverage": 0.0}
    row = cc.cell_shapes_row("t.png", sh)
    assert len(row) == len(cc.CELL_SHAPES_HEADER) == 10 and row[:2] == ["t.png", sh["num_cells"]]
    assert row[2] == f"{np.mean(sh['perimeters']):.4f}" and row[9] == f"{np.median(sh['eccentricities']):.4f}"
    assert cc.cell_shapes_row("t.png")[1:] == [0] + ["0.0000"] * 8 == cc.cell_shapes_row("t.png", empty)[1:]
    # the statistics' surface is what it was
    assert cc.CELL_STATS_HEADER == ["name", "num_cells", "mean_area", "median_area", "min_area", "max_area", "tissue_coverage"]
    with pytest.raises(ValueError):
        cc.cell_shapes(np.zeros((2, 8, 8), np.float32))


def test_shape_tile_matches_the_header():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "adipose_hip.h")).read()
    vals = {k: int(v) for k, v in re.findall(r"#define (ADP_CC_[A-Z0-9_]+) (\d+)", src)}
    assert (vals["ADP_CC_SHAPE_TILE_ROWS"], vals["ADP_CC_SHAPE_TILE_COLS"]) == (cc.SHAPE_TILE_ROWS, cc.SHAPE_TILE_COLS)


def test_cli_parsers():
    from cli import reconstruct_full_images, segmentation_inference
    from adipose_amd.reconstruct import _component_settings
    seg = ["--images-dir", "i", "--output-dir", "o", "--weights", "w"]
    assert segmentation_inference.build_parser().parse_args(seg).cell_shapes is False
    a = segmentation_inference.build_parser().parse_args(seg + ["--cell-shapes", "--cell-min-area", "25"])
    assert (a.cell_shapes, a.cell_stats, a.cell_min_area) == (True, False, 25)
    base = ["--weights", "w", "--data-root", "d", "--output-dir", "o"]
    assert reconstruct_full_images.parse_args(base).cell_shapes is False
    a = reconstruct_full_images.parse_args(base + ["--cell-shapes"])
    assert a.cell_shapes is True and a.cell_stats is False
    assert _component_settings(a) == {"min_cc_px": 0, "cell_stats": False, "cell_min_area": 10, "cell_shapes": True}
    # without the flag: what it was
    assert _component_settings(reconstruct_full_images.parse_args(base)) == {}
    assert _component_settings(reconstruct_full_images.parse_args(base + ["--min-cc-px", "300"])) == {
        "min_cc_px": 300, "cell_stats": False, "cell_min_area": None}
    assert _component_settings(reconstruct_full_images.parse_args(base + ["--cell-stats"])) == {
        "min_cc_px": 0, "cell_stats": True, "cell_min_area": 10}
