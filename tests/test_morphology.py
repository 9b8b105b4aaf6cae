"""The numpy path of adipose_amd.morphology (no GPU): footprints and the four operations against the statement of
OpenCV's construction in oracle/numpy_ref.py (cv_ellipse_rows / cv_morph, the functions the boundary refiner is pinned
to) and, for odd k, against scipy.ndimage; packing; the reference's morph_close surface; the CLIs' flag.
Everything is integers, so every comparison is array_equal. cv2 is not installed: parity with cv2 itself is unpinned.
"""
import functools

import numpy as np
import pytest

from adipose_amd import morphology as mo
from oracle import numpy_ref as O

KS = [1, 2, 3, 4, 5, 8, 15, 16, 31, 63]
SHAPES = [(1, 1), (2, 2), (7, 9), (5, 63), (5, 64), (5, 65), (33, 130)]
DENSITIES = [0.03, 0.5, 0.97]


@pytest.fixture(autouse=True)
def host_only(monkeypatch):
    """The host path, also where a GPU is present."""
    from adipose_amd import components
    monkeypatch.setattr(components, "_gpu", lambda: False)


@functools.lru_cache(maxsize=None)
def bernoulli(shape, density):
    m = np.random.default_rng(int(density * 100) + 7 * shape[0] + shape[1]).random(shape) < density
    m = m.astype(np.uint8)
    m.setflags(write=False)
    return m


@pytest.mark.parametrize("k", range(1, 64))
def test_ellipse_rows_are_the_oracles(k):
    lo, hi = mo.footprint_rows(k, "ellipse")
    want = O.cv_ellipse_rows(k)
    assert (list(lo), list(hi)) == (list(want[0]), list(want[1]))


def test_known_footprints():
    assert mo.footprint_array(mo.footprint_rows(5)).tolist() == [[0, 0, 1, 0, 0], [1] * 5, [1] * 5, [1] * 5, [0, 0, 1, 0, 0]]
    assert mo.footprint_array(mo.footprint_rows(2)).tolist() == [[0, 1], [1, 1]]
    assert mo.footprint_array(mo.footprint_rows(3, "rect")).tolist() == [[1] * 3] * 3
    assert mo.footprint_array(mo.footprint_rows(3, "cross")).tolist() == [[0, 1, 0], [1, 1, 1], [0, 1, 0]]
    assert mo.footprint_array(mo.footprint_rows(4, "cross")).tolist() == [[0, 0, 1, 0], [0, 0, 1, 0], [1] * 4, [0, 0, 1, 0]]
    for bad in (0, 64, -3):
        with pytest.raises(ValueError):
            mo.footprint_rows(bad)
    with pytest.raises(ValueError):
        mo.footprint_rows(3, "disk")


@pytest.mark.parametrize("kind", mo.SHAPES)
@pytest.mark.parametrize("k", KS)
def test_numpy_path_against_the_oracle(k, kind):
    rows = mo.footprint_rows(k, kind)
    for shape in SHAPES:
        for density in DENSITIES:
            m = bernoulli(shape, density)
            g = m * np.uint8(255)
            d, e = O.cv_morph(g, rows, True), O.cv_morph(g, rows, False)
            want = {"dilate": d, "erode": e, "close": O.cv_morph(d, rows, False), "open": O.cv_morph(e, rows, True)}
            got = {"dilate": mo.dilate_np, "erode": mo.erode_np, "close": mo.close_np, "open": mo.open_np}
            for name, fn in got.items():
                out = fn(m, k, kind)
                assert out.dtype == np.uint8 and out.shape == m.shape
                assert np.array_equal(out * np.uint8(255), want[name]), (name, k, kind, shape, density)


@pytest.mark.parametrize("k", [1, 3, 5, 7, 9, 15, 31, 63])
def test_numpy_path_against_scipy_odd_k(k):
    ndi = pytest.importorskip("scipy.ndimage")
    for kind in mo.SHAPES:
        se = mo.footprint_array(mo.footprint_rows(k, kind)).astype(bool)
        for shape in ((7, 9), (5, 65), (33, 130)):
            for density in DENSITIES:
                m = bernoulli(shape, density).astype(bool)
                d = ndi.binary_dilation(m, structure=se, border_value=0)
                assert np.array_equal(mo.dilate_np(m, k, kind), d)
                assert np.array_equal(mo.close_np(m, k, kind), ndi.binary_erosion(d, structure=se, border_value=1))
                assert np.array_equal(mo.erode_np(m, k, kind), ndi.binary_erosion(m, structure=se, border_value=1))


def test_batch_threshold_and_dtype():
    rng = np.random.default_rng(4)
    p = rng.random((3, 20, 70)).astype(np.float32)
    p[rng.random(p.shape) < 0.2] = 0.5   # background at thr = 0.5
    fg = (p > 0.5).astype(np.uint8)
    for fn in (mo.dilate_np, mo.erode_np, mo.close_np, mo.open_np):
        whole = fn(p, 4, threshold=0.5, dtype=np.float32)
        assert whole.dtype == np.float32 and set(np.unique(whole)) <= {0.0, 1.0}
        for n in range(3):
            assert np.array_equal(whole[n], fn(fg[n], 4))
    with pytest.raises(TypeError):
        mo.close_np(p, 3)
    with pytest.raises(ValueError):
        mo.close_np(np.zeros((1, 2, 3, 4), np.uint8), 3)
    assert np.array_equal(mo.dilate_np(fg, mo.footprint_rows(5, "cross")), mo.dilate_np(fg, 5, "cross"))


@pytest.mark.parametrize("shape", [(1, 1), (5, 63), (5, 64), (5, 65), (2, 3, 130)], ids=str)
def test_pack_roundtrip_and_tail(shape):
    m = (np.random.default_rng(1).random(shape) < 0.5).astype(np.uint8)
    W = shape[-1]
    bits = mo.pack_np(m)
    assert bits.dtype == np.uint64 and bits.shape == shape[:-1] + ((W + 63) // 64,)
    assert np.array_equal(mo.unpack_np(bits, W), m)
    assert np.array_equal(mo.unpack_np(bits, W, np.float32), m.astype(np.float32))
    if W % 64:
        assert not (bits[..., -1] >> np.uint64(W % 64)).any()
    assert int(bits[..., 0].ravel()[0]) & 1 == int(m.reshape(-1, W)[0, 0])   # bit 0 of word 0 is x = 0
    ones = mo.pack_np(np.ones(shape, bool))
    assert int(ones[..., -1].ravel()[0]) == (1 << (W % 64 or 64)) - 1
    assert np.array_equal(mo.pack_np(m.astype(np.float32) * 0.5 + 0.5, threshold=0.5), bits)


@pytest.mark.parametrize("kind", mo.SHAPES)
@pytest.mark.parametrize("k", [1, 2, 5, 8, 15])
def test_single_pixel_dilates_to_the_footprint(k, kind):
    rows = mo.footprint_rows(k, kind)
    se = mo.footprint_array(rows)
    c = k // 2
    H, W = 11, 70
    for py, px in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (5, 63), (5, 64), (4, 30)):
        m = np.zeros((H, W), np.uint8)
        m[py, px] = 1
        want = np.zeros((H, W), np.uint8)
        for a in range(k):
            for b in range(k):
                y, x = py - (a - c), px - (b - c)   # out(p - o) sees p through the offset o
                if se[a, b] and 0 <= y < H and 0 <= x < W:
                    want[y, x] = 1
        assert np.array_equal(mo.dilate_np(m, k, kind), want)


@pytest.mark.parametrize("k", KS)
def test_constant_masks(k):
    for shape in ((1, 1), (5, 65), (40, 7)):
        ones, zeros = np.ones(shape, np.uint8), np.zeros(shape, np.uint8)
        for kind in mo.SHAPES:
            assert np.array_equal(mo.erode_np(ones, k, kind), ones)
            for fn in (mo.dilate_np, mo.erode_np, mo.close_np, mo.open_np):
                assert np.array_equal(fn(zeros, k, kind), zeros)


def test_morph_close_surface():
    import torch
    m = bernoulli((33, 130), 0.5)
    for k in (0, -1):
        assert mo.morph_close(m, k) is m
        t = torch.from_numpy(m.copy())
        assert mo.morph_close(t, k) is t
    want = mo.close_np(m, 5)
    assert (want != m).any()
    got = mo.morph_close(m, 5)
    assert isinstance(got, np.ndarray) and got.dtype == m.dtype and np.array_equal(got, want)
    got = mo.morph_close(m.astype(np.float32), 5)
    assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32))
    got = mo.morph_close(m * np.uint8(255), 5)   # non-zero is foreground, the result is 0 / 1
    assert np.array_equal(got, want)
    got = mo.morph_close(torch.from_numpy(m.copy()), 5)
    assert isinstance(got, torch.Tensor) and not got.is_cuda and got.dtype == torch.uint8
    assert np.array_equal(got.numpy(), want)
    rows = mo.footprint_rows(5)
    assert np.array_equal(want * np.uint8(255), O.cv_morph(O.cv_morph(m * np.uint8(255), rows, True), rows, False))


def test_tile_constants_match_the_header():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "adipose_hip.h")).read()
    vals = {k: int(v) for k, v in re.findall(r"#define (ADP_MORPH_[A-Z0-9_]+) (\d+)", src)}
    assert (vals["ADP_MORPH_TILE_ROWS"], vals["ADP_MORPH_TILE_WORDS"]) == (mo.TILE_ROWS, mo.TILE_WORDS)
    assert (vals["ADP_MORPH_DILATE"], vals["ADP_MORPH_ERODE"], vals["ADP_MORPH_KMAX"]) == (mo.DILATE, mo.ERODE, mo.KMAX)
    assert mo.TILE_ROWS * mo.TILE_WORDS == 256   # one thread per output word


def test_cli_parsers():
    from cli import full_evaluation_enhanced, reconstruct_full_images, segmentation_inference
    inf = ["--images-dir", "i", "--output-dir", "o", "--weights", "w"]
    rec = ["--weights", "w", "--data-root", "d", "--output-dir", "o"]
    ev = ["--weights", "w", "--test-dataset", "d"]
    for parse, base in ((segmentation_inference.build_parser().parse_args, inf), (reconstruct_full_images.parse_args, rec),
                        (full_evaluation_enhanced.build_parser().parse_args, ev)):
        assert parse(base).morph_close_k == 0
        assert parse(base + ["--morph-close-k", "15"]).morph_close_k == 15
        assert parse(base + ["--morph-close-k", "63", "--min-cc-px", "9"]).min_cc_px == 9
        for bad in ("64", "-1"):
            with pytest.raises(SystemExit):
                parse(base + ["--morph-close-k", bad])
    for parser in (segmentation_inference.build_parser(), reconstruct_full_images.build_parser(),
                   full_evaluation_enhanced.build_parser()):
        assert "build_dataset.py --morph-close-k" in " ".join(parser.format_help().split())


def test_component_settings():
    from adipose_amd.reconstruct import _component_settings
    from cli import full_evaluation_enhanced, reconstruct_full_images
    base = ["--weights", "w", "--data-root", "d", "--output-dir", "o"]
    parse = reconstruct_full_images.parse_args
    assert _component_settings(parse(base)) == {}
    assert _component_settings(full_evaluation_enhanced.build_parser().parse_args(["--weights", "w", "--test-dataset", "d"])) == {}
    # without the new flag: the dicts of the existing tests
    assert _component_settings(parse(base + ["--min-cc-px", "300"])) == {
        "min_cc_px": 300, "cell_stats": False, "cell_min_area": None}
    assert _component_settings(parse(base + ["--cell-stats"])) == {"min_cc_px": 0, "cell_stats": True, "cell_min_area": 10}
    assert _component_settings(parse(base + ["--cell-shapes"])) == {
        "min_cc_px": 0, "cell_stats": False, "cell_min_area": 10, "cell_shapes": True}
    # with it: the three keys and its own
    assert _component_settings(parse(base + ["--morph-close-k", "5"])) == {
        "min_cc_px": 0, "cell_stats": False, "cell_min_area": None, "morph_close_k": 5}
    assert _component_settings(parse(base + ["--morph-close-k", "5", "--min-cc-px", "9", "--cell-stats"])) == {
        "min_cc_px": 9, "cell_stats": True, "cell_min_area": 10, "morph_close_k": 5}
