"""The polygon rasteriser on the GPU (csrc/polyraster.hip: adp_poly_raster) against the numpy path of
adipose_amd.annotations, which tests/test_annotations.py pins to the definition.

Everything is integers, so every comparison is array_equal, the raw 64-bit words included (the bits past W are zero):
there is no tolerance. The row scan covers C = ADP_POLY_SCAN_WORDS words a step and shares a wave among rows narrower
than that; a lane walks up to 32 rows of an edge alone and the wave walks a longer one together: the widths sit around
a word, C words and 2 C words, the heights are 1, 2 and 70, and the polygons have short and raster-high edges.
"""
import argparse
import functools
import json
import os
import shutil
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

C = 64   # ADP_POLY_SCAN_WORDS (asserted against the module below)
JSON_DIR = Path(os.path.dirname(__file__)) / "golden" / "annotations"
RECT = [(1, 1), (6, 1), (6, 5), (1, 5)]
KNOWN = [([RECT], 7, 8, 30), ([RECT, RECT], 7, 8, 18), ([[(-3, -3), (4, -3), (4, 4), (-3, 4)]], 6, 6, 25),
         ([[(0, 0), (6, 6), (6, 0), (0, 6)]], 7, 7, 31),
         ([[(0, 0), (4, 0), (4, 4), (0, 4)], [(2, 2), (6, 2), (6, 6), (2, 6)]], 8, 8, 40),
         ([[(1, 1), (6, 2), (3, 6)]], 8, 8, 19), ([[(2, 1)] * 3], 4, 4, 1), ([[(0, 3), (7, 3), (3, 3)]], 6, 8, 8)]
WIDTHS = [1, 63, 64, 65, 64 * C - 1, 64 * C, 64 * C + 1, 2 * 64 * C + 1]
HEIGHTS = [1, 2, 70]


def AN():
    from adipose_amd import annotations
    return annotations


def MO():
    from adipose_amd import morphology
    return morphology


def check(polys_per_image, H, W):
    """Device words == packed numpy raster, and the unpacked mask == the numpy raster. -> the numpy raster."""
    an, mo = AN(), MO()
    want = an.rasterize_np(polys_per_image, H, W)
    bits = an.rasterize_bits(polys_per_image, H, W)
    assert bits.dtype == torch.int64 and tuple(bits.shape) == (len(polys_per_image), H, (W + 63) // 64)
    assert np.array_equal(bits.cpu().numpy().view(np.uint64), mo.pack_np(want))
    got = an.rasterize(polys_per_image, H, W)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    return want


def test_constants():
    assert AN().SCAN_WORDS == C and AN().COORD_MAX == 2 ** 24


def test_known_answers():
    for polys, H, W, ones in KNOWN:
        assert int(check([polys], H, W).sum()) == ones
    # all of them as the images of one call (the largest raster: the smaller cases are clipped or padded by it)
    check([k[0] for k in KNOWN], 8, 8)


@functools.lru_cache(maxsize=None)
def shape_polys(H, W):
    """Two images of seeded polygons scaled to the raster: vertices up to a quarter outside on every side, one polygon with
    an edge through every row, one sliver, and a blob of short edges (an annotator's outline)."""
    rng = np.random.default_rng(H * 100003 + W)
    mx, my = max(W // 4, 4), max(H // 4, 4)
    images = []
    for _ in range(2):
        polys = [np.stack([rng.integers(-mx, W + mx, k), rng.integers(-my, H + my, k)], axis=1) for k in (3, 5, 9)]
        polys.append(np.array([(W // 3, -my), (W // 3 + 7, H + my), (2 * W // 3, H + my), (2 * W // 3 - 5, -my)]))
        polys.append(np.array([(-mx, H // 2), (W + mx, H // 2), (W // 2, H // 2 + 1)]))
        t = np.linspace(0, 2 * np.pi, 48, endpoint=False)
        cx, cy, r = rng.integers(0, W), rng.integers(0, H), rng.integers(2, 40)
        polys.append(np.stack([np.rint(cx + r * np.cos(t)), np.rint(cy + 0.6 * r * np.sin(t))], axis=1).astype(np.int64))
        images.append(polys)
    return images


@pytest.mark.parametrize("H", HEIGHTS)
@pytest.mark.parametrize("W", WIDTHS)
def test_shapes(H, W):
    want = check(shape_polys(H, W), H, W)
    assert want.any() or W * H < 4   # (the cases draw something)


def test_outside_far_flat_and_repeated():
    an = AN()
    H, W = 70, 64 * C + 1
    for side in ([(-90, 1), (-2, 1), (-2, 60)], [(W + 1, 1), (W + 300, 1), (W + 25, 60)], [(1, -90), (600, -2), (1, -2)],
                 [(1, H), (600, H + 30), (1, H + 30)]):
        assert not check([[np.array(side)]], H, W).any()   # wholly outside on each side (left of it: every toggle clamps to 0 twice)
    big = an.COORD_MAX
    far = [np.array([(-big, -big), (big, -big), (big, big), (-big, big)])]
    for h, w in ((70, 129), (2, 2 * 64 * C + 1), (1, 1)):
        assert check([far], h, w).all()   # (an edge 2^25 long is cut to the raster's rows before it is walked)
    assert check([[np.array([(-big, 3), (big, 5), (7, big)])]], 70, 65).any()
    flat = [np.array([(3, 9), (W + 40, 9), (-5, 9), (90, 9)]), np.array([(7, 2)] * 5), np.array([(5, 30), (5, 30), (400, 30)])]
    want = check([flat], H, W)[0]
    assert want[9].all() and want[2].sum() == 1 and want[30].sum() == 396 and want.sum() == W + 1 + 396
    # one edge through all rows, steep and shallow, both directions
    for poly in ([(0, 0), (W - 1, H - 1), (0, H - 1)], [(W - 1, 0), (0, H - 1), (W - 1, H - 1)], [(10, -5), (13, H + 5), (40, H + 5)],
                 [(3, 0), (3, H - 1), (4, 0)]):
        assert check([[np.array(poly)]], H, W).any()


def test_two_thousand_small_polygons_and_determinism():
    an = AN()
    rng = np.random.default_rng(2000)
    H, W = 300, 700
    polys = []
    for _ in range(2000):
        k = int(rng.integers(3, 9))
        c = np.array([rng.integers(-10, W + 10), rng.integers(-10, H + 10)])
        polys.append(c + rng.integers(-12, 13, (k, 2)))
    want = check([polys], H, W)
    assert 0.05 < want.mean() < 0.95
    a = an.rasterize_bits([polys], H, W).cpu().numpy()
    b = an.rasterize_bits([polys], H, W).cpu().numpy()
    assert np.array_equal(a, b)


def test_three_images_with_different_polygon_counts():
    rng = np.random.default_rng(3)
    H, W = 70, 130

    def some(n):
        return [np.stack([rng.integers(-9, W + 9, k), rng.integers(-9, H + 9, k)], axis=1) for k in rng.integers(3, 8, n)]
    images = [some(5), [], some(2)]
    want = check(images, H, W)
    assert want[0].any() and not want[1].any() and want[2].any()
    assert np.array_equal(want[2], AN().rasterize_np([images[2]], H, W)[0])
    check([[], []], 5, 70)   # no polygon at all: a zeroed plane
    assert tuple(AN().rasterize_bits([], 5, 70).shape) == (0, 5, 2)


def test_create_binary_mask_and_the_chain():
    an, mo = AN(), MO()
    from adipose_amd import components as cc
    polys = an.load_json_annotations(JSON_DIR / "slideA_fat_annotations.json", 2)[0]
    sub = an.load_json_annotations(JSON_DIR / "slideA_bubbles_annotations.json", 2)[0]
    H, W = 100, 130
    assert np.array_equal(an.create_binary_mask(polys, W, H), an.rasterize_np([polys], H, W)[0])
    assert np.array_equal(an.create_binary_mask(polys + [polys[0][:2]], W, H), an.rasterize_np([polys], H, W)[0])
    # a blob field with pinholes and specks, so that the closing and the filter both change pixels
    rng = np.random.default_rng(11)
    H, W = 150, 260
    blobs = []
    for _ in range(60):
        c = np.array([rng.integers(0, W), rng.integers(0, H)])
        r = int(rng.integers(1, 14))
        t = np.linspace(0, 2 * np.pi, 12, endpoint=False)
        blobs.append(c + np.rint(np.stack([r * np.cos(t), r * np.sin(t)], axis=1)).astype(np.int64))
    holes = [np.array([(x, y), (x + 2, y), (x + 2, y + 1)]) for x, y in rng.integers(0, (W, H), (80, 2))]
    raster = an.rasterize_np([blobs], H, W)[0]
    minus = raster & (1 - an.rasterize_np([holes], H, W)[0])
    closed = mo.close_np(minus, 5)
    lab = cc.label_np(closed, 8)
    want = cc.filter_np(lab, cc.areas_np(lab), 20)
    assert (minus != raster).any() and (closed != minus).any() and (want != closed).any()
    got = an.target_mask_bits(blobs, holes, H, W, 5, 20)
    assert tuple(got.shape) == (H, (W + 63) // 64)
    assert np.array_equal(got.cpu().numpy().view(np.uint64), mo.pack_np(want))
    assert np.array_equal(want, an.target_mask_np(blobs, holes, H, W, 5, 20))
    assert np.array_equal(an.target_mask_bits(blobs, None, H, W).cpu().numpy().view(np.uint64), mo.pack_np(raster))
    assert np.array_equal(an.target_mask_bits(blobs, holes, H, W).cpu().numpy().view(np.uint64), mo.pack_np(minus))


# ------------------------------------------------------------------------------ reconstruction
class FakePredictor:
    def predict_single(self, image, mean, std):
        h, w = image.shape
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        z = (image - mean) / (std + 1e-10)
        return (1.0 / (1.0 + np.exp(-(0.03 * yy - 0.05 * xx + 0.7 * z)))).astype(np.float32)


def tree(path):
    return {str(p.relative_to(path)): p.read_bytes() for p in sorted(Path(path).rglob("*")) if p.is_file()}


def test_reconstruction_takes_its_ground_truth_from_the_json(tmp_path):
    from PIL import Image

    from adipose_amd import reconstruct as R
    an = AN()
    T, S = 64, 32
    H, W = 96, 128   # 2 x 3 tiles a slide
    rng = np.random.default_rng(5)
    data = tmp_path / "data"
    (data / "images").mkdir(parents=True)
    (data / "masks").mkdir()
    for sid in ("slideA", "slideC"):   # slideA has a JSON, slideC has none
        img = rng.integers(0, 256, (H, W)).astype(np.uint8)
        gt = (rng.random((H, W)) < 0.4).astype(np.uint8)
        for r in range(2):
            for c in range(3):
                t = img[r * S:r * S + T, c * S:c * S + T]
                Image.fromarray(np.stack([t, t, t], axis=-1)).save(data / "images" / f"{sid}_r{r}_c{c}.jpg", format="PNG")
                Image.fromarray(gt[r * S:r * S + T, c * S:c * S + T]).save(data / "masks" / f"{sid}_r{r}_c{c}.tif", format="TIFF")
    masks = tmp_path / "Masks"
    (masks / "fat").mkdir(parents=True)
    (masks / "bubbles").mkdir()
    shutil.copy(JSON_DIR / "slideA_fat_annotations.json", masks / "fat")
    shutil.copy(JSON_DIR / "slideA_bubbles_annotations.json", masks / "bubbles")
    ck = tmp_path / "ckpt"
    ck.mkdir()
    (ck / "normalization_stats.json").write_text(json.dumps({"mean": 120.0, "std": 40.0}))

    def run(name, **kw):
        args = argparse.Namespace(weights=str(ck / "w.weights.h5"), data_root=str(data), output_dir=str(tmp_path / name),
                                  tile_size=T, stride=S, threshold=0.5, blend_mode="gaussian", use_tta=False,
                                  tta_mode="basic", boundary_refine=False, refine_kernel=5, save_metrics=True,
                                  min_coverage=0.9, max_tiles=None, **kw)
        return R.reconstruct_all_slides(args, model=FakePredictor())

    def gt_of(out, sid):
        with Image.open(out / sid / "ground_truth_mask.tif") as im:
            return np.asarray(im)

    off = run("off")
    on = run("on", annotations_dir=str(masks))
    both = run("both", annotations_dir=str(masks), gt_morph_close_k=5, gt_min_cc_px=20, min_cc_px=3)
    nosub = run("nosub", annotations_dir=str(masks), annotation_subtract_class="none", annotation_min_confidence=3)
    polys = an.load_json_annotations(JSON_DIR / "slideA_fat_annotations.json", 2)[0]
    sub = an.load_json_annotations(JSON_DIR / "slideA_bubbles_annotations.json", 2)[0]
    want = an.target_mask_np(polys, sub, H, W)
    assert want.any() and np.array_equal(gt_of(on, "slideA"), want * np.uint8(255))
    assert not np.array_equal(gt_of(on, "slideA"), gt_of(off, "slideA"))
    assert np.array_equal(gt_of(both, "slideA"), an.target_mask_np(polys, sub, H, W, 5, 20) * np.uint8(255))
    polys3 = an.load_json_annotations(JSON_DIR / "slideA_fat_annotations.json", 3)[0]
    assert np.array_equal(gt_of(nosub, "slideA"), an.rasterize_np([polys3], H, W)[0] * np.uint8(255))
    # the slide without a JSON: the same files as without the flag, but for the new entry of its metrics JSON
    t_off, t_on = tree(off), tree(on)
    assert set(t_off) == set(t_on)
    for name in t_off:
        if name.startswith("slideC/"):
            assert t_off[name] == t_on[name], name
    for sid in ("slideA", "slideC"):
        assert t_off[f"{sid}/prediction_mask.tif"] == t_on[f"{sid}/prediction_mask.tif"]
        assert t_off[f"{sid}/original_image.tif"] == t_on[f"{sid}/original_image.tif"]
    m_off = json.loads(t_off["metrics/slideC_metrics.json"])
    m_on = json.loads(t_on["metrics/slideC_metrics.json"])
    assert "ground_truth_source" not in m_off and m_on.pop("ground_truth_source") == "mask_tiles" and m_on == m_off
    assert json.loads(t_on["metrics/slideA_metrics.json"])["ground_truth_source"] == "annotations"
    log_off = json.loads(t_off["reconstruction_log.json"])
    log_on = json.loads(t_on["reconstruction_log.json"])
    assert "annotations_dir" not in log_off["configuration"] and "ground_truth_source" not in log_off["slide_results"][0]
    assert log_on["configuration"]["annotations_dir"] == str(masks) and log_on["configuration"]["annotation_class"] == "fat"
    assert [r["ground_truth_source"] for r in log_on["slide_results"]] == ["annotations", "mask_tiles"]
