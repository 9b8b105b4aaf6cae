"""Host-side checks of adipose_amd.stain (src/utils/stain_normalization.py:32-146, 312-438): the float64 numpy
conversions at the CIE fixed points, the semantics of the Reinhard transform, the class surface (reference loading,
metadata, batch files), the fused gray formula against PIL, and the inference CLI's two new flags. The colour
conversions restate skimage's documented rgb2lab / lab2rgb (D65, 2-degree observer): parity with skimage itself is
unpinned (skimage is not installed; the red triple below is its well-known value).

Sources and targets are always different images: with source = reference every value of the f64 path lands within
1e-15 of an integer before truncation and the result is noise.
"""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from adipose_amd import stain  # noqa: E402

PINK, PURPLE = (226, 168, 202), (186, 142, 208)


def histology_tile(seed, h, w, base, amp=28.0, noise=5.0):
    """A seeded histology-like uint8 RGB tile: a tinted base colour, smooth structure and noise."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    p = rng.rand(3)
    s = 0.5 * np.sin(2 * np.pi * (x / (7 + w / 3) + p[0])) * np.cos(2 * np.pi * (y / (5 + h / 2.5) + p[1])) \
        + 0.5 * np.sin(2 * np.pi * ((x + y) / (11 + (h + w) / 5) + p[2]))
    img = np.asarray(base, np.float64) + amp * s[..., None] * np.array([0.6, 1.0, 0.7]) + noise * rng.randn(h, w, 3)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def target_of(img):
    return stain.lab_stats_np(stain.rgb2lab_np(img / 255.0))


SRC = histology_tile(11, 64, 96, PINK)
TGT = target_of(histology_tile(12, 48, 80, PURPLE, amp=22.0))


@pytest.mark.parametrize("rgb, lab", [
    ((1, 1, 1), (100.0, -2.45493786e-3, 4.65342115e-3)),
    ((1, 0, 0), (53.24058794, 80.09230823, 67.20275104)),
    ((0, 0, 1), (32.29567257, 79.18559091, -107.85730021)),
    ((128 / 255, 128 / 255, 128 / 255), (53.5850135, -1.47264555e-3, 2.79145150e-3)),
])
def test_rgb2lab_fixed_points(rgb, lab):
    got = stain.rgb2lab_np(np.array(rgb, np.float64))
    assert np.abs(got - np.array(lab)).max() < 1e-6


def test_lab_round_trip():
    x = np.random.RandomState(0).rand(37, 41, 3)
    assert np.abs(stain.lab2rgb_np(stain.rgb2lab_np(x)) - x).max() < 1e-9


def test_inverse_matrix_first_row():
    assert np.allclose(stain.RGB_FROM_XYZ[0], (3.24048134, -1.53715152, -0.49853633), atol=1e-8)


def test_reinhard_matches_target_statistics():
    lab = stain.reinhard_lab_np(SRC, TGT)
    assert np.abs(stain.lab_stats_np(lab) - TGT).max() < 1e-9       # before quantisation: exactly the target
    out = stain.reinhard_np(SRC, TGT)
    err = np.abs(target_of(out) - TGT)
    print("post-quantisation |stats - target|:", err)
    assert err.max() < 0.5                                           # truncation biases L by about -0.2


def test_reinhard_range_rule():
    out = stain.reinhard_np(SRC, TGT)
    assert out.dtype == np.uint8 and out.shape == SRC.shape
    f = stain.reinhard_np(SRC / 255.0, TGT)
    assert f.dtype == np.float64 and 0.0 <= f.min() and f.max() <= 1.0
    # the float result is the uint8 one before truncation
    assert np.array_equal((f * 255).astype(np.uint8), out)


def test_zero_spread_channel_becomes_target_mean():
    # two equal values sum exactly, so numpy's std is exactly 0 here (for larger constant tiles it is ~1e-14, not 0)
    src = np.broadcast_to(np.array([200, 150, 180], np.uint8), (1, 2, 3))
    assert np.all(stain.lab_stats_np(stain.rgb2lab_np(src / 255.0))[3:] == 0)
    out = stain.reinhard_lab_np(src, TGT)
    for c in range(3):
        assert np.all(out[..., c] == TGT[c])
    want = (stain.lab2rgb_np(TGT[:3]) * 255).astype(np.uint8)
    assert np.all(stain.reinhard_np(src, TGT) == want)


def test_class_surface(tmp_path):
    from PIL import Image
    ref = histology_tile(12, 48, 80, PURPLE, amp=22.0)
    ref_path = tmp_path / "ref.png"
    Image.fromarray(ref).save(ref_path)
    nz = stain.ReinhardStainNormalizer(str(ref_path))
    assert set(nz.reference_lab_stats) == {"L", "A", "B"}
    assert set(nz.reference_lab_stats["L"]) == {"mean", "std"}
    got = [nz.reference_lab_stats[c]["mean"] for c in "LAB"] + [nz.reference_lab_stats[c]["std"] for c in "LAB"]
    assert np.allclose(got, TGT, rtol=0, atol=1e-12)
    info = nz.get_reference_info()
    assert info["reference_name"] == "ref.png" and info["lab_stats"] is nz.reference_lab_stats
    assert stain.ReinhardStainNormalizer().get_reference_info() == "No reference loaded"
    with pytest.raises(ValueError, match="No reference loaded"):
        stain.ReinhardStainNormalizer().normalize_image(SRC)
    with pytest.raises(FileNotFoundError):
        stain.ReinhardStainNormalizer(str(tmp_path / "missing.png"))
    Image.fromarray(ref[..., 0]).save(tmp_path / "gray.png")
    with pytest.raises(ValueError, match="Reference image must be RGB"):
        stain.ReinhardStainNormalizer(str(tmp_path / "gray.png"))

    # the six numbers alone
    nz2 = stain.ReinhardStainNormalizer()
    nz2.set_reference_stats(TGT)
    assert nz2.reference_lab_stats == nz.reference_lab_stats or np.allclose(
        stain._stats_vec(nz2.reference_lab_stats), TGT, rtol=0, atol=1e-12)
    f = nz2.normalize_image(SRC / 255.0)   # float input: the f64 numpy path on any host
    assert np.array_equal(f, stain.reinhard_np(SRC / 255.0, TGT))


def test_load_best_reference(tmp_path):
    from PIL import Image
    ref_path = tmp_path / "best.png"
    Image.fromarray(histology_tile(12, 48, 80, PURPLE, amp=22.0)).save(ref_path)
    meta = tmp_path / "meta.json"
    meta.write_text(json.dumps({"selected_reference": {"path": str(ref_path), "name": "best.png",
                                                        "composite_score": 0.9, "stain_type": "sybr_gold_eosin"}}))
    nz = stain.load_best_reference(meta)
    assert nz.reference_metadata["selected_reference"]["name"] == "best.png"
    assert np.allclose(stain._stats_vec(nz.reference_lab_stats), TGT, rtol=0, atol=1e-12)
    with pytest.raises(FileNotFoundError):
        stain.load_best_reference(tmp_path / "none.json")


def test_normalize_batch_writes_one_file_per_input(tmp_path, monkeypatch):
    from PIL import Image
    monkeypatch.setattr(stain, "_gpu", lambda: False)   # the file plumbing, on the numpy path everywhere
    nz = stain.ReinhardStainNormalizer()
    nz.set_reference_stats(TGT)
    src_dir, out_dir = tmp_path / "in", tmp_path / "out"
    src_dir.mkdir()
    names = ["a.png", "b.png", "c.tif"]
    for i, n in enumerate(names):
        Image.fromarray(histology_tile(20 + i, 12, 10, PINK)).save(src_dir / n)
    done = nz.normalize_batch(str(src_dir), output_dir=str(out_dir))
    assert sorted(p.name for p in done) == names == sorted(os.listdir(out_dir))
    a = np.array(Image.open(out_dir / "a.png"))
    assert np.array_equal(a, stain.reinhard_np(histology_tile(20, 12, 10, PINK), TGT))
    done = nz.normalize_batch([src_dir / "a.png", src_dir / "b.png"], output_dir=out_dir / "n", preserve_names=False)
    assert [p.name for p in done] == ["normalized_0000.png", "normalized_0001.png"]


def test_zscore_and_pipeline(monkeypatch):
    monkeypatch.setattr(stain, "_gpu", lambda: False)
    nz = stain.ReinhardStainNormalizer()
    nz.set_reference_stats(TGT)
    z = stain.normalize_with_zscore(SRC, mean=150.0, std=20.0)
    assert z.dtype == np.uint8 and abs(z.mean() - 150.0) < 1.0 and abs(z.std() - 20.0) < 1.0
    assert np.array_equal(stain.normalize_with_zscore(np.full((4, 4), 7, np.uint8)), np.full((4, 4), 7, np.uint8))
    out = stain.complete_preprocessing_pipeline(SRC, nz, apply_zscore=False)
    assert np.array_equal(out, stain.reinhard_np(SRC, TGT))
    assert np.array_equal(stain.complete_preprocessing_pipeline(SRC, nz), stain.normalize_with_zscore(out))


def test_gray_formula_is_pil_mode_l():
    from PIL import Image
    rgb = np.random.RandomState(3).randint(0, 256, (33, 47, 3)).astype(np.uint8)
    want = np.asarray(Image.fromarray(rgb).convert("L"), np.float32)
    assert np.array_equal(stain.gray_from_rgb_np(rgb), want)


def test_read_rgb(tmp_path):
    from PIL import Image

    from adipose_amd.data import read_gray, read_rgb
    rgb = histology_tile(4, 9, 13, PINK)
    Image.fromarray(rgb).save(tmp_path / "t.png")
    assert np.array_equal(read_rgb(tmp_path / "t.png"), rgb)
    assert np.array_equal(read_gray(tmp_path / "t.png"), stain.gray_from_rgb_np(rgb))


def test_inference_cli_stain_flags():
    from cli.segmentation_inference import build_parser
    base = ["--images-dir", "i", "--output-dir", "o", "--weights", "w"]
    a = build_parser().parse_args(base)
    assert a.stain_reference is None and a.stain_metadata is None
    assert (a.threshold, a.use_tta, a.tta_mode, a.save_overlays, a.overlay_color, a.save_probability, a.tile, a.dtype,
            a.batch) == (0.5, False, "basic", False, "cyan", False, 1024, "f32", 8)
    assert build_parser().parse_args(base + ["--stain-reference", "ref.png"]).stain_reference == "ref.png"
    assert build_parser().parse_args(base + ["--stain-metadata", "m.json"]).stain_metadata == "m.json"
    with pytest.raises(SystemExit):
        build_parser().parse_args(base + ["--stain-reference", "ref.png", "--stain-metadata", "m.json"])
