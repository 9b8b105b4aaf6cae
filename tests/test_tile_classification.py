"""Tile-level "Has Fat / No Fat" evaluation (adipose_amd.tile_classification vs
Segmentation/tile_classification_evaluation.py) on the host.

Golden vectors: tests/golden/tile_classification.npz, produced by the reference's own functions
(tests/golden/make_tile_classification_golden.py): calculate_fat_percentage of maps with values at and beside every
threshold, ground-truth percentages after the reference's normalisation for every kind of mask, classify_tile,
confusion matrices and metrics (all-one-class and empty lists included), the four naming helpers, and evaluate_tiles
on a 9-tile set with and without TTA. Everything is integer arithmetic up to one float64 division, so every comparison
is equality. The tile decode is pinned by construction (lossless PNG content under the reference's *.jpg names).
"""
import argparse
import csv
import json
import os
import re
from pathlib import Path

import numpy as np
import pytest

from adipose_amd import _lib
from adipose_amd import tile_classification as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "tile_classification.npz"))
MAP_THRESHOLDS = [float(t) for t in GOLD["map_thresholds"]]
KINDS = [str(k) for k in GOLD["gt_kinds"]]
SHAPES = [(17, 19), (64, 64)]
MEAN, STD = (float(v) for v in GOLD["mean_std"])


class FakePredictor:
    """Same deterministic predictor the golden generator used (make_golden.fake_predictor); counts its calls."""

    def __init__(self):
        self.calls = 0

    def predict_single(self, image, mean, std):
        self.calls += 1
        h, w = image.shape
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        z = (image - mean) / (std + 1e-10)
        return (1.0 / (1.0 + np.exp(-(0.03 * yy - 0.05 * xx + 0.7 * z + 0.001 * yy * xx / h)))).astype(np.float32)


def write_dataset(base):
    """The golden's 9-tile set under base/clean_test (PNG content under *.jpg names, TIFF masks; one tile has no
    mask), and the training statistics beside the weights path. Returns (data_root, weights path)."""
    from PIL import Image
    root, ckpt = Path(base) / "clean_test", Path(base) / "ckpt"
    (root / "images").mkdir(parents=True)
    (root / "masks").mkdir()
    ckpt.mkdir()
    for k in GOLD.files:
        if k.startswith("eval_tile_"):
            Image.fromarray(GOLD[k]).save(root / "images" / f"{k[10:]}.jpg", format="PNG")
        elif k.startswith("eval_mask_"):
            Image.fromarray(GOLD[k]).save(root / "masks" / f"{k[10:]}.tif", format="TIFF")
    (ckpt / "normalization_stats.json").write_text(json.dumps({"mean": MEAN, "std": STD}))
    return root, ckpt / "best.weights.h5"


def make_args(root, weights, **kw):
    a = dict(weights=str(weights), data_root=str(root), output_dir=None, threshold=10.0, mask_threshold=0.5,
             multi_threshold=None, use_tta=False, tta_mode="basic", boundary_refine=False, refine_kernel=5, tile=64,
             dtype="f32", batch=4)
    a.update(kw)
    return argparse.Namespace(**a)


@pytest.mark.parametrize("shape", SHAPES)
def test_calculate_fat_percentage_of_maps_golden(shape):
    m = GOLD[f"map_{shape[0]}x{shape[1]}"]
    got = np.array([TC.calculate_fat_percentage(m, t) for t in MAP_THRESHOLDS])
    assert np.array_equal(got, GOLD[f"map_pct_{shape[0]}x{shape[1]}"])
    ref = TC.fat_counts_ref(m, None, 0.5)
    assert ref.dtype == np.uint64 and ref.shape == (1, 4) and not ref[0, 1:].any()
    assert np.array_equal(TC.fat_counts(m, None, 0.5), ref)


@pytest.mark.parametrize("shape", SHAPES)
def test_ground_truth_percentages_golden(shape):
    """The reference's normalisation (divide by 255.0 only above a maximum of 1.0) as the choice between columns."""
    want = GOLD[f"gt_pct_{shape[0]}x{shape[1]}"]
    stack = np.stack([GOLD[f"gt_{shape[0]}x{shape[1]}_{k}"] for k in KINDS])
    dummy = np.zeros(stack.shape, np.float32)
    for j, t in enumerate(MAP_THRESHOLDS):
        c = TC.fat_counts_ref(None, stack, t)
        assert np.array_equal(c[:, 1], stack.reshape(len(KINDS), -1).max(axis=1))
        assert np.array_equal(TC.gt_count(c) / stack[0].size * 100.0, want[:, j])
        assert np.array_equal(TC.fat_percentages(dummy, stack, t)[1], want[:, j])
        for i in range(len(KINDS)):   # what the reference does itself: convert, normalise, count
            g = stack[i].astype(np.float32)
            g = g / np.float32(255.0) if g.max() > 1.0 else g
            assert TC.calculate_fat_percentage(g, t) == want[i, j]
    # a uint8 mask handed to calculate_fat_percentage is counted as it is (the raw cut only)
    raw = GOLD[f"gt_{shape[0]}x{shape[1]}_0255"]
    assert TC.calculate_fat_percentage(raw, 0.5) == TC.calculate_fat_percentage(raw.astype(np.float32), 0.5)


@pytest.mark.parametrize("thr", [0.0, 0.3, 0.5, 1.0 / 255.0, 0.999, 1.0, float("nan")])
def test_cuts_agree_with_the_restatement_for_every_gray_value(thr):
    cut_raw, cut_scaled = TC.gt_cuts(thr)
    assert 0 <= cut_raw <= 256 and 0 <= cut_scaled <= 256
    g = np.arange(256, dtype=np.uint8).reshape(256, 1, 1)   # 256 one-pixel images
    c = TC.fat_counts_ref(None, g, thr)
    assert np.array_equal(c[:, 1], np.arange(256))
    assert np.array_equal(c[:, 2], (np.arange(256) >= cut_raw).astype(np.uint64))
    assert np.array_equal(c[:, 3], (np.arange(256) >= cut_scaled).astype(np.uint64))
    assert not c[:, 0].any()


def test_cuts_of_the_common_thresholds():
    assert TC.gt_cuts(0.5) == (1, 128)
    assert TC.gt_cuts(1.0 / 255.0) == (1, 2)
    assert TC.gt_cuts(1.0) == (2, 256)
    assert TC.gt_cuts(float("nan")) == (256, 256)


def test_ground_truth_that_is_not_uint8_takes_the_restatement():
    rng = np.random.default_rng(3)
    m = rng.random((2, 9, 11)) > 0.5
    for g in (m, m.astype(np.uint16) * 65535, m.astype(np.float32) * 0.75, m.astype(np.float64) * 1.5):
        c = TC.fat_counts(None, g, 0.5)
        assert np.array_equal(c, TC.fat_counts_ref(None, g, 0.5))
        f = g.astype(np.float32)
        want = [int(((f[i] / 255.0 if f[i].max() > 1.0 else f[i]) > 0.5).sum()) for i in range(2)]
        assert TC.gt_count(c).tolist() == want


def test_classify_tile_golden():
    got = [TC.classify_tile(float(p), float(t)) for p, t in zip(GOLD["classify_pct"], GOLD["classify_thr"])]
    assert got == [str(s) for s in GOLD["classify_out"]]
    assert TC.classify_tile(10.0, 10.0) == "Has Fat"


def test_confusion_matrix_and_metrics_golden():
    cm_keys, metric_keys = [str(k) for k in GOLD["cm_keys"]], [str(k) for k in GOLD["metric_keys"]]
    for k in range(int(GOLD["cm_cases"])):
        pred, true = [str(s) for s in GOLD[f"cm_{k}_pred"]], [str(s) for s in GOLD[f"cm_{k}_true"]]
        cm = TC.calculate_confusion_matrix(pred, true)
        assert list(cm) == cm_keys
        assert np.array_equal(np.array([cm[q] for q in cm_keys]), GOLD[f"cm_{k}_cm"])
        met = TC.calculate_classification_metrics(cm)
        assert list(met) == metric_keys
        assert np.array_equal(np.array([met[q] for q in metric_keys], np.float64), GOLD[f"cm_{k}_metrics"])
    with pytest.raises(AssertionError):
        TC.calculate_confusion_matrix(["Has Fat"], [])


def test_naming_helpers_golden():
    paths = [str(p) for p in GOLD["name_paths"]]
    assert [TC.extract_dataset_name(p) for p in paths] == [str(s) for s in GOLD["name_dataset"]]
    assert [TC.detect_data_source(p) for p in paths] == [str(s) for s in GOLD["name_source"]]
    for combo, suffixes, out in zip(GOLD["dir_combos"], GOLD["dir_suffixes"], GOLD["dir_out"]):
        use_tta, mode, refine, rtype, thr, path = str(combo).split("|")
        a = make_args(path, "/ckpt/run_20250101/best.weights.h5", use_tta=bool(int(use_tta)), tta_mode=mode,
                      boundary_refine=bool(int(refine)), threshold=int(thr) if thr.isdigit() else float(thr))
        if rtype:
            a.refine_type = rtype
        assert ",".join(TC.build_enhancement_suffixes(a)) == str(suffixes)
        assert TC.build_output_directory(a).as_posix() == str(out)


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return write_dataset(tmp_path_factory.mktemp("tilefat"))


@pytest.mark.parametrize("tta", ["none", "basic"])
@pytest.mark.parametrize("mask_threshold", [0.5, 0.3])
def test_evaluate_tiles_golden(dataset, tta, mask_threshold):
    """Per-tile percentages, classes, confusion matrix and metrics of the reference, for three thresholds from ONE
    pass: the second and third threshold find the cache filled and call the predictor zero times."""
    root, weights = dataset
    cm_keys, metric_keys = [str(k) for k in GOLD["cm_keys"]], [str(k) for k in GOLD["metric_keys"]]
    model, cache = FakePredictor(), {}
    args = make_args(root, weights, mask_threshold=mask_threshold, use_tta=tta != "none", tta_mode="basic")
    for n, ct in enumerate(float(t) for t in GOLD["class_thresholds"]):
        before = model.calls
        res = TC.evaluate_tiles(args, ct, model=model, fat_cache=cache)
        if n == 0:
            assert model.calls == 8 * (4 if tta == "basic" else 1)   # 8 paired tiles; the ninth has no mask
        else:
            assert model.calls == before
        key = f"eval_{tta}_{mask_threshold}_{ct}"
        rows = res["per_tile_results"]
        assert list(res) == [str(k) for k in GOLD[key + "_result_keys"]]
        assert res["threshold"] == float(GOLD[key + "_threshold"])
        assert all(list(r) == [str(k) for k in GOLD[key + "_keys"]] for r in rows)
        assert [r["tile_name"] for r in rows] == [str(s) for s in GOLD[key + "_names"]]
        assert np.array_equal(np.array([r["predicted_fat_pct"] for r in rows]), GOLD[key + "_pred_pct"])
        assert np.array_equal(np.array([r["ground_truth_fat_pct"] for r in rows]), GOLD[key + "_gt_pct"])
        assert [r["predicted_class"] for r in rows] == [str(s) for s in GOLD[key + "_pred_class"]]
        assert [r["ground_truth_class"] for r in rows] == [str(s) for s in GOLD[key + "_gt_class"]]
        assert [r["correct"] for r in rows] == GOLD[key + "_correct"].tolist()
        assert np.array_equal(np.array([res["confusion_matrix"][q] for q in cm_keys]), GOLD[key + "_cm"])
        assert np.array_equal(np.array([res["metrics"][q] for q in metric_keys]), GOLD[key + "_metrics"])
    # without a cache every call is a pass of its own, with the same result
    again = TC.evaluate_tiles(args, 10.0, model=model)
    assert model.calls == 2 * 8 * (4 if tta == "basic" else 1)
    assert again["per_tile_results"] == TC.evaluate_tiles(args, 10.0, model=model, fat_cache=cache)["per_tile_results"]


def test_evaluate_tiles_skips_a_tile_of_another_size_and_needs_both_folders(dataset, tmp_path, capsys):
    from PIL import Image
    root, weights = dataset
    other = tmp_path / "val"
    (other / "images").mkdir(parents=True)
    with pytest.raises(FileNotFoundError, match="Masks directory not found"):
        TC.evaluate_tiles(make_args(other, weights), 10.0, model=FakePredictor())
    (other / "masks").mkdir()
    with pytest.raises(FileNotFoundError, match="Images directory not found"):
        TC.evaluate_tiles(make_args(tmp_path / "nothing", weights), 10.0, model=FakePredictor())
    for stem, size in (("a", 64), ("b", 48)):
        Image.fromarray(np.full((size, size), 200, np.uint8)).save(other / "images" / f"{stem}.jpg", format="PNG")
        Image.fromarray(np.ones((size, size), np.uint8)).save(other / "masks" / f"{stem}.tif", format="TIFF")
    res = TC.evaluate_tiles(make_args(other, weights), 10.0, model=FakePredictor())
    assert [r["tile_name"] for r in res["per_tile_results"]] == ["a"]
    assert res["per_tile_results"][0]["ground_truth_fat_pct"] == 100.0
    assert "b.jpg is (48, 48), expected (64, 64), skipping" in capsys.readouterr().out


def test_save_results_files(dataset, tmp_path):
    root, weights = dataset
    args = make_args(root, weights, use_tta=True, tta_mode="basic")
    res = TC.evaluate_tiles(args, 10.0, model=FakePredictor())
    assert any(not r["correct"] for r in res["per_tile_results"]), "the set has misclassified tiles at 10 %"
    out = tmp_path / "out" / "deep"
    TC.save_results(res, out, args)
    with open(out / "per_tile_results.csv", newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["tile_name", "predicted_fat_pct", "ground_truth_fat_pct", "predicted_class",
                       "ground_truth_class", "correct"]
    assert len(rows) == 1 + len(res["per_tile_results"])
    for row, r in zip(rows[1:], res["per_tile_results"]):
        assert row == [r["tile_name"], repr(r["predicted_fat_pct"]), repr(r["ground_truth_fat_pct"]),
                       r["predicted_class"], r["ground_truth_class"], "True" if r["correct"] else "False"]
        assert float(row[1]) == r["predicted_fat_pct"]
    summary = json.loads((out / "summary_metrics.json").read_text())
    assert list(summary) == ["timestamp", "configuration", "confusion_matrix", "metrics", "total_tiles"]
    assert summary["configuration"] == {"weights": str(weights), "data_root": str(root),
                                        "classification_threshold_pct": 10.0, "mask_threshold": 0.5, "use_tta": True,
                                        "tta_mode": "basic", "boundary_refine": False}
    assert summary["confusion_matrix"] == res["confusion_matrix"] and summary["metrics"] == res["metrics"]
    assert summary["total_tiles"] == 8
    text = (out / "misclassified_tiles.txt").read_text().splitlines()
    wrong = [r for r in res["per_tile_results"] if not r["correct"]]
    assert text[0] == f"Misclassified Tiles ({len(wrong)} total)" and text[1] == "=" * 80 and text[2] == ""
    assert text[3:7] == [wrong[0]["tile_name"],
                         f"  Predicted: {wrong[0]['predicted_class']} ({wrong[0]['predicted_fat_pct']:.2f}%)",
                         f"  Actual:    {wrong[0]['ground_truth_class']} ({wrong[0]['ground_truth_fat_pct']:.2f}%)", ""]
    # without TTA the summary names no mode; without a misclassified tile there is no list of them
    args2 = make_args(root, weights)
    res2 = TC.evaluate_tiles(args2, 10.0, model=FakePredictor())
    for r in res2["per_tile_results"]:
        r["correct"] = True
    TC.save_results(res2, tmp_path / "out2", args2)
    assert json.loads((tmp_path / "out2" / "summary_metrics.json").read_text())["configuration"]["tta_mode"] is None
    assert not (tmp_path / "out2" / "misclassified_tiles.txt").exists()


def test_cli_multi_threshold_folder_tree(dataset, capsys):
    """--multi-threshold through main() with a fake model: one folder per threshold under the base folder the
    reference builds, the comparison beside them, all from one pass."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "cli"))
    import tile_classification_evaluation as cli
    root, weights = dataset
    model = FakePredictor()
    rc = cli.main(["--weights", str(weights), "--data-root", str(root), "--multi-threshold", "1,10,50", "--use-tta",
                   "--tta-mode", "minimal", "--tile", "64"], model=model)
    assert rc == 0
    assert model.calls == 8 * 2   # one pass of the two minimal views
    base = Path(weights).parent / "evaluation" / "clean_test_original_tta_minimal"
    for t in ("1.0", "10.0", "50.0"):
        d = base / f"binary_classification_{t}"
        assert (d / "per_tile_results.csv").exists() and (d / "summary_metrics.json").exists()
        cfg = json.loads((d / "summary_metrics.json").read_text())["configuration"]
        assert cfg["classification_threshold_pct"] == float(t)
    with open(base / "threshold_analysis.csv", newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["threshold", "accuracy", "precision", "recall", "f1_score", "specificity"]
    assert [r[0] for r in rows[1:]] == ["1.0", "10.0", "50.0"]
    args = make_args(root, weights, use_tta=True, tta_mode="minimal")
    for row, t in zip(rows[1:], (1.0, 10.0, 50.0)):
        met = TC.evaluate_tiles(args, t, model=FakePredictor())["metrics"]
        assert row[1:] == [repr(met[k]) for k in rows[0][1:]]
    try:
        import matplotlib  # noqa: F401
        has_mpl = True
    except ImportError:
        has_mpl = False
    assert (base / "threshold_analysis.png").exists() == has_mpl
    assert (base / "binary_classification_1.0" / "confusion_matrix.png").exists() == has_mpl
    # defaults of the reference's flags, and a failure is reported as 1
    d = cli.build_parser().parse_args(["--weights", "w", "--data-root", "d"])
    assert (d.output_dir, d.threshold, d.mask_threshold, d.multi_threshold, d.use_tta, d.tta_mode, d.boundary_refine,
            d.refine_kernel) == (None, 10.0, 0.5, None, False, "basic", False, 5)
    assert (d.tile, d.dtype, d.batch) == (1024, "f32", 8)
    assert cli.main(["--weights", str(weights), "--data-root", str(Path(root) / "missing")], model=model) == 1
    assert "Evaluation failed" in capsys.readouterr().out


def test_abi_has_the_fat_count_export():
    hdr = open(os.path.join(ROOT, "include", "adipose_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+adp_fat_counts\s*\(", code)
    assert "adp_fat_counts" in _lib.exported_symbols()
    assert len(_lib._SIGS["adp_fat_counts"]) == 9
    assert hasattr(_lib.lib(), "adp_fat_counts")
    assert int(re.search(r"#define ADP_FAT_BLOCK_PX (\d+)", hdr).group(1)) == TC.FAT_BLOCK_PX
    assert int(re.search(r"#define ADP_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 21
    assert _lib.lib().adp_abi_version() == 21
