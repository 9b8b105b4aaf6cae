"""Golden vectors for the tile-level "Has Fat / No Fat" evaluation (Segmentation/tile_classification_evaluation.py),
generated HERE from the reference's own functions. The module imports cv2 / tifffile / tensorflow / seaborn at load
time; they are satisfied by make_golden's inert stubs and, for the two reads evaluate_tiles makes, by a small in-memory
file table:
  cv2.imread(path, IMREAD_GRAYSCALE) -> the tile's uint8 gray plane (the build reads tiles with PIL, so the golden
  pins everything after decoding); tifffile.imread(path) -> the mask array.
Model: make_golden.fake_predictor (deterministic, asymmetric) behind the reference's AdiposeUNet name; the training
statistics are fixed (120, 40). The ground truths' percentages come out of the reference's evaluate_tiles itself, so
its normalisation lines are run, not restated. Data only is written (tests/golden/tile_classification.npz); no
reference source is stored. Usage:
    python tests/golden/make_tile_classification_golden.py [/root/reference]
"""
import contextlib
import io
import os
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
MEAN, STD = 120.0, 40.0
MAP_THRESHOLDS = [0.5, 0.3, 0.0, 1.0]
SHAPES = [(17, 19), (64, 64)]
GT_KINDS = ["01", "0255", "zero", "01two", "random"]
CLASS_THRESHOLDS = [1.0, 10.0, 50.0]
MASK_THRESHOLDS = [0.5, 0.3]


def planted_map(rng, shape):
    """Seeded probabilities with every threshold and its two float32 neighbours planted."""
    m = rng.random(shape).astype(np.float32)
    flat = m.reshape(-1)
    spots = rng.choice(flat.size, size=3 * len(MAP_THRESHOLDS) * 3, replace=False)
    k = 0
    for t in MAP_THRESHOLDS:
        t32 = np.float32(t)
        for v in (t32, np.nextafter(t32, np.float32(-np.inf)), np.nextafter(t32, np.float32(np.inf))):
            for _ in range(3):
                flat[spots[k]] = v
                k += 1
    return m


def gt_mask(rng, kind, shape, density=0.4):
    if kind == "zero":
        return np.zeros(shape, np.uint8)
    if kind == "random":
        return rng.integers(0, 256, size=shape).astype(np.uint8)
    m = (rng.random(shape) < density).astype(np.uint8)
    if kind == "0255":
        m *= 255
    if kind == "01two":
        m.reshape(-1)[int(rng.integers(0, m.size))] = 2
    return m


def gray_tile(rng, shape, level):
    return np.clip(level + rng.normal(0, 30, size=shape), 0, 255).astype(np.uint8)


def args_for(root, ckpt, **kw):
    a = dict(weights=str(Path(ckpt) / "best.weights.h5"), data_root=str(root), output_dir=None, threshold=10.0,
             mask_threshold=0.5, multi_threshold=None, use_tta=False, tta_mode="basic", boundary_refine=False,
             refine_kernel=5)
    a.update(kw)
    return types.SimpleNamespace(**a)


def main():
    make_golden.REF = REF
    make_golden.load_reference()
    import tile_classification_evaluation as tc  # noqa: E402
    rng = np.random.default_rng(4711)
    files, masks = {}, {}

    class Model:
        def __init__(self):
            self._p = make_golden.fake_predictor()

        def build_model(self, *a, **k):
            return None

        def load_weights(self, *a, **k):
            return None

        def predict_single(self, image, mean, std):
            return self._p.predict_single(image, mean, std)

    tc.AdiposeUNet = Model
    tc.load_training_stats = lambda d: (MEAN, STD)
    tc.cv2 = types.SimpleNamespace(IMREAD_GRAYSCALE=0, imread=lambda p, flag: files[p])
    tc.tiff = types.SimpleNamespace(imread=lambda p: masks[p])
    tc.tqdm = lambda it, **k: it
    quiet = contextlib.redirect_stdout(io.StringIO())
    out = {"map_thresholds": np.array(MAP_THRESHOLDS), "gt_kinds": np.array(GT_KINDS),
           "class_thresholds": np.array(CLASS_THRESHOLDS), "mask_thresholds": np.array(MASK_THRESHOLDS),
           "mean_std": np.array([MEAN, STD])}

    # calculate_fat_percentage of probability maps
    for h, w in SHAPES:
        m = planted_map(rng, (h, w))
        out[f"map_{h}x{w}"] = m
        out[f"map_pct_{h}x{w}"] = np.array([tc.calculate_fat_percentage(m, t) for t in MAP_THRESHOLDS], np.float64)

    # classify_tile at and around the threshold
    pcts, thrs = [], []
    for t in (0.0, 1.0, 10.0, 50.0, 100.0):
        for p in (np.nextafter(t, -np.inf), t, np.nextafter(t, np.inf), 0.0, 100.0):
            pcts.append(p)
            thrs.append(t)
    out["classify_pct"], out["classify_thr"] = np.array(pcts), np.array(thrs)
    out["classify_out"] = np.array([tc.classify_tile(p, t) for p, t in zip(pcts, thrs)])

    # confusion matrices and metrics, the all-one-class cases included
    labels = np.array(["Has Fat", "No Fat"])
    cases = [(labels[rng.integers(0, 2, 40)], labels[rng.integers(0, 2, 40)]),
             (labels[rng.integers(0, 2, 7)], labels[rng.integers(0, 2, 7)]),
             (labels[np.zeros(9, int)], labels[np.zeros(9, int)]), (labels[np.ones(9, int)], labels[np.ones(9, int)]),
             (labels[np.zeros(5, int)], labels[np.ones(5, int)]), (labels[np.ones(5, int)], labels[np.zeros(5, int)]),
             (labels[np.zeros(6, int)], labels[rng.integers(0, 2, 6)]), (labels[rng.integers(0, 2, 6)], labels[np.ones(6, int)]),
             (labels[:0], labels[:0])]
    cm_keys = metric_keys = None
    for k, (pred, true) in enumerate(cases):
        cm = tc.calculate_confusion_matrix(list(pred), list(true))
        met = tc.calculate_classification_metrics(cm)
        cm_keys, metric_keys = list(cm), list(met)
        out[f"cm_{k}_pred"], out[f"cm_{k}_true"] = np.array(pred, dtype="U7"), np.array(true, dtype="U7")
        out[f"cm_{k}_cm"] = np.array([cm[q] for q in cm_keys], np.int64)
        out[f"cm_{k}_metrics"] = np.array([met[q] for q in metric_keys], np.float64)
    out["cm_cases"], out["cm_keys"], out["metric_keys"] = np.array(len(cases)), np.array(cm_keys), np.array(metric_keys)

    # naming helpers
    paths = ["/path/to/clean_test", "/path/to/clean_test_50_overlap", "/path/to/stain_normalized/clean_test",
             "/data/Stain_Normalized/val", "/data/NORMALIZED/foo", "/x/human_test", "/x/mytest_set", "/a/b/custom",
             "/a/validation/tiles", "relative/clean_test_50_overlap/", "/x/Stain/human_test_v2", ""]
    out["name_paths"] = np.array(paths)
    out["name_dataset"] = np.array([tc.extract_dataset_name(p) for p in paths])
    out["name_source"] = np.array([tc.detect_data_source(p) for p in paths])
    combos, suffixes, dirs = [], [], []
    for use_tta, mode, refine, rtype, thr in [(False, "basic", False, None, 10.0), (True, "basic", False, None, 10.0),
                                              (True, "full", True, None, 0.1), (False, "minimal", True, None, 25.0),
                                              (True, "minimal", True, "fast", 5), (False, "basic", True, "adaptive", 1.5)]:
        for p in paths[:5]:
            a = args_for(p, "/ckpt/run_20250101", use_tta=use_tta, tta_mode=mode, boundary_refine=refine, threshold=thr)
            if rtype is not None:
                a.refine_type = rtype
            combos.append(f"{int(use_tta)}|{mode}|{int(refine)}|{rtype or ''}|{thr!r}|{p}")
            suffixes.append(",".join(tc.build_enhancement_suffixes(a)))
            dirs.append(tc.build_output_directory(a).as_posix())
    out["dir_combos"], out["dir_suffixes"], out["dir_out"] = np.array(combos), np.array(suffixes), np.array(dirs)

    def run(root, thr_pct, **kw):
        with quiet:
            return tc.evaluate_tiles(args_for(root, Path(root).parent / "ckpt", **kw), thr_pct)

    with tempfile.TemporaryDirectory() as td:
        # ground truths after the reference's normalisation lines: one tile per mask kind, both shapes
        for h, w in SHAPES:
            root = Path(td) / f"gt_{h}x{w}"
            (root / "images").mkdir(parents=True)
            (root / "masks").mkdir()
            for k, kind in enumerate(GT_KINDS):
                stem = f"k{k}_{kind}"
                tile, m = gray_tile(rng, (h, w), 128), gt_mask(rng, kind, (h, w))
                files[str(root / "images" / f"{stem}.jpg")] = tile
                masks[str(root / "masks" / f"{stem}.tif")] = m
                (root / "images" / f"{stem}.jpg").write_bytes(b"")
                (root / "masks" / f"{stem}.tif").write_bytes(b"")
                out[f"gt_{h}x{w}_{kind}"] = m
            pct = np.zeros((len(GT_KINDS), len(MAP_THRESHOLDS)), np.float64)
            for j, t in enumerate(MAP_THRESHOLDS):
                res = run(root, 10.0, mask_threshold=t)
                assert [r["tile_name"] for r in res["per_tile_results"]] == [f"k{k}_{q}" for k, q in enumerate(GT_KINDS)]
                pct[:, j] = [r["ground_truth_fat_pct"] for r in res["per_tile_results"]]
            out[f"gt_pct_{h}x{w}"] = pct

        # evaluate_tiles on a 9-tile 64 x 64 set: every mask kind, both classes, one tile without a mask
        root = Path(td) / "clean_test"
        (root / "images").mkdir(parents=True)
        (root / "masks").mkdir()
        tiles = [("t0_01", 60, "01", 0.004), ("t1_01", 200, "01", 0.3), ("t2_0255", 150, "0255", 0.07),
                 ("t3_0255", 90, "0255", 0.6), ("t4_zero", 230, "zero", 0.0), ("t5_01two", 120, "01two", 0.12),
                 ("t6_random", 30, "random", 0.0), ("t7_nomask", 128, None, 0.0), ("t8_01two", 250, "01two", 0.005)]
        for stem, level, kind, density in tiles:
            tile = gray_tile(rng, (64, 64), level)
            files[str(root / "images" / f"{stem}.jpg")] = tile
            (root / "images" / f"{stem}.jpg").write_bytes(b"")
            out[f"eval_tile_{stem}"] = tile
            if kind is not None:
                m = gt_mask(rng, kind, (64, 64), density)
                masks[str(root / "masks" / f"{stem}.tif")] = m
                (root / "masks" / f"{stem}.tif").write_bytes(b"")
                out[f"eval_mask_{stem}"] = m
        out["eval_stems"] = np.array([t[0] for t in tiles])
        for tta in (None, "basic"):
            for mt in MASK_THRESHOLDS:
                for ct in CLASS_THRESHOLDS:
                    res = run(root, ct, mask_threshold=mt, use_tta=tta is not None, tta_mode=tta or "basic")
                    key = f"eval_{tta or 'none'}_{mt}_{ct}"
                    rows = res["per_tile_results"]
                    out[key + "_keys"] = np.array(list(rows[0]))
                    out[key + "_names"] = np.array([r["tile_name"] for r in rows])
                    out[key + "_pred_pct"] = np.array([r["predicted_fat_pct"] for r in rows], np.float64)
                    out[key + "_gt_pct"] = np.array([r["ground_truth_fat_pct"] for r in rows], np.float64)
                    out[key + "_pred_class"] = np.array([r["predicted_class"] for r in rows])
                    out[key + "_gt_class"] = np.array([r["ground_truth_class"] for r in rows])
                    out[key + "_correct"] = np.array([bool(r["correct"]) for r in rows])
                    out[key + "_threshold"] = np.array(res["threshold"])
                    out[key + "_cm"] = np.array([res["confusion_matrix"][q] for q in cm_keys], np.int64)
                    out[key + "_metrics"] = np.array([res["metrics"][q] for q in metric_keys], np.float64)
                    out[key + "_result_keys"] = np.array(list(res))
    np.savez_compressed(os.path.join(HERE, "tile_classification.npz"), **out)
    size = os.path.getsize(os.path.join(HERE, "tile_classification.npz"))
    print("wrote", os.path.join(HERE, "tile_classification.npz"), len(out), "arrays,", size, "bytes")


if __name__ == "__main__":
    main()
