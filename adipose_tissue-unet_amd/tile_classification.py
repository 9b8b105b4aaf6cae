"""Tile-level "Has Fat / No Fat" evaluation: the surface of Segmentation/tile_classification_evaluation.py (:80-592)
on the HIP engine, the fourth caller of the predictor seam predict_single(image, mean, std).

Same names, arguments, return values and output files as the reference:
  extract_dataset_name / detect_data_source / build_enhancement_suffixes / build_output_directory   :80-204
  calculate_fat_percentage / classify_tile                                                          :211-240
  calculate_confusion_matrix / calculate_classification_metrics                                     :243-313
  evaluate_tiles                                                                                    :402-530
  save_results                                                                                      :533-592
and run_evaluation, the body of the reference's main() (:652-736) after its argument parsing.

What a tile contributes is four integers (fat_counts). For image i of n_px pixels, with t = float32(mask_threshold):
  column 0  #(pred[i] > t), compared in float32 (a NaN on either side counts nothing)
  column 1  max gt[i]
  column 2  #(float32(gt[i]) > t)            the ground truth as it is          ("raw")
  column 3  #(float32(gt[i]) / 255 > t)      the ground truth in 0 .. 255       ("scaled")
The reference's ground-truth normalisation divides by 255.0 only if the mask's maximum exceeds 1.0, so the host takes
column 3 where column 1 is greater than 1 and column 2 otherwise; a percentage is count / n_px * 100.0 in float64.

MI355X-first differences (same results): the probability maps of a chunk of tiles stay on the device from the batched
forward (predict_views, all TTA views of a tile in one batch) through BoundaryRefiner.refine_device to one
adp_fat_counts call (csrc/tilefat.hip) for the chunk's maps and uint8 masks; 32 bytes a tile come back. For a uint8
ground truth both predicates are monotone in the byte, so the device compares bytes with two integer cuts that the host
computes (gt_cuts) and never divides. The classification threshold is applied to stored percentages: evaluate_tiles
fills a `fat_cache` on its first call and every further threshold runs no forward (the reference runs the whole
inference again for every value of --multi-threshold). fat_counts_ref is the numpy restatement of the same four
integers with the reference's expressions: hosts without a device, duck-typed predictors without predict_views, and
ground truths that are not uint8 (bool, uint16, float TIFFs) take it.

pandas and seaborn are not needed: the CSVs are written with the csv module (floats by repr, booleans as True / False,
the reference's columns; byte parity with pandas is not claimed) and the two figures are drawn with matplotlib alone,
only if it imports (their pixels are pinned nowhere).
"""
from __future__ import annotations

import argparse
import csv
import json
from datetime import datetime
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .evaluation import (BoundaryRefiner, _detect_deep_supervision, load_training_stats, read_image_gray, read_mask,
                         resolve_weights_path, set_deterministic_seeds)
from .predictor import TestTimeAugmentation

FAT_BLOCK_PX = 32768  # include/adipose_hip.h ADP_FAT_BLOCK_PX: the pixels one block counts (the GPU tests' shapes)
HAS_FAT, NO_FAT = "Has Fat", "No Fat"
KNOWN_DATASETS = ("clean_test", "clean_test_50_overlap", "test", "val", "human_test")
RESULT_KEYS = ("tile_name", "predicted_fat_pct", "ground_truth_fat_pct", "predicted_class", "ground_truth_class",
               "correct")
ANALYSIS_KEYS = ("threshold", "accuracy", "precision", "recall", "f1_score", "specificity")


# ------------------------------------------------------------------------------ output folder naming
def extract_dataset_name(data_root: str) -> str:
    """:80-114 — the last path component if it is a known dataset name, else the first known name (in the reference's
    order) that occurs anywhere in the path, else the last component ("unknown" for an empty path)."""
    path = Path(data_root)
    parts = [p for p in path.parts if p]
    last = parts[-1] if parts else "unknown"
    if last in KNOWN_DATASETS:
        return last
    whole = str(path)
    for name in KNOWN_DATASETS:
        if name in whole:
            return name
    return last


def detect_data_source(data_root: str) -> str:
    """:117-132 — 'stain' if the lower-cased path mentions "stain" or "normalized", else 'original'."""
    low = str(data_root).lower()
    return "stain" if ("stain" in low or "normalized" in low) else "original"


def build_enhancement_suffixes(args) -> List[str]:
    """:135-165 — tta_{mode}, then refine_adaptive (refine_{type} for another args.refine_type)."""
    out = []
    if args.use_tta:
        out.append(f"tta_{args.tta_mode}")
    if args.boundary_refine:
        out.append("refine_" + str(getattr(args, "refine_type", "adaptive")))
    return out


def _evaluation_folder(args) -> Path:
    """{checkpoint}/evaluation/{dataset}_{source}[_{enhancements}]"""
    name = f"{extract_dataset_name(args.data_root)}_{detect_data_source(args.data_root)}"
    suffixes = build_enhancement_suffixes(args)
    if suffixes:
        name += "_" + "_".join(suffixes)
    return Path(args.weights).parent / "evaluation" / name


def build_output_directory(args) -> Path:
    """:168-204 — {checkpoint}/evaluation/{dataset}_{source}_{enhancements}/binary_classification_{threshold}"""
    return _evaluation_folder(args) / f"binary_classification_{args.threshold}"


# ------------------------------------------------------------------------------ the four integers
def gt_cuts(mask_threshold: float) -> Tuple[int, int]:
    """(cut_raw, cut_scaled) for a uint8 ground truth: the smallest byte g with float32(g) > t, and the smallest with
    float32(g) / float32(255) > t, t = float32(mask_threshold); 256 where no byte passes (t >= 255 or 1, a NaN).
    Both predicates are monotone in g (float32(g) is exact and the division is correctly rounded, so monotone), hence
    `g >= cut` is the predicate."""
    t = np.float32(mask_threshold)
    g = np.arange(256, dtype=np.uint8).astype(np.float32)
    cuts = []
    for passes in (g > t, g / np.float32(255.0) > t):
        assert not np.any(passes[:-1] & ~passes[1:]), "monotone in the byte"
        cuts.append(int(np.argmax(passes)) if passes.any() else 256)
    return cuts[0], cuts[1]


def _planes(a, name):
    """(N, n_px) view, (H, W) of one image: a 2-D plane is N = 1, a 3-D stack is (N, H, W); a list is stacked."""
    if isinstance(a, (list, tuple)):
        a = torch.stack(list(a)) if isinstance(a[0], torch.Tensor) else np.stack([np.asarray(x) for x in a])
    if not isinstance(a, torch.Tensor):
        a = np.asarray(a)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or a.shape[1] * a.shape[2] < 1:
        raise ValueError(f"{name} must be an (H, W) plane or an (N, H, W) stack of non-empty planes")
    return a


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a


def fat_counts_ref(pred=None, gt=None, mask_threshold: float = 0.5) -> np.ndarray:
    """The (N, 4) uint64 counts of the module docstring in numpy, with the reference's expressions (:222-223 for a map,
    :478-489 for the ground truth) and float32(threshold) written out, so that the comparison's precision does not
    depend on numpy's scalar promotion. For a ground truth that is not uint8 column 1 is ceil(max) (0 for a maximum
    that is not positive), so that `> 1` still says what the reference's `max() > 1.0` says."""
    if pred is None and gt is None:
        raise ValueError("fat_counts_ref: pred and gt must not both be None")
    t = np.float32(mask_threshold)
    p = None if pred is None else np.asarray(_host(_planes(pred, "pred")), np.float32)
    g = None if gt is None else _host(_planes(gt, "gt"))
    if p is not None and g is not None and len(p) != len(g):
        raise ValueError("fat_counts_ref: pred and gt must hold the same number of images")
    out = np.zeros((len(p if p is not None else g), 4), np.uint64)
    for i in range(len(out)):
        if p is not None:
            out[i, 0] = (p[i] > t).astype(np.uint8).sum()
        if g is not None:
            m = g[i].astype(np.float32)
            top = m.max()
            out[i, 1] = int(np.ceil(min(top, np.float32(2.0 ** 62)))) if top > 0 else 0
            out[i, 2] = (m > t).astype(np.uint8).sum()
            out[i, 3] = (m / np.float32(255.0) > t).astype(np.uint8).sum()
    return out


def _is_u8(a):
    return a.dtype == (torch.uint8 if isinstance(a, torch.Tensor) else np.uint8)


def fat_counts(pred=None, gt=None, mask_threshold: float = 0.5) -> np.ndarray:
    """The (N, 4) uint64 counts of the module docstring. Device tensors, and host arrays where a device is present, go
    through adp_fat_counts: one call, and N x 32 bytes come back. Host arrays without a device, and every ground truth
    that is not uint8, take fat_counts_ref."""
    if pred is None and gt is None:
        raise ValueError("fat_counts: pred and gt must not both be None")
    p = None if pred is None else _planes(pred, "pred")
    g = None if gt is None else _planes(gt, "gt")
    on_device = any(isinstance(a, torch.Tensor) and a.is_cuda for a in (p, g))
    if (g is not None and not _is_u8(g)) or not (on_device or torch.cuda.is_available()):
        return fat_counts_ref(p, g, mask_threshold)
    from ._lib import call, ptr, stream_ptr
    dev = next((a.device for a in (p, g) if isinstance(a, torch.Tensor) and a.is_cuda),
               torch.device("cuda", torch.cuda.current_device()))
    if p is not None:
        p = (p if isinstance(p, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(p, np.float32)))
        p = p.to(dev, torch.float32).contiguous()
    if g is not None:
        g = (g if isinstance(g, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(g))).to(dev).contiguous()
    if p is not None and g is not None and (p.shape[0] != g.shape[0] or p[0].numel() != g[0].numel()):
        raise ValueError("fat_counts: pred and gt must hold the same number of images of the same size")
    first = p if p is not None else g
    N, n_px = first.shape[0], first[0].numel()
    cut_raw, cut_scaled = gt_cuts(mask_threshold)
    out = torch.empty((N, 4), dtype=torch.int64, device=dev)   # (the call zeroes it; uint64 read as int64 bits below)
    with torch.cuda.device(dev):
        call("adp_fat_counts", N, n_px, ptr(p), float(np.float32(mask_threshold)), ptr(g), cut_raw, cut_scaled, ptr(out),
             stream_ptr())
    return out.cpu().numpy().view(np.uint64)


def _percent(count, n_px):
    """:223-226 — (fat_pixels / total_pixels) * 100.0 in float64"""
    return np.asarray(count, np.uint64).astype(np.float64) / n_px * 100.0


def gt_count(counts: np.ndarray) -> np.ndarray:
    """The ground truth's column of fat_counts' rows: scaled where the mask's maximum exceeds 1, raw otherwise."""
    return np.where(counts[:, 1] > 1, counts[:, 3], counts[:, 2])


def fat_percentages(pred, gt, mask_threshold: float = 0.5) -> Tuple[np.ndarray, np.ndarray]:
    """(pred_pct, gt_pct), float64 per image: calculate_fat_percentage of every map, and of every ground truth after
    the reference's normalisation. One fat_counts call."""
    n_px = int(np.prod(_planes(pred, "pred").shape[1:]))
    c = fat_counts(pred, gt, mask_threshold)
    return _percent(c[:, 0], n_px), _percent(gt_count(c), n_px)


def calculate_fat_percentage(mask, threshold: float = 0.5) -> float:
    """:211-226 — percentage (0 .. 100) of the pixels of one map with mask > threshold, device or host. A uint8 mask is
    counted as the reference counts an array it has already converted to float32 (the raw cut only: the normalisation
    is the caller's, as in the reference); a host array of another type than float32 / uint8 is compared in its own
    type."""
    if isinstance(mask, torch.Tensor) or np.asarray(mask).dtype in (np.float32, np.uint8):
        m = mask if isinstance(mask, torch.Tensor) else np.asarray(mask)
        m = m.reshape(1, 1, -1)
        if m.dtype in (torch.bool, np.bool_):
            raise TypeError("calculate_fat_percentage: a probability map or a uint8 mask is expected")
        if _is_u8(m):
            return float(_percent(fat_counts(None, m, threshold)[0, 2], m.shape[-1]))
        return float(_percent(fat_counts(m, None, threshold)[0, 0], m.shape[-1]))
    m = np.asarray(mask)
    return float(_percent(np.count_nonzero(m > threshold), m.size))


def classify_tile(fat_percentage: float, classification_threshold: float) -> str:
    """:229-240 — "Has Fat" from the threshold on (>=), else "No Fat"."""
    return HAS_FAT if fat_percentage >= classification_threshold else NO_FAT


def calculate_confusion_matrix(predictions: List[str], ground_truth: List[str]) -> Dict:
    """:243-267 — "Has Fat" is the positive class."""
    if len(predictions) != len(ground_truth):
        raise AssertionError("Mismatch in list lengths")
    pairs = list(zip(predictions, ground_truth))
    n = {(a, b): pairs.count((a, b)) for a in (HAS_FAT, NO_FAT) for b in (HAS_FAT, NO_FAT)}
    return {"true_positive": n[HAS_FAT, HAS_FAT], "true_negative": n[NO_FAT, NO_FAT],
            "false_positive": n[HAS_FAT, NO_FAT], "false_negative": n[NO_FAT, HAS_FAT], "total": len(pairs)}


def calculate_classification_metrics(cm: Dict) -> Dict:
    """:270-313 — every ratio is 0.0 where its denominator is 0."""
    def ratio(a, b):
        return a / b if b > 0 else 0.0
    tp, tn, fp, fn = cm["true_positive"], cm["true_negative"], cm["false_positive"], cm["false_negative"]
    precision, recall, specificity = ratio(tp, tp + fp), ratio(tp, tp + fn), ratio(tn, tn + fp)
    return {"accuracy": ratio(tp + tn, cm["total"]), "precision": precision, "recall": recall, "sensitivity": recall,
            "specificity": specificity, "f1_score": ratio(2 * (precision * recall), precision + recall),
            "npv": ratio(tn, tn + fn), "balanced_accuracy": (recall + specificity) / 2.0}


# ------------------------------------------------------------------------------ evaluation
def find_paired_tiles(data_root) -> List[Tuple[Path, Path]]:
    """:418-453 — images/*.jpg with the masks/*.tif of the same stem, sorted by image path."""
    images_dir, masks_dir = Path(data_root) / "images", Path(data_root) / "masks"
    if not images_dir.exists():
        raise FileNotFoundError(f"Images directory not found: {images_dir}")
    if not masks_dir.exists():
        raise FileNotFoundError(f"Masks directory not found: {masks_dir}")
    masks = {p.stem: p for p in masks_dir.glob("*.tif")}
    return [(p, masks[p.stem]) for p in sorted(images_dir.glob("*.jpg")) if p.stem in masks]


def build_model(args):
    """The predictor of cli/full_evaluation_enhanced.py for args.weights (--tile, --dtype, --batch of this build)."""
    from .predictor import AdiposeUNet
    ds = _detect_deep_supervision(Path(args.weights).parent)
    model = AdiposeUNet(tile_size=getattr(args, "tile", 1024), dtype=getattr(args, "dtype", "f32"),
                        max_batch=getattr(args, "batch", 8))
    model.build_model(init_nb=44, dropout_rate=0.3, use_deep_supervision=ds)
    model.load_weights(args.weights)
    return model


def _tile_percentages(args, model) -> Dict:
    """One inference pass over the paired tiles: {"tile_names", "pred_pct", "gt_pct"} (what fat_cache holds)."""
    paired = find_paired_tiles(args.data_root)
    print(f"Found {len(paired)} paired tiles")
    train_mean, train_std = load_training_stats(str(Path(args.weights).parent))
    if model is None:
        model = build_model(args)
    refiner = BoundaryRefiner(kernel_size=args.refine_kernel, bilateral_d=5, bilateral_sigma_color=50,
                              bilateral_sigma_space=50) if args.boundary_refine else None
    tta = TestTimeAugmentation(mode=args.tta_mode) if args.use_tta else None
    size = getattr(args, "tile", None) or getattr(model, "tile_size", None)
    thr = args.mask_threshold
    names, pred_pct, gt_pct = [], [], []
    loaded = []
    for img_path, mask_path in paired:
        tile = read_image_gray(str(img_path))
        if size is not None and tile.shape[:2] != (size, size):
            print(f"⚠️  Warning: {img_path.name} is {tile.shape}, expected ({size}, {size}), skipping")
            continue
        loaded.append((img_path.stem, tile, mask_path))
    if not hasattr(model, "predict_views"):   # any object with predict_single: the reference's loop, on the host
        for stem, tile, mask_path in loaded:
            pred = tta.predict_with_tta(model, tile, train_mean, train_std) if tta is not None \
                else model.predict_single(tile, train_mean, train_std)
            if refiner is not None:
                pred = refiner.refine(pred, tile)
            pred, mask = np.asarray(pred, np.float32), read_mask(str(mask_path))
            names.append(stem)
            pred_pct.append(_percent(fat_counts_ref(pred, None, thr)[0, 0], pred.size))
            gt_pct.append(_percent(gt_count(fat_counts_ref(None, mask, thr))[0], mask.size))
    else:
        views = tta.views if tta is not None else [0]
        per = max(1, int(getattr(args, "batch", 8) or 8))
        for k0 in range(0, len(loaded), per):
            chunk = loaded[k0:k0 + per]
            maps = model.predict_views([t for _, t, _ in chunk], train_mean, train_std, views)   # (n, S, S) on the device
            if refiner is not None:
                maps = torch.stack([refiner.refine_device(m) for m in maps])
            masks = [read_mask(str(m)) for _, _, m in chunk]
            n_px = maps[0].numel()
            if all(m.dtype == np.uint8 and m.shape == tuple(maps.shape[1:]) for m in masks):
                c = fat_counts(maps, torch.from_numpy(np.stack(masks)).to(maps.device), thr)   # the chunk in one call
                gt_pct.extend(_percent(gt_count(c), n_px))
            else:   # masks of another type or size: the maps in one call, every mask on its own
                c = fat_counts(maps, None, thr)
                gt_pct.extend(_percent(gt_count(fat_counts(None, m, thr))[0], m.size) for m in masks)
            pred_pct.extend(_percent(c[:, 0], n_px))
            names.extend(stem for stem, _, _ in chunk)
    return {"tile_names": names, "pred_pct": np.asarray(pred_pct, np.float64), "gt_pct": np.asarray(gt_pct, np.float64)}


def evaluate_tiles(args, threshold_pct: float, model=None, fat_cache: Optional[Dict] = None) -> Dict:
    """:402-530 — the binary classification of every paired tile of args.data_root at one threshold (percent):
    {"threshold", "confusion_matrix", "metrics", "per_tile_results"}. `model` overrides building AdiposeUNet from
    args.weights and may be any object with predict_single (with predict_views the tiles run in chunks of args.batch on
    the device and no probability map leaves it). `fat_cache`: a dict that the first call fills with the per-tile
    percentages (they do not depend on threshold_pct); a call that finds it filled runs no forward."""
    print(f"\n{'=' * 80}\nEVALUATING WITH {threshold_pct:.1f}% THRESHOLD\n{'=' * 80}")
    if fat_cache is not None and "pred_pct" in fat_cache:
        fat = fat_cache
    else:
        fat = _tile_percentages(args, model)
        if fat_cache is not None:
            fat_cache.update(fat)
    results, predictions, truths = [], [], []
    for name, p, g in zip(fat["tile_names"], fat["pred_pct"], fat["gt_pct"]):
        pc, gc = classify_tile(p, threshold_pct), classify_tile(g, threshold_pct)
        predictions.append(pc)
        truths.append(gc)
        results.append(dict(zip(RESULT_KEYS, (name, float(p), float(g), pc, gc, pc == gc))))
    cm = calculate_confusion_matrix(predictions, truths)
    metrics = calculate_classification_metrics(cm)
    print("\nConfusion Matrix:")
    print(f"  True Positives (Has Fat → Has Fat):   {cm['true_positive']}")
    print(f"  True Negatives (No Fat → No Fat):     {cm['true_negative']}")
    print(f"  False Positives (No Fat → Has Fat):   {cm['false_positive']}")
    print(f"  False Negatives (Has Fat → No Fat):   {cm['false_negative']}")
    print("\nMetrics:")
    for label, key in (("Accuracy:   ", "accuracy"), ("Precision:  ", "precision"), ("Recall:     ", "recall"),
                       ("F1-Score:   ", "f1_score"), ("Specificity:", "specificity")):
        print(f"  {label} {metrics[key]:.1%}")
    return {"threshold": threshold_pct, "confusion_matrix": cm, "metrics": metrics, "per_tile_results": results}


# ------------------------------------------------------------------------------ output files
def _pyplot():
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        return plt
    except Exception:  # noqa: BLE001 (absent or unusable: the figures are optional)
        return None


def plot_confusion_matrix(cm: Dict, output_path, title: str = "Confusion Matrix") -> bool:
    """:320-362 without seaborn: rows actual, columns predicted, counts in the cells. False if matplotlib is absent."""
    plt = _pyplot()
    if plt is None:
        return False
    m = np.array([[cm["true_positive"], cm["false_negative"]], [cm["false_positive"], cm["true_negative"]]])
    fig, ax = plt.subplots(figsize=(8, 6))
    im = ax.imshow(m, cmap="Blues")
    fig.colorbar(im, ax=ax, label="Count")
    ax.set_xticks([0, 1], labels=["Predicted: Has Fat", "Predicted: No Fat"])
    ax.set_yticks([0, 1], labels=["Actual: Has Fat", "Actual: No Fat"])
    for (y, x), v in np.ndenumerate(m):
        ax.text(x, y, str(int(v)), ha="center", va="center", color="white" if v > m.max() / 2 else "black")
    ax.set_title(title, fontsize=14, fontweight="bold", pad=20)
    total = cm["total"]
    acc = (cm["true_positive"] + cm["true_negative"]) / total if total else 0.0
    fig.text(0.5, 0.02, f"Total Tiles: {total}\nAccuracy: {acc:.1%}\nTP: {cm['true_positive']}  FN: {cm['false_negative']}\n"
                        f"FP: {cm['false_positive']}  TN: {cm['true_negative']}", ha="center", fontsize=10)
    fig.savefig(output_path, dpi=150, bbox_inches="tight")
    plt.close(fig)
    return True


def plot_threshold_analysis(results: List[Dict], output_path) -> bool:
    """:365-395 — accuracy, precision, recall and F1 over the thresholds. False if matplotlib is absent."""
    plt = _pyplot()
    if plt is None:
        return False
    x = [r["threshold"] for r in results]
    fig, ax = plt.subplots(figsize=(10, 6))
    for key, label, mark in (("accuracy", "Accuracy", "o-"), ("precision", "Precision", "s-"), ("recall", "Recall", "^-"),
                             ("f1_score", "F1-Score", "d-")):
        ax.plot(x, [r["metrics"][key] for r in results], mark, label=label, linewidth=2, markersize=8)
    ax.set_xlabel("Fat Percentage Threshold (%)")
    ax.set_ylabel("Score")
    ax.set_title("Classification Metrics vs Threshold")
    ax.legend(loc="best")
    ax.grid(True, alpha=0.3)
    ax.set_ylim([0, 1.05])
    fig.savefig(output_path, dpi=150, bbox_inches="tight")
    plt.close(fig)
    return True


def _cell(v):
    return repr(float(v)) if isinstance(v, (float, np.floating)) else str(v)


def _write_csv(path, keys, rows):
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(keys)
        w.writerows([_cell(r[k]) for k in keys] for r in rows)


def save_results(results: Dict, output_dir, args) -> None:
    """:533-592 — per_tile_results.csv, summary_metrics.json, confusion_matrix.png (if matplotlib imports) and, if a
    tile is misclassified, misclassified_tiles.txt."""
    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    _write_csv(output_dir / "per_tile_results.csv", RESULT_KEYS, results["per_tile_results"])
    print(f"\n✓ Per-tile results saved: {output_dir / 'per_tile_results.csv'}")
    summary = {
        "timestamp": datetime.now().isoformat(),
        "configuration": {"weights": args.weights, "data_root": args.data_root,
                          "classification_threshold_pct": results["threshold"], "mask_threshold": args.mask_threshold,
                          "use_tta": args.use_tta, "tta_mode": args.tta_mode if args.use_tta else None,
                          "boundary_refine": args.boundary_refine},
        "confusion_matrix": results["confusion_matrix"],
        "metrics": results["metrics"],
        "total_tiles": results["confusion_matrix"]["total"],
    }
    with open(output_dir / "summary_metrics.json", "w") as f:
        json.dump(summary, f, indent=2)
    print(f"✓ Summary metrics saved: {output_dir / 'summary_metrics.json'}")
    png = output_dir / "confusion_matrix.png"
    if plot_confusion_matrix(results["confusion_matrix"], png,
                             title=f"Confusion Matrix ({results['threshold']:.1f}% Threshold)"):
        print(f"✓ Confusion matrix saved: {png}")
    else:
        print("  (matplotlib is not installed: confusion_matrix.png is not written)")
    wrong = [r for r in results["per_tile_results"] if not r["correct"]]
    if wrong:
        with open(output_dir / "misclassified_tiles.txt", "w") as f:
            f.write(f"Misclassified Tiles ({len(wrong)} total)\n" + "=" * 80 + "\n\n")
            for r in wrong:
                f.write(f"{r['tile_name']}\n"
                        f"  Predicted: {r['predicted_class']} ({r['predicted_fat_pct']:.2f}%)\n"
                        f"  Actual:    {r['ground_truth_class']} ({r['ground_truth_fat_pct']:.2f}%)\n\n")
        print(f"✓ Misclassified tiles saved: {output_dir / 'misclassified_tiles.txt'}")


def run_evaluation(args, model=None) -> int:
    """The reference's main() (:649-736) after parse_args: seeds, the output folder, one threshold or the
    --multi-threshold analysis (one inference pass for all of them), 0 or 1."""
    import traceback
    set_deterministic_seeds(1337)
    if args.output_dir is None:
        args.output_dir = str(build_output_directory(args))
        print(f"\n📁 Auto-generated output directory:\n   {args.output_dir}")
    print(f"\n{'=' * 80}\nTILE-LEVEL BINARY CLASSIFICATION EVALUATION\n{'=' * 80}")
    print(f"Weights: {args.weights}\nData: {args.data_root}\nOutput: {args.output_dir}")
    try:
        if args.multi_threshold:
            thresholds = [float(t) for t in args.multi_threshold.split(",")]
            print(f"\nRunning threshold analysis: {thresholds}")
            base = _evaluation_folder(args)
            cache, every = {}, []
            for t in thresholds:
                t_args = argparse.Namespace(**vars(args))
                t_args.threshold = t
                res = evaluate_tiles(t_args, t, model=model, fat_cache=cache)
                every.append(res)
                save_results(res, base / f"binary_classification_{t}", t_args)
            base.mkdir(parents=True, exist_ok=True)
            _write_csv(base / "threshold_analysis.csv", ANALYSIS_KEYS,
                       [{"threshold": r["threshold"], **{k: r["metrics"][k] for k in ANALYSIS_KEYS[1:]}} for r in every])
            print(f"\n✓ Threshold analysis saved: {base / 'threshold_analysis.csv'}")
            if plot_threshold_analysis(every, base / "threshold_analysis.png"):
                print(f"✓ Threshold plot saved: {base / 'threshold_analysis.png'}")
            else:
                print("  (matplotlib is not installed: threshold_analysis.png is not written)")
        else:
            save_results(evaluate_tiles(args, args.threshold, model=model), Path(args.output_dir), args)
        print(f"\n✅ Evaluation complete!\n   Output: {args.output_dir}")
        return 0
    except Exception as e:  # noqa: BLE001 (the reference prints the failure and returns 1, :732-736)
        print(f"\n❌ Evaluation failed: {e}")
        traceback.print_exc()
        return 1
