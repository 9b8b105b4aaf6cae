#!/usr/bin/env python3
"""Drop-in CLI for Segmentation/segmentation_inference.py (flags and defaults of :325-348, flow of
:307-488) on the HIP engine.

Same behaviour as the reference: weights from a file or a checkpoint directory (find_weights_file
:252-285, genuine `.weights.h5` first, then an earlier build's `.weights.safetensors`), z-score stats from `normalization_stats.json` next to the
weights (defaults 0/1 with a warning, :232-249), images of the wrong size are skipped with a warning
(:441-444), `masks/{stem}_mask.tif` (uint8 0/1), optional `probabilities/{stem}_prob.tif` (uint8
prob*255) and `overlays/{stem}_overlay.png`; returns 0/1. All TTA views of a tile run as one batched
forward on the GPU. Extra flags of this build: --tile (the reference hard-codes 1024), --dtype
(f32 = the reference's numerics, bf16 = throughput), --batch (tiles x views per forward), and
--stain-reference IMAGE | --stain-metadata JSON: the tiles are raw RGB and are Reinhard stain-normalised on the GPU
(src/utils/stain_normalization.py, which the reference applies when it builds its datasets) before the network.
--tile-qc: the tiles are raw RGB and are sorted into empty / blurry / tissue on the GPU first (the reference's
classify_tiles_batch, build_dataset.py:1253-1284; --white-threshold, --white-ratio-limit, --blurry-threshold are its
defaults). Empty tiles (with --skip-blurry also blurry ones) get an all-zero mask without a forward; `tile_qc.csv` in
the output directory lists every tile's measurements and class. The files of the other tiles are what they are without
the flag.
--enhance-contrast: every tile's gray plane goes through CLAHE on the GPU before the network (contrast.py;
preprocess_small_MS_SIMs.py's flag, with its --clahe-tile-size 16 and --clahe-clip-limit 3.0). The run's header names
the enhancement only when it is set.
--illumination-method rolling-ball | tophat (--rolling-ball-radius 100, --tophat-kernel 301) and --banding-method
morphological (--morph-width 1, --morph-height 512): preprocess_small_MS_SIMs.py's background corrections by gray-scale
morphology (illumination.py), on every tile's gray plane on the GPU, banding removal first, before --enhance-contrast.
Applied per tile, a correction differs from that of the whole slide within a footprint radius of the tile's edges, and
its background mean is the tile's own. Sizes are checked against the kernel's limit before a model is loaded.
--banding-method column (--column-preserve-global) and --normalization-method percentile | zscore (--percentile-low 1,
--percentile-high 99): preprocess_small_MS_SIMs.py's statistical steps (normalization.py), on every tile's gray plane on
the GPU in the script's order: banding removal, normalisation, illumination correction, --enhance-contrast. The
statistics are the tile's own. The percentiles are checked before a model is loaded.
--sharpen (--sharpen-sigma 1.0, --sharpen-amount 0.5): preprocess_small_MS_SIMs.py's last step, an unsharp mask
(sharpen.py), on every tile's gray plane on the GPU after --enhance-contrast; the border is the tile's own. The sigma is
checked against the kernel's blur radius limit before a model is loaded.
"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COLORS = {"cyan": (0, 255, 255), "yellow": (255, 255, 0), "magenta": (255, 0, 255), "green": (0, 255, 0),
          "red": (255, 0, 0)}
IMAGE_EXTS = {".jpg", ".jpeg", ".png", ".tif", ".tiff"}


def load_normalization_stats(checkpoint_dir):
    """segmentation_inference.py:232-249"""
    p = Path(checkpoint_dir) / "normalization_stats.json"
    if not p.exists():
        print(f"⚠️  Warning: {p} not found, using default normalization")
        return 0.0, 1.0
    with open(p) as f:
        st = json.load(f)
    mean, std = float(st["mean"]), float(st["std"])
    print(f"✓ Loaded normalization stats: mean={mean:.4f}, std={std:.4f}")
    return mean, std


def create_overlay_visualization(image, mask, color=(0, 255, 255)):
    """segmentation_inference.py:288-304: 0.6*image + 0.4*(image with mask pixels painted), rounded as
    cv2.addWeighted does (saturate_cast of the rounded sum)."""
    import numpy as np

    img = np.asarray(image)
    rgb = np.repeat(img.astype(np.uint8)[..., None], 3, axis=-1) if img.ndim == 2 else img.astype(np.uint8)
    over = rgb.copy()
    over[np.asarray(mask) > 0] = color
    out = rgb.astype(np.float64) * 0.6 + over.astype(np.float64) * 0.4
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def build_parser():
    p = argparse.ArgumentParser(description="Run segmentation inference on a folder of images (MI355X HIP engine)")
    p.add_argument("--images-dir", type=str, required=True, help="Directory containing input images")
    p.add_argument("--output-dir", type=str, required=True, help="Directory to save predictions")
    p.add_argument("--weights", type=str, required=True, help="Path to model weights file or checkpoint directory")
    p.add_argument("--threshold", type=float, default=0.5, help="Binarization threshold (0-1, default: 0.5)")
    p.add_argument("--use-tta", action="store_true", default=False, help="Use Test Time Augmentation")
    p.add_argument("--tta-mode", type=str, default="basic", choices=["minimal", "basic", "full"])
    p.add_argument("--save-overlays", action="store_true", default=False)
    p.add_argument("--overlay-color", type=str, default="cyan", choices=list(COLORS))
    p.add_argument("--save-probability", action="store_true", default=False)
    # this build
    p.add_argument("--tile", type=int, default=1024, help="tile size the network is built for (reference: 1024)")
    p.add_argument("--dtype", type=str, default="f32", choices=["f32", "bf16"])
    p.add_argument("--batch", type=int, default=8, help="tiles x TTA views per batched forward")
    # Reinhard stain normalisation of raw RGB tiles on the GPU (the reference normalises when it builds its datasets)
    g = p.add_mutually_exclusive_group()
    g.add_argument("--stain-reference", type=str, default=None, metavar="PATH",
                   help="reference RGB image: tiles are read as RGB and stain-normalised towards it")
    g.add_argument("--stain-metadata", type=str, default=None, metavar="PATH",
                   help="the reference selector's JSON (selected_reference.path names the reference image)")
    # tile quality control on the GPU (the reference sorts tiles when it builds its datasets; only tissue is trained on)
    q = p.add_argument_group("tile quality control")
    q.add_argument("--tile-qc", action="store_true", default=False,
                   help="tiles are read as RGB and classified empty / blurry / tissue; skipped tiles get a zero mask")
    q.add_argument("--white-threshold", type=int, default=235, help="a pixel is white when R, G and B reach this")
    q.add_argument("--white-ratio-limit", type=float, default=0.70, help="empty: more than this share of white pixels")
    q.add_argument("--blurry-threshold", type=float, default=7.5, help="blurry: variance of the Laplacian below this")
    q.add_argument("--skip-blurry", action="store_true", default=False,
                   help="skip blurry tiles too (default: only empty ones, as the reference keeps blurry tiles)")
    e = p.add_argument_group("contrast enhancement (on the device)")
    e.add_argument("--enhance-contrast", action="store_true", default=False,
                   help="CLAHE on every tile's gray plane before the network (preprocess_small_MS_SIMs.py "
                        "--enhance-contrast)")
    e.add_argument("--clahe-tile-size", type=int, default=16, help="CLAHE grid: this many tiles both ways (1..64)")
    e.add_argument("--clahe-clip-limit", type=float, default=3.0, help="CLAHE clip limit")
    b = p.add_argument_group("background correction by gray-scale morphology (on the device)")
    b.add_argument("--illumination-method", type=str, default="none", choices=["none", "rolling-ball", "tophat"],
                   help="illumination correction of every tile's gray plane (preprocess_small_MS_SIMs.py's methods by "
                        "morphology)")
    b.add_argument("--rolling-ball-radius", type=int, default=100, help="radius of the rolling ball's disc (0..256)")
    b.add_argument("--tophat-kernel", type=int, default=301, help="size of the top-hat's ellipse (even: the next odd; 1..513)")
    b.add_argument("--banding-method", type=str, default="none", choices=["none", "morphological", "column"],
                   help="banding removal before the illumination method (column: every column to the image's mean and "
                        "deviation)")
    b.add_argument("--morph-width", type=int, default=1, help="width of the banding opening's rectangle (1..513)")
    b.add_argument("--morph-height", type=int, default=512, help="height of the banding opening's rectangle (1..513)")
    b.add_argument("--column-preserve-global", action="store_true", default=True,
                   help="--banding-method column: keep the image's mean and deviation (the default, as in "
                        "preprocess_small_MS_SIMs.py)")
    n = p.add_argument_group("normalisation of the gray plane (on the device)")
    n.add_argument("--normalization-method", type=str, default="none", choices=["none", "percentile", "zscore"],
                   help="after banding removal, before the illumination method (preprocess_small_MS_SIMs.py's methods)")
    n.add_argument("--percentile-low", type=float, default=1.0, help="lower percentile of --normalization-method percentile")
    n.add_argument("--percentile-high", type=float, default=99.0, help="upper percentile")
    s = p.add_argument_group("sharpening (on the device)")
    s.add_argument("--sharpen", action="store_true", default=False,
                   help="unsharp mask on every tile's gray plane, the last step before the network "
                        "(preprocess_small_MS_SIMs.py --sharpen)")
    s.add_argument("--sharpen-sigma", type=float, default=1.0, help="sigma of the unsharp mask's Gaussian (up to about 16)")
    s.add_argument("--sharpen-amount", type=float, default=0.5, help="strength of the unsharp mask")
    c = p.add_argument_group("connected components (on the device)")
    c.add_argument("--morph-close-k", type=int, default=0, choices=range(0, 64), metavar="K",
                   help="close the binarised mask with a K x K ellipse before anything else is done with it "
                        "(build_dataset.py --morph-close-k; 0 = off, 1..63)")
    c.add_argument("--min-cc-px", type=int, default=0,
                   help="remove 8-connected components below this many pixels from the binarised mask "
                        "(build_dataset.py --min-cc-px; 0 = off)")
    c.add_argument("--cell-stats", action="store_true", default=False,
                   help="write cell_stats.csv: per image num_cells, mean / median / min / max area, tissue_coverage "
                        "of the mask that is written")
    c.add_argument("--cell-min-area", type=int, default=10, help="regions below this area are not counted as cells")
    c.add_argument("--cell-shapes", action="store_true", default=False,
                   help="write cell_shapes.csv: per image num_cells, mean / median perimeter, circularity, aspect ratio "
                        "and eccentricity of the cells (--cell-min-area) of the mask that is written")
    return p


def build_illumination(args):
    """The IlluminationCorrection the flags ask for, or None; ValueError on a size the kernel does not take. Needs no
    device."""
    if args.illumination_method == "none" and args.banding_method in ("none", "column"):   # column: build_normalization
        return None
    import _adipose_pkg  # noqa: F401
    from adipose_amd.illumination import IlluminationCorrection
    return IlluminationCorrection(
        banding=(args.morph_width, args.morph_height) if args.banding_method == "morphological" else None,
        method=None if args.illumination_method == "none" else args.illumination_method,
        radius=args.rolling_ball_radius, kernel_size=args.tophat_kernel)


def build_normalization(args):
    """The GrayNormalization the flags ask for, or None; ValueError on percentiles out of order. Needs no device."""
    if args.banding_method != "column" and args.normalization_method == "none":
        return None
    import _adipose_pkg  # noqa: F401
    from adipose_amd.normalization import GrayNormalization
    return GrayNormalization(
        column_banding=args.banding_method == "column", preserve_global=args.column_preserve_global,
        method=None if args.normalization_method == "none" else args.normalization_method,
        p_low=args.percentile_low, p_high=args.percentile_high)


def build_sharpen(args):
    """The UnsharpMask the flags ask for, or None; ValueError on a sigma whose blur radius the kernel does not take, or
    a non-finite amount. Needs no device."""
    if not args.sharpen:
        return None
    import _adipose_pkg  # noqa: F401
    from adipose_amd.sharpen import UnsharpMask
    return UnsharpMask(args.sharpen_sigma, args.sharpen_amount)


def main(argv=None):
    args = build_parser().parse_args(argv)
    try:
        illumination = build_illumination(args)
        normalization = build_normalization(args)
        sharpen = build_sharpen(args)
    except ValueError as e:
        print(f"❌ {e}")
        return 1
    images_dir, output_dir = Path(args.images_dir), Path(args.output_dir)
    if not images_dir.exists():
        print(f"❌ Error: Images directory not found: {images_dir}")
        return 1
    masks_dir = output_dir / "masks"
    masks_dir.mkdir(parents=True, exist_ok=True)
    overlays_dir = output_dir / "overlays"
    prob_dir = output_dir / "probabilities"
    if args.save_overlays:
        overlays_dir.mkdir(parents=True, exist_ok=True)
    if args.save_probability:
        prob_dir.mkdir(parents=True, exist_ok=True)

    print(f"\n{'=' * 80}\nADIPOSE TISSUE SEGMENTATION - INFERENCE\n{'=' * 80}")
    print(f"Images: {images_dir}\nOutput: {output_dir}\nThreshold: {args.threshold:.2f}")
    print(f"TTA: {'Enabled (' + args.tta_mode + ')' if args.use_tta else 'Disabled'}\n{'=' * 80}\n")

    import numpy as np

    import _adipose_pkg  # noqa: F401
    from adipose_amd.checkpoint import resolve_weights_file
    from adipose_amd.data import read_gray, read_rgb, write_mask
    from adipose_amd.predictor import AdiposeUNet, TestTimeAugmentation

    print("Loading model...")
    try:
        weights_file, checkpoint_dir = resolve_weights_file(args.weights)
    except FileNotFoundError as e:
        print(f"❌ {e}")
        return 1
    if weights_file.lower().endswith(".onnx"):
        print("❌ ONNX weights are not supported by the HIP engine (export the Keras-named weights instead)")
        return 1
    normalizer = None
    if args.stain_reference or args.stain_metadata:
        from adipose_amd.stain import ReinhardStainNormalizer, load_best_reference
        try:   # (both print the reference's name and LAB statistics)
            normalizer = (ReinhardStainNormalizer(args.stain_reference) if args.stain_reference
                          else load_best_reference(args.stain_metadata))
        except (FileNotFoundError, ValueError) as e:
            print(f"❌ {e}")
            return 1
    contrast = None
    if args.enhance_contrast:
        from adipose_amd.contrast import Clahe, clahe_geometry
        try:
            contrast = Clahe(args.clahe_clip_limit, args.clahe_tile_size)
            clahe_geometry(args.tile, args.tile, contrast.tile_grid)
        except ValueError as e:
            print(f"❌ {e}")
            return 1
        print(f"✓ Contrast enhancement: CLAHE clip limit {contrast.clip_limit:g}, "
              f"{contrast.tile_size} x {contrast.tile_size} tiles")
    if illumination is not None:
        print(f"✓ Background correction: {illumination}")
    if normalization is not None:
        print(f"✓ Gray normalisation: {normalization}")
    if sharpen is not None:
        print(f"✓ Sharpening: {sharpen} (blur radius {sharpen.radius})")
    model = AdiposeUNet(tile_size=args.tile, dtype=args.dtype, max_batch=args.batch, stain_normalizer=normalizer,
                        contrast=contrast, illumination=illumination, normalization=normalization, sharpen=sharpen)
    model.build_model()
    model.load_weights(weights_file)
    mean, std = load_normalization_stats(checkpoint_dir)
    tta = None
    if args.use_tta:
        tta = TestTimeAugmentation(mode=args.tta_mode)
        print(f"✓ TTA enabled: {args.tta_mode} mode ({len(tta.transforms)} augmentations)")
    color = COLORS[args.overlay_color]
    qc, qc_rows, skip_classes = None, [], ("empty", "blurry") if args.skip_blurry else ("empty",)
    if args.tile_qc:
        from adipose_amd.quality import CLASSES, TileQC, measures
        qc = TileQC(args.white_threshold, args.white_ratio_limit, args.blurry_threshold)
    raw_rgb = normalizer is not None or qc is not None
    cell_rows, shape_rows = [], []
    post = args.morph_close_k > 0 or args.min_cc_px > 0 or args.cell_stats or args.cell_shapes
    if post:
        import torch

        from adipose_amd import morphology
        from adipose_amd.components import (CELL_SHAPES_HEADER, CELL_STATS_HEADER, cell_shapes, cell_shapes_row,
                                            cell_statistics, cell_stats_row, remove_small_components,
                                            stats_from_shapes)

    image_files = [f for f in images_dir.iterdir() if f.suffix.lower() in IMAGE_EXTS and f.is_file()]
    if not image_files:
        print(f"❌ Error: No images found in {images_dir}\n   Looking for: {IMAGE_EXTS}")
        return 1
    print(f"\nFound {len(image_files)} images\nProcessing...\n")
    t0 = time.time()
    for img_path in image_files:
        try:
            image = read_rgb(img_path) if raw_rgb else read_gray(img_path)
        except Exception:  # cv2.imread returns None on unreadable files (:437-439)
            print(f"⚠️  Warning: Failed to load {img_path.name}, skipping")
            continue
        if image.shape[:2] != (args.tile, args.tile):
            print(f"⚠️  Warning: {img_path.name} is {image.shape}, expected ({args.tile}, {args.tile}), skipping")
            continue
        skipped = False
        if qc is not None:
            if image.ndim != 3 or image.shape[2] != 3:
                print(f"⚠️  Warning: {img_path.name} is not RGB, skipping")
                continue
            sums = qc.sums(image)
            ratio, var = measures(sums)
            cls = qc.classes_from_sums(sums)[0]
            skipped = cls in skip_classes
            qc_rows.append((img_path.name, f"{ratio[0]:.6f}", f"{var[0]:.6f}", cls, int(skipped)))
            if normalizer is None:   # the gray plane read_gray gives for the same file
                from adipose_amd.stain import gray_from_rgb_np
                image = gray_from_rgb_np(image)
        if normalizer is None:
            image = image.astype(np.float32)
        if skipped:   # no forward: the network is taken to have said "background"
            pred = np.zeros((args.tile, args.tile), np.float32)
        else:
            pred = (tta.predict_with_tta(model, image, mean, std) if tta is not None
                    else model.predict_single(image, mean, std))
        if args.save_probability:
            write_mask(prob_dir / f"{img_path.stem}_prob.tif", (pred * 255).astype(np.uint8))
        binary = (pred > args.threshold).astype(np.uint8)
        if skipped:   # all background: nothing to label
            if args.cell_stats:
                cell_rows.append(cell_stats_row(img_path.name))
            if args.cell_shapes:
                shape_rows.append(cell_shapes_row(img_path.name))
        elif post:   # threshold -> close -> small components -> statistics, as the reference builds its masks
            mask_dev = torch.from_numpy(binary).cuda()
            if args.morph_close_k > 0:
                mask_dev = morphology.close(mask_dev, args.morph_close_k)
            if args.min_cc_px > 0:
                mask_dev = remove_small_components(mask_dev, args.min_cc_px)
            if args.morph_close_k > 0 or args.min_cc_px > 0:
                binary = mask_dev.cpu().numpy()
            if args.cell_shapes:   # its dict holds the statistics too: with both flags the mask is labelled once
                shapes = cell_shapes(mask_dev, args.cell_min_area, 0.5)
                shape_rows.append(cell_shapes_row(img_path.name, shapes))
                if args.cell_stats:
                    cell_rows.append(cell_stats_row(img_path.name, stats_from_shapes(shapes)))
            elif args.cell_stats:
                cell_rows.append(cell_stats_row(img_path.name, cell_statistics(mask_dev, args.cell_min_area, 0.5)))
        write_mask(masks_dir / f"{img_path.stem}_mask.tif", binary)
        if args.save_overlays:
            from PIL import Image
            Image.fromarray(create_overlay_visualization(image, binary, color)).save(
                overlays_dir / f"{img_path.stem}_overlay.png")
    elapsed = time.time() - t0
    if qc is not None:
        import csv
        with open(output_dir / "tile_qc.csv", "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["name", "white_ratio", "lap_var", "class", "skipped"])
            w.writerows(qc_rows)
    if args.cell_stats:
        import csv
        with open(output_dir / "cell_stats.csv", "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(CELL_STATS_HEADER)
            w.writerows(cell_rows)
    if args.cell_shapes:
        import csv
        with open(output_dir / "cell_shapes.csv", "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(CELL_SHAPES_HEADER)
            w.writerows(shape_rows)
    print(f"\n{'=' * 80}\nINFERENCE COMPLETE\n{'=' * 80}")
    print(f"Processed: {len(image_files)} images")
    print(f"Time: {elapsed:.1f}s ({elapsed / len(image_files):.2f}s per image)")
    if qc is not None:
        counts = ", ".join(f"{c}={sum(1 for r in qc_rows if r[3] == c)}" for c in CLASSES)
        print(f"Tile QC: {counts}; skipped {sum(r[4] for r in qc_rows)} (classes {', '.join(skip_classes)}); "
              f"{output_dir / 'tile_qc.csv'}")
    print(f"\nOutput saved to:\n  Masks: {masks_dir}")
    if args.save_overlays:
        print(f"  Overlays: {overlays_dir}")
    if args.save_probability:
        print(f"  Probabilities: {prob_dir}")
    print(f"{'=' * 80}\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
