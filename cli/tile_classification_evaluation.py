#!/usr/bin/env python3
"""Drop-in CLI for Segmentation/tile_classification_evaluation.py (flags and defaults of :599-634, flow of main()
:637-736, returns 0/1) on the HIP engine: per-tile "Has Fat / No Fat" confusion matrices of a dataset's images/*.jpg
against its masks/*.tif.

Same behaviour as the reference: the output folder is {checkpoint}/evaluation/{dataset}_{source}_{enhancements}/
binary_classification_{threshold} when --output-dir is absent; --multi-threshold "1,5,10" writes one
binary_classification_{t} folder per threshold under {checkpoint}/evaluation/{dataset}_{source}_{enhancements} and
threshold_analysis.csv (and .png, if matplotlib is installed) beside them. Here all thresholds come from ONE inference
pass: the tiles' fat percentages are counted on the GPU (adp_fat_counts) and kept, and a threshold only classifies them.
The weights are resolved as cli/full_evaluation_enhanced.py resolves them (a file or a checkpoint directory).
Extra flags of this build: --tile (the reference hard-codes 1024), --dtype (f32 = the reference's numerics, bf16),
--batch (tiles per fat-count call, and tiles x TTA views per batched forward)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_parser():
    p = argparse.ArgumentParser(description="Tile-level binary classification evaluation (MI355X HIP engine)",
                                formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--weights", type=str, required=True, help="Path to trained model weights")
    p.add_argument("--data-root", type=str, required=True, help="Path to test dataset (contains images/ and masks/)")
    p.add_argument("--output-dir", type=str, default=None,
                   help="Output directory (optional - auto-generated if not provided)")
    p.add_argument("--threshold", type=float, default=10.0,
                   help='Fat percentage threshold for "Has Fat" classification (default: 10.0%%)')
    p.add_argument("--mask-threshold", type=float, default=0.5, help="Pixel threshold for binary mask (default: 0.5)")
    p.add_argument("--multi-threshold", type=str, default=None,
                   help='Evaluate multiple thresholds (comma-separated, e.g., "1,5,10,15,25")')
    p.add_argument("--use-tta", action="store_true", default=False, help="Enable Test Time Augmentation")
    p.add_argument("--tta-mode", type=str, default="basic", choices=["minimal", "basic", "full"])
    p.add_argument("--boundary-refine", action="store_true", default=False, help="Enable boundary refinement")
    p.add_argument("--refine-kernel", type=int, default=5, help="Kernel size for boundary refinement (default: 5)")
    # this build
    p.add_argument("--tile", type=int, default=1024, help="tile size the network is built for (reference: 1024)")
    p.add_argument("--dtype", type=str, default="f32", choices=["f32", "bf16"])
    p.add_argument("--batch", type=int, default=8, help="tiles per fat-count call; tiles x TTA views per batched forward")
    return p


def parse_args(argv=None):
    return build_parser().parse_args(argv)


def main(argv=None, model=None):
    """`model` (any object with predict_single) overrides loading AdiposeUNet from --weights: tests, custom
    predictors."""
    args = parse_args(argv)
    import _adipose_pkg  # noqa: F401
    from adipose_amd.tile_classification import resolve_weights_path, run_evaluation
    if model is None:
        try:
            args.weights, _ = resolve_weights_path(args.weights)
        except (ValueError, FileNotFoundError) as e:
            print(e)
            return 1
    return run_evaluation(args, model=model)


if __name__ == "__main__":
    sys.exit(main())
