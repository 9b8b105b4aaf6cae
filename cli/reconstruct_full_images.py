#!/usr/bin/env python3
"""Drop-in CLI for Segmentation/reconstruct_full_images.py (flags and defaults of :873-931, main() :934-953,
returns 0/1) on the HIP engine. Extra flags of this build: --dtype (f32 = the reference's numerics, bf16),
--batch (tiles x TTA views per forward). Launched with torch.distributed.run (WORLD_SIZE > 1), each rank
predicts a contiguous run of every slide's tiles and the blend accumulators are SUM-reduced over RCCL."""
import argparse
import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_parser():
    p = argparse.ArgumentParser(description="Reconstruct full images from overlapping tiles",
                                formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--weights", type=str, required=True, help="Path to trained model weights")
    p.add_argument("--data-root", type=str, required=True,
                   help="Path to dataset directory (contains images/ and masks/)")
    p.add_argument("--output-dir", type=str, required=True, help="Output directory for reconstructed images")
    p.add_argument("--tile-size", type=int, default=1024, help="Tile size (default: 1024)")
    p.add_argument("--stride", type=int, default=512, help="Stride between tiles (default: 512 for 50%% overlap)")
    p.add_argument("--threshold", type=float, default=0.5, help="Threshold for binary masks (default: 0.5)")
    p.add_argument("--blend-mode", type=str, default="gaussian", choices=["gaussian", "linear"])
    p.add_argument("--use-tta", action="store_true", default=False, help="Enable Test Time Augmentation")
    p.add_argument("--tta-mode", type=str, default="basic", choices=["minimal", "basic", "full"])
    p.add_argument("--boundary-refine", action="store_true", default=False, help="Enable boundary refinement")
    p.add_argument("--refine-kernel", type=int, default=5)
    p.add_argument("--save-masks", action="store_true", default=True)
    p.add_argument("--save-overlays", action="store_true", default=False)
    p.add_argument("--save-comparisons", action="store_true", default=False)
    p.add_argument("--save-metrics", action="store_true", default=False)
    p.add_argument("--min-coverage", type=float, default=0.90)
    p.add_argument("--max-tiles", type=int, default=None)
    p.add_argument("--dtype", type=str, default="f32", choices=["f32", "bf16"])
    p.add_argument("--batch", type=int, default=8)
    c = p.add_argument_group("connected components (on the device, on the whole-slide mask)")
    c.add_argument("--morph-close-k", type=int, default=0, choices=range(0, 64), metavar="K",
                   help="close the thresholded slide mask with a K x K ellipse before anything else is done with it "
                        "(build_dataset.py --morph-close-k; 0 = off, 1..63)")
    c.add_argument("--min-cc-px", type=int, default=0,
                   help="remove 8-connected components below this many pixels from the thresholded slide mask "
                        "(build_dataset.py --min-cc-px; 0 = off); the mask, the overlays and the metrics then use it")
    c.add_argument("--cell-stats", action="store_true", default=False,
                   help="write cell_stats.csv: per slide num_cells, mean / median / min / max area, tissue_coverage")
    c.add_argument("--cell-min-area", type=int, default=10, help="regions below this area are not counted as cells")
    c.add_argument("--cell-shapes", action="store_true", default=False,
                   help="write cell_shapes.csv: per slide num_cells, mean / median perimeter, circularity, aspect ratio "
                        "and eccentricity of the cells (--cell-min-area)")
    g = p.add_argument_group("ground truth from the annotators' polygons (rasterised on the device at full resolution)")
    g.add_argument("--annotations-dir", type=str, default=None, metavar="DIR",
                   help="the builder's Masks folder (<class>/*.json): a slide whose stem has a JSON gets its ground truth "
                        "from the polygons instead of the blended mask tiles")
    g.add_argument("--annotation-class", type=str, default="fat", help="class folder of the target polygons")
    g.add_argument("--annotation-subtract-class", type=str, default="bubbles",
                   help="class whose polygons are subtracted (build_dataset.py --subtract-class; 'none' = off; a slide "
                        "without such a JSON is not subtracted)")
    g.add_argument("--annotation-min-confidence", type=int, default=2,
                   help="records below this confidenceScore are left out (build_dataset.py --test-min-confidence)")
    g.add_argument("--gt-morph-close-k", type=int, default=0, choices=range(0, 64), metavar="K",
                   help="close the rasterised ground truth with a K x K ellipse (build_dataset.py --morph-close-k; 0 = off)")
    g.add_argument("--gt-min-cc-px", type=int, default=0,
                   help="remove the ground truth's 8-connected components below this many pixels "
                        "(build_dataset.py --min-cc-px; 0 = off)")
    return p


def parse_args(argv=None):
    return build_parser().parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    group = None
    try:
        import torch
        import _adipose_pkg  # noqa: F401
        from adipose_amd.reconstruct import reconstruct_all_slides
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            import torch.distributed as dist
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
            dist.init_process_group("nccl")
            group = dist.group.WORLD
        reconstruct_all_slides(args, process_group=group)
        return 0
    except Exception as e:  # noqa: BLE001 (:949-953)
        print(f"\n❌ Reconstruction failed: {e}")
        traceback.print_exc()
        return 1
    finally:
        if group is not None:
            import torch.distributed as dist
            dist.destroy_process_group()


if __name__ == "__main__":
    sys.exit(main())
