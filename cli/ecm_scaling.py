#!/usr/bin/env python3
"""Drop-in CLI for pre-post-processing_tools/ECM_scaling.py (flags of :196-208, flow of main() :195-326): every image of
--target-dir (the ECM channel) is resampled to the exact width and height of the image of the same stem in
--reference-dir (the Pseudocolored slides), so that annotations and masks carry over between the two.

Same behaviour as the reference: --output-dir defaults to {target-dir}/resampled; a target stem matches a reference stem
exactly or after a trailing -ddd (-002, -003, ..) is stripped; a target without a match is counted as skipped; one that
already has the size is reported and counted as processed, and nothing is written for it; a target that fails is reported
with its traceback and the run goes on; the summary at the end; --dry-run writes nothing. Formats are kept (TIFF with
deflate, JPEG quality 95, PNG optimised); a 16-bit gray TIFF is brought to 8 bits by its minimum and maximum first.

Extra flag of this build: --interpolation {lanczos,bilinear,bicubic,nearest}, which the reference's docstring promises
and its parser lacks; the default, lanczos, is what the reference's code does. The resampling is Pillow's, bit for bit
(adipose_amd.resample): on the GPU (adp_resample_u8) where there is one, on the numpy path otherwise. Argument parsing
and --dry-run need neither a device nor the library."""
import argparse
import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

INTERPOLATIONS = ("lanczos", "bilinear", "bicubic", "nearest")
RULE = "=" * 70


def build_parser():
    p = argparse.ArgumentParser(description="Resample ECM images to match Pseudocolored reference dimensions")
    p.add_argument("--reference-dir", required=True, type=str, help="Directory containing Pseudocolored reference images")
    p.add_argument("--target-dir", required=True, type=str, help="Directory containing ECM images to resample")
    p.add_argument("--output-dir", type=str, default=None, help="Output directory (default: target-dir/resampled)")
    p.add_argument("--dry-run", action="store_true", help="Show what would be processed without writing files")
    # this build
    p.add_argument("--interpolation", type=str, default="lanczos", choices=INTERPOLATIONS,
                   help="resampling filter (default: lanczos, the reference's)")
    return p


def parse_args(argv=None):
    return build_parser().parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    reference_dir, target_dir = args.reference_dir, args.target_dir
    output_dir = args.output_dir or os.path.join(target_dir, "resampled")
    if not os.path.isdir(reference_dir):
        print(f"❌ Reference directory not found: {reference_dir}")
        return 1
    if not os.path.isdir(target_dir):
        print(f"❌ Target directory not found: {target_dir}")
        return 1
    import _adipose_pkg  # noqa: F401
    from adipose_amd.resample import (IMAGE_EXTS, build_reference_dict, get_image_size, match_reference,
                                      resample_image)   # (loads neither torch nor the library until an image is resampled)
    if not args.dry_run:
        os.makedirs(output_dir, exist_ok=True)
    print(RULE)
    print("ECM Image Scaling")
    print(RULE)
    print(f"Reference dir: {reference_dir}")
    print(f"Target dir:    {target_dir}")
    print(f"Output dir:    {output_dir}")
    print(f"Interpolation: {args.interpolation}")
    print(f"Dry run:       {args.dry_run}")
    print()
    print("📏 Reading reference image sizes...")
    sizes = build_reference_dict(reference_dir)
    if not sizes:
        print("❌ No valid reference images found")
        return 1
    print(f"\n✓ Found {len(sizes)} reference images")
    print("\n🔄 Processing target images...")
    processed = skipped = matched = 0
    for name in sorted(os.listdir(target_dir)):
        path = os.path.join(target_dir, name)
        stem, ext = os.path.splitext(name)
        if not os.path.isfile(path) or ext.lower() not in IMAGE_EXTS:
            continue
        ref = match_reference(stem, sizes)
        if ref is None:
            print(f"⚠️  No reference match for: {stem}")
            skipped += 1
            continue
        matched += 1
        target = sizes[ref]
        try:
            current = get_image_size(path)
            if current == target:
                print(f"✓ {stem}: Already correct size {current[0]}×{current[1]}")
                processed += 1
                continue
            print(f"🔄 {stem}:")
            print(f"   Current: {current[0]}×{current[1]}")
            print(f"   Target:  {target[0]}×{target[1]}")
            print(f"   Delta:   {current[0] - target[0]:+d}×{current[1] - target[1]:+d}")
            if args.dry_run:
                print(f"   [DRY RUN] Would save to: {name}")
            else:
                resample_image(path, target, os.path.join(output_dir, name), args.interpolation)
                print(f"   ✅ Saved to: {name}")
            processed += 1
        except Exception as e:   # the reference goes on with the next image
            print(f"❌ Failed to process {stem}: {e}")
            traceback.print_exc()
    print("\n" + RULE)
    print("Summary")
    print(RULE)
    print(f"Reference images:     {len(sizes)}")
    print(f"Matched targets:      {matched}")
    print(f"Successfully processed: {processed}")
    print(f"Skipped (no match):   {skipped}")
    print(RULE)
    if args.dry_run:
        print("\n⚠️  DRY RUN - No files were written")
    else:
        print(f"\n✅ Output saved to: {output_dir}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
