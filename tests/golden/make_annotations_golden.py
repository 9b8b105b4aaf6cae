"""Golden vectors for the annotation JSON readers (Segmentation/build_dataset.py: parse_image_stem_from_json :494-503,
load_json_annotations :738-800, slide_has_valid_annotations :803-837, get_tile_annotations :840-900), generated HERE
from the reference's own functions on the hand-written files under tests/golden/annotations/. The module imports cv2 /
tifffile at load time; they are satisfied by make_golden's inert stubs (none of the four functions calls them). Data only
is written (tests/golden/annotations.npz); no reference source is stored. The rasters are NOT reference output (cv2 is
not installed) and are not stored here. Usage:
    python tests/golden/make_annotations_golden.py [/root/reference]
"""
import contextlib
import importlib.util
import io
import os
import sys
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
JSON_DIR = Path(HERE) / "annotations"
CONFIDENCES = [1, 2, 3]
BBOXES = [(0, 0, 64, 64), (64, 0, 128, 64), (0, 32, 48, 128), (90, 90, 130, 130), (-20, 40, 0, 80), (200, 200, 264, 264)]
STEM_CASES = [("slideA_fat_annotations.json", "fat"), ("slideA_bubbles_annotations.json", "bubbles"),
              ("slide_B x_fat_v2.json", "fat"), ("a_b_c_fat_annotations_v3.json", "fat"), ("plain.json", "fat"),
              ("x_fat_y_fat_annotations.json", "fat"), ("slideA_fat_annotations.json", "muscle"),
              ("s_bubbles_fat_annotations.json", "bubbles")]


def pack(polys):
    """A list of (n, 2) arrays -> (flat int64 (V, 2), lengths)."""
    lens = np.array([len(p) for p in polys], np.int64)
    flat = np.concatenate([np.asarray(p, np.int64).reshape(-1, 2) for p in polys]) if polys else np.zeros((0, 2), np.int64)
    return flat, lens


def main():
    make_golden.REF = REF
    sys.meta_path.insert(0, make_golden._StubFinder())
    sys.path.insert(0, REF)
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("ref_build_dataset", os.path.join(REF, "Segmentation", "build_dataset.py"))
    bd = importlib.util.module_from_spec(spec)
    with contextlib.redirect_stdout(io.StringIO()):
        spec.loader.exec_module(bd)
    out = {"confidences": np.array(CONFIDENCES), "bboxes": np.array(BBOXES)}
    names = sorted(p.name for p in JSON_DIR.glob("*.json"))
    out["files"] = np.array(names)
    for i, name in enumerate(names):
        path = JSON_DIR / name
        for c in CONFIDENCES:
            polys, missing = bd.load_json_annotations(path, c)
            assert all(p.dtype == np.int32 for p in polys)
            out[f"load_{i}_{c}_xy"], out[f"load_{i}_{c}_len"] = pack(polys)
            out[f"load_{i}_{c}_missing"] = np.array(bool(missing))
            out[f"valid_{i}_{c}"] = np.array(bool(bd.slide_has_valid_annotations(path, c)))
            for b, box in enumerate(BBOXES):
                polys, low_only = bd.get_tile_annotations(path, box, c)
                out[f"tile_{i}_{c}_{b}_xy"], out[f"tile_{i}_{c}_{b}_len"] = pack(polys)
                out[f"tile_{i}_{c}_{b}_low"] = np.array(bool(low_only))
    out["stem_names"] = np.array([n for n, _ in STEM_CASES])
    out["stem_cls"] = np.array([c for _, c in STEM_CASES])
    out["stem_out"] = np.array([bd.parse_image_stem_from_json(Path("/some/dir") / n, c) for n, c in STEM_CASES])
    dst = os.path.join(HERE, "annotations.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, len(out), "arrays,", os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
