"""Writes tests/golden/resample.npz: inputs, target sizes and PIL.Image.resize's outputs for tests/test_resample.py.

Only numpy and Pillow are used here, so the file records what Pillow itself computed (Pillow 12.2.0 when it was made) and
keeps adipose_amd.resample pinned where another Pillow, or another C library's sin, is installed. Pillow has no interface
to its coefficient tables, so none are recorded: the `impulse` cases (one 255 pixel per 16 on a zero row, and its
complement) bring single taps to the output instead.

    python tests/golden/make_resample_golden.py
"""
import os

import numpy as np
from PIL import Image

FILTERS = ("box", "bilinear", "hamming", "bicubic", "lanczos", "nearest")
# (name, H, W, C, Ho, Wo)
CASES = [
    ("ecm", 45, 53, 1, 48, 50),
    ("up", 20, 24, 1, 47, 55),
    ("down", 61, 70, 1, 23, 26),
    ("rgb", 31, 29, 3, 27, 34),
    ("wide_only", 17, 40, 1, 17, 33),
    ("tall_only", 40, 17, 3, 33, 17),
    ("one", 1, 1, 1, 3, 5),
    ("thin", 1, 7, 1, 4, 3),
    ("far_down", 96, 100, 1, 3, 4),
]


def main():
    rng = np.random.default_rng(20261021)
    out = {"filters": np.array(FILTERS), "cases": np.array([c[0] for c in CASES])}
    for name, H, W, C, Ho, Wo in CASES:
        a = rng.integers(0, 256, (H, W) if C == 1 else (H, W, C), dtype=np.uint8)
        if name == "down":
            a = ((a > 127) * 255).astype(np.uint8)   # a 0 / 255 image: the clamp on both sides
        out[f"{name}_in"] = a
        out[f"{name}_size"] = np.array([Wo, Ho])
        for f in FILTERS:
            out[f"{name}_{f}"] = np.asarray(Image.fromarray(a).resize((Wo, Ho), getattr(Image.Resampling, f.upper())))
    row = np.zeros((1, 160), np.uint8)
    row[0, 5::16] = 255
    out["impulse_in"] = np.concatenate([row, 255 - row])
    for m in (163, 157, 320, 61, 11):
        for f in FILTERS:
            out[f"impulse_{m}_{f}"] = np.asarray(Image.fromarray(out["impulse_in"]).resize((m, 2), getattr(Image.Resampling, f.upper())))
    out["impulse_widths"] = np.array([163, 157, 320, 61, 11])
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "resample.npz"), **out)


if __name__ == "__main__":
    main()
