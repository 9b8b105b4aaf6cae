"""Reinhard stain normalisation (Reinhard et al., "Color transfer between images", 2001) of RGB tiles.

Mirrors the public surface of src/utils/stain_normalization.py so that a user of the reference can switch imports:
  * ReinhardStainNormalizer(reference_path=None, reference_metadata_path=None)   :32-146, :148-204, :297-309
      load_reference, reference_lab_stats ({'L': {'mean', 'std'}, 'A': ..., 'B': ...}), normalize_image,
      normalize_batch, get_reference_info
  * load_best_reference(metadata_path)                                           :312-345
  * normalize_with_zscore, complete_preprocessing_pipeline                       :348-376, :409-438
Extras: set_reference_stats (the six numbers without an image) and normalize_tiles ((N, H, W, 3) uint8 batch on the
device, on the current stream; the predictor's entry). validate_normalization and the matplotlib comparison are left
out (they need cv2).

uint8 HWC input on a host with a GPU runs on the device (adp_stain_lab_stats + adp_stain_reinhard_apply: conversions
in f32, sums in f64, every tile with its own statistics). Float input in [0, 1] -- and any input on a host without a
GPU -- takes the float64 numpy implementation of the same maths in this module (rgb2lab_np, lab2rgb_np, reinhard_np),
which is also the tests' reference. The colour conversions restate skimage's documented rgb2lab / lab2rgb (D65 white,
2-degree observer); skimage is not a dependency.
"""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np

CHANNELS = ("L", "A", "B")
IMAGE_EXTS = {".jpg", ".jpeg", ".png", ".tif", ".tiff"}

XYZ_FROM_RGB = np.array([[0.412453, 0.357580, 0.180423],
                         [0.212671, 0.715160, 0.072169],
                         [0.019334, 0.119193, 0.950227]], np.float64)
RGB_FROM_XYZ = np.linalg.inv(XYZ_FROM_RGB)
WHITE_D65 = np.array([0.95047, 1.0, 1.08883], np.float64)


# ---------------------------------------------------------------- float64 numpy path
def rgb2lab_np(rgb):
    """(..., 3) RGB in [0, 1] -> CIE LAB, float64."""
    c = np.asarray(rgb, np.float64)
    lin = np.where(c > 0.04045, np.power((c + 0.055) / 1.055, 2.4), c / 12.92)
    xyz = lin @ XYZ_FROM_RGB.T / WHITE_D65
    f = np.where(xyz > 0.008856, np.cbrt(xyz), 7.787 * xyz + 16.0 / 116.0)
    fx, fy, fz = f[..., 0], f[..., 1], f[..., 2]
    return np.stack([116.0 * fy - 16.0, 500.0 * (fx - fy), 200.0 * (fy - fz)], axis=-1)


def lab2rgb_np(lab):
    """(..., 3) CIE LAB -> RGB, float64, clipped to [0, 1]."""
    lab = np.asarray(lab, np.float64)
    fy = (lab[..., 0] + 16.0) / 116.0
    fx = lab[..., 1] / 500.0 + fy
    fz = np.maximum(fy - lab[..., 2] / 200.0, 0.0)
    f = np.stack([fx, fy, fz], axis=-1)
    xyz = np.where(f > 0.2068966, f ** 3, (f - 16.0 / 116.0) / 7.787) * WHITE_D65
    lin = xyz @ RGB_FROM_XYZ.T
    enc = np.where(lin > 0.0031308, 1.055 * np.power(np.maximum(lin, 0.0), 1.0 / 2.4) - 0.055, 12.92 * lin)
    return np.clip(enc, 0.0, 1.0)


def lab_stats_np(lab):
    """(H, W, 3) LAB -> [meanL, meanA, meanB, stdL, stdA, stdB] (population std), float64."""
    flat = np.asarray(lab, np.float64).reshape(-1, 3)
    return np.concatenate([flat.mean(axis=0), flat.std(axis=0)])


def reinhard_lab_np(image, target):
    """The transformed LAB image (before the conversion back to RGB) of one (H, W, 3) image; `target` as lab_stats_np
    returns it. The image is scaled by 1/255 when its maximum exceeds 1 (the reference's range rule)."""
    image = np.asarray(image)
    src = image / 255.0 if image.max() > 1.0 else image.astype(np.float64)
    lab = rgb2lab_np(src)
    st = lab_stats_np(lab)
    out = np.empty_like(lab)
    for c in range(3):
        if st[3 + c] == 0:
            out[..., c] = target[c]
        else:
            out[..., c] = (lab[..., c] - st[c]) * (target[3 + c] / st[3 + c]) + target[c]
    return out


def reinhard_np(image, target):
    """normalize_image in float64 numpy: an image with values above 1 comes back as uint8 (x * 255 truncated), one in
    [0, 1] as float64."""
    image = np.asarray(image)
    rgb = lab2rgb_np(reinhard_lab_np(image, target))
    return (rgb * 255).astype(np.uint8) if image.max() > 1.0 else rgb


def gray_from_rgb_np(rgb):
    """PIL's mode-L conversion of uint8 RGB, (R*19595 + G*38470 + B*7471 + 0x8000) >> 16, as data.read_gray returns it
    for the saved image -> float32."""
    v = np.asarray(rgb).astype(np.uint32)
    return ((v[..., 0] * 19595 + v[..., 1] * 38470 + v[..., 2] * 7471 + 0x8000) >> 16).astype(np.float32)


def _stats_dict(vec):
    return {ch: {"mean": float(vec[i]), "std": float(vec[3 + i])} for i, ch in enumerate(CHANNELS)}


def _stats_vec(stats):
    if isinstance(stats, dict):
        return np.array([stats[ch]["mean"] for ch in CHANNELS] + [stats[ch]["std"] for ch in CHANNELS], np.float64)
    vec = np.asarray(stats, np.float64).reshape(-1)
    if vec.shape != (6,):
        raise ValueError("reference statistics: six numbers (mean L, A, B, std L, A, B) or the nested dict")
    return vec


def _gpu():
    import torch
    return torch.cuda.is_available()


# ---------------------------------------------------------------- device path
def _check_batch(batch):
    import torch
    if not (batch.is_cuda and batch.dtype == torch.uint8 and batch.dim() == 4 and batch.shape[3] == 3
            and batch.is_contiguous()):
        raise TypeError("stain kernels take a contiguous (N, H, W, 3) uint8 device tensor")
    return batch.shape[:3]


def lab_stats_device(batch):
    """(N, H, W, 3) uint8 device tensor -> (N, 6) f64 device tensor of per-tile LAB statistics."""
    import torch

    from ._lib import call, ptr, stream_ptr
    N, H, W = _check_batch(batch)
    stats = torch.empty((N, 6), dtype=torch.float64, device=batch.device)
    call("adp_stain_lab_stats", N, H, W, ptr(batch), ptr(stats), stream_ptr())
    return stats


def apply_device(batch, src_stats, target, rgb=True, gray=False):
    """adp_stain_reinhard_apply -> (rgb uint8 (N, H, W, 3) or None, gray f32 (N, H, W) or None)."""
    import ctypes as C

    import torch

    from ._lib import call, ptr, stream_ptr
    N, H, W = _check_batch(batch)
    out = torch.empty_like(batch) if rgb else None
    g = torch.empty((N, H, W), dtype=torch.float32, device=batch.device) if gray else None
    tgt = (C.c_double * 6)(*[float(v) for v in target])
    call("adp_stain_reinhard_apply", N, H, W, ptr(batch), ptr(src_stats), tgt, ptr(out), ptr(g), stream_ptr())
    return out, g


class ReinhardStainNormalizer:
    """Reinhard normalisation towards the LAB statistics of a reference image."""

    def __init__(self, reference_path=None, reference_metadata_path=None):
        self.reference_path = reference_path
        self.reference_metadata_path = reference_metadata_path
        self.reference_image = None
        self.reference_lab_stats = None
        self.reference_metadata = None
        if reference_path:
            self.load_reference(reference_path, reference_metadata_path)

    # -- reference
    def load_reference(self, reference_path, metadata_path=None):
        from PIL import Image

        path = Path(reference_path)
        if not path.exists():
            raise FileNotFoundError(f"Reference image not found: {reference_path}")
        self.reference_path = path
        self.reference_image = np.array(Image.open(path))
        if self.reference_image.ndim != 3 or self.reference_image.shape[2] != 3:
            raise ValueError("Reference image must be RGB")
        self.reference_lab_stats = self._calculate_lab_stats(self.reference_image)
        if metadata_path:
            self.reference_metadata_path = Path(metadata_path)
            if self.reference_metadata_path.exists():
                with open(self.reference_metadata_path) as f:
                    self.reference_metadata = json.load(f)
        print(f"Reference loaded: {path.name}")
        print(self.stats_line())

    def set_reference_stats(self, stats):
        """Target statistics without an image: [meanL, meanA, meanB, stdL, stdA, stdB] or the nested dict."""
        self.reference_lab_stats = _stats_dict(_stats_vec(stats))

    def stats_line(self):
        s = self.reference_lab_stats
        return "Reference LAB stats: " + ", ".join(
            f"{ch}={s[ch]['mean']:.1f}±{s[ch]['std']:.1f}" for ch in CHANNELS)

    def _calculate_lab_stats(self, image):
        """Statistics of one image in float64 (the reference is read once; tiles go through normalize_tiles)."""
        image = np.asarray(image)
        return _stats_dict(lab_stats_np(rgb2lab_np(image / 255.0 if image.max() > 1.0 else image)))

    def _target(self):
        if self.reference_lab_stats is None:
            raise ValueError("No reference loaded. Call load_reference() first.")
        return _stats_vec(self.reference_lab_stats)

    # -- normalisation
    def normalize_tiles(self, batch_uint8, out_gray=False):
        """(N, H, W, 3) uint8 tensor or array -> normalised uint8 device tensor (N, H, W, 3), every tile with its own
        statistics; with out_gray the fused PIL-mode-L plane (N, H, W) f32 instead. Runs on the current stream."""
        import torch

        target = self._target()
        b = torch.from_numpy(np.ascontiguousarray(batch_uint8)) if isinstance(batch_uint8, np.ndarray) else batch_uint8
        if b.dtype != torch.uint8 or b.dim() != 4 or b.shape[3] != 3:
            raise TypeError("normalize_tiles takes (N, H, W, 3) uint8")
        if not b.is_cuda:
            b = b.to(torch.device("cuda", torch.cuda.current_device()))
        b = b.contiguous()
        rgb, gray = apply_device(b, lab_stats_device(b), target, rgb=not out_gray, gray=out_gray)
        return gray if out_gray else rgb

    def normalize_image(self, source_image):
        """One (H, W, 3) image, 0-255 or 0-1 -> the normalised image in the input's range (uint8 or float)."""
        target = self._target()
        img = np.asarray(source_image)
        if img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3 and img.size and _gpu():
            return self.normalize_tiles(img[None])[0].cpu().numpy()
        return reinhard_np(img, target)

    def normalize_batch(self, image_paths, output_dir=None, preserve_names=True):
        """Normalise image files (a list of paths, one path or a directory); without output_dir the files are
        overwritten. Returns the paths written; a file that fails is reported and skipped."""
        from PIL import Image

        if isinstance(image_paths, (str, Path)):
            p = Path(image_paths)
            image_paths = [q for q in p.iterdir() if q.suffix.lower() in IMAGE_EXTS] if p.is_dir() else [p]
        if output_dir:
            output_dir = Path(output_dir)
            output_dir.mkdir(parents=True, exist_ok=True)
        done = []
        print(f"Normalizing {len(image_paths)} images...")
        for i, src in enumerate(image_paths):
            src = Path(src)
            print(f"Processing {src.name} ({i + 1}/{len(image_paths)})")
            try:
                out = self.normalize_image(np.array(Image.open(src)))
                if not output_dir:
                    dst = src
                elif preserve_names:
                    dst = output_dir / src.name
                else:
                    dst = output_dir / f"normalized_{i:04d}{src.suffix}"
                Image.fromarray(out).save(dst)
                done.append(dst)
            except Exception as e:  # the reference reports and goes on
                print(f"Error processing {src.name}: {e}")
        print(f"Successfully normalized {len(done)} images")
        return done

    def get_reference_info(self):
        if self.reference_path is None:
            return "No reference loaded"
        return {"reference_path": str(self.reference_path), "reference_name": Path(self.reference_path).name,
                "lab_stats": self.reference_lab_stats, "metadata": self.reference_metadata}


def load_best_reference(metadata_path=None):
    """The normaliser for the reference chosen by the reference selector: `selected_reference.path` of its JSON
    (default: stain_reference_metadata.json beside this module)."""
    metadata_path = Path(metadata_path) if metadata_path else Path(__file__).parent / "stain_reference_metadata.json"
    if not metadata_path.exists():
        raise FileNotFoundError(f"Reference metadata not found: {metadata_path}\n"
                                "Run select_stain_reference.py first to select optimal reference")
    with open(metadata_path) as f:
        sel = json.load(f)["selected_reference"]
    normalizer = ReinhardStainNormalizer(sel["path"], metadata_path)
    for key, label, fmt in (("name", "Loaded best reference", "{}"), ("composite_score", "Composite score", "{:.3f}"),
                            ("stain_type", "Stain type", "{}")):
        if key in sel:
            print(f"{label}: {fmt.format(sel[key])}")
    return normalizer


def normalize_with_zscore(image, mean=200.99, std=25.26):
    """Shift and scale a 0-255 image to the given mean and std (float32 arithmetic), clipped, as uint8."""
    x = np.asarray(image).astype(np.float32)
    m, s = x.mean(), x.std()
    if s > 0:
        x = (x - m) / s * std + mean
    return np.clip(x, 0, 255).astype(np.uint8)


def complete_preprocessing_pipeline(image, normalizer, apply_zscore=True, zscore_mean=200.99, zscore_std=25.26,
                                    percentile_low=1.0, percentile_high=99.0):
    """Stain normalisation, then (optionally) normalize_with_zscore; `image` is an array or a path. The percentile
    arguments are accepted for the reference's signature and, as there, unused."""
    if isinstance(image, (str, Path)):
        from PIL import Image
        image = np.array(Image.open(image))
    out = normalizer.normalize_image(image)
    return normalize_with_zscore(out, zscore_mean, zscore_std) if apply_zscore else out
