"""Tile quality control: empty / blurry / tissue, the reference's classify_tiles_batch
(Segmentation/build_dataset.py:1253-1284, build_test_dataset.py:634-660; defaults :170-172).

  empty    more than `white_ratio_limit` (0.70) of the pixels have R, G and B all >= `white_threshold` (235)
  blurry   the variance of the 3x3 Laplacian of the gray tile is below `blurry_threshold` (7.5)
  tissue   everything else (the tests run in this order: a white and smooth tile is empty)

The measurements come from four integers per tile, {white, S1 = sum lap, S2 = sum lap^2, n = H*W}:
  gray  (R*9798 + G*19235 + B*3735 + 16384) >> 15   OpenCV 4's 8-bit COLOR_BGR2GRAY, restated: cv2 is not a dependency,
        so parity with cv2 itself is unpinned. The tiles here are RGB (the reference passes BGR): the white test is
        symmetric in the channels and the gray formula names its channels.
  lap   g(y-1,x) + g(y+1,x) + g(y,x-1) + g(y,x+1) - 4 g(y,x), reflect-101 borders within the tile: cv2.Laplacian(gray,
        CV_64F) with its default ksize=1 and border.
On a host with a GPU the sums are adp_tile_qc (csrc/tileqc.hip): one launch for a batch of tiles, or for any number of
-- possibly overlapping -- windows of one device image, read in place. qc_sums_np is the same arithmetic in numpy: the
path of hosts without a GPU and the tests' reference. Integer sums are exact, so the two agree bit for bit.
"""
from __future__ import annotations

import numpy as np

CLASSES = ("empty", "blurry", "tissue")


# ---------------------------------------------------------------- numpy path
def gray_cv_np(rgb):
    """OpenCV's 8-bit gray of uint8 RGB (..., 3) -> int64 (...)."""
    v = np.asarray(rgb).astype(np.int64)
    return (v[..., 0] * 9798 + v[..., 1] * 19235 + v[..., 2] * 3735 + 16384) >> 15


def qc_sums_np(tiles, white_threshold=235):
    """(N, H, W, 3) or (H, W, 3) uint8 RGB -> (N, 4) int64 {white, S1, S2, H*W}."""
    t = np.asarray(tiles)
    if t.ndim == 3:
        t = t[None]
    if t.dtype != np.uint8 or t.ndim != 4 or t.shape[3] != 3:
        raise TypeError("quality control takes (N, H, W, 3) uint8 RGB tiles")
    N, H, W = t.shape[:3]
    if N < 1 or H < 2 or W < 2:
        raise ValueError("quality control needs N >= 1 and H, W >= 2 (reflect-101 borders)")
    white = (t.astype(np.int64) >= int(white_threshold)).all(axis=-1).sum(axis=(1, 2))
    g = np.pad(gray_cv_np(t), ((0, 0), (1, 1), (1, 1)), mode="reflect")
    lap = g[:, :-2, 1:-1] + g[:, 2:, 1:-1] + g[:, 1:-1, :-2] + g[:, 1:-1, 2:] - 4 * g[:, 1:-1, 1:-1]
    return np.stack([white, lap.sum(axis=(1, 2)), (lap * lap).sum(axis=(1, 2)), np.full(N, H * W, np.int64)],
                    axis=1).astype(np.int64)


def measures(sums):
    """(N, 4) sums (array or tensor) -> (white_ratio, lap_var) float64 arrays. lap_var is the population variance
    (n*S2 - S1^2) / n^2, numerator and denominator in Python ints: n*S2 passes 2^63 just above 1024^2 pixels."""
    s = sums.cpu().numpy() if hasattr(sums, "cpu") else np.asarray(sums)
    rows = [[int(v) for v in r] for r in s.reshape(-1, 4)]
    ratio = np.array([w / n for w, _, _, n in rows], np.float64)
    var = np.array([(n * s2 - s1 * s1) / (n * n) for _, s1, s2, n in rows], np.float64)
    return ratio, var


# ---------------------------------------------------------------- device path
def _launch(N, H, W, base, pitch, origins, white_threshold, device):
    import torch

    from ._lib import call, ptr, stream_ptr
    sums = torch.empty((N, 4), dtype=torch.int64, device=device)
    call("adp_tile_qc", N, H, W, ptr(base), pitch, ptr(origins), int(white_threshold), ptr(sums), stream_ptr())
    return sums


def qc_sums_device(batch, white_threshold=235):
    """Contiguous (N, H, W, 3) uint8 device tensor -> (N, 4) int64 device tensor. Runs on the current stream."""
    import torch
    if not (batch.is_cuda and batch.dtype == torch.uint8 and batch.dim() == 4 and batch.shape[3] == 3
            and batch.is_contiguous()):
        raise TypeError("qc_sums_device takes a contiguous (N, H, W, 3) uint8 device tensor")
    N, H, W = batch.shape[:3]
    return _launch(N, H, W, batch, 0, None, white_threshold, batch.device)


def qc_sums_windows(image, positions, tile, white_threshold=235):
    """The sums of the tile x tile windows with top-left corners `positions` [(y, x), ...] of an (H, W, 3) uint8 device
    image: one launch, the windows are read in place (each reflects at its own edge)."""
    import torch
    if not (image.is_cuda and image.dtype == torch.uint8 and image.dim() == 3 and image.shape[2] == 3
            and image.is_contiguous()):
        raise TypeError("qc_sums_windows takes a contiguous (H, W, 3) uint8 device image")
    H, W = image.shape[:2]
    T = int(tile)
    pos = [(int(y), int(x)) for y, x in positions]
    if not pos:
        return torch.empty((0, 4), dtype=torch.int64, device=image.device)
    if any(y < 0 or x < 0 or y + T > H or x + T > W for y, x in pos):
        raise ValueError(f"a {T} x {T} window lies outside the {H} x {W} image")
    pitch = 3 * W
    origins = torch.tensor([y * pitch + 3 * x for y, x in pos], dtype=torch.int64).to(image.device)
    return _launch(len(pos), T, T, image, pitch, origins, white_threshold, image.device)


def _gpu():
    import torch
    return torch.cuda.is_available()


def _is_tensor(t):
    return hasattr(t, "is_cuda")


def _as_batch(tiles):
    """A batch (N, H, W, 3) array / tensor, one tile (H, W, 3), or a list of tiles -> one array or tensor (N, H, W, 3)."""
    if isinstance(tiles, (list, tuple)):
        if any(_is_tensor(t) for t in tiles):
            import torch
            return torch.stack([t if _is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t)).to(tiles[0].device)
                                for t in tiles])
        return np.stack([np.asarray(t) for t in tiles])
    return tiles[None] if tiles.ndim == 3 else tiles


class TileQC:
    """The reference's tile classifier with its defaults (build_dataset.py:170-172)."""

    def __init__(self, white_threshold=235, white_ratio_limit=0.70, blurry_threshold=7.5):
        self.white_threshold = int(white_threshold)
        self.white_ratio_limit = float(white_ratio_limit)
        self.blurry_threshold = float(blurry_threshold)

    # -- sums
    def sums(self, tiles):
        """RGB uint8 tiles (array or tensor, host or device, a batch, one tile or a list) -> (N, 4) sums: on the device
        where there is one (a host array is uploaded), in numpy otherwise."""
        b = _as_batch(tiles)
        if _is_tensor(b):
            import torch
            if b.dtype != torch.uint8 or b.dim() != 4 or b.shape[3] != 3:
                raise TypeError("quality control takes (N, H, W, 3) uint8 RGB tiles")
            if not b.is_cuda and not _gpu():
                return qc_sums_np(b.numpy(), self.white_threshold)
            if not b.is_cuda:
                b = b.to(torch.device("cuda", torch.cuda.current_device()))
            return qc_sums_device(b.contiguous(), self.white_threshold)
        if not _gpu():
            return qc_sums_np(b, self.white_threshold)
        import torch
        if b.dtype != np.uint8 or b.ndim != 4 or b.shape[3] != 3:
            raise TypeError("quality control takes (N, H, W, 3) uint8 RGB tiles")
        dev = torch.device("cuda", torch.cuda.current_device())
        b = np.ascontiguousarray(b)
        return qc_sums_device(torch.from_numpy(b if b.flags.writeable else b.copy()).to(dev), self.white_threshold)

    def window_sums(self, image, positions, tile):
        """The sums of windows of one (H, W, 3) uint8 RGB image (array or tensor, host or device)."""
        T = int(tile)
        if not _gpu() and not (_is_tensor(image) and image.is_cuda):
            img = image.numpy() if _is_tensor(image) else np.asarray(image)
            if not len(positions):
                return np.empty((0, 4), np.int64)
            return qc_sums_np(np.stack([img[y:y + T, x:x + T] for y, x in positions]), self.white_threshold)
        import torch
        img = image if _is_tensor(image) else torch.from_numpy(np.array(image, order="C"))
        if not img.is_cuda:
            img = img.to(torch.device("cuda", torch.cuda.current_device()))
        return qc_sums_windows(img.contiguous(), positions, T, self.white_threshold)

    # -- classes
    def classes_from_sums(self, sums):
        """The reference's order of tests: white_ratio > limit first, then lap_var < blurry_threshold."""
        ratio, var = measures(sums)
        return ["empty" if r > self.white_ratio_limit else "blurry" if v < self.blurry_threshold else "tissue"
                for r, v in zip(ratio, var)]

    def measure(self, tiles):
        """-> (white_ratio, lap_var), float64 arrays of length N."""
        return measures(self.sums(tiles))

    def classify(self, tiles):
        """-> a list of "empty" | "blurry" | "tissue", one per tile."""
        return self.classes_from_sums(self.sums(tiles))

    def classify_windows(self, image, positions, tile):
        """classify() for the tile x tile windows at `positions` [(y, x), ...] of one image; on the device one launch for
        all windows, without copies of them."""
        return self.classes_from_sums(self.window_sums(image, positions, tile))
