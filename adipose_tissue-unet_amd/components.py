"""Connected components of binary masks: labelling, component areas, small-object removal and per-component statistics.

The reference treats a mask as a set of objects in two places:

  remove_small_components(mask, min_px)   Segmentation/build_dataset.py:1122-1131, build_test_dataset.py:374 (flag
      --min-cc-px): cv2.connectedComponentsWithStats(connectivity=8), keep the components with area >= min_px.
  analyze_cell_characteristics            pre-post-processing_tools/analysis/morphology parameter_analysis/
      analyze_training_data.py:76-130: skimage measure.label of mask > 0.5, then num_cells, the areas of the regions of
      at least 10 px, and tissue_coverage (cell_statistics); their perimeter, circularity, aspect ratio and
      eccentricity (cell_shapes). skimage's regionprops is not a dependency: the measures are defined here, from
      integer sums per component (second-order moments and three counts of boundary-pixel configurations:
      shape_table / shape_table_np) turned into floats by one host function (region_shapes).

Labels are canonical: 0 for background, else 1 + the raster index y*W + x (within the pixel's own image) of the first
pixel of the component. That numbering does not depend on the algorithm, the batch or the run, so the device path
(csrc/components.hip: adp_cc_label / adp_cc_areas / adp_cc_filter / adp_cc_table / adp_cc_relabel / adp_cc_shape) and
the numpy path below (label_np / areas_np / filter_np / table_np / shape_table_np: hosts without a GPU, and the tests'
reference) agree bit for bit.
Connectivity 8 is cv2's connectivity=8 and skimage's 2-D default; 4 is scipy.ndimage.label's default.

cv2 and skimage are not dependencies, so parity with cv2.connectedComponentsWithStats and skimage.measure.label
themselves is unpinned; where scipy is installed the tests compare against scipy.ndimage.label.
"""
from __future__ import annotations

import numpy as np

SRC_U8, SRC_F32 = 0, 1
# region of the kernels' in-LDS labelling stage (include/adipose_hip.h ADP_CC_REGION_ROWS / _COLS): the GPU tests place
# their shapes around it
REGION_ROWS, REGION_COLS = 32, 64
# tile of the shape kernel, which reads a two-pixel halo around it (ADP_CC_SHAPE_TILE_ROWS / _COLS)
SHAPE_TILE_ROWS, SHAPE_TILE_COLS = 64, 128
MAX_PIXELS = 2 ** 31 - 2


# ---------------------------------------------------------------- numpy path
def _fg_np(mask, threshold=None):
    m = np.asarray(mask)
    if threshold is not None:
        return m > threshold
    if m.dtype.kind == "f":
        raise TypeError("a float mask needs a threshold")
    return m != 0


def _check_conn(connectivity):
    if connectivity not in (4, 8):
        raise ValueError("connectivity must be 4 or 8")


def _label2d_pure(fg, connectivity):
    """Canonical labels of one (H, W) bool map in plain numpy: every foreground pixel starts with 1 + its own index
    and takes the minimum over its neighbourhood inside the foreground (rows and columns by running minima over runs,
    the diagonals by shifted copies) until nothing changes."""
    H, W = fg.shape
    big = np.int64(H * W + 1)
    lab = np.where(fg, np.arange(1, H * W + 1, dtype=np.int64).reshape(H, W), big)

    def run_min(a, f, axis):
        # minimum over each run of foreground along `axis`: a forward and a backward sweep of doubling shifts
        a = a.copy()
        n = a.shape[axis]
        for rev in (False, True):
            step = 1
            conn = f.copy()   # conn[i]: pixels i - step + 1 .. i (or mirrored) are all foreground
            while step < n:
                src = [slice(None)] * 2
                dst = [slice(None)] * 2
                if not rev:
                    dst[axis], src[axis] = slice(step, None), slice(None, n - step)
                else:
                    dst[axis], src[axis] = slice(None, n - step), slice(step, None)
                dst, src = tuple(dst), tuple(src)
                ok = conn[dst] & conn[src]
                a[dst] = np.where(ok, np.minimum(a[dst], a[src]), a[dst])
                nc = np.zeros_like(conn)
                nc[dst] = ok
                conn = nc
                step *= 2
        return a

    while True:
        new = run_min(run_min(lab, fg, 1), fg, 0)
        if connectivity == 8:
            p = np.pad(new, 1, constant_values=big)
            d = np.minimum(np.minimum(p[:-2, :-2], p[:-2, 2:]), np.minimum(p[2:, :-2], p[2:, 2:]))
            new = np.where(fg, np.minimum(new, d), big)
        if np.array_equal(new, lab):
            break
        lab = new
    return np.where(fg, lab, 0).astype(np.int32)


def _label2d_scipy(fg, connectivity, ndi):
    st = np.ones((3, 3), int) if connectivity == 8 else None
    lab, k = ndi.label(fg, structure=st)
    if k == 0:
        return np.zeros(fg.shape, np.int32)
    flat = lab.ravel()
    idx = np.flatnonzero(flat)
    first = np.full(k + 1, flat.size, np.int64)
    np.minimum.at(first, flat[idx], idx)
    out = np.zeros(flat.size, np.int32)
    out[idx] = (first[flat[idx]] + 1).astype(np.int32)
    return out.reshape(fg.shape)


def _scipy_ndimage():
    try:
        import scipy.ndimage as ndi
        return ndi
    except Exception:
        return None


def label_np(mask, connectivity=8, threshold=None, force_pure=False):
    """(H, W) or (N, H, W) mask -> canonical int32 labels of the same shape. Foreground is non-zero, or > threshold
    where one is given. scipy.ndimage.label renumbered to "1 + first index" where scipy is importable, plain numpy
    otherwise (or with force_pure)."""
    _check_conn(connectivity)
    fg = _fg_np(mask, threshold)
    if fg.ndim not in (2, 3):
        raise ValueError("label_np takes an (H, W) or (N, H, W) mask")
    if fg.shape[-1] * fg.shape[-2] > MAX_PIXELS:
        raise ValueError("H * W is above 2^31 - 2")
    ndi = None if force_pure else _scipy_ndimage()
    one = (lambda f: _label2d_pure(f, connectivity)) if ndi is None else (lambda f: _label2d_scipy(f, connectivity, ndi))
    if fg.ndim == 2:
        return one(fg)
    return np.stack([one(f) for f in fg]) if len(fg) else np.zeros(fg.shape, np.int32)


def _as3(a):
    a = np.asarray(a)
    return (a[None], True) if a.ndim == 2 else (a, False)


def areas_np(labels):
    """Canonical labels -> int32 of the same shape: a component's pixel count at its first pixel, 0 elsewhere."""
    lab, squeeze = _as3(labels)
    N, H, W = lab.shape
    out = np.zeros((N, H * W), np.int32)
    for n in range(N):
        v = lab[n].ravel()
        out[n] = np.bincount(v[v > 0] - 1, minlength=H * W).astype(np.int32)
    out = out.reshape(N, H, W)
    return out[0] if squeeze else out


def filter_np(labels, area, min_px, dtype=np.uint8):
    """1 where the pixel's component has area >= min_px, else 0."""
    lab, squeeze = _as3(labels)
    ar, _ = _as3(area)
    N, H, W = lab.shape
    out = np.zeros((N, H, W), dtype)
    for n in range(N):
        a = ar[n].ravel()
        fg = lab[n] > 0
        keep = np.zeros((H, W), bool)
        keep[fg] = a[lab[n][fg] - 1] >= min_px
        out[n] = keep
    return out[0] if squeeze else out


def table_np(labels, max_rows):
    """Canonical labels -> (table (N, max_rows, 8) int64, counts (N,) int32): rows {first, area, x_min, y_min, x_max,
    y_max, sum_x, sum_y} in ascending `first`; components beyond max_rows dropped, rows past counts[n] zero."""
    lab, squeeze = _as3(labels)
    N, H, W = lab.shape
    table = np.zeros((N, max_rows, 8), np.int64)
    counts = np.zeros(N, np.int32)
    for n in range(N):
        v = lab[n].ravel().astype(np.int64)
        idx = np.flatnonzero(v)
        firsts = np.unique(v[idx]) - 1
        counts[n] = len(firsts)
        k = np.searchsorted(firsts, v[idx] - 1)
        keep = k < max_rows
        k, idx = k[keep], idx[keep]
        rows = min(len(firsts), max_rows)
        y, x = idx // W, idx % W
        t = table[n]
        t[:rows, 0] = firsts[:rows]
        t[:rows, 1] = np.bincount(k, minlength=rows)[:rows]
        for col, val, fn, init in ((2, x, np.minimum, W), (3, y, np.minimum, H), (4, x, np.maximum, -1), (5, y, np.maximum, -1)):
            acc = np.full(rows, init, np.int64)
            fn.at(acc, k, val)
            t[:rows, col] = acc
        t[:rows, 6] = _int_bincount(k, x, rows)
        t[:rows, 7] = _int_bincount(k, y, rows)
    return (table[0], counts[0]) if squeeze else (table, counts)


def _int_bincount(k, val, rows):
    acc = np.zeros(rows, np.int64)
    np.add.at(acc, k, val.astype(np.int64))
    return acc


# the perimeter codes counted by p_straight, p_diag and p_mixed, and what each contributes to the perimeter
PERIMETER_CODES = ((5, 7, 15, 17, 25, 27), (21, 33), (13, 23))
PERIMETER_WEIGHTS = (1.0, float(np.sqrt(2.0)), float((1.0 + np.sqrt(2.0)) / 2.0))


def _check_moment_bound(H, W):
    if H * W * (max(H, W) - 1) ** 2 >= 2 ** 63:
        raise ValueError("H * W * (max(H, W) - 1)^2 is 2^63 or more (the moment sums are int64)")


def shape_table_np(labels, max_rows):
    """Canonical labels -> (N, max_rows, 8) int64 (2-D labels: without N), rows {first, S_xx, S_yy, S_xy, p_straight,
    p_diag, p_mixed, border_px} in table_np's order and with its truncation. S_xx / S_yy / S_xy are the sums of x^2,
    y^2 and x*y over the component's pixels (x the column, y the row). A border pixel has an edge neighbour outside its
    component (another label, or outside the image); its code is 1 + 2 n4 + 10 nd, n4 / nd counting its edge / diagonal
    neighbours that are border pixels of the same component; p_straight, p_diag and p_mixed count the codes in
    PERIMETER_CODES, border_px all border pixels."""
    lab, squeeze = _as3(labels)
    N, H, W = lab.shape
    _check_moment_bound(H, W)
    out = np.zeros((N, max_rows, 8), np.int64)
    for n in range(N):
        L = lab[n].astype(np.int64)
        v = L.ravel()
        idx = np.flatnonzero(v)
        firsts = np.unique(v[idx]) - 1
        k = np.searchsorted(firsts, v[idx] - 1)
        keep = k < max_rows
        k, idx = k[keep], idx[keep]
        rows = min(len(firsts), max_rows)
        y, x = idx // W, idx % W
        P = np.pad(L, 1)   # label 0 outside the image
        border = (L != 0) & ((P[:-2, 1:-1] != L) | (P[2:, 1:-1] != L) | (P[1:-1, :-2] != L) | (P[1:-1, 2:] != L))
        B = np.pad(np.where(border, L, -1), 1, constant_values=-1)   # the label of a border pixel, else no label
        n4 = sum((B[dy:dy + H, dx:dx + W] == L).astype(np.int64) for dy, dx in ((0, 1), (2, 1), (1, 0), (1, 2)))
        nd = sum((B[dy:dy + H, dx:dx + W] == L).astype(np.int64) for dy, dx in ((0, 0), (0, 2), (2, 0), (2, 2)))
        code = np.where(border, 1 + 2 * n4 + 10 * nd, 0).ravel()[idx]
        t = out[n]
        t[:rows, 0] = firsts[:rows]
        t[:rows, 1] = _int_bincount(k, x * x, rows)
        t[:rows, 2] = _int_bincount(k, y * y, rows)
        t[:rows, 3] = _int_bincount(k, x * y, rows)
        for col, codes in enumerate(PERIMETER_CODES):
            t[:rows, 4 + col] = _int_bincount(k, np.isin(code, codes), rows)
        t[:rows, 7] = _int_bincount(k, code > 0, rows)
    return out[0] if squeeze else out


def region_shapes(table_rows, shape_rows):
    """The float measures of components from their integer rows: table_rows (..., 8) as table / table_np give them and
    shape_rows (..., 8) as shape_table / shape_table_np do, for the same components. A dict of float64 arrays of
    shape (...): area, perimeter, circularity, major_axis_length, minor_axis_length, aspect_ratio, eccentricity,
    centroid_x, centroid_y. Rows of area 0 (unused rows) give zeros.

      perimeter = p_straight + sqrt(2) p_diag + (1 + sqrt(2)) / 2 p_mixed
      circularity = 4 pi A / (P^2 + 1e-10), aspect_ratio = major / (minor + 1e-10)    (the reference's lines 113-114)
      a = (A S_xx - S_x^2) / A^2, b = (A S_yy - S_y^2) / A^2, c = (A S_xy - S_x S_y) / A^2     (central moments)
      d = sqrt(((a - b) / 2)^2 + c^2), l1 = (a + b) / 2 + d, l2 = max((a + b) / 2 - d, 0)
      major / minor axis = 4 sqrt(l1) / 4 sqrt(l2), eccentricity = sqrt(1 - l2 / l1) (0 where l1 == 0)

    The numerators A S_xx - S_x^2 and the like are formed in Python integers (A S_xx passes 2^63 for large
    components) and divided once; both paths go through this function, so their floats are the same."""
    t, s = np.asarray(table_rows, np.int64), np.asarray(shape_rows, np.int64)
    if t.shape != s.shape or t.shape[-1] != 8:
        raise ValueError("region_shapes takes table rows and shape rows of the same (..., 8) shape")
    lead = t.shape[:-1]
    t, s = t.reshape(-1, 8), s.reshape(-1, 8)
    K = t.shape[0]
    out = {k: np.zeros(K, np.float64) for k in ("area", "perimeter", "circularity", "major_axis_length",
                                                "minor_axis_length", "aspect_ratio", "eccentricity", "centroid_x",
                                                "centroid_y")}
    a, b, c = np.zeros(K, np.float64), np.zeros(K, np.float64), np.zeros(K, np.float64)
    for i in range(K):
        A, Sx, Sy = int(t[i, 1]), int(t[i, 6]), int(t[i, 7])
        if A <= 0:
            continue
        Sxx, Syy, Sxy = int(s[i, 1]), int(s[i, 2]), int(s[i, 3])
        a[i] = (A * Sxx - Sx * Sx) / (A * A)   # int / int: one correctly rounded division
        b[i] = (A * Syy - Sy * Sy) / (A * A)
        c[i] = (A * Sxy - Sx * Sy) / (A * A)
        out["centroid_x"][i], out["centroid_y"][i] = Sx / A, Sy / A
    area = t[:, 1].astype(np.float64)
    live = area > 0
    per = PERIMETER_WEIGHTS[0] * s[:, 4] + PERIMETER_WEIGHTS[1] * s[:, 5] + PERIMETER_WEIGHTS[2] * s[:, 6]
    per = np.where(live, per, 0.0)
    d = np.sqrt(((a - b) / 2) ** 2 + c ** 2)
    l1 = (a + b) / 2 + d
    l2 = np.maximum((a + b) / 2 - d, 0.0)
    major, minor = 4 * np.sqrt(l1), 4 * np.sqrt(l2)
    ecc = np.zeros(K, np.float64)
    nz = l1 > 0
    ecc[nz] = np.sqrt(1 - l2[nz] / l1[nz])   # l2 <= l1, as d >= 0
    out["area"], out["perimeter"] = np.where(live, area, 0.0), per
    out["circularity"] = 4 * np.pi * out["area"] / (per ** 2 + 1e-10)
    out["major_axis_length"], out["minor_axis_length"] = major, minor
    out["aspect_ratio"] = major / (minor + 1e-10)
    out["eccentricity"] = ecc
    return {k: v.reshape(lead) for k, v in out.items()}


def relabel_np(labels):
    """Canonical labels -> dense labels 1..K in raster order of first pixel (cv2's numbering), int32."""
    lab, squeeze = _as3(labels)
    out = np.zeros(lab.shape, np.int32)
    for n in range(lab.shape[0]):
        v = lab[n]
        firsts = np.unique(v[v > 0])
        out[n][v > 0] = np.searchsorted(firsts, v[v > 0]) + 1
    return out[0] if squeeze else out


# ---------------------------------------------------------------- device path
def _is_tensor(t):
    return hasattr(t, "is_cuda")


def _gpu():
    import torch
    return torch.cuda.is_available()


def _nhw(t):
    if t.dim() == 2:
        return 1, int(t.shape[0]), int(t.shape[1])
    if t.dim() == 3:
        return int(t.shape[0]), int(t.shape[1]), int(t.shape[2])
    raise ValueError("connected components take an (H, W) or (N, H, W) map")


def _to_device(a):
    """A host array or tensor -> a tensor on the current device; a device tensor as it is."""
    import torch
    if _is_tensor(a):
        return a if a.is_cuda else a.to(torch.device("cuda", torch.cuda.current_device()))
    a = np.ascontiguousarray(a)
    if a.dtype == np.bool_:
        a = a.view(np.uint8)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(torch.device("cuda", torch.cuda.current_device()))


def label(mask, connectivity=8, threshold=None):
    """Canonical labels on the device: (H, W) or (N, H, W) uint8 / bool (foreground non-zero), or float32 together with
    `threshold` (foreground > threshold, fused into the load) -> int32 device tensor of the same shape. A host array
    is uploaded. Runs on the current stream."""
    import torch

    from ._lib import call, ptr, stream_ptr
    _check_conn(connectivity)
    m = _to_device(mask)
    if m.dtype == torch.bool:
        m = m.view(torch.uint8)
    if m.dtype == torch.uint8:
        if threshold is not None:
            m, kind = m.to(torch.float32), SRC_F32
        else:
            kind = SRC_U8
    elif m.dtype == torch.float32:
        if threshold is None:
            raise TypeError("a float32 mask needs a threshold")
        kind = SRC_F32
    else:
        raise TypeError("label takes a uint8 / bool mask, or float32 with a threshold")
    m = m.contiguous()
    N, H, W = _nhw(m)
    if N == 0:
        return torch.zeros(m.shape, dtype=torch.int32, device=m.device)
    out = torch.empty(m.shape, dtype=torch.int32, device=m.device)
    with torch.cuda.device(m.device):
        call("adp_cc_label", N, H, W, ptr(m), kind, float(threshold if threshold is not None else 0.0),
             int(connectivity), ptr(out), stream_ptr())
    return out


def _labels_arg(labels):
    import torch
    if not (_is_tensor(labels) and labels.is_cuda and labels.dtype == torch.int32):
        raise TypeError("expected the int32 device tensor that label() returns")
    return labels.contiguous()


def areas(labels):
    """Device labels -> int32 device tensor: a component's pixel count at its first pixel, 0 elsewhere."""
    import torch

    from ._lib import call, ptr, stream_ptr
    lab = _labels_arg(labels)
    N, H, W = _nhw(lab)
    out = torch.empty_like(lab)
    with torch.cuda.device(lab.device):
        call("adp_cc_areas", N, H, W, ptr(lab), ptr(out), stream_ptr())
    return out


def filter_small(labels, area, min_px, dtype=None):
    """1 where the pixel's component has area >= min_px, else 0: uint8 (default) or float32 device tensor."""
    import torch

    from ._lib import call, ptr, stream_ptr
    lab, ar = _labels_arg(labels), _labels_arg(area)
    if ar.shape != lab.shape:
        raise ValueError("labels and area differ in shape")
    dtype = dtype or torch.uint8
    if dtype not in (torch.uint8, torch.float32):
        raise TypeError("filter_small writes uint8 or float32")
    N, H, W = _nhw(lab)
    out = torch.empty(lab.shape, dtype=dtype, device=lab.device)
    mp = int(max(min(int(min_px), 2 ** 31 - 1), -(2 ** 31)))
    with torch.cuda.device(lab.device):
        call("adp_cc_filter", N, H, W, ptr(lab), ptr(ar), mp, ptr(out) if dtype == torch.uint8 else None,
             ptr(out) if dtype == torch.float32 else None, stream_ptr())
    return out


def table(labels, max_rows):
    """Device labels -> (table (N, max_rows, 8) int64, counts (N,) int32) device tensors (2-D labels: without N)."""
    import torch

    from ._lib import call, ptr, stream_ptr
    lab = _labels_arg(labels)
    N, H, W = _nhw(lab)
    max_rows = int(max_rows)
    tab = torch.empty((N, max_rows, 8), dtype=torch.int64, device=lab.device)
    counts = torch.empty((N,), dtype=torch.int32, device=lab.device)
    with torch.cuda.device(lab.device):
        call("adp_cc_table", N, H, W, ptr(lab), max_rows, ptr(tab) if max_rows > 0 else None, ptr(counts), stream_ptr())
    return (tab[0], counts[0]) if lab.dim() == 2 else (tab, counts)


def shape_table(labels, max_rows):
    """Device labels -> (N, max_rows, 8) int64 device tensor (2-D labels: without N): shape_table_np's rows."""
    import torch

    from ._lib import call, ptr, stream_ptr
    lab = _labels_arg(labels)
    N, H, W = _nhw(lab)
    _check_moment_bound(H, W)
    max_rows = int(max_rows)
    out = torch.empty((N, max_rows, 8), dtype=torch.int64, device=lab.device)
    with torch.cuda.device(lab.device):
        call("adp_cc_shape", N, H, W, ptr(lab), max_rows, ptr(out) if max_rows > 0 else None, stream_ptr())
    return out[0] if lab.dim() == 2 else out


def relabel(labels):
    """Device labels -> dense labels 1..K in raster order of first pixel (cv2's numbering), int32 device tensor."""
    import torch

    from ._lib import call, ptr, stream_ptr
    lab = _labels_arg(labels)
    N, H, W = _nhw(lab)
    out = torch.empty_like(lab)
    with torch.cuda.device(lab.device):
        call("adp_cc_relabel", N, H, W, ptr(lab), ptr(out), stream_ptr())
    return out


# ---------------------------------------------------------------- the reference's surface
def _on_device(mask):
    """Whether `mask` is processed on the device: a device tensor always, a host input where there is a GPU."""
    if _is_tensor(mask) and mask.is_cuda:
        return True
    return _gpu()


def remove_small_components(mask, min_px, connectivity=8):
    """The reference's remove_small_components (build_dataset.py:1122-1131): the components of `mask` (non-zero pixels;
    connectivity 8 as the reference's cv2 call) with at least `min_px` pixels, as 0 / 1 in the input's dtype and
    container: numpy in, numpy out; tensor in, tensor out on the same device. min_px <= 0 returns `mask` itself."""
    if min_px <= 0:
        return mask
    _check_conn(connectivity)
    if not _is_tensor(mask):
        mask = np.asarray(mask)
    if not _on_device(mask):
        m = mask.numpy() if _is_tensor(mask) else mask
        lab = label_np(m != 0, connectivity)
        out = filter_np(lab, areas_np(lab), min_px, m.dtype)
        if _is_tensor(mask):
            import torch
            return torch.from_numpy(out)
        return out
    import torch
    src = _to_device(mask)
    if src.dtype in (torch.uint8, torch.bool):
        lab = label(src, connectivity)
    elif src.dtype == torch.float32:
        # non-zero of a float mask: |x| > 0 (a negative value is foreground for the reference's astype(uint8) only
        # where it wraps to non-zero; masks are 0 / 1)
        lab = label(src.abs(), connectivity, threshold=0.0)
    else:
        lab = label(src != 0, connectivity)
    ar = areas(lab)
    if src.dtype == torch.float32:
        out = filter_small(lab, ar, min_px, torch.float32)
    else:
        out = filter_small(lab, ar, min_px, torch.uint8)
        if src.dtype != torch.uint8:
            out = out.to(src.dtype)
    if _is_tensor(mask):
        return out if mask.is_cuda else out.cpu()
    return out.cpu().numpy().astype(mask.dtype, copy=False)


def _stats_from_table(tab, background):
    """cv2-shaped (stats (K+1, 5) int32 {left, top, width, height, area}, centroids (K+1, 2) float64 (x, y)) from the K
    table rows of one image and the background's row (None for an empty background: zeros)."""
    K = tab.shape[0]
    rows = np.zeros((K + 1, 8), np.int64)
    rows[1:] = tab
    if background is not None:
        rows[0] = background
    stats = np.zeros((K + 1, 5), np.int32)
    cent = np.zeros((K + 1, 2), np.float64)
    live = rows[:, 1] > 0
    stats[:, 0], stats[:, 1], stats[:, 4] = rows[:, 2], rows[:, 3], rows[:, 1]
    stats[live, 2] = (rows[:, 4] - rows[:, 2] + 1)[live]
    stats[live, 3] = (rows[:, 5] - rows[:, 3] + 1)[live]
    cent[live, 0] = rows[live, 6] / rows[live, 1]
    cent[live, 1] = rows[live, 7] / rows[live, 1]
    return stats, cent


def _background_row(bg):
    """The table row {0, area, x_min, y_min, x_max, y_max, sum_x, sum_y} of the background pixels of a bool map (numpy
    or device tensor), or None when there are none."""
    if _is_tensor(bg):
        n = int(bg.sum().item())
        if n == 0:
            return None
        yy, xx = bg.nonzero(as_tuple=True)
        vals = [xx.min(), yy.min(), xx.max(), yy.max(), xx.sum(), yy.sum()]
        return np.array([0, n] + [int(v.item()) for v in vals], np.int64)
    n = int(bg.sum())
    if n == 0:
        return None
    yy, xx = np.nonzero(bg)
    return np.array([0, n, xx.min(), yy.min(), xx.max(), yy.max(), xx.sum(), yy.sum()], np.int64)


def connected_components_with_stats(mask, connectivity=8):
    """cv2.connectedComponentsWithStats for one (H, W) mask (non-zero = foreground): (num_labels, labels, stats,
    centroids). Labels are dense, 0..K, numbered in raster order of each component's first pixel; stats (K+1, 5) int32
    {left, top, width, height, area}; centroids (K+1, 2) float64 (x, y); row 0 is the background with its real box and
    area (zeros for an all-foreground mask, where cv2 gives a degenerate box and a NaN centroid). labels comes back in
    the mask's container (numpy array, host or device tensor); stats and centroids are numpy. On the device the table
    call is sized with a first guess of 4096 rows and made once more when `counts` says there are more; the dense
    labels are a gather through the same ranks (adp_cc_relabel)."""
    _check_conn(connectivity)
    is_t = _is_tensor(mask)
    if len(tuple(mask.shape)) != 2:
        raise ValueError("connected_components_with_stats takes one (H, W) mask")
    if not _on_device(mask):
        m = mask.numpy() if is_t else np.asarray(mask)
        fg = m != 0
        lab = label_np(fg, connectivity)
        k = int(np.count_nonzero(areas_np(lab)))
        tab, _ = table_np(lab, k)
        dense = relabel_np(lab)
        background = _background_row(~fg)
        if is_t:
            import torch
            dense = torch.from_numpy(dense)
    else:
        src = _to_device(mask)
        fg = src != 0
        lab = label(fg, connectivity)
        guess = 4096
        tab_d, cnt = table(lab, guess)
        k = int(cnt.item())
        if k > guess:
            tab_d, cnt = table(lab, k)
        tab = tab_d[:k].cpu().numpy()
        dense = relabel(lab)
        background = _background_row(~fg)
        if not (is_t and mask.is_cuda):
            dense = dense.cpu() if is_t else dense.cpu().numpy()
    stats, cent = _stats_from_table(tab[:k], background)
    return k + 1, dense, stats, cent


def cell_statistics(mask, min_area=10, threshold=0.5):
    """The per-sample numbers of the reference's analyze_cell_characteristics for one (H, W) mask: a dict with
      num_cells         the 8-connected components of mask > threshold with at least min_area pixels (the reference
                        skips regions with area < 10)
      areas             their areas, a list of floats in raster order of first pixel
      tissue_coverage   the share of pixels above the threshold (all of them, small regions included)
    An integer or bool mask is compared as the reference's float mask would be (1 > 0.5). The reference's perimeter,
    circularity, aspect ratio and eccentricity of the same cells are cell_shapes' part."""
    shape = tuple(mask.shape)
    if len(shape) != 2:
        raise ValueError("cell_statistics takes one (H, W) mask")
    H, W = shape
    if not _on_device(mask):
        m = mask.numpy() if _is_tensor(mask) else np.asarray(mask)
        fg = m > threshold
        lab = label_np(fg, 8)
        a = areas_np(lab).ravel()
        a = a[a > 0]
        total = int(fg.sum())
    else:
        import torch
        src = _to_device(mask)
        if src.dtype != torch.float32:
            src = src.to(torch.float32)
        lab = label(src, 8, threshold=float(threshold))
        ar = areas(lab).flatten()
        a = ar[ar > 0].cpu().numpy()   # raster order of first pixel
        total = int(a.sum())
    kept = a[a >= min_area]
    return {"num_cells": int(len(kept)), "areas": [float(v) for v in kept], "tissue_coverage": float(total / (H * W))}


def cell_shapes(mask, min_area=10, threshold=0.5):
    """The rest of analyze_cell_characteristics for one (H, W) mask: for the 8-connected components of mask > threshold
    with at least min_area pixels, in raster order of first pixel, a dict with num_cells, areas, perimeters,
    circularities, aspect_ratios, eccentricities (lists of floats, one entry per cell; region_shapes has the formulas)
    and tissue_coverage (the share of pixels above the threshold). num_cells, areas and tissue_coverage are
    cell_statistics' (stats_from_shapes). On the device: labels with the fused threshold, the table sized by a first
    guess of 4096 rows and made once more when there are more components, the shape rows for the same row count, and
    one copy of the K rows of both to the host."""
    shape = tuple(mask.shape)
    if len(shape) != 2:
        raise ValueError("cell_shapes takes one (H, W) mask")
    H, W = shape
    if not _on_device(mask):
        m = mask.numpy() if _is_tensor(mask) else np.asarray(mask)
        lab = label_np(m > threshold, 8)
        k = int(np.count_nonzero(areas_np(lab)))
        tab, _ = table_np(lab, k)
        shp = shape_table_np(lab, k)
    else:
        import torch
        src = _to_device(mask)
        if src.dtype != torch.float32:
            src = src.to(torch.float32)
        lab = label(src, 8, threshold=float(threshold))
        rows = 4096
        tab_d, cnt = table(lab, rows)
        k = int(cnt.item())
        if k > rows:
            rows = k
            tab_d, cnt = table(lab, rows)
        both = torch.cat((tab_d[:k], shape_table(lab, rows)[:k]), dim=1).cpu().numpy()
        tab, shp = both[:, :8], both[:, 8:]
    r = region_shapes(tab, shp)
    total = int(tab[:, 1].sum())
    keep = r["area"] >= min_area

    def kept(name):
        return [float(v) for v in r[name][keep]]

    return {"num_cells": int(keep.sum()), "areas": kept("area"), "perimeters": kept("perimeter"),
            "circularities": kept("circularity"), "aspect_ratios": kept("aspect_ratio"),
            "eccentricities": kept("eccentricity"), "tissue_coverage": float(total / (H * W))}


def stats_from_shapes(shapes):
    """cell_statistics' dict for the same mask and arguments, from cell_shapes' (a run that wants both labels once)."""
    return {k: shapes[k] for k in ("num_cells", "areas", "tissue_coverage")}


CELL_SHAPES_HEADER = ["name", "num_cells", "mean_perimeter", "median_perimeter", "mean_circularity", "median_circularity",
                      "mean_aspect_ratio", "median_aspect_ratio", "mean_eccentricity", "median_eccentricity"]


def cell_shapes_row(name, shapes=None):
    """One row of cell_shapes.csv from cell_shapes' dict (None: the all-zero row of a tile that was not processed)."""
    if not shapes or not shapes["num_cells"]:
        return [name, 0] + ["0.0000"] * 8
    row = [name, int(shapes["num_cells"])]
    for key in ("perimeters", "circularities", "aspect_ratios", "eccentricities"):
        v = np.asarray(shapes[key], np.float64)
        row += [f"{v.mean():.4f}", f"{np.median(v):.4f}"]
    return row


CELL_STATS_HEADER = ["name", "num_cells", "mean_area", "median_area", "min_area", "max_area", "tissue_coverage"]


def cell_stats_row(name, stats=None):
    """One row of cell_stats.csv from cell_statistics' dict (None: the all-zero row of a tile that was not processed)."""
    a = np.asarray(stats["areas"], np.float64) if stats and stats["areas"] else None
    if a is None:
        return [name, 0, "0.000", "0.000", "0.000", "0.000", f"{(stats['tissue_coverage'] if stats else 0.0):.6f}"]
    return [name, int(stats["num_cells"]), f"{a.mean():.3f}", f"{np.median(a):.3f}", f"{a.min():.3f}", f"{a.max():.3f}",
            f"{stats['tissue_coverage']:.6f}"]
