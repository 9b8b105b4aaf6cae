"""Connected components on the GPU (csrc/components.hip) against the numpy path of adipose_amd.components.

Labels are canonical (1 + raster index of the component's first pixel) and every derived quantity is an integer, so
every comparison is array_equal: there is no tolerance. The numpy path itself is pinned against scipy.ndimage.label in
tests/test_components.py; cv2 and skimage are not installed, so parity with them is unpinned.

The labelling kernel's first stage works on regions of R x C pixels; the shapes below sit on, just past and well
past one region, and the structure cases are drawn to cross the regions' borders.
"""
import csv
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def CC():
    from adipose_amd import components
    return components


R, C = 32, 64   # the region of the kernel's first stage (asserted against the module below)

SHAPES = [(1, 1, 1), (1, 2, 2), (3, 7, 9), (2, 64, 96), (1, 257, 131),
          (1, R, C),                # exactly one region
          (1, R + 1, C + 1),        # one region plus one row and one column
          (1, 3 * R, 2 * C),
          (5, R + 1, 2 * C - 1)]


def test_region_constants():
    assert (CC().REGION_ROWS, CC().REGION_COLS) == (R, C)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def random_case(shape, connectivity):
    """A seeded f32 map with exact 0.5 values (background at thr = 0.5) and its reference, computed once."""
    rng = np.random.default_rng(shape[0] * 1000003 + shape[1] * 1009 + shape[2] * 10 + connectivity)
    dens = rng.choice([0.1, 0.45, 0.6, 0.9], size=shape[0])
    p = rng.random(shape).astype(np.float32)
    prob = np.where(p < dens[:, None, None], 0.5 + 0.5 * rng.random(shape).astype(np.float32) + 1e-3, 0.5 * p).astype(np.float32)
    prob[rng.random(shape) < 0.1] = 0.5
    fg = prob > 0.5
    assert (prob == 0.5).any() or prob.size < 8
    lab = CC().label_np(fg, connectivity)
    area = CC().areas_np(lab)
    return prob, fg.astype(np.uint8), lab, area


def check_all(mask_u8, lab_want, connectivity, prob=None):
    """labels (both input kinds), areas, filter (both outputs) and table of one input against the numpy path."""
    cc = CC()
    area_want = cc.areas_np(lab_want)
    lab = cc.label(dev(mask_u8), connectivity)
    assert lab.dtype == torch.int32 and np.array_equal(lab.cpu().numpy(), lab_want)
    if prob is not None:
        assert np.array_equal(cc.label(dev(prob), connectivity, threshold=0.5).cpu().numpy(), lab_want)
    area = cc.areas(lab)
    assert np.array_equal(area.cpu().numpy(), area_want)
    for min_px in (1, 2, 5, 40):
        want = cc.filter_np(lab_want, area_want, min_px)
        assert np.array_equal(cc.filter_small(lab, area, min_px).cpu().numpy(), want)
        f = cc.filter_small(lab, area, min_px, torch.float32)
        assert f.dtype == torch.float32 and np.array_equal(f.cpu().numpy(), want.astype(np.float32))
    kmax = int((area_want.reshape(area_want.shape[0], -1) > 0).sum(axis=1).max())
    for rows in sorted({kmax + 3, max(kmax // 2, 1)}):
        tab, cnt = cc.table(lab, rows)
        tw, cw = cc.table_np(lab_want, rows)
        assert np.array_equal(cnt.cpu().numpy(), cw) and np.array_equal(tab.cpu().numpy(), tw)
    assert np.array_equal(cc.relabel(lab).cpu().numpy(), cc.relabel_np(lab_want))
    return lab


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_random_maps(shape, connectivity):
    prob, u8, lab, _ = random_case(shape, connectivity)
    check_all(u8, lab, connectivity, prob)


# ---------------------------------------------------------------- structures across region borders
H3, W2 = 3 * R, 2 * C


def serpentine(h, w):
    """A one-pixel-wide path filling the map: full even rows, joined at alternating ends."""
    m = np.zeros((h, w), np.uint8)
    m[0::2] = 1
    m[1::4, -1] = 1
    m[3::4, 0] = 1
    return m


def u_shape(h, w):
    m = np.zeros((h, w), np.uint8)
    m[:, 1] = 1
    m[:, w - 2] = 1
    m[h - 1, 1:w - 1] = 1
    return m


def comb(h, w):
    """Teeth two pixels apart that cross every horizontal border, joined by a spine in the last row."""
    m = np.zeros((h, w), np.uint8)
    m[:, 0::2] = 1
    m[h - 1] = 1
    return m


def diagonal(h, w):
    """A line through the regions' corners: (k, 2k) would miss them, so it runs at slope R : C."""
    m = np.zeros((h, w), np.uint8)
    k = np.arange(min(h, w))
    m[k, k] = 1                           # crosses (R, R): inside a region
    m2 = np.zeros((h, w), np.uint8)
    for j in range(min(h // R, w // C) + 1):   # staircase with single diagonal steps exactly at the corners (jR, jC)
        y0, x0 = j * R, j * C
        if y0 < h and x0 < w:
            m2[y0, x0:min(x0 + C, w)] = 1             # along the top row of region (j, j)
            ys = np.arange(y0, min(y0 + R, h))
            m2[ys, min(x0 + C, w) - 1] = 1            # down its last column to (y0 + R - 1, x0 + C - 1)
    return m, m2


def checkerboard(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy + xx) % 2 == 0).astype(np.uint8)


def structures():
    d1, d2 = diagonal(H3, W2)
    return {"serpentine": serpentine(H3, W2), "u": u_shape(H3, W2), "comb": comb(H3, W2), "diagonal": d1,
            "corner_staircase": d2, "checkerboard": checkerboard(H3, W2), "ones": np.ones((H3, W2), np.uint8),
            "zeros": np.zeros((H3, W2), np.uint8)}


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", sorted(structures()))
def test_structures(name, connectivity):
    m = structures()[name][None]
    want = CC().label_np(m, connectivity)
    lab = check_all(m, want, connectivity, m.astype(np.float32))
    k = len(np.unique(want[want > 0]))
    if name in ("serpentine", "u", "comb", "ones"):
        assert k == 1 and int(lab.max()) == int(np.flatnonzero(m)[0]) + 1
    if name == "checkerboard":
        assert k == (1 if connectivity == 8 else (H3 * W2 + 1) // 2)
    if name == "corner_staircase":   # its two stairs meet only through the corner neighbour at (R, C)
        assert k == (1 if connectivity == 8 else 2)
    if name == "diagonal":
        assert k == (1 if connectivity == 8 else min(H3, W2))
    if name == "zeros":
        assert k == 0


def adipocyte_mask(seed, h, w):
    """synthetic_tile's mask (ellipses: the cells), cropped to h x w."""
    from adipose_amd.data import synthetic_tile
    _, mask = synthetic_tile(np.random.default_rng(seed), size=max(h, w), channels=1)
    return (mask[:h, :w] > 0.5).astype(np.uint8)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_adipocyte_mask(connectivity):
    m = adipocyte_mask(3, 512, 768)[None]
    inv = (1 - m).astype(np.uint8)   # the membranes and the background: one large component with holes
    for x in (m, inv):
        assert x.any() and not x.all()
        check_all(x, CC().label_np(x, connectivity), connectivity)


def test_independent_of_batching_and_run():
    prob, u8, lab, _ = random_case((5, R + 1, 2 * C - 1), 8)
    d = dev(u8)
    one = CC().label(d, 8)
    assert one.cpu().numpy().tobytes() == CC().label(d, 8).cpu().numpy().tobytes()
    for n in range(5):
        alone = CC().label(d[n].contiguous(), 8)
        assert alone.shape == (R + 1, 2 * C - 1) and torch.equal(alone, one[n])
        assert torch.equal(CC().areas(alone), CC().areas(one)[n])
    # bool and host inputs go the same way
    assert torch.equal(CC().label(d.bool(), 8), one)
    assert torch.equal(CC().label(u8, 8), one)


def test_table_rows_limit():
    m = checkerboard(9, 11)[None]
    lab = CC().label(dev(m), 4)
    K = (9 * 11 + 1) // 2
    full, cfull = CC().table(lab, K)
    assert int(cfull[0]) == K
    small, cs = CC().table(lab, 7)
    assert int(cs[0]) == K and torch.equal(small[0], full[0, :7])
    big, cb = CC().table(lab, K + 9)
    assert int(cb[0]) == K and torch.equal(big[0, :K], full[0]) and not big[0, K:].any()
    none, c0 = CC().table(lab, 0)
    assert int(c0[0]) == K and none.shape == (1, 0, 8)
    # a row: {first, area, x_min, y_min, x_max, y_max, sum_x, sum_y} of single pixels
    r = full[0, 3].cpu().numpy()
    assert r.tolist() == [6, 1, 6, 0, 6, 0, 6, 0]


def test_argument_errors():
    from adipose_amd import _lib
    L = _lib.lib()
    src = torch.ones((2, 3), dtype=torch.uint8, device="cuda")
    lab = torch.full((2, 3), -7, dtype=torch.int32, device="cuda")
    area = torch.full((2, 3), -7, dtype=torch.int32, device="cuda")
    out = torch.full((2, 3), 9, dtype=torch.uint8, device="cuda")
    cnt = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    tab = torch.full((1, 2, 8), -7, dtype=torch.int64, device="cuda")
    s, p = _lib.stream_ptr(), _lib.ptr

    def fails(rc):
        return rc != 0 and len(L.adp_last_error()) > 0

    assert fails(L.adp_cc_label(1, 2, 3, None, 0, 0.0, 8, p(lab), s))
    assert fails(L.adp_cc_label(1, 2, 3, p(src), 0, 0.0, 8, None, s))
    assert fails(L.adp_cc_label(1, 2, 3, p(src), 0, 0.0, 6, p(lab), s))
    assert b"connectivity" in L.adp_last_error()
    assert fails(L.adp_cc_label(0, 2, 3, p(src), 0, 0.0, 8, p(lab), s))
    assert fails(L.adp_cc_label(1, 0, 3, p(src), 0, 0.0, 8, p(lab), s))
    assert fails(L.adp_cc_label(1, 2, 0, p(src), 0, 0.0, 8, p(lab), s))
    assert fails(L.adp_cc_label(1, 2, 3, p(src), 7, 0.0, 8, p(lab), s))
    # H * W = 2^31 - 1 is one too many (sizes only: no such buffer exists)
    assert fails(L.adp_cc_label(1, 1, 2 ** 31 - 1, p(src), 0, 0.0, 8, p(lab), s))
    assert fails(L.adp_cc_label(1, 65536, 32768, p(src), 0, 0.0, 8, p(lab), s))
    assert b"2^31" in L.adp_last_error()
    assert fails(L.adp_cc_areas(1, 2, 3, None, p(area), s)) and fails(L.adp_cc_areas(1, 2, 3, p(lab), None, s))
    assert fails(L.adp_cc_areas(0, 2, 3, p(lab), p(area), s)) and fails(L.adp_cc_areas(1, 65536, 32768, p(lab), p(area), s))
    assert fails(L.adp_cc_filter(1, 2, 3, p(lab), p(area), 1, None, None, s))
    assert fails(L.adp_cc_filter(1, 2, 3, None, p(area), 1, p(out), None, s))
    assert fails(L.adp_cc_filter(0, 2, 3, p(lab), p(area), 1, p(out), None, s))
    assert fails(L.adp_cc_table(1, 2, 3, p(lab), 2, None, p(cnt), s))
    assert fails(L.adp_cc_table(1, 2, 3, p(lab), 2, p(tab), None, s))
    assert fails(L.adp_cc_table(1, 2, 3, p(lab), -1, p(tab), p(cnt), s))
    assert fails(L.adp_cc_table(1, 65536, 32768, p(lab), 2, p(tab), p(cnt), s))
    assert fails(L.adp_cc_relabel(1, 2, 3, p(lab), None, s)) and fails(L.adp_cc_relabel(0, 2, 3, p(lab), p(area), s))
    torch.cuda.synchronize()
    for t, v in ((lab, -7), (area, -7), (out, 9), (cnt, -7), (tab, -7)):
        assert (t == v).all()   # nothing was launched
    with pytest.raises(_lib.AdpError):
        _lib.call("adp_cc_label", 1, 2, 3, p(src), 0, 0.0, 5, p(lab), s)
    with pytest.raises(ValueError):
        CC().label(src, 6)
    with pytest.raises(TypeError):
        CC().label(src.float())   # a float map needs its threshold
    assert L.adp_cc_label(1, 2, 3, p(src), 0, 0.0, 8, p(lab), s) == 0
    assert (lab == 1).all()


# ---------------------------------------------------------------- the reference's surface on the device
def test_remove_small_components_and_stats():
    cc = CC()
    m = adipocyte_mask(5, 200, 300)
    m[::7, ::5] |= 1   # specks
    lab = cc.label_np(m, 8)
    want = cc.filter_np(lab, cc.areas_np(lab), 20)
    assert 0 < want.sum() < m.sum()
    d = dev(m)
    assert cc.remove_small_components(d, 0) is d
    got = cc.remove_small_components(d, 20)
    assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    got = cc.remove_small_components(m, 20)   # numpy in, numpy out, through the device where there is one
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want)
    gf = cc.remove_small_components(d.float(), 20)
    assert gf.dtype == torch.float32 and np.array_equal(gf.cpu().numpy(), want.astype(np.float32))
    gb = cc.remove_small_components(d.bool(), 20)
    assert gb.dtype == torch.bool and np.array_equal(gb.cpu().numpy(), want.astype(bool))
    # cv2-shaped statistics: the device's equal the numpy path's
    n, dense, stats, cent = cc.connected_components_with_stats(d)
    tab, k = cc.table_np(lab, 10 ** 6)
    assert n == k + 1 and dense.is_cuda and np.array_equal(dense.cpu().numpy(), cc.relabel_np(lab))
    assert stats.shape == (n, 5) and stats.dtype == np.int32 and stats[:, 4].sum() == m.size
    assert np.array_equal(stats[1:, 4], tab[:k, 1]) and np.array_equal(stats[1:, 0], tab[:k, 2])
    assert np.array_equal(stats[1:, 2], tab[:k, 4] - tab[:k, 2] + 1) and np.array_equal(stats[1:, 3], tab[:k, 5] - tab[:k, 3] + 1)
    assert np.array_equal(cent[1:, 0], tab[:k, 6] / tab[:k, 1]) and np.array_equal(cent[1:, 1], tab[:k, 7] / tab[:k, 1])
    yy, xx = np.nonzero(m == 0)
    assert stats[0].tolist() == [xx.min(), yy.min(), xx.max() - xx.min() + 1, yy.max() - yy.min() + 1, len(yy)]
    # more components than the first guess of rows: one more call
    board = checkerboard(100, 100)
    n2, dense2, stats2, _ = cc.connected_components_with_stats(dev(board), 4)
    assert n2 == 5001 and (stats2[1:, 4] == 1).all() and int(dense2.max()) == 5000
    # cell statistics
    st = cc.cell_statistics(d.float(), min_area=10, threshold=0.5)
    a = cc.areas_np(lab).ravel()
    a = a[a > 0]
    assert st == {"num_cells": int((a >= 10).sum()), "areas": [float(v) for v in a[a >= 10]],
                  "tissue_coverage": float(m.sum() / m.size)}


# ---------------------------------------------------------------- CLI and whole-slide reconstruction
def cell_tile(seed, size=64):
    """A gray-ish RGB tile with a few dark and bright blobs: the seeded network says something on it."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:size, 0:size]
    g = np.full((size, size), 150.0)
    for _ in range(6):
        cy, cx, r = rng.uniform(0, size), rng.uniform(0, size), rng.uniform(4, 12)
        g[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = rng.choice([60.0, 235.0])
    g = np.clip(g + rng.normal(0, 12, g.shape), 0, 255).astype(np.uint8)
    return np.stack([g, g, g], axis=-1)


def read_cell_stats(path):
    with open(path) as f:
        return list(csv.reader(f))


def test_cli_min_cc_px_and_cell_stats(tmp_path):
    from PIL import Image

    from adipose_amd.checkpoint import save_weights
    from cli.segmentation_inference import main
    from oracle import torch_ref as TR
    cc = CC()
    (tmp_path / "img").mkdir()
    for name, seed in (("a", 61), ("b", 62)):
        Image.fromarray(cell_tile(seed)).save(tmp_path / "img" / f"{name}.png")
    (tmp_path / "ck").mkdir()
    save_weights(None, tmp_path / "ck" / "phase2_best.weights.h5",
                 weights=TR.adipose_v3_keras_weights(seed=5, deep_supervision=False))
    (tmp_path / "ck" / "normalization_stats.json").write_text('{"mean": 120.0, "std": 40.0}')
    base = ["--images-dir", str(tmp_path / "img"), "--weights", str(tmp_path / "ck"), "--tile", "64"]
    masks = {}
    for run, extra in (("off", []), ("stats", ["--cell-stats", "--cell-min-area", "4"]),
                       ("on", ["--min-cc-px", "12", "--cell-stats", "--cell-min-area", "4"])):
        assert main(base + ["--output-dir", str(tmp_path / run), "--threshold", "0.5"] + extra) == 0
        masks[run] = {n: np.array(Image.open(tmp_path / run / "masks" / f"{n}_mask.tif")) for n in ("a", "b")}
    assert not (tmp_path / "off" / "cell_stats.csv").exists()
    changed = 0
    for n in ("a", "b"):
        off = masks["off"][n]
        assert off.dtype == np.uint8 and off.max() <= 1
        assert np.array_equal(masks["stats"][n], off)   # statistics alone leave the mask as it is
        lab = cc.label_np(off, 8)
        want = cc.filter_np(lab, cc.areas_np(lab), 12)
        assert np.array_equal(masks["on"][n], want)
        changed += int((want != off).sum())
    print(f"pixels removed by --min-cc-px 12: {changed}")
    for run in ("stats", "on"):
        rows = read_cell_stats(tmp_path / run / "cell_stats.csv")
        assert rows[0] == cc.CELL_STATS_HEADER
        by = {r[0]: r for r in rows[1:]}
        assert sorted(by) == ["a.png", "b.png"]
        for n in ("a", "b"):
            st = cc.cell_statistics(masks[run][n], min_area=4, threshold=0.5)
            assert by[n + ".png"] == [str(v) for v in cc.cell_stats_row(n + ".png", st)]


class TilePredictor:
    """predict_single = the tile itself as a probability: the slide's prediction is the blended image."""

    def predict_single(self, image, mean, std):
        return (np.asarray(image, np.float32) / 255.0).astype(np.float32)


def test_reconstruct_all_slides_min_cc_px_and_cell_stats(tmp_path):
    import argparse
    import json

    from PIL import Image

    from adipose_amd import reconstruct as Rc
    from adipose_amd.predictor import GaussianBlender
    cc = CC()
    T, S = 64, 32
    H, W = 96, 160   # a grid of 2 x 4 tiles
    m = adipocyte_mask(9, H, W)
    m[5::11, 3::13] = 1   # specks
    rng = np.random.default_rng(2)
    img = np.clip(m * 200.0 + 20.0 + rng.normal(0, 6, m.shape), 0, 255).astype(np.uint8)
    (tmp_path / "data" / "images").mkdir(parents=True)
    for r in range(2):
        for c in range(4):
            t = img[r * S:r * S + T, c * S:c * S + T]
            Image.fromarray(np.stack([t, t, t], axis=-1)).save(tmp_path / "data" / "images" / f"s1_r{r}_c{c}.jpg", format="PNG")
    ck = tmp_path / "ckpt"
    ck.mkdir()
    (ck / "normalization_stats.json").write_text(json.dumps({"mean": 120.0, "std": 40.0}))

    def run(name, **kw):
        args = argparse.Namespace(weights=str(ck / "w.weights.h5"), data_root=str(tmp_path / "data"),
                                  output_dir=str(tmp_path / name), tile_size=T, stride=S, threshold=0.5,
                                  blend_mode="gaussian", use_tta=False, tta_mode="basic", boundary_refine=False,
                                  refine_kernel=5, save_metrics=True, min_coverage=0.9, max_tiles=None, **kw)
        out = Rc.reconstruct_all_slides(args, model=TilePredictor())
        with Image.open(out / "s1" / "prediction_mask.tif") as im:
            return out, np.asarray(im)

    out_off, p_off = run("off")
    out_on, p_on = run("on", min_cc_px=9, cell_stats=True, cell_min_area=10)
    out_st, p_st = run("stats", cell_stats=True)
    # the slide's prediction itself, to binarise it as the run does
    tiles = Rc.group_tiles_by_slide(tmp_path / "data" / "images", None)["s1"]["tiles"]
    _, pred, _ = Rc.reconstruct_slide(TilePredictor(), tiles, (H, W), T, S, 120.0, 40.0, GaussianBlender(T, 0.25))
    assert pred.shape == (H, W) and np.array_equal((pred * 255).astype(np.uint8), p_off) and np.array_equal(p_st, p_off)
    binary = (pred > 0.5).astype(np.uint8)
    lab = cc.label_np(binary, 8)
    want = cc.filter_np(lab, cc.areas_np(lab), 9)
    assert 0 < want.sum() < binary.sum()
    assert np.array_equal(p_on, want * 255)
    assert not (out_off / "cell_stats.csv").exists()
    rows = read_cell_stats(out_on / "cell_stats.csv")
    assert rows[0] == cc.CELL_STATS_HEADER and len(rows) == 2
    assert rows[1] == [str(v) for v in cc.cell_stats_row("s1", cc.cell_statistics(want, 10, 0.5))]
    rows = read_cell_stats(out_st / "cell_stats.csv")
    assert rows[1] == [str(v) for v in cc.cell_stats_row("s1", cc.cell_statistics(binary, 10, 0.5))]
    conf = json.loads((out_on / "reconstruction_log.json").read_text())["configuration"]
    assert conf["min_cc_px"] == 9 and conf["cell_stats"] is True and conf["cell_min_area"] == 10
    assert "min_cc_px" not in json.loads((out_off / "reconstruction_log.json").read_text())["configuration"]
