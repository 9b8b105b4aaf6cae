"""Per-component shape sums on the GPU (csrc/components.hip adp_cc_shape) against the numpy path of
adipose_amd.components.

Every device result is an integer, so every comparison is array_equal; the floats of cell_shapes come from the same
host function on both paths and are compared for equality too. The numpy path itself is pinned in
tests/test_component_shapes.py.

The kernel works on tiles of TR x TC pixels and reads a two-pixel halo around each; the shapes below sit on, one past
and two past a tile, and the structures are drawn across the tiles' borders and corners.
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


TR, TC = 64, 128   # the kernel's tile (asserted against the module below)

SHAPES = [(1, 1, 1), (1, 2, 2), (3, 7, 9),
          (1, TR, TC),                # exactly one tile
          (1, TR + 1, TC + 1),        # the halo's first pixel is the next tile's
          (1, TR + 2, TC + 2),        # ... and its second
          (1, 2 * TR - 1, 65),        # the second wave of a tile row has one live lane
          (5, TR + 1, 2 * TC - 1)]    # batch offsets


def test_tile_constants():
    assert (CC().SHAPE_TILE_ROWS, CC().SHAPE_TILE_COLS) == (TR, TC)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def random_case(shape, connectivity):
    """A seeded 0 / 1 map (a density per image) and its reference labels, computed once."""
    rng = np.random.default_rng(shape[0] * 1000003 + shape[1] * 1009 + shape[2] * 10 + connectivity)
    dens = rng.choice([0.1, 0.45, 0.6, 0.9], size=shape[0])
    m = (rng.random(shape) < dens[:, None, None]).astype(np.uint8)
    return m, CC().label_np(m, connectivity)


def check(mask_u8, connectivity, lab_want=None):
    """shape_table of the device's labels against shape_table_np of the numpy labels, for more rows than components
    and for about half of them. Returns the full reference rows of image 0."""
    cc = CC()
    if lab_want is None:
        lab_want = cc.label_np(mask_u8, connectivity)
    lab = cc.label(dev(mask_u8), connectivity)
    assert np.array_equal(lab.cpu().numpy(), lab_want)
    _, counts = cc.table_np(lab_want, 0)
    kmax = int(counts.max())
    for rows in sorted({kmax + 3, max(kmax // 2, 1)}):
        got = cc.shape_table(lab, rows)
        want = cc.shape_table_np(lab_want, rows)
        assert got.dtype == torch.int64 and got.shape == want.shape
        assert np.array_equal(got.cpu().numpy(), want)
    return want[0][:int(counts[0])]


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_random_maps(shape, connectivity):
    m, lab = random_case(shape, connectivity)
    check(m, connectivity, lab)


# ---------------------------------------------------------------- structures that stress the aggregation
def checkerboard(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy + xx) % 2 == 0).astype(np.uint8)


def frame(h, w):
    m = np.zeros((h, w), np.uint8)
    m[0] = m[-1] = 1
    m[:, 0] = m[:, -1] = 1
    return m


def corner_bars(h, w):
    """A horizontal bar ending at (TR - 1, TC - 1) and a vertical one starting at (TR, TC): they meet only across the
    corner of four tiles."""
    m = np.zeros((h, w), np.uint8)
    m[TR - 1, 5:TC] = 1
    m[TR:h - 3, TC] = 1
    return m


@pytest.mark.parametrize("connectivity", [4, 8])
def test_all_foreground(connectivity):
    """One component: every tile adds to one row."""
    H, W = 2 * TR, 2 * TC
    rows = check(np.ones((1, H, W), np.uint8), connectivity)
    x, y = np.arange(W, dtype=np.int64), np.arange(H, dtype=np.int64)
    assert rows.tolist() == [[0, H * int((x * x).sum()), W * int((y * y).sum()), int(x.sum()) * int(y.sum()),
                              2 * (H + W) - 4, 0, 0, 2 * (H + W) - 4]]


@pytest.mark.parametrize("connectivity", [4, 8])
def test_checkerboard(connectivity):
    """At connectivity 4: more labels in a tile than the hash table holds (the overflow path), and every diagonal
    neighbour is a border pixel of another label. At connectivity 8: one component whose pixels are all border."""
    H, W = TR + 3, TC + 3
    rows = check(checkerboard(H, W)[None], connectivity)
    if connectivity == 4:
        assert len(rows) == (H * W + 1) // 2 and (rows[:, 4:7] == 0).all() and (rows[:, 7] == 1).all()
    else:
        assert len(rows) == 1 and rows[0, 7] == (H * W + 1) // 2


@pytest.mark.parametrize("connectivity", [4, 8])
def test_frame_along_the_image_edge(connectivity):
    H, W = TR + 5, TC + 7
    rows = check(frame(H, W)[None], connectivity)
    # every pixel is a border pixel with two border neighbours along the frame; the four corners turn
    assert len(rows) == 1 and rows[0, 4:8].tolist() == [2 * (H + W) - 4, 0, 0, 2 * (H + W) - 4]


@pytest.mark.parametrize("connectivity", [4, 8])
def test_bars_meeting_across_a_tile_corner(connectivity):
    rows = check(corner_bars(2 * TR, 2 * TC)[None], connectivity)
    assert len(rows) == (1 if connectivity == 8 else 2)


def test_long_row_at_the_int64_bound():
    """(1, 1, 2^21) is the longest single row whose moments fit: one run over 2^14 tiles, S_xx near 2^63 / 3."""
    cc = CC()
    W = 2 ** 21
    lab = cc.label(torch.ones((1, W), dtype=torch.uint8, device="cuda"), 8)
    got = cc.shape_table(lab, 2).cpu().numpy()
    assert got[0].tolist() == [0, (W - 1) * W * (2 * W - 1) // 6, 0, 0, W - 2, 0, 0, W] and not got[1].any()


# ---------------------------------------------------------------- determinism, arguments
def test_independent_of_batching_and_run():
    m, lab_want = random_case((5, TR + 1, 2 * TC - 1), 8)
    cc = CC()
    lab = cc.label(dev(m), 8)
    _, counts = cc.table_np(lab_want, 0)
    rows = int(counts.max()) + 1
    one = cc.shape_table(lab, rows)
    assert one.cpu().numpy().tobytes() == cc.shape_table(lab, rows).cpu().numpy().tobytes()
    for n in range(5):
        alone = cc.shape_table(lab[n].contiguous(), rows)
        assert alone.shape == (rows, 8) and torch.equal(alone, one[n])


def test_argument_errors():
    from adipose_amd import _lib
    L = _lib.lib()
    lab = CC().label(torch.ones((2, 3), dtype=torch.uint8, device="cuda"), 8)
    shp = torch.full((2, 8), -7, dtype=torch.int64, device="cuda")
    s, p = _lib.stream_ptr(), _lib.ptr

    def fails(rc):
        return rc != 0 and len(L.adp_last_error()) > 0

    assert fails(L.adp_cc_shape(1, 2, 3, None, 2, p(shp), s))
    assert fails(L.adp_cc_shape(1, 2, 3, p(lab), 2, None, s))
    assert fails(L.adp_cc_shape(1, 2, 3, p(lab), -1, p(shp), s))
    assert fails(L.adp_cc_shape(0, 2, 3, p(lab), 2, p(shp), s))
    assert fails(L.adp_cc_shape(1, 0, 3, p(lab), 2, p(shp), s))
    assert fails(L.adp_cc_shape(1, 65536, 32768, p(lab), 2, p(shp), s))
    assert b"2^31" in L.adp_last_error()
    # H * W * (max(H, W) - 1)^2 >= 2^63 (sizes only: no such buffer exists)
    assert fails(L.adp_cc_shape(1, 1, 2 ** 21 + 1, p(lab), 2, p(shp), s))
    assert b"2^63" in L.adp_last_error()
    assert fails(L.adp_cc_shape(1, 1, 2 ** 31 - 3, p(lab), 2, p(shp), s))
    torch.cuda.synchronize()
    assert (shp == -7).all()   # nothing was launched
    with pytest.raises(_lib.AdpError):
        _lib.call("adp_cc_shape", 1, 2, 3, p(lab), -1, p(shp), s)
    with pytest.raises(TypeError):
        CC().shape_table(lab.float(), 2)
    assert L.adp_cc_shape(1, 2, 3, p(lab), 0, None, s) == 0   # no rows: nothing to do
    assert L.adp_cc_shape(1, 2, 3, p(lab), 2, p(shp), s) == 0
    assert shp.cpu().numpy().tolist() == [[0, 10, 3, 3, 6, 0, 0, 6], [0] * 8]


# ---------------------------------------------------------------- the reference's surface on the device
def adipocyte_mask(seed, h, w):
    """synthetic_tile's mask (ellipses: the cells), cropped to h x w."""
    from adipose_amd.data import synthetic_tile
    _, mask = synthetic_tile(np.random.default_rng(seed), size=max(h, w), channels=1)
    return (mask[:h, :w] > 0.5).astype(np.uint8)


def test_cell_shapes_device_equals_numpy(monkeypatch):
    cc = CC()
    m = adipocyte_mask(5, 200, 300)
    m[::7, ::5] |= 1   # specks
    check(m[None], 8)
    got = cc.cell_shapes(dev(m).float(), min_area=10, threshold=0.5)
    got_u8 = cc.cell_shapes(dev(m), 10)
    with monkeypatch.context() as mp:
        mp.setattr(cc, "_gpu", lambda: False)
        want = cc.cell_shapes(m, min_area=10, threshold=0.5)
        st = cc.cell_statistics(m, 10, 0.5)
    assert got == want and got_u8 == want and want["num_cells"] > 3
    assert cc.stats_from_shapes(got) == st == cc.cell_statistics(dev(m).float(), 10, 0.5)
    # more components than the first guess of rows: one more call of the table, and as many shape rows
    dots = np.zeros((140, 140), np.uint8)
    dots[::2, ::2] = 1
    dots[0:3, 0:3] = 1
    b = cc.cell_shapes(dev(dots), min_area=1)
    with monkeypatch.context() as mp:
        mp.setattr(cc, "_gpu", lambda: False)
        assert b == cc.cell_shapes(dots, min_area=1)
    assert b["num_cells"] == 70 * 70 - 3 and b["areas"][:2] == [9.0, 1.0] and b["perimeters"][0] == 8.0
    assert cc.cell_shapes(torch.zeros((8, 8), device="cuda")) == {
        "num_cells": 0, "areas": [], "perimeters": [], "circularities": [], "aspect_ratios": [], "eccentricities": [],
        "tissue_coverage": 0.0}


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


def read_csv(path):
    with open(path) as f:
        return list(csv.reader(f))


def test_cli_cell_shapes(tmp_path):
    from PIL import Image

    from adipose_amd.checkpoint import save_weights
    from cli.segmentation_inference import main
    from oracle import torch_ref as TRef
    cc = CC()
    (tmp_path / "img").mkdir()
    for name, seed in (("a", 61), ("b", 62)):
        Image.fromarray(cell_tile(seed)).save(tmp_path / "img" / f"{name}.png")
    Image.fromarray(np.full((64, 64, 3), 255, np.uint8)).save(tmp_path / "img" / "w.png")   # empty for --tile-qc
    (tmp_path / "ck").mkdir()
    save_weights(None, tmp_path / "ck" / "phase2_best.weights.h5",
                 weights=TRef.adipose_v3_keras_weights(seed=5, deep_supervision=False))
    (tmp_path / "ck" / "normalization_stats.json").write_text('{"mean": 120.0, "std": 40.0}')
    base = ["--images-dir", str(tmp_path / "img"), "--weights", str(tmp_path / "ck"), "--tile", "64", "--threshold", "0.5"]
    runs = {"off": [], "shapes": ["--cell-shapes", "--cell-min-area", "4"],
            "both": ["--min-cc-px", "12", "--cell-stats", "--cell-shapes", "--cell-min-area", "4", "--tile-qc"]}
    masks = {}
    for run, extra in runs.items():
        assert main(base + ["--output-dir", str(tmp_path / run)] + extra) == 0
        masks[run] = {n: np.array(Image.open(tmp_path / run / "masks" / f"{n}_mask.tif")) for n in ("a", "b", "w")}
    assert not (tmp_path / "off" / "cell_shapes.csv").exists() and not (tmp_path / "off" / "cell_stats.csv").exists()
    assert not (tmp_path / "shapes" / "cell_stats.csv").exists()
    for n in ("a", "b", "w"):
        assert np.array_equal(masks["shapes"][n], masks["off"][n])   # the measures leave the mask as it is
    assert not masks["both"]["w"].any()
    for run in ("shapes", "both"):
        rows = read_csv(tmp_path / run / "cell_shapes.csv")
        assert rows[0] == cc.CELL_SHAPES_HEADER
        by = {r[0]: r for r in rows[1:]}
        assert sorted(by) == ["a.png", "b.png", "w.png"]
        for n in ("a", "b"):
            sh = cc.cell_shapes(masks[run][n], min_area=4, threshold=0.5)
            assert by[n + ".png"] == [str(v) for v in cc.cell_shapes_row(n + ".png", sh)]
    assert sum(int(r[1]) for r in read_csv(tmp_path / "shapes" / "cell_shapes.csv")[1:]) > 0
    # the tile that --tile-qc skipped: the zero rows
    assert by["w.png"] == [str(v) for v in cc.cell_shapes_row("w.png")]
    stats = {r[0]: r for r in read_csv(tmp_path / "both" / "cell_stats.csv")[1:]}
    assert stats["w.png"] == [str(v) for v in cc.cell_stats_row("w.png")]
    for n in ("a", "b"):   # from the one labelling, what cell_statistics gives
        st = cc.cell_statistics(masks["both"][n], min_area=4, threshold=0.5)
        assert stats[n + ".png"] == [str(v) for v in cc.cell_stats_row(n + ".png", st)]


class TilePredictor:
    """predict_single = the tile itself as a probability: the slide's prediction is the blended image."""

    def predict_single(self, image, mean, std):
        return (np.asarray(image, np.float32) / 255.0).astype(np.float32)


def test_reconstruct_all_slides_cell_shapes(tmp_path):
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
    out_sh, p_sh = run("shapes", cell_shapes=True)
    out_on, p_on = run("on", min_cc_px=9, cell_stats=True, cell_shapes=True, cell_min_area=12)
    tiles = Rc.group_tiles_by_slide(tmp_path / "data" / "images", None)["s1"]["tiles"]
    _, pred, _ = Rc.reconstruct_slide(TilePredictor(), tiles, (H, W), T, S, 120.0, 40.0, GaussianBlender(T, 0.25))
    assert np.array_equal(p_sh, p_off)
    binary = (pred > 0.5).astype(np.uint8)
    lab = cc.label_np(binary, 8)
    want = cc.filter_np(lab, cc.areas_np(lab), 9)
    assert np.array_equal(p_on, want * 255)
    assert not (out_off / "cell_shapes.csv").exists() and not (out_sh / "cell_stats.csv").exists()
    rows = read_csv(out_sh / "cell_shapes.csv")
    assert rows[0] == cc.CELL_SHAPES_HEADER and len(rows) == 2
    assert rows[1] == [str(v) for v in cc.cell_shapes_row("s1", cc.cell_shapes(binary, 10, 0.5))] and int(rows[1][1]) > 0
    rows = read_csv(out_on / "cell_shapes.csv")
    assert rows[1] == [str(v) for v in cc.cell_shapes_row("s1", cc.cell_shapes(want, 12, 0.5))]
    rows = read_csv(out_on / "cell_stats.csv")
    assert rows[1] == [str(v) for v in cc.cell_stats_row("s1", cc.cell_statistics(want, 12, 0.5))]
    conf = json.loads((out_on / "reconstruction_log.json").read_text())["configuration"]
    assert conf["cell_shapes"] is True and conf["cell_stats"] is True and conf["cell_min_area"] == 12
    conf = json.loads((out_sh / "reconstruction_log.json").read_text())["configuration"]
    assert conf == {**conf, "min_cc_px": 0, "cell_stats": False, "cell_min_area": 10, "cell_shapes": True}
    assert "cell_shapes" not in json.loads((out_off / "reconstruction_log.json").read_text())["configuration"]
