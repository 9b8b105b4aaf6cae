"""Annotation polygons -> ground-truth masks on the host (adipose_amd.annotations vs Segmentation/build_dataset.py).

The JSON readers are pinned to tests/golden/annotations.npz, produced by the reference's own functions
(tests/golden/make_annotations_golden.py) on the hand-written files under tests/golden/annotations/. The raster is not
reference output (cv2 is not installed; parity with cv2.fillPoly is unpinned): rasterize_np is pinned to the known
answers of the definition and to a brute-force statement of it written here, per pixel and per edge, in exact integers,
with the line by LineIterator's error walk rather than the closed form. Everything is integers: every comparison is
equality.
"""
import argparse
import importlib.util
import os
import re
from pathlib import Path

import numpy as np
import pytest

from adipose_amd import _lib
from adipose_amd import annotations as AN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "annotations.npz"))
JSON_DIR = Path(os.path.dirname(__file__)) / "golden" / "annotations"

RECT = [(1, 1), (6, 1), (6, 5), (1, 5)]
# name -> (polygons, H, W, ones, pattern check)
KNOWN = {
    "rectangle": ([RECT], 7, 8, 30),
    "rectangle twice": ([RECT, RECT], 7, 8, 18),
    "clipped square": ([[(-3, -3), (4, -3), (4, 4), (-3, 4)]], 6, 6, 25),
    "bow-tie": ([[(0, 0), (6, 6), (6, 0), (0, 6)]], 7, 7, 31),
    "overlapping squares": ([[(0, 0), (4, 0), (4, 4), (0, 4)], [(2, 2), (6, 2), (6, 6), (2, 6)]], 8, 8, 40),
    "triangle": ([[(1, 1), (6, 2), (3, 6)]], 8, 8, 19),
    "repeated point": ([[(2, 1)] * 3], 4, 4, 1),
    "flat polygon": ([[(0, 3), (7, 3), (3, 3)]], 6, 8, 8),
}


def rows_of(m):
    return ["".join(str(int(v)) for v in r) for r in m]


def check_known(name, m):
    polys, H, W, ones = KNOWN[name]
    assert m.shape == (H, W) and m.dtype == np.uint8 and int(m.sum()) == ones and m.max() <= 1, name
    if name == "rectangle":
        assert m[1:6, 1:7].all()
    elif name == "rectangle twice":
        want = np.zeros((7, 8), np.uint8)
        want[1:6, 1:7] = 1
        want[2:5, 2:6] = 0
        assert np.array_equal(m, want)
    elif name == "clipped square":
        assert m[0:5, 0:5].all()
    elif name == "bow-tie":
        assert m[3].all() and rows_of(m)[0] == "1000001" and rows_of(m)[6] == "1000001"
    elif name == "overlapping squares":
        assert m[3, 3] == 0
    elif name == "triangle":
        assert rows_of(m)[1:7] == ["01110000", "01111110", "00111100", "00111000", "00011000", "00010000"]


@pytest.mark.parametrize("name", list(KNOWN))
def test_known_answers(name):
    polys, H, W, _ = KNOWN[name]
    check_known(name, AN.rasterize_np([polys], H, W)[0])
    check_known(name, AN.create_binary_mask([np.array(p) for p in polys], W, H))


# ------------------------------------------------------------------------------ the definition, brute force
def line_walk(p, q):
    """LineIterator's 8-connected integer error walk from the endpoint with the smaller x."""
    (xa, ya), (xb, yb) = (p, q) if p[0] <= q[0] else (q, p)
    dx, dy = xb - xa, yb - ya
    sy = 1 if dy > 0 else -1
    dy = abs(dy)
    steep = dy > dx
    major, minor = (dy, dx) if steep else (dx, dy)
    err = major - 2 * minor
    x, y, pts = xa, ya, []
    for _ in range(major + 1):
        pts.append((x, y))
        neg = err < 0
        err += -2 * minor + (2 * major if neg else 0)
        if steep:
            y += sy
            x += 1 if neg else 0
        else:
            x += 1
            y += sy if neg else 0
    return pts


def brute(polys, H, W):
    edges = [(tuple(int(v) for v in p[i]), tuple(int(v) for v in p[(i + 1) % len(p)])) for p in polys for i in range(len(p))]
    m = np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            par = 0
            for (x0, y0), (x1, y1) in edges:
                if y0 == y1:
                    continue
                (xlo, ylo), (xhi, yhi) = ((x0, y0), (x1, y1)) if y0 < y1 else ((x1, y1), (x0, y0))
                D = yhi - ylo
                if ylo <= y < yhi and xlo * D + (y - ylo) * (xhi - xlo) <= x * D:
                    par ^= 1
            m[y, x] = par
    for p, q in edges:
        for x, y in line_walk(p, q):
            if 0 <= x < W and 0 <= y < H:
                m[y, x] = 1
    return m


def random_cases(n, seed=20260):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        H, W = int(rng.integers(1, 17)), int(rng.integers(1, 17))
        polys = [np.stack([rng.integers(-4, W + 4, k), rng.integers(-4, H + 4, k)], axis=1)
                 for k in rng.integers(3, 8, int(rng.integers(1, 4)))]
        yield polys, H, W


def test_rasterize_np_equals_the_brute_force_definition():
    cases = list(random_cases(150))
    got = [AN.rasterize_np([polys], H, W)[0] for polys, H, W in cases]
    for (polys, H, W), g in zip(cases, got):
        assert np.array_equal(g, brute(polys, H, W)), (polys, H, W)
    # several images in one call: each equals its own raster
    polys_a, polys_b = cases[0][0], cases[1][0]
    both = AN.rasterize_np([polys_a, [], polys_b], 11, 13)
    assert both.shape == (3, 11, 13) and not both[1].any()
    assert np.array_equal(both[0], brute(polys_a, 11, 13)) and np.array_equal(both[2], brute(polys_b, 11, 13))


def test_closed_form_line_equals_the_error_walk():
    rng = np.random.default_rng(7)
    for _ in range(300):
        p, q = tuple(int(v) for v in rng.integers(-20, 21, 2)), tuple(int(v) for v in rng.integers(-20, 21, 2))
        # p -> q, q -> q, q -> p: the line twice and a point; the two crossings of a row cancel, so the line is all
        got = AN.rasterize_np([[np.array([p, q, q]) + 24]], 48, 48)[0]
        want = np.zeros((48, 48), np.uint8)
        for x, y in line_walk(p, q):
            want[y + 24, x + 24] = 1
        assert np.array_equal(got, want), (p, q)


def test_pixel_centres_on_an_edge_are_set():
    n = 0
    for polys, H, W in random_cases(120, seed=99):
        m = AN.rasterize_np([polys], H, W)[0]
        for p in polys:
            for i in range(len(p)):
                (x0, y0), (x1, y1) = (int(v) for v in p[i]), (int(v) for v in p[(i + 1) % len(p)])
                for y in range(max(min(y0, y1), 0), min(max(y0, y1), H - 1) + 1):
                    for x in range(max(min(x0, x1), 0), min(max(x0, x1), W - 1) + 1):
                        if (x - x0) * (y1 - y0) == (y - y0) * (x1 - x0):
                            assert m[y, x] == 1, (polys, H, W, x, y)
                            n += 1
    assert n > 1000


def test_far_vertices_and_bounds():
    big = AN.COORD_MAX
    sq = [np.array([(-big, -big), (big, -big), (big, big), (-big, big)])]
    assert AN.rasterize_np([sq], 70, 129).all()
    for far in ([(0, 0), (big + 1, 0), (0, 5)], [(0, -big - 1), (3, 0), (0, 5)]):
        with pytest.raises(ValueError):
            AN.rasterize_np([[np.array(far)]], 8, 8)
        with pytest.raises(ValueError):   # before anything is launched: no device is needed to be refused
            AN.rasterize_bits([[np.array(far)]], 8, 8)
    with pytest.raises(ValueError):
        AN.rasterize_np([[np.array([(0.5, 0), (3, 0), (0, 5)])]], 8, 8)
    with pytest.raises(ValueError):
        AN.rasterize_np([[]], 0, 8)
    for side in ([(-9, 1), (-2, 1), (-2, 6)], [(20, 1), (30, 1), (25, 6)], [(1, -9), (6, -2), (1, -2)], [(1, 20), (6, 30), (1, 30)]):
        assert not AN.rasterize_np([[np.array(side)]], 8, 8).any()   # wholly outside, on each side
    assert AN.rasterize_np([], 4, 4).shape == (0, 4, 4)


def test_packed_words_have_zero_tail_bits():
    from adipose_amd import morphology as mo
    big = AN.COORD_MAX
    sq = [np.array([(-big, -big), (big, -big), (big, big), (-big, big)])]
    for W in (1, 63, 64, 65, 130):
        m = AN.rasterize_np([sq], 3, W)
        bits = mo.pack_np(m)
        assert bits.shape == (1, 3, (W + 63) // 64)
        tail = (1 << (W % 64)) - 1 if W % 64 else (1 << 64) - 1
        assert (bits[..., -1] == np.uint64(tail)).all()
        assert np.array_equal(mo.unpack_np(bits, W), m)


# ------------------------------------------------------------------------------ the JSON readers, golden
def unpack_polys(xy, lens):
    out, k = [], 0
    for n in lens:
        out.append(xy[k:k + int(n)])
        k += int(n)
    return out


def same_polys(got, xy, lens):
    want = unpack_polys(xy, lens)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert np.asarray(g).dtype.kind == "i" and np.array_equal(np.asarray(g), w)


def test_json_readers_equal_the_golden():
    names = [str(n) for n in GOLD["files"]]
    assert names == sorted(p.name for p in JSON_DIR.glob("*.json"))
    seen_missing = seen_low = seen_polys = 0
    for i, name in enumerate(names):
        path = JSON_DIR / name
        for c in (int(v) for v in GOLD["confidences"]):
            polys, missing = AN.load_json_annotations(path, c)
            same_polys(polys, GOLD[f"load_{i}_{c}_xy"], GOLD[f"load_{i}_{c}_len"])
            assert missing is bool(GOLD[f"load_{i}_{c}_missing"])
            assert AN.slide_has_valid_annotations(path, c) is bool(GOLD[f"valid_{i}_{c}"])
            seen_missing += missing
            seen_polys += len(polys)
            for b, box in enumerate(GOLD["bboxes"]):
                polys, low = AN.get_tile_annotations(path, tuple(int(v) for v in box), c)
                same_polys(polys, GOLD[f"tile_{i}_{c}_{b}_xy"], GOLD[f"tile_{i}_{c}_{b}_len"])
                assert low is bool(GOLD[f"tile_{i}_{c}_{b}_low"])
                seen_low += low
    assert seen_missing and seen_low and seen_polys   # the fixtures reach those branches
    for n, cls, want in zip(GOLD["stem_names"], GOLD["stem_cls"], GOLD["stem_out"]):
        assert AN.parse_image_stem_from_json(Path("/some/dir") / str(n), str(cls)) == str(want)
    # round-half-to-even at the .5 fractions of the first file's first polygon
    polys, _ = AN.load_json_annotations(JSON_DIR / "slideA_fat_annotations.json", 3)
    assert polys[0].tolist() == [[10, 10], [40, 10], [42, 30], [10, 32]]


# ------------------------------------------------------------------------------ ABI, header, CLI
def test_abi_has_the_raster_export():
    hdr = open(os.path.join(ROOT, "include", "adipose_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+adp_poly_raster\s*\(", code)
    assert "adp_poly_raster" in _lib.exported_symbols()
    assert len(_lib._SIGS["adp_poly_raster"]) == 10
    assert hasattr(_lib.lib(), "adp_poly_raster")
    assert int(re.search(r"#define ADP_POLY_COORD_MAX (\d+)", hdr).group(1)) == AN.COORD_MAX == 2 ** 24
    assert int(re.search(r"#define ADP_POLY_SCAN_WORDS (\d+)", hdr).group(1)) == AN.SCAN_WORDS
    assert int(re.search(r"#define ADP_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 21
    assert _lib.lib().adp_abi_version() == 21


def test_abi_refuses_bad_arguments_without_a_launch():
    L = _lib.lib()
    for args in ((-1, 4, 4, None, None, None, 0, 0, None, None), (1, 0, 4, None, None, None, 0, 0, None, None),
                 (1, 4, 0, None, None, None, 0, 0, None, None), (1, 4, 4, None, None, None, 0, 0, None, None),
                 (1, 4, 4, None, None, None, -1, 0, None, None), (1, 4, 4, None, None, None, 0, -1, None, None)):
        assert L.adp_poly_raster(*args) != 0
        assert b"adp_poly_raster" in L.adp_last_error()
    assert L.adp_poly_raster(0, 4, 4, None, None, None, 0, 0, None, None) == 0   # N = 0: nothing to do


def load_cli():
    spec = importlib.util.spec_from_file_location("recon_cli_ann", os.path.join(ROOT, "cli", "reconstruct_full_images.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_cli_flags_and_defaults():
    cli = load_cli()
    base = ["--weights", "w.h5", "--data-root", "d", "--output-dir", "o"]
    a = cli.parse_args(base)
    assert (a.annotations_dir, a.annotation_class, a.annotation_subtract_class, a.annotation_min_confidence,
            a.gt_morph_close_k, a.gt_min_cc_px) == (None, "fat", "bubbles", 2, 0, 0)
    assert (a.tile_size, a.stride, a.threshold, a.morph_close_k, a.min_cc_px) == (1024, 512, 0.5, 0, 0)
    a = cli.parse_args(base + ["--annotations-dir", "M", "--annotation-class", "muscle", "--annotation-subtract-class",
                               "none", "--annotation-min-confidence", "3", "--gt-morph-close-k", "5", "--gt-min-cc-px", "20"])
    assert (a.annotations_dir, a.annotation_class, a.annotation_subtract_class, a.annotation_min_confidence,
            a.gt_morph_close_k, a.gt_min_cc_px) == ("M", "muscle", "none", 3, 5, 20)
    with pytest.raises(SystemExit):
        cli.parse_args(base + ["--gt-morph-close-k", "64"])


# ------------------------------------------------------------------------------ the reconstruction's ground truth
def write_masks_folder(root):
    """The reference's Masks folder from the golden JSON files: fat/ (two for slideA: the later name wins) and bubbles/."""
    import shutil
    (root / "fat").mkdir(parents=True)
    (root / "bubbles").mkdir()
    shutil.copy(JSON_DIR / "lowonly_fat_annotations.json", root / "fat" / "slideA_fat_annotations.json")
    shutil.copy(JSON_DIR / "slideA_fat_annotations.json", root / "fat" / "slideA_fat_annotations_v2.json")
    shutil.copy(JSON_DIR / "slide_B x_fat_v2.json", root / "fat" / "slide_B x_fat_v2.json")
    shutil.copy(JSON_DIR / "slideA_bubbles_annotations.json", root / "bubbles" / "slideA_bubbles_annotations.json")


def test_annotation_ground_truth_of_a_slide(tmp_path):
    """What reconstruct_all_slides puts in full_gt for a slide with a JSON (the reconstruction itself blends on the device
    and is tested in tests/test_gpu_annotations.py): the JSON lookup and the chain, here on whichever path the host has."""
    from adipose_amd import reconstruct as R
    write_masks_folder(tmp_path / "Masks")
    with pytest.warns(UserWarning, match="replaces"):
        fat = R.find_annotation_jsons(tmp_path / "Masks", "fat")
    assert {k: v.name for k, v in fat.items()} == {"slideA": "slideA_fat_annotations_v2.json", "slide_B x": "slide_B x_fat_v2.json"}
    bub = R.find_annotation_jsons(tmp_path / "Masks", "bubbles")
    assert list(bub) == ["slideA"] and R.find_annotation_jsons(tmp_path / "Masks", "muscle") == {}
    H, W = 100, 130
    polys = AN.load_json_annotations(fat["slideA"], 2)[0]
    sub = AN.load_json_annotations(bub["slideA"], 2)[0]
    assert len(polys) == 5 and len(sub) == 2
    for kw in (dict(), dict(morph_close_k=5, min_cc_px=20)):
        got = R.annotation_ground_truth(fat["slideA"], bub["slideA"], (H, W), 2, *kw.values())
        got = got.cpu().numpy() if hasattr(got, "cpu") else got
        want = AN.target_mask_np(polys, sub, H, W, **kw)
        assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32)) and want.any()
    plain = AN.rasterize_np([polys], H, W)[0]
    assert np.array_equal(AN.target_mask_np(polys, sub, H, W), plain & (1 - AN.rasterize_np([sub], H, W)[0]))
    assert (AN.target_mask_np(polys, sub, H, W) != plain).any() and np.array_equal(AN.target_mask_np(polys, None, H, W), plain)
    a = argparse.Namespace(annotations_dir=str(tmp_path / "Masks"), gt_morph_close_k=5)
    assert R._annotation_settings(a) == {"annotations_dir": str(tmp_path / "Masks"), "annotation_class": "fat",
                                         "annotation_subtract_class": "bubbles", "annotation_min_confidence": 2,
                                         "gt_morph_close_k": 5, "gt_min_cc_px": 0}
    assert R._annotation_settings(argparse.Namespace()) == {} == R._annotation_settings(argparse.Namespace(annotations_dir=None))


def test_a_missing_annotation_folder_is_refused(tmp_path):
    from adipose_amd import reconstruct as R
    (tmp_path / "Masks" / "bubbles").mkdir(parents=True)
    args = argparse.Namespace(annotations_dir=str(tmp_path / "Masks"))   # no fat/ in it
    with pytest.raises(FileNotFoundError, match="Annotation directory not found"):
        R.reconstruct_all_slides(args)   # (refused before anything else is looked at)
