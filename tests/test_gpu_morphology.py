"""Bit-packed binary morphology on the GPU (csrc/morph.hip) against the numpy path of adipose_amd.morphology.

Everything is integers, so every comparison is array_equal: there is no tolerance. The numpy path itself is pinned to
oracle/numpy_ref.py's cv_morph and to scipy.ndimage in tests/test_morphology.py; cv2 is not installed, so parity with
cv2 itself is unpinned.

A block of the kernel produces TR rows x TW words (64 TW pixels) from a tile with k - 1 halo rows and one halo word per
side; the shapes below sit below, on and just past a word and a tile, and the structure cases are drawn across the words'
and tiles' borders.
"""
import functools
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def MO():
    from adipose_amd import morphology
    return morphology


TR, TW = 32, 8   # the kernel's tile in rows and words (asserted against the module and the header below)

SHAPES = [(1, 1, 1), (1, 2, 2), (3, 7, 9), (1, 5, 63), (1, 5, 64), (1, 5, 65), (2, 64, 96), (1, 257, 131),
          (1, TR, 64 * TW),               # exactly one tile
          (1, TR + 1, 64 * TW + 1),       # one tile plus one row and one pixel
          (5, TR + 1, 2 * 64 * TW - 1)]
FOOTPRINTS = [(k, "ellipse") for k in (1, 2, 3, 4, 5, 8, 15, 16, 31, 63)] + \
             [(k, kind) for kind in ("rect", "cross") for k in (2, 5, 16)]
OPS = ("dilate", "erode", "close", "open")


def test_tile_constants():
    mo = MO()
    assert (mo.TILE_ROWS, mo.TILE_WORDS) == (TR, TW)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "adipose_hip.h")).read()
    vals = {k: int(v) for k, v in re.findall(r"#define (ADP_MORPH_[A-Z0-9_]+) (\d+)", src)}
    assert (vals["ADP_MORPH_TILE_ROWS"], vals["ADP_MORPH_TILE_WORDS"]) == (TR, TW)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def random_case(shape):
    """A seeded f32 map with exact 0.5 values (background at thr = 0.5) and its foreground, computed once."""
    rng = np.random.default_rng(shape[0] * 1000003 + shape[1] * 1009 + shape[2] * 10)
    dens = rng.choice([0.03, 0.5, 0.97], size=shape[0])
    p = rng.random(shape).astype(np.float32)
    prob = np.where(p < dens[:, None, None], 0.5 + 0.5 * rng.random(shape).astype(np.float32) + 1e-3, 0.5 * p).astype(np.float32)
    prob[rng.random(shape) < 0.1] = 0.5
    assert (prob == 0.5).any() or prob.size < 8
    return prob, (prob > 0.5).astype(np.uint8)


def want_all(fg, k, kind):
    mo = MO()
    return {"dilate": mo.dilate_np(fg, k, kind), "erode": mo.erode_np(fg, k, kind), "close": mo.close_np(fg, k, kind),
            "open": mo.open_np(fg, k, kind)}


def check_all(fg, k, kind, prob=None):
    """The four operations of one u8 input (through dilate / erode / close / open, u8 out) and, where `prob` is given,
    of the f32 input with the fused threshold (through the plane calls, f32 out) against the numpy path."""
    mo = MO()
    want = want_all(fg, k, kind)
    W = fg.shape[-1]
    d = dev(fg)
    for name in OPS:
        got = getattr(mo, name)(d, k, kind)
        assert got.dtype == torch.uint8 and got.shape == d.shape
        assert np.array_equal(got.cpu().numpy(), want[name]), (name, k, kind, fg.shape)
    if prob is None:
        return
    rows = mo.footprint_rows(k, kind)
    bits = mo.pack(dev(prob), threshold=0.5)
    dil, ero = mo.dilate_bits(bits, W, rows), mo.erode_bits(bits, W, rows)
    planes = {"dilate": dil, "erode": ero, "close": mo.erode_bits(dil, W, rows), "open": mo.dilate_bits(ero, W, rows)}
    for name in OPS:
        assert np.array_equal(planes[name].cpu().numpy().view(np.uint64), mo.pack_np(want[name])), (name, k, kind, fg.shape)
        got = mo.unpack(planes[name], W, torch.float32)
        assert got.dtype == torch.float32
        assert np.array_equal(got.cpu().numpy(), want[name].astype(np.float32)), (name, k, kind, fg.shape)


@pytest.mark.parametrize("k,kind", FOOTPRINTS, ids=lambda v: str(v))
def test_device_equals_numpy(k, kind):
    for shape in SHAPES:
        prob, fg = random_case(shape)
        check_all(fg, k, kind, prob)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pack_equals_pack_np(shape):
    mo = MO()
    prob, fg = random_case(shape)
    want = mo.pack_np(fg)
    W = shape[2]
    for got in (mo.pack(dev(fg)), mo.pack(dev(prob), threshold=0.5), mo.pack(dev(fg.astype(bool))), mo.pack(fg)):
        assert got.dtype == torch.int64 and tuple(got.shape) == want.shape and got.is_cuda
        g = got.cpu().numpy().view(np.uint64)
        assert np.array_equal(g, want)
        if W % 64:
            assert not (g[..., -1] >> np.uint64(W % 64)).any()
    assert np.array_equal(mo.unpack(mo.pack(dev(fg)), W).cpu().numpy(), fg)
    assert np.array_equal(mo.pack(dev(fg[0])).cpu().numpy().view(np.uint64), want[0])   # (H, W) in, (H, WW) out


@pytest.mark.parametrize("shape", [(1, 1, 64), (3, 5, 128), (2, TR + 1, 64 * TW), (1, 3, 64 * 33)], ids=str)
def test_whole_word_widths(shape):
    """W % 64 == 0 on 16-byte aligned maps takes the kernels that move 16 pixels per lane; the same map at an address
    that is not 16-byte aligned takes the wave-per-word kernels. Both against the numpy path."""
    mo = MO()
    prob, fg = random_case(shape)
    W = shape[2]
    want = mo.pack_np(fg)
    n = fg.size
    for src, thr in ((fg, None), (prob, 0.5)):
        d = dev(src)
        base = torch.zeros(n + 16, dtype=d.dtype, device="cuda")
        odd = base[1:1 + n].view(shape)   # 1 B (u8) or 4 B (f32) past the allocation's start
        odd.copy_(d)
        assert d.data_ptr() % 16 == 0 and odd.data_ptr() % 16 != 0 and odd.is_contiguous()
        for t in (d, odd):
            bits = mo.pack(t, threshold=thr)
            assert np.array_equal(bits.cpu().numpy().view(np.uint64), want)
    bits = mo.pack(dev(fg))
    assert np.array_equal(mo.unpack(bits, W).cpu().numpy(), fg)
    assert np.array_equal(mo.unpack(bits, W, torch.float32).cpu().numpy(), fg.astype(np.float32))
    assert np.array_equal(mo.close(dev(fg), 5).cpu().numpy(), mo.close_np(fg, 5))
    assert np.array_equal(mo.close(dev(prob), 4, threshold=0.5, dtype=torch.float32).cpu().numpy(),
                          mo.close_np(fg, 4, dtype=np.float32))


@pytest.mark.parametrize("k", [5, 16, 63])
def test_close_against_the_oracle(k):
    from oracle import numpy_ref as O
    _, fg = random_case((1, 257, 131))
    rows = O.cv_ellipse_rows(k)
    g = fg[0] * np.uint8(255)
    want = O.cv_morph(O.cv_morph(g, rows, True), rows, False)
    got = MO().close(dev(fg[0]), k)
    assert np.array_equal(got.cpu().numpy() * np.uint8(255), want)


# ---------------------------------------------------------------- structure across word and tile borders
STRUCT_FOOTPRINTS = [(2, "ellipse"), (5, "ellipse"), (16, "ellipse"), (31, "ellipse"), (5, "cross"), (4, "rect")]


def test_single_pixels():
    H, W = TR + 9, 64 * TW + 37
    for py, px in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (3, 63), (3, 64), (TR - 1, 64 * TW - 1), (TR, 64 * TW)):
        m = np.zeros((1, H, W), np.uint8)
        m[0, py, px] = 1
        for k, kind in STRUCT_FOOTPRINTS:
            check_all(m, k, kind)
    for k, kind in STRUCT_FOOTPRINTS:   # the 1 x 1 image: every offset but the anchor's falls outside
        check_all(np.ones((1, 1, 1), np.uint8), k, kind)


@pytest.mark.parametrize("gap", [1, 2, 3, 4, 7])
def test_bars_with_a_gap(gap):
    """Two bars with `gap` background pixels between them, the gap straddling x = 64 and, transposed, row TR: they
    close exactly where the numpy path says, and that depends on the footprint."""
    mo = MO()
    H, W = 2 * TR + 5, 150
    closed_somewhere = False
    for vertical in (False, True):
        m = np.zeros((1, H, W), np.uint8)
        if not vertical:
            a = 64 - (gap + 1) // 2
            m[0, 10:50, 20:a] = 1
            m[0, 10:50, a + gap:120] = 1
        else:
            a = TR - (gap + 1) // 2
            m[0, 4:a, 30:110] = 1
            m[0, a + gap:H - 3, 30:110] = 1
        for k, kind in STRUCT_FOOTPRINTS:
            check_all(m, k, kind)
            closed_somewhere |= bool((mo.close_np(m, k, kind) != m).any())
    assert closed_somewhere


def test_pinholes_and_adipocytes():
    ones = np.ones((1, TR + 7, 64 * TW + 3), np.uint8)
    for y, x in ((0, 0), (5, 63), (5, 64), (TR - 1, 100), (TR, 64 * TW), (TR + 6, 64 * TW + 2)):
        ones[0, y, x] = 0
    from adipose_amd.data import synthetic_tile
    _, mask = synthetic_tile(np.random.default_rng(3), size=256, channels=1)
    cells = (mask > 0.5).astype(np.uint8)[None]
    assert cells.any() and not cells.all()
    for k, kind in STRUCT_FOOTPRINTS + [(15, "ellipse")]:
        check_all(ones, k, kind)
        check_all(cells, k, kind)
    assert np.array_equal(MO().close_np(ones, 3), np.ones_like(ones))   # a one-pixel hole closes


def test_independent_of_batch_and_run():
    mo = MO()
    prob, fg = random_case((5, TR + 1, 2 * 64 * TW - 1))
    d = dev(fg)
    for k, kind in ((5, "ellipse"), (16, "ellipse"), (63, "ellipse")):
        whole = mo.close(d, k, kind)
        assert torch.equal(whole, mo.close(d, k, kind))   # two runs
        for n in range(fg.shape[0]):
            assert torch.equal(whole[n], mo.close(d[n], k, kind))
            assert torch.equal(whole[n:n + 1], mo.close(d[n:n + 1], k, kind))


@pytest.mark.parametrize("k", [3, 5, 15])
def test_rect_close_equals_max_pool(k):
    """A device-side baseline that shares no code with the library: max_pool2d's -inf padding is the same "outside takes
    no part" border, so for odd k the rect closing is max_pool2d, then its negation's."""
    import torch.nn.functional as F
    for shape in ((2, 64, 96), (1, 257, 131)):
        _, fg = random_case(shape)
        x = dev(fg).float()[:, None]
        dil = F.max_pool2d(x, k, 1, k // 2)
        want = (-F.max_pool2d(-dil, k, 1, k // 2))[:, 0]
        got = MO().close(dev(fg), k, "rect", dtype=torch.float32)
        assert torch.equal(got, want)


def test_argument_errors():
    import ctypes as C

    from adipose_amd._lib import AdpError, call, ptr, stream_ptr
    mo = MO()
    _, fg = random_case((3, 7, 9))
    bits = mo.pack(dev(fg))
    out = torch.empty_like(bits)

    def raw(src, dst, k, op=0, lo=None, hi=None):
        n = max(k, 1)
        lo, hi = lo or [0] * n, hi or [min(k, 1)] * n
        call("adp_morph_bits", 3, 7, 9, ptr(src), ptr(dst), k, (C.c_int * n)(*lo), (C.c_int * n)(*hi), op, stream_ptr())

    raw(bits, out, 1)   # the identity
    assert torch.equal(out, bits)
    for k in (0, 64):
        with pytest.raises(AdpError, match="ksize"):
            raw(bits, out, k)
    with pytest.raises(AdpError, match="alias"):
        raw(bits, bits, 3, lo=[0] * 3, hi=[3] * 3)
    with pytest.raises(AdpError, match="op"):
        raw(bits, out, 1, op=2)
    with pytest.raises(AdpError, match="footprint row"):
        raw(bits, out, 2, lo=[0, 1], hi=[3, 2])
    with pytest.raises(AdpError, match="both NULL"):
        call("adp_morph_unpack", 3, 7, 9, ptr(bits), None, None, stream_ptr())
    with pytest.raises(TypeError):
        mo.close(dev(fg).float(), 3)              # a float mask without a threshold
    with pytest.raises(TypeError):
        mo.close(dev(fg).to(torch.int32), 3)      # wrong dtype
    with pytest.raises(ValueError):
        mo.close(dev(fg)[None], 3)                # 4-D
    with pytest.raises(ValueError):
        mo.close(dev(fg), 64)
    with pytest.raises(TypeError):
        mo.dilate_bits(dev(fg), 9, mo.footprint_rows(3))   # not a plane
    with pytest.raises(ValueError):
        mo.unpack(bits, 65)                       # W does not match the words
    empty = mo.close(torch.zeros((0, 7, 9), dtype=torch.uint8, device="cuda"), 3)
    assert empty.shape == (0, 7, 9) and empty.dtype == torch.uint8


def test_morph_close_surface():
    mo = MO()
    _, fg = random_case((1, 257, 131))
    m = np.array(fg[0])
    want = mo.close_np(m, 5)
    assert (want != m).any()
    got = mo.morph_close(m, 5)   # a host array goes through the device where there is one
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want)
    d = dev(m)
    assert mo.morph_close(d, 0) is d
    got = mo.morph_close(d, 5)
    assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    got = mo.morph_close(d.float(), 5)
    assert got.is_cuda and got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), want.astype(np.float32))
    got = mo.morph_close(torch.from_numpy(m), 5)
    assert not got.is_cuda and np.array_equal(got.numpy(), want)


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


def test_cli_morph_close_k(tmp_path):
    from PIL import Image

    from adipose_amd import components as cc
    from adipose_amd.checkpoint import save_weights
    from cli.segmentation_inference import main
    from oracle import torch_ref as TRf
    mo = MO()
    (tmp_path / "img").mkdir()
    for name, seed in (("a", 61), ("b", 62)):
        Image.fromarray(cell_tile(seed)).save(tmp_path / "img" / f"{name}.png")
    (tmp_path / "ck").mkdir()
    save_weights(None, tmp_path / "ck" / "phase2_best.weights.h5",
                 weights=TRf.adipose_v3_keras_weights(seed=5, deep_supervision=False))
    (tmp_path / "ck" / "normalization_stats.json").write_text('{"mean": 120.0, "std": 40.0}')
    base = ["--images-dir", str(tmp_path / "img"), "--weights", str(tmp_path / "ck"), "--tile", "64"]
    masks = {}
    for run, extra in (("off", []), ("close", ["--morph-close-k", "5"]),
                       ("both", ["--morph-close-k", "5", "--min-cc-px", "12"])):
        assert main(base + ["--output-dir", str(tmp_path / run), "--threshold", "0.5"] + extra) == 0
        masks[run] = {n: np.array(Image.open(tmp_path / run / "masks" / f"{n}_mask.tif")) for n in ("a", "b")}
    changed = 0
    for n in ("a", "b"):
        off = masks["off"][n]
        assert off.dtype == np.uint8 and off.max() <= 1
        closed = mo.close_np(off, 5)
        assert np.array_equal(masks["close"][n], closed)
        lab = cc.label_np(closed, 8)
        assert np.array_equal(masks["both"][n], cc.filter_np(lab, cc.areas_np(lab), 12))   # close, then filter
        changed += int((closed != off).sum())
    print(f"pixels changed by --morph-close-k 5: {changed}")
    assert changed > 0


class TilePredictor:
    """predict_single = the tile itself as a probability: the slide's prediction is the blended image."""

    def predict_single(self, image, mean, std):
        return (np.asarray(image, np.float32) / 255.0).astype(np.float32)


def test_reconstruct_all_slides_morph_close_k(tmp_path):
    import argparse
    import json

    from PIL import Image

    from adipose_amd import reconstruct as Rc
    from adipose_amd.data import synthetic_tile
    from adipose_amd.predictor import GaussianBlender
    mo = MO()
    T, S = 64, 32
    H, W = 96, 160   # a grid of 2 x 4 tiles
    _, mask = synthetic_tile(np.random.default_rng(9), size=max(H, W), channels=1)
    m = (mask[:H, :W] > 0.5).astype(np.uint8)
    m[:, 40::37] = 0      # one-pixel slits
    m[7::13, 5::17] = 0   # pinholes
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
    out_on, p_on = run("on", morph_close_k=5)
    out_zero, p_zero = run("zero", morph_close_k=0)
    tiles = Rc.group_tiles_by_slide(tmp_path / "data" / "images", None)["s1"]["tiles"]
    _, pred, _ = Rc.reconstruct_slide(TilePredictor(), tiles, (H, W), T, S, 120.0, 40.0, GaussianBlender(T, 0.25))
    assert np.array_equal((pred * 255).astype(np.uint8), p_off) and np.array_equal(p_zero, p_off)   # as without the flag
    binary = (pred > 0.5).astype(np.uint8)
    closed = mo.close_np(binary, 5)
    assert 0 < (closed != binary).sum()
    assert np.array_equal(p_on, closed * np.uint8(255))
    conf = json.loads((out_on / "reconstruction_log.json").read_text())["configuration"]
    assert conf["morph_close_k"] == 5 and conf["min_cc_px"] == 0 and conf["cell_stats"] is False
    for out in (out_off, out_zero):
        conf = json.loads((out / "reconstruction_log.json").read_text())["configuration"]
        assert "morph_close_k" not in conf and "min_cc_px" not in conf
