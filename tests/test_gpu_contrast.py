"""CLAHE, the gray statistics and the percentile stretch on the GPU (csrc/clahe.hip) against the numpy path of
adipose_amd.contrast.

Everything up to the look-up table is integers and every float32 step after it is a single IEEE operation, so every
comparison is array_equal, stage by stage (histograms, tables, output) and end to end: there is no tolerance. The numpy
path itself is pinned to the definition in tests/test_contrast.py; cv2 is not installed, so parity with cv2 itself is
unpinned.

A block of the histogram kernel counts a slab of SLAB_ROWS x SLAB_COLS pixels of one tile and the slabs of a tile meet in
global atomics; the interpolation kernel takes 16 pixels per lane where W % 16 == 0 and one otherwise. The shapes below
sit on, just past and well past those sizes, with grids that do and do not divide the image.
"""
import functools
import os
import re
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SLAB_ROWS, SLAB_COLS = 64, 1024   # asserted against the module and the header below


def CT():
    from adipose_amd import contrast
    return contrast


# (N, H, W), tile_grid = (tx, ty)
CASES = [((1, 8, 8), (8, 8)),                     # tiles of 1 x 1
         ((1, 2, 2), (1, 1)),
         ((3, 67, 64), (8, 8)),                   # W divides, and is still extended
         ((1, 64, 67), (8, 8)),
         ((1, 129, 95), (12, 12)),
         ((2, 64, 96), (8, 8)), ((2, 64, 96), (4, 2)),      # the 16-pixel path
         ((1, 65, 96), (8, 8)), ((1, 65, 96), (4, 2)),      # one row past it, with reflected rows
         ((1, 33, 17), (4, 2)),
         ((1, 2 * SLAB_ROWS, 32), (2, 2)),        # tile height = one slab
         ((1, 2 * SLAB_ROWS + 2, 32), (2, 2)),    # one slab and one row
         ((1, 2 * SLAB_ROWS + 12, 32), (2, 1)),   # more than two slabs
         ((1, 4, SLAB_COLS + 32), (1, 1)),        # more than one slab of columns, 16-pixel loads
         ((1, 5, SLAB_COLS + 17), (1, 1)),        # and byte loads
         ((5, 48, 80), (3, 5))]
CLIPS = [0.0, 0.01, 1.5, 2.0, 3.0, 40.0]
KINDS = ["zeros", "white", "const77", "two", "ramp", "random", "histology"]


def case_id(v):
    return "x".join(map(str, v))


@functools.lru_cache(maxsize=None)
def image(kind, shape):
    N, H, W = shape
    rng = np.random.default_rng(len(kind) * 7919 + N * 1000003 + H * 1009 + W)
    if kind == "zeros":
        return np.zeros(shape, np.uint8)
    if kind == "white":
        return np.full(shape, 255, np.uint8)
    if kind == "const77":
        return np.full(shape, 77, np.uint8)
    if kind == "two":
        return np.where(rng.random(shape) < 0.3, 31, 200).astype(np.uint8)
    if kind == "ramp":
        return np.broadcast_to((np.arange(W) * 255 // max(W - 1, 1)).astype(np.uint8), shape).copy()
    if kind == "random":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    # near-white background with long runs, stained blobs in between
    img = np.full(shape, 243, np.uint8)
    img[rng.random(shape) < 0.2] = 241
    blob = rng.random(shape) < 0.25
    img[blob] = rng.integers(90, 200, int(blob.sum()), dtype=np.uint8)
    return img


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def test_slab_constants():
    ct = CT()
    assert (ct.SLAB_ROWS, ct.SLAB_COLS, ct.MAX_GRID) == (SLAB_ROWS, SLAB_COLS, 64)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "adipose_hip.h")).read()
    vals = {k: int(v) for k, v in re.findall(r"#define (ADP_CLAHE_[A-Z0-9_]+) (\d+)", src)}
    assert (vals["ADP_CLAHE_SLAB_ROWS"], vals["ADP_CLAHE_SLAB_COLS"], vals["ADP_CLAHE_MAX_GRID"]) == (SLAB_ROWS, SLAB_COLS, 64)


@pytest.mark.parametrize("shape,grid", CASES, ids=case_id)
def test_stages_equal_numpy(shape, grid):
    ct = CT()
    _, _, th, tw = ct.clahe_geometry(shape[1], shape[2], grid)
    area = th * tw
    for kind in KINDS:
        img = image(kind, shape)
        d = dev(img)
        want_hist = ct.clahe_hist_np(img, grid)
        assert want_hist.sum() == shape[0] * grid[0] * grid[1] * area
        hist = ct.clahe_hist(d, grid)
        assert hist.dtype == torch.int32 and tuple(hist.shape) == want_hist.shape
        assert np.array_equal(u32(hist), want_hist), (kind, "hist")
        for clip in CLIPS:
            want_lut = ct.clahe_lut_np(want_hist, area, clip)
            lut = ct.clahe_lut(hist, area, clip)
            assert lut.dtype == torch.uint8 and np.array_equal(lut.cpu().numpy(), want_lut), (kind, clip, "lut")
            want = ct.clahe_apply_np(img, want_lut, grid)
            got = ct.clahe_apply(d, lut, grid)
            assert got.dtype == torch.uint8 and got.shape == d.shape
            assert np.array_equal(got.cpu().numpy(), want), (kind, clip, "apply")
        assert np.array_equal(ct.clahe(d, 2.0, grid).cpu().numpy(), ct.clahe_np(img, 2.0, grid)), kind


def test_constant_77_gives_84():
    got = CT().clahe(dev(np.full((64, 64), 77, np.uint8)), 2.0, (8, 8))
    assert got.shape == (64, 64) and (got == 84).all()


@pytest.mark.parametrize("shape,grid", [((2, 64, 96), (8, 8)), ((1, 65, 96), (4, 2)), ((3, 67, 64), (8, 8)),
                                        ((1, 4, SLAB_COLS + 32), (1, 1))], ids=case_id)
def test_f32_planes_and_unaligned_planes(shape, grid):
    """A float32 source is rounded to nearest and clamped on load, a float32 destination holds the same integers, and a
    plane that does not start on 16 bytes takes the one-pixel path: all the same image."""
    ct = CT()
    for kind in ("random", "histology", "const77"):
        img = image(kind, shape)
        want = ct.clahe_np(img, 3.0, grid)
        d = dev(img)
        f = d.float()
        assert np.array_equal(u32(ct.clahe_hist(f, grid)), ct.clahe_hist_np(img, grid))
        got = ct.clahe(f, 3.0, grid)
        assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), want.astype(np.float32))
        assert np.array_equal(ct.clahe(f, 3.0, grid, torch.uint8).cpu().numpy(), want)
        assert np.array_equal(ct.clahe(d, 3.0, grid, torch.float32).cpu().numpy(), want.astype(np.float32))
        n = img.size
        for src in (d, f):
            base = torch.zeros(n + 16, dtype=src.dtype, device="cuda")
            odd = base[1:1 + n].view(shape)
            odd.copy_(src)
            assert odd.data_ptr() % 16 != 0 and odd.is_contiguous()
            assert np.array_equal(ct.clahe(odd, 3.0, grid, torch.uint8).cpu().numpy(), want)
    # values off the integers, and outside 0 .. 255
    rng = np.random.default_rng(8)
    x = (image("random", shape).astype(np.float32) + rng.choice([-0.5, -0.3, 0.0, 0.3, 0.5, 300.0, -300.0], size=shape)
         .astype(np.float32))
    as_u8 = np.clip(np.rint(x), 0, 255).astype(np.uint8)
    assert np.array_equal(ct.clahe(dev(x), 2.0, grid, torch.uint8).cpu().numpy(), ct.clahe_np(as_u8, 2.0, grid))
    assert np.array_equal(ct.clahe_np(x, 2.0, grid), ct.clahe_np(as_u8, 2.0, grid))


def test_independent_of_batch_and_run():
    ct = CT()
    img = image("histology", (5, 48, 80))
    d = dev(img)
    whole = ct.clahe(d, 2.0, (3, 5))
    assert torch.equal(whole, ct.clahe(d, 2.0, (3, 5)))
    for n in range(5):
        assert torch.equal(whole[n], ct.clahe(d[n], 2.0, (3, 5)))
    assert ct.clahe(d[0], 2.0, (3, 5)).shape == (48, 80)


def test_sentinels_stay():
    """Rows of sentinel bytes behind hist, lut and dst: no kernel writes past its output."""
    from adipose_amd._lib import call, ptr, stream_ptr
    ct = CT()
    for shape, grid in (((3, 67, 64), (8, 8)), ((2, 64, 96), (4, 2)), ((1, 5, SLAB_COLS + 17), (1, 1))):
        N, H, W = shape
        tx, ty = grid
        _, _, th, tw = ct.clahe_geometry(H, W, grid)
        img = image("random", shape)
        d = dev(img)
        nh, extra = N * ty * tx * 256, 4096
        hist = torch.full((nh + extra,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        call("adp_clahe_hist", N, H, W, ptr(d), 0, ty, tx, ptr(hist), stream_ptr())
        assert (hist[nh:] == 0x5A5A5A5A).all()
        assert np.array_equal(u32(hist[:nh]).reshape(N, ty, tx, 256), ct.clahe_hist_np(img, grid))
        lut = torch.full((nh + extra,), 0xA5, dtype=torch.uint8, device="cuda")
        call("adp_clahe_lut", N, ty, tx, th * tw, 2.0, ptr(hist), ptr(lut), stream_ptr())
        assert (lut[nh:] == 0xA5).all()
        for f32 in (0, 1):
            dst = torch.full((img.size + 4 * W,), 0xA5 if not f32 else -7, dtype=torch.float32 if f32 else torch.uint8,
                             device="cuda")
            call("adp_clahe_apply", N, H, W, ptr(d), 0, ty, tx, ptr(lut), ptr(dst), f32, stream_ptr())
            assert (dst[img.size:] == (-7 if f32 else 0xA5)).all()
            assert np.array_equal(dst[:img.size].cpu().numpy().reshape(shape), ct.clahe_np(img, 2.0, grid).astype(np.float32 if f32 else np.uint8))


def test_argument_errors():
    """Every bad argument returns non-zero with a message and leaves the output as it was. The checks run on the host
    before any launch: nothing is sent to the device."""
    from adipose_amd._lib import AdpError, call, ptr, stream_ptr
    ct = CT()
    img = dev(image("random", (2, 64, 96)))
    hist = torch.full((2, 8, 8, 256), 7, dtype=torch.int32, device="cuda")
    lut = torch.full((2, 8, 8, 256), 7, dtype=torch.uint8, device="cuda")
    dst = torch.full((2, 64, 96), 7, dtype=torch.uint8, device="cuda")
    sums = torch.full((2, 5), 7, dtype=torch.int64, device="cuda")
    out = torch.full((2, 64 * 96), 7.0, dtype=torch.float32, device="cuda")
    s = stream_ptr()
    bad = [
        ("non-null", "adp_clahe_hist", (2, 64, 96, None, 0, 8, 8, ptr(hist), s)),
        ("non-null", "adp_clahe_hist", (2, 64, 96, ptr(img), 0, 8, 8, None, s)),
        ("grid", "adp_clahe_hist", (2, 64, 96, ptr(img), 0, 0, 8, ptr(hist), s)),
        ("grid", "adp_clahe_hist", (2, 64, 96, ptr(img), 0, 8, 65, ptr(hist), s)),
        ("too small", "adp_clahe_hist", (2, 3, 96, ptr(img), 0, 8, 8, ptr(hist), s)),
        ("N must", "adp_clahe_hist", (0, 64, 96, ptr(img), 0, 8, 8, ptr(hist), s)),
        ("non-null", "adp_clahe_lut", (2, 8, 8, 96, 2.0, None, ptr(lut), s)),
        ("non-null", "adp_clahe_lut", (2, 8, 8, 96, 2.0, ptr(hist), None, s)),
        ("grid", "adp_clahe_lut", (2, 65, 8, 96, 2.0, ptr(hist), ptr(lut), s)),
        ("grid", "adp_clahe_lut", (2, 8, 0, 96, 2.0, ptr(hist), ptr(lut), s)),
        ("area", "adp_clahe_lut", (2, 8, 8, 0, 2.0, ptr(hist), ptr(lut), s)),
        ("finite", "adp_clahe_lut", (2, 8, 8, 96, float("inf"), ptr(hist), ptr(lut), s)),
        ("non-null", "adp_clahe_apply", (2, 64, 96, None, 0, 8, 8, ptr(lut), ptr(dst), 0, s)),
        ("non-null", "adp_clahe_apply", (2, 64, 96, ptr(img), 0, 8, 8, None, ptr(dst), 0, s)),
        ("non-null", "adp_clahe_apply", (2, 64, 96, ptr(img), 0, 8, 8, ptr(lut), None, 0, s)),
        ("grid", "adp_clahe_apply", (2, 64, 96, ptr(img), 0, 65, 8, ptr(lut), ptr(dst), 0, s)),
        ("grid", "adp_clahe_apply", (2, 64, 96, ptr(img), 0, 8, 0, ptr(lut), ptr(dst), 0, s)),
        ("too small", "adp_clahe_apply", (2, 64, 4, ptr(img), 0, 8, 8, ptr(lut), ptr(dst), 0, s)),
        ("non-null", "adp_gray_stats", (2, 64, 96, None, 0, ptr(sums), s)),
        ("non-null", "adp_gray_stats", (2, 64, 96, ptr(img), 0, None, s)),
        ("at least 2", "adp_gray_stats", (2, 1, 96, ptr(img), 0, ptr(sums), s)),
        ("at least 2", "adp_gray_stats", (2, 64, 1, ptr(img), 0, ptr(sums), s)),
        ("non-null", "adp_u8_stretch", (2, 64 * 96, None, ptr(hist), 5.0, 95.0, 0, ptr(out), s)),
        ("non-null", "adp_u8_stretch", (2, 64 * 96, ptr(img), None, 5.0, 95.0, 0, ptr(out), s)),
        ("non-null", "adp_u8_stretch", (2, 64 * 96, ptr(img), ptr(hist), 5.0, 95.0, 0, None, s)),
        ("mode", "adp_u8_stretch", (2, 64 * 96, ptr(img), ptr(hist), 5.0, 95.0, 2, ptr(out), s)),
        ("percentiles", "adp_u8_stretch", (2, 64 * 96, ptr(img), ptr(hist), -1.0, 95.0, 0, ptr(out), s)),
    ]
    for match, name, args in bad:
        with pytest.raises(AdpError, match=match):
            call(name, *args)
    torch.cuda.synchronize()
    assert (hist == 7).all() and (lut == 7).all() and (dst == 7).all() and (sums == 7).all() and (out == 7).all()
    # the module refuses the same before it reaches the library
    with pytest.raises(ValueError):
        ct.clahe(img, 2.0, (65, 8))
    with pytest.raises(ValueError):
        ct.clahe(img[:, :3], 2.0, (8, 8))
    with pytest.raises(ValueError):
        ct.clahe(img[None], 2.0, (8, 8))            # 4-D
    with pytest.raises(TypeError):
        ct.clahe(img.to(torch.int32), 2.0, (8, 8))
    with pytest.raises(ValueError):
        ct.gray_stats(img[:, :1])
    with pytest.raises(TypeError):
        ct.clahe_lut(lut, 96, 2.0)                  # not a histogram
    with pytest.raises(ValueError):
        ct.clahe_apply(img, lut[:1], (8, 8))        # tables of another batch


@pytest.mark.parametrize("shape", [(1, 2, 2), (3, 7, 9), (2, 64, 96)], ids=case_id)
def test_gray_stats(shape):
    ct = CT()
    for kind in ("random", "histology", "const77", "ramp"):
        img = image(kind, shape)
        want = ct.gray_stats_np(img)
        got = ct.gray_stats(dev(img))
        assert got.dtype == torch.int64 and tuple(got.shape) == (shape[0], 5)
        assert np.array_equal(got.cpu().numpy(), want), kind
        assert np.array_equal(ct.gray_stats(dev(img).float()).cpu().numpy(), want), kind
    assert ct.quality_class(ct.gray_stats(dev(image("random", shape)))) == ct.quality_class(ct.gray_stats_np(image("random", shape)))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", [(3, 30, 31), (2, 64, 96)], ids=case_id)
def test_u8_stretch(shape, mode):
    """Bit-equal to the module's numpy path, and within float32 rounding of the float64 formula written with
    np.percentile: the quotient is formed in float64 (a few ulp of 255 / den) and rounded to float32 once (half an ulp of
    a value up to 1, 2^-25)."""
    ct = CT()
    for kind in ("random", "histology", "two"):
        img = image(kind, shape)
        d = dev(img)
        for p in ((5, 95), (2, 98), (1, 99), (0, 100)):
            got = ct.u8_stretch(d, p[0], p[1], mode)
            assert got.dtype == torch.float32 and got.shape == d.shape
            g = got.cpu().numpy()
            assert np.array_equal(g, ct.u8_stretch_np(img, p[0], p[1], mode)), (kind, p)
            for n in range(shape[0]):
                v = img[n].astype(np.float64)
                lo, hi = np.percentile(v, p)
                den = (hi - lo) + 1e-3 if mode == 0 else max(hi - lo, 1e-3)
                want = np.clip((v - lo) / den, 0, 1)
                assert np.abs(g[n] - want).max() <= 2.0 ** -25 + 8 * 2.0 ** -53 * 255 / den, (kind, p, n)
    flat = dev(np.full(shape, 9, np.uint8))   # hi == lo: den = 1e-3 either way, every pixel 0
    assert (ct.u8_stretch(flat, 5, 95, mode) == 0).all()
    step = np.full(shape, 9, np.uint8)
    step[:, 0, 0] = 10                        # still hi == lo; the one brighter pixel is (10 - 9) / 1e-3, clipped to 1
    got = ct.u8_stretch(dev(step), 5, 95, mode)
    assert np.array_equal(got.cpu().numpy(), ct.u8_stretch_np(step, 5, 95, mode)) and (got[:, 0, 0] == 1).all()


def class_images():
    rng = np.random.default_rng(17)
    yy, xx = np.mgrid[0:96, 0:96]
    poor = np.clip(200 + rng.normal(0, 8, (96, 96)), 0, 255).astype(np.uint8)
    medium = np.clip(40 + 2.0 * xx + 0.2 * yy, 0, 255).astype(np.uint8)
    good = rng.integers(0, 256, (96, 96), dtype=np.uint8)
    return np.stack([good, poor, medium, poor, good])


def test_adaptive_normalization():
    ct = CT()
    batch = class_images()
    assert ct.quality_class(ct.gray_stats_np(batch)) == ["good", "poor", "medium", "poor", "good"]
    want = ct.adaptive_clahe_normalization_np(batch)
    got = ct.adaptive_clahe_normalization(dev(batch))
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == (5, 96, 96)
    assert np.array_equal(got.cpu().numpy(), want)
    one = ct.adaptive_clahe_normalization(dev(batch[2]))
    assert one.shape == (96, 96) and np.array_equal(one.cpu().numpy(), want[2])
    host = ct.adaptive_clahe_normalization(batch[1])    # a host array goes through the device and comes back
    assert isinstance(host, np.ndarray) and np.array_equal(host, want[1])


def test_surface():
    ct = CT()
    rng = np.random.default_rng(6)
    rgb = rng.integers(0, 256, (40, 48, 3), dtype=np.uint8)
    want = np.stack([ct.clahe_np(np.ascontiguousarray(rgb[..., c]), 2.0, (8, 8)) for c in range(3)], axis=-1)
    got = ct.enhance_clahe(rgb)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want)
    got = ct.enhance_clahe(dev(rgb))
    assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    cl = ct.Clahe(2.0, 8)
    assert np.array_equal(cl(dev(rgb[..., 0])).cpu().numpy(), want[..., 0])
    f = cl(dev(rgb[..., 0]).float())
    assert f.dtype == torch.float32 and np.array_equal(f.cpu().numpy(), want[..., 0].astype(np.float32))
    assert np.array_equal(cl(rgb[..., 1].astype(np.float32)), want[..., 1].astype(np.float32))
    t = cl(torch.from_numpy(np.ascontiguousarray(rgb[..., 2])))
    assert not t.is_cuda and np.array_equal(t.numpy(), want[..., 2])


# ---------------------------------------------------------------- predictor
S = 64   # the smallest tile the predictor tests use


def gray_tile(seed, shape=(S, S)):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    g = 150 + 50 * np.sin(yy / 9.0 + seed) * np.cos(xx / 6.0) + rng.normal(0, 12, shape)
    return np.clip(np.rint(g), 0, 255).astype(np.float32)


@pytest.fixture(scope="module")
def net():
    from adipose_amd.nets import AdiposeV3Net
    from oracle import torch_ref as R
    n = AdiposeV3Net(1, S, dtype="f32", device="cuda", deep_supervision=False)
    n.set_weights(R.adipose_v3_keras_weights(seed=865, deep_supervision=False))
    return n


def test_predictor_contrast(net):
    from adipose_amd.predictor import HipUnetPredictor
    ct = CT()
    cl = ct.Clahe(2.0, 8)
    tiles = [gray_tile(s) for s in (1, 2, 3)]
    plain = HipUnetPredictor(net, max_batch=8)
    for views in ([0], [0, 4, 5, 1]):
        want = plain.predict_views([ct.clahe_np(t, 2.0, (8, 8), np.float32) for t in tiles], 120.0, 40.0, views).clone()
        got = HipUnetPredictor(net, max_batch=8, contrast=cl).predict_views(tiles, 120.0, 40.0, views).clone()
        assert torch.equal(got, want)
        off = plain.predict_views(tiles, 120.0, 40.0, views).clone()
        assert not torch.equal(off, want)     # the enhancement changes the prediction
        # contrast=None: the same bits as a predictor built without the keyword
        assert torch.equal(HipUnetPredictor(net, max_batch=8, contrast=None).predict_views(tiles, 120.0, 40.0, views), off)
        assert torch.equal(HipUnetPredictor(net, max_batch=8, contrast=cl).predict_views(tiles, 120.0, 40.0, views,
                                                                                         enhance=False), off)
    rgb_net = types.SimpleNamespace(device=net.device, in_ch=3)
    with pytest.raises(ValueError, match="1-channel"):
        HipUnetPredictor(rgb_net, contrast=cl).predict_views(tiles, 120.0, 40.0, [0])


def test_cli_enhance_contrast(tmp_path, capsys):
    """--enhance-contrast on gray tiles writes what the plain run writes for the same tiles enhanced on the host, and
    names the enhancement in its header; without the flag the header does not mention it."""
    from PIL import Image

    from adipose_amd.checkpoint import save_weights
    from cli.segmentation_inference import main
    from oracle import torch_ref as R
    ct = CT()
    for d in ("raw", "enhanced", "ck"):
        (tmp_path / d).mkdir()
    for name, seed in (("a", 21), ("b", 22)):
        g = gray_tile(seed).astype(np.uint8)
        e = ct.clahe_np(g, 3.0, (16, 16))
        assert (e != g).any()
        # R = G = B = g: PIL's gray of it is g again, so read_gray returns the plane that was written
        Image.fromarray(np.stack([g, g, g], axis=-1)).save(tmp_path / "raw" / f"{name}.png")
        Image.fromarray(np.stack([e, e, e], axis=-1)).save(tmp_path / "enhanced" / f"{name}.png")
    save_weights(None, tmp_path / "ck" / "phase2_best.weights.h5",
                 weights=R.adipose_v3_keras_weights(seed=5, deep_supervision=False))
    (tmp_path / "ck" / "normalization_stats.json").write_text('{"mean": 120.0, "std": 40.0}')
    out = {}
    for run, images, extra in (("on", "raw", ["--enhance-contrast"]), ("host", "enhanced", []), ("off", "raw", [])):
        assert main(["--images-dir", str(tmp_path / images), "--weights", str(tmp_path / "ck"), "--tile", str(S),
                     "--output-dir", str(tmp_path / run), "--save-probability"] + extra) == 0
        said = capsys.readouterr().out
        assert ("CLAHE clip limit 3, 16 x 16 tiles" in said) == (run == "on")
        out[run] = {n: (np.array(Image.open(tmp_path / run / "masks" / f"{n}_mask.tif")),
                        np.array(Image.open(tmp_path / run / "probabilities" / f"{n}_prob.tif"))) for n in ("a", "b")}
    for n in ("a", "b"):
        assert np.array_equal(out["on"][n][0], out["host"][n][0]) and np.array_equal(out["on"][n][1], out["host"][n][1])
    assert any((out["on"][n][1] != out["off"][n][1]).any() for n in ("a", "b"))
    assert main(["--images-dir", str(tmp_path / "raw"), "--weights", str(tmp_path / "ck"), "--tile", str(S),
                 "--output-dir", str(tmp_path / "bad"), "--enhance-contrast", "--clahe-tile-size", "65"]) == 1


def test_sliding_window_enhances_the_whole_image_once(net):
    from adipose_amd.predictor import HipUnetPredictor, SlidingWindowInference
    ct = CT()
    cl = ct.Clahe(3.0, 4)
    img = gray_tile(7, (96, 160))
    sw = SlidingWindowInference(S, 0.5, "gaussian", verbose=False)
    got = sw.predict_with_sliding_window(img, HipUnetPredictor(net, max_batch=8, contrast=cl), 120.0, 40.0)
    whole = ct.clahe_np(img, 3.0, (4, 4), np.float32)
    plain = HipUnetPredictor(net, max_batch=8)
    want = sw.predict_with_sliding_window(whole, plain, 120.0, 40.0)
    assert np.array_equal(got, want)
    per_tile = sw.predict_with_sliding_window(img, plain, 120.0, 40.0)
    assert not np.array_equal(per_tile, want)
