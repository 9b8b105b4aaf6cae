"""Gray-scale morphology and the background corrections on the device (csrc/graymorph.hip) against the numpy path of
adipose_amd.illumination, bit for bit: every comparison is equality, there is no tolerance. The numpy path itself is
pinned to oracle/numpy_ref.py's cv_morph, to scipy and to brute-force loops in tests/test_illumination.py.

Shapes sit around the block's tile (TR x TC output pixels), the staging round (4 input rows) and the dword the levels are
built in: 1-pixel planes, widths 63 / 64 / 65, one tile exactly, one pixel more, several tiles with ragged edges.
Footprints cover every level count (row lengths 1 .. 513), even sizes (asymmetric offsets), boxes that are not square,
empty rows, and footprints larger than the image and than a tile.
"""
import os
import re
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def IL():
    from adipose_amd import illumination
    return illumination


from adipose_amd.illumination import TILE_COLS as TC, TILE_ROWS as TR, KMAX  # noqa: E402

SHAPES = [(1, 1, 1), (1, 1, 7), (1, 9, 1), (2, 5, 63), (1, 5, 64), (1, 5, 65), (3, 37, 53), (1, 257, 131),
          (1, TR, TC), (1, TR + 1, TC + 1), (2, 2 * TR - 1, 2 * TC + 3)]
BIG_SHAPES = [(1, 70, 333), (1, 320, 310), (2, TR + 1, TC + 1)]
OPS = ["erode", "dilate", "open", "close", "tophat", "blackhat"]
KINDS = ["random", "zeros", "white", "blobs"]


def footprints():
    il = IL()
    fps = [(f"ellipse{k}", il.ellipse_rows(k)) for k in (1, 2, 3, 4, 5, 16, 31, 64, 65)]
    fps += [(f"disc{r}", il.disc_rows(r)) for r in (1, 7)]
    fps += [(f"rect{kh}x{kw}", il.rect_rows(kh, kw)) for kh, kw in ((9, 1), (8, 1), (1, 6), (3, 5), (16, 16))]
    fps.append(("holes", ([0, 3, 0, 6, 2, 0], [2, 3, 7, 9, 2, 1], 9)))   # empty rows, rows off centre, a wide box
    return fps


def big_footprints():
    il = IL()
    return [("ellipse301", il.ellipse_rows(301)), ("disc100", il.disc_rows(100)), ("line512", il.rect_rows(512, 1)),
            ("kmax_rows", il.rect_rows(KMAX, 1)), ("kmax_cols", il.rect_rows(1, KMAX))]


def case_id(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)


def image(kind, shape, seed=0):
    rng = np.random.default_rng([KINDS.index(kind), seed, *shape])
    if kind == "zeros":
        return np.zeros(shape, np.uint8)
    if kind == "white":
        return np.full(shape, 255, np.uint8)
    if kind == "blobs":   # a smooth ramp with dark blobs: what the corrections are for
        yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
        g = 120 + 100 * (yy / max(shape[0] - 1, 1)) * (xx / max(shape[1] - 1, 1)) + rng.normal(0, 3, shape)
        for _ in range(1 + min(shape[0] * shape[1] // 400, 300)):
            cy, cx, r = int(rng.integers(0, shape[0])), int(rng.integers(0, shape[1])), int(rng.integers(1, 6))
            y1, x1 = max(cy - r, 0), max(cx - r, 0)
            win = g[y1:cy + r + 1, x1:cx + r + 1]
            win[(yy[y1:cy + r + 1, x1:cx + r + 1] - cy) ** 2 + (xx[y1:cy + r + 1, x1:cx + r + 1] - cx) ** 2 <= r * r] -= 80
        return np.clip(np.rint(g), 0, 255).astype(np.uint8)
    img = rng.integers(0, 256, size=shape, dtype=np.uint8)   # full range, 0 and 255 present
    flat = img.reshape(-1)
    flat[rng.integers(0, flat.size)] = 0
    flat[rng.integers(0, flat.size)] = 255
    return img


def batch(shape, kinds=("random", "blobs", "random")):
    """(N, H, W): image n of kind kinds[n % len(kinds)], every one different."""
    return np.stack([image(kinds[n % len(kinds)], shape[1:], n) for n in range(shape[0])])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_ops(img, fps, ops=OPS):
    il = IL()
    d = dev(img)
    for name, rows in fps:
        for op in ops:
            got = getattr(il, op)(d, rows)
            assert got.dtype == torch.uint8 and got.shape == d.shape
            want = getattr(il, op + "_np")(img, rows)
            assert np.array_equal(got.cpu().numpy(), want), (name, op, img.shape)


def test_tile_constants():
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "adipose_hip.h")).read()
    val = {k: int(v) for k, v in re.findall(r"#define (ADP_GMORPH_\w+) (\d+)", hdr)}
    assert (val["ADP_GMORPH_TILE_ROWS"], val["ADP_GMORPH_TILE_COLS"], val["ADP_GMORPH_KMAX"]) == (TR, TC, KMAX)
    assert KMAX >= 513


@pytest.mark.parametrize("shape", SHAPES, ids=case_id)
def test_ops_equal_numpy(shape):
    check_ops(batch(shape), footprints())


@pytest.mark.parametrize("shape", BIG_SHAPES, ids=case_id)
def test_large_footprints_equal_numpy(shape):
    check_ops(batch(shape), big_footprints())


def test_full_size_opening():
    il = IL()
    img = image("blobs", (1024, 1024))[None]
    rows = il.ellipse_rows(301)
    assert np.array_equal(il.open(dev(img), rows).cpu().numpy(), il.open_np(img, rows))


@pytest.mark.parametrize("shape", [(4, 37, 53), (4, TR + 1, TC + 1)], ids=case_id)
def test_kinds_and_dtypes(shape):
    """A batch whose images differ in kind; uint8 and float32 in, uint8 and float32 out."""
    il = IL()
    img = batch(shape, KINDS)
    f = img.astype(np.float32)
    f[0] += np.where(np.arange(shape[2]) % 2 == 0, 0.25, -0.25).astype(np.float32)   # rounds back to img
    f[0, 0, :4] = [-3.0, 300.0, 0.5, 1.5][:min(4, shape[2])]
    u = np.clip(np.rint(f), 0, 255).astype(np.uint8)
    assert (u[1:] == img[1:]).all()
    for name, rows in (("ellipse5", il.ellipse_rows(5)), ("ellipse64", il.ellipse_rows(64)), ("rect3x5", il.rect_rows(3, 5))):
        for op in OPS:
            want = getattr(il, op + "_np")(u, rows)
            for src in (dev(u), dev(f)):
                got = getattr(il, op)(src, rows)
                assert got.dtype == src.dtype and np.array_equal(got.cpu().numpy(), want.astype(got.cpu().numpy().dtype)), (name, op)
                for dt, npdt in ((torch.uint8, np.uint8), (torch.float32, np.float32)):
                    got = getattr(il, op)(src, rows, dt)
                    assert got.dtype == dt and np.array_equal(got.cpu().numpy(), want.astype(npdt)), (name, op, dt)
    # constant planes keep their borders
    assert (il.erode(dev(img[2:3]), il.ellipse_rows(31)) == 255).all()
    assert (il.dilate(dev(img[1:2]), il.ellipse_rows(31)) == 0).all()
    # an empty footprint
    empty = ([1, 0, 2], [1, 0, 2])
    assert (il.erode(dev(img), empty) == 255).all() and (il.dilate(dev(img), empty) == 0).all()


def sum_past_2_24():
    """(1, 300, 300) whose opening by the 3-disc is 255 almost everywhere: the background's sum passes 2^24."""
    img = np.full((1, 300, 300), 255, np.uint8)
    img[0, 100:140, 60:200] = image("random", (40, 140), 5)
    return img


@pytest.mark.parametrize("case", ["3x37x53", "1x320x310", "1x1024x1024", "sum"])
def test_corrections_equal_numpy(case):
    il = IL()
    if case == "sum":
        img = sum_past_2_24()
        params = dict(radius=3, width=1, height=12, ksize=9)
    elif case == "1x1024x1024":
        img = image("blobs", (1024, 1024))[None]
        params = dict(radius=100, width=1, height=512, ksize=301)
    else:
        shape = tuple(int(v) for v in case.split("x"))
        img = batch(shape, ("blobs", "random", "white"))
        params = dict(radius=7, width=1, height=12, ksize=31) if shape[1] < 100 else dict(radius=100, width=1, height=512, ksize=301)
    d = dev(img)
    bg = il.open_np(img, il.disc_rows(params["radius"]))
    want = {"rb": il.subtract_background_np(img, bg),
            "band": il.remove_banding_morphological_np(img, params["width"], params["height"]),
            "th": il.tophat_correction_np(img, params["ksize"])}
    got = {"rb": il.rolling_ball(d, params["radius"]),
           "band": il.remove_banding_morphological(d, params["width"], params["height"]),
           "th": il.tophat_correction(d, params["ksize"])}
    if case == "sum":
        assert int(bg.sum(dtype=np.int64)) > 1 << 24
    for k in want:
        assert got[k].dtype == torch.uint8 and np.array_equal(got[k].cpu().numpy(), want[k]), k
    # float32 in and out: the same integers
    f = il.rolling_ball(d.float(), params["radius"])
    assert f.dtype == torch.float32 and np.array_equal(f.cpu().numpy(), want["rb"].astype(np.float32))
    f = il.tophat_correction(d, params["ksize"], torch.float32)
    assert f.dtype == torch.float32 and np.array_equal(f.cpu().numpy(), want["th"].astype(np.float32))
    # the background's sum and the subtraction on their own
    assert np.array_equal(il.background_sum(dev(bg)).cpu().numpy(), bg.reshape(bg.shape[0], -1).sum(axis=1, dtype=np.int64))
    assert np.array_equal(il.subtract_background(d, dev(bg)).cpu().numpy(), il.subtract_background_np(img, bg))


def test_surface():
    """Arrays in, arrays out; tensors in, tensors out where they were; the input's dtype."""
    il = IL()
    img = batch((2, 37, 53), ("blobs", "random"))
    c = il.IlluminationCorrection(banding=(1, 12), method="rolling-ball", radius=7)
    want = il.rolling_ball_np(il.remove_banding_morphological_np(img, 1, 12), 7)
    got = c(img)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want)
    got = c(img.astype(np.float32))
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32))
    got = c(dev(img))
    assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    got = c(torch.from_numpy(img))
    assert not got.is_cuda and np.array_equal(got.numpy(), want)
    got = il.IlluminationCorrection(method="tophat", kernel_size=30)(dev(img[0]).float())
    assert got.shape == (37, 53) and np.array_equal(got.cpu().numpy(), il.tophat_correction_np(img[0], 31, np.float32))


def test_streams_and_back_to_back_calls():
    il = IL()
    img = batch((2, TR + 1, TC + 1))
    d = dev(img)
    rows = il.ellipse_rows(31)
    want_o, want_rb = il.open_np(img, rows), il.rolling_ball_np(img, 7)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        a = il.open(d, rows)
        b = il.rolling_ball(d, 7)
        c = il.open(d, rows)
    st.synchronize()
    assert np.array_equal(a.cpu().numpy(), want_o) and np.array_equal(c.cpu().numpy(), want_o)
    assert np.array_equal(b.cpu().numpy(), want_rb)
    # independent of the batch and of the run
    for n in range(2):
        assert torch.equal(il.open(d[n], rows), a[n])


def test_sentinels_stay():
    """Sentinel bytes behind dst: no kernel writes past its output."""
    from adipose_amd._lib import call, ptr, stream_ptr
    import ctypes as C
    il = IL()
    for shape in ((2, TR + 1, TC + 1), (1, 5, 65), (3, 37, 53)):
        N, H, W = shape
        img = batch(shape)
        d = dev(img)
        lo, hi = il.ellipse_rows(31)
        for op, ref in ((il.ERODE, il.erode_np), (il.DILATE, il.dilate_np)):
            dst = torch.full((img.size + 4 * W + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            call("adp_gray_morph", N, H, W, ptr(d), 0, ptr(dst), 31, 31, (C.c_int * 31)(*lo), (C.c_int * 31)(*hi), op, stream_ptr())
            assert (dst[img.size:] == 0xA5).all()
            assert np.array_equal(dst[:img.size].cpu().numpy().reshape(shape), ref(img, (lo, hi)))
        bg = dev(il.open_np(img, (lo, hi)))
        sums = torch.full((N + 8,), 7, dtype=torch.int64, device="cuda")
        call("adp_gray_bgsum", N, H, W, ptr(bg), ptr(sums), stream_ptr())
        assert (sums[N:] == 7).all()
        for f32 in (0, 1):
            dst = torch.full((img.size + 4 * W,), -7 if f32 else 0xA5, dtype=torch.float32 if f32 else torch.uint8, device="cuda")
            call("adp_illum_finish", N, H, W, ptr(d), 0, ptr(bg), ptr(sums), il.SUBTRACT_MEAN, ptr(dst), f32, stream_ptr())
            assert (dst[img.size:] == (-7 if f32 else 0xA5)).all()
            assert np.array_equal(dst[:img.size].cpu().numpy().reshape(shape),
                                  il.subtract_background_np(img, bg.cpu().numpy(), np.float32 if f32 else np.uint8))


def test_argument_errors():
    """Every bad argument returns non-zero with a message and leaves the output as it was. The checks run on the host
    before any launch: nothing is sent to the device."""
    import ctypes as C

    from adipose_amd._lib import AdpError, call, ptr, stream_ptr
    il = IL()
    img = dev(batch((2, 64, 96)))
    dst = torch.full((2, 64, 96), 7, dtype=torch.uint8, device="cuda")
    dstf = torch.full((2, 64, 96), 7.0, dtype=torch.float32, device="cuda")
    sums = torch.full((2,), 7, dtype=torch.int64, device="cuda")
    s = stream_ptr()

    def arr(v):
        return (C.c_int * len(v))(*v)

    lo, hi = arr([0, 0, 0]), arr([3, 3, 3])
    big = arr([0] * (KMAX + 1)), arr([1] * (KMAX + 1))
    bad = [
        ("non-null", "adp_gray_morph", (2, 64, 96, None, 0, ptr(dst), 3, 3, lo, hi, 0, s)),
        ("non-null", "adp_gray_morph", (2, 64, 96, ptr(img), 0, None, 3, 3, lo, hi, 0, s)),
        ("non-null", "adp_gray_morph", (2, 64, 96, ptr(img), 0, ptr(dst), 3, 3, None, hi, 0, s)),
        ("non-null", "adp_gray_morph", (2, 64, 96, ptr(img), 0, ptr(dst), 3, 3, lo, None, 0, s)),
        ("N must", "adp_gray_morph", (-1, 64, 96, ptr(img), 0, ptr(dst), 3, 3, lo, hi, 0, s)),
        ("N must", "adp_gray_morph", (2, 0, 96, ptr(img), 0, ptr(dst), 3, 3, lo, hi, 0, s)),
        ("N must", "adp_gray_morph", (2, 64, 0, ptr(img), 0, ptr(dst), 3, 3, lo, hi, 0, s)),
        ("1 .. 513", "adp_gray_morph", (2, 64, 96, ptr(img), 0, ptr(dst), 0, 3, lo, hi, 0, s)),
        ("1 .. 513", "adp_gray_morph", (2, 64, 96, ptr(img), 0, ptr(dst), 3, 0, lo, hi, 0, s)),
        ("1 .. 513", "adp_gray_morph", (2, 64, 96, ptr(img), 0, ptr(dst), KMAX + 1, 1, big[0], big[1], 0, s)),
        ("1 .. 513", "adp_gray_morph", (2, 64, 96, ptr(img), 0, ptr(dst), 3, KMAX + 1, lo, hi, 0, s)),
        ("bad footprint", "adp_gray_morph", (2, 64, 96, ptr(img), 0, ptr(dst), 3, 3, arr([0, -1, 0]), hi, 0, s)),
        ("bad footprint", "adp_gray_morph", (2, 64, 96, ptr(img), 0, ptr(dst), 3, 3, lo, arr([3, 4, 3]), 0, s)),
        ("bad footprint", "adp_gray_morph", (2, 64, 96, ptr(img), 0, ptr(dst), 3, 3, arr([0, 2, 0]), arr([3, 1, 3]), 0, s)),
        ("op must", "adp_gray_morph", (2, 64, 96, ptr(img), 0, ptr(dst), 3, 3, lo, hi, 2, s)),
        ("overlap", "adp_gray_morph", (2, 64, 96, ptr(dst), 0, ptr(dst), 3, 3, lo, hi, 0, s)),
        ("overlap", "adp_gray_morph", (1, 64, 96, ptr(dst), 0, C.c_void_p(dst.data_ptr() + 64 * 96 - 1), 3, 3, lo, hi, 0, s)),
        ("non-null", "adp_gray_bgsum", (2, 64, 96, None, ptr(sums), s)),
        ("non-null", "adp_gray_bgsum", (2, 64, 96, ptr(img), None, s)),
        ("N must", "adp_gray_bgsum", (-1, 64, 96, ptr(img), ptr(sums), s)),
        ("N must", "adp_gray_bgsum", (2, 64, 0, ptr(img), ptr(sums), s)),
        ("non-null", "adp_illum_finish", (2, 64, 96, None, 0, ptr(img), ptr(sums), 0, ptr(dst), 0, s)),
        ("non-null", "adp_illum_finish", (2, 64, 96, ptr(img), 0, None, ptr(sums), 0, ptr(dst), 0, s)),
        ("non-null", "adp_illum_finish", (2, 64, 96, ptr(img), 0, ptr(img), ptr(sums), 0, None, 0, s)),
        ("needs sums", "adp_illum_finish", (2, 64, 96, ptr(img), 0, ptr(img), None, 0, ptr(dst), 0, s)),
        ("mode must", "adp_illum_finish", (2, 64, 96, ptr(img), 0, ptr(img), ptr(sums), 3, ptr(dst), 0, s)),
        ("N must", "adp_illum_finish", (2, 0, 96, ptr(img), 0, ptr(img), ptr(sums), 0, ptr(dst), 0, s)),
        ("overlap", "adp_illum_finish", (2, 64, 96, ptr(dst), 0, ptr(img), ptr(sums), 0, ptr(dst), 0, s)),
        ("overlap", "adp_illum_finish", (2, 64, 96, ptr(img), 0, ptr(dst), ptr(sums), 0, ptr(dst), 0, s)),
        ("overlap", "adp_illum_finish", (2, 64, 96, ptr(img), 0, ptr(img), ptr(sums), 0, ptr(img), 1, s)),
    ]
    before = img.clone()
    for match, name, args in bad:
        with pytest.raises(AdpError, match=match):
            call(name, *args)
    torch.cuda.synchronize()
    assert (dst == 7).all() and (dstf == 7).all() and (sums == 7).all() and torch.equal(img, before)
    # the module refuses the same before it reaches the library
    with pytest.raises(ValueError):
        il.erode(img, ([0], [2]))
    with pytest.raises(ValueError):
        il.erode(img[None], il.ellipse_rows(3))            # 4-D
    with pytest.raises(TypeError):
        il.erode(img.to(torch.int32), il.ellipse_rows(3))
    with pytest.raises(TypeError):
        il.erode(img, il.ellipse_rows(3), torch.int32)
    with pytest.raises(ValueError):
        il.subtract_background(img, img[:1])
    with pytest.raises(TypeError):
        il.background_sum(img.float())
    with pytest.raises(ValueError):
        il.rolling_ball(img, KMAX)


# ---------------------------------------------------------------- predictor
S = 64   # the smallest tile the predictor tests use


def gray_tile(seed, shape=(S, S)):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    g = 100 + 90 * (yy / shape[0]) + 40 * np.sin(yy / 9.0 + seed) * np.cos(xx / 6.0) + rng.normal(0, 12, shape)
    return np.clip(np.rint(g), 0, 255).astype(np.float32)


@pytest.fixture(scope="module")
def net():
    from adipose_amd.nets import AdiposeV3Net
    from oracle import torch_ref as R
    n = AdiposeV3Net(1, S, dtype="f32", device="cuda", deep_supervision=False)
    n.set_weights(R.adipose_v3_keras_weights(seed=865, deep_supervision=False))
    return n


def host_corrected(il, t, dtype=np.float32):
    return il.rolling_ball_np(il.remove_banding_morphological_np(t, 1, 12), 7, dtype)


def test_predictor_illumination(net):
    from adipose_amd.contrast import Clahe, clahe_np
    from adipose_amd.predictor import HipUnetPredictor
    il = IL()
    ic = il.IlluminationCorrection(banding=(1, 12), method="rolling-ball", radius=7)
    tiles = [gray_tile(s) for s in (1, 2, 3)]
    plain = HipUnetPredictor(net, max_batch=8)
    for views in ([0], [0, 4, 5, 1]):
        want = plain.predict_views([host_corrected(il, t) for t in tiles], 120.0, 40.0, views).clone()
        got = HipUnetPredictor(net, max_batch=8, illumination=ic).predict_views(tiles, 120.0, 40.0, views).clone()
        assert torch.equal(got, want)
        off = plain.predict_views(tiles, 120.0, 40.0, views).clone()
        assert not torch.equal(off, want)     # the correction changes the prediction
        # illumination=None: the same bits as a predictor built without the keyword
        assert torch.equal(HipUnetPredictor(net, max_batch=8, illumination=None).predict_views(tiles, 120.0, 40.0, views), off)
        assert torch.equal(HipUnetPredictor(net, max_batch=8, illumination=ic).predict_views(tiles, 120.0, 40.0, views,
                                                                                             enhance=False), off)
    # before the contrast enhancement
    want = plain.predict_views([clahe_np(host_corrected(il, t), 2.0, (8, 8), np.float32) for t in tiles], 120.0, 40.0, [0]).clone()
    got = HipUnetPredictor(net, max_batch=8, contrast=Clahe(2.0, 8), illumination=ic).predict_views(tiles, 120.0, 40.0, [0])
    assert torch.equal(got, want)
    rgb_net = types.SimpleNamespace(device=net.device, in_ch=3)
    with pytest.raises(ValueError, match="1-channel"):
        HipUnetPredictor(rgb_net, illumination=ic).predict_views(tiles, 120.0, 40.0, [0])


def test_sliding_window_corrects_the_whole_image_once(net):
    from adipose_amd.predictor import HipUnetPredictor, SlidingWindowInference
    il = IL()
    ic = il.IlluminationCorrection(banding=(1, 12), method="rolling-ball", radius=7)
    img = gray_tile(7, (96, 160))
    sw = SlidingWindowInference(S, 0.5, "gaussian", verbose=False)
    got = sw.predict_with_sliding_window(img, HipUnetPredictor(net, max_batch=8, illumination=ic), 120.0, 40.0)
    whole = host_corrected(il, img)
    plain = HipUnetPredictor(net, max_batch=8)
    want = sw.predict_with_sliding_window(whole, plain, 120.0, 40.0)
    assert np.array_equal(got, want)
    # per tile the correction is another one: the windows' own backgrounds and means
    per_tile = np.zeros_like(whole)
    per_tile[:S, :S] = host_corrected(il, img[:S, :S])
    assert not np.array_equal(per_tile[:S, :S], whole[:S, :S])
