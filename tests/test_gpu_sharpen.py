"""The unsharp mask on the device (csrc/sharpen.hip) against the numpy path of adipose_amd.sharpen, bit for bit: every
comparison is equality, there is no tolerance, on the integer blur sum S (adp_gray_blur) and on the sharpened image
(adp_gray_sharpen). The numpy path itself is pinned to Python-int arithmetic and to the reference's formula in
tests/test_sharpen.py.

Shapes sit around the TR x TC tile a block makes: 1-pixel and few-pixel planes (the radius exceeds both extents and the
border folds many times), one pixel less and more than a tile, several tiles, a plane with a block whose halo lies
inside the image (the path without the fold), and a batch of 3 distinct images. Radii: 0 (the identity), 1, the default
4, F and F + 1 (the last fused radius and the first that takes two launches through the plane of row sums), and the
limit 64; sigma = r / 4 gives radius r.
"""
import functools
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from adipose_amd.sharpen import FUSED_RMAX as F, RMAX, TILE_COLS as TC, TILE_ROWS as TR  # noqa: E402

SHAPES = [(1, 1), (1, 7), (3, 5), (TR - 1, TC + 1), (TR + 1, 2 * TC + 3), (2 * TR + 5, TC - 1), (3 * TR + 5, 3 * TC + 7),
          (3, TR + 3, TC + 9)]
RADII = [0, 1, 4, F, F + 1, RMAX]


def SH():
    from adipose_amd import sharpen
    return sharpen


def sigma_of(r):
    return r / 4 if r else 0.01


def case_id(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)


def image(shape, seed=0):
    """Texture over the whole range, with a saturated corner and a dark one; the images of a batch differ."""
    rng = np.random.default_rng([seed, *shape])
    yy, xx = np.mgrid[0:shape[-2], 0:shape[-1]]
    g = 120 + 60 * np.sin(yy / 5.0) * np.cos(xx / 7.0) + rng.normal(0, 40, shape)
    a = np.clip(np.rint(g), 0, 255).astype(np.uint8)
    a[..., : shape[-2] // 4, : shape[-1] // 4] = 255
    a[..., shape[-2] - shape[-2] // 5:, shape[-1] - shape[-1] // 5:] = 0
    return a


@functools.lru_cache(maxsize=None)
def expected(shape, r, amount=0.5, seed=0):
    """(S, sharpened) by the numpy path, computed once per case and read-only."""
    sh = SH()
    img = image(shape, seed)
    S, out = sh.blur_sum_np(img, sigma_of(r)), sh.sharpen_np(img, sigma_of(r), amount)
    S.setflags(write=False)
    out.setflags(write=False)
    return S, out


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("shape", SHAPES, ids=case_id)
@pytest.mark.parametrize("r", RADII)
def test_device_equals_numpy(r, shape):
    """S and the image, uint8 and float32 on both sides: the four combinations hold the same integers."""
    sh = SH()
    sigma = sigma_of(r)
    assert sh.radius(sigma) == r
    img = image(shape)
    wantS, want = expected(shape, r)
    d8, d32 = dev(img), dev(img.astype(np.float32))
    for d in (d8, d32):
        S = sh.blur_sum(d, sigma)
        assert S.dtype == torch.int64 and tuple(S.shape) == img.shape and np.array_equal(S.cpu().numpy(), wantS)
    got = sh.sharpen(d8, sigma, 0.5)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    got = sh.sharpen(d32, sigma, 0.5)
    assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), want.astype(np.float32))
    assert np.array_equal(sh.sharpen(d8, sigma, 0.5, torch.float32).cpu().numpy(), want.astype(np.float32))
    assert np.array_equal(sh.sharpen(d32, sigma, 0.5, torch.uint8).cpu().numpy(), want)
    if r == 0:
        assert np.array_equal(want, img)


@pytest.mark.parametrize("r", [4, F + 1])
def test_batch_is_image_by_image(r):
    sh = SH()
    shape = SHAPES[-1]
    img = image(shape)
    assert not np.array_equal(img[0], img[1]) and not np.array_equal(img[1], img[2])
    got = sh.sharpen(dev(img), sigma_of(r), 0.7).cpu().numpy()
    for i in range(3):
        assert np.array_equal(got[i], sh.sharpen_np(img[i], sigma_of(r), 0.7))
    assert sh.sharpen(dev(img)[:0], sigma_of(r)).shape == (0,) + shape[1:]
    assert sh.blur_sum(dev(img)[:0], sigma_of(r)).shape == (0,) + shape[1:]


@pytest.mark.parametrize("amount", [0.0, -0.5, 2.5, 0.3])
@pytest.mark.parametrize("r", [4, F + 1])
def test_amounts(r, amount):
    sh = SH()
    shape = (TR + 1, 2 * TC + 3)
    want = expected(shape, r, amount)[1]
    assert np.array_equal(sh.sharpen(dev(image(shape)), sigma_of(r), amount).cpu().numpy(), want)
    if amount == 0.0:
        assert np.array_equal(want, image(shape))


@pytest.mark.parametrize("r", [4, F, F + 1, RMAX])
def test_unaligned_plane_and_sentinels(r):
    """A base pointer one byte off, for the source and for the destination, through the library: the bytes and words
    around each output stay as they were."""
    from adipose_amd._lib import call, ptr, stream_ptr
    sh = SH()
    shape = (TR + 1, 2 * TC + 3)
    H, W = shape
    img = image(shape)
    wantS, want = expected(shape, r)
    buf = torch.zeros(img.size + 64, dtype=torch.uint8, device="cuda")
    view = buf[1:1 + img.size].view(H, W)
    view.copy_(dev(img))
    assert view.data_ptr() % 16 == 1 and view.is_contiguous()
    assert np.array_equal(sh.sharpen(view, sigma_of(r), 0.5).cpu().numpy(), want)
    q = sh.taps(sigma_of(r))
    rb = torch.full((img.size + 16,), 7, dtype=torch.int32, device="cuda") if r > F else None
    rbp = ptr(rb[8:]) if r > F else None
    s = stream_ptr()
    for f32 in (0, 1):
        fill = -7 if f32 else 0xA5
        out = torch.full((img.size + 2 * W + 64,), fill, dtype=torch.float32 if f32 else torch.uint8, device="cuda")
        o = W + 31
        body = out[o:o + img.size]
        call("adp_gray_sharpen", 1, H, W, ptr(view), 0, sh._taps_arg(q), r, 0.5, rbp, ptr(body), f32, s)
        assert (out[:o] == fill).all() and (out[o + img.size:] == fill).all()
        assert np.array_equal(body.cpu().numpy().reshape(shape), want.astype(np.float32 if f32 else np.uint8))
    Sbuf = torch.full((img.size + 16,), -7, dtype=torch.int64, device="cuda")
    call("adp_gray_blur", 1, H, W, ptr(view), 0, sh._taps_arg(q), r, rbp, ptr(Sbuf[8:]), s)
    assert (Sbuf[:8] == -7).all() and (Sbuf[8 + img.size:] == -7).all()
    assert np.array_equal(Sbuf[8:8 + img.size].cpu().numpy().reshape(shape), wantS)
    if rb is not None:
        assert (rb[:8] == 7).all() and (rb[8 + img.size:] == 7).all()
        # a caller's plane of row sums through the module
        assert np.array_equal(sh.sharpen(view, sigma_of(r), 0.5, rowbuf=rb).cpu().numpy(), want)
        with pytest.raises(ValueError):
            sh.sharpen(view, sigma_of(r), 0.5, rowbuf=rb[:100])
        with pytest.raises(ValueError):
            sh.sharpen(view, sigma_of(r), 0.5, rowbuf=rb.float())


@pytest.mark.parametrize("r", [4, F + 1])
def test_window_and_side_stream(r):
    sh = SH()
    shape = (TR + 1, 2 * TC + 3)
    img = image(shape)
    want = expected(shape, r)[1]
    big = torch.zeros((shape[0] + 9, shape[1] + 11), dtype=torch.uint8, device="cuda")
    win = big[3:3 + shape[0], 5:5 + shape[1]]
    win.copy_(dev(img))
    assert not win.is_contiguous()
    first = sh.sharpen(win, sigma_of(r), 0.5)
    assert np.array_equal(first.cpu().numpy(), want)
    assert np.array_equal(sh.sharpen(win.float(), sigma_of(r), 0.5).cpu().numpy(), want.astype(np.float32))
    assert torch.equal(sh.sharpen(win, sigma_of(r), 0.5), first)          # repeatable
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = sh.sharpen(win, sigma_of(r), 0.5)
        S = sh.blur_sum(win, sigma_of(r))
    side.synchronize()
    assert torch.equal(other, first) and np.array_equal(S.cpu().numpy(), expected(shape, r)[0])


def test_largest_sum_and_clipping():
    sh = SH()
    # all 255 at the largest radius: S is at its maximum 255 * 2^48 and the image a fixed point
    flat = torch.full((2, TR + 3, TC + 5), 255, dtype=torch.uint8, device="cuda")
    assert (sh.blur_sum(flat, 16.0) == 255 * (1 << 48)).all()
    for amount in (0.5, 1e6, -1e6):
        assert (sh.sharpen(flat, 16.0, amount) == 255).all()
    for level in (0, 37):
        flat.fill_(level)
        for sigma in (1.0, 4.25):
            assert (sh.sharpen(flat, sigma, 1e6) == level).all() and (sh.sharpen(flat, sigma, -1e6) == level).all()
    # a 0 / 255 checkerboard under amounts of +-1e6 clips at both ends
    yy, xx = np.mgrid[0:TR + 3, 0:TC + 5]
    board = (((yy + xx) & 1) * 255).astype(np.uint8)
    for sigma in (1.0, 4.25, 16.0):
        for amount in (1e6, -1e6):
            want = sh.sharpen_np(board, sigma, amount)
            assert set(np.unique(want)) == {0, 255}
            assert np.array_equal(sh.sharpen(dev(board), sigma, amount).cpu().numpy(), want)
    assert np.array_equal(sh.sharpen_np(board, 1.0, 1e6), board) and np.array_equal(sh.sharpen_np(board, 1.0, -1e6), 255 - board)


def test_argument_errors():
    """Every bad argument returns non-zero with a message and leaves the outputs as they were. The checks run on the host
    before any launch: nothing is sent to the device."""
    import ctypes as CT

    from adipose_amd._lib import AdpError, call, ptr, stream_ptr
    sh = SH()
    N, H, W = 2, 40, 72
    img = dev(image((N, H, W), 4))
    dst = torch.full((N, H, W), 7, dtype=torch.uint8, device="cuda")
    dstf = torch.full((N, H, W), 7.0, dtype=torch.float32, device="cuda")
    Sb = torch.full((N, H, W), 7, dtype=torch.int64, device="cuda")
    rb = torch.full((N, H, W), 7, dtype=torch.int32, device="cuda")
    s = stream_ptr()
    i, d, df, S_, R_ = (ptr(t) for t in (img, dst, dstf, Sb, rb))
    q4, r4 = sh._taps_arg(sh.taps(1.0)), 4
    qb, rbig = sh._taps_arg(sh.taps((F + 1) / 4)), F + 1
    off = sh.taps(1.0)
    off[0] += 1
    qoff = sh._taps_arg(off)
    bad = [
        ("N must", "adp_gray_sharpen", (-1, H, W, i, 0, q4, r4, 0.5, None, d, 0, s)),
        ("N must", "adp_gray_sharpen", (65536, 1, 1, i, 0, q4, r4, 0.5, None, d, 0, s)),
        ("N must", "adp_gray_sharpen", (N, 0, W, i, 0, q4, r4, 0.5, None, d, 0, s)),
        ("N must", "adp_gray_sharpen", (N, H, 0, i, 0, q4, r4, 0.5, None, d, 0, s)),
        ("N must", "adp_gray_sharpen", (1, 65536, 32768, i, 0, q4, r4, 0.5, None, d, 0, s)),      # H * W = 2^31
        ("r must", "adp_gray_sharpen", (N, H, W, i, 0, q4, -1, 0.5, None, d, 0, s)),
        ("r must", "adp_gray_sharpen", (N, H, W, i, 0, q4, RMAX + 1, 0.5, R_, d, 0, s)),
        ("sum to 2\\^24", "adp_gray_sharpen", (N, H, W, i, 0, qoff, r4, 0.5, None, d, 0, s)),
        ("sum to 2\\^24", "adp_gray_sharpen", (N, H, W, i, 0, q4, r4 - 1, 0.5, None, d, 0, s)),
        ("amount must", "adp_gray_sharpen", (N, H, W, i, 0, q4, r4, float("nan"), None, d, 0, s)),
        ("amount must", "adp_gray_sharpen", (N, H, W, i, 0, q4, r4, float("inf"), None, d, 0, s)),
        ("non-null", "adp_gray_sharpen", (N, H, W, None, 0, q4, r4, 0.5, None, d, 0, s)),
        ("non-null", "adp_gray_sharpen", (N, H, W, i, 0, None, r4, 0.5, None, d, 0, s)),
        ("non-null", "adp_gray_sharpen", (N, H, W, i, 0, q4, r4, 0.5, None, None, 0, s)),
        ("rowbuf must be non-null", "adp_gray_sharpen", (N, H, W, i, 0, qb, rbig, 0.5, None, d, 0, s)),
        ("overlap", "adp_gray_sharpen", (N, H, W, d, 0, q4, r4, 0.5, None, d, 0, s)),
        ("overlap", "adp_gray_sharpen", (1, H, W, d, 0, q4, r4, 0.5, None, CT.c_void_p(dst.data_ptr() + H * W - 1), 0, s)),
        ("overlap", "adp_gray_sharpen", (N, H, W, df, 1, q4, r4, 0.5, None, df, 1, s)),
        ("overlap", "adp_gray_sharpen", (N, H, W, i, 0, qb, rbig, 0.5, i, d, 0, s)),
        ("overlap", "adp_gray_sharpen", (N, H, W, i, 0, qb, rbig, 0.5, df, df, 1, s)),
        ("N must", "adp_gray_blur", (-1, H, W, i, 0, q4, r4, None, S_, s)),
        ("N must", "adp_gray_blur", (N, H, 0, i, 0, q4, r4, None, S_, s)),
        ("r must", "adp_gray_blur", (N, H, W, i, 0, q4, RMAX + 1, R_, S_, s)),
        ("sum to 2\\^24", "adp_gray_blur", (N, H, W, i, 0, qoff, r4, None, S_, s)),
        ("non-null", "adp_gray_blur", (N, H, W, None, 0, q4, r4, None, S_, s)),
        ("non-null", "adp_gray_blur", (N, H, W, i, 0, None, r4, None, S_, s)),
        ("non-null", "adp_gray_blur", (N, H, W, i, 0, q4, r4, None, None, s)),
        ("rowbuf must be non-null", "adp_gray_blur", (N, H, W, i, 0, qb, rbig, None, S_, s)),
        ("overlap", "adp_gray_blur", (N, H, W, S_, 0, q4, r4, None, S_, s)),
        ("overlap", "adp_gray_blur", (N, H, W, i, 0, qb, rbig, S_, S_, s)),
    ]
    before = img.clone()
    for match, name, args in bad:
        with pytest.raises(AdpError, match=match):
            call(name, *args)
    torch.cuda.synchronize()
    assert (dst == 7).all() and (dstf == 7).all() and (Sb == 7).all() and (rb == 7).all() and torch.equal(img, before)
    # N = 0 returns 0 without a launch
    assert call("adp_gray_sharpen", 0, H, W, i, 0, q4, r4, 0.5, None, d, 0, s) == 0
    assert call("adp_gray_sharpen", 0, H, W, i, 0, qb, rbig, 0.5, R_, d, 0, s) == 0
    assert call("adp_gray_blur", 0, H, W, i, 0, q4, r4, None, S_, s) == 0
    torch.cuda.synchronize()
    assert (dst == 7).all() and (Sb == 7).all() and (rb == 7).all()
    # the module refuses the same before it reaches the library
    for fn in (lambda: sh.sharpen(img, 16.25), lambda: sh.sharpen(img, 0.0), lambda: sh.sharpen(img, 1.0, float("nan")),
               lambda: sh.blur_sum(img, -1.0), lambda: sh.sharpen(img[None])):
        with pytest.raises(ValueError):
            fn()
    with pytest.raises(TypeError):
        sh.sharpen(img.to(torch.int32))
    with pytest.raises(TypeError):
        sh.sharpen(img, 1.0, 0.5, torch.int32)


def test_reference_surface_on_device():
    """Tensor in, tensor out on the same device and in the input's dtype; array in, array out."""
    sh = SH()
    img = image((2, 40, 72), 6)
    want = sh.sharpen_np(img, 1.0, 0.5)
    got = sh.sharpen_image(dev(img))
    assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    got = sh.sharpen_image(img.astype(np.float32), 1.0, 0.5)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32))
    got = sh.sharpen_image(torch.from_numpy(img), 4.25, 0.3)
    assert not got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.numpy(), sh.sharpen_np(img, 4.25, 0.3))
    u = sh.UnsharpMask(2.3, 0.7)
    assert np.array_equal(u(dev(img).float()).cpu().numpy(), sh.sharpen_np(img, 2.3, 0.7, np.float32))


# ---------------------------------------------------------------- predictor
S = 64   # the smallest tile the predictor tests use


def gray_tile(seed, shape=(S, S)):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    g = (100 + 90 * (yy / shape[0]) + 40 * np.sin(yy / 9.0 + seed) * np.cos(xx / 6.0) + 25 * np.sin(xx / 2.0)
         + rng.normal(0, 12, shape))
    return np.clip(np.rint(g), 0, 255).astype(np.float32)


@pytest.fixture(scope="module")
def net():
    from adipose_amd.nets import AdiposeV3Net
    from oracle import torch_ref as R_
    n = AdiposeV3Net(1, S, dtype="f32", device="cuda", deep_supervision=False)
    n.set_weights(R_.adipose_v3_keras_weights(seed=865, deep_supervision=False))
    return n


def test_predictor_sharpen(net):
    from adipose_amd.contrast import Clahe, clahe_np
    from adipose_amd.predictor import HipUnetPredictor
    sh = SH()
    u = sh.UnsharpMask(1.0, 0.5)
    tiles = [gray_tile(s) for s in (1, 2, 3)]
    plain = HipUnetPredictor(net, max_batch=8)
    for views in ([0], [0, 4, 5, 1]):
        want = plain.predict_views([sh.sharpen_np(t, 1.0, 0.5, np.float32) for t in tiles], 120.0, 40.0, views).clone()
        got = HipUnetPredictor(net, max_batch=8, sharpen=u).predict_views(tiles, 120.0, 40.0, views).clone()
        assert torch.equal(got, want)
        off = plain.predict_views(tiles, 120.0, 40.0, views).clone()
        assert not torch.equal(off, want)
        # sharpen=None: the same bits as a predictor built without the keyword; enhance=False switches it off
        assert torch.equal(HipUnetPredictor(net, max_batch=8, sharpen=None).predict_views(tiles, 120.0, 40.0, views), off)
        assert torch.equal(HipUnetPredictor(net, max_batch=8, sharpen=u).predict_views(tiles, 120.0, 40.0, views, enhance=False), off)
    # with contrast set the order is contrast, then sharpen
    first_clahe = [sh.sharpen_np(clahe_np(t, 2.0, (8, 8)), 1.0, 0.5, np.float32) for t in tiles]
    first_sharp = [clahe_np(sh.sharpen_np(t, 1.0, 0.5), 2.0, (8, 8), np.float32) for t in tiles]
    assert any(not np.array_equal(a, b) for a, b in zip(first_clahe, first_sharp))
    want = plain.predict_views(first_clahe, 120.0, 40.0, [0]).clone()
    got = HipUnetPredictor(net, max_batch=8, contrast=Clahe(2.0, 8), sharpen=u).predict_views(tiles, 120.0, 40.0, [0])
    assert torch.equal(got, want)
    rgb_net = types.SimpleNamespace(device=net.device, in_ch=3)
    with pytest.raises(ValueError, match="1-channel"):
        HipUnetPredictor(rgb_net, sharpen=u).predict_views(tiles, 120.0, 40.0, [0])


def test_sliding_window_sharpens_the_whole_image_once(net):
    from adipose_amd.contrast import Clahe, clahe_np
    from adipose_amd.predictor import AdiposeUNet, HipUnetPredictor, SlidingWindowInference
    sh = SH()
    u = sh.UnsharpMask(2.3, 0.7)
    img = gray_tile(7, (96, 160))
    sw = SlidingWindowInference(S, 0.5, "gaussian", verbose=False)
    plain = HipUnetPredictor(net, max_batch=8)
    got = sw.predict_with_sliding_window(img, HipUnetPredictor(net, max_batch=8, sharpen=u), 120.0, 40.0)
    whole = sh.sharpen_np(img, 2.3, 0.7, np.float32)
    assert np.array_equal(got, sw.predict_with_sliding_window(whole, plain, 120.0, 40.0))
    # per tile the border is the window's own
    assert not np.array_equal(sh.sharpen_np(img[:S, :S], 2.3, 0.7, np.float32), whole[:S, :S])
    # after the contrast enhancement of the whole image
    got = sw.predict_with_sliding_window(img, HipUnetPredictor(net, max_batch=8, contrast=Clahe(2.0, 4), sharpen=u), 120.0, 40.0)
    whole = sh.sharpen_np(clahe_np(img, 2.0, (4, 4)), 2.3, 0.7, np.float32)
    assert np.array_equal(got, sw.predict_with_sliding_window(whole, plain, 120.0, 40.0))
    # the wrapper hands the keyword on
    m = AdiposeUNet(tile_size=S, sharpen=u)
    assert m.sharpen is u
