"""Column de-banding and the z-score / percentile stretch on the device (csrc/graynorm.hip) against the numpy path of
adipose_amd.normalization, bit for bit: every comparison is equality, there is no tolerance. The numpy path itself is
pinned to the reference's formulas in tests/test_normalization.py.

Shapes sit around the band a block of adp_gray_colstats reduces (R rows x C columns): 1-pixel planes, single rows and
columns, one band exactly, one pixel less and more, many bands into few columns (where the atomics combine them), many
column bands, the aligned 16-byte path, an unaligned view, a 1024^2 plane, and planes of T and T + 1 blocks, where the
16-byte path of the statistics pass changes to blocks of F bands of rows (one image and a batch; the scalar path, which
keeps its bands, at the same size).

test_statistics_bits compares the float64 column parameters themselves: it is the check that float64 sqrt and division
on gfx950 are correctly rounded, which the definition assumes.
"""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from adipose_amd.normalization import BAND_COLS as C, BAND_ROWS as R, TALL_BLOCKS as T, TALL_FACTOR as F  # noqa: E402

SHAPES = [(1, 1, 1), (1, 1, 37), (1, 37, 1), (3, 37, 53), (2, R - 1, C - 1), (2, R, C), (2, R + 1, C + 1), (1, 4099, 7),
          (1, 5, 4099), (1, 3 * R + 5, 48), (1, 1024, 1024),
          (1, T * R, 16), (1, T * R + 1, 16), (1, T * R + F * R + 3, 7), (2, T * R // 2 + 1, 32)]
OPS = ["column_global", "column_range", "zscore", "percentile"]


def NM():
    from adipose_amd import normalization
    return normalization


def case_id(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)


def image(shape, seed=0):
    """Noise under a column-wise illumination profile, one constant column, one column with a single outlier."""
    rng = np.random.default_rng([seed, *shape])
    W = shape[-1]
    a = np.clip((rng.integers(0, 256, shape) * 0.5 + 60) * (1 + 0.3 * np.sin(np.arange(W) / 7)), 0, 255).astype(np.uint8)
    a[..., W // 3] = 77
    if W > 2:
        a[..., W - 1] = 255
        a[..., shape[-2] // 2, W - 1] = 254
    return a


def special_batch():
    """A constant image, a full-range ramp and noise."""
    H, W = 70, 272
    b = np.empty((3, H, W), np.uint8)
    b[0] = 200
    b[1] = (np.arange(H * W).reshape(H, W) % 256).astype(np.uint8)
    b[2] = np.random.default_rng(5).integers(0, 256, (H, W))
    return b


def ops(nm):
    return {
        "column_global": (lambda t, dt=None: nm.column_normalize(t, True, dt), lambda a, dt: nm.column_normalize_np(a, True, dt)),
        "column_range": (lambda t, dt=None: nm.column_normalize(t, False, dt), lambda a, dt: nm.column_normalize_np(a, False, dt)),
        "zscore": (lambda t, dt=None: nm.zscore(t, dt), lambda a, dt: nm.normalize_zscore_np(a, dt)),
        "percentile": (lambda t, dt=None: nm.percentile(t, 2.5, 97.5, dt), lambda a, dt: nm.normalize_percentile_np(a, 2.5, 97.5, dt)),
    }


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check(op, img):
    """uint8 and float32 on both sides: the four combinations hold the same integers."""
    d_fn, n_fn = ops(NM())[op]
    want = n_fn(img, np.uint8)
    d8, d32 = dev(img), dev(img.astype(np.float32))
    got = d_fn(d8)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    got = d_fn(d32)
    assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), want.astype(np.float32))
    assert np.array_equal(d_fn(d8, torch.float32).cpu().numpy(), want.astype(np.float32))
    assert np.array_equal(d_fn(d32, torch.uint8).cpu().numpy(), want)


@pytest.mark.parametrize("shape", SHAPES, ids=case_id)
@pytest.mark.parametrize("op", OPS)
def test_device_equals_numpy(op, shape):
    check(op, image(shape))


@pytest.mark.parametrize("op", OPS)
def test_special_batch_and_2d(op):
    b = special_batch()
    check(op, b)
    check(op, b[2])   # (H, W)
    d_fn, n_fn = ops(NM())[op]
    # every image on its own: the batch's results are the single images'
    got = d_fn(dev(b)).cpu().numpy()
    for i in range(3):
        assert np.array_equal(got[i], n_fn(b[i], np.uint8))
    if op == "zscore":
        assert (got[0] == 127).all()


@pytest.mark.parametrize("op", OPS)
def test_unaligned_plane(op):
    """(1, 64, 50) from an offset view of a larger buffer: the base is not 16-byte aligned, the scalar paths run."""
    from adipose_amd._lib import call, ptr, stream_ptr
    nm = NM()
    img = image((1, 64, 50), 3)
    buf = torch.zeros(img.size + 64, dtype=torch.uint8, device="cuda")
    view = buf[3:3 + img.size].view(1, 64, 50)
    view.copy_(dev(img))
    assert view.data_ptr() % 16 == 3 and view.is_contiguous()
    d_fn, n_fn = ops(nm)[op]
    assert np.array_equal(d_fn(view).cpu().numpy(), n_fn(img, np.uint8))
    # and an unaligned destination, through the library
    out = torch.full((img.size + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    dst = out[5:5 + img.size]
    s = stream_ptr()
    if op.startswith("column"):
        col, glob = nm.column_stats(view)
        call("adp_gray_colnorm", 1, 64, 50, ptr(view), 0, ptr(col), ptr(glob), int(op == "column_global"), ptr(dst), 0, s)
    else:
        hist = torch.empty((1, 256), dtype=torch.int32, device="cuda")
        call("adp_clahe_hist", 1, 64, 50, ptr(view), 0, 1, 1, ptr(hist), s)
        call("adp_gray_normalize", 1, 64 * 50, ptr(view), 0, ptr(hist), nm.ZSCORE if op == "zscore" else nm.PERCENTILE,
             2.5, 97.5, ptr(dst), 0, s)
    assert np.array_equal(dst.cpu().numpy().reshape(1, 64, 50), n_fn(img, np.uint8))
    assert (out[:5] == 0xA5).all() and (out[5 + img.size:] == 0xA5).all()


@pytest.mark.parametrize("shape", SHAPES + [(3, 70, 272)], ids=case_id)
def test_statistics_bits(shape):
    """cm, d per column and gm, gs, lo, hi per image as bits: float64 sqrt and division on the device round as numpy's."""
    nm = NM()
    img = special_batch() if shape == (3, 70, 272) else image(shape)
    for a in (img, img.astype(np.float32)):
        col, glob = nm.column_stats(dev(a))
        wc, wg = nm.column_stats_np(a)
        assert col.dtype == torch.float64 and glob.dtype == torch.float64
        assert tuple(col.shape) == wc.shape and tuple(glob.shape) == wg.shape
        assert np.array_equal(col.cpu().numpy().view(np.int64), wc.view(np.int64))
        assert np.array_equal(glob.cpu().numpy().view(np.int64), wg.view(np.int64))


def test_repeatable_and_side_stream():
    nm = NM()
    img = dev(image((2, 4 * R + 3, C + 16), 9))
    for op in OPS:
        d_fn = ops(nm)[op][0]
        first = d_fn(img).clone()
        assert torch.equal(d_fn(img), first)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            other = d_fn(img)
        side.synchronize()
        assert torch.equal(other, first)
    c1, g1 = nm.column_stats(img)
    c2, g2 = nm.column_stats(img)
    assert torch.equal(c1.view(torch.int64), c2.view(torch.int64)) and torch.equal(g1.view(torch.int64), g2.view(torch.int64))


def test_sentinels_stay():
    """Bytes before and after each output stay as they were."""
    from adipose_amd._lib import call, ptr, stream_ptr
    nm = NM()
    s = stream_ptr()
    for shape in ((2, R + 1, C + 1), (1, 5, 65), (3, 37, 48)):
        N, H, W = shape
        img = image(shape, 2)
        d = dev(img)
        cols = N * W
        sums = torch.full((cols * 2 + 16,), 7, dtype=torch.int64, device="cuda")
        mm = torch.full((cols * 2 + 16,), 7, dtype=torch.int32, device="cuda")
        call("adp_gray_colstats", N, H, W, ptr(d), 0, ptr(sums[8:]), ptr(mm[8:]), s)
        assert (sums[:8] == 7).all() and (sums[8 + 2 * cols:] == 7).all()
        assert (mm[:8] == 7).all() and (mm[8 + 2 * cols:] == 7).all()
        b = img.astype(np.int64)
        want = np.stack([b.sum(axis=1), (b * b).sum(axis=1)], axis=-1)
        assert np.array_equal(sums[8:8 + 2 * cols].cpu().numpy().reshape(N, W, 2), want)
        assert np.array_equal(mm[8:8 + 2 * cols].cpu().numpy().reshape(N, W, 2), np.stack([b.min(axis=1), b.max(axis=1)], axis=-1))
        col = torch.full((cols * 2 + 16,), -7.0, dtype=torch.float64, device="cuda")
        glob = torch.full((N * 4 + 16,), -7.0, dtype=torch.float64, device="cuda")
        call("adp_gray_colparams", N, H, W, ptr(sums[8:]), ptr(mm[8:]), ptr(col[8:]), ptr(glob[8:]), s)
        assert (col[:8] == -7).all() and (col[8 + 2 * cols:] == -7).all()
        assert (glob[:8] == -7).all() and (glob[8 + 4 * N:] == -7).all()
        hist = torch.empty((N, 256), dtype=torch.int32, device="cuda")
        call("adp_clahe_hist", N, H, W, ptr(d), 0, 1, 1, ptr(hist), s)
        for f32 in (0, 1):
            fill = -7 if f32 else 0xA5
            for op in OPS:
                dst = torch.full((img.size + 2 * (4 * W + 64),), fill, dtype=torch.float32 if f32 else torch.uint8, device="cuda")
                o = 4 * W + 64
                body = dst[o:o + img.size]
                if op.startswith("column"):
                    call("adp_gray_colnorm", N, H, W, ptr(d), 0, ptr(col[8:]), ptr(glob[8:]), int(op == "column_global"),
                         ptr(body), f32, s)
                else:
                    call("adp_gray_normalize", N, H * W, ptr(d), 0, ptr(hist), nm.ZSCORE if op == "zscore" else nm.PERCENTILE,
                         2.5, 97.5, ptr(body), f32, s)
                assert (dst[:o] == fill).all() and (dst[o + img.size:] == fill).all()
                assert np.array_equal(body.cpu().numpy().reshape(shape),
                                      ops(nm)[op][1](img, np.float32 if f32 else np.uint8))


def test_argument_errors():
    """Every bad argument returns non-zero with a message and leaves the outputs as they were. The checks run on the host
    before any launch: nothing is sent to the device."""
    import ctypes as CT

    from adipose_amd._lib import AdpError, call, ptr, stream_ptr
    nm = NM()
    N, H, W = 2, 64, 96
    img = dev(image((N, H, W), 4))
    dst = torch.full((N, H, W), 7, dtype=torch.uint8, device="cuda")
    dstf = torch.full((N, H, W), 7.0, dtype=torch.float32, device="cuda")
    sums = torch.full((N, W, 2), 7, dtype=torch.int64, device="cuda")
    mm = torch.full((N, W, 2), 7, dtype=torch.int32, device="cuda")
    col = torch.full((N, W, 2), 7.0, dtype=torch.float64, device="cuda")
    glob = torch.full((N, 4), 7.0, dtype=torch.float64, device="cuda")
    hist = torch.full((N, 256), 7, dtype=torch.int32, device="cuda")
    s = stream_ptr()
    i, d, df, S_, M, Cc, G, Hh = (ptr(t) for t in (img, dst, dstf, sums, mm, col, glob, hist))
    Z, P = nm.ZSCORE, nm.PERCENTILE
    bad = [
        ("non-null", "adp_gray_colstats", (N, H, W, None, 0, S_, M, s)),
        ("non-null", "adp_gray_colstats", (N, H, W, i, 0, None, M, s)),
        ("non-null", "adp_gray_colstats", (N, H, W, i, 0, S_, None, s)),
        ("N must", "adp_gray_colstats", (-1, H, W, i, 0, S_, M, s)),
        ("N must", "adp_gray_colstats", (65536, 1, 1, i, 0, S_, M, s)),
        ("N must", "adp_gray_colstats", (N, 0, W, i, 0, S_, M, s)),
        ("N must", "adp_gray_colstats", (N, H, 0, i, 0, S_, M, s)),
        ("N must", "adp_gray_colstats", (1, 65536, 32768, i, 0, S_, M, s)),      # H * W = 2^31
        ("overlap", "adp_gray_colstats", (N, H, W, S_, 0, S_, M, s)),
        ("overlap", "adp_gray_colstats", (N, H, W, i, 0, S_, CT.c_void_p(sums.data_ptr() + 8), s)),
        ("non-null", "adp_gray_colparams", (N, H, W, None, M, Cc, G, s)),
        ("non-null", "adp_gray_colparams", (N, H, W, S_, None, Cc, G, s)),
        ("non-null", "adp_gray_colparams", (N, H, W, S_, M, None, G, s)),
        ("non-null", "adp_gray_colparams", (N, H, W, S_, M, Cc, None, s)),
        ("N must", "adp_gray_colparams", (-1, H, W, S_, M, Cc, G, s)),
        ("N must", "adp_gray_colparams", (N, 0, W, S_, M, Cc, G, s)),
        ("overlap", "adp_gray_colparams", (N, H, W, S_, M, S_, G, s)),
        ("overlap", "adp_gray_colparams", (N, H, W, S_, M, Cc, Cc, s)),
        ("non-null", "adp_gray_colnorm", (N, H, W, None, 0, Cc, G, 1, d, 0, s)),
        ("non-null", "adp_gray_colnorm", (N, H, W, i, 0, None, G, 1, d, 0, s)),
        ("non-null", "adp_gray_colnorm", (N, H, W, i, 0, Cc, None, 1, d, 0, s)),
        ("non-null", "adp_gray_colnorm", (N, H, W, i, 0, Cc, G, 1, None, 0, s)),
        ("N must", "adp_gray_colnorm", (-1, H, W, i, 0, Cc, G, 1, d, 0, s)),
        ("N must", "adp_gray_colnorm", (N, H, 0, i, 0, Cc, G, 1, d, 0, s)),
        ("N must", "adp_gray_colnorm", (1, 32768, 65536, i, 0, Cc, G, 1, d, 0, s)),
        ("overlap", "adp_gray_colnorm", (N, H, W, d, 0, Cc, G, 1, d, 0, s)),
        ("overlap", "adp_gray_colnorm", (1, H, W, d, 0, Cc, G, 1, CT.c_void_p(dst.data_ptr() + H * W - 1), 0, s)),
        ("overlap", "adp_gray_colnorm", (N, H, W, i, 0, Cc, G, 1, Cc, 1, s)),
        ("non-null", "adp_gray_normalize", (N, H * W, None, 0, Hh, Z, 1.0, 99.0, d, 0, s)),
        ("non-null", "adp_gray_normalize", (N, H * W, i, 0, None, Z, 1.0, 99.0, d, 0, s)),
        ("non-null", "adp_gray_normalize", (N, H * W, i, 0, Hh, Z, 1.0, 99.0, None, 0, s)),
        ("N must", "adp_gray_normalize", (-1, H * W, i, 0, Hh, Z, 1.0, 99.0, d, 0, s)),
        ("N must", "adp_gray_normalize", (65536, 1, i, 0, Hh, Z, 1.0, 99.0, d, 0, s)),
        ("n_px must", "adp_gray_normalize", (N, 0, i, 0, Hh, Z, 1.0, 99.0, d, 0, s)),
        ("n_px must", "adp_gray_normalize", (1, 2 ** 31, i, 0, Hh, Z, 1.0, 99.0, d, 0, s)),
        ("method must", "adp_gray_normalize", (N, H * W, i, 0, Hh, 2, 1.0, 99.0, d, 0, s)),
        ("method must", "adp_gray_normalize", (N, H * W, i, 0, Hh, -1, 1.0, 99.0, d, 0, s)),
        ("percentiles", "adp_gray_normalize", (N, H * W, i, 0, Hh, P, 60.0, 40.0, d, 0, s)),
        ("percentiles", "adp_gray_normalize", (N, H * W, i, 0, Hh, P, -1.0, 99.0, d, 0, s)),
        ("percentiles", "adp_gray_normalize", (N, H * W, i, 0, Hh, P, 1.0, 100.5, d, 0, s)),
        ("percentiles", "adp_gray_normalize", (N, H * W, i, 0, Hh, P, float("nan"), 99.0, d, 0, s)),
        ("overlap", "adp_gray_normalize", (N, H * W, d, 0, Hh, Z, 1.0, 99.0, d, 0, s)),
        ("overlap", "adp_gray_normalize", (N, H * W, i, 0, Hh, Z, 1.0, 99.0, i, 1, s)),
        ("overlap", "adp_gray_normalize", (1, 64, i, 0, Hh, Z, 1.0, 99.0, Hh, 0, s)),
    ]
    before = img.clone()
    for match, name, args in bad:
        with pytest.raises(AdpError, match=match):
            call(name, *args)
    torch.cuda.synchronize()
    assert (dst == 7).all() and (dstf == 7).all() and (sums == 7).all() and (mm == 7).all() and (col == 7).all()
    assert (glob == 7).all() and (hist == 7).all() and torch.equal(img, before)
    # N = 0 returns 0 without a launch
    for name, args in (("adp_gray_colstats", (0, H, W, i, 0, S_, M, s)), ("adp_gray_colparams", (0, H, W, S_, M, Cc, G, s)),
                       ("adp_gray_colnorm", (0, H, W, i, 0, Cc, G, 1, d, 0, s)),
                       ("adp_gray_normalize", (0, H * W, i, 0, Hh, Z, 1.0, 99.0, d, 0, s))):
        assert call(name, *args) == 0
    torch.cuda.synchronize()
    assert (dst == 7).all() and (sums == 7).all() and (col == 7).all()
    assert nm.column_normalize(img[:0]).shape == (0, H, W) and nm.zscore(img[:0]).shape == (0, H, W)
    # the module refuses the same before it reaches the library
    with pytest.raises(ValueError):
        nm.percentile(img, 60, 40)
    with pytest.raises(ValueError):
        nm.percentile(img, -1, 99)
    with pytest.raises(ValueError):
        nm.zscore(img[None])                       # 4-D
    with pytest.raises(TypeError):
        nm.zscore(img.to(torch.int32))
    with pytest.raises(TypeError):
        nm.column_normalize(img, True, torch.int32)


def test_reference_surface_on_device():
    """Tensor in, tensor out on the same device and in the input's dtype; array in, array out."""
    nm = NM()
    img = image((2, 40, 64), 6)
    want = nm.column_normalize_np(img, True)
    got = nm.remove_banding_column_normalize(dev(img))
    assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    got = nm.remove_banding_column_normalize(img.astype(np.float32), True)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32))
    got = nm.normalize_percentile(dev(img).float(), 5, 95)
    assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), nm.normalize_percentile_np(img, 5, 95, np.float32))
    assert np.array_equal(nm.normalize_zscore(img), nm.normalize_zscore_np(img))
    g = nm.GrayNormalization(column_banding=True, preserve_global=False, method="zscore")
    assert np.array_equal(g(dev(img)).cpu().numpy(), nm.normalize_zscore_np(nm.column_normalize_np(img, False)))


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


def host_pipeline(t, dtype=np.float32):
    """The reference's order in numpy: column banding, morphological banding, percentile, rolling ball."""
    from adipose_amd import illumination as il
    nm = NM()
    v = nm.column_normalize_np(t, True)
    v = il.remove_banding_morphological_np(v, 1, 12)
    v = nm.normalize_percentile_np(v, 2.0, 98.0)
    return il.rolling_ball_np(v, 7, dtype)


def settings():
    from adipose_amd.illumination import IlluminationCorrection
    nm = NM()
    return (nm.GrayNormalization(column_banding=True, method="percentile", p_low=2.0, p_high=98.0),
            IlluminationCorrection(banding=(1, 12), method="rolling-ball", radius=7))


def test_predictor_normalization(net):
    from adipose_amd.contrast import Clahe, clahe_np
    from adipose_amd.predictor import HipUnetPredictor
    gn, ic = settings()
    tiles = [gray_tile(s) for s in (1, 2, 3)]
    plain = HipUnetPredictor(net, max_batch=8)
    for views in ([0], [0, 4, 5, 1]):
        want = plain.predict_views([host_pipeline(t) for t in tiles], 120.0, 40.0, views).clone()
        got = HipUnetPredictor(net, max_batch=8, illumination=ic, normalization=gn).predict_views(tiles, 120.0, 40.0, views).clone()
        assert torch.equal(got, want)
        off = plain.predict_views(tiles, 120.0, 40.0, views).clone()
        assert not torch.equal(off, want)
        # normalization=None: the same bits as a predictor built without the keyword
        assert torch.equal(HipUnetPredictor(net, max_batch=8, normalization=None).predict_views(tiles, 120.0, 40.0, views), off)
        with_ic = HipUnetPredictor(net, max_batch=8, illumination=ic).predict_views(tiles, 120.0, 40.0, views).clone()
        assert torch.equal(HipUnetPredictor(net, max_batch=8, illumination=ic, normalization=None)
                           .predict_views(tiles, 120.0, 40.0, views), with_ic)
        assert torch.equal(HipUnetPredictor(net, max_batch=8, normalization=gn).predict_views(tiles, 120.0, 40.0, views,
                                                                                             enhance=False), off)
    # the order is not the composition of the two objects: the normalisation sits between banding and illumination
    nm = NM()
    composed = [ic(gn(t)) for t in tiles]
    assert any(not np.array_equal(c, host_pipeline(t)) for c, t in zip(composed, tiles))
    # normalisation alone, and before the contrast enhancement
    want = plain.predict_views([nm.normalize_zscore_np(t, np.float32) for t in tiles], 120.0, 40.0, [0]).clone()
    got = HipUnetPredictor(net, max_batch=8, normalization=nm.GrayNormalization(method="zscore")).predict_views(tiles, 120.0, 40.0, [0])
    assert torch.equal(got, want)
    want = plain.predict_views([clahe_np(host_pipeline(t), 2.0, (8, 8), np.float32) for t in tiles], 120.0, 40.0, [0]).clone()
    got = HipUnetPredictor(net, max_batch=8, contrast=Clahe(2.0, 8), illumination=ic, normalization=gn).predict_views(tiles, 120.0, 40.0, [0])
    assert torch.equal(got, want)
    rgb_net = types.SimpleNamespace(device=net.device, in_ch=3)
    with pytest.raises(ValueError, match="1-channel"):
        HipUnetPredictor(rgb_net, normalization=gn).predict_views(tiles, 120.0, 40.0, [0])


def test_sliding_window_normalises_the_whole_image_once(net):
    from adipose_amd.predictor import HipUnetPredictor, SlidingWindowInference
    gn, ic = settings()
    img = gray_tile(7, (96, 160))
    sw = SlidingWindowInference(S, 0.5, "gaussian", verbose=False)
    got = sw.predict_with_sliding_window(img, HipUnetPredictor(net, max_batch=8, illumination=ic, normalization=gn), 120.0, 40.0)
    whole = host_pipeline(img)
    plain = HipUnetPredictor(net, max_batch=8)
    want = sw.predict_with_sliding_window(whole, plain, 120.0, 40.0)
    assert np.array_equal(got, want)
    # per tile the statistics are the window's own
    assert not np.array_equal(host_pipeline(img[:S, :S]), whole[:S, :S])
    # the wrapper hands the keyword on
    from adipose_amd.predictor import AdiposeUNet
    m = AdiposeUNet(tile_size=S, normalization=gn)
    assert m.normalization is gn
