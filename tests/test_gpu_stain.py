"""Device Reinhard stain normalisation (adp_stain_lab_stats / adp_stain_reinhard_apply, adipose_amd.stain, and the
predictor's `stain_normalizer`) against the module's float64 numpy path (rgb2lab_np / lab2rgb_np / reinhard_np), which
restates skimage's documented rgb2lab / lab2rgb (D65, 2-degree observer): parity with skimage itself is unpinned
(skimage is not installed).

Inputs are seeded histology-like tiles (a pink-ish base, smooth structure, noise); the target statistics come from a
second, differently tinted tile. Two cases are avoided on purpose: source = reference (every f64 value lands within
1e-15 of an integer before the truncation to uint8, so the f64 result itself is noise) and constant tiles against the
f64 path (numpy's std of a constant tile is ~1e-14, not 0).

Bounds: statistics 1e-3 absolute (an f32 restatement differs by ~5e-6 on such tiles; a wrong constant or a sample
std moves them by > 1e-2); output bytes within 1 of f64 everywhere and different in at most 0.1 % of the bytes (a
truncation can only flip where the f64 value sits within the f32 error of an integer), with at most 1 % of the
reference's bytes at 0 or 255 so that clipping cannot hide a wrong transform.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PINK, PURPLE = (226, 168, 202), (186, 142, 208)
BASES = [PINK, (214, 150, 190), (232, 180, 196)]
SHAPES = [(1, 1, 1), (1, 3, 5), (3, 7, 9), (2, 64, 96), (1, 257, 131)]


def histology_tile(seed, h, w, base, amp=28.0, noise=5.0):
    """A seeded histology-like uint8 RGB tile: a tinted base colour, smooth structure and noise."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    p = rng.rand(3)
    s = 0.5 * np.sin(2 * np.pi * (x / (7 + w / 3) + p[0])) * np.cos(2 * np.pi * (y / (5 + h / 2.5) + p[1])) \
        + 0.5 * np.sin(2 * np.pi * ((x + y) / (11 + (h + w) / 5) + p[2]))
    img = np.asarray(base, np.float64) + amp * s[..., None] * np.array([0.6, 1.0, 0.7]) + noise * rng.randn(h, w, 3)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def stain():
    from adipose_amd import stain as S
    return S


@functools.lru_cache(maxsize=None)
def target():
    S = stain()
    return S.lab_stats_np(S.rgb2lab_np(histology_tile(12, 48, 80, PURPLE, amp=22.0) / 255.0))


@functools.lru_cache(maxsize=None)
def case(shape):
    """(batch uint8 (N, H, W, 3), f64 statistics (N, 6), f64-path output (N, H, W, 3) uint8); computed once, read-only."""
    S = stain()
    N, H, W = shape
    batch = np.stack([histology_tile(100 + 7 * n + H, H, W, BASES[n % 3], amp=28.0 - 6 * n) for n in range(N)])
    stats = np.stack([S.lab_stats_np(S.rgb2lab_np(t / 255.0)) for t in batch])
    ref = np.stack([(S.lab2rgb_np(S.reinhard_lab_np(t / 255.0, target())) * 255).astype(np.uint8) for t in batch])
    for a in (batch, stats, ref):
        a.setflags(write=False)
    return batch, stats, ref


def normalizer():
    nz = stain().ReinhardStainNormalizer()
    nz.set_reference_stats(target())
    return nz


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()   # (a C-ordered copy: the cases are read-only, one is a broadcast)


def run(batch, rgb=True, gray=False):
    S = stain()
    b = dev(batch)
    st = S.lab_stats_device(b)
    out, g = S.apply_device(b, st, target(), rgb=rgb, gray=gray)
    torch.cuda.synchronize()
    return st, out, g


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_statistics(shape):
    batch, stats, _ = case(shape)
    got = stain().lab_stats_device(dev(batch)).cpu().numpy()
    err = np.abs(got - stats).max()
    print(f"stats {shape}: max |device - f64| = {err:.3e}")
    assert err < 1e-3


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_output_bytes(shape):
    batch, _, ref = case(shape)
    _, out, _ = run(batch)
    got = out.cpu().numpy()
    diff = np.abs(got.astype(np.int16) - ref.astype(np.int16))
    frac, sat = (diff > 0).mean(), ((ref == 0) | (ref == 255)).mean()
    print(f"bytes {shape}: max diff {diff.max()}, differing {int((diff > 0).sum())} of {diff.size}, saturated {sat:.4f}")
    assert diff.max() <= 1
    if shape[1] * shape[2] > 15:
        assert frac <= 1e-3
        assert sat <= 0.01


def test_deterministic():
    batch, _, _ = case((1, 257, 131))
    s1, o1, g1 = run(batch, gray=True)
    s2, o2, g2 = run(batch, gray=True)
    assert torch.equal(s1, s2) and torch.equal(o1, o2) and torch.equal(g1, g2)


def test_constant_tile():
    S = stain()
    tile = np.broadcast_to(np.array([200, 150, 180], np.uint8), (1, 8, 8, 3))
    st, out, _ = run(tile)
    st = st.cpu().numpy()
    assert np.all(st[0, 3:] == 0.0)
    assert np.abs(st[0, :3] - S.rgb2lab_np(np.array([200, 150, 180]) / 255.0)).max() < 1e-3
    want = (S.lab2rgb_np(target()[:3]) * 255).astype(np.int16)
    assert np.abs(out.cpu().numpy().astype(np.int16) - want).max() <= 1


def test_gray_is_pil_luma_of_the_output_bytes():
    S = stain()
    batch, _, _ = case((3, 7, 9))
    _, out, g = run(batch, gray=True)
    assert np.array_equal(g.cpu().numpy(), S.gray_from_rgb_np(out.cpu().numpy()))
    _, none, g2 = run(batch, rgb=False, gray=True)
    assert none is None and torch.equal(g, g2)
    batch, _, _ = case((2, 64, 96))
    _, out, g = run(batch, gray=True)
    assert np.array_equal(g.cpu().numpy(), S.gray_from_rgb_np(out.cpu().numpy()))


@pytest.mark.parametrize("shape", [(3, 7, 9), (2, 64, 96)], ids=str)
def test_batch_independence(shape):
    batch, _, _ = case(shape)
    st, out, _ = run(batch)
    for k in range(shape[0]):
        s1, o1, _ = run(batch[k:k + 1])
        assert torch.equal(s1[0], st[k]) and torch.equal(o1[0], out[k])


def test_normalize_image_and_tiles():
    nz = normalizer()
    batch, _, _ = case((2, 64, 96))
    tiles = nz.normalize_tiles(np.array(batch))   # a host array is uploaded
    assert tiles.dtype == torch.uint8 and tiles.is_cuda and tuple(tiles.shape) == batch.shape
    one = nz.normalize_image(np.array(batch[1]))
    assert isinstance(one, np.ndarray) and one.dtype == np.uint8
    assert np.array_equal(one, tiles[1].cpu().numpy())
    g = nz.normalize_tiles(dev(batch), out_gray=True)
    assert np.array_equal(g.cpu().numpy(), stain().gray_from_rgb_np(tiles.cpu().numpy()))


@pytest.fixture(scope="module")
def models():
    from adipose_amd.predictor import AdiposeUNet
    from oracle import torch_ref as TR
    w = TR.adipose_v3_keras_weights(seed=5, deep_supervision=False)
    out = []
    for nz in (None, normalizer()):
        m = AdiposeUNet(tile_size=64, dtype="f32", max_batch=8, stain_normalizer=nz)
        m.build_model()
        m.net.set_weights(w)
        out.append(m)
    return out


def test_predictor_takes_raw_rgb(models):
    plain, with_nz = models
    rgb = histology_tile(31, 64, 64, PINK)
    gray = with_nz.stain_normalizer.normalize_tiles(rgb[None], out_gray=True)[0].cpu().numpy()
    want = plain.predict_single(gray, 120.0, 40.0)
    assert np.array_equal(with_nz.predict_single(rgb, 120.0, 40.0), want)
    # TTA views and device tensors go the same way
    v = with_nz.predict_views([dev(rgb)], 120.0, 40.0, [0, 4, 5, 1]).cpu().numpy()
    assert np.array_equal(v, plain.predict_views([gray], 120.0, 40.0, [0, 4, 5, 1]).cpu().numpy())
    # a gray tile is untouched by a predictor with a normaliser, and a predictor without one is what it was
    assert np.array_equal(with_nz.predict_single(gray, 120.0, 40.0), want)


def test_sliding_window_takes_raw_rgb(models):
    from adipose_amd.predictor import SlidingWindowInference
    plain, with_nz = models
    rgb = histology_tile(32, 64, 96, PINK)
    sw = SlidingWindowInference(tile_size=64, overlap=0.5, verbose=False)
    got = sw.predict_with_sliding_window(rgb, with_nz, 120.0, 40.0)
    pos = sw.extract_tile_positions(rgb.shape)
    assert len(pos) == 2
    wins = np.stack([rgb[y:y + 64, x:x + 64] for y, x in pos])
    grays = with_nz.stain_normalizer.normalize_tiles(wins, out_gray=True)
    probs = plain.predict_views(list(grays), 120.0, 40.0, [0])
    want = sw.blender.reconstruct(list(probs), pos, rgb.shape[:2])
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-6)


def test_error_paths():
    from adipose_amd import _lib
    L = _lib.lib()
    batch, _, _ = case((1, 3, 5))
    b = dev(batch)
    st = torch.zeros((1, 6), dtype=torch.float64, device="cuda")
    out = torch.zeros_like(b)
    tgt = (C.c_double * 6)(*target())
    s = _lib.stream_ptr()
    p = _lib.ptr

    def fails(rc):
        return rc != 0 and len(L.adp_last_error()) > 0

    assert fails(L.adp_stain_lab_stats(1, 3, 5, None, p(st), s))
    assert fails(L.adp_stain_lab_stats(1, 3, 5, p(b), None, s))
    assert fails(L.adp_stain_lab_stats(1, 0, 5, p(b), p(st), s))
    assert fails(L.adp_stain_lab_stats(0, 3, 5, p(b), p(st), s))
    assert fails(L.adp_stain_reinhard_apply(1, 3, 5, None, p(st), tgt, p(out), None, s))
    assert fails(L.adp_stain_reinhard_apply(1, 3, 0, p(b), p(st), tgt, p(out), None, s))
    assert fails(L.adp_stain_reinhard_apply(1, 3, 5, p(b), None, tgt, p(out), None, s))
    assert fails(L.adp_stain_reinhard_apply(1, 3, 5, p(b), p(st), None, p(out), None, s))
    assert fails(L.adp_stain_reinhard_apply(1, 3, 5, p(b), p(st), tgt, None, None, s))
    assert b"both NULL" in L.adp_last_error()
    torch.cuda.synchronize()
    assert not out.any() and not st.any()   # nothing was launched
    with pytest.raises(_lib.AdpError):
        _lib.call("adp_stain_lab_stats", 1, 0, 0, p(b), p(st), s)
