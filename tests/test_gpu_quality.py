"""Device tile quality control (adp_tile_qc, adipose_amd.quality, the predictors' `tile_filter`, the inference CLI's
--tile-qc) against the module's numpy path qc_sums_np, which restates OpenCV 4's 8-bit BGR2GRAY and cv2.Laplacian
(ksize 1, reflect-101): parity with cv2 itself is unpinned (cv2 is not installed).

The sums are integers, so every comparison of sums is array_equal: there is no tolerance to choose. Inputs are seeded
histology-like tiles (the generator of test_gpu_stain.py): a 64x96 PINK tile with noise 5 has lap_var ~ 228 (tissue),
with noise 0 ~ 3.07 (blurry), and base (245, 244, 246) with amp 4, noise 2 has white_ratio 1.0 (empty), all far from
the thresholds 0.70 and 7.5.
"""
import csv
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PINK, WHITE = (226, 168, 202), (245, 244, 246)
SHAPES = [(1, 2, 2), (1, 2, 5), (3, 7, 9), (2, 64, 96), (1, 257, 131), (5, 33, 65),
          # whole 32 x 256 regions only: the kernel's instance without per-lane and per-row guards (one region, several)
          (2, 32, 256), (1, 64, 512)]


def histology_tile(seed, h, w, base, amp=28.0, noise=5.0):
    """A seeded histology-like uint8 RGB tile: a tinted base colour, smooth structure and noise."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    p = rng.rand(3)
    s = 0.5 * np.sin(2 * np.pi * (x / (7 + w / 3) + p[0])) * np.cos(2 * np.pi * (y / (5 + h / 2.5) + p[1])) \
        + 0.5 * np.sin(2 * np.pi * ((x + y) / (11 + (h + w) / 5) + p[2]))
    img = np.asarray(base, np.float64) + amp * s[..., None] * np.array([0.6, 1.0, 0.7]) + noise * rng.randn(h, w, 3)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def tissue(seed, h, w):
    return histology_tile(seed, h, w, PINK)


def blurry(seed, h, w):
    return histology_tile(seed, h, w, PINK, noise=0.0)


def empty(seed, h, w):
    return histology_tile(seed, h, w, WHITE, amp=4.0, noise=2.0)


def Q():
    from adipose_amd import quality
    return quality


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


@functools.lru_cache(maxsize=None)
def case(shape):
    """(batch uint8 (N, H, W, 3) of mixed classes, its numpy sums (N, 4)); computed once, read-only."""
    N, H, W = shape
    kinds = [tissue, empty, blurry]
    batch = np.stack([kinds[n % 3](200 + 11 * n + H, H, W) for n in range(N)])
    ref = Q().qc_sums_np(batch)
    batch.setflags(write=False)
    ref.setflags(write=False)
    return batch, ref


def checkerboard(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.repeat((((y + x) & 1) * 255).astype(np.uint8)[..., None], 3, axis=-1)[None]


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_contiguous_batches(shape):
    batch, ref = case(shape)
    got = Q().qc_sums_device(dev(batch)).cpu().numpy()
    print(f"sums {shape}: device {got.tolist()} numpy {ref.tolist()}")
    assert got.dtype == np.int64 and np.array_equal(got, ref)


def test_mixed_classes_in_one_batch():
    batch, ref = case((5, 33, 65))
    qc = Q().TileQC()
    assert qc.classes_from_sums(ref) == ["tissue", "empty", "blurry", "tissue", "empty"]
    assert qc.classify(dev(batch)) == ["tissue", "empty", "blurry", "tissue", "empty"]
    assert qc.classify(np.array(batch)) == ["tissue", "empty", "blurry", "tissue", "empty"]   # a host array is uploaded


@pytest.mark.parametrize("thr", [-3, 0, 200, 255, 256, 1000])
def test_any_white_threshold(thr):
    batch, _ = case((3, 7, 9))
    assert np.array_equal(Q().qc_sums_device(dev(batch), thr).cpu().numpy(), Q().qc_sums_np(batch, thr))


def window_case(h, w, T, positions):
    img = tissue(77 + h, h, w)
    img[:, 2 * w // 3:] = empty(78, h, w - 2 * w // 3)
    wins = np.stack([img[y:y + T, x:x + T] for y, x in positions])
    got = Q().qc_sums_windows(dev(img), positions, T).cpu().numpy()
    contiguous = Q().qc_sums_device(dev(wins)).cpu().numpy()
    assert np.array_equal(got, contiguous)            # reflection stops at the window's own edge
    assert np.array_equal(got, Q().qc_sums_np(wins))


def test_windows_strided():
    from adipose_amd.predictor import SlidingWindowInference
    sw = SlidingWindowInference(tile_size=32, overlap=0.25, verbose=False)
    assert sw.stride == 24
    pos = sw.extract_tile_positions((96, 160))
    assert len(pos) > 8
    # the grid's own origins are multiples of 24 or the clamped last column; add odd ones: byte offsets of every
    # residue mod 4
    pos = pos + [(1, 1), (5, 2), (63, 3), (64, 127), (17, 101)]
    assert {(y * 480 + 3 * x) % 4 for y, x in pos} == {0, 1, 2, 3}
    window_case(96, 160, 32, pos)


def test_windows_overlapping_almost_entirely():
    window_case(40, 40, 32, [(0, 0), (0, 8), (8, 0), (8, 8)])


def test_windows_of_an_odd_width_image():
    """3 * W odd: the rows of one window alternate between all four alignments."""
    window_case(45, 51, 16, [(0, 0), (29, 35), (7, 13), (28, 1)])


def test_windows_of_whole_regions_at_every_alignment():
    """256 x 256 windows take the kernel's whole-region instance; 3 * 301 is odd and the origins have every residue
    mod 4, so its rows start at every byte alignment."""
    pos = [(0, 0), (1, 1), (44, 45), (1, 2), (17, 31)]
    assert {(y * 903 + 3 * x) % 4 for y, x in pos} == {0, 1, 2, 3}
    window_case(300, 301, 256, pos)


def test_windows_outside_the_image_are_refused():
    img = dev(tissue(1, 40, 40))
    with pytest.raises(ValueError):
        Q().qc_sums_windows(img, [(0, 9)], 32)
    with pytest.raises(ValueError):
        Q().qc_sums_windows(img, [(-1, 0)], 32)


def test_checkerboard_passes_32_bits_per_block():
    """Every lap = +-1020: S2 = 128 * 128 * 1 040 400 = 1.7e10 > 2^32."""
    got = Q().qc_sums_device(dev(checkerboard(128, 128))).cpu().numpy()
    assert got.tolist() == [[128 * 128 // 2, 0, 128 * 128 * 1040400, 128 * 128]]
    _, var = Q().measures(got)
    assert var[0] == 1040400.0


def test_checkerboard_1024():
    got = Q().qc_sums_device(dev(checkerboard(1024, 1024))).cpu().numpy()
    assert got.tolist() == [[1024 * 1024 // 2, 0, 1024 * 1024 * 1040400, 1024 * 1024]]


def test_bit_identity():
    batch, _ = case((5, 33, 65))
    b = dev(batch)
    one = Q().qc_sums_device(b)
    assert torch.equal(one, Q().qc_sums_device(b))
    for k in range(5):
        assert torch.equal(Q().qc_sums_device(b[k:k + 1].contiguous())[0], one[k])


def test_error_paths():
    from adipose_amd import _lib
    L = _lib.lib()
    batch, _ = case((1, 2, 5))
    b = dev(batch)
    sums = torch.full((1, 4), -7, dtype=torch.int64, device="cuda")
    org = torch.zeros(1, dtype=torch.int64, device="cuda")
    s = _lib.stream_ptr()
    p = _lib.ptr

    def fails(rc):
        return rc != 0 and len(L.adp_last_error()) > 0

    assert fails(L.adp_tile_qc(1, 2, 5, None, 0, None, 235, p(sums), s))
    assert fails(L.adp_tile_qc(1, 2, 5, p(b), 0, None, 235, None, s))
    assert fails(L.adp_tile_qc(0, 2, 5, p(b), 0, None, 235, p(sums), s))
    assert fails(L.adp_tile_qc(-1, 2, 5, p(b), 0, p(org), 235, p(sums), s))
    assert fails(L.adp_tile_qc(1, 1, 5, p(b), 0, None, 235, p(sums), s))
    assert fails(L.adp_tile_qc(1, 2, 1, p(b), 0, None, 235, p(sums), s))
    assert fails(L.adp_tile_qc(1, 2, 5, p(b), 14, None, 235, p(sums), s))
    assert b"row_pitch" in L.adp_last_error()
    torch.cuda.synchronize()
    assert (sums == -7).all()   # nothing was launched
    with pytest.raises(_lib.AdpError):
        _lib.call("adp_tile_qc", 1, 0, 0, p(b), 0, None, 235, p(sums), s)
    # the explicit pitch of a contiguous batch is the default one
    assert L.adp_tile_qc(1, 2, 5, p(b), 15, None, 235, p(sums), s) == 0
    assert np.array_equal(sums.cpu().numpy(), case((1, 2, 5))[1])


# ---------------------------------------------------------------- predictors
PURPLE = (186, 142, 208)
MEAN, STD = 120.0, 40.0


def normalizer():
    from adipose_amd import stain as S
    nz = S.ReinhardStainNormalizer()
    nz.set_reference_stats(S.lab_stats_np(S.rgb2lab_np(histology_tile(12, 48, 80, PURPLE, amp=22.0) / 255.0)))
    return nz


@pytest.fixture(scope="module")
def models():
    """(plain, filtered): the same seeded network without and with a TileQC."""
    from adipose_amd.predictor import AdiposeUNet
    from oracle import torch_ref as TR
    w = TR.adipose_v3_keras_weights(seed=5, deep_supervision=False)
    out = []
    for qc in (None, Q().TileQC()):
        m = AdiposeUNet(tile_size=64, dtype="f32", max_batch=8, tile_filter=qc)
        m.build_model()
        m.net.set_weights(w)
        out.append(m)
    return out


@pytest.fixture
def forwards(models, monkeypatch):
    """Batch sizes of the filtered model's forwards."""
    seen = []
    inner = models[1]._pred._forward
    monkeypatch.setattr(models[1]._pred, "_forward", lambda B: (seen.append(B), inner(B))[1])
    return seen


def pil_gray(rgb):
    from adipose_amd.stain import gray_from_rgb_np
    return gray_from_rgb_np(rgb)


def four_tiles():
    return [tissue(41, 64, 64), empty(42, 64, 64), tissue(43, 64, 64), blurry(44, 64, 64)]


def test_predictor_skips_empty_tiles(models, forwards):
    plain, filt = models
    tiles = four_tiles()
    got = filt.predict_views(tiles, MEAN, STD, [0]).cpu().numpy()
    assert filt.last_tile_classes == ["tissue", "empty", "tissue", "blurry"]
    assert forwards == [3]
    want = plain.predict_views([pil_gray(tiles[k]) for k in (0, 2, 3)], MEAN, STD, [0]).cpu().numpy()
    assert plain.last_tile_classes is None
    assert np.array_equal(got[[0, 2, 3]], want) and want.any()
    assert not got[1].any()
    # device tensors go the same way, and so do TTA views
    assert np.array_equal(filt.predict_views([dev(t) for t in tiles], MEAN, STD, [0]).cpu().numpy(), got)
    v = filt.predict_views(tiles, MEAN, STD, [0, 4]).cpu().numpy()
    wv = plain.predict_views([pil_gray(tiles[k]) for k in (0, 2, 3)], MEAN, STD, [0, 4]).cpu().numpy()
    assert np.array_equal(v[[0, 2, 3]], wv) and not v[1].any()
    assert forwards == [3, 3, 6]
    # predict_single of an empty tile: zeros without a forward
    assert not filt.predict_single(tiles[1], MEAN, STD).any() and filt.last_tile_classes == ["empty"]
    assert forwards == [3, 3, 6]


def test_predictor_skip_classes(models, forwards):
    plain, filt = models
    tiles = four_tiles()
    filt.skip_classes = ("empty", "blurry")
    try:
        got = filt.predict_views(tiles, MEAN, STD, [0]).cpu().numpy()
    finally:
        filt.skip_classes = ("empty",)
    assert forwards == [2] and filt.last_tile_classes == ["tissue", "empty", "tissue", "blurry"]
    want = plain.predict_views([pil_gray(tiles[k]) for k in (0, 2)], MEAN, STD, [0]).cpu().numpy()
    assert np.array_equal(got[[0, 2]], want) and not got[1].any() and not got[3].any()


def test_gray_float_tile_passes_unclassified(models, forwards):
    plain, filt = models
    gray = pil_gray(empty(42, 64, 64))   # would be skipped as RGB
    got = filt.predict_single(gray, MEAN, STD)
    assert filt.last_tile_classes is None and forwards == [1]
    assert np.array_equal(got, plain.predict_single(gray, MEAN, STD))


def sliding_case():
    img = tissue(90, 64, 160)
    img[:, 107:] = empty(91, 64, 53)   # the right third is glass
    return img


@pytest.mark.parametrize("with_stain", [False, True], ids=["plain", "stain"])
def test_sliding_window_skips_empty_windows(models, monkeypatch, with_stain):
    from adipose_amd.predictor import SlidingWindowInference
    plain, filt = models
    img = sliding_case()
    sw = SlidingWindowInference(tile_size=64, overlap=0.5, verbose=False)
    pos = sw.extract_tile_positions(img.shape)
    wins = np.stack([img[y:y + 64, x:x + 64] for y, x in pos])
    classes = Q().TileQC().classes_from_sums(Q().qc_sums_np(wins))
    assert pos == [(0, 0), (0, 32), (0, 64), (0, 96)] and classes == ["tissue", "tissue", "tissue", "empty"]
    live = [k for k, c in enumerate(classes) if c != "empty"]
    seen = []
    inner = filt.predict_views
    monkeypatch.setattr(filt, "predict_views", lambda tiles, *a, **kw: (seen.extend(tiles), inner(tiles, *a, **kw))[1])
    nz = normalizer() if with_stain else None
    filt.stain_normalizer = nz
    try:
        got = sw.predict_with_sliding_window(dev(img) if with_stain else img, filt, MEAN, STD)
    finally:
        filt.stain_normalizer = None
    assert sw.last_tile_classes == classes
    assert len(seen) == len(live) and all(np.array_equal(t.cpu().numpy(), wins[k]) for t, k in zip(seen, live))
    grays = nz.normalize_tiles(wins[live], out_gray=True) if with_stain else [pil_gray(wins[k]) for k in live]
    probs = iter(plain.predict_views(list(grays), MEAN, STD, [0]))
    maps = [next(probs) if k in live else np.zeros((64, 64), np.float32) for k in range(len(pos))]
    want = sw.blender.reconstruct(maps, pos, img.shape[:2])
    err = np.abs(got - want).max()
    print(f"sliding window with skipped windows: max |difference| = {err:.3e}")
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-6)
    assert want[:, :96].any()


# ---------------------------------------------------------------- CLI
def test_cli_tile_qc(tmp_path):
    from PIL import Image

    from adipose_amd.checkpoint import save_weights
    from cli.segmentation_inference import main
    from oracle import torch_ref as TR
    tiles = {"a_tissue": tissue(51, 64, 64), "b_empty": empty(52, 64, 64), "c_blurry": blurry(53, 64, 64)}
    (tmp_path / "img").mkdir()
    for name, t in tiles.items():
        Image.fromarray(t).save(tmp_path / "img" / f"{name}.png")
    (tmp_path / "ck").mkdir()
    save_weights(None, tmp_path / "ck" / "phase2_best.weights.h5",
                 weights=TR.adipose_v3_keras_weights(seed=5, deep_supervision=False))
    (tmp_path / "ck" / "normalization_stats.json").write_text('{"mean": 120.0, "std": 40.0}')
    base = ["--images-dir", str(tmp_path / "img"), "--weights", str(tmp_path / "ck"), "--tile", "64",
            "--save-probability", "--threshold", "0.5"]
    assert main(base + ["--output-dir", str(tmp_path / "off")]) == 0
    assert main(base + ["--output-dir", str(tmp_path / "on"), "--tile-qc"]) == 0
    assert not (tmp_path / "off" / "tile_qc.csv").exists()

    def out(run, name, kind):
        sub = "masks" if kind == "mask" else "probabilities"
        return (tmp_path / run / sub / f"{name}_{kind}.tif").read_bytes()

    for name in ("a_tissue", "c_blurry"):
        assert out("on", name, "mask") == out("off", name, "mask")
        assert out("on", name, "prob") == out("off", name, "prob")
    for kind in ("mask", "prob"):
        z = np.array(Image.open(tmp_path / "on" / ("masks" if kind == "mask" else "probabilities") / f"b_empty_{kind}.tif"))
        assert z.shape == (64, 64) and not z.any()
    assert np.array(Image.open(tmp_path / "off" / "probabilities" / "b_empty_prob.tif")).any()   # the forward does say something
    with open(tmp_path / "on" / "tile_qc.csv") as f:
        rows = list(csv.DictReader(f))
    assert sorted((r["name"], r["class"], r["skipped"]) for r in rows) == [
        ("a_tissue.png", "tissue", "0"), ("b_empty.png", "empty", "1"), ("c_blurry.png", "blurry", "0")]
    assert all(set(r) == {"name", "white_ratio", "lap_var", "class", "skipped"} for r in rows)
    ratio, var = Q().measures(Q().qc_sums_np(np.stack(list(tiles.values()))))
    by = {r["name"]: r for r in rows}
    for k, name in enumerate(tiles):
        assert abs(float(by[name + ".png"]["white_ratio"]) - ratio[k]) < 1e-6
        assert abs(float(by[name + ".png"]["lap_var"]) - var[k]) < 1e-6
