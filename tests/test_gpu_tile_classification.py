"""adp_fat_counts (csrc/tilefat.hip) and the device path of adipose_amd.tile_classification on the GPU. Every
comparison is equality, there is no tolerance: the kernel makes integers, and the reference is fat_counts_ref, the
numpy restatement that tests/test_tile_classification.py holds to the reference's golden vectors.

Shapes sit around ADP_FAT_BLOCK_PX (the pixels one block counts): one pixel, a few, fewer than a block, exactly one,
one more, more than two blocks; with an odd number of pixels and N > 1 the images after the first start off the
16-byte alignment, at different images in the float plane and in the byte plane."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

from adipose_amd import tile_classification as TC
from adipose_amd._lib import lib, ptr, stream_ptr
from adipose_amd.evaluation import BoundaryRefiner, read_image_gray
from adipose_amd.nets import AdiposeV3Net
from adipose_amd.predictor import TTA_VIEWS, HipUnetPredictor
from oracle import torch_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "tile_classification.npz"))
B = TC.FAT_BLOCK_PX
SHAPES = [(1, 1), (3, 5), (17, 19), (64, 64), (1, B - 1), (1, B), (1, B + 1), (1, 2 * B + 7)]
THRESHOLDS = [0.5, 0.3, 0.0, 1.0]
MASK_KINDS = ["zero", "01", "0255", "random", "01_two_last", "01_two_first"]
SENTINEL = 0x5A5A5A5A5A5A5A5A


def planted(thr):
    t = np.float32(thr)
    return [t, np.nextafter(t, np.float32(-np.inf)), np.nextafter(t, np.float32(np.inf)), np.float32(0.0),
            np.float32(1.0), np.float32(-0.25), np.float32(-3.0), np.float32(np.inf), np.float32(-np.inf),
            np.float32(np.nan)]


def make_pred(rng, N, shape, thr):
    p = rng.random((N,) + shape).astype(np.float32)
    flat = p.reshape(-1)
    for v in planted(thr):   # among the seeded pixels (a tiny plane may lose some to a later one)
        flat[rng.integers(0, flat.size, size=2)] = v
    return p


def make_mask(rng, kind, N, shape):
    if kind == "zero":
        return np.zeros((N,) + shape, np.uint8)
    if kind == "random":
        return rng.integers(0, 256, size=(N,) + shape).astype(np.uint8)
    m = (rng.random((N,) + shape) < 0.4).astype(np.uint8)
    if kind == "0255":
        m *= 255
    elif kind == "01_two_last":
        m.reshape(-1)[-1] = 2
    elif kind == "01_two_first":
        m.reshape(-1)[0] = 2
    return m


def raw_call(N, n_px, pred, thr, gt, cut_raw, cut_scaled, out):
    rc = lib().adp_fat_counts(N, n_px, pred, thr, gt, cut_raw, cut_scaled, out, stream_ptr())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("N", [1, 2, 5])
@pytest.mark.parametrize("shape", SHAPES)
def test_fat_counts_match_the_restatement(shape, N):
    rng = np.random.default_rng(1000 * N + shape[0] * shape[1])
    masks = {k: make_mask(rng, k, N, shape) for k in MASK_KINDS}
    dmasks = {k: torch.from_numpy(m).to(DEV) for k, m in masks.items()}
    for thr in THRESHOLDS:
        pred = make_pred(rng, N, shape, thr)
        dpred = torch.from_numpy(pred).to(DEV)
        for kind in MASK_KINDS:
            got = TC.fat_counts(dpred, dmasks[kind], thr)
            assert got.dtype == np.uint64 and got.shape == (N, 4)
            assert np.array_equal(got, TC.fat_counts_ref(pred, masks[kind], thr)), (kind, thr)
        # one input only: the other's columns stay zero
        only_p, only_g = TC.fat_counts(dpred, None, thr), TC.fat_counts(None, dmasks["random"], thr)
        assert np.array_equal(only_p, TC.fat_counts_ref(pred, None, thr)) and not only_p[:, 1:].any()
        assert np.array_equal(only_g, TC.fat_counts_ref(None, masks["random"], thr)) and not only_g[:, 0].any()
        # every planted value at the first pixel of the first image and at the last pixel of the last one
        for v in planted(thr):
            pred.reshape(-1)[0] = pred.reshape(-1)[-1] = v
            dpred.view(-1)[0] = float(v)
            dpred.view(-1)[-1] = float(v)
            assert np.array_equal(TC.fat_counts(dpred, None, thr), TC.fat_counts_ref(pred, None, thr)), (v, thr)
        # host arrays take the device too, and percentages are the counts over the pixels
        pp, gp = TC.fat_percentages(pred, masks["0255"], thr)
        c = TC.fat_counts_ref(pred, masks["0255"], thr)
        n_px = shape[0] * shape[1]
        assert np.array_equal(pp, c[:, 0].astype(np.float64) / n_px * 100.0)
        assert np.array_equal(gp, TC.gt_count(c).astype(np.float64) / n_px * 100.0)
        assert TC.calculate_fat_percentage(dpred[0], thr) == pp[0]
        assert TC.calculate_fat_percentage(dmasks["0255"][0], thr) == c[0, 2] / n_px * 100.0


def test_fat_counts_three_tiles_of_1024():
    rng = np.random.default_rng(7)
    pred = make_pred(rng, 3, (1024, 1024), 0.5)
    mask = make_mask(rng, "01_two_last", 3, (1024, 1024))
    mask[1] *= 255
    dp, dm = torch.from_numpy(pred).to(DEV), torch.from_numpy(mask).to(DEV)
    want = TC.fat_counts_ref(pred, mask, 0.5)
    got = TC.fat_counts(dp, dm, 0.5)
    assert np.array_equal(got, want)
    assert want[:, 1].tolist() == [1, 255, 2] and TC.gt_count(want).tolist() == [want[0, 2], want[1, 3], want[2, 3]]
    assert np.array_equal(TC.fat_counts(dp, dm, 0.5), got)   # two calls: identical


def test_views_and_unaligned_bases():
    rng = np.random.default_rng(11)
    big = make_pred(rng, 3, (40, 50), 0.5)
    bigm = make_mask(rng, "random", 3, (40, 50))
    dbig, dbigm = torch.from_numpy(big).to(DEV), torch.from_numpy(bigm).to(DEV)
    for sl in ((slice(None), slice(None, None, 2), slice(1, None)), (slice(None, None, 2), slice(3, 30), slice(None, None, 3))):
        v, vm = dbig[sl], dbigm[sl]
        assert not v.is_contiguous()
        got = TC.fat_counts(v, vm, 0.5)
        assert np.array_equal(got, TC.fat_counts(v.contiguous(), vm.contiguous(), 0.5))
        assert np.array_equal(got, TC.fat_counts_ref(big[sl], bigm[sl], 0.5))
    # contiguous planes whose first image already starts off the 16-byte alignment (float + 4 bytes, bytes + 1, + 3)
    N, n_px = 3, B + 13
    pred, mask = make_pred(rng, N, (1, n_px), 0.3), make_mask(rng, "random", N, (1, n_px))
    cut_raw, cut_scaled = TC.gt_cuts(0.3)
    for off_p, off_g in ((1, 1), (3, 3), (2, 15)):
        fbuf = torch.zeros(N * n_px + 8, dtype=torch.float32, device=DEV)
        gbuf = torch.zeros(N * n_px + 32, dtype=torch.uint8, device=DEV)
        fbuf[off_p:off_p + N * n_px] = torch.from_numpy(pred.reshape(-1)).to(DEV)
        gbuf[off_g:off_g + N * n_px] = torch.from_numpy(mask.reshape(-1)).to(DEV)
        out = torch.full((N, 4), 77, dtype=torch.int64, device=DEV)
        assert raw_call(N, n_px, ptr(fbuf[off_p:]), float(np.float32(0.3)), ptr(gbuf[off_g:]), cut_raw, cut_scaled, ptr(out)) == 0
        assert np.array_equal(out.cpu().numpy().view(np.uint64), TC.fat_counts_ref(pred, mask, 0.3))


def test_failure_cases_leave_out_untouched():
    N, n_px = 2, 100
    p = torch.rand(N, n_px, device=DEV)
    g = torch.randint(0, 256, (N, n_px), dtype=torch.uint8, device=DEV)
    out = torch.full((N, 4), SENTINEL, dtype=torch.int64, device=DEV)
    P, G, O = ptr(p), ptr(g), ptr(out)
    cases = [("N must", (-1, n_px, P, 0.5, G, 1, 128, O)),
             ("N must", (65536, n_px, P, 0.5, G, 1, 128, O)),
             ("n_px must", (N, 0, P, 0.5, G, 1, 128, O)),
             ("both be null", (N, n_px, None, 0.5, None, 1, 128, O)),
             ("out must", (N, n_px, P, 0.5, G, 1, 128, None)),
             ("cut_raw and cut_scaled must", (N, n_px, P, 0.5, G, -1, 128, O)),
             ("cut_raw and cut_scaled must", (N, n_px, P, 0.5, G, 257, 128, O)),
             ("cut_raw and cut_scaled must", (N, n_px, P, 0.5, G, 1, -1, O)),
             ("cut_raw and cut_scaled must", (N, n_px, P, 0.5, G, 1, 257, O))]
    for msg, a in cases:
        assert raw_call(*a) < 0, msg
        assert msg in lib().adp_last_error().decode(), (msg, lib().adp_last_error())
        assert (out == SENTINEL).all().item(), msg
    assert raw_call(0, n_px, P, 0.5, G, 1, 128, O) == 0   # N = 0: nothing to do, nothing written
    assert (out == SENTINEL).all().item()
    assert raw_call(N, n_px, P, 0.5, G, 0, 256, O) == 0   # the cuts' ends are legal: every byte counts, none does
    assert out.cpu().numpy()[:, 2:].tolist() == [[n_px, 0]] * N


# ------------------------------------------------------------------------------ pipeline
MEAN, STD = 120.0, 40.0


@pytest.fixture(scope="module")
def small_predictor():
    w = R.adipose_v3_keras_weights(seed=865, deep_supervision=False)
    net = AdiposeV3Net(1, 64, dtype="f32", device=DEV, deep_supervision=False)
    net.set_weights(w)
    return HipUnetPredictor(net, max_batch=8)


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """The golden's 9-tile 64 x 64 set (PNG content under *.jpg names, TIFF masks; one tile has no mask)."""
    from PIL import Image
    base = tmp_path_factory.mktemp("tilefat_gpu")
    root, ckpt = base / "clean_test", base / "ckpt"
    (root / "images").mkdir(parents=True)
    (root / "masks").mkdir()
    ckpt.mkdir()
    for k in GOLD.files:
        if k.startswith("eval_tile_"):
            Image.fromarray(GOLD[k]).save(root / "images" / f"{k[10:]}.jpg", format="PNG")
        elif k.startswith("eval_mask_"):
            Image.fromarray(GOLD[k]).save(root / "masks" / f"{k[10:]}.tif", format="TIFF")
    (ckpt / "normalization_stats.json").write_text(json.dumps({"mean": MEAN, "std": STD}))
    return root, ckpt / "best.weights.h5"


def make_args(root, weights, **kw):
    a = dict(weights=str(weights), data_root=str(root), output_dir=None, threshold=10.0, mask_threshold=0.5,
             multi_threshold=None, use_tta=False, tta_mode="basic", boundary_refine=False, refine_kernel=5, tile=64,
             dtype="f32", batch=4)
    a.update(kw)
    return argparse.Namespace(**a)


@pytest.mark.parametrize("variant", ["plain", "tta_full", "refine"])
def test_evaluate_tiles_equals_host_counts_of_the_same_maps(small_predictor, dataset, variant):
    """evaluate_tiles' percentages (maps counted on the device) = the same maps copied to the host and counted by the
    restatement; the maps come from predict_views over the same chunks of tiles."""
    root, weights = dataset
    args = make_args(root, weights, use_tta=variant == "tta_full", tta_mode="full", boundary_refine=variant == "refine")
    res = TC.evaluate_tiles(args, 10.0, model=small_predictor)
    paired = TC.find_paired_tiles(root)
    assert [r["tile_name"] for r in res["per_tile_results"]] == [p.stem for p, _ in paired] and len(paired) == 8
    views = TTA_VIEWS["full"] if args.use_tta else [0]
    refiner = BoundaryRefiner(kernel_size=5, bilateral_d=5, bilateral_sigma_color=50, bilateral_sigma_space=50)
    want_p, want_g = [], []
    for k0 in range(0, len(paired), args.batch):
        chunk = paired[k0:k0 + args.batch]
        maps = small_predictor.predict_views([read_image_gray(str(p)) for p, _ in chunk], MEAN, STD, views)
        if args.boundary_refine:
            maps = torch.stack([refiner.refine_device(m) for m in maps])
        masks = np.stack([GOLD[f"eval_mask_{p.stem}"] for p, _ in chunk])
        c = TC.fat_counts_ref(maps.cpu().numpy(), masks, 0.5)
        want_p.extend(c[:, 0].astype(np.float64) / 4096 * 100.0)
        want_g.extend(TC.gt_count(c).astype(np.float64) / 4096 * 100.0)
    assert [r["predicted_fat_pct"] for r in res["per_tile_results"]] == want_p
    assert [r["ground_truth_fat_pct"] for r in res["per_tile_results"]] == want_g
    assert [r["ground_truth_fat_pct"] for r in res["per_tile_results"]] == GOLD["eval_none_0.5_10.0_gt_pct"].tolist()


def test_one_pass_with_a_cache_equals_three_passes(small_predictor, dataset):
    root, weights = dataset
    args = make_args(root, weights)
    cache = {}
    for t in (1.0, 10.0, 50.0):
        one = TC.evaluate_tiles(args, t, model=small_predictor, fat_cache=cache)
        own = TC.evaluate_tiles(args, t, model=small_predictor)
        assert one["confusion_matrix"] == own["confusion_matrix"] and one["metrics"] == own["metrics"]
        assert one["per_tile_results"] == own["per_tile_results"]
