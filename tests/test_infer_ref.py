"""oracle/infer_ref.py checked on the CPU against independent implementations: the brute-force EDT against
scipy.ndimage.distance_transform_edt on every mask family, the integer-count ROC AUC and the grouped average
precision against scikit-learn on every score family, the sequential float32 TTA merge against np.mean of the
stack, and the float32 blending restatement against oracle/numpy_ref's two reconstructions."""
import numpy as np
import pytest

from oracle import infer_ref as IR
from oracle import numpy_ref as NR


@pytest.mark.parametrize("shape", IR.EDT_SHAPES, ids=[f"{h}x{w}" for h, w in IR.EDT_SHAPES])
def test_edt_brute_vs_scipy(shape):
    """Exact samplings: scipy's own arithmetic is exact there too, so the two agree to the last bit or to one
    rounding of scipy's sqrt argument; the gate is the project's 1e-9 * max(1, ref.max()) throughout. A mask
    without a zero pixel is undefined in scipy and is not part of any family."""
    from scipy import ndimage
    H, W = shape
    for name, m in IR.edt_masks(H, W):
        assert not m.all(), name
        for sp in IR.EDT_EXACT_SAMPLINGS + [IR.EDT_INEXACT_SAMPLING]:
            if H * W * int((~m).sum()) > IR.EDT_BRUTE_BUDGET:
                continue
            got = IR.edt_brute(m, sp)
            ref = ndimage.distance_transform_edt(m, sampling=sp)
            assert np.abs(got - ref).max() <= 1e-9 * max(1.0, ref.max()), (name, sp)
            assert (got[~m] == 0).all() and (got[m] > 0).all()


def test_edt_brute_known_answers():
    m = np.ones((3, 5), bool)
    m[1, 1] = False
    d = IR.edt_brute(m, (2.0, 3.0))
    assert d[1, 1] == 0 and d[0, 1] == 2 and d[1, 4] == 9 and d[2, 2] == np.sqrt(13.0) and d[0, 4] == np.sqrt(85.0)
    with pytest.raises(ValueError):
        IR.edt_brute(np.ones((2, 2), bool))


@pytest.mark.parametrize("n", IR.AUC_N)
def test_auc_exact_and_ap_vs_sklearn(n):
    from sklearn.metrics import average_precision_score, roc_auc_score
    names = set()
    for name, s, y in IR.auc_cases(n):
        names.add(name)
        roc, ap = IR.auc_exact(s, y), IR.average_precision(s, y)
        yt = (y > 0.5).astype(int)
        if yt.min() == yt.max():                      # scikit-learn refuses a single class; the reference returns NaN
            assert np.isnan(roc) and np.isnan(ap), name
            continue
        assert 0.0 <= roc <= 1.0 and 0.0 < ap <= 1.0
        assert abs(roc - roc_auc_score(yt, s)) <= 1e-9, (name, roc)
        assert abs(ap - average_precision_score(yt, s)) <= 1e-9, (name, ap)
    assert {"continuous", "levels3", "levels17", "allequal", "signedzeros", "range-2to3", "subnormal",
            "allnegative", "allpositive"} <= names
    assert n < 2 or {"onepositive", "onenegative"} <= names


def test_auc_exact_known_answers():
    y = np.array([0, 0, 1, 1], np.float32)
    assert IR.auc_exact([0.1, 0.4, 0.35, 0.8], y) == 0.75
    assert IR.auc_exact([0.5, 0.5, 0.5, 0.5], y) == 0.5 and IR.average_precision([0.5] * 4, y) == 0.5
    assert IR.auc_exact([-0.0, 0.0, 0.0, -0.0], y) == 0.5                # one group
    assert IR.auc_exact([0.0, 0.0, 1e-45, 1e-45], y) == 1.0              # the smallest subnormal is its own group
    assert IR.auc_exact([1, 2, 3], [1, 0, 1]) == 0.5 and IR.auc_exact([1, 2, 3], [0, 0, 1]) == 1.0
    assert IR.average_precision([0.1, 0.4, 0.35, 0.8], y) == pytest.approx(0.5 * 1.0 + 0.5 * (2 / 3))
    assert np.isnan(IR.auc_exact([0.3], [1])) and np.isnan(IR.average_precision([0.3, 0.2], [0, 0]))


VIEW_LISTS = [NR.TTA_MODES["minimal"], NR.TTA_MODES["basic"], NR.TTA_MODES["full"], [3], [6, 2, 7, 0, 5, 3, 1, 4],
              [1, 4, 1, 6]]


@pytest.mark.parametrize("S", [1, 5, 64])
def test_tta_merge_seq_is_numpy_mean_of_the_stack(S):
    rng = np.random.default_rng(S)
    for views in VIEW_LISTS:
        per_view = rng.random((len(views), S, S)).astype(np.float32)
        seq = IR.tta_merge_seq(per_view, views)
        stack = np.stack([NR.TTA_TRANSFORMS[v][1](p) for p, v in zip(per_view, views)])
        ref = np.mean(stack, axis=0)
        assert seq.dtype == np.float32 and ref.dtype == np.float32
        np.testing.assert_array_equal(seq, ref)
        f64 = IR.tta_merge_f64(per_view, views)
        # nv - 1 additions and one division in float32, per pixel
        assert (np.abs(seq - f64) <= (len(views) + 1) * 2.0 ** -24 * np.abs(stack).mean(axis=0)).all()
        # each transform pair is an inverse pair
        img = rng.random((S, S)).astype(np.float32)
        for v in views:
            aug, deaug = NR.TTA_TRANSFORMS[v]
            np.testing.assert_array_equal(deaug(aug(img)), img)


def test_prep_input_reference_views_and_padding():
    rng = np.random.default_rng(0)
    img = (rng.random((2, 5, 9, 3)) * 255).astype(np.float32)
    out = IR.prep_input(img, 120.5, 33.25, 4, 8)
    assert out.shape == (2, 5, 9, 8) and out.dtype == np.float32 and not out[..., 3:].any()
    np.testing.assert_array_equal(out[1, 2, 0, :3], (img[1, 2, 8] - np.float32(120.5)) / np.float32(33.25))
    sq = (rng.random((1, 7, 7)) * 255).astype(np.float32)
    out = IR.prep_input(sq, 120.5, 33.25, 1, 8)
    np.testing.assert_array_equal(out[0, :, :, 0], (np.rot90(sq[0]) - np.float32(120.5)) / np.float32(33.25))


@pytest.mark.parametrize("shape,T,ov", [((70, 93), 32, 0.25), ((70, 93), 33, 0.5), ((33, 33), 32, 0.5)])
def test_blend_restatement_matches_numpy_ref(shape, T, ov):
    rng = np.random.default_rng(T)
    pos = NR.tile_positions(shape, T, ov)
    assert any(y + T == shape[0] for y, _ in pos) and any(x + T == shape[1] for _, x in pos)
    tiles = [rng.random((T, T)).astype(np.float32) for _ in pos]
    wm = NR.gaussian_weight_map(T)
    acc, ws = IR.blend_accumulate(tiles, pos, shape, wm)
    np.testing.assert_array_equal(IR.blend_finalize(acc, ws, 1e-8), NR.gaussian_reconstruct(tiles, pos, shape, wm))
    acc, ws = IR.blend_accumulate(tiles, pos, shape, None)
    np.testing.assert_array_equal(IR.blend_finalize(acc, ws, 1.0), NR.linear_reconstruct(tiles, pos, shape))
    # a band fed its own tiles equals the same rows of the full canvas when no other tile reaches into it
    ys = sorted({y for y, _ in pos})
    band = [(k, p) for k, p in enumerate(pos) if p[0] == ys[-1]]
    bacc, bws = IR.blend_accumulate([tiles[k] for k, _ in band], [p for _, p in band], shape, wm, rows=(ys[-1], shape[0]))
    only = IR.blend_accumulate([tiles[k] for k, _ in band], [p for _, p in band], shape, wm)
    np.testing.assert_array_equal(bacc, only[0][ys[-1]:])
    np.testing.assert_array_equal(bws, only[1][ys[-1]:])
