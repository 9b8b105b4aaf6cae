"""The kernels between the network's output and a reported number -- csrc/infer.hip (input preparation with the TTA
view folded in, TTA merge, tile blending), csrc/metrics.hip (ROC AUC / average precision, the exact Euclidean
distance transform, the boundary metrics) and csrc/refine.hip (the boundary refiner) -- against the plain references
of oracle/infer_ref.py and oracle/numpy_ref.py (checked on the CPU by tests/test_infer_ref.py and
tests/test_evaluation.py), at the shapes where kernels of this form go wrong: one pixel, odd and non-square sizes,
sizes around the block edges, images smaller than a footprint, grids that wrap, ties and signed zeros.

Gates:
  prep_input, blending, refiner   bit equality with the float32 / uint8 restatement
  tta_merge                       bit equality with the sequential float32 sum / f32(nv), and within
                                  (nv + 1) * 2^-24 * mean|p| of the float64 mean (nv - 1 additions, one division)
  distance transform              equality with the brute-force reference at samplings whose squares and sums are
                                  exact in float64; 1e-9 * max(1, ref.max()) against scipy otherwise
  ROC AUC                         bit equality with float(Fraction(num2, 2 P N)) (integer and half terms below 2^53)
  average precision, boundary     the project's 1e-9
Every device output is a view of a buffer one row longer, filled with 7.0: the tail must survive the launch."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from adipose_amd import evaluation as E
from adipose_amd import ops
from adipose_amd import predictor as P
from adipose_amd._lib import call, ptr, stream_ptr
from oracle import infer_ref as IR
from oracle import numpy_ref as NR

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16, F64, U8 = torch.float32, torch.bfloat16, torch.float64, torch.uint8
U24 = 2.0 ** -24
MEAN, STD = 120.5, 33.25          # exactly representable in f32, not trivial


class Guarded:
    """An output of `shape` as a view of a buffer one row (`pad` elements) longer, all 7.0."""

    def __init__(self, shape, dt=F32, pad=None):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + (pad if pad is not None else shape[-1]),), 7.0, dtype=dt, device=DEV)
        self.t = self.buf[:self.n].view(*shape)

    def zero(self):
        self.t.zero_()
        return self

    def ok(self):
        torch.cuda.synchronize()
        assert bool((self.buf[self.n:] == 7.0).all()), "wrote past the end of the output"
        return self.t


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def assert_bits(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    bad = bits(got) != bits(ref)
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} differ, first at {tuple(np.argwhere(bad)[0])}: "
                           f"got {got[bad][0]!r}, ref {ref[bad][0]!r}")


# --------------------------------------------------------------------------------------------- adp_prep_input
def windowed(N, H, W, Cin, seed):
    """A (N, H, W[, Cin]) source as an interior window of a parent (N, H + 6, W + 10[, Cin]): the row stride is
    not W, the image stride is not H * W, and a wrong row or column index stays inside the allocation."""
    rng = np.random.default_rng(seed)
    shape = (N, H + 6, W + 10) + ((Cin,) if Cin > 1 else ())
    parent = (rng.random(shape) * 255).astype(np.float32)
    dpar = torch.from_numpy(parent).to(DEV)
    return parent[:, 3:3 + H, 5:5 + W], dpar[:, 3:3 + H, 5:5 + W]


def check_prep(N, H, W, Cin, Cs, dt, view, seed=0):
    host, win = windowed(N, H, W, Cin, seed)
    dst = Guarded((N, H, W, Cs), dt)
    ops.prep_input(win, dst.t, mean=MEAN, std=STD, view=view)
    ref = torch.from_numpy(IR.prep_input(host, MEAN, STD, view, Cs)).to(dt)      # torch casts round-to-nearest-even
    got = dst.ok().cpu()
    what = f"prep N{N} {H}x{W} Cin{Cin} Cs{Cs} {dt} view{view}"
    assert_bits(got.float().numpy(), ref.float().numpy(), what)
    assert float(got[..., Cin:].float().abs().max()) == 0.0, what + ": pad channels"


@pytest.mark.parametrize("S", [1, 7, 40])
@pytest.mark.parametrize("view", range(8))
def test_prep_input_all_views_on_squares(view, S):
    for dt in (F32, BF16):
        for Cin in (1, 3):
            for Cs in (8, 16):
                for N in (1, 3):
                    check_prep(N, S, S, Cin, Cs, dt, view, seed=view + 8 * S)


@pytest.mark.parametrize("shape", [(5, 9), (9, 5), (37, 53)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("view", [0, 4, 5])
def test_prep_input_flips_on_non_square_tiles(view, shape):
    """Views 0, 4 and 5 are admitted on non-square tiles. The flip along axis 1 mirrors columns in W (it once
    mirrored them in H: wrong for H != W, and outside the row for H < W)."""
    H, W = shape
    for dt in (F32, BF16):
        for Cin in (1, 3):
            for Cs in (8, 16):
                for N in (1, 3):
                    check_prep(N, H, W, Cin, Cs, dt, view, seed=view + H)


def test_prep_input_grid_wraps():
    """1500 x 1400 = 2 100 000 pixels: more than the 8192 blocks of 256 the launch is capped at."""
    assert 1500 * 1400 > 8192 * 256
    check_prep(1, 1500, 1400, 1, 8, F32, 5)


def test_prep_input_refuses_rotations_of_non_square_tiles():
    _, win = windowed(1, 5, 9, 1, 0)
    dst = Guarded((1, 5, 9, 8))
    for view in (1, 2, 3, 6, 7):
        with pytest.raises(Exception, match="square"):
            ops.prep_input(win, dst.t, mean=MEAN, std=STD, view=view)
    assert bool((dst.ok() == 7.0).all())


# --------------------------------------------------------------------------------------------- adp_tta_merge
VIEW_LISTS = [NR.TTA_MODES["minimal"], NR.TTA_MODES["basic"], NR.TTA_MODES["full"], [3], [6, 2, 7, 0, 5, 3, 1, 4],
              [1, 4, 1, 6]]


def check_merge(S, views, seed):
    rng = np.random.default_rng(seed)
    per_view = rng.random((len(views), S, S)).astype(np.float32)
    out = Guarded((S, S))
    ops.tta_merge(torch.from_numpy(per_view).to(DEV), views, out.t)
    got = out.ok().cpu().numpy()
    assert_bits(got, IR.tta_merge_seq(per_view, views), f"tta_merge S{S} views{views}")
    stack = np.stack([NR.TTA_TRANSFORMS[v][1](p) for p, v in zip(per_view, views)]).astype(np.float64)
    tol = (len(views) + 1) * U24 * np.abs(stack).mean(axis=0)
    assert (np.abs(got - stack.mean(axis=0)) <= tol).all()


@pytest.mark.parametrize("S", [1, 5, 64])
def test_tta_merge_sequential_f32(S):
    for k, views in enumerate(VIEW_LISTS):
        check_merge(S, views, 10 * S + k)


def test_tta_merge_grid_wraps():
    assert 1500 * 1500 > 8192 * 256
    check_merge(1500, [4, 1], 3)


# --------------------------------------------------------------------------------------------- blending
def blend_case(shape, T, ov, seed, xlimit=None):
    rng = np.random.default_rng(seed)
    pos = NR.tile_positions(shape if xlimit is None else (shape[0], xlimit), T, ov)
    tiles = [rng.random((T, T)).astype(np.float32) for _ in pos]
    return pos, tiles


def run_blend(canvas_rows, shape, pos, tiles, wmap):
    """Feeds the tiles to a BandCanvas over `canvas_rows` whose buffer is guarded; returns (canvas, guard)."""
    c = P.BandCanvas(shape, canvas_rows, DEV)
    g = Guarded(tuple(c.buf.shape)).zero()
    c.buf = g.t
    c.acc, c.ws = c.buf[0], c.buf[1]
    dw = None if wmap is None else torch.from_numpy(np.ascontiguousarray(wmap)).to(DEV)
    for t, (y, x) in zip(tiles, pos):
        c.add(torch.from_numpy(t).to(DEV), dw, y, x)
    g.ok()
    return c, g


def finalize(c, floor_):
    out = Guarded(tuple(c.acc.shape))
    ops.blend_finalize(c.acc, c.ws, out.t, floor_)
    return out.ok().cpu().numpy()


@pytest.mark.parametrize("gauss", [True, False], ids=["gaussian", "linear"])
@pytest.mark.parametrize("ov", [0.25, 0.5])
@pytest.mark.parametrize("T", [32, 33])
@pytest.mark.parametrize("shape", [(70, 93), (33, 33)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_blend_accum_finalize_bit_equal(shape, T, ov, gauss):
    """adp_blend_accum (weight map or NULL) and adp_blend_finalize bit for bit against the float32 restatement, tiles
    flush with the right and bottom edges included."""
    pos, tiles = blend_case(shape, T, ov, T + int(100 * ov))
    assert any(y + T == shape[0] for y, _ in pos) and any(x + T == shape[1] for _, x in pos)
    wmap, floor_ = (NR.gaussian_weight_map(T), 1e-8) if gauss else (None, 1.0)
    c, _ = run_blend((0, shape[0]), shape, pos, tiles, wmap)
    acc, ws = IR.blend_accumulate(tiles, pos, shape, wmap)
    assert_bits(c.acc.cpu().numpy(), acc, "acc")
    assert_bits(c.ws.cpu().numpy(), ws, "wsum")
    got = finalize(c, floor_)
    assert_bits(got, IR.blend_finalize(acc, ws, floor_), "finalize")
    ref = NR.gaussian_reconstruct(tiles, pos, shape, wmap) if gauss else NR.linear_reconstruct(tiles, pos, shape)
    assert_bits(got, ref, "reconstruction")


@pytest.mark.parametrize("gauss", [True, False], ids=["gaussian", "linear"])
def test_blend_uncovered_strip_finalizes_to_zero(gauss):
    """Tiles cover the columns [0, 64) of a (70, 93) canvas only: 0 / floor = 0 in the strip, the blend elsewhere."""
    shape, T = (70, 93), 32
    pos, tiles = blend_case(shape, T, 0.5, 5, xlimit=64)
    wmap, floor_ = (NR.gaussian_weight_map(T), 1e-8) if gauss else (None, 1.0)
    c, _ = run_blend((0, shape[0]), shape, pos, tiles, wmap)
    got = finalize(c, floor_)
    acc, ws = IR.blend_accumulate(tiles, pos, shape, wmap)
    assert not ws[:, 64:].any() and ws[:, :64].all()
    assert_bits(got[:, 64:], np.zeros((70, 29), np.float32), "uncovered strip")
    assert_bits(got, IR.blend_finalize(acc, ws, floor_), "finalize")


@pytest.mark.parametrize("gauss", [True, False], ids=["gaussian", "linear"])
@pytest.mark.parametrize("T", [32, 33])
def test_band_canvas_equals_rows_of_full_canvas(T, gauss):
    """A BandCanvas over rows [y0, y1), y0 > 0, fed the tiles of that band, holds before finalize the bits a
    full-frame canvas fed the same tiles holds in those rows (and the restatement's)."""
    shape = (70, 93)
    pos, tiles = blend_case(shape, T, 0.5, 9 + T)
    ys = sorted({y for y, _ in pos})
    assert len(ys) >= 3
    keep = [k for k, (y, _) in enumerate(pos) if y >= ys[1]]
    bpos, btiles = [pos[k] for k in keep], [tiles[k] for k in keep]
    rows = P.band_rows(bpos, T)
    assert rows[0] > 0 and rows[1] == shape[0]
    wmap = NR.gaussian_weight_map(T) if gauss else None
    band, _ = run_blend(rows, shape, bpos, btiles, wmap)
    full, _ = run_blend((0, shape[0]), shape, bpos, btiles, wmap)
    fa, fw = full.acc.cpu().numpy(), full.ws.cpu().numpy()
    assert_bits(band.acc.cpu().numpy(), fa[rows[0]:rows[1]], "band acc")
    assert_bits(band.ws.cpu().numpy(), fw[rows[0]:rows[1]], "band wsum")
    assert not fa[:rows[0]].any() and not fw[:rows[0]].any()
    acc, ws = IR.blend_accumulate(btiles, bpos, shape, wmap, rows=rows)
    assert_bits(band.acc.cpu().numpy(), acc, "band acc vs restatement")
    assert_bits(band.ws.cpu().numpy(), ws, "band wsum vs restatement")


def test_blend_finalize_grid_wraps():
    H, W = 1500, 1400
    assert H * W > 8192 * 256
    rng = np.random.default_rng(11)
    acc = rng.random((H, W)).astype(np.float32) * 3
    ws = (rng.random((H, W)).astype(np.float32) * 3) * (rng.random((H, W)) > 0.1)
    acc[ws == 0] = 0
    out = Guarded((H, W))
    ops.blend_finalize(torch.from_numpy(acc).to(DEV), torch.from_numpy(ws).to(DEV), out.t, 1e-8)
    assert_bits(out.ok().cpu().numpy(), IR.blend_finalize(acc, ws, 1e-8), "finalize")


# --------------------------------------------------------------------------------------------- distance transform
def gpu_edt(m, sampling):
    """adp_distance_transform as evaluation.distance_transform_edt calls it (sites: mask == 0), guarded output."""
    H, W = m.shape
    src = torch.from_numpy((~m).astype(np.float32)).to(DEV)
    out = Guarded((H, W), F64)
    call("adp_distance_transform", H, W, ptr(src), 0.5, float(sampling[0]), float(sampling[1]), ptr(out.t), stream_ptr())
    return out.ok().cpu().numpy()


@pytest.mark.parametrize("shape", IR.EDT_SHAPES, ids=[f"{h}x{w}" for h, w in IR.EDT_SHAPES])
def test_distance_transform_exact_and_vs_scipy(shape):
    """At samplings (1, 1), (2, 3) and (0.5, 2) every square and sum is exact in float64 and sqrt is correctly
    rounded: the result equals the brute-force reference (where pixels x zeros stays within its budget) however
    the parabola intersections break ties between equidistant sites. At (0.7, 1.3) the project's gate against
    scipy. A mask without a zero is undefined in scipy and is not among the families."""
    from scipy import ndimage
    H, W = shape
    for name, m in IR.edt_masks(H, W):
        for sp in IR.EDT_EXACT_SAMPLINGS:
            got = gpu_edt(m, sp)
            ref = ndimage.distance_transform_edt(m, sampling=sp)
            assert np.abs(got - ref).max() <= 1e-9 * max(1.0, ref.max()), (name, sp)
            if H * W * int((~m).sum()) <= IR.EDT_BRUTE_BUDGET:
                assert_bits(got, IR.edt_brute(m, sp), f"edt {shape} {name} {sp}")
        got = gpu_edt(m, IR.EDT_INEXACT_SAMPLING)
        ref = ndimage.distance_transform_edt(m, sampling=IR.EDT_INEXACT_SAMPLING)
        assert np.abs(got - ref).max() <= 1e-9 * max(1.0, ref.max()), name


# --------------------------------------------------------------------------------------------- ROC AUC / AP
def gpu_auc(s, y):
    p, t = torch.from_numpy(s).to(DEV), torch.from_numpy(y).to(DEV)
    out = Guarded((2,), F64, pad=2)
    call("adp_auc_metrics", p.numel(), ptr(p), ptr(t), ptr(out.t), stream_ptr())
    return out.ok().cpu().numpy()


@pytest.mark.parametrize("n", IR.AUC_N)
def test_auc_exact_and_average_precision(n):
    from sklearn.metrics import average_precision_score
    for name, s, y in IR.auc_cases(n):
        got = gpu_auc(s, y)
        roc, ap = IR.auc_exact(s, y), IR.average_precision(s, y)
        if math.isnan(roc):                                   # a single class (always at n = 1): both NaN
            assert np.isnan(got).all(), (name, got)
            continue
        assert got[0] == roc, (name, got[0], roc)
        assert abs(got[1] - ap) <= 1e-9, (name, got[1], ap)
        assert abs(got[1] - average_precision_score((y > 0.5).astype(int), s)) <= 1e-9, (name, got[1])


def test_auc_repeatable_and_on_a_side_stream():
    name, s, y = IR.auc_cases(3000)[0]
    first = gpu_auc(s, y)
    assert_bits(gpu_auc(s, y), first, "second run")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again = gpu_auc(s, y)
    torch.cuda.current_stream().wait_stream(side)
    assert_bits(again, first, "side stream")
    assert first[0] == IR.auc_exact(s, y)


# --------------------------------------------------------------------------------------------- boundary metrics
def boundary_cases(H, W):
    """[(name, pred, truth, threshold)] f32 maps of (H, W)."""
    rng = np.random.default_rng(H * 7 + W)
    z = np.zeros((H, W), np.float32)

    def px(y, x):
        m = z.copy()
        m[y, x] = 1
        return m

    yy, xx = np.mgrid[0:H, 0:W]
    cross = ((yy == H // 2) | (xx == W // 2)).astype(np.float32)               # touches all four borders
    frame = np.ones((H, W), np.float32)
    frame[1:-1, 1:-1][(yy[1:-1, 1:-1] + xx[1:-1, 1:-1]) % 3 == 0] = 0          # full border, holes inside
    part = (xx < W // 2).astype(np.float32)
    soft = np.clip(part * 0.6 + rng.random((H, W)) * 0.5 - 0.05, 0, 1).astype(np.float32)
    tie = np.where(rng.random((H, W)) < 0.5, np.float32(0.5), soft).astype(np.float32)
    tie[H // 2, W // 2], tie[0, 0] = 0.75, 0.5
    return [("pixel/pixel", px(H // 2, W // 2), px(0, 0), 0.5),
            ("pixel-corner/pixel-corner", px(H - 1, W - 1), px(0, W - 1), 0.5),
            ("cross/frame", cross, frame, 0.5),
            ("frame/cross", frame, cross, 0.5),
            ("allones/partial", np.ones((H, W), np.float32), part, 0.5),
            ("empty/empty", z, z, 0.5),
            ("empty/partial", z, part, 0.5),
            ("partial/empty", part, z, 0.5),
            ("soft/partial", soft, part, 0.3),
            ("threshold-equals-pixels", tie, part, 0.5)]


@pytest.mark.parametrize("spacing", [(1.0, 1.0), (1.0, 1.5)], ids=["iso", "aniso"])
@pytest.mark.parametrize("shape", [(5, 130), (130, 5), (64, 65)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_boundary_metrics_edges(shape, spacing):
    for name, p, t, thr in boundary_cases(*shape):
        got = E.calculate_boundary_metrics(p, t, thr, spacing=spacing)
        ref = NR.boundary_metrics(p, t, thr, spacing=spacing)
        for k in ("hausdorff95", "assd"):
            assert got[k] == ref[k] or abs(got[k] - ref[k]) <= 1e-9, (name, k, got, ref)


# --------------------------------------------------------------------------------------------- boundary refiner
def ramp_values():
    """float32(j / 255), j = 0..255, and the float32 neighbour on each side (kept inside [0, 1]): the truncation
    boundaries of uint8(mask * 255)."""
    c = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)
    v = np.stack([np.nextafter(c, np.float32(-1)), c, np.nextafter(c, np.float32(2))], axis=1).ravel()
    return np.clip(v, 0, 1).astype(np.float32)


def refine_inputs(H, W, seed):
    """Inputs stay inside [0, 1]: outside it, and for NaN, the reference's astype(uint8) is undefined."""
    from scipy import ndimage
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    sm = ndimage.gaussian_filter(rng.random((H, W)), min(3.0, max(H, W) / 4), mode="reflect")
    sm = np.clip((sm - sm.mean()) * 8 + 0.5, 0, 1).astype(np.float32)
    rad = max(H, W) * 0.45
    disc = (((yy - H * 0.3) ** 2 + (xx - W * 0.2) ** 2) < rad * rad).astype(np.float32)    # cut by two borders
    bars = (((xx // 3) % 2 == 0) | (yy == 0) | (yy == H - 1)).astype(np.float32)
    rv = ramp_values()
    ramp = np.resize(np.roll(rv, -int(rng.integers(0, rv.size))), (H, W)).astype(np.float32)
    return [("smoothed", sm), ("random", rng.random((H, W)).astype(np.float32)), ("disc", disc), ("bars", bars),
            ("ramp", ramp), ("zeros", np.zeros((H, W), np.float32)), ("ones", np.ones((H, W), np.float32))]


def gpu_refine(m, k, d, sc, ss):
    r = E.BoundaryRefiner(kernel_size=k, bilateral_d=d, bilateral_sigma_color=sc, bilateral_sigma_space=ss)
    H, W = m.shape
    work = Guarded((4, H, W), U8)
    out = Guarded((H, W))
    lo, hi = (C.c_int * k)(*r.rows[0]), (C.c_int * k)(*r.rows[1])
    dm = torch.from_numpy(m).to(DEV)
    call("adp_boundary_refine", H, W, ptr(dm), k, lo, hi, int(d), float(sc), float(ss), ptr(work.t), ptr(out.t),
         stream_ptr())
    work.ok()
    got = out.ok().cpu().numpy()
    assert_bits(r.refine(m), got, "BoundaryRefiner.refine vs the direct launch")
    return got


REFINE = [((1, 1), 5, 5, 50.0), ((2, 3), 5, 5, 50.0), ((3, 2), 5, 5, 50.0),
          ((1, 1), 7, 9, 50.0), ((2, 3), 7, 9, 50.0), ((3, 2), 7, 9, 50.0),     # smaller than either footprint
          ((7, 64), 1, 5, 50.0), ((65, 33), 1, 5, 50.0),                         # k = 1: no band, identity morphology
          ((40, 40), 31, 31, 50.0),                                              # the largest footprints
          ((24, 32), 5, 5, 50.0),                                                # 768 pixels: the whole ramp
          ((33, 20), 5, 0, 3.0), ((9, 11), 3, -1, 0.0)]                          # d <= 0: radius from sigma_space


@pytest.mark.parametrize("shape,k,d,ss", REFINE, ids=[f"{s[0]}x{s[1]}-k{k}-d{d}-ss{ss:g}" for s, k, d, ss in REFINE])
def test_boundary_refine_bit_equal(shape, k, d, ss):
    """adp_boundary_refine bit for bit against NR.boundary_refine. d <= 0 takes the radius round(1.5 sigma_space)
    (4 from 4.5 at sigma_space 3: half to even; sigma_space <= 0 counts as 1, radius 2)."""
    H, W = shape
    for name, m in refine_inputs(H, W, H * 100 + W + k):
        got = gpu_refine(m, k, d, 50.0, ss)
        ref = NR.boundary_refine(m, kernel_size=k, d=d, sigma_color=50.0, sigma_space=ss)
        assert_bits(got, ref, f"refine {shape} k{k} d{d} {name}")
        if name in ("zeros", "ones"):
            assert_bits(got, m, "fixed point")
