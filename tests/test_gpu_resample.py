"""adipose_amd.resample on the device (csrc/resample.hip: adp_resample_u8 / adp_resample_nearest_u8) against the numpy
path, bit for bit, in both of the device's forms: the fused launch (option resample_fused = 1) and the two launches
through an intermediate (0). The numpy path itself is held to Pillow in tests/test_resample.py. Shapes sit around the
fused form's output tile (TR x TC), the footprint that admits it, and the tap limit.
"""
import ctypes as CT
import os
import sys

import numpy as np
import pytest
import torch

from adipose_amd import resample as R
from adipose_amd.resample import KMAX, LDS_BYTES, TILE_COLS as TC, TILE_ROWS as TR

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_resample import _cli, _tree, check_cli_outputs, image  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _default_form():
    yield
    from adipose_amd import ops
    ops.set_option("resample_fused", None)


def both_forms(a, size, f, **kw):
    """The device's result in the two-launch form and in the fused form (where it fits; the same launches otherwise)."""
    from adipose_amd import ops
    out = []
    for form in (0, 1):
        ops.set_option("resample_fused", form)
        out.append(R.resize(a, size, f, **kw).cpu().numpy())
    ops.set_option("resample_fused", None)
    return out


def check(a, size, f, **kw):
    want = R.resize_np(a, size, f, **kw)
    two, fused = both_forms(a, size, f, **kw)
    assert two.shape == want.shape and two.dtype == np.uint8
    assert np.array_equal(two, want), ("two launches", a.shape, size, f)
    assert np.array_equal(fused, want), ("fused", a.shape, size, f)
    return want


# (H, W, Ho, Wo). The support exceeds tiny images on both sides, so their bounds clamp at both ends; the outputs sit at
# TR - 1 x TC + 1, TR + 1 x 2 TC + 3 and 3 TR + 5 x 3 TC + 7 (a block of the last has its whole support inside).
SHAPES = [
    (1, 1, 4, 3), (1, 7, 2, 5), (3, 5, 5, 3), (3, 5, 3, 9), (1, 1, 1, 1),
    (TR + 2, TC - 2, TR - 1, TC + 1),                       # the ECM case: three pixels off in each extent
    (14, 57, TR + 1, 2 * TC + 3),                           # about 2.3 x up
    (273, 538, 3 * TR + 5, 3 * TC + 7),                     # about 0.37 x down, 4 x 4 tiles
    (70, 131, 75, 131), (70, 131, 70, 120),                 # one extent: each pass alone, rows of an odd byte count
    (64, 132, 50, 132), (50, 132, 64, 128),                 # the same on whole words
]


@pytest.mark.parametrize("f", R.METHODS)
@pytest.mark.parametrize("C", [1, 3])
def test_device_equals_numpy(f, C):
    for H, W, Ho, Wo in SHAPES:
        a = image((H, W) if C == 1 else (H, W, C), 1)
        assert R.fused_fits(H, W, C, Ho, Wo, f) == (f != "nearest" and H != Ho and W != Wo)   # all of these fit
        check(a, (Wo, Ho), f)


@pytest.mark.parametrize("C", [2, 4])
def test_two_and_four_channels(C):
    a = image((45, 70, C), 2)
    for f in ("lanczos", "box", "nearest"):
        check(a, (TC + 5, TR + 9), f)


def test_clamp_on_binary_images():
    a = image((90, 100), 3, binary=True)                   # 0 / 255: sums below 0 and above 255 << 22
    for f in ("lanczos", "bicubic", "hamming"):
        want = check(a, (143, 61), f)
        assert want.min() == 0 and want.max() == 255


def test_batch_is_image_by_image():
    a = image((3, 40, 70, 3), 4)
    want = check(a, (TC + 3, TR + 3), "lanczos")
    for n in range(3):
        assert np.array_equal(want[n], R.resize_np(a[n], (TC + 3, TR + 3), "lanczos"))
    g = image((3, 40, 70), 5)
    check(g, (61, 37), "bilinear")
    check(g, (61, 37), "nearest")


def _last_fitting_height(Ho, W, C, Wo, f):
    """The largest H (down-scale to Ho rows) whose tiles' rows still fit the fused form's LDS."""
    H = Ho
    while R.fused_fits(H + 1, W, C, Ho, Wo, f):
        H += 1
    assert not R.fused_fits(H + 1, W, C, Ho, Wo, f) and H > 2 * Ho
    return H


@pytest.mark.parametrize("f,C", [("lanczos", 3), ("bilinear", 4), ("lanczos", 1)])
def test_footprint_decides_the_form(f, C):
    """Just inside and just outside what the fused form admits: both equal numpy, and with no intermediate to fall back
    on (tmp = NULL) the call succeeds exactly where the footprint fits."""
    from adipose_amd._lib import AdpError, call, ptr, stream_ptr
    from adipose_amd import ops
    Ho, W, Wo = TR + 1, 70, 60
    H_in = _last_fitting_height(Ho, W, C, Wo, f)
    for H, fits in ((H_in, True), (H_in + 1, False)):
        a = image((H, W, C), 6)
        want = check(a, (Wo, Ho), f)
        src = torch.from_numpy(a).cuda()
        dst = torch.full((Ho, Wo, C), 7, dtype=torch.uint8, device="cuda")
        xb, xk, xks = R.coefficients(W, Wo, f)
        yb, yk, yks = R.coefficients(H, Ho, f)
        rows = max(int(yb[min(y + TR, Ho) - 1].sum() - yb[y, 0]) for y in range(0, Ho, TR))
        assert (rows * TC * C <= LDS_BYTES) == fits
        args = (1, H, W, C, Ho, Wo, ptr(src), R._host_ptr(xb), R._host_ptr(xk), xks, R._host_ptr(yb), R._host_ptr(yk), yks,
                None, ptr(dst), stream_ptr())
        ops.set_option("resample_fused", 1)
        if fits:
            call("adp_resample_u8", *args)
            assert np.array_equal(dst.cpu().numpy(), want)
        else:
            with pytest.raises(AdpError, match="tmp must be non-null"):
                call("adp_resample_u8", *args)
            assert (dst == 7).all()
        ops.set_option("resample_fused", 0)                 # never fused: the intermediate is needed either way
        with pytest.raises(AdpError, match="tmp must be non-null"):
            call("adp_resample_u8", *args)


def test_tap_limit_and_unstaged_span():
    assert R.ksize_of(32 * 140, 140, "lanczos") == KMAX
    a = image((64, 32 * 140), 7)                            # 1 / 32 in both extents: KMAX taps, three column tiles
    check(a, (140, 2), "lanczos")
    a = image((96, 128, 3), 8)
    check(a, (4, 3), "lanczos")
    # the box filter 192 times down: KMAX taps, and a run's span (TC * 192 * 3 bytes) is beyond what a block stages
    assert R.ksize_of(192 * 70, 70, "box") == KMAX and TC * 192 * 3 > LDS_BYTES
    a = image((3, 192 * 70, 3), 9)
    check(a, (70, 3), "box")
    check(a, (70, 5), "box")
    with pytest.raises(ValueError, match="193"):
        R.resize(a, (69, 3), "box")


def test_side_stream_and_repeatability():
    a = image((2, 150, 210, 3), 10)
    want = R.resize_np(a, (97, 171), "lanczos")
    src = torch.from_numpy(a).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    from adipose_amd import ops
    for form in (0, 1):
        ops.set_option("resample_fused", form)
        with torch.cuda.stream(side):
            runs = [R.resize(src, (97, 171), "lanczos") for _ in range(3)]
            near = R.resize(src, (97, 171), "nearest")
        side.synchronize()
        for r in runs:
            assert np.array_equal(r.cpu().numpy(), want)
        assert np.array_equal(near.cpu().numpy(), R.resize_np(a, (97, 171), "nearest"))


def test_dispatch_and_callers_intermediate():
    a = image((40, 50, 3), 11)
    want = R.resize_np(a, (47, 43), "bicubic")
    out = R.resample_image_array(a, (47, 43), "bicubic")                       # array in, array out, through the device
    assert isinstance(out, np.ndarray) and np.array_equal(out, want)
    t = R.resample_image_array(torch.from_numpy(a).cuda(), (47, 43), "bicubic")
    assert t.is_cuda and np.array_equal(t.cpu().numpy(), want)
    t = R.Resampler((47, 43), "bicubic")(torch.from_numpy(a))                  # a host tensor comes back on the host
    assert not t.is_cuda and np.array_equal(t.numpy(), want)
    from adipose_amd import ops
    ops.set_option("resample_fused", 0)
    tmp = torch.full((40 * 47 * 3 + 5,), 9, dtype=torch.uint8, device="cuda")
    assert np.array_equal(R.resize(a, (47, 43), "bicubic", tmp=tmp).cpu().numpy(), want)
    hb, hk, _ = R.coefficients(50, 47, "bicubic")
    assert np.array_equal(tmp[:40 * 47 * 3].cpu().numpy().reshape(40, 47, 3), R.pass_np(a, hb, hk, 1))   # the uint8 image between
    assert (tmp[40 * 47 * 3:] == 9).all()
    with pytest.raises(ValueError, match="tmp must be"):
        R.resize(a, (47, 43), "bicubic", tmp=tmp[:100])
    with pytest.raises(TypeError):
        R.resize(torch.zeros(4, 4, device="cuda"), (3, 3))


def test_argument_errors():
    """Every documented failure returns its status with a message and leaves the output as it was; N = 0 launches
    nothing."""
    from adipose_amd._lib import AdpError, call, lib, ptr, stream_ptr
    N, H, W, C, Ho, Wo = 2, 40, 50, 3, 43, 47
    src = torch.from_numpy(image((N, H, W, C), 12)).cuda()
    dst = torch.full((N, Ho, Wo, C), 7, dtype=torch.uint8, device="cuda")
    tmp = torch.full((N, H, Wo, C), 7, dtype=torch.uint8, device="cuda")
    s, i, d, t = stream_ptr(), ptr(src), ptr(dst), ptr(tmp)
    xb, xk, xks = R.coefficients(W, Wo, "lanczos")
    yb, yk, yks = R.coefficients(H, Ho, "lanczos")
    P = R._host_ptr

    def conv(**kw):
        a = dict(N=N, H=H, W=W, C=C, Ho=Ho, Wo=Wo, src=i, xb=P(xb), xk=P(xk), xks=xks, yb=P(yb), yk=P(yk), yks=yks, tmp=t, dst=d)
        a.update(kw)
        return tuple(a.values()) + (s,)

    def edited(arr, at, v):
        e = arr.copy()
        e[at] = v
        keep.append(e)
        return P(e)

    keep = []
    huge = np.full_like(xk, 1 << 24)
    bad = [
        ("N must", conv(N=-1)), ("N must", conv(N=65536)), ("C must", conv(C=0)), ("C must", conv(C=5)),
        ("extent", conv(H=0)), ("extent", conv(W=0)), ("extent", conv(Ho=0)), ("extent", conv(Wo=0)),
        ("2\\^31", conv(N=1, H=1 << 16, W=1 << 14, C=2)), ("2\\^31", conv(N=1, Ho=1 << 16, Wo=1 << 14, C=2)),
        ("2\\^31", conv(N=1, H=1 << 16, Wo=1 << 14, C=2)),
        ("non-null", conv(src=None)), ("non-null", conv(dst=None)),
        ("horizontal bounds and taps must be non-null", conv(xb=None)), ("horizontal bounds and taps must be non-null", conv(xk=None)),
        ("vertical bounds and taps must be non-null", conv(yb=None)), ("vertical bounds and taps must be non-null", conv(yk=None)),
        ("horizontal ksize", conv(xks=0)), ("vertical ksize", conv(yks=KMAX + 1)),
        ("horizontal bounds must hold", conv(xb=edited(xb, (0, 0), -1))),
        ("horizontal bounds must hold", conv(xb=edited(xb, (Wo - 1, 1), xb[Wo - 1, 1] + 1))),        # lo + cnt = W + 1
        ("vertical bounds must hold", conv(yb=edited(yb, (5, 1), yks + 1))),
        ("vertical bounds must hold", conv(yb=edited(yb, (5, 1), -1))),
        ("horizontal bounds must not descend", conv(xb=edited(xb, (20, 0), xb[19, 0] - 1))),
        ("vertical bounds must not descend", conv(yb=edited(yb, (20, 1), yb[20, 1] - 2))),
        ("horizontal taps", conv(xk=P(huge))),
        ("overlap", conv(src=d)), ("overlap", conv(tmp=i)), ("overlap", conv(tmp=d)),
        ("overlap", conv(N=1, dst=CT.c_void_p(src.data_ptr() + H * W * C - 1))),
    ]
    from adipose_amd import ops
    ops.set_option("resample_fused", 0)
    bad_two = [("tmp must be non-null", conv(tmp=None))]
    xi, yi = R.nearest_table(W, Wo), R.nearest_table(H, Ho)

    def near(**kw):
        a = dict(N=N, H=H, W=W, C=C, Ho=Ho, Wo=Wo, src=i, xi=P(xi), yi=P(yi), dst=d)
        a.update(kw)
        return tuple(a.values()) + (s,)

    bad_near = [
        ("N must", near(N=-1)), ("N must", near(N=65536)), ("C must", near(C=5)), ("extent", near(Wo=0)), ("extent", near(H=0)),
        ("2\\^31", near(N=1, H=1 << 16, W=1 << 15, C=1)),
        ("non-null", near(src=None)), ("non-null", near(dst=None)), ("non-null", near(xi=None)), ("non-null", near(yi=None)),
        ("column index", near(xi=edited(xi, 3, W))), ("column index", near(xi=edited(xi, 3, -1))),
        ("row index", near(yi=edited(yi, Ho - 1, H))), ("overlap", near(src=d)),
    ]
    before = src.clone()
    for match, args in bad + bad_two:
        with pytest.raises(AdpError, match=match):
            call("adp_resample_u8", *args)
        assert match.replace("\\", "") in lib().adp_last_error().decode()
    for match, args in bad_near:
        with pytest.raises(AdpError, match=match):
            call("adp_resample_nearest_u8", *args)
    ops.set_option("resample_fused", 2)
    with pytest.raises(AdpError, match="resample_fused"):
        call("adp_resample_u8", *conv())
    ops.set_option("resample_fused", None)
    torch.cuda.synchronize()
    assert (dst == 7).all() and (tmp == 7).all() and torch.equal(src, before)
    # N = 0 returns 0 without a launch, in either form
    for form in (0, 1):
        ops.set_option("resample_fused", form)
        assert call("adp_resample_u8", *conv(N=0)) == 0
    assert call("adp_resample_nearest_u8", *near(N=0)) == 0
    torch.cuda.synchronize()
    assert (dst == 7).all() and (tmp == 7).all()
    assert R.resize(torch.zeros((0, 4, 5, 3), dtype=torch.uint8, device="cuda"), (2, 3)).shape == (0, 3, 2, 3)
    # the module refuses the same before it reaches the library
    for fn in (lambda: R.resize(src, (0, 3)), lambda: R.resize(src, (3, 3), "sinc"), lambda: R.resize(torch.zeros((1, 4, 5, 5), dtype=torch.uint8, device="cuda"), (3, 3)),
               lambda: R.resize(src, (1, 1), "lanczos")):
        with pytest.raises(ValueError):
            fn()


def test_cli_on_the_device_equals_the_numpy_path(tmp_path, capsys, monkeypatch):
    """cli/ecm_scaling.py over a tiny tree on the device and on the numpy path: the same files, byte for byte in their
    pixels, and both Pillow's."""
    from adipose_amd import components
    cli = _cli()
    ref, tgt, sizes, src = _tree(tmp_path)
    argv = ["--reference-dir", str(ref), "--target-dir", str(tgt)]
    calls = []
    real = R.resize
    monkeypatch.setattr(R, "resize", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    assert cli.main(argv + ["--output-dir", str(tmp_path / "dev")]) == 0
    assert len(calls) == 4                                                     # every resampled file went through the device
    monkeypatch.setattr(components, "_gpu", lambda: False)
    assert cli.main(argv + ["--output-dir", str(tmp_path / "host")]) == 0
    assert len(calls) == 4
    capsys.readouterr()
    check_cli_outputs(str(tmp_path / "dev"), sizes, src, "lanczos")
    check_cli_outputs(str(tmp_path / "host"), sizes, src, "lanczos")
    from PIL import Image
    for name in sorted(os.listdir(tmp_path / "host")):
        with Image.open(tmp_path / "dev" / name) as x, Image.open(tmp_path / "host" / name) as y:
            assert x.mode == y.mode and np.array_equal(np.asarray(x), np.asarray(y)), name
