"""adipose_amd.resample on the host: the numpy path against live PIL.Image.resize and against tests/golden/resample.npz
(what Pillow 12.2.0 computed: tests/golden/make_resample_golden.py), on every pixel and with no tolerance; the
coefficient tables against Python-int arithmetic; the limits; the header, the ctypes table and the exports; and
cli/ecm_scaling.py on the numpy path. The device path is held to this numpy path bit for bit in
tests/test_gpu_resample.py.
"""
import math
import os
import re

import numpy as np
import pytest
from PIL import Image

from adipose_amd import resample as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIL_FILTER = {f: getattr(Image.Resampling, f.upper()) for f in R.METHODS}


def pil_resize(a, size, f):
    return np.asarray(Image.fromarray(a).resize(size, PIL_FILTER[f]))


def image(shape, seed=0, binary=False):
    rng = np.random.default_rng([seed, *shape])
    a = rng.integers(0, 256, shape, dtype=np.uint8)
    return ((a > 127) * 255).astype(np.uint8) if binary else a


# (H, W, Ho, Wo): up, down, both mixed, 1-pixel extents on either side, one extent unchanged, far down
SHAPES_2D = [(37, 53, 40, 50), (64, 64, 147, 150), (100, 90, 37, 33), (1, 7, 3, 5), (5, 1, 1, 9), (1, 1, 4, 4),
             (33, 47, 33, 20), (33, 47, 60, 47), (200, 210, 7, 9)]


# ---------------------------------------------------------------- against live Pillow
@pytest.mark.parametrize("f", R.METHODS)
def test_equals_pillow_2d(f):
    """5 filters (and nearest) x 9 shapes x {random, 0 / 255} gray, and RGB: 90 convolution cases and 27 RGB ones."""
    for H, W, Ho, Wo in SHAPES_2D:
        for binary in (False, True):
            a = image((H, W), 1, binary)
            assert np.array_equal(R.resize_np(a, (Wo, Ho), f), pil_resize(a, (Wo, Ho), f)), (f, H, W, Ho, Wo, binary)
        a = image((H, W, 3), 2)
        assert np.array_equal(R.resize_np(a, (Wo, Ho), f), pil_resize(a, (Wo, Ho), f)), (f, H, W, Ho, Wo, "RGB")


def test_equals_pillow_1d_sweep():
    """1500 random (n, m) in 1 .. 700 on both sides, the filters in turn: one pass (no ksize limit) against Pillow."""
    rng = np.random.default_rng(7)
    filters = list(R.FILTERS)
    for i in range(1500):
        n, m = int(rng.integers(1, 701)), int(rng.integers(1, 701))
        f = filters[i % len(filters)]
        a = rng.integers(0, 256, (1, n), dtype=np.uint8)
        b, k, _ = R.coefficients(n, m, f)
        got = R.pass_np(a, b, k, 1) if n != m else a
        assert np.array_equal(got, pil_resize(a, (m, 1), f)), (f, n, m)


def test_nearest_table_equals_pillow_sweep():
    """3000 random (n, m) up to 3000: the accumulated table, and that the closed form is a different one."""
    rng = np.random.default_rng(11)
    closed_form_wrong = 0
    for _ in range(3000):
        n, m = int(rng.integers(1, 3001)), int(rng.integers(1, 3001))
        ramp = np.arange(n)
        want = pil_resize(np.stack([ramp % 256, ramp // 256]).astype(np.uint8), (m, 2), "nearest").astype(np.int64)
        t = R.nearest_table(n, m)
        assert t.dtype == np.int32 and np.array_equal(t, want[0] + 256 * want[1]), (n, m)
        closed_form_wrong += not np.array_equal(t, ((np.arange(m) + 0.5) * n / m).astype(np.int64))
    assert closed_form_wrong > 0


def test_batches_channels_and_layouts():
    a = image((3, 20, 31, 3), 5)
    out = R.resize_np(a, (25, 27), "lanczos")
    assert out.shape == (3, 27, 25, 3) and out.dtype == np.uint8
    for n in range(3):
        assert np.array_equal(out[n], pil_resize(a[n], (25, 27), "lanczos"))
        for c in range(3):                                      # every channel on its own
            assert np.array_equal(out[n, :, :, c], pil_resize(np.ascontiguousarray(a[n, :, :, c]), (25, 27), "lanczos"))
    g = image((5, 20, 31), 6)                                   # (N, H, W): the last extent is above 4
    assert np.array_equal(R.resize_np(g, (9, 8), "bicubic")[4], pil_resize(g[4], (9, 8), "bicubic"))
    thin = image((6, 9, 3), 7)                                  # (H, W, 3) by the rule, (N, H, W) when told
    assert R.resize_np(thin, (4, 5), "box").shape == (5, 4, 3)
    assert R.resize_np(thin, (4, 5), "box", channels=False).shape == (6, 5, 4)
    four = image((8, 9, 4), 8)                                  # four independent planes: Pillow's RGBX, not its RGBA
    assert np.array_equal(R.resize_np(four, (5, 6), "lanczos"),
                          np.asarray(Image.fromarray(four, "RGBX").resize((5, 6), Image.Resampling.LANCZOS)))
    assert R.resize_np(np.zeros((0, 4, 5, 3), np.uint8), (2, 3)).shape == (0, 3, 2, 3)


# ---------------------------------------------------------------- against the committed golden
def test_equals_golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "resample.npz"))
    filters = [str(f) for f in g["filters"]]
    assert filters == ["box", "bilinear", "hamming", "bicubic", "lanczos", "nearest"]
    for name in (str(c) for c in g["cases"]):
        a, (wo, ho) = g[f"{name}_in"], g[f"{name}_size"]
        for f in filters:
            assert np.array_equal(R.resize_np(a, (int(wo), int(ho)), f), g[f"{name}_{f}"]), (name, f)
    a = g["impulse_in"]
    for m in g["impulse_widths"]:
        for f in filters:
            assert np.array_equal(R.resize_np(a, (int(m), 2), f), g[f"impulse_{m}_{f}"]), (m, f)


# ---------------------------------------------------------------- the tables, by hand
def _coefficients_py(n, m, f):
    """The docstring's definition in Python floats and ints, one output at a time."""
    support0, fn = R.FILTERS[f]
    scale = n / m
    fs = max(scale, 1.0)
    support = support0 * fs
    ksize = 2 * math.ceil(support) + 1
    rows = []
    for i in range(m):
        c = (i + 0.5) * scale
        lo = max(int(c - support + 0.5), 0)
        hi = min(int(c + support + 0.5), n)
        w = [fn((j + lo - c + 0.5) * (1.0 / fs)) for j in range(hi - lo)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        rows.append((lo, hi - lo, [int(v * (1 << 22) + 0.5) if v >= 0 else int(v * (1 << 22) - 0.5) for v in w]))
    return rows, ksize


@pytest.mark.parametrize("f", R.FILTERS)
@pytest.mark.parametrize("n,m", [(8, 8), (8, 11), (11, 8), (5, 2), (2, 5), (1, 6), (6, 1), (30, 7), (7, 30)])
def test_coefficients_by_hand(f, n, m):
    b, k, ks = R.coefficients(n, m, f)
    rows, ksize = _coefficients_py(n, m, f)
    assert ks == ksize == R.ksize_of(n, m, f) == 2 * math.ceil(R.FILTERS[f][0] * max(n / m, 1.0)) + 1
    assert b.shape == (m, 2) and k.shape == (m, ks) and b.dtype == k.dtype == np.int32
    for i, (lo, cnt, taps) in enumerate(rows):
        assert (int(b[i, 0]), int(b[i, 1])) == (lo, cnt) and k[i, :cnt].tolist() == taps and not k[i, cnt:].any()
        assert 0 <= lo and 1 <= cnt <= ks and lo + cnt <= n
        assert abs(sum(taps) - (1 << 22)) <= cnt                   # each tap is rounded once: within cnt / 2 units
    assert b[0, 0] == 0 and b[-1, 0] + b[-1, 1] == n              # the bounds clamp at both ends
    assert (np.diff(b[:, 0]) >= 0).all() and (np.diff(b[:, 0] + b[:, 1]) >= 0).all()


def test_bounds_clamp_where_the_support_exceeds_the_image():
    b, k, ks = R.coefficients(3, 5, "lanczos")
    assert ks == 7 and (b[:, 0] == 0).all() and (b[:, 1] == 3).all()   # every output sees the whole row
    b, k, ks = R.coefficients(700, 3, "lanczos")
    assert ks == 2 * 700 + 1 and b[1].tolist() == [0, 700]


def test_pass_is_python_int_arithmetic():
    a = image((1, 23), 3)
    for f in R.FILTERS:
        b, k, _ = R.coefficients(23, 9, f)
        want = [min(max(((1 << 21) + sum(int(k[i, j]) * int(a[0, b[i, 0] + j]) for j in range(b[i, 1]))) >> 22, 0), 255)
                for i in range(9)]
        assert R.pass_np(a, b, k, 1)[0].tolist() == want


def test_int32_range_is_asserted():
    a = np.full((1, 4), 255, np.uint8)
    b = np.array([[0, 4]], np.int32)
    ok = np.full((1, 4), ((1 << 31) - (1 << 21) - 1) // 255 // 4, np.int32)      # 2^21 + 255 sum |k| just below 2^31
    assert R.pass_np(a, b, ok, 1)[0, 0] == 255
    with pytest.raises(OverflowError, match="int32"):
        R.pass_np(a, b, ok + 1, 1)
    with pytest.raises(OverflowError):
        R.pass_np(a, b, -(ok + 1), 1)
    for f in R.FILTERS:                                            # every table of the definition is far inside
        for n, m in ((700, 3), (64, 147), (2048, 64)):
            k = R.coefficients(n, m, f)[1].astype(np.int64)
            assert (1 << 21) + 255 * np.abs(k).sum(axis=1).max() < 1 << 31
    with pytest.raises(ValueError, match="bounds"):
        R.pass_np(a, np.array([[1, 4]], np.int32), ok, 1)


def test_a_skipped_pass_is_skipped():
    a = image((19, 40), 9)
    for f in R.FILTERS:
        b, k, _ = R.coefficients(40, 33, f)
        assert np.array_equal(R.resize_np(a, (33, 19), f), R.pass_np(a, b, k, 1))
        b, k, _ = R.coefficients(19, 26, f)
        assert np.array_equal(R.resize_np(a, (40, 26), f), R.pass_np(a, b, k, 0))
        assert np.array_equal(R.resize_np(a, (40, 19), f), a)
    # identity taps would not be a skip: bicubic at an unchanged extent still has taps, and Pillow does not run them
    assert np.array_equal(R.resize_np(a, (40, 26), "bicubic"), pil_resize(a, (40, 26), "bicubic"))


def test_value_errors():
    a = image((6, 7), 1)
    for bad in ((0, 3), (3, 0), (-1, 3), (2.5, 3), 5, (1, 2, 3)):
        with pytest.raises(ValueError):
            R.resize_np(a, bad)
    with pytest.raises(ValueError, match="unknown filter"):
        R.resize_np(a, (3, 3), "cubic")
    with pytest.raises(ValueError):
        R.resize_np(np.zeros((6, 7, 5, 5, 1), np.uint8), (3, 3))
    with pytest.raises(ValueError, match="1 .. 4 channels"):
        R.resize_np(np.zeros((2, 6, 7, 5), np.uint8), (3, 3))
    with pytest.raises(ValueError, match="at least 1 x 1"):
        R.resize_np(np.zeros((0, 7), np.uint8), (3, 3))
    with pytest.raises(TypeError):
        R.resize_np(a.astype(np.float32), (3, 3))
    with pytest.raises(TypeError):
        R.pass_np(a.astype(np.int32), *R.coefficients(7, 3, "box")[:2], 1)
    # ksize: Lanczos down to 1 / 32 is the last that passes; nearest has no taps
    assert R.ksize_of(64, 2, "lanczos") == R.KMAX == 193
    assert R.resize_np(np.zeros((1, 64), np.uint8), (2, 1), "lanczos").shape == (1, 2)
    with pytest.raises(ValueError, match="193"):
        R.resize_np(np.zeros((1, 66), np.uint8), (2, 1), "lanczos")
    with pytest.raises(ValueError, match="193"):
        R.resize_np(np.zeros((66, 1), np.uint8), (1, 2), "lanczos")
    assert R.resize_np(np.zeros((1, 660), np.uint8), (2, 1), "nearest").shape == (1, 2)
    # the size limits are checked on the shapes alone, before anything is allocated
    with pytest.raises(ValueError, match="2\\^31"):
        R._limits(1, 1 << 16, 1 << 15, 1, 8, 8, "box")
    with pytest.raises(ValueError, match="2\\^31"):
        R._limits(1, 8, 8, 4, 1 << 15, 1 << 14, "nearest")
    with pytest.raises(ValueError, match="2\\^31"):
        R._limits(1, 1 << 16, 8, 1, 8, 1 << 15, "box")           # the intermediate (H, Wo)
    with pytest.raises(ValueError, match="65535"):
        R._limits(65536, 2, 2, 1, 3, 3, "box")
    for fn in (lambda: R.Resampler((0, 4)), lambda: R.Resampler((4, 4), "sinc"), lambda: R.coefficients(0, 4, "box"),
               lambda: R.nearest_table(4, 0), lambda: R.resample_image_array(a, (3, 3), "sinc")):
        with pytest.raises(ValueError):
            fn()


def test_resampler_and_dispatch_on_host_arrays():
    a = image((12, 15, 3), 4)
    r = R.Resampler((10, 9))
    assert repr(r) == "Resampler(size=(10, 9), filter='lanczos')" and r.filter == "lanczos"
    assert repr(R.Resampler([7, 8], "nearest")) == "Resampler(size=(7, 8), filter='nearest')"
    out = r(a)
    assert isinstance(out, np.ndarray) and np.array_equal(out, pil_resize(a, (10, 9), "lanczos"))


def test_fused_fits_follows_the_footprint():
    TR, TC, L = R.TILE_ROWS, R.TILE_COLS, R.LDS_BYTES
    assert (TR, TC, L) == (32, 64, 32768)
    assert R.fused_fits(100, 100, 1, 103, 97, "lanczos") and R.fused_fits(100, 100, 4, 230, 230, "lanczos")
    assert not R.fused_fits(100, 100, 1, 100, 97, "lanczos") and not R.fused_fits(100, 100, 1, 90, 97, "nearest")
    b = R.coefficients(4000, 300, "lanczos")[0].astype(np.int64)
    rows = max(int(b[min(y + TR, 300) - 1].sum() - b[y, 0]) for y in range(0, 300, TR))
    assert R.fused_fits(4000, 70, 1, 300, 60, "lanczos") == (rows * TC <= L) and not R.fused_fits(4000, 70, 4, 300, 60, "lanczos")


# ---------------------------------------------------------------- header, ctypes table, exports
def test_header_table_and_exports_agree():
    from adipose_amd import _lib
    src = open(os.path.join(ROOT, "include", "adipose_hip.h")).read()
    for name, val in (("KMAX", R.KMAX), ("TILE_ROWS", R.TILE_ROWS), ("TILE_COLS", R.TILE_COLS), ("LDS_BYTES", R.LDS_BYTES)):
        assert int(re.search(rf"#define ADP_RESAMPLE_{name} (\d+)", src).group(1)) == val
    assert re.search(r"#define ADP_ABI_VERSION 21 ", src)
    version_comment = src[src.index("#define ADP_ABI_VERSION"):src.index("typedef void* adp_stream_t")]
    lib = _lib.lib()
    for name, nargs in (("adp_resample_u8", 16), ("adp_resample_nearest_u8", 11)):
        assert name in version_comment and hasattr(lib, name) and len(_lib._SIGS[name]) == nargs
        decl = re.search(rf"int {name}\((.*?)\);", re.sub(r"/\*.*?\*/", "", src, flags=re.S), re.S).group(1)
        assert decl.count(",") + 1 == nargs
    assert "resample.hip" in open(os.path.join(ROOT, "adipose_tissue-unet_amd", "csrc", "Makefile")).read()


# ---------------------------------------------------------------- the script's helpers and the CLI
def _cli():
    import importlib.util
    spec = importlib.util.spec_from_file_location("ecm_scaling", os.path.join(ROOT, "cli", "ecm_scaling.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_flags_and_defaults():
    cli = _cli()
    args = cli.parse_args(["--reference-dir", "r", "--target-dir", "t"])
    assert (args.reference_dir, args.target_dir, args.output_dir, args.dry_run, args.interpolation) == ("r", "t", None, False, "lanczos")
    args = cli.parse_args(["--reference-dir", "r", "--target-dir", "t", "--output-dir", "o", "--dry-run", "--interpolation", "nearest"])
    assert (args.output_dir, args.dry_run, args.interpolation) == ("o", True, "nearest")
    for f in ("lanczos", "bilinear", "bicubic", "nearest"):
        assert cli.parse_args(["--reference-dir", "r", "--target-dir", "t", "--interpolation", f]).interpolation == f
    for bad in (["--target-dir", "t"], ["--reference-dir", "r"], ["--reference-dir", "r", "--target-dir", "t", "--interpolation", "box"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)


def _tree(tmp_path):
    """reference/ and target/: a PNG and a TIFF to resample, a -002 stem, an unmatched stem, an image already at size,
    a 16-bit TIFF and a file that is no image."""
    ref, tgt = tmp_path / "reference", tmp_path / "target"
    ref.mkdir()
    tgt.mkdir()
    sizes = {"slideA": (50, 45), "slideB": (41, 47), "slideC": (30, 20), "slideD": (33, 31), "slideE": (28, 36)}
    for stem, (w, h) in sizes.items():
        Image.fromarray(image((h, w, 3), 1)).save(ref / f"{stem}.png")
    src = {"slideA.png": image((48, 53, 3), 2), "slideB.tif": image((44, 43), 3), "slideC-002.png": image((23, 27), 4),
           "stray.png": image((10, 10), 5), "slideD.png": image((31, 33), 6)}
    for name, a in src.items():
        Image.fromarray(a).save(tgt / name)
    deep = (np.random.default_rng(8).integers(300, 40000, (40, 30))).astype(np.uint16)
    Image.fromarray(deep).save(tgt / "slideE.tif")
    src["slideE.tif"] = deep
    (tgt / "notes.txt").write_text("not an image")
    (ref / "broken.png").write_bytes(b"not a png")
    return ref, tgt, sizes, src


def test_cli_dry_run(tmp_path, capsys):
    cli = _cli()
    ref, tgt, sizes, _ = _tree(tmp_path)
    assert cli.main(["--reference-dir", str(ref), "--target-dir", str(tgt), "--dry-run"]) == 0
    out = capsys.readouterr().out
    assert not (tgt / "resampled").exists()
    assert "Failed to read broken.png" in out and "Found 5 reference images" in out
    assert "slideC-002:" in out and "Target:  30×20" in out and "Delta:   -3×+3" in out          # the -ddd strip
    assert "No reference match for: stray" in out
    assert "slideD: Already correct size 33×31" in out
    assert out.count("[DRY RUN] Would save to") == 4
    assert "Matched targets:      5" in out and "Successfully processed: 5" in out and "Skipped (no match):   1" in out
    assert "DRY RUN - No files were written" in out
    assert cli.main(["--reference-dir", str(tmp_path / "none"), "--target-dir", str(tgt)]) == 1
    assert cli.main(["--reference-dir", str(ref), "--target-dir", str(tmp_path / "none")]) == 1
    (tmp_path / "empty").mkdir()
    assert cli.main(["--reference-dir", str(tmp_path / "empty"), "--target-dir", str(tgt), "--dry-run"]) == 1


def check_cli_outputs(outdir, sizes, src, f):
    """The files a run of the CLI wrote, against Pillow's resize of the inputs."""
    assert sorted(os.listdir(outdir)) == ["slideA.png", "slideB.tif", "slideC-002.png", "slideE.tif"]
    for name, stem in (("slideA.png", "slideA"), ("slideB.tif", "slideB"), ("slideC-002.png", "slideC")):
        with Image.open(os.path.join(outdir, name)) as im:
            assert im.size == sizes[stem] and im.format == ("TIFF" if name.endswith(".tif") else "PNG")
            assert np.array_equal(np.asarray(im), pil_resize(src[name], sizes[stem], f)), name
            if name.endswith(".tif"):
                assert im.info.get("compression") == "tiff_adobe_deflate"
    with Image.open(os.path.join(outdir, "slideE.tif")) as im:
        assert im.mode == "L" and np.array_equal(np.asarray(im), pil_resize(R.to_uint8_minmax(src["slideE.tif"]), sizes["slideE"], f))


@pytest.mark.parametrize("f", ["lanczos", "nearest"])
def test_cli_real_run_on_the_numpy_path(tmp_path, capsys, monkeypatch, f):
    from adipose_amd import components
    monkeypatch.setattr(components, "_gpu", lambda: False)        # the numpy path, whatever the host has
    cli = _cli()
    ref, tgt, sizes, src = _tree(tmp_path)
    out_dir = tmp_path / "out"
    argv = ["--reference-dir", str(ref), "--target-dir", str(tgt), "--output-dir", str(out_dir)]
    assert cli.main(argv + ([] if f == "lanczos" else ["--interpolation", f])) == 0
    out = capsys.readouterr().out
    check_cli_outputs(str(out_dir), sizes, src, f)
    assert "Successfully processed: 5" in out and f"Output saved to: {out_dir}" in out
    # one failing image is reported and the run goes on
    (tgt / "slideA.png").write_bytes(b"broken")
    assert cli.main(["--reference-dir", str(ref), "--target-dir", str(tgt)]) == 0
    out = capsys.readouterr().out
    assert "Failed to process slideA" in out and "Successfully processed: 4" in out
    assert sorted(os.listdir(tgt / "resampled")) == ["slideB.tif", "slideC-002.png", "slideE.tif"]   # the default --output-dir


def test_sixteen_bit_conversion_is_the_formula():
    a = np.random.default_rng(2).integers(0, 65536, (9, 11)).astype(np.uint16)
    lo, hi = a.min(), a.max()
    want = ((a.astype(np.float32) - lo) / (hi - lo) * 255).astype(np.uint8)     # the reference's expression
    got = R.to_uint8_minmax(a)
    assert got.dtype == np.uint8 and np.array_equal(got, want) and got.min() == 0 and got.max() == 255
    assert not R.to_uint8_minmax(np.full((3, 3), 777, np.uint16)).any()
    s = (a.astype(np.int32) // 4).astype(np.int16)
    assert np.array_equal(R.to_uint8_minmax(s), ((s.astype(np.float32) - s.min()) / np.float32(int(s.max()) - int(s.min())) * 255).astype(np.uint8))


def test_host_helpers(tmp_path):
    ref, tgt, sizes, src = _tree(tmp_path)
    log = []
    got = R.build_reference_dict(str(ref), log.append)
    assert got == sizes and any("broken.png" in line for line in log)
    assert R.get_image_size(str(tgt / "slideB.tif")) == (43, 44)
    assert R.match_reference("slideC-002", sizes) == "slideC" and R.match_reference("slideC-02", sizes) is None
    assert R.match_reference("slideA", sizes) == "slideA" and R.match_reference("stray", sizes) is None
    # RGBA goes to Pillow on the host, and says so
    rgba = image((12, 14, 4), 3)
    Image.fromarray(rgba, "RGBA").save(tmp_path / "a.png")
    R.resample_image(str(tmp_path / "a.png"), (9, 10), str(tmp_path / "b.png"), "bicubic", log.append)
    assert any("RGBA" in line and "Pillow on the host" in line for line in log)
    with Image.open(tmp_path / "b.png") as im:
        assert np.array_equal(np.asarray(im), np.asarray(Image.fromarray(rgba, "RGBA").resize((9, 10), Image.Resampling.BICUBIC)))
    # JPEG keeps its format and settings
    Image.fromarray(image((20, 22, 3), 4)).save(tmp_path / "c.jpg", quality=95)
    R.resample_image(str(tmp_path / "c.jpg"), (11, 13), str(tmp_path / "d.jpg"), "bilinear")
    with Image.open(tmp_path / "d.jpg") as im:
        assert im.format == "JPEG" and im.size == (11, 13)
