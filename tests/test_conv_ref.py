"""oracle/conv_ref.py (the float64 reference tests/test_gpu_conv_exact.py compares the convolution kernels with)
against independent formulations: torch.nn.functional.conv2d / conv_transpose2d and torch.autograd in float64,
to 1e-12 relative (the bound of tests/test_ew_ref.py). Then the two comparison helpers are shown to bite: each
defect the max-norm gate of the older tests lets through is applied to the reference's own output and must be
rejected by assert_exact / assert_sum_gate while `relerr < 2e-2` accepts it. Last, every kernel family the
launchers can name owns a row of the GPU file's case table. Runs on any machine."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import conv_ref as CR
from oracle import ew_ref as E

F64 = torch.float64
TOL = 1e-12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16


def close(a, b):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    assert a.shape == b.shape, (a.shape, b.shape)
    err, ref = (a - b).abs().max().item(), max(b.abs().max().item(), 1e-300)
    assert err <= TOL * ref, f"{err:.3e} against {ref:.3e}"


def gen(seed):
    return torch.Generator().manual_seed(seed)


def nchw(x):
    return x.permute(0, 3, 1, 2)


def nhwc(x):
    return x.permute(0, 2, 3, 1)


def torch_conv(xs, W, nout, kh, kw, dil, pad, up, stride=1):
    """F.conv2d of the concatenated (and upsampled) sources with the packed weights W[n][tap*C + c]."""
    x = torch.cat(xs, -1)
    if up:
        x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    C = x.shape[-1]
    wk = W[:nout, :kh * kw * C].reshape(nout, kh, kw, C).permute(0, 3, 1, 2)
    return nhwc(F.conv2d(nchw(x), wk, padding=pad, dilation=dil, stride=stride))


GEOM = [
    # id, (N, H, W), parts, nout, kh, dil, up
    ("3x3", (2, 7, 9), [8], 16, 3, 1, False),
    ("dil2", (1, 9, 6), [16], 8, 3, 2, False),
    ("dil8", (1, 20, 17), [8], 8, 3, 8, False),
    ("dil32", (1, 40, 36), [8], 8, 3, 32, False),
    ("dil_past_image", (2, 6, 5), [8], 16, 3, 32, False),
    ("up", (2, 4, 5), [8], 8, 3, 1, True),
    ("up_dil2", (1, 5, 4), [8], 8, 3, 2, True),
    ("concat", (2, 6, 6), [8, 16], 24, 3, 1, False),
    ("1x1", (2, 5, 7), [24], 8, 1, 1, False),
    ("1x1_concat", (1, 5, 7), [8, 8], 8, 1, 1, False),
]


@pytest.mark.parametrize("case", GEOM, ids=[c[0] for c in GEOM])
def test_forward_and_gradients_match_autograd(case):
    """Gather + GEMM, the data gradient from the master weights and the weight / bias gradient against
    autograd through F.conv2d."""
    _, (N, H, W_), parts, nout, k, dil, up = case
    g = gen(len(parts) * 100 + dil)
    xs = [torch.randn(N, H, W_, c, generator=g, dtype=F64).requires_grad_(True) for c in parts]
    C = sum(parts)
    Wt = torch.randn(nout + 3, k * k * C + 5, generator=g, dtype=F64).requires_grad_(True)   # pad rows / columns ignored
    bias = torch.randn(nout, generator=g, dtype=F64).requires_grad_(True)
    pad = dil * (k // 2)
    y = torch_conv(xs, Wt, nout, k, k, dil, pad, up) + bias
    dY = torch.randn(y.shape, generator=g, dtype=F64)
    (y * dY).sum().backward()
    r = CR.conv_fwd([x.detach() for x in xs], Wt.detach(), nout, bias=bias.detach(), kh=k, kw=k, dil=dil, up=up)
    close(r["out"], y.detach())
    assert bool((r["A_out"] + 1e-9 >= r["v"].abs()).all())
    wg = CR.conv_wgrad([x.detach() for x in xs], dY, nout, kh=k, kw=k, dil=dil, up=up)
    close(wg["dW"], Wt.grad[:nout, :k * k * C])
    close(wg["dB"], bias.grad)
    assert float(Wt.grad[nout:].abs().max()) == 0.0 and float(Wt.grad[:, k * k * C:].abs().max()) == 0.0
    # data gradient on the virtual (upsampled) grid; its 2x2 block sums are the gradient of the sources
    Hv, Wv = (2 * H, 2 * W_) if up else (H, W_)
    dX, A = CR.conv_dgrad(dY, Wt.detach(), nout, C, Hs=Hv, Ws=Wv, kh=k, kw=k, dil=dil)
    if up:
        dX = E.upsample2_bwd(dX)
    close(dX, torch.cat([x.grad for x in xs], -1))
    assert A.shape[:3] == (N, Hv, Wv)


def test_data_gradient_equals_forward_on_packed_weights():
    """The documented repack (adp_pack_weights mode 1: dst[ci][t*Nout + co] = src[co][(taps-1-t)*Cin_s + ci])
    followed by a forward launch over dY is the same float64 transpose."""
    g = gen(5)
    N, H, W_, C, nout = 2, 6, 7, 8, 16
    for dil in (1, 2, 8):
        dY = torch.randn(N, H, W_, nout, generator=g, dtype=F64)
        Wm = torch.randn(nout, 9 * C, generator=g, dtype=F64)
        Wd = Wm.reshape(nout, 9, C).flip(1).permute(2, 1, 0).reshape(C, 9 * nout)
        close(CR.conv_fwd([dY], Wd, C, dil=dil)["out"], CR.conv_dgrad(dY, Wm, nout, C, Hs=H, Ws=W_, dil=dil)[0])


def test_conv_transpose_matches_autograd():
    """Pixel-shuffle forward, the stride-2 four-tap data gradient and the weight gradient over the shuffled dY."""
    g = gen(7)
    N, H, W_, cin, cps = 2, 3, 5, 8, 16
    x = torch.randn(N, H, W_, cin, generator=g, dtype=F64).requires_grad_(True)
    k = torch.randn(cin, cps, 2, 2, generator=g, dtype=F64).requires_grad_(True)
    b = torch.randn(cps, generator=g, dtype=F64).requires_grad_(True)
    y = nhwc(F.conv_transpose2d(nchw(x), k, b, stride=2))
    dY = torch.randn(y.shape, generator=g, dtype=F64)
    (y * dY).sum().backward()
    Wm = k.detach().permute(2, 3, 1, 0).reshape(4 * cps, cin)      # [sub*cps + c][ci], sub = 2*dy + dx
    r = CR.convt_fwd(x.detach(), Wm, cps, bias=b.detach(), bn_stats=True)
    close(r["out"], y.detach())
    close(r["stats"][0], y.detach().reshape(-1, cps).sum(0))
    close(r["stats"][1], (y.detach() ** 2).reshape(-1, cps).sum(0))
    close(CR.convt_dgrad(dY, Wm, cps, cin)[0], x.grad)
    # the same through the documented device path: transpose, then the 2x2 / stride-2 gather over dY
    close(CR.conv_fwd([dY], Wm.T.contiguous(), cin, kh=2, kw=2, stride=2, pad=0, Ho=H, Wo=W_)["out"], x.grad)
    wg = CR.conv_wgrad([x.detach()], dY, 4 * cps, kh=1, kw=1, pad=0, shuffle_c=cps)
    close(wg["dW"], k.grad.permute(2, 3, 1, 0).reshape(4 * cps, cin))
    close(wg["dB"], b.grad)


def test_epilogue_switches():
    """bias -> relu -> dropout -> addend -> mask -> store, split store with mask2, accum, statistics before the
    rounding, the BatchNorm-backward sums of the stored value, BatchNorm on load: each against a direct torch
    formulation built on F.conv2d."""
    g = gen(11)
    N, H, W_, C, nout = 2, 5, 6, 8, 16
    x = torch.randn(N, H, W_, C, generator=g, dtype=F64).to(BF16).to(F64)
    Wt = (torch.randn(nout, 9 * C, generator=g, dtype=F64) * 0.2).to(BF16).to(F64)
    bias = torch.randn(nout, generator=g, dtype=F64).float().to(F64)
    add = torch.randn(N, H, W_, nout, generator=g, dtype=F64).to(BF16).to(F64)
    mask = torch.randn(N, H, W_, nout, generator=g, dtype=F64)
    acc0 = torch.randn(N, H, W_, nout, generator=g, dtype=F64).float().to(F64)
    base = torch_conv([x], Wt, nout, 3, 3, 1, 1, False) + bias
    M = N * H * W_
    # relu + dropout (keep factor 2)
    r = CR.conv_fwd([x], Wt, nout, bias=bias, relu=True, dropout_rate=0.5, dropout_seed=1234, round_to=BF16)
    u = CR.adp_uniform(1234, np.arange(M * nout, dtype=np.uint64)).reshape(N, H, W_, nout)
    keep = torch.from_numpy(u >= 0.5)
    assert torch.equal(r["keep"], keep) and 0.4 < keep.double().mean().item() < 0.6
    want = torch.where(keep, 2.0 * base.clamp(min=0), torch.zeros((), dtype=F64))
    close(r["v"], want)
    assert torch.equal(r["out"], want.float().to(BF16).to(F64))
    # addend, mask, accum, statistics of the unrounded value
    r = CR.conv_fwd([x], Wt, nout, bias=bias, addend=add, mask=mask, mask_scale=0.5, accum=acc0, bn_stats=True,
                    round_to=BF16)
    v = torch.where(mask > 0, (base + add) * 0.5, torch.zeros((), dtype=F64))
    close(r["v"], v)
    close(r["accum"], acc0 + r["out"])
    close(r["stats"][0], v.reshape(M, nout).sum(0))
    close(r["stats"][1], (v * v).reshape(M, nout).sum(0))
    close(r["A_stats"][0], v.abs().reshape(M, nout).sum(0))
    # split store: addend / mask on the first part, mask2 on the second
    m2 = torch.randn(N, H, W_, 8, generator=g, dtype=F64)
    r = CR.conv_fwd([x], Wt, nout, out_mode=2, split_c=8, mask=mask[..., :8], mask_scale=2.0, mask2=m2,
                    mask2_scale=0.5, bn_stats=True)
    nb = base - bias
    close(r["out"], torch.where(mask[..., :8] > 0, nb[..., :8] * 2.0, torch.zeros((), dtype=F64)))
    close(r["out2"], torch.where(m2 > 0, nb[..., 8:] * 0.5, torch.zeros((), dtype=F64)))
    close(r["stats"][0], torch.cat([r["out"], r["out2"]], -1).reshape(M, nout).sum(0))
    # fused BatchNorm-backward reduction over the STORED gradient
    z = torch.randn(N, H, W_, nout, generator=g, dtype=F64).to(BF16).to(F64)
    sc, sh, mu, ist = (torch.randn(nout, generator=g, dtype=F64) for _ in range(4))
    r = CR.conv_fwd([x], Wt, nout, bn_reduce=(z, sc, sh, mu, ist), round_to=BF16)
    dg, db = E.bn_bwd_reduce(nb.float().to(BF16).to(F64), z, sc, sh, mu, ist)
    close(r["bnr"][0], dg)
    close(r["bnr"][1], db)
    assert bool((r["A_bnr"][0] + 1e-9 >= dg.abs()).all()) and bool((r["A_bnr"][1] + 1e-9 >= db.abs()).all())
    # BatchNorm on load: the rounded activation is what the conv multiplies, and what act_out receives
    scA, shA = torch.randn(C, generator=g, dtype=F64), torch.randn(C, generator=g, dtype=F64)
    act = (x * scA + shA).clamp(min=0).float().to(BF16).to(F64)
    r = CR.conv_fwd([x], Wt, nout, bn_load=[(scA, shA)], round_to=BF16)
    close(r["act"][0], act)
    close(r["v"], torch_conv([act], Wt, nout, 3, 3, 1, 1, False))


def test_weight_gradient_with_bn_apply():
    """dz = rt(bn_bwd_apply(...)) is returned and is the dY of the sums."""
    g = gen(13)
    N, H, W_, C, nout = 2, 4, 4, 8, 8
    x = torch.randn(N, H, W_, C, generator=g, dtype=F64)
    dA, z = (torch.randn(N, H, W_, nout, generator=g, dtype=F64).to(BF16).to(F64) for _ in range(2))
    vec = [torch.randn(nout, generator=g, dtype=F64) for _ in range(7)]
    r = CR.conv_wgrad([x], None, nout, bn_apply=(dA, z, *vec, float(N * H * W_)), round_to=BF16)
    dz = E.bn_bwd_apply(dA, z, *vec, float(N * H * W_)).float().to(BF16).to(F64)
    assert torch.equal(r["dz"], dz)
    plain = CR.conv_wgrad([x], dz, nout)
    close(r["dW"], plain["dW"])
    close(r["dB"], plain["dB"])


# --------------------------------------------------------------------- the comparisons bite
def relerr(a, b):
    """The criterion of tests/test_gpu_ops.py: the largest error over the largest element."""
    a, b = a.float(), b.float()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-6)


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


@pytest.fixture(scope="module")
def exact_case():
    """The M = 529 shape of test_tap64_configs (1, 23, 23, [128] -> 192) on wide-regime integers, with relu +
    dropout, and its weight gradient; narrow-regime statistics."""
    g = gen(17)
    x = _ints(g, (1, 23, 23, 128), -8, 8)
    Wt = _ints(g, (192, 9 * 128), -4, 4)
    bias = _ints(g, (192,), -8, 8)
    fw = CR.conv_fwd([x], Wt, 192, bias=bias, relu=True, dropout_rate=0.5, dropout_seed=99, round_to=BF16)
    assert CR.exact(fw["A_out"])
    dY = _ints(g, (1, 23, 23, 192), -8, 8)
    wg = CR.conv_wgrad([x], dY, 192)
    assert CR.exact(wg["A_dW"], wg["A_dB"])
    xn = _ints(g, (1, 23, 23, 128), -2, 2)
    Wn = _ints(g, (192, 9 * 128), -1, 1) * (torch.rand(192, 9 * 128, generator=g) < 0.25)
    st = CR.conv_fwd([xn], Wn, 192, bias=bias, relu=True, bn_stats=True, round_to=BF16)
    assert CR.exact(st["A_out"], *st["A_stats"])
    return dict(x=x, W=Wt, bias=bias, fw=fw, dY=dY, wg=wg, xn=xn, Wn=Wn, st=st)


def _rejected(fn):
    with pytest.raises(AssertionError):
        fn()


def test_mutation_pixel_left_out_of_statistics(exact_case):
    st = exact_case["st"]
    s, q = st["stats"]
    v = st["v"].reshape(-1, 192)
    pix = int(v.abs().sum(1).argmax())
    s_bad, q_bad = s - v[pix], q - v[pix] ** 2
    assert relerr(s_bad, s) < 2e-2 and relerr(q_bad, q) < 2e-2
    _rejected(lambda: CR.assert_exact(s_bad.float(), s, "sum"))
    _rejected(lambda: CR.assert_exact(q_bad.float(), q, "sqsum"))
    # on the derived gate too: one pixel is far outside an f32 chain of 529 additions
    _rejected(lambda: CR.assert_sum_gate(s_bad, s, st["A_stats"][0], 529, "sum"))
    _rejected(lambda: CR.assert_sum_gate(q_bad, q, st["A_stats"][1], 529, "sqsum"))
    assert CR.assert_sum_gate(s.float(), s, st["A_stats"][0], 529) <= 1.0


def test_mutation_truncating_store(exact_case):
    fw = exact_case["fw"]
    v32 = fw["v"].float()
    trunc = (v32.view(torch.int32) & -65536).view(torch.float32).to(F64)      # drop the low 16 bits: round toward 0
    assert not torch.equal(trunc, fw["out"])
    assert relerr(trunc, fw["out"]) < 2e-2
    _rejected(lambda: CR.assert_exact(trunc.to(BF16), fw["out"], "out"))
    CR.assert_exact(v32.to(BF16), fw["out"], "out")


def test_mutation_k_element_zeroed(exact_case):
    c = exact_case
    Wb = c["W"].clone()
    Wb[:, 5 * 128 + 77] = 0.0
    bad = CR.conv_fwd([c["x"]], Wb, 192, bias=c["bias"], relu=True, dropout_rate=0.5, dropout_seed=99, round_to=BF16)
    assert relerr(bad["out"], c["fw"]["out"]) < 2e-2
    _rejected(lambda: CR.assert_exact(bad["out"].to(BF16), c["fw"]["out"], "out"))


def test_mutation_pixel_left_out_of_weight_gradient(exact_case):
    """At M = 529 the max-norm gate still sees a dropped pixel (one product of 64 against a largest entry of
    about 2 500); the margin shrinks with sqrt(M), and at the M = 2 048 of the persistent weight-gradient shapes
    the same defect passes it."""
    c = exact_case
    dYb = c["dY"].clone()
    dYb[0, 11, 7] = 0.0
    bad = CR.conv_wgrad([c["x"]], dYb, 192)
    _rejected(lambda: CR.assert_exact(bad["dW"].float(), c["wg"]["dW"], "dW"))
    g = gen(19)
    x, dY = _ints(g, (2, 32, 32, 64), -8, 8), _ints(g, (2, 32, 32, 64), -8, 8)
    ref = CR.conv_wgrad([x], dY, 64)
    assert CR.exact(ref["A_dW"], ref["A_dB"])
    dYb = dY.clone()
    dYb[1, 11, 7] = 0.0
    bad = CR.conv_wgrad([x], dYb, 64)
    assert relerr(bad["dW"], ref["dW"]) < 2e-2
    _rejected(lambda: CR.assert_exact(bad["dW"].float(), ref["dW"], "dW"))
    _rejected(lambda: CR.assert_exact(bad["dB"].float(), ref["dB"], "dB"))
    _rejected(lambda: CR.assert_sum_gate(bad["dW"], ref["dW"], ref["A_dW"], 2048, "dW"))


def test_mutation_dropout_decision_flipped(exact_case):
    fw = exact_case["fw"]
    v = fw["v"].reshape(-1)
    kept = torch.nonzero(fw["keep"].reshape(-1) & (v > 0) & (v < 0.015 * v.max()))
    bad = fw["out"].clone().reshape(-1)
    bad[int(kept[0])] = 0.0
    bad = bad.reshape(fw["out"].shape)
    assert relerr(bad, fw["out"]) < 2e-2
    _rejected(lambda: CR.assert_exact(bad.to(BF16), fw["out"], "out"))
    _rejected(lambda: CR.assert_exact((bad != 0), (fw["out"] != 0), "kept set"))


def test_mutation_guard_column_written(exact_case):
    fw = exact_case["fw"]
    out = fw["out"].to(BF16)
    buf = torch.full((1, 23, 23, 200), -7.0, dtype=BF16)
    buf[..., :192] = out
    CR.assert_exact(buf[..., :192], fw["out"], "out", sentinel=-7.0, guard=buf[..., 192:])
    zeroed = torch.zeros(1, 23, 23, 200, dtype=BF16)        # what the older tests start from: a stray zero is unseen
    zeroed[..., :192] = out
    assert zeroed[..., 192:].abs().max().item() == 0.0
    buf[0, 3, 4, 193] = 0.0
    _rejected(lambda: CR.assert_exact(buf[..., :192], fw["out"], "out", sentinel=-7.0, guard=buf[..., 192:]))


def test_sum_gate_value():
    assert float(CR.sum_gate(56, torch.tensor(1.0))) == 64 * 2.0 ** -24
    _rejected(lambda: CR.assert_sum_gate(torch.tensor([1.0]), torch.tensor([0.0]), torch.tensor([0.0]), 4))


# -------------------------------------------------------------------------------- completeness
def kernel_families():
    """The family names of the set_kernel("<name>...") calls of csrc/*.hip: the kernel name up to its template
    arguments, without the igemm_ prefix and the _kernel suffix."""
    csrc = os.path.join(ROOT, "adipose_tissue-unet_amd", "csrc")
    fams = set()
    for fn in sorted(os.listdir(csrc)):
        if fn.endswith(".hip"):
            with open(os.path.join(csrc, fn)) as f:
                for m in re.finditer(r'set_kernel\("([A-Za-z0-9_]+)', f.read()):
                    fams.add(re.sub(r"_kernel$", "", re.sub(r"^igemm_", "", m.group(1))))
    return fams


def gpu_module():
    spec = importlib.util.spec_from_file_location("gpu_conv_exact_table",
                                                  os.path.join(ROOT, "tests", "test_gpu_conv_exact.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# kernels whose name is not "igemm_<family>_kernel" / "<family>_kernel": the generic kernels, named by a
# conditional expression in the launcher (the pattern above does not see them, so they are no required family)
KERNEL_ALIASES = {"fwd_generic": "igemm_fwd_kernel", "wgrad_generic": "igemm_wgrad_kernel"}


def row_families(c):
    """{family: expected kernel prefix} of a row, per dtype where the row says so."""
    out = {}
    for dtn in c["dts"]:
        fam = c["family"][dtn] if isinstance(c["family"], dict) else c["family"]
        out[fam] = c["kernel"][dtn] if isinstance(c["kernel"], dict) else c["kernel"]
    return out


def kernel_of_family(fam):
    return KERNEL_ALIASES.get(fam, ("" if fam == "wgrad_in1_f32" else "igemm_") + fam + "_kernel")


def test_every_kernel_family_has_an_exact_case():
    fams = kernel_families()
    assert len(fams) >= 19 and {"fwd_tap64p", "fwd_halop", "wgrad_halopair", "wgrad_in1_f32"} <= fams, fams
    mod = gpu_module()
    covered = set()
    for c in mod.CASES:
        for fam, kernel in row_families(c).items():
            # the label is tied to the kernel the row asserts: a mislabelled row cannot cover a family
            want = kernel_of_family(fam)
            assert kernel.startswith(want) and kernel[len(want):len(want) + 1] in ("", "<"), (c["id"], fam, kernel)
            covered.add(fam)
    for c in mod.GATE_CASES + mod.BNR_GATE_CASES:
        assert c["kernel"].startswith(kernel_of_family(c["family"]) + "<"), (c["id"], c["kernel"])
    excluded = set(mod.EXCLUDED)
    assert all(len(reason) > 20 for reason in mod.EXCLUDED.values())
    assert len(excluded) <= 3, "the exclusion list stays short"
    assert not (covered & excluded)
    assert not fams - covered - excluded, sorted(fams - covered - excluded)
    assert excluded <= fams, sorted(excluded - fams)
    # a row may cover a kernel the pattern does not see (a name chosen by a conditional expression): the generic
    # kernels of KERNEL_ALIASES and igemm_wgrad_halo_f32_kernel
    assert covered - fams <= set(KERNEL_ALIASES) | {"wgrad_halo_f32"}, sorted(covered - fams)


def test_case_table_is_mostly_exact():
    """At most one case in ten on a derived gate, every case names its kernel, ids are unique."""
    mod = gpu_module()
    ids = [c["id"] for c in mod.CASES]
    assert len(set(ids)) == len(ids)
    gated = mod.GATE_CASES + mod.BNR_GATE_CASES
    assert all("gate" in c["id"] and not c["exact"] for c in gated) and not any("gate" in i for i in ids)
    assert 10 * len(gated) <= len(mod.CASES) + len(gated)
    assert all(c["kernel"] for c in mod.CASES + gated)
