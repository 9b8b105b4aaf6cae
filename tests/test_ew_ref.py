"""oracle/ew_ref.py (the float64 reference the GPU elementwise tests compare with) against independent
formulations: torch.autograd through oracle/torch_ref.py in float64. Agreement to 1e-12 relative is what
makes the GPU comparison in tests/test_gpu_elementwise.py meaningful; runs on any machine."""
import numpy as np
import pytest
import torch

from oracle import ew_ref as E
from oracle import torch_ref as R

F64 = torch.float64
TOL = 1e-12


def close(a, b):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    assert a.shape == b.shape
    err, ref = (a - b).abs().max().item(), max(b.abs().max().item(), 1e-300)
    assert err <= TOL * ref, f"{err:.3e} against {ref:.3e}"


def gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("shape", [(1, 1, 3, 8), (2, 5, 7, 24), (3, 4, 6, 40)])
def test_batchnorm_chain_matches_autograd(shape):
    """finalize -> apply -> reduce -> bwd-apply == autograd through bn_relu_train (training statistics)."""
    g = gen(shape[-1])
    C, M = shape[-1], shape[0] * shape[1] * shape[2]
    z = (torch.randn(shape, generator=g, dtype=F64) * 2 + torch.randn(C, generator=g, dtype=F64)).requires_grad_(True)
    gamma = (torch.rand(C, generator=g, dtype=F64) + 0.5).requires_grad_(True)
    beta = (torch.randn(C, generator=g, dtype=F64) * 0.3).requires_grad_(True)
    dA = torch.randn(shape, generator=g, dtype=F64)
    eps = 1e-3
    y = R.bn_relu_train(z, gamma, beta, eps=eps)
    (y * dA).sum().backward()
    zd = z.detach()
    f = E.bn_finalize(zd.reshape(-1, C).sum(0), (zd * zd).reshape(-1, C).sum(0), M, gamma, beta, eps)
    close(f["mean"], zd.mean((0, 1, 2)))
    close(f["var"], zd.var((0, 1, 2), unbiased=False))
    close(E.bn_apply(zd, f["scale"], f["shift"]), y.detach())
    dg, db = E.bn_bwd_reduce(dA, zd, f["scale"], f["shift"], f["mean"], f["invstd"])
    close(dg, gamma.grad)
    close(db, beta.grad)
    close(E.bn_bwd_apply(dA, zd, f["scale"], f["shift"], f["mean"], f["invstd"], gamma, dg, db, M), z.grad)


def test_batchnorm_finalize_forms():
    """Eval form (count < 0), running statistics with the unbiased variance, count == 1."""
    g = gen(3)
    C, n = 5, 37
    x = torch.randn(n, C, generator=g, dtype=F64) * 3 + 1
    gamma, beta = torch.rand(C, generator=g, dtype=F64) + 0.5, torch.randn(C, generator=g, dtype=F64)
    rm, rv = torch.randn(C, generator=g, dtype=F64), torch.rand(C, generator=g, dtype=F64) + 0.5
    f = E.bn_finalize(x.sum(0), (x * x).sum(0), n, gamma, beta, 1e-5, 0.1, rm, rv)
    close(f["rmean"], 0.9 * rm + 0.1 * x.mean(0))
    close(f["rvar"], 0.9 * rv + 0.1 * x.var(0, unbiased=True))
    close(f["invstd"], 1 / torch.sqrt(x.var(0, unbiased=False) + 1e-5))
    e = E.bn_finalize(rm, rv, -1, gamma, beta, 1e-5, 0.1, rm, rv)
    assert "rmean" not in e
    close(e["scale"], gamma / torch.sqrt(rv + 1e-5))
    close(e["shift"], beta - rm * gamma / torch.sqrt(rv + 1e-5))
    one = E.bn_finalize(x[0], x[0] * x[0], 1, gamma, beta, 1e-5, 1.0, rm, rv)
    close(one["rmean"], x[0])
    assert one["var"].abs().max().item() < 1e-12 and one["rvar"].abs().max().item() < 1e-12   # no n/(n-1) at n = 1


@pytest.mark.parametrize("shape", [(1, 2, 2, 8), (2, 6, 10, 16), (3, 14, 2, 8)])
def test_pool_and_upsample_backward_match_autograd(shape):
    g = gen(sum(shape))
    N, H, W, C = shape
    v = torch.randn(shape, generator=g, dtype=F64).requires_grad_(True)   # continuous: no ties
    dpool = torch.randn(N, H // 2, W // 2, C, generator=g, dtype=F64)
    add = torch.randn(shape, generator=g, dtype=F64)
    mask = torch.randn(shape, generator=g, dtype=F64)
    pooled = R.maxpool2(v)
    close(E.maxpool2_fwd(v), pooled.detach())
    (pooled * dpool).sum().backward()
    close(E.maxpool2_bwd(v, dpool), v.grad)
    close(E.maxpool2_bwd(v, dpool, addend=add, mask=mask, mask_scale=1.5),
          torch.where(mask > 0, (v.grad + add) * 1.5, torch.zeros((), dtype=F64)))
    # BatchNorm on load: the argmax over relu(src*sc + sh); scale > 0 keeps strict order above the ReLU kink
    sc, sh = torch.rand(C, generator=g, dtype=F64) + 0.5, torch.full((C,), 6.0, dtype=F64)
    v2 = v.detach().clone().requires_grad_(True)
    (R.maxpool2(torch.relu(v2 * sc + sh)) * dpool).sum().backward()
    routed = E.maxpool2_bwd(E.bn_apply(v2.detach(), sc, sh), dpool)
    close(routed * sc, v2.grad)
    s = torch.randn(N, H // 2, W // 2, C, generator=g, dtype=F64).requires_grad_(True)
    dup = torch.randn(shape, generator=g, dtype=F64)
    (R.upsample_nearest2(s) * dup).sum().backward()
    close(E.upsample2_bwd(dup), s.grad)
    close(E.upsample2_bwd(dup, addend=dpool, mask=s.detach(), mask_scale=2.0),
          torch.where(s.detach() > 0, (s.grad + dpool) * 2.0, torch.zeros((), dtype=F64)))
    close(E.add_mask(add, b=mask, mask=v.detach(), mask_scale=0.5),
          torch.where(v.detach() > 0, (add + mask) * 0.5, torch.zeros((), dtype=F64)))


def test_pool_argmax_takes_the_first_maximum():
    v = torch.zeros(1, 2, 4, 1, dtype=F64)
    v[0, :, 2:, 0] = torch.tensor([[1.0, 3.0], [3.0, 3.0]])   # window 0 all equal, window 1 ties at (0,1),(1,0),(1,1)
    assert E.pool_argmax(v).reshape(-1).tolist() == [0, 1]
    d = E.maxpool2_bwd(v, torch.tensor([5.0, 7.0], dtype=F64).reshape(1, 1, 2, 1))
    assert d.reshape(2, 4).tolist() == [[5.0, 0.0, 0.0, 7.0], [0.0, 0.0, 0.0, 0.0]]


@pytest.mark.parametrize("softmax2", [False, True])
@pytest.mark.parametrize("cs,cin", [(8, 8), (8, 1), (48, 44)])
def test_heads_match_autograd(softmax2, cs, cin):
    g = gen(cs + cin)
    nout = 2 if softmax2 else 1
    x = torch.randn(2, 3, 5, cs, generator=g, dtype=F64)
    k = (torch.randn(1, 1, cin, nout, generator=g, dtype=F64) * 0.3).requires_grad_(True)
    b = (torch.randn(nout, generator=g, dtype=F64) * 0.1).requires_grad_(True)
    xr = x[..., :cin].clone().requires_grad_(True)
    z = R.conv1x1(xr, k, b)
    p = torch.softmax(z, -1)[..., 1] if softmax2 else torch.sigmoid(z)[..., 0]
    dp = torch.randn(p.shape, generator=g, dtype=F64)
    (p * dp).sum().backward()
    Wp = k.detach()[0, 0].T.contiguous()   # packed layout W[o*Cin + c]
    xm = x.reshape(-1, cs)
    close(E.head_fwd(xm, Wp, b, softmax2=softmax2), p.detach().reshape(-1))
    dx, dW, dB = E.head_bwd(xm, Wp, p.detach(), dp, softmax2=softmax2)
    close(dW, k.grad[0, 0].T)
    close(dB, b.grad)
    close(dx[:, :cin], xr.grad.reshape(-1, cin))
    assert dx[:, cin:].abs().sum().item() == 0.0
    # BatchNorm + ReLU on load, and the BatchNorm-backward step below the sigmoid head
    sc, sh = torch.rand(cs, generator=g, dtype=F64) + 0.5, torch.randn(cs, generator=g, dtype=F64) * 0.3
    zr = x.clone().requires_grad_(True)
    kk, bb = k.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
    z2 = R.conv1x1(torch.relu(zr * sc + sh)[..., :cin], kk, bb)
    p2 = torch.softmax(z2, -1)[..., 1] if softmax2 else torch.sigmoid(z2)[..., 0]
    (p2 * dp).sum().backward()
    close(E.head_fwd(xm, Wp, b, softmax2=softmax2, bn=(sc, sh)), p2.detach().reshape(-1))
    dx2, dW2, dB2 = E.head_bwd(xm, Wp, p2.detach(), dp, softmax2=softmax2, bn=(sc, sh))
    close(dW2, kk.grad[0, 0].T)
    close(dB2, bb.grad)
    close(torch.where(E.gate(xm, sc, sh), dx2, torch.zeros((), dtype=F64)) * sc, zr.grad.reshape(-1, cs))
    if not softmax2:
        mean, inv, gam = torch.randn(cs, generator=g, dtype=F64), torch.rand(cs, generator=g, dtype=F64) + 0.5, sc + 1
        dg, dbt = E.bn_bwd_reduce(dx2, xm, sc, sh, mean, inv)
        close(E.bn_bwd_apply_head(Wp, p2.detach(), dp, xm, sc, sh, mean, inv, gam, dg, dbt, 30.0, None),
              E.bn_bwd_apply(dx2, xm, sc, sh, mean, inv, gam, dg, dbt, 30.0))


RESIZES = [((16, 16), (128, 128)), ((5, 9), (10, 36)), ((7, 3), (7, 3)), ((6, 10), (15, 25)), ((20, 8), (50, 20))]


@pytest.mark.parametrize("src,dst", RESIZES, ids=[f"{a[0]}x{a[1]}to{b[0]}x{b[1]}" for a, b in RESIZES])
def test_resize_matches_half_pixel_bilinear(src, dst):
    g = gen(src[0] * dst[1])
    s = torch.randn(3, *src, generator=g, dtype=F64).requires_grad_(True)
    d = torch.randn(3, *dst, generator=g, dtype=F64)
    o = R.resize_bilinear_half_pixel(s[..., None], dst)[..., 0]
    (o * d).sum().backward()
    close(E.resize_bilinear_fwd(s, *dst, coord=np.float64), o.detach())
    close(E.resize_bilinear_bwd(d, *src, coord=np.float64), s.grad)
    if all(b % a == 0 and (b // a) & (b // a - 1) == 0 for a, b in zip(src, dst)):
        close(E.resize_bilinear_fwd(s, *dst), o.detach())   # power-of-two ratios: the f32 coordinates are exact
    for n_in, n_out in zip(src, dst):
        close(E.bilinear_matrix(n_in, n_out).sum(1), torch.ones(n_out, dtype=F64))


@pytest.mark.parametrize("wd,gs", [(0.0, 1.0), (2.0 ** -7, 1.0), (2.0 ** -7, 0.125)])
def test_adam_matches_keras(wd, gs):
    g = gen(19)
    hp = dict(lr=2.0 ** -10, beta1=0.875, beta2=1 - 2.0 ** -10, eps=2.0 ** -23)   # exact in f32
    w = torch.randn(300, generator=g, dtype=F64)
    ref = R.KerasAdam([w.clone()], weight_decay=wd, **hp)
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    for t in range(1, 5):
        gr = torch.randn(300, generator=g, dtype=F64)
        ref.step([gr])
        exact = hp["lr"] * np.sqrt(1 - hp["beta2"] ** t) / (1 - hp["beta1"] ** t)
        assert abs(E.adam_alpha(hp["lr"], hp["beta1"], hp["beta2"], t) - exact) <= 2.0 ** -24 * exact
        w, m, v = E.adam(w, gr / gs, m, v, step=t, weight_decay=wd, grad_scale=gs, alpha=exact, **hp)
        close(w, ref.p[0])
        close(m, ref.m[0])
        close(v, ref.v[0])
    close(E.ema(w, m, 0.75), 0.75 * w + 0.25 * m)


@pytest.mark.parametrize("ohem,smooth", [(True, False), (False, False), (True, True), (False, True)])
@pytest.mark.parametrize("keep", [0.7, 0.5, 1.0])
def test_loss_matches_reference_losses(monkeypatch, ohem, smooth, keep):
    """value = select term + dice from the statistics, gradient = autograd of the R.* loss (the epsilon taken as
    the double 1e-7 both sides: the f32 value the kernels use differs from it by 1e-8 relative)."""
    monkeypatch.setattr(E, "KEPS", 1e-7)
    monkeypatch.setattr(E, "ONE_M_KEPS", 1.0 - 1e-7)
    g = gen(17)
    N, H, W = 2, 11, 9
    ep, en = 0.03125, 0.0625
    p = torch.rand(N, H, W, generator=g, dtype=F64)
    p[0, 0, :4] = torch.tensor([0.0, 1.0, 1e-9, 1 - 1e-9], dtype=F64)   # the clip and its zero gradient
    p[1, 2, :2] = torch.tensor([1e-7, 1 - 1e-7], dtype=F64)             # the clip's edges: gradient passes
    y = (torch.rand(N, H, W, generator=g, dtype=F64) > 0.6).to(F64)
    pr = p.clone().requires_grad_(True)
    if ohem:
        L = R.ohem_loss_with_smoothing(y, pr, keep, ep, en) if smooth else R.ohem_loss(y, pr, keep)
    else:
        L = R.combined_loss_with_label_smoothing(y, pr, ep, en) if smooth else R.combined_loss_standard(y, pr)
    L.backward()
    rows, _, st = E.loss_rows(p, y, smooth, ep, en)
    close(rows, R.keras_bce_rows(R.smooth_labels(y, ep, en) if smooth else y, p))
    k = int(np.float32(H) * np.float32(keep)) if ohem else H
    kept, coef, term = E.loss_select(rows, W=W, ohem=ohem, keep_ratio=keep, weight=1.0, norm_rows=N * k)
    assert kept.sum(1).tolist() == [k] * N
    dice = 1.0 - (2 * st[0] + 1) / (st[1] + st[2] + 1)
    close(term + dice, L.detach())
    assert abs(coef - 1.0 / (N * k * W)) <= 2.0 ** -22 * coef   # the kernel's f32 coefficient
    close(E.loss_grad(p, y, kept.to(F64) / (N * k * W), st, weight=1.0, smooth=smooth, eps_pos=ep, eps_neg=en), pr.grad)
    close(st[3:6], torch.stack([(y * p).sum(), y.sum(), p.sum()]))
    assert st[6].item() == round(R.binary_accuracy(y, p).item() * N * H * W)   # (an f32 mean of 0 / 1)


def test_loss_select_keeps_the_lowest_index_among_ties():
    rows = torch.tensor([[2.0, 5.0, 5.0, 1.0, 5.0, 5.0, 0.5, 2.0]], dtype=F64)
    kept, _, term = E.loss_select(rows, W=4, ohem=True, keep_ratio=0.4, weight=1.0, norm_rows=3)   # k = 3
    assert kept[0].tolist() == [False, True, True, False, True, False, False, False]
    assert term == 5.0


def test_round_to_goes_through_f32():
    x = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -30, 1.0 + 2.0 ** -8], dtype=F64)   # above / on a bf16 tie
    assert E.rt(x, torch.bfloat16).tolist() == [1.0, 1.0]       # f32 drops the 2^-30 first: both ties, to even
    assert E.rt(x, torch.float32).tolist() == [1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8]
    assert E.rt(x, None) is x
    close(E.scale_rows(torch.ones(3, 2), torch.tensor([2.0, 3.0])), torch.tensor([[2.0, 2.0], [3.0, 3.0], [0.0, 0.0]]))
