"""Plain float64 reference of the step's bandwidth-bound passes -- TEST INFRASTRUCTURE ONLY.

One short function per pass of csrc/elementwise.hip and csrc/heads_loss.hip, written from the semantics
the kernels document (include/adipose_hip.h, the kernel header comments), in torch float64 on the CPU.
Every function takes the values the device gets (f32, or bf16-rounded) and returns float64.

The reference reproduces the kernels' DECISIONS exactly and their arithmetic only to float64:
  * the ReLU gate fmaf(z, sc, sh) > 0 has the sign of float64(z) * float64(sc) + float64(sh): the product
    of two f32 values is exact in f64 and rounding keeps the sign, so `gate` below is the kernel's gate;
  * the pool argmax is the first maximum in (0,0), (0,1), (1,0), (1,1) order over the stored values;
  * where a kernel rounds an intermediate to the storage type on purpose (the activation of the BNR and
    head forms, the argmax recomputed from z), the function takes `round_to` and rounds the same way:
    to f32 first (the kernel holds an f32 register), then to the storage type.
Activation maps are (..., C) with the channel last; per-channel vectors are (C,).
"""
from __future__ import annotations

import numpy as np
import torch

F64 = torch.float64
KEPS = float(np.float32(1e-7))                          # the kernels' f32 keras epsilon
ONE_M_KEPS = float(np.float32(1.0) - np.float32(1e-7))  # 1.f - KEPS as the kernels evaluate it


def f64(t):
    return torch.as_tensor(t).detach().cpu().to(F64)


def rt(x, dtype):
    """x rounded to the storage type `dtype` the way a kernel stores an f32 register, back in float64."""
    if dtype is None:
        return x
    return x.to(torch.float32).to(dtype).to(F64)


def _chan_sum(t):
    return t.reshape(-1, t.shape[-1]).sum(0)


# ------------------------------------------------------------------------------------- BatchNorm
def bn_finalize(ssum, ssq, count, gamma, beta, eps, momentum=0.0, rmean=None, rvar=None):
    """count > 0: batch statistics from the sums (var = q/n - mean^2, clamped at 0); count < 0: eval form,
    (ssum, ssq) hold the running (mean, var). Returns a dict of float64 vectors; the running statistics
    (momentum update with the unbiased variance, count > 1) only when given and in the training form."""
    s, q, g, b = f64(ssum), f64(ssq), f64(gamma), f64(beta)
    if count > 0:
        mean = s / count
        var = torch.clamp(q / count - mean * mean, min=0.0)
    else:
        mean, var = s, q
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = g * invstd
    out = {"mean": mean, "var": var, "invstd": invstd, "scale": scale, "shift": b - mean * scale}
    if rmean is not None and count > 0:
        unb = var * count / (count - 1.0) if count > 1 else var
        out["rmean"] = (1.0 - momentum) * f64(rmean) + momentum * mean
        out["rvar"] = (1.0 - momentum) * f64(rvar) + momentum * unb
    return out


def bn_pre(z, scale, shift):
    return f64(z) * f64(scale) + f64(shift)


def gate(z, scale, shift):
    """The ReLU gate z*scale + shift > 0 (exactly the kernels' fmaf(z, sc, sh) > 0)."""
    return bn_pre(z, scale, shift) > 0


def bn_apply(z, scale, shift, round_to=None):
    """relu(z*scale + shift); round_to: as the pass stores it."""
    return rt(torch.clamp(bn_pre(z, scale, shift), min=0.0), round_to)


def bn_bwd_reduce(dA, z, scale, shift, mean, invstd):
    """(dgamma, dbeta) = (sum db*xhat, sum db), db = dA*gate, xhat = (z - mean)*invstd."""
    db = torch.where(gate(z, scale, shift), f64(dA), torch.zeros((), dtype=F64))
    return _chan_sum(db * (f64(z) - f64(mean)) * f64(invstd)), _chan_sum(db)


def bn_bwd_apply_terms(dA, z, scale, shift, mean, invstd, gamma, dgamma, dbeta, count):
    """The three terms P*db, Q*(z - mean), R of dz (k = gamma*invstd, P = k, Q = -k*invstd*dgamma/count,
    R = -k*dbeta/count)."""
    k = f64(gamma) * f64(invstd)
    db = torch.where(gate(z, scale, shift), f64(dA), torch.zeros((), dtype=F64))
    t1 = k * db
    t2 = -k * f64(invstd) * f64(dgamma) / count * (f64(z) - f64(mean))
    t3 = (-k * f64(dbeta) / count).expand_as(t1)
    return t1, t2, t3


def bn_bwd_apply(dA, z, scale, shift, mean, invstd, gamma, dgamma, dbeta, count):
    t1, t2, t3 = bn_bwd_apply_terms(dA, z, scale, shift, mean, invstd, gamma, dgamma, dbeta, count)
    return t1 + t2 + t3


# --------------------------------------------------------------------------- pool / upsample / add
def _quads(x):
    """(N, H, W, C) -> (N, H/2, W/2, 4, C), the 2x2 window in (0,0), (0,1), (1,0), (1,1) order."""
    N, H, W, C = x.shape
    return x.reshape(N, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, H // 2, W // 2, 4, C)


def _unquads(q):
    N, Ho, Wo, _, C = q.shape
    return q.reshape(N, Ho, Wo, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, 2 * Ho, 2 * Wo, C)


def pool_argmax(v):
    """Index 0..3 of the first maximum of each 2x2 window, (N, H/2, W/2, C)."""
    q = _quads(f64(v))
    best, arg = q[..., 0, :].clone(), torch.zeros(q[..., 0, :].shape, dtype=torch.int64)
    for k in (1, 2, 3):
        up = q[..., k, :] > best
        best = torch.where(up, q[..., k, :], best)
        arg = torch.where(up, torch.full_like(arg, k), arg)
    return arg


def maxpool2_fwd(v):
    return _quads(f64(v)).max(dim=3).values


def _mask(x, mask, mask_scale):
    if mask is None:
        return x
    return torch.where(f64(mask) > 0, x * float(np.float32(mask_scale)), torch.zeros((), dtype=F64))


def maxpool2_bwd(v, dpool, addend=None, mask=None, mask_scale=1.0):
    """dsrc = route(dpool to the first maximum of v) + addend, then the ReLU mask (mask > 0 ? x*scale : 0).
    v: the values the argmax is taken over (with BatchNorm on load the caller passes bn_apply(src, ...);
    with the argmax recomputed from z, bn_apply(z, ..., round_to=T))."""
    arg = pool_argmax(v)
    dp = f64(dpool)
    routed = torch.stack([torch.where(arg == k, dp, torch.zeros((), dtype=F64)) for k in range(4)], dim=3)
    x = _unquads(routed)
    if addend is not None:
        x = x + f64(addend)
    return _mask(x, mask, mask_scale)


def upsample2_bwd(dup, addend=None, mask=None, mask_scale=1.0):
    """Gradient of the nearest 2x upsample: the sum of each 2x2 block, + addend, then the mask."""
    x = _quads(f64(dup)).sum(dim=3)
    if addend is not None:
        x = x + f64(addend)
    return _mask(x, mask, mask_scale)


def add_mask(a, b=None, mask=None, mask_scale=1.0):
    x = f64(a)
    if b is not None:
        x = x + f64(b)
    return _mask(x, mask, mask_scale)


# ----------------------------------------------------------------------------------------- heads
def head_act(x, bn=None, round_to=None):
    """What the head reads: x, or relu(x*scale + shift) rounded to the storage type (BatchNorm on load)."""
    return f64(x) if bn is None else bn_apply(x, bn[0], bn[1], round_to)


def head_logits(x, W, b, *, softmax2, bn=None, round_to=None):
    """x (M, Cs); W (nout, Cin) in the packed layout W[o*Cin + c]; channels >= Cin do not count.
    Returns (z, sum of |terms| of z), z = z1 - z0 for the two-class softmax (p = sigmoid(z) either way)."""
    nout = 2 if softmax2 else 1
    Wm, bv = f64(W).reshape(nout, -1), f64(b)
    a = head_act(x, bn, round_to)[..., :Wm.shape[1]]
    zs = a @ Wm.T + bv
    absz = a.abs() @ Wm.abs().T + bv.abs()
    if softmax2:
        return zs[..., 1] - zs[..., 0], absz[..., 0] + absz[..., 1]
    return zs[..., 0], absz[..., 0]


def head_fwd(x, W, b, *, softmax2, bn=None, round_to=None):
    """sigmoid(x.W + b), or channel 1 of the two-class softmax = 1 / (1 + exp(z0 - z1))."""
    return torch.sigmoid(head_logits(x, W, b, softmax2=softmax2, bn=bn, round_to=round_to)[0])


def head_bwd(x, W, p, dp, *, softmax2, bn=None, round_to=None, addend=None, mask=None, mask_scale=1.0):
    """(dx, dW, db) for the upstream gradient dp of p. dz = dp*p*(1-p) is d/dz for the sigmoid and
    d/d(z1 - z0) for the softmax: dW = (-s, +s), db = (-t, +t) there, s = sum dz*act, t = sum dz.
    dx = dz*(w1 - w0) (0 past Cin) + addend, then the mask. dW (nout, Cin)."""
    nout = 2 if softmax2 else 1
    Wm = f64(W).reshape(nout, -1)
    cin, cs = Wm.shape[1], x.shape[-1]
    a = head_act(x, bn, round_to)
    pz = f64(p).reshape(-1)
    dz = f64(dp).reshape(-1) * pz * (1.0 - pz)
    s = dz @ a.reshape(-1, cs)[:, :cin]
    t = dz.sum()
    wd = torch.zeros(cs, dtype=F64)
    wd[:cin] = Wm[1] - Wm[0] if softmax2 else Wm[0]
    dx = (dz[:, None] * wd).reshape(a.shape)
    if addend is not None:
        dx = dx + f64(addend)
    dx = _mask(dx, mask, mask_scale)
    if softmax2:
        return dx, torch.stack([-s, s]), torch.stack([-t, t])
    return dx, s[None], t[None]


def bn_bwd_apply_head(W, p, dp, z, scale, shift, mean, invstd, gamma, dgamma, dbeta, count, round_to):
    """bn_bwd_apply with dA = the dx the sigmoid head backward stores: T(dp*p*(1-p)*W[c]), 0 past Cin."""
    cs, Wv = z.shape[-1], f64(W).reshape(-1)
    wd = torch.zeros(cs, dtype=F64)
    wd[:Wv.numel()] = Wv
    pz = f64(p).reshape(-1)
    dA = rt(((f64(dp).reshape(-1) * pz * (1.0 - pz))[:, None] * wd).reshape(z.shape), round_to)
    return bn_bwd_apply(dA, z, scale, shift, mean, invstd, gamma, dgamma, dbeta, count)


# ---------------------------------------------------------------------------------------- resize
def bilinear_matrix(n_in, n_out, coord=np.float32):
    """(n_out, n_in) weights of the half-pixel bilinear resize: in = (o + 0.5)*scale - 0.5,
    lo = max(floor(in), 0), hi = min(ceil(in), n_in - 1), t = in - floor(in); row o has 1 - t at lo and t
    at hi. coord: the type the coordinates are evaluated in (the kernel's f32 by default)."""
    c = coord
    scale = c(c(n_in) / c(n_out))
    m = np.zeros((n_out, n_in), np.float64)
    for o in range(n_out):
        x = c(c(c(o) + c(0.5)) * scale) - c(0.5)
        fl = np.floor(x)
        lo = int(fl) if x > 0 else 0
        hi = int(np.ceil(x)) if x < n_in - 1 else n_in - 1
        t = float(c(x - fl))
        m[o, lo] += 1.0 - t
        m[o, hi] += t
    return torch.from_numpy(m)


def resize_bilinear_fwd(src, Ho, Wo, coord=np.float32):
    """src (N, Hs, Ws) -> (N, Ho, Wo)."""
    s = f64(src)
    return torch.einsum("oh,nhw,pw->nop", bilinear_matrix(s.shape[1], Ho, coord), s,
                        bilinear_matrix(s.shape[2], Wo, coord))


def resize_bilinear_bwd(dout, Hs, Ws, coord=np.float32):
    """The adjoint: dout (N, Ho, Wo) -> (N, Hs, Ws)."""
    d = f64(dout)
    return torch.einsum("oh,nop,pw->nhw", bilinear_matrix(Hs, d.shape[1], coord), d,
                        bilinear_matrix(Ws, d.shape[2], coord))


# ------------------------------------------------------------------------------------------ loss
def smooth_y(y, smooth, eps_pos=0.03, eps_neg=0.07):
    y = f64(y)
    if not smooth:
        return y
    ep, en = float(np.float32(eps_pos)), float(np.float32(eps_neg))
    return y * (1.0 - ep - en) + en


def loss_rows(p, y, smooth=False, eps_pos=0.03, eps_neg=0.07):
    """Row BCE (N, H) (Keras binary_crossentropy: p clipped to [eps, 1-eps], log(p + eps), mean over W),
    its per-pixel |terms| mean (for error bounds; with smoothed labels 1 - ys is a difference that cancels, so its
    two parts 1 and ys count separately), and the 8 batch statistics: sum ys*pc, sum ys, sum pc (smoothed labels,
    clipped p), sum y*p, sum y, sum p, count(y == (p > 0.5)), sum y*(p > 0.5)."""
    pv, yv = f64(p), f64(y)
    ys = smooth_y(y, smooth, eps_pos, eps_neg)
    pc = torch.clamp(pv, KEPS, ONE_M_KEPS)
    t1, t2 = ys * torch.log(pc + KEPS), (1.0 - ys) * torch.log(1.0 - pc + KEPS)
    pb = (pv > 0.5).to(F64)
    stats = torch.stack([(ys * pc).sum(), ys.sum(), pc.sum(), (yv * pv).sum(), yv.sum(), pv.sum(),
                         (yv == pb).to(F64).sum(), (yv * pb).sum()])
    a2 = (1.0 + ys) * torch.log(1.0 - pc + KEPS).abs() if smooth else t2.abs()
    return -(t1 + t2).mean(-1), (t1.abs() + a2).mean(-1), stats


def loss_select(row_bce, *, W, ohem, keep_ratio, weight, norm_rows):
    """row_bce (N, H) -> (kept (N, H) bool, coef, loss term). OHEM keeps the k = int(f32(H)*f32(keep))
    largest rows of each image, the lowest row index first among equal losses; coef = weight/(norm_rows*W)
    evaluated in f32 as the kernel does; term = weight * sum(kept rows) / norm_rows."""
    r = f64(row_bce)
    N, H = r.shape
    kept = torch.ones(N, H, dtype=torch.bool)
    if ohem:
        k = int(np.float32(H) * np.float32(keep_ratio))
        kept = torch.zeros(N, H, dtype=torch.bool)
        for n in range(N):
            order = np.argsort(-r[n].numpy(), kind="stable")   # descending, ties by ascending index
            kept[n, torch.from_numpy(order[:k].copy())] = True
    coef = float(np.float32(weight) / (np.float32(norm_rows) * np.float32(W)))
    term = float(np.float32(weight)) * (r * kept).sum().item() / float(np.float32(norm_rows))
    return kept, coef, term


def loss_grad_terms(p, y, row_coef, stats, *, weight, smooth=False, eps_pos=0.03, eps_neg=0.07):
    """The terms of d(loss)/dp: row_coef * dBCE/dp = rc * (-ys/(p + eps) + (1 - ys)/(1 - p + eps)) and the dice
    gradient g_i*ys + g_c, all 0 where p is outside [eps, 1-eps] (the clip has no gradient there). With smoothed
    labels 1 - ys = 1 - (y*(1 - ep - en) + en) is a difference of rounded values that cancels to 0.03: its two
    parts are separate terms, so that the sum of |terms| bounds its error (hard labels: 1 - y is exact, one
    term). row_coef (N, H); stats from loss_rows."""
    pv = f64(p)
    ys = smooth_y(y, smooth, eps_pos, eps_neg)
    st = f64(stats)
    den = st[1] + st[2] + 1.0
    w = float(np.float32(weight))
    g_i, g_c = -(w * 2.0) / den, w * (2.0 * st[0] + 1.0) / (den * den)
    rc = f64(row_coef).reshape(pv.shape[0], pv.shape[1], 1)
    inside = (pv >= KEPS) & (pv <= ONE_M_KEPS)
    inv1 = 1.0 / (1.0 - pv + KEPS)
    second = [rc * inv1, rc * (-ys * inv1)] if smooth else [rc * ((1.0 - ys) * inv1)]
    terms = [rc * (-ys / (pv + KEPS))] + second + [g_i * ys, g_c.expand_as(pv)]
    return [torch.where(inside, t, torch.zeros((), dtype=F64)) for t in terms]


def loss_grad(p, y, row_coef, stats, **kw):
    return sum(loss_grad_terms(p, y, row_coef, stats, **kw))


# ------------------------------------------------------------------------------- optimizer / flat
def adam_alpha(lr, beta1, beta2, step):
    """The bias-corrected step size, taken in double and handed to the kernel as f32."""
    lr, b1, b2 = (float(np.float32(v)) for v in (lr, beta1, beta2))
    return float(np.float32(lr * np.sqrt(1.0 - b2 ** step) / (1.0 - b1 ** step)))


def adam(w, g, m, v, *, lr, beta1, beta2, eps, step, weight_decay=0.0, grad_scale=1.0, alpha=None):
    """Keras Adam.update_step in the kernel's order: g *= grad_scale; w -= w*wd*lr (AdamW);
    m += (g - m)(1 - b1); v += (g^2 - v)(1 - b2); w -= m*alpha / (sqrt(v) + eps). Returns (w, m, v).
    alpha: the step size when the caller has it (default: adam_alpha, as the launcher computes it)."""
    lr_, b1, b2, ep, wd, gs = (float(np.float32(x)) for x in (lr, beta1, beta2, eps, weight_decay, grad_scale))
    if alpha is None:
        alpha = adam_alpha(lr, beta1, beta2, step)
    gi, wi, mi, vi = f64(g) * gs, f64(w), f64(m), f64(v)
    if wd != 0.0:
        wi = wi - wi * wd * lr_
    mi = mi + (gi - mi) * (1.0 - b1)
    vi = vi + (gi * gi - vi) * (1.0 - b2)
    return wi - (mi * alpha) / (torch.sqrt(vi) + ep), mi, vi


def ema(ema_buf, param, decay):
    d = float(np.float32(decay))
    return d * f64(ema_buf) + (1.0 - d) * f64(param)


def scale_rows(src, scale):
    """src (R, K) * scale[r], rows past len(scale) zero."""
    s = torch.zeros(src.shape[0], dtype=F64)
    n = min(src.shape[0], scale.numel())
    s[:n] = f64(scale).reshape(-1)[:n]
    return f64(src) * s[:, None]
