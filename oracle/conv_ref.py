"""Plain float64 reference of the convolution launches -- TEST INFRASTRUCTURE ONLY.

What ops.conv_fwd, ops.conv_wgrad and the data-gradient packers compute, restated from the documented semantics
(ops.py, include/adipose_hip.h, the FwdArgs / WgradArgs comments of csrc/conv_common.h) in torch float64 on the
CPU; nothing here is taken from a kernel. Activations are NHWC (N, H, W, Cs) with the channel STRIDE as last
dimension (pad channels included: the device multiplies them too), weights are the packed GEMM matrix
W[n][k], k = tap*(CA + CB) + c, tap = ky*kw + kx; only W[:nout, :K] counts.

Every function takes the values the device gets (f32, or bf16-rounded) and returns float64. Where the device
rounds on purpose (the store, the BatchNorm-on-load activation, the dz of a fused bn_apply) the function
rounds the same way through ew_ref.rt. Next to every sum it returns A = the sum of |terms| of that sum: with
integer operands and A < 2^24 every f32 partial sum of the device is an exact integer in any summation order
(`exact`), and on real-valued data A is the base of the derived gates.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ew_ref as E
from .ew_ref import F64, f64, rt

EXACT_LIMIT = float(2 ** 24)


# ------------------------------------------------------------------------------------- dropout
def adp_hash(x):
    """common.h adp_hash on numpy uint32 arrays (wrapping arithmetic)."""
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def adp_uniform(seed, idx):
    """common.h adp_uniform: idx a numpy uint64 array of element indices; returns float64 in [0, 1) (a multiple of
    2^-24, so it is also the f32 value the kernel compares)."""
    idx = np.asarray(idx, dtype=np.uint64)
    lo = (idx & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    hi = (idx >> np.uint64(32)).astype(np.uint32)
    with np.errstate(over="ignore"):
        h = adp_hash(np.uint32(seed & 0xFFFFFFFF) ^ adp_hash(lo ^ adp_hash(hi + np.uint32(0x9e3779b9))))
    return (h >> np.uint32(8)).astype(np.float64) / 16777216.0


def dropout_keep(seed, rate, M, nout):
    """(M, nout) bool: element m*nout + n is kept when adp_uniform >= rate (rate as the f32 the kernel holds)."""
    idx = np.arange(M, dtype=np.uint64)[:, None] * np.uint64(nout) + np.arange(nout, dtype=np.uint64)[None, :]
    return torch.from_numpy(adp_uniform(seed, idx) >= float(np.float32(rate)))


# -------------------------------------------------------------------------------------- gather
def out_size(n_src, *, up, stride, k, dil, pad):
    return (n_src * (2 if up else 1) + 2 * pad - dil * (k - 1) - 1) // stride + 1


def _coords(n_src, n_out, k, stride, dil, pad, up):
    """Source index and validity of (output o, tap t): virtual coordinate o*stride + t*dil - pad on the grid
    upsampled x2 by nearest where `up`; outside the virtual grid the operand is zero."""
    v = torch.arange(n_out)[:, None] * stride + torch.arange(k)[None, :] * dil - pad
    ok = (v >= 0) & (v < n_src * (2 if up else 1))
    s = torch.where(ok, torch.div(v.clamp(min=0), 2 if up else 1, rounding_mode="floor"), torch.zeros_like(v))
    return s, ok


def gather(srcs, *, Ho=None, Wo=None, up=False, stride=1, kh=3, kw=3, dil=1, pad=None):
    """The implicit GEMM's A operand X[N, Ho, Wo, K], K index = tap*(CA + CB) + c, one or two sources
    concatenated per tap. pad None: 'same' for odd kernels, as ops.conv_geometry."""
    x = torch.cat([f64(s) for s in srcs], -1)
    N, Hs, Ws, C = x.shape
    if pad is None:
        pad = dil * (kh // 2)
    Ho = out_size(Hs, up=up, stride=stride, k=kh, dil=dil, pad=pad) if Ho is None else Ho
    Wo = out_size(Ws, up=up, stride=stride, k=kw, dil=dil, pad=pad) if Wo is None else Wo
    iy, oky = _coords(Hs, Ho, kh, stride, dil, pad, up)
    ix, okx = _coords(Ws, Wo, kw, stride, dil, pad, up)
    g = x[:, iy][:, :, :, ix]                                  # N, Ho, kh, Wo, kw, C
    ok = oky[None, :, :, None, None, None] & okx[None, None, None, :, :, None]
    g = torch.where(ok, g, torch.zeros((), dtype=F64))
    return g.permute(0, 1, 3, 2, 4, 5).reshape(N, Ho, Wo, kh * kw * C)


def scatter(cols, Hs, Ws, *, stride=1, kh=3, kw=3, dil=1, pad=None):
    """The transpose of gather (no upsample): cols[N, Ho, Wo, K] -> [N, Hs, Ws, C], every column added to the
    source element gather read it from."""
    N, Ho, Wo, K = cols.shape
    C = K // (kh * kw)
    if pad is None:
        pad = dil * (kh // 2)
    iy, oky = _coords(Hs, Ho, kh, stride, dil, pad, False)
    ix, okx = _coords(Ws, Wo, kw, stride, dil, pad, False)
    c6 = cols.reshape(N, Ho, Wo, kh, kw, C)
    out = torch.zeros(N, Hs, Ws, C, dtype=F64)
    for ky in range(kh):
        for kx in range(kw):
            oy, ox = torch.nonzero(oky[:, ky]).reshape(-1), torch.nonzero(okx[:, kx]).reshape(-1)
            if oy.numel() == 0 or ox.numel() == 0:
                continue
            part = c6[:, oy][:, :, ox][:, :, :, ky, kx]       # N, |oy|, |ox|, C
            rows = torch.zeros(N, Hs, ox.numel(), C, dtype=F64)
            rows.index_add_(1, iy[oy, ky], part)
            out.index_add_(2, ix[ox, kx], rows)
    return out


# ------------------------------------------------------------------------------------- forward
def _mask(x, mask, mask_scale):
    return torch.where(f64(mask) > 0, x * float(np.float32(mask_scale)), torch.zeros((), dtype=F64))


def pixel_shuffle(v, cps):
    """[N, Ho, Wo, 4*cps] (n = sub*cps + c, sub = 2*dy + dx) -> [N, 2Ho, 2Wo, cps]."""
    N, Ho, Wo, _ = v.shape
    return v.reshape(N, Ho, Wo, 2, 2, cps).permute(0, 1, 3, 2, 4, 5).reshape(N, 2 * Ho, 2 * Wo, cps)


def pixel_unshuffle(v):
    """The inverse: [N, 2Ho, 2Wo, cps] -> [N, Ho, Wo, 4*cps]."""
    N, H2, W2, cps = v.shape
    return v.reshape(N, H2 // 2, 2, W2 // 2, 2, cps).permute(0, 1, 3, 2, 4, 5).reshape(N, H2 // 2, W2 // 2, 4 * cps)


def _chan(t):
    return t.reshape(-1, t.shape[-1]).sum(0)


def conv_fwd(srcs, W, nout, *, bn_load=None, bias=None, Ho=None, Wo=None, up=False, stride=1, kh=3, kw=3, dil=1,
             pad=None, relu=False, dropout_rate=0.0, dropout_seed=0, out_mode=0, shuffle_c=0, split_c=0,
             addend=None, mask=None, mask_scale=1.0, mask2=None, mask2_scale=1.0, accum=None, bn_stats=False,
             bn_reduce=None, round_to=None, gemm=None, v_round=None):
    """One forward-shaped launch. srcs: one or two NHWC maps; bn_load: per source None or (scale, shift), the
    BatchNorm on load: rt(relu(x*scale + shift)) is what the conv multiplies (returned as "act", what act_out
    receives). Epilogue in the kernel's order: bias (index n % shuffle_c in pixel-shuffle mode) -> relu -> dropout
    -> addend -> mask -> store. bn_reduce = (z, scale, shift, mean, invstd).

    Returns a dict: "v" the f32 value before the storage rounding [N, Ho, Wo, nout]; "out" (and "out2" of a split
    store) as stored, "out" pixel-shuffled in out_mode 1; "A_out" the sum of |terms| of v; "keep" the dropout mask;
    "accum" = accum + the stored value; "stats" = (sum v, sum v^2) per channel (n % shuffle_c in mode 1) with
    "A_stats" = (sum |v|, sum v^2); "bnr" = (dgamma, dbeta) of the stored gradient with "A_bnr"; "act".
    gemm = (v, A): the accumulator and its sum of |terms| from elsewhere (conv_dgrad / convt_dgrad: a data-gradient
    launch, whose epilogue is this one); srcs and W are then not read.
    v_round (torch.float32): round accumulator + bias to the f32 register the device holds. On integer data this
    changes nothing; on real-valued data with a one-hot weight (an exact GEMM) it makes "v" the very f32 values the
    device sums and stores, so its fused sums can be held to the float64 sums of the same values."""
    acts = []
    for i, s in enumerate(srcs if gemm is None else []):
        bl = bn_load[i] if bn_load is not None else None
        acts.append(f64(s) if bl is None else E.bn_apply(s, bl[0], bl[1], round_to))
    if gemm is None:
        X = gather(acts, Ho=Ho, Wo=Wo, up=up, stride=stride, kh=kh, kw=kw, dil=dil, pad=pad)
        Wm = f64(W)[:nout, :X.shape[-1]]
        v = X @ Wm.T
        A = X.abs() @ Wm.abs().T
    else:
        v, A = f64(gemm[0])[..., :nout], f64(gemm[1])[..., :nout]
    N, Ho, Wo = v.shape[:3]
    if bias is not None:
        b = f64(bias).reshape(-1)
        b = b[torch.arange(nout) % shuffle_c] if out_mode == 1 else b[:nout]
        v, A = v + b, A + b.abs()
    if v_round is not None:
        v = rt(v, v_round)
    if relu:
        v = v.clamp(min=0.0)
    res = {}
    if dropout_rate > 0:
        keep = dropout_keep(dropout_seed, dropout_rate, N * Ho * Wo, nout).reshape(v.shape)
        ks = float(np.float32(1.0) / (np.float32(1.0) - np.float32(dropout_rate)))
        v = torch.where(keep, v * ks, torch.zeros((), dtype=F64))
        A = A * ks
        res["keep"] = keep
    n1 = split_c if out_mode == 2 else nout
    if out_mode != 1:
        v1 = v[..., :n1]
        if addend is not None:
            ad = f64(addend)[..., :n1]
            v1 = v1 + ad
            A = torch.cat([A[..., :n1] + ad.abs(), A[..., n1:]], -1)
        if mask is not None:
            v1 = _mask(v1, f64(mask)[..., :n1], mask_scale)
        v2 = v[..., n1:]
        if out_mode == 2 and mask2 is not None:
            v2 = _mask(v2, f64(mask2)[..., :nout - n1], mask2_scale)
        v = torch.cat([v1, v2], -1)
    res["v"], res["A_out"] = v, A
    stored = rt(v, round_to)
    if out_mode == 1:
        res["out"] = pixel_shuffle(stored, shuffle_c)
    else:
        res["out"] = stored[..., :n1]
        if out_mode == 2:
            res["out2"] = stored[..., n1:]
    if accum is not None:
        res["accum"] = f64(accum)[..., :n1] + stored[..., :n1]
    if bn_stats:
        s, q, a = _chan(v), _chan(v * v), _chan(v.abs())
        if out_mode == 1:
            s, q, a = (t.reshape(4, shuffle_c).sum(0) for t in (s, q, a))
        res["stats"], res["A_stats"] = (s, q), (a, q)
    if bn_reduce is not None:
        z, sc, sh, mu, ist = bn_reduce
        c = slice(0, nout)
        zz, scc, shh, muu, iss = f64(z)[..., c], f64(sc)[c], f64(sh)[c], f64(mu)[c], f64(ist)[c]
        res["bnr"] = E.bn_bwd_reduce(stored, zz, scc, shh, muu, iss)
        db = torch.where(E.gate(zz, scc, shh), stored, torch.zeros((), dtype=F64))
        res["A_bnr"] = (_chan((db * (zz - muu) * iss).abs()), _chan(db.abs()))
    if bn_load is not None:
        res["act"] = acts
    return res


# ------------------------------------------------------------------------------- data gradients
def conv_dgrad(dY, Wmaster, nout, cin_s, *, Hs, Ws, stride=1, kh=3, kw=3, dil=1, pad=None):
    """The data gradient of a convolution as the float64 transpose of the forward, from the MASTER weights
    Wmaster[n][tap*cin_s + c]: dX[N, Hs, Ws, cin_s] (on the virtual grid of an upsampled layer) and its sum of
    |terms|. The device path is pack_weights(mode 1) -> conv_fwd(dY), checked together with its packer."""
    d = f64(dY)[..., :nout]
    Wm = f64(Wmaster)[:nout, :kh * kw * cin_s]
    kwargs = dict(stride=stride, kh=kh, kw=kw, dil=dil, pad=pad)
    return scatter(d @ Wm, Hs, Ws, **kwargs), scatter(d.abs() @ Wm.abs(), Hs, Ws, **kwargs)


def convt_fwd(x, Wmaster, cps, **kw):
    """ConvTranspose 2x2 / stride 2 forward: the 1x1 GEMM with Nout = 4*cps and the pixel-shuffle store."""
    return conv_fwd([x], Wmaster, 4 * cps, kh=1, kw=1, pad=0, out_mode=1, shuffle_c=cps, **kw)


def convt_dgrad(dY, Wmaster, cps, cin_s):
    """The data gradient of that ConvTranspose from the master weights Wmaster[sub*cps + c][ci]: dX[N, H, W, cin_s]
    = unshuffle(dY) @ W, and its sum of |terms| (device: pack_weights(mode 2) -> the stride-2 four-tap gather)."""
    d = pixel_unshuffle(f64(dY)[..., :cps])
    Wm = f64(Wmaster)[:4 * cps, :cin_s]
    return d @ Wm, d.abs() @ Wm.abs()


# ------------------------------------------------------------------------------ weight gradient
def conv_wgrad(srcs, dY, nout, *, bn_load=None, Ho=None, Wo=None, up=False, stride=1, kh=3, kw=3, dil=1, pad=None,
               shuffle_c=0, bn_apply=None, round_to=None):
    """dW[n][k] = sum_m dY[m][n] * X_k[m], dB[n] = sum_m dY[m][n] (n % shuffle_c for the pixel-shuffled dY of a
    ConvTranspose). bn_apply = (dA, z, scale, shift, mean, invstd, gamma, dgamma, dbeta, count): dY is first
    dz = rt(bn_bwd_apply(...)), returned as "dz" (stored and used).
    Returns a dict: "dW" [nout, K], "dB", "A_dW", "A_dB" and, with bn_apply, "dz"."""
    acts = []
    for i, s in enumerate(srcs):
        bl = bn_load[i] if bn_load is not None else None
        acts.append(f64(s) if bl is None else E.bn_apply(s, bl[0], bl[1], round_to))
    res = {}
    if bn_apply is not None:
        dA, z, sc, sh, mu, ist, gam, dg, dbt, count = bn_apply
        c = slice(0, nout)
        d = rt(E.bn_bwd_apply(f64(dA)[..., c], f64(z)[..., c], f64(sc)[c], f64(sh)[c], f64(mu)[c], f64(ist)[c],
                              f64(gam)[c], f64(dg)[c], f64(dbt)[c], float(np.float32(count))), round_to)
        res["dz"] = d
    elif shuffle_c:
        d = pixel_unshuffle(f64(dY)[..., :shuffle_c])
    else:
        d = f64(dY)[..., :nout]
    Ho, Wo = d.shape[1], d.shape[2]
    X = gather(acts, Ho=Ho, Wo=Wo, up=up, stride=stride, kh=kh, kw=kw, dil=dil, pad=pad)
    X2, d2 = X.reshape(-1, X.shape[-1]), d.reshape(-1, nout)
    res["dW"], res["A_dW"] = d2.T @ X2, d2.abs().T @ X2.abs()
    dB, aB = d2.sum(0), d2.abs().sum(0)
    if shuffle_c:
        dB, aB = dB.reshape(4, shuffle_c).sum(0), aB.reshape(4, shuffle_c).sum(0)
    res["dB"], res["A_dB"] = dB, aB
    return res


# ----------------------------------------------------------------------------------- comparisons
def exact(*terms, grid=1.0):
    """The exactness condition: every sum of |terms| below 2^24 * grid, the operands' products being multiples of
    `grid` (1 for integers): every f32 partial sum is then an exact multiple of grid in any summation order."""
    return all(float(f64(t).abs().max()) < EXACT_LIMIT * grid for t in terms)


def assert_exact(got, ref, what="", sentinel=None, guard=None):
    """got (any dtype) equals the float64 reference bit for bit: both compared in float64, where bf16 and f32
    values are exact. guard: the part of the buffer the launch must not write, which must still hold `sentinel`."""
    g, r = f64(got), f64(ref)
    assert g.shape == r.shape, f"{what}: shape {tuple(g.shape)} != {tuple(r.shape)}"
    if not torch.equal(g, r):
        bad = torch.nonzero(g != r)
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {g.numel()} elements differ; first at {i}: "
                             f"got {g[i].item()!r}, reference {r[i].item()!r}")
    if guard is not None:
        gd = f64(guard)
        if not bool((gd == float(sentinel)).all()):
            bad = torch.nonzero(gd != float(sentinel))
            i = tuple(bad[0].tolist())
            raise AssertionError(f"{what}: guard written at {i}: {gd[i].item()!r} (sentinel {sentinel})")


def sum_gate(K, A):
    """an f32 chain of K additions over terms of absolute sum A is within (K + 8) * 2^-24 * A."""
    return (K + 8) * 2.0 ** -24 * f64(A)


def assert_sum_gate(got, ref, A, K, what=""):
    """|got - ref| <= (K + 8) * 2^-24 * A elementwise; returns the largest error / gate (for the record)."""
    g, r, gate = f64(got), f64(ref), sum_gate(K, A)
    err = (g - r).abs()
    ratio = torch.where(gate > 0, err / gate.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                           torch.zeros_like(err)))
    worst = float(ratio.max())
    if not worst <= 1.0:
        i = int(ratio.argmax())
        raise AssertionError(f"{what}: error / gate = {worst:.3g} at {i}: got {g.reshape(-1)[i].item()!r}, "
                             f"reference {r.reshape(-1)[i].item()!r}, gate {gate.reshape(-1)[i].item():.3g} (K = {K})")
    return worst
