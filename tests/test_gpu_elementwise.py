"""The HBM-bound passes of the step (csrc/elementwise.hip, csrc/heads_loss.hip) against the plain float64
reference oracle/ew_ref.py (itself checked on the CPU by tests/test_ew_ref.py), at the shapes where kernels
of this form go wrong: channel counts whose groups do not divide the block (idle threads), pixel counts that
leave tails, capped grids (unrolled loop and tail in one launch), every unroll, ties, and grids that wrap.

Gates (derived), with A = the sum of the absolute values of the reference's terms in f64:
  f32 elementwise   |got - ref| <= 16 * 2^-24 * A        (no term passes through more than 8 f32 roundings)
  bf16 elementwise  the f32 bound + 2^-8 * |ref|         (one rounding, or one ulp across a rounding boundary)
  reductions        |got - ref| <= (K + 8) * 2^-24 * sum|terms|, K the longest f32 summation chain
Inputs on a dyadic grid make every intermediate exact in both types: those cases assert equality.
Every output is a view of a buffer one pixel longer, filled with 7.0: the tail must survive the launch."""
import contextlib
import math

import numpy as np
import pytest
import torch

from adipose_amd import ops
from oracle import ew_ref as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
DTS = [pytest.param(F32, id="f32"), pytest.param(BF16, id="bf16")]
U24 = 2.0 ** -24
TPB = 256


@contextlib.contextmanager
def options(**kw):
    """ops.set_option for the block (None: leave the default), restored in a finally."""
    kw = {k: v for k, v in kw.items() if v is not None}
    try:
        for k, v in kw.items():
            ops.set_option(k, v)
        yield
    finally:
        for k in kw:
            ops.set_option(k, None)


def gen(*seed):
    return torch.Generator().manual_seed(hash(tuple(int(s) for s in seed)) % (2 ** 31))


def dev(t, dt=F32):
    return t.to(dt).to(DEV).contiguous()


def host(t):
    return t.detach().to("cpu").to(F64)


class Guarded:
    """An output of `shape` as a view of a buffer `pad` elements longer, all 7.0."""

    def __init__(self, shape, dt=F32, pad=None):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + (pad if pad is not None else shape[-1]),), 7.0, dtype=dt, device=DEV)
        self.t = self.buf[:self.n].view(*shape)

    def set(self, src):
        self.t.copy_(src)
        return self

    def ok(self):
        torch.cuda.synchronize()
        assert bool((self.buf[self.n:] == 7.0).all()), "wrote past the end of the output"
        return self.t


def elem_gate(got, ref, A, dt, what, extra=None):
    """f32 / bf16 elementwise gate; extra: an additional derived allowance (same shape)."""
    tol = 16 * U24 * A
    if dt == BF16:
        tol = tol + 2.0 ** -8 * ref.abs()
    if extra is not None:
        tol = tol + extra
    err = (host(got).reshape(ref.shape) - ref).abs()
    bad = err > tol
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {err.numel()} outside the gate, worst "
                                 f"err {err[bad].max().item():.3e} at tol {tol[bad][err[bad].argmax()].item():.3e}")


def sum_gate(got, ref, abssum, K, what):
    tol = (K + 8) * U24 * abssum
    err = (host(got).reshape(ref.shape) - ref).abs()
    bad = err > tol
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {err.numel()} outside the gate (K = {K}), worst "
                                 f"err {err[bad].max().item():.3e} at tol {tol[bad][err[bad].argmax()].item():.3e}")


def equal(got, ref, dt, what):
    """Bit equality with the reference stored to dt (inputs on a dyadic grid: every intermediate is exact)."""
    r = E.rt(ref, dt)
    g = host(got).reshape(r.shape)
    assert torch.equal(g, r), f"{what}: {int((g != r).sum())} of {r.numel()} differ"


def lanes_of(C):
    return TPB // (C // 8)


# ------------------------------------------------------------------------------------------- BatchNorm
BN_C = [8, 48, 64, 88, 192, 352, 1024, 2048]
BN_M = ["one", "lanes-1", "lanes+1", "4*lanes*3+lanes+3", "prime1499"]


def bn_m(kind, C):
    lanes = lanes_of(C)
    return {"one": 1, "lanes-1": max(1, lanes - 1), "lanes+1": lanes + 1, "4*lanes*3+lanes+3": 4 * lanes * 3 + lanes + 3,
            "prime1499": 1499}[kind]


def bn_case(C, M, dt, seed):
    """z, dA of (M, C) and per-channel coefficients (negative gammas / scales included)."""
    g = gen(C, M, seed)
    sign = torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)
    c = {"z": dev(torch.randn(M, C, generator=g) * 2, dt), "dA": dev(torch.randn(M, C, generator=g), dt),
         "sc": dev((torch.rand(C, generator=g) + 0.5) * sign), "sh": dev(torch.randn(C, generator=g) * 0.5),
         "mean": dev(torch.randn(C, generator=g) * 0.3), "inv": dev(torch.rand(C, generator=g) + 0.5),
         "gamma": dev((torch.rand(C, generator=g) + 0.5) * sign),
         "dgamma": dev(torch.randn(C, generator=g) * math.sqrt(M)), "dbeta": dev(torch.randn(C, generator=g) * math.sqrt(M))}
    return c


@pytest.mark.parametrize("cap", [pytest.param(None, id="capdefault"), pytest.param(3, id="cap3")])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("mkind", BN_M)
@pytest.mark.parametrize("C", BN_C, ids=[f"C{c}" for c in BN_C])
def test_bn_apply_and_bwd_apply_unrolls_u1_u2_u4(C, mkind, dt, cap):
    """adp_bn_apply and adp_bn_bwd_apply against float64, out of place and in place, at every unroll; the three
    unrolls give the same bits (the claim in the launcher's comment)."""
    M = bn_m(mkind, C)
    c = bn_case(C, M, dt, 1)
    ref_a = E.bn_apply(c["z"], c["sc"], c["sh"])
    A_a = (host(c["z"]) * host(c["sc"])).abs() + host(c["sh"]).abs()
    args = (c["sc"], c["sh"], c["mean"], c["inv"], c["gamma"], c["dgamma"], c["dbeta"], float(M))
    t = E.bn_bwd_apply_terms(c["dA"], c["z"], *args)
    ref_d, A_d = t[0] + t[1] + t[2], t[0].abs() + t[1].abs() + t[2].abs()
    outs_a, outs_d = [], []
    for U in (1, 2, 4):
        with options(bn_unroll=U, bn_cap=cap):
            out = Guarded((M, C), dt)
            ops.bn_apply(c["z"], c["sc"], c["sh"], out.t)
            inpl = Guarded((M, C), dt).set(c["z"])
            ops.bn_apply(inpl.t, c["sc"], c["sh"], inpl.t)
            dz = Guarded((M, C), dt)
            ops.bn_bwd_apply(c["dA"], c["z"], *args, dz.t)
            dinp = Guarded((M, C), dt).set(c["dA"])
            ops.bn_bwd_apply(dinp.t, c["z"], *args, dinp.t)
            out.ok(), dz.ok()
            if not outs_a:   # the other unrolls are held to the same bits below
                elem_gate(out.t, ref_a, A_a, dt, f"bn_apply U={U}")
                elem_gate(dz.t, ref_d, A_d, dt, f"bn_bwd_apply U={U}")
            assert torch.equal(inpl.ok(), out.t), f"bn_apply in place, U={U}"
            assert torch.equal(dinp.ok(), dz.t), f"bn_bwd_apply in place (dz == dA), U={U}"
            outs_a.append(out.t)
            outs_d.append(dz.t)
    assert torch.equal(outs_a[0], outs_a[1]) and torch.equal(outs_a[0], outs_a[2]), "bn_apply differs across unrolls"
    assert torch.equal(outs_d[0], outs_d[1]) and torch.equal(outs_d[0], outs_d[2]), "bn_bwd_apply differs across unrolls"


@pytest.mark.parametrize("cap", [pytest.param(None, id="capdefault"), pytest.param(3, id="cap3")])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("mkind", BN_M)
@pytest.mark.parametrize("C", BN_C, ids=[f"C{c}" for c in BN_C])
def test_bn_bwd_apply_head_unrolls_u1_u2_u4(C, mkind, dt, cap):
    """adp_bn_bwd_apply_head (dA = T(dp*p*(1-p)*W[c]) recomputed) against float64 at every unroll, Cin = C and
    C - 8; the unrolls give the same bits. bf16: the recomputed dA is rounded from an f32 product (three f32
    roundings) that may sit across a bf16 rounding boundary from the reference's float64 product, so the two dA
    differ by at most one bf16 ulp, which is at most 2^-7 relative (8 significant bits): allowance 2^-7 * |P*dA|.
    (The bit-for-bit check against the dx the head backward stores is test_head_backward_fused_bn_reduce's.)"""
    M = bn_m(mkind, C)
    c = bn_case(C, M, dt, 2)
    g = gen(C, M, 3)
    p, dp = dev(torch.rand(M, generator=g) * 0.98 + 0.01), dev(torch.randn(M, generator=g))
    args = (c["sc"], c["sh"], c["mean"], c["inv"], c["gamma"], c["dgamma"], c["dbeta"], float(M))
    for cin in sorted({C, max(8, C - 8)}):
        W = dev(torch.randn(cin, generator=g) * 0.3)
        wd = torch.zeros(C, dtype=F64)
        wd[:cin] = host(W)
        dA = E.rt(((host(dp) * host(p) * (1 - host(p)))[:, None] * wd), dt)
        t = E.bn_bwd_apply_terms(dA, c["z"], *args)
        ref, A = t[0] + t[1] + t[2], t[0].abs() + t[1].abs() + t[2].abs()
        outs = []
        for U in (1, 2, 4):
            with options(bn_unroll=U, bn_cap=cap):
                dz = Guarded((M, C), dt)
                ops.bn_bwd_apply_head(W, p, dp, c["z"], *args, dz.t, cin=cin)
                dz.ok()
                if not outs:   # the other unrolls are held to the same bits below
                    elem_gate(dz.t, ref, A, dt, f"bn_bwd_apply_head U={U} cin={cin}",
                              extra=2.0 ** -7 * t[0].abs() if dt == BF16 else None)
                outs.append(dz.t)
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), "differs across unrolls"


def _reduce_check(C, M, dt, seed):
    c = bn_case(C, M, dt, seed)
    g = gen(C, M, seed, 9)
    dg0, db0 = torch.randn(C, generator=g), torch.randn(C, generator=g)
    dg, db = Guarded((C,), pad=8).set(dev(dg0)), Guarded((C,), pad=8).set(dev(db0))   # it accumulates
    ops.bn_bwd_reduce(c["dA"], c["z"], c["sc"], c["sh"], c["mean"], c["inv"], dg.t, db.t)
    rg, rb_ = E.bn_bwd_reduce(c["dA"], c["z"], c["sc"], c["sh"], c["mean"], c["inv"])
    dabs = torch.where(E.gate(c["z"], c["sc"], c["sh"]), host(c["dA"]).abs(), torch.zeros((), dtype=F64))
    ag, ab = (dabs * ((host(c["z"]) - host(c["mean"])) * host(c["inv"])).abs()).sum(0), dabs.sum(0)
    lanes = lanes_of(C)
    blocks = min((M + lanes - 1) // lanes, 2048)
    K = (M + blocks * lanes - 1) // (blocks * lanes) + lanes
    sum_gate(dg.ok(), rg + E.f64(dg0), ag + dg0.abs().to(F64), K, "dgamma")
    sum_gate(db.ok(), rb_ + E.f64(db0), ab + db0.abs().to(F64), K, "dbeta")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("mkind", BN_M)
@pytest.mark.parametrize("C", BN_C, ids=[f"C{c}" for c in BN_C])
def test_bn_bwd_reduce(C, mkind, dt):
    """adp_bn_bwd_reduce adds the float64 sums into non-zero dgamma / dbeta."""
    _reduce_check(C, bn_m(mkind, C), dt, 4)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("C,M", [(2048, 2048 + 5), (1024, 2 * 2048 + 3), (352, 5 * 2048 + 7), (2048, 1000)],
                         ids=["C2048_above", "C1024_above", "C352_above", "C2048_below"])
def test_bn_bwd_reduce_grid_cap_2048(C, M, dt):
    """M on both sides of 2048 * lanes: above it the capped grid strides over the map a second time."""
    _reduce_check(C, M, dt, 5)


FIN_C = [1, 64, 65, 300, 2048]


def _finalize_check(got, ref, tol_var, gamma, beta, eps, momentum, rm0, rv0, count, what):
    """got: device vectors by name; ref: E.bn_finalize of the same f32 sums. Gates: mean 4 * 2^-24 relative, var
    `tol_var` (absolute), the rest by first-order propagation of those through rsqrt(var + eps)."""
    mean, var, inv, sc = ref["mean"], ref["var"], ref["invstd"], ref["scale"]
    gm, bt = host(gamma), host(beta)
    tol_mu = 4 * U24 * mean.abs()
    tol_is = 0.5 * inv ** 3 * tol_var + 4 * U24 * inv
    tol_sc = gm.abs() * tol_is + 2 * U24 * sc.abs()
    tol_sh = mean.abs() * tol_sc + sc.abs() * tol_mu + 4 * U24 * (bt.abs() + (mean * sc).abs())
    for name, r, tol in (("mean", mean, tol_mu), ("invstd", inv, tol_is), ("scale", sc, tol_sc),
                         ("shift", ref["shift"], tol_sh)):
        err = (host(got[name]) - r).abs()
        assert bool((err <= tol).all()), f"{what} {name}: err {err.max().item():.3e}, tol at it {tol[err.argmax()].item():.3e}"
    if "rmean" in ref:
        m = float(np.float32(momentum))
        unb = count / (count - 1.0) if count > 1 else 1.0
        tol_rm = m * tol_mu + 4 * U24 * (((1 - m) * host(rm0)).abs() + (m * mean).abs())
        tol_rv = m * unb * tol_var + 4 * U24 * (((1 - m) * host(rv0)).abs() + m * unb * var)
        for name, tol in (("rmean", tol_rm), ("rvar", tol_rv)):
            err = (host(got[name]) - ref[name]).abs()
            assert bool((err <= tol).all()), f"{what} {name}: err {err.max().item():.3e}, tol at it {tol[err.argmax()].item():.3e}"


@pytest.mark.parametrize("count", [1, 2, 4096, -1], ids=["n1", "n2", "n4096", "eval"])
@pytest.mark.parametrize("C", FIN_C, ids=[f"C{c}" for c in FIN_C])
def test_bn_finalize(C, count):
    """adp_bn_finalize: training statistics from f32 sums of a real data matrix with mean/std in {0, 3, 10} (the
    sums taken in float64, rounded once), the eval form (count < 0: the sums are the running mean / variance), with
    and without running statistics, momentum 0.1 and 1.0. var gate 8 * 2^-24 * (1 + mean^2/var) relative."""
    g = gen(C, count, 6)
    eps = 1e-3
    gamma = dev((torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0))
    beta = dev(torch.randn(C, generator=g) * 0.5)
    if count > 0:
        ratio = torch.tensor([0.0, 3.0, 10.0], dtype=F64)[torch.arange(C) % 3]
        x = torch.randn(count, C, generator=g, dtype=F64) + ratio
        ssum, ssq = dev(x.sum(0)), dev((x * x).sum(0))
    else:
        ssum, ssq = dev(torch.randn(C, generator=g)), dev(torch.rand(C, generator=g) + 0.1)
    for momentum in (0.1, 1.0):
        for running in (False, True):
            rm0, rv0 = dev(torch.randn(C, generator=g)), dev(torch.rand(C, generator=g) + 0.5)
            out = {k: Guarded((C,), pad=8) for k in ("scale", "shift", "mean", "invstd", "rmean", "rvar")}
            out["rmean"].set(rm0)
            out["rvar"].set(rv0)
            ops.bn_finalize(count, ssum, ssq, gamma, beta, eps, momentum, out["scale"].t, out["shift"].t, out["mean"].t,
                            out["invstd"].t, out["rmean"].t if running else None, out["rvar"].t if running else None)
            got = {k: v.ok() for k, v in out.items()}
            ref = E.bn_finalize(ssum, ssq, count, gamma, beta, eps, momentum, rm0 if running else None,
                                rv0 if running else None)
            what = f"momentum={momentum} running={running}"
            if count > 0:
                tol_var = 8 * U24 * (ref["var"] + ref["mean"] ** 2)
                # the variance itself is not an output: it is pinned through rvar at momentum 1 (rvar = unbiased var)
                assert bool((host(got["invstd"]) > 0).all())
            else:
                tol_var = torch.zeros(C, dtype=F64)
                assert torch.equal(host(got["mean"]), host(ssum)), "eval form: mean is the running mean"
            if not (running and count > 0):   # untouched: no running statistics given, or the eval form
                assert torch.equal(got["rmean"], rm0) and torch.equal(got["rvar"], rv0), what
            _finalize_check(got, ref, tol_var, gamma, beta, eps, momentum, rm0, rv0, count, what)


def test_bn_finalize_fold():
    """adp_bn_finalize_fold after a conv launch that left its statistics in the accumulator replicas: the folded
    sums are those of the non-deferred launch (and of the stored map, to its bf16 rounding), and the BatchNorm
    vectors are the float64 finalize of the folded sums."""
    g = gen(5)
    N, H, Wd, C = 2, 16, 32, 64
    x = torch.randn(N, H, Wd, 64, generator=g).to(DEV, BF16)
    Wt = (torch.randn(64, 9 * 64, generator=g) * 0.05).to(DEV, BF16)
    out = torch.zeros(N, H, Wd, C, device=DEV, dtype=BF16)
    gamma, beta = dev(torch.rand(C, generator=g) + 0.5), dev(torch.randn(C, generator=g))
    rm0, rv0 = dev(torch.randn(C, generator=g)), dev(torch.rand(C, generator=g) + 0.5)
    count, eps = N * H * Wd, 1e-3
    s_ref, q_ref = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    ops.conv_fwd(x, Wt, C, out=out, bn_stats=(s_ref, q_ref))
    for momentum, running in ((0.1, True), (1.0, True), (0.1, False)):
        s0, q0 = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        ops.conv_fwd(x, Wt, C, out=out, bn_stats=(s0, q0), defer_fold=True)
        o = {k: Guarded((C,), pad=8) for k in ("scale", "shift", "mean", "invstd", "rmean", "rvar")}
        o["rmean"].set(rm0)
        o["rvar"].set(rv0)
        ops.bn_finalize(count, s0, q0, gamma, beta, eps, momentum, o["scale"].t, o["shift"].t, o["mean"].t, o["invstd"].t,
                        o["rmean"].t if running else None, o["rvar"].t if running else None, fold=True)
        got = {k: v.ok() for k, v in o.items()}
        z = host(out).reshape(-1, C)
        # f64 replicas of f32 partials, folded once: the two launches agree to the f32 rounding of the result
        assert bool(((host(s0) - host(s_ref)).abs() <= 4 * U24 * z.abs().sum(0)).all())
        assert bool(((host(q0) - host(q_ref)).abs() <= 4 * U24 * (z * z).sum(0)).all())
        # and with the stored map: each stored value is within 2^-9 relative of the accumulator the sums saw
        # (plus the f32 partial sums, chains of at most `count` terms)
        chain = (count + 8) * U24
        assert bool(((host(s0) - z.sum(0)).abs() <= (2.0 ** -9 + chain) * z.abs().sum(0)).all())
        assert bool(((host(q0) - (z * z).sum(0)).abs() <= (2.0 ** -8 + chain) * (z * z).sum(0)).all())
        ref = E.bn_finalize(s0, q0, count, gamma, beta, eps, momentum, rm0 if running else None, rv0 if running else None)
        if not running:
            assert torch.equal(got["rmean"], rm0) and torch.equal(got["rvar"], rv0)
        _finalize_check(got, ref, 8 * U24 * (ref["var"] + ref["mean"] ** 2), gamma, beta, eps, momentum, rm0, rv0, count,
                        f"fold momentum={momentum} running={running}")


# ------------------------------------------------------------------------------ pool / upsample / add
POOL_SHAPES = [(1, 2, 2, 8), (3, 6, 10, 48), (2, 14, 2, 88), (1, 4, 34, 1024)]
POOL_IDS = ["x".join(map(str, s)) for s in POOL_SHAPES]


def dyadic(g, shape, lo, hi, step):
    """Multiples of `step` in [lo*step, hi*step]."""
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64) * step


def pool_case(shape, dt, seed, exact=True):
    N, H, W, C = shape
    g = gen(*shape, seed)
    half = (N, H // 2, W // 2, C)
    if exact:   # dyadic grid: every intermediate is exact in bf16 and f32, 2x2 ties are frequent
        c = {"z": dyadic(g, shape, -32, 32, 0.125), "sc": torch.tensor([0.5, 1.0, 2.0], dtype=F64)[torch.randint(0, 3, (C,), generator=g)],
             "sh": dyadic(g, (C,), -8, 8, 0.25), "dpool": dyadic(g, half, -16, 16, 0.25), "dfull": dyadic(g, shape, -16, 16, 0.25),
             "add": dyadic(g, shape, -16, 16, 0.25), "addh": dyadic(g, half, -16, 16, 0.25),
             "mask": dyadic(g, shape, -2, 2, 0.5), "maskh": dyadic(g, half, -2, 2, 0.5),
             "mean": dyadic(g, (C,), -4, 4, 0.25), "inv": torch.tensor([0.5, 1.0, 2.0], dtype=F64)[torch.randint(0, 3, (C,), generator=g)],
             "dg0": dyadic(g, (C,), -8, 8, 0.25), "db0": dyadic(g, (C,), -8, 8, 0.25)}
    else:
        r = lambda s, k=1.0: torch.randn(s, generator=g, dtype=F64) * k   # noqa: E731
        c = {"z": r(shape, 2), "sc": torch.rand(C, generator=g, dtype=F64) + 0.5, "sh": r((C,), 0.5), "dpool": r(half),
             "dfull": r(shape), "add": r(shape), "addh": r(half), "mask": r(shape), "maskh": r(half), "mean": r((C,), 0.3),
             "inv": torch.rand(C, generator=g, dtype=F64) + 0.5, "dg0": r((C,)), "db0": r((C,))}
    out = {}
    for k, v in c.items():
        out[k] = dev(v, dt if v.dim() == 4 else F32)
    return out


MS = [pytest.param(1.0, id="ms1"), pytest.param(1.0 / 0.7, id="ms1over0.7")]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=POOL_IDS)
def test_pool_forward_exact(shape, dt):
    """adp_maxpool2_fwd (plain and BatchNorm on load) and adp_bn_apply_maxpool2 on the dyadic grid: equality."""
    N, H, W, C = shape
    c = pool_case(shape, dt, 1)
    half = (N, H // 2, W // 2, C)
    p0, p1, p2, act = Guarded(half, dt), Guarded(half, dt), Guarded(half, dt), Guarded(shape, dt)
    ops.maxpool2_fwd(c["z"], p0.t)
    ops.maxpool2_fwd(c["z"], p1.t, bn=(c["sc"], c["sh"]))
    ops.bn_apply_maxpool2(c["z"], c["sc"], c["sh"], act.t, p2.t)
    a = E.bn_apply(c["z"], c["sc"], c["sh"])
    equal(p0.ok(), E.maxpool2_fwd(c["z"]), dt, "maxpool2_fwd")
    equal(p1.ok(), E.maxpool2_fwd(a), dt, "maxpool2_fwd bn")
    equal(act.ok(), a, dt, "bn_apply_maxpool2 act")
    equal(p2.ok(), E.maxpool2_fwd(a), dt, "bn_apply_maxpool2 pool")


@pytest.mark.parametrize("ms", MS)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=POOL_IDS)
def test_pool_upsample_add_backward_exact(shape, dt, ms):
    """adp_maxpool2_bwd, adp_upsample2_bwd and adp_ew_add_mask with / without BatchNorm on load, addend and mask on
    the dyadic grid (ties in most 2x2 windows: the first maximum takes the gradient): equality with the reference
    stored to the type (x * mask_scale is one f32 rounding of an exact product, as in the kernel)."""
    c = pool_case(shape, dt, 2)
    N, H, W, C = shape
    half = (N, H // 2, W // 2, C)
    for bn in (None, (c["sc"], c["sh"])):
        v = c["z"] if bn is None else E.bn_apply(c["z"], c["sc"], c["sh"])
        for add in (None, c["add"]):
            for mask in (None, c["mask"]):
                if mask is None and ms != 1.0:
                    continue
                d = Guarded(shape, dt)
                ops.maxpool2_bwd(c["z"], c["dpool"], d.t, bn=bn, addend=add, mask=mask, mask_scale=ms)
                equal(d.ok(), E.maxpool2_bwd(v, c["dpool"], add, mask, ms), dt,
                      f"maxpool2_bwd bn={bn is not None} add={add is not None} mask={mask is not None}")
    for add in (None, c["addh"]):
        for mask in (None, c["maskh"]):
            if mask is None and ms != 1.0:
                continue
            d = Guarded(half, dt)
            ops.upsample2_bwd(c["dfull"], d.t, addend=add, mask=mask, mask_scale=ms)
            equal(d.ok(), E.upsample2_bwd(c["dfull"], add, mask, ms), dt,
                  f"upsample2_bwd add={add is not None} mask={mask is not None}")
            o = Guarded(shape, dt)
            ops.add_mask(c["dfull"], o.t, b=None if add is None else c["add"], mask=None if mask is None else c["mask"],
                         mask_scale=ms)
            equal(o.ok(), E.add_mask(c["dfull"], None if add is None else c["add"], None if mask is None else c["mask"], ms),
                  dt, f"add_mask b={add is not None} mask={mask is not None}")


@pytest.mark.parametrize("blocks", [pytest.param(None, id="blocksdefault"), pytest.param(3, id="blocks3")])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=POOL_IDS)
def test_pool_backward_bnr_exact(shape, dt, blocks):
    """adp_maxpool2_bwd_bnr with the stored activation and with the argmax recomputed from z: dsrc and the fused
    BatchNorm-backward sums (added into non-zero dgamma / dbeta) equal the reference exactly on the dyadic grid."""
    c = pool_case(shape, dt, 3)
    a = torch.empty_like(c["z"])
    ops.bn_apply(c["z"], c["sc"], c["sh"], a)
    equal(a, E.bn_apply(c["z"], c["sc"], c["sh"]), dt, "stored activation")
    ref = E.maxpool2_bwd(E.bn_apply(c["z"], c["sc"], c["sh"], round_to=dt), c["dpool"], c["add"])
    rg, rb_ = E.bn_bwd_reduce(E.rt(ref, dt), c["z"], c["sc"], c["sh"], c["mean"], c["inv"])
    for from_z in (False, True):
        with options(pool_bnr_blocks=blocks):
            d, dg, db = Guarded(shape, dt), Guarded((shape[3],), pad=8).set(c["dg0"]), Guarded((shape[3],), pad=8).set(c["db0"])
            ops.maxpool2_bwd(a, c["dpool"], d.t, addend=c["add"], argmax_from_z=from_z,
                             bn_reduce=(c["z"], c["sc"], c["sh"], c["mean"], c["inv"], dg.t, db.t))
            equal(d.ok(), ref, dt, f"dsrc from_z={from_z}")
            equal(dg.ok(), rg + host(c["dg0"]), F32, f"dgamma from_z={from_z}")
            equal(db.ok(), rb_ + host(c["db0"]), F32, f"dbeta from_z={from_z}")


@pytest.mark.parametrize("dt", DTS)
def test_pool_upsample_add_random_values(dt):
    """One random-valued case per pass, gated: f32 elementwise / bf16 elementwise / reduction."""
    shape = (3, 6, 10, 48)
    N, H, W, C = shape
    half = (N, H // 2, W // 2, C)
    c = pool_case(shape, dt, 4, exact=False)
    ms = 1.0 / 0.7
    msf = float(np.float32(ms))
    a = E.bn_apply(c["z"], c["sc"], c["sh"])
    pl, pb = Guarded(half, dt), Guarded(half, dt)
    ops.maxpool2_fwd(c["z"], pl.t)
    ops.maxpool2_fwd(c["z"], pb.t, bn=(c["sc"], c["sh"]))
    equal(pl.ok(), E.maxpool2_fwd(c["z"]), dt, "maxpool2_fwd")   # a selection: exact
    A_a = (host(c["z"]) * host(c["sc"])).abs() + host(c["sh"]).abs()
    elem_gate(pb.ok(), E.maxpool2_fwd(a), E.maxpool2_fwd(A_a), dt, "maxpool2_fwd bn")
    act, p2 = Guarded(shape, dt), Guarded(half, dt)
    ops.bn_apply_maxpool2(c["z"], c["sc"], c["sh"], act.t, p2.t)
    elem_gate(act.ok(), a, A_a, dt, "bn_apply_maxpool2 act")
    equal(p2.ok(), E.maxpool2_fwd(act.t), dt, "bn_apply_maxpool2 pool of the stored act")
    d = Guarded(shape, dt)
    ops.maxpool2_bwd(c["z"], c["dpool"], d.t, addend=c["add"], mask=c["mask"], mask_scale=ms)
    A = E.maxpool2_bwd(c["z"], host(c["dpool"]).abs(), host(c["add"]).abs(), c["mask"], ms)
    elem_gate(d.ok(), E.maxpool2_bwd(c["z"], c["dpool"], c["add"], c["mask"], ms), A, dt, "maxpool2_bwd")
    u = Guarded(half, dt)
    ops.upsample2_bwd(c["dfull"], u.t, addend=c["addh"], mask=c["maskh"], mask_scale=ms)
    elem_gate(u.ok(), E.upsample2_bwd(c["dfull"], c["addh"], c["maskh"], ms),
              E.upsample2_bwd(host(c["dfull"]).abs(), host(c["addh"]).abs(), c["maskh"], ms), dt, "upsample2_bwd")
    o = Guarded(shape, dt)
    ops.add_mask(c["dfull"], o.t, b=c["add"], mask=c["mask"], mask_scale=ms)
    elem_gate(o.ok(), E.add_mask(c["dfull"], c["add"], c["mask"], ms),
              (host(c["dfull"]).abs() + host(c["add"]).abs()) * msf, dt, "add_mask")
    # BNR form: the argmax over the activation as the device stored it; the sums over the dsrc it stored
    ops.bn_apply(c["z"], c["sc"], c["sh"], act.t)
    for from_z in (False, True):
        d, dg, db = Guarded(shape, dt), Guarded((C,), pad=8).set(c["dg0"]), Guarded((C,), pad=8).set(c["db0"])
        ops.maxpool2_bwd(act.t, c["dpool"], d.t, addend=c["add"], argmax_from_z=from_z,
                         bn_reduce=(c["z"], c["sc"], c["sh"], c["mean"], c["inv"], dg.t, db.t))
        elem_gate(d.ok(), E.maxpool2_bwd(act.t, c["dpool"], c["add"]),
                  E.maxpool2_bwd(act.t, host(c["dpool"]).abs(), host(c["add"]).abs()), dt, f"bnr dsrc from_z={from_z}")
        rg, rb_ = E.bn_bwd_reduce(d.t, c["z"], c["sc"], c["sh"], c["mean"], c["inv"])
        gt = E.gate(c["z"], c["sc"], c["sh"])
        dabs = torch.where(gt, host(d.t).abs(), torch.zeros((), dtype=F64))
        xh = ((host(c["z"]) - host(c["mean"])) * host(c["inv"])).abs()
        lanes, P = lanes_of(C), N * (H // 2) * (W // 2)
        nb = min((P + lanes - 1) // lanes, 2048)
        K = 4 * ((P + nb * lanes - 1) // (nb * lanes)) + lanes   # four pixels per pooled pixel, then the LDS fold
        sum_gate(dg.ok(), rg + host(c["dg0"]), (dabs * xh).reshape(-1, C).sum(0) + host(c["dg0"]).abs(), K, "bnr dgamma")
        sum_gate(db.ok(), rb_ + host(c["db0"]), dabs.reshape(-1, C).sum(0) + host(c["db0"]).abs(), K, "bnr dbeta")


# ------------------------------------------------------------------------------------------------ heads
HEAD_M = [1, 7, "lanes+1", 1000]


def head_ms(Cs):
    G = Cs // 8
    return [1, 7, (TPB // G if G <= 64 and G & (G - 1) == 0 else TPB) + 1, 1000]


def head_cins(Cs, mult8=False):
    c = {Cs, Cs - 4, 1} if not mult8 else {Cs, Cs - 8}
    return sorted(x for x in c if x >= 1)


def head_abs(xm, W, p, dp, softmax2, bn, dt, add=None, mask=None, ms=1.0):
    """Sums of |terms| of the head backward: of dx (M, Cs) elementwise, of dW (nout * Cin) and of db (nout)."""
    nout = 2 if softmax2 else 1
    Wm = host(W).reshape(nout, -1)
    cin, (M, Cs) = Wm.shape[1], xm.shape
    adz = host(dp).abs() * host(p) * (1 - host(p))
    wd = torch.zeros(Cs, dtype=F64)
    wd[:cin] = (Wm[1].abs() + Wm[0].abs()) if softmax2 else Wm[0].abs()
    adx = adz[:, None] * wd
    if add is not None:
        adx = adx + host(add).abs().reshape(M, Cs)
    if mask is not None:
        adx = torch.where(host(mask).reshape(M, Cs) > 0, adx * float(np.float32(ms)), torch.zeros((), dtype=F64))
    aW = adz @ E.head_act(xm, bn, dt).abs()[:, :cin]
    return adx, aW.repeat(nout), adz.sum().expand(nout)


def head_case(M, Cs, cin, dt, softmax2, seed):
    g = gen(M, Cs, cin, seed)
    nout = 2 if softmax2 else 1
    sign = torch.where(torch.rand(Cs, generator=g) < 0.25, -1.0, 1.0)
    return {"x": dev(torch.randn(M, 1, 1, Cs, generator=g), dt), "W": dev(torch.randn(nout * cin, generator=g) * (2.0 / math.sqrt(cin))),
            "b": dev(torch.randn(nout, generator=g) * 0.3), "sc": dev((torch.rand(Cs, generator=g) + 0.5) * sign),
            "sh": dev(torch.randn(Cs, generator=g) * 0.5), "dp": dev(torch.randn(M, generator=g)),
            "add": dev(torch.randn(M, 1, 1, Cs, generator=g), dt), "mask": dev(torch.randn(M, 1, 1, Cs, generator=g), dt),
            "mean": dev(torch.randn(Cs, generator=g) * 0.3), "inv": dev(torch.rand(Cs, generator=g) + 0.5),
            "gamma": dev((torch.rand(Cs, generator=g) + 0.5) * sign)}


@pytest.mark.parametrize("softmax2", [pytest.param(False, id="sigmoid"), pytest.param(True, id="softmax2")])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("Cs", [8, 16, 48, 64, 128, 512, 1024], ids=["Cs8_G1", "Cs16_G2", "Cs48_generic", "Cs64_G8", "Cs128_G16",
                                                                     "Cs512_G64", "Cs1024_generic"])
def test_head_forward(Cs, dt, softmax2):
    """adp_head_{sigmoid,softmax2}_fwd at M in {1, 7, lanes + 1, 1000}, Cin in {Cs, Cs - 4, 1}, with and without
    BatchNorm on load. z is an f32 fma chain of at most Cs terms (the thread-per-pixel form; the grouped forms
    are shorter): |dz| <= (Cs + 8) * 2^-24 * sum|terms|; p = sigmoid(z) has slope <= 1/4, and expf, the add and
    the divide cost <= 8 * 2^-24 relative."""
    for M in head_ms(Cs):
        for cin in head_cins(Cs):
            c = head_case(M, Cs, cin, dt, softmax2, 1)
            for bn in (None, (c["sc"], c["sh"])):
                p = Guarded((M,), pad=8)
                ops.head_fwd(c["x"], c["W"], c["b"], p.t, cin=cin, softmax2=softmax2, bn=bn)
                z, az = E.head_logits(c["x"].reshape(M, Cs), c["W"], c["b"], softmax2=softmax2, bn=bn, round_to=dt)
                ref = torch.sigmoid(z)
                tol = 0.25 * (Cs + 8) * U24 * az + 8 * U24 * ref
                err = (host(p.ok()) - ref).abs()
                assert bool((err <= tol).all()), (f"M={M} cin={cin} bn={bn is not None}: err {err.max().item():.3e}, "
                                                  f"tol at it {tol[err.argmax()].item():.3e}")


@pytest.mark.parametrize("blocks", [pytest.param(None, id="blocksdefault"), pytest.param(2, id="blocks2")])
@pytest.mark.parametrize("softmax2", [pytest.param(False, id="sigmoid"), pytest.param(True, id="softmax2")])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("Cs", [8, 48, 64, 512], ids=lambda c: f"Cs{c}")
def test_head_backward(Cs, dt, softmax2, blocks):
    """adp_head_{sigmoid,softmax2}_bwd: dx (stored, with addend + mask, and dx=None), dW and db added into non-zero
    buffers; head_bwd_blocks=2 makes two blocks stride the map, so the 4-pixel pass and the tail both run at
    M = 1000. dW / db chains: pixels per thread + the LDS fold over the lanes + one f32 atomic per block."""
    nout = 2 if softmax2 else 1
    lanes = lanes_of(Cs)
    for M in [1, 7, lanes + 1, 1000]:
        nb = min((M + lanes - 1) // lanes, blocks or 10 ** 9)
        K = (M + nb * lanes - 1) // (nb * lanes) + lanes + nb
        for cin in head_cins(Cs):
            c = head_case(M, Cs, cin, dt, softmax2, 2)
            xm = c["x"].reshape(M, Cs)
            for bn in (None, (c["sc"], c["sh"])):
                p = torch.empty(M, device=DEV)
                ops.head_fwd(c["x"], c["W"], c["b"], p, cin=cin, softmax2=softmax2, bn=bn)
                for extras in (False, True):
                    add, mask, ms = (c["add"], c["mask"], 1.0 / 0.7) if extras else (None, None, 1.0)
                    g = gen(M, Cs, cin, 7)
                    dW0, db0 = torch.randn(nout * cin, generator=g), torch.randn(nout, generator=g)
                    dW, db = Guarded((nout * cin,), pad=8).set(dev(dW0)), Guarded((nout,), pad=8).set(dev(db0))
                    dx = Guarded((M, 1, 1, Cs), dt)
                    with options(head_bwd_blocks=blocks):
                        ops.head_bwd(c["x"], c["W"], p, c["dp"], dW.t, db.t, cin=cin, softmax2=softmax2, dx=dx.t, bn=bn,
                                     addend=add, mask=mask, mask_scale=ms)
                        dW2, db2 = Guarded((nout * cin,), pad=8).set(dev(dW0)), Guarded((nout,), pad=8).set(dev(db0))
                        ops.head_bwd(c["x"], c["W"], p, c["dp"], dW2.t, db2.t, cin=cin, softmax2=softmax2, dx=None, bn=bn,
                                     addend=add, mask=mask, mask_scale=ms)
                    what = f"M={M} cin={cin} bn={bn is not None} extras={extras}"
                    rdx, rW, rb_ = E.head_bwd(xm, c["W"], p, c["dp"], softmax2=softmax2, bn=bn, round_to=dt,
                                              addend=None if add is None else add.reshape(M, Cs),
                                              mask=None if mask is None else mask.reshape(M, Cs), mask_scale=ms)
                    adx, aW, ab = head_abs(xm, c["W"], p, c["dp"], softmax2, bn, dt, add, mask, ms)
                    elem_gate(dx.ok(), rdx, adx, dt, "dx " + what)
                    for gW, gb in ((dW, db), (dW2, db2)):
                        sum_gate(gW.ok(), rW.reshape(-1) + dW0.to(F64), aW.reshape(-1) + dW0.abs().to(F64), K, "dW " + what)
                        sum_gate(gb.ok(), rb_ + db0.to(F64), ab + db0.abs().to(F64), K, "db " + what)


@pytest.mark.parametrize("blocks", [pytest.param(None, id="blocksdefault"), pytest.param(2, id="blocks2")])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("Cs", [8, 48, 64, 512], ids=lambda c: f"Cs{c}")
def test_head_backward_fused_bn_reduce(Cs, dt, blocks):
    """adp_head_sigmoid_bwd_bnr in both head_bwd_fast settings: dx, dW, db and the fused BatchNorm-backward sums (over
    the dx it stored; f32 partials per thread and block, f64 across blocks) added into non-zero buffers, with dx
    stored and dx=None; and adp_bn_bwd_apply_head == adp_bn_bwd_apply fed that stored dx, bit for bit at every
    unroll (Cin % 8 == 0), and within the elementwise gate of the float64 reference."""
    lanes = lanes_of(Cs)
    for M in [1, 7, lanes + 1, 1000]:
        for cin in head_cins(Cs):
            c = head_case(M, Cs, cin, dt, False, 3)
            xm, bn = c["x"].reshape(M, Cs), (c["sc"], c["sh"])
            p = torch.empty(M, device=DEV)
            ops.head_fwd(c["x"], c["W"], c["b"], p, cin=cin, softmax2=False, bn=bn)
            g = gen(M, Cs, cin, 8)
            init = {"dW": torch.randn(cin, generator=g), "db": torch.randn(1, generator=g),
                    "dg": torch.randn(Cs, generator=g), "dbeta": torch.randn(Cs, generator=g)}
            rdx, rW, rb_ = E.head_bwd(xm, c["W"], p, c["dp"], softmax2=False, bn=bn, round_to=dt)
            _, aW, ab = head_abs(xm, c["W"], p, c["dp"], False, bn, dt)
            dx_first = None
            for fast in (1, 0):
                for store in (True, False):
                    o = {k: Guarded((v.numel(),), pad=8).set(dev(v)) for k, v in init.items()}
                    dx = Guarded((M, 1, 1, Cs), dt)
                    with options(head_bwd_fast=fast, head_bwd_blocks=blocks):
                        ops.head_bwd(c["x"], c["W"], p, c["dp"], o["dW"].t, o["db"].t, cin=cin, softmax2=False,
                                     dx=dx.t if store else None, bn=bn, bn_reduce=(c["mean"], c["inv"], o["dg"].t, o["dbeta"].t))
                    what = f"M={M} cin={cin} fast={fast} store={store}"
                    if store:
                        elem_gate(dx.ok(), rdx, rdx.abs(), dt, "dx " + what)
                        if dx_first is None:
                            dx_first = dx.t
                        assert torch.equal(dx.t, dx_first), "dx differs between the head_bwd_fast forms: " + what
                    else:
                        assert bool((dx.ok() == 7.0).all()), "dx=None wrote a map: " + what
                    nb = min((M + lanes - 1) // lanes, blocks or 10 ** 9)
                    K = (M + nb * lanes - 1) // (nb * lanes) + lanes
                    sum_gate(o["dW"].ok(), rW.reshape(-1) + init["dW"].to(F64), aW.reshape(-1) + init["dW"].abs().to(F64), K, "dW " + what)
                    sum_gate(o["db"].ok(), rb_ + init["db"].to(F64), ab + init["db"].abs().to(F64), K, "db " + what)
                    # the reduction over the dx the device stored (the unfused formulation's input)
                    rg, rbt = E.bn_bwd_reduce(dx_first.reshape(M, Cs), xm, *bn, c["mean"], c["inv"])
                    dabs = torch.where(E.gate(xm, *bn), host(dx_first).reshape(M, Cs).abs(), torch.zeros((), dtype=F64))
                    xh = ((host(xm) - host(c["mean"])) * host(c["inv"])).abs()
                    sum_gate(o["dg"].ok(), rg + init["dg"].to(F64), (dabs * xh).sum(0) + init["dg"].abs().to(F64), K, "dgamma " + what)
                    sum_gate(o["dbeta"].ok(), rbt + init["dbeta"].to(F64), dabs.sum(0) + init["dbeta"].abs().to(F64), K, "dbeta " + what)
            if cin % 8 == 0:
                dgam, dbet = dev(init["dg"] * math.sqrt(M)), dev(init["dbeta"] * math.sqrt(M))
                args = (c["x"], c["sc"], c["sh"], c["mean"], c["inv"], c["gamma"], dgam, dbet, float(M))
                t = E.bn_bwd_apply_terms(dx_first, *args)
                for U in (1, 2, 4):
                    with options(bn_unroll=U, bn_cap=3 if blocks else None):
                        d1, d2 = Guarded((M, 1, 1, Cs), dt), Guarded((M, 1, 1, Cs), dt)
                        ops.bn_bwd_apply(dx_first, *args, d1.t)
                        ops.bn_bwd_apply_head(c["W"], p, c["dp"], *args, d2.t, cin=cin)
                        assert torch.equal(d1.ok(), d2.ok()), f"bn_bwd_apply_head != bn_bwd_apply(stored dx): M={M} cin={cin} U={U}"
                        elem_gate(d2.t, t[0] + t[1] + t[2], t[0].abs() + t[1].abs() + t[2].abs(), dt, f"bn_bwd_apply_head M={M} U={U}")


# ------------------------------------------------------------------------------------------------- loss
LOSS_SHAPES = [(1, 1, 1), (2, 48, 37), (3, 100, 64), (1, 1500, 8), (5, 512, 8), (2, 2048, 4)]


def _loss_check(p, y, *, ohem, smooth, keep, weight, tag):
    N, H, W = p.shape
    pd, yd = dev(p), dev(y)
    rows, stats = Guarded((N * H,), pad=8), torch.zeros(8, dtype=F64, device=DEV)
    ops.loss_rows(pd, yd, rows.t, stats, smooth=smooth)
    r_ref, r_abs, s_ref = E.loss_rows(pd, yd, smooth)
    K = (W + 63) // 64
    # + 1 per pixel: log(pc + eps) and log(1 - pc + eps) see their argument rounded to f32 (|d log| <= 2^-24 each)
    sum_gate(rows.ok(), r_ref.reshape(-1), r_abs.reshape(-1) + 1.0, K, f"row_bce {tag}")
    sum_gate(stats, s_ref, s_ref.abs(), K, f"stats {tag}")   # f32 per lane and row, f64 beyond; all terms >= 0
    assert host(stats)[6].item() == s_ref[6].item() and host(stats)[7].item() == s_ref[7].item()   # counts
    k = int(np.float32(H) * np.float32(keep)) if ohem else H
    norm = float(N * max(k, 1))
    coef_t, out = Guarded((N * H,), pad=8), torch.full((1,), 0.25, dtype=F64, device=DEV)
    ops.loss_select(rows.t, coef_t.t, out, N=N, H=H, W=W, ohem=ohem, keep_ratio=keep, weight=weight, norm_rows=norm)
    kept, coef, term = E.loss_select(rows.t.reshape(N, H), W=W, ohem=ohem, keep_ratio=keep, weight=weight, norm_rows=norm)
    rc = coef_t.ok().cpu()
    assert torch.equal(rc != 0, kept.reshape(-1)), f"kept rows {tag}"
    assert bool((rc[kept.reshape(-1)] == np.float32(coef)).all()), f"row_coef is coef or 0 {tag}"
    assert abs(out.item() - 0.25 - term) <= 1e-12 * max(1.0, abs(term)), f"loss term {tag}"   # f64 from the same f32 rows
    for acc in (False, True):
        dp0 = torch.randn(N, H, W, generator=gen(N, H, W)) if acc else torch.zeros(N, H, W)
        dp = Guarded((N, H, W), pad=8).set(dev(dp0) if acc else torch.full((N, H, W), 3.0, device=DEV))
        ops.loss_grad(pd, yd, coef_t.t, stats, dp.t, weight=weight, smooth=smooth, accumulate=acc)
        t = E.loss_grad_terms(pd, yd, rc.reshape(N, H), stats, weight=weight, smooth=smooth)
        elem_gate(dp.ok(), sum(t) + dp0.to(F64), sum(x.abs() for x in t) + dp0.abs().to(F64), F32, f"loss_grad acc={acc} {tag}")
    return rows.t, rc


@pytest.mark.parametrize("smooth", [pytest.param(False, id="hard"), pytest.param(True, id="smooth")])
@pytest.mark.parametrize("ohem", [pytest.param(False, id="mean"), pytest.param(True, id="ohem")])
@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=["x".join(map(str, s)) for s in LOSS_SHAPES])
def test_loss_rows_select_grad(shape, ohem, smooth):
    """adp_loss_rows / adp_loss_select / adp_loss_grad: 5x512x8 has more than 2048 rows (the row sweep wraps), 1x1500x8
    and 2x2048x4 have H > 1024 (two sort keys per thread, H not a power of two), keep ratios 0.7 / 0.5 / 1.0 with
    k = int(f32(H) * f32(keep)), weight != 1, accumulate into a non-zero dp."""
    N, H, W = shape
    g = gen(N, H, W, 11)
    p = torch.rand(N, H, W, generator=g)
    p.reshape(-1)[:4] = torch.tensor([0.0, 1.0, 1e-9, 1 - 1e-9])[:min(4, p.numel())]   # the clip and its zero gradient
    y = (torch.rand(N, H, W, generator=g) > 0.6).float()
    for keep in ((0.7, 0.5, 1.0) if ohem else (0.7,)):
        _loss_check(p, y, ohem=ohem, smooth=smooth, keep=keep, weight=0.4, tag=f"keep={keep}")


@pytest.mark.parametrize("H", [48, 1500, 2048], ids=lambda h: f"H{h}")
def test_loss_select_ties_keep_lowest_rows(H):
    """Whole groups of identical rows: their row losses tie bit for bit, and the kept set is the lowest row indices
    among the ties (the sort's index tie-break), at H <= 1024 and H > 1024."""
    N, W, grp = 2, 8, 16
    g = gen(H, 12)
    base_p = torch.rand(N, (H + grp - 1) // grp, W, generator=g)
    base_y = (torch.rand(N, (H + grp - 1) // grp, W, generator=g) > 0.5).float()
    perm = torch.randperm(H, generator=g)   # scatter the groups' members over the image
    p = base_p.repeat_interleave(grp, dim=1)[:, :H][:, perm]
    y = base_y.repeat_interleave(grp, dim=1)[:, :H][:, perm]
    rows, rc = _loss_check(p, y, ohem=True, smooth=False, keep=0.5, weight=1.0, tag="ties")
    r = rows.cpu().reshape(N, H)
    assert all(len(torch.unique(r[n])) <= (H + grp - 1) // grp for n in range(N)), "identical rows must tie exactly"
    kept = (rc != 0).reshape(N, H)
    for n in range(N):   # within every tied value, the kept rows are a prefix by index
        for v in torch.unique(r[n]):
            idx = torch.nonzero(r[n] == v).reshape(-1)
            kk = kept[n, idx].to(torch.int64)
            assert bool((kk[:-1] >= kk[1:]).all()), f"tie at {v.item()} not broken towards the lowest index"


def test_loss_select_refuses_H_above_2048():
    rows, coef = torch.zeros(2049, device=DEV), torch.zeros(2049, device=DEV)
    out = torch.zeros(1, dtype=F64, device=DEV)
    with pytest.raises(ops.AdpError):
        ops.loss_select(rows, coef, out, N=1, H=2049, W=4, ohem=True, keep_ratio=0.7, weight=1.0, norm_rows=1434.0)
    ops.loss_select(rows[:2048], coef[:2048], out, N=1, H=2048, W=4, ohem=True, keep_ratio=0.7, weight=1.0, norm_rows=1433.0)
    torch.cuda.synchronize()
    assert out.item() == 0.0


# ------------------------------------------------------------------------------------------ flat kernels
BIG = 2 ** 21 * 8 + 8 * 37   # groups of 8 past the 8192-block x 256-thread grid: the grid-stride loop goes round again
FLAT_N = [1, 8, 255, 257, BIG]
FLAT_IDS = ["n1", "n8", "n255", "n257", "n2^24+296"]


@pytest.mark.parametrize("n", FLAT_N, ids=FLAT_IDS)
def test_adam(n):
    """adp_adam against float64 in the kernel's order of operations: grad_scale, weight decay, and steps 1, 2 and
    100000 (the bias correction is taken in double on the host: alpha(100000) = lr, alpha(1) = 0.316 * lr)."""
    g = gen(n, 13)
    hp = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7)
    combos = [(1.0, 0.0, 1), (0.125, 0.01, 2), (1.0, 0.01, 100000), (0.125, 0.0, 100000)] if n != BIG else [(0.125, 0.01, 100000)]
    w0, g0 = torch.randn(n, generator=g), torch.randn(n, generator=g) * 4
    m0, v0 = torch.randn(n, generator=g) * 0.1, torch.rand(n, generator=g) * 0.1
    for gs, wd, step in combos:
        w, m, v = (Guarded((n,), pad=8).set(dev(t)) for t in (w0, m0, v0))
        ops.adam(w.t, dev(g0), m.t, v.t, step=step, weight_decay=wd, grad_scale=gs, **hp)
        rw, rm, rv = E.adam(w0, g0, m0, v0, step=step, weight_decay=wd, grad_scale=gs, **hp)
        gi = g0.to(F64) * gs
        alpha = E.adam_alpha(hp["lr"], hp["beta1"], hp["beta2"], step)
        what = f"gs={gs} wd={wd} step={step}"
        A_m = m0.abs().to(F64) + (gi - m0).abs() * 0.1
        elem_gate(m.ok(), rm, A_m, F32, "m " + what)
        elem_gate(v.ok(), rv, v0.abs().to(F64) + (gi * gi + v0).abs() * 0.001, F32, "v " + what)
        # (A_m, not |m|: where the new m cancels, its absolute error still reaches w)
        elem_gate(w.ok(), rw, w0.abs().to(F64) * (1 + wd * hp["lr"]) + A_m * alpha / (rv.sqrt() + 1e-7), F32, "w " + what)
    if n != BIG:   # the step does count: the two alphas differ by a factor of three
        assert abs(E.adam_alpha(1e-3, 0.9, 0.999, 100000) / E.adam_alpha(1e-3, 0.9, 0.999, 1) - 10 ** 0.5) < 1e-3


@pytest.mark.parametrize("n", FLAT_N, ids=FLAT_IDS)
def test_ema_fill_vec_mul(n):
    g = gen(n, 14)
    e0, p0 = torch.randn(n, generator=g), torch.randn(n, generator=g)
    for decay in ((0.0, 0.999, 1.0) if n != BIG else (0.999,)):
        e = Guarded((n,), pad=8).set(dev(e0))
        ops.ema(e.t, dev(p0), decay)
        d = float(np.float32(decay))
        elem_gate(e.ok(), E.ema(e0, p0, decay), d * e0.abs().to(F64) + (1 - d) * p0.abs().to(F64), F32, f"ema decay={decay}")
        if decay in (0.0, 1.0):
            assert torch.equal(e.t.cpu(), p0 if decay == 0.0 else e0)
    f = Guarded((n,), pad=8)
    ops.fill(f.t, -2.5)
    assert bool((f.ok() == -2.5).all())
    o = Guarded((n,), pad=8)
    ops.vec_mul(dev(e0), dev(p0), o.t)
    equal(o.ok(), e0.to(F64) * p0.to(F64), F32, "vec_mul")   # one rounding of an exact product


@pytest.mark.parametrize("n", FLAT_N, ids=FLAT_IDS)
def test_cast_all_pairs(n):
    """adp_cast f32->bf16 (round to nearest even, as torch), bf16->f32 (exact), f32->f32 and bf16->bf16 (copies)."""
    g = gen(n, 15)
    x = torch.randn(n, generator=g) * 100
    xb = x.to(BF16)
    for src, dt in ((x, BF16), (xb, F32), (x, F32), (xb, BF16)):
        o = Guarded((n,), dt, pad=8)
        ops.cast(dev(src, src.dtype), o.t)
        assert torch.equal(o.ok().cpu(), src.to(dt)), f"{src.dtype} -> {dt}"


def test_cast_f32_to_bf16_rounding_and_specials():
    """Exact ties go to the even bf16 neighbour; +-0, +-inf and subnormals pass; the largest finite f32 lies above
    the midpoint between the largest finite bf16 and 2^128, so it rounds to +inf (as torch's conversion does)."""
    k = torch.arange(0, 64, dtype=torch.int32)
    ties = ((0x3F80 + k) << 16 | 0x8000).view(F32)          # 1.xxx exactly half way between two bf16 values
    ties = torch.cat([ties, -ties])
    fmax = torch.finfo(F32).max
    spec = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), 1e-40, -1e-40, 2.0 ** -149, 2.0 ** -126, fmax, -fmax,
                         3.3895313892515355e38, 3.3961775292304601e38])   # the largest finite bf16, and near the midpoint to 2^128
    for x in (ties, spec):
        o = Guarded((x.numel(),), BF16, pad=8)
        ops.cast(dev(x), o.t)
        got, ref = o.ok().cpu(), x.to(BF16)
        assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), (got, ref)
    up = ((0x3F80 + k + (k & 1)) << 16).view(F32)            # the even neighbour
    assert torch.equal(ties[:64].to(BF16).float(), up)
    assert spec.to(BF16)[8].item() == float("inf") and spec.to(BF16)[9].item() == float("-inf")
    assert torch.equal(spec.to(BF16)[:2].view(torch.int16), torch.tensor([0, -32768], dtype=torch.int16))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n", [8, 248, 264, BIG], ids=["n8", "n248", "n264", "n2^24+296"])
def test_add_mask_flat(n, dt):
    """adp_ew_add_mask on a flat vector of n/8 groups (dyadic values: equality)."""
    g = gen(n, 16)
    a, b, m = dyadic(g, (n,), -16, 16, 0.25), dyadic(g, (n,), -16, 16, 0.25), dyadic(g, (n,), -2, 2, 0.5)
    ad, bd, md = dev(a, dt), dev(b, dt), dev(m, dt)
    for ms in (1.0, 1.0 / 0.7):
        o = Guarded((n,), dt, pad=8)
        ops.add_mask(ad, o.t, b=bd, mask=md, mask_scale=ms)
        equal(o.ok(), E.add_mask(a, b, m, ms), dt, f"add_mask ms={ms}")
    o = Guarded((n,), dt, pad=8)
    ops.add_mask(ad, o.t)
    equal(o.ok(), a, dt, "add_mask copy")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("rows,cols,nscale", [(1, 1, 1), (3, 85, 2), (257, 1, 257), (2 ** 14 + 1, 1024 + 8, 2 ** 14)],
                         ids=["1x1", "3x85", "257x1", "16385x1032"])
def test_scale_rows(rows, cols, nscale, dt):
    """adp_scale_rows: dst = T(src * scale[r]), rows past the scale vector zero; the last case has more than 2^21
    elements. One f32 rounding of an exact product, then the store's: equality."""
    g = gen(rows, cols, 17)
    src, sc = torch.randn(rows, cols, generator=g), torch.randn(nscale, generator=g)
    o = Guarded((rows, cols), dt, pad=8)
    ops.scale_rows(dev(src), dev(sc), o.t)
    equal(o.ok(), E.scale_rows(src, sc), dt, "scale_rows")


# ----------------------------------------------------------------------------------------------- resize
# (the last: x2.5 with more than 9 source rows / columns, where a gather window in multiples of ceil(ratio) fell
#  short of the rows that weigh on a source pixel)
RESIZES = [((16, 16), (128, 128)), ((5, 9), (10, 36)), ((7, 3), (7, 3)), ((6, 10), (15, 25)), ((20, 12), (50, 30))]


@pytest.mark.parametrize("src,dst", RESIZES, ids=[f"{a[0]}x{a[1]}to{b[0]}x{b[1]}" for a, b in RESIZES])
def test_resize_bilinear(src, dst):
    """adp_resize_bilinear_fwd / _bwd at x8, non-square, identity and non-integer (x2.5) ratios; the backward is the
    adjoint: <resize(s), d> = <s, resize_bwd(d)> in float64 from the device results, to 1e-5 relative."""
    g = gen(*src, *dst, 18)
    N = 3
    s, d = torch.randn(N, *src, generator=g), torch.randn(N, *dst, generator=g)
    o, ds = Guarded((N, *dst), pad=8), Guarded((N, *src), pad=8)
    ops.resize_bilinear_fwd(dev(s), o.t)
    ops.resize_bilinear_bwd(dev(d), ds.t)
    # the source coordinate is an f32 expression of two roundings at magnitude <= n_in, so each lerp weight is off
    # by <= 2 * 2^-24 * n_in; its effect is bounded by the corners it weighs (indicator matrices below)
    iy, ix = (E.bilinear_matrix(src[0], dst[0]) > 0).to(F64), (E.bilinear_matrix(src[1], dst[1]) > 0).to(F64)
    dcoord = 2 * U24 * (src[0] + src[1])
    # forward: three lerps of four corners; |terms| <= the same interpolation of |s|, three times over
    elem_gate(o.ok(), E.resize_bilinear_fwd(s, *dst), 3 * E.resize_bilinear_fwd(s.abs(), *dst), F32, "forward",
              extra=dcoord * torch.einsum("oh,nhw,pw->nop", iy, s.abs().to(F64), ix))
    # backward: an fma chain over the window's columns, then over its rows
    fy, fx = -(-dst[0] // src[0]), -(-dst[1] // src[1])
    K = 5 * fy + 5 * fx + 2
    sum_gate(ds.ok(), E.resize_bilinear_bwd(d, *src), E.resize_bilinear_bwd(d.abs(), *src)
             + dcoord / ((K + 8) * U24) * torch.einsum("oh,nop,pw->nhw", iy, d.abs().to(F64), ix), K, "backward")
    sp, dpos = torch.rand(N, *src, generator=g) + 0.5, torch.rand(N, *dst, generator=g) + 0.5   # no cancellation
    o2, ds2 = torch.empty(N, *dst, device=DEV), torch.empty(N, *src, device=DEV)
    ops.resize_bilinear_fwd(dev(sp), o2)
    ops.resize_bilinear_bwd(dev(dpos), ds2)
    lhs, rhs = (host(o2) * dpos.to(F64)).sum().item(), (sp.to(F64) * host(ds2)).sum().item()
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs), (lhs, rhs)


# --------------------------------------------------------------------------------------- argument errors
def test_argument_errors_are_refused_before_any_launch():
    """Each of these returns from the entry point's argument check (no launch); the next valid call succeeds."""
    v = lambda c: torch.ones(c, device=DEV)   # noqa: E731

    def valid():
        z, out = torch.ones(4, 8, device=DEV), torch.zeros(4, 8, device=DEV)
        ops.bn_apply(z, v(8), v(8), out)
        torch.cuda.synchronize()
        assert bool((out == 2.0).all())

    z12 = torch.ones(4, 12, device=DEV)
    z2056 = torch.ones(2, 2056, device=DEV)
    bad = [
        lambda: ops.bn_apply(z12, v(12), v(12), torch.zeros_like(z12)),                          # C % 8 != 0
        lambda: ops.bn_apply(z2056, v(2056), v(2056), torch.zeros_like(z2056)),                  # C > 2048
        lambda: ops.bn_bwd_apply(z2056, z2056, *(v(2056),) * 7, 2.0, torch.zeros_like(z2056)),   # C > 2048
        lambda: ops.bn_bwd_reduce(z12, z12, *(v(12),) * 6),                                      # C % 8 != 0
        lambda: ops.maxpool2_fwd(torch.ones(1, 3, 4, 8, device=DEV), torch.zeros(1, 1, 2, 8, device=DEV)),   # odd H
        lambda: ops.maxpool2_bwd(torch.ones(1, 4, 3, 8, device=DEV), torch.ones(1, 2, 1, 8, device=DEV),
                                 torch.zeros(1, 4, 3, 8, device=DEV)),                           # odd W
        lambda: ops.bn_finalize(0, v(8), v(8), v(8), v(8), 1e-3, 0.1, v(8), v(8), v(8), v(8)),   # count == 0
        lambda: ops.bn_bwd_apply(torch.ones(4, 8, device=DEV), torch.ones(4, 8, device=DEV), *(v(8),) * 7, 0.0,
                                 torch.zeros(4, 8, device=DEV)),                                 # count == 0
        lambda: ops.head_bwd(torch.ones(2, 1, 1, 1024, device=DEV), v(1024), v(2), v(2), v(1024), v(1), cin=1024,
                             softmax2=False, bn=(v(1024), v(1024)),
                             bn_reduce=(v(1024), v(1024), v(1024), v(1024))),                    # Cs + Cin + 1 > 2048
    ]
    for i, f in enumerate(bad):
        with pytest.raises(ops.AdpError):
            f()
        valid()
