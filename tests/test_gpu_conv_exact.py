"""The convolution kernels against float64, bit for bit (oracle/conv_ref.py).

Operands are small integers (exact in bf16), so every product and every partial sum of a launch is an integer
below 2^24: the f32 accumulators of the bf16 and f32 MFMA paths, split-K partials, weight-gradient slabs and f32
atomics hold the exact result in ANY summation order, and the only rounding left is the store, which the reference
performs itself. Every dispatch form is therefore held to float64 with torch.equal, no tolerance:

  wide regime    activations / gradients in [-8, 8], dense weights in [-4, 4]: outputs reach a few thousand, so
                 the bf16 store rounds a third to a half of them (round to nearest even, every K element counts);
  narrow regime  activations in [-2, 2], weights in {-1, 0, 1} with one in four non-zero: the sum of v^2 over all
                 pixels stays below 2^24, so the fused BatchNorm statistics are exact too.

The reference asserts the exactness condition of every case (each sum of |terms| below 2^24 on the operands'
grid). Every output buffer is filled with a sentinel first: the columns from Nout to the channel stride, the
pixels behind the tensor, the pad rows and columns of dW and the tails of the per-channel vectors must keep it.
Every case asserts the kernel the launch reports (adp_last_kernel), so no case can silently run another form; a
row's options come from the test of tests/test_gpu_ops.py that forces the same form. tests/test_conv_ref.py
holds the reference to float64 autograd and checks that every kernel family owns a row of CASES.
"""
import contextlib
import functools
import zlib

import pytest
import torch

from oracle import conv_ref as CR

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7.0          # sentinel of the activation-typed and per-channel buffers (exact in bf16)
WSENT = 12345.0      # sentinel of the pad rows / columns of dW
DT = {"bf16": torch.bfloat16, "f32": torch.float32}
DROP_SEED = 20261
BOTH = ("bf16", "f32")

# families without a row, with the reason
_REG = ("register-staged bf16 kernel: launched only under option conv_fast = 1 or for a "
        "BatchNorm-on-load source without act_out, which neither the networks nor any test of the suite do; a row "
        "here would be the first launch of an option combination nothing else runs")
EXCLUDED = {
    "fwd_halop_f8": "fp8 forward: tests/test_gpu_fp8.py holds it to 1e-3 absolute against the dequantised operands",
    "fwd_bf16": _REG,
    "wgrad_bf16": _REG,
}

CASES = []


def round_up(x, m):
    return (x + m - 1) // m * m


def case(id, family, kernel, kind, shape, parts, nout, epi=(), *, dts=("bf16",), regime="wide", opts=None,
         kfields=None, **geom):
    """One row. family: the kernel family the row covers (per dtype when a dict). kind: fwd | dgrad | convt_dgrad | wgrad. shape: (N, H, W) of the sources. parts: channel strides of
    the sources. epi: epilogue / variant tokens. geom: the keyword arguments of the gather (dil, up, kh, kw, pad,
    stride, Ho, Wo) plus split / cps / real. kernel: the expected adp_last_kernel prefix (per dtype when a dict);
    kfields: {index: text} of its comma-separated template arguments."""
    CASES.append(dict(id=id, family=family, kernel=kernel, kind=kind, shape=tuple(shape), parts=tuple(parts),
                      nout=nout, epi=tuple(epi), dts=tuple(dts), regime=regime, opts=dict(opts or {}),
                      kfields=dict(kfields or {}), geom=dict(geom)))


# ------------------------------------------------------------------------------------------------ the case table
# generic forward (conv_igemm.hip): channel strides that are no multiple of 64 (test_conv_fwd CONV_CASES)
GEN_F = {"bf16": "fwd_glds", "f32": "fwd_generic"}   # (f32 at these strides: the generic kernel, igemm_fwd_kernel<float>)
GEN_K = {"bf16": "igemm_fwd_glds_kernel<128, 128>", "f32": "igemm_fwd_kernel<float>"}
GEN_K64 = {"bf16": "igemm_fwd_glds_kernel<256, 64>", "f32": "igemm_fwd_kernel<float>"}
case("gen_dil2", GEN_F, GEN_K, "fwd", (2, 16, 16), [48], 88, ("bias", "relu"), dts=BOTH, dil=2)
case("gen_dil2_stats", GEN_F, GEN_K, "fwd", (2, 16, 16), [48], 88, ("bias", "stats", "acc0"), dts=BOTH,
     regime="narrow", dil=2)
case("gen_up", GEN_F, GEN_K64, "fwd", (2, 8, 8), [88], 48, ("bias", "relu"), dts=BOTH, up=True)
case("gen_concat", GEN_F, GEN_K64, "fwd", (2, 16, 16), [48, 48], 48, ("bias", "relu"), dts=BOTH)
case("gen_drop_accum", GEN_F, GEN_K, "fwd", (2, 16, 16), [48], 88, ("bias", "relu", "drop", "accum"), dts=BOTH)
case("gen_mask_add", GEN_F, GEN_K, "fwd", (2, 16, 16), [48], 88, ("add", "mask"), dts=BOTH)
case("gen_dgrad_dil2", GEN_F, GEN_K64, "dgrad", (2, 16, 16), [88], 48, ("add", "mask"), dts=BOTH, dil=2)
# dilation 32 on a 16 x 16 image: every tap but the centre lies outside (64-channel stride: the tap64 kernel)
case("dil32_centre_only", "fwd_tap64", {"bf16": "igemm_fwd_tap64_kernel<4, 1, 64,", "f32": "igemm_fwd_tap64_kernel<4, 1, 64,"},
     "fwd", (1, 16, 16), [64], 64, ("bias", "relu"), dts=BOTH, dil=32)

# input layer (test_cin8_pipelined_matches_plain, test_cin8_f32_input_layer)
for pf, fam, kn in ((0, "fwd_cin8", "igemm_fwd_cin8_kernel<"), (1, "fwd_cin8p", "igemm_fwd_cin8p_kernel<")):
    case(f"cin8_pf{pf}_ragged_dil2", fam, kn, "fwd", (1, 13, 13), [8], 64, ("bias", "stats"), opts=dict(cin8_pf=pf), dil=2)
    case(f"cin8_pf{pf}_n24", fam, kn, "fwd", (3, 10, 10), [8], 24, ("bias", "relu", "stats", "acc0"), opts=dict(cin8_pf=pf))
    case(f"cin8_pf{pf}_32", fam, kn, "fwd", (2, 32, 32), [8], 64, ("bias", "relu", "stats"), regime="narrow",
         opts=dict(cin8_pf=pf))
case("cin8_narrow_store", "fwd_cin8", "igemm_fwd_cin8_kernel<", "fwd", (2, 32, 32), [8], 64, ("bias", "relu"),
     opts=dict(cin8_pf=0, cin8_wide=0))
case("cin8_f32_ragged_dil2", "fwd_cin8_f32", "igemm_fwd_cin8_f32_kernel<2, 4>", "fwd", (1, 13, 13), [8], 64,
     ("bias", "relu", "stats"), dts=("f32",), dil=2)
case("cin8_f32_n24", "fwd_cin8_f32", "igemm_fwd_cin8_f32_kernel<2, 4>", "fwd", (3, 10, 10), [8], 24,
     ("bias", "stats", "acc0"), dts=("f32",))
case("cin8_f32_real3", "fwd_cin8_f32", "igemm_fwd_cin8_f32_kernel<1, 4>", "fwd", (2, 32, 32), [8], 64,
     ("bias", "relu", "stats"), dts=("f32",), regime="narrow", real=(3, 0, 64))

# tap64, non-persistent (test_tap64_configs, test_tap64_kpipe_matches, test_tap64_split_k, test_tap64_bnr_lds_epilogue,
# test_tap64_mask_lds_epilogue): M = 529 with ragged M and N, M = 512 two full tiles, M = 35 less than a tile
T64_TILE = {2: "2, 4, 128", 3: "4, 2, 64", 4: "4, 1, 128", 5: "4, 1, 64"}
for cfg in (2, 3, 4, 5):
    o = dict(fwd_tap64=cfg, tap64_persist=0)
    kn = {"bf16": f"igemm_fwd_tap64_kernel<{T64_TILE[cfg]},", "f32": f"igemm_fwd_tap64_kernel<{T64_TILE[max(cfg, 3)]},"}
    case(f"tap64_cfg{cfg}_m529", "fwd_tap64", kn, "fwd", (1, 23, 23), [128], 192, ("bias", "relu"),
         dts=BOTH if cfg in (3, 5) else ("bf16",), opts=o)
    case(f"tap64_cfg{cfg}_m529_stats", "fwd_tap64", kn, "fwd", (1, 23, 23), [128], 192, ("bias", "relu", "stats"),
         dts=BOTH if cfg in (3, 5) else ("bf16",), regime="narrow", opts=o)
case("tap64_kpipe_m529", "fwd_tap64", "igemm_fwd_tap64_kernel<2, 4, 128,", "fwd", (1, 23, 23), [128], 192,
     ("bias", "relu", "stats"), regime="narrow", opts=dict(fwd_tap64=2, tap64_persist=0, fwd_halo=0, tap64_kpipe=1),
     kfields={7: "1"})
for dil in (1, 2, 8):
    case(f"tap64_m512_dil{dil}", "fwd_tap64", "igemm_fwd_tap64_kernel<", "fwd", (2, 16, 16), [64], 64,
         ("bias", "relu", "stats", "acc0"), dts=BOTH, regime="narrow", opts=dict(fwd_halo=0, tap64_persist=0), dil=dil)
case("tap64_m35", "fwd_tap64", "igemm_fwd_tap64_kernel<", "fwd", (1, 5, 7), [64], 64, ("bias", "relu"), dts=BOTH,
     opts=dict(fwd_halo=0, tap64_persist=0))
case("tap64_m35_fold", "fwd_tap64", "igemm_fwd_tap64_kernel<", "fwd", (1, 4, 8), [64], 64, ("bias", "stats", "fold"),
     regime="narrow", opts=dict(fwd_halo=0, tap64_persist=0))
case("tap64_drop", "fwd_tap64", "igemm_fwd_tap64_kernel<", "fwd", (1, 23, 23), [128], 192, ("bias", "relu", "drop"),
     dts=BOTH)
case("tap64_accum", "fwd_tap64", "igemm_fwd_tap64_kernel<", "fwd", (2, 16, 16), [64], 64, ("accum",), dts=BOTH,
     opts=dict(fwd_halo=0))
for lds in (0, 1):
    case(f"tap64_bnr_lds{lds}", "fwd_tap64", "igemm_fwd_tap64_kernel<2, 4, 128, true, true,", "dgrad", (1, 24, 40), [256],
         192, ("bnr", "acc0"), regime="narrow", opts=dict(tap64_bnr_lds=lds, fwd_tap64=2, fwd_halo=0))
    case(f"tap64_mask_lds{lds}", "fwd_tap64", "igemm_fwd_tap64_kernel<", "fwd", (1, 24, 40), [128], 96,
         ("mask", "stats"), regime="narrow", opts=dict(tap64_mask_lds=lds, fwd_halo=0, tap64_persist=0))
    case(f"tap64_mask_add_lds{lds}", "fwd_tap64", "igemm_fwd_tap64_kernel<", "fwd", (2, 32, 32), [192], 192,
         ("mask", "add"), opts=dict(tap64_mask_lds=lds, fwd_halo=0, tap64_persist=0))
    case(f"tap64_f32_mask_add_lds{lds}", "fwd_tap64", "igemm_fwd_tap64_kernel<", "fwd", (1, 24, 40), [96], 96,
         ("mask", "add", "stats"), dts=("f32",), regime="narrow", opts=dict(tap64_mask_lds=lds, fwd_halo=0, tap64_persist=0))
for epi in (("bias", "relu"), ("bias", "stats"), ("accum",), ("mask", "add")):
    case("tap64_splitk_" + "_".join(epi), "fwd_tap64", "igemm_fwd_tap64_kernel<", "fwd", (2, 32, 32), [384], 384, epi,
         regime="narrow" if "stats" in epi else "wide", opts=dict(tap64_ksplit=1), kfields={"ksplit": 2})
case("tap64_splitk_f32", "fwd_tap64", "igemm_fwd_tap64_kernel<", "fwd", (2, 32, 32), [352], 352, ("bias", "relu"),
     dts=("f32",), opts=dict(tap64_ksplit=1), kfields={"ksplit": 2})
case("tap64_splitk_bnr", "fwd_tap64", "igemm_fwd_tap64_kernel<", "dgrad", (2, 32, 32), [384], 384, ("bnr",),
     regime="narrow", opts=dict(tap64_ksplit=1), kfields={"ksplit": 2})

# tap64p, persistent (test_tap64p_halo_matches): the whole product gathered / halo x tile x grid x store width x
# claiming of that test, each in both regimes (wide: the store's rounding; narrow: statistics added into non-zero
# sums). The loops keep the rows of one data key together, so the cached reference serves its 54 option rows.
P_MODES = {"plain": ([128], 320, 192), "one_chunk": ([64], 256, 128), "concat": ([64, 128], 256, 128),
           "split": ([128, 64], 256, 256)}
P_AXES = [(None, 1, 0), (3, 0, 1), (7, 2, 2), (3, 2, 0), (7, 1, 1), (None, 0, 2), (3, 1, 2), (7, 0, 0), (None, 2, 1)]


def tap64p_halo_row(tag, shape, parts, nout, tile, split, stats, halo, grid, wide, claim):
    o = dict(fwd_tap64=2 if tile == 256 else 3, fwd_halo=0, tap64p_halo=halo, fwd_w4=0, tap64p_wide=wide,
             tap64p_claim=min(claim, 1), claim_full=1 if claim == 2 else 0)
    if grid:
        o["tap64_persist_grid"] = grid
    kn = "igemm_fwd_tap64p_kernel<256, %d, %d, false, %s, false" % (tile, 2 if tile == 256 else 3,
                                                                  "true" if halo else "false")
    epi = ("bias",) + (("split",) if split else ("relu",)) + (("stats", "acc0") if stats else ())
    case(f"tap64p_{tag}_{'stats' if stats else 'wide'}_halo{halo}_t{tile}_g{grid}_w{wide}_c{claim}", "fwd_tap64p", kn, "fwd",
         shape, parts, nout, epi, regime="narrow" if stats else "wide", opts=o, split=split)


for mode, (parts, n256, n128) in P_MODES.items():
    for tile in (256, 128):
        for stats in (0, 1):
            for halo in (1, 0):
                for grid in (None, 3, 7):
                    for wide in (0, 1, 2):
                        for claim in (0, 1, 2):
                            tap64p_halo_row(mode, (2, 32, 64), parts, n256 if tile == 256 else n128, tile,
                                            128 if mode == "split" else 0, stats, halo, grid, wide, claim)
# (1, 16, 64), 64 -> 128: four 256-row tiles, fewer than a chip-sized grid; on 3 blocks one block walks two tiles, on 7
# the grid is cut to the tile count
for stats in (0, 1):
    for halo in (1, 0):
        for grid in (None, 3, 7):
            for wide, claim in ((2, 0), (0, 1), (1, 2)):
                tap64p_halo_row("small", (1, 16, 64), [64], 128, 128, 0, stats, halo, grid, wide, claim)
case("tap64p_fold", "fwd_tap64p", "igemm_fwd_tap64p_kernel<256, 256, 2, false, true, false", "fwd", (2, 32, 64), [64], 256,
     ("bias", "stats", "fold"), regime="narrow", opts=dict(fwd_tap64=2, fwd_halo=0, fwd_w4=0))
for mode in ("one_chunk", "concat"):   # test_tap64p_wreg_matches_dma
    case(f"tap64p_wreg_{mode}", "fwd_tap64p", "igemm_fwd_tap64p_kernel<256, 256, 2, false, true, false, true, false, -1>",
         "fwd", (2, 32, 64), P_MODES[mode][0], 256, ("bias", "relu", "stats"), regime="narrow",
         opts=dict(fwd_tap64=2, fwd_halo=0, fwd_w4=0, tap64p_wreg=1, tap64_persist_grid=3))
# test_upsample_gather_halo_forms
case("tap64p_up_256", "fwd_tap64p", "igemm_fwd_tap64p_kernel<256, 256, 2, false, true, false", "fwd", (2, 16, 32), [128],
     256, ("bias", "relu", "stats"), regime="narrow", opts=dict(fwd_halo=0, fwd_tap64=2, fwd_w4=0, tap64_persist_grid=3),
     up=True)
case("tap64p_up_128", "fwd_tap64p", "igemm_fwd_tap64p_kernel<256, 128, 3, false, true, false, false", "fwd", (2, 16, 32),
     [192], 128, ("bias", "relu"), opts=dict(fwd_halo=0, fwd_tap64=3, fwd_w4=0), up=True)
# test_tap64_persistent_matches: the gather forms in the three tile / ring shapes
P_CFG = {1: "256, 256, 2", 2: "256, 128, 3", 3: "128, 256, 3"}
for cfg in (1, 2, 3):
    grid, wide, claim = P_AXES[cfg]
    o = dict(tap64_persist=1, fwd_tap64=2, tap64p_cfg=cfg, tap64p_wide=min(wide, 1), tap64p_claim=min(claim, 1))
    if grid:
        o["tap64_persist_grid"] = grid
    kn = f"igemm_fwd_tap64p_kernel<{P_CFG[cfg]}, false, false"
    case(f"tap64p_gather_cfg{cfg}", "fwd_tap64p", kn, "fwd", (2, 23, 23), [128], 320, ("bias", "relu", "stats"),
         regime="narrow", opts=o)
    case(f"tap64p_dilated_cfg{cfg}", "fwd_tap64p", kn, "fwd", (2, 23, 23), [128], 320, ("bias", "relu"), opts=o, dil=4, pad=4)
    case(f"tap64p_bnr_cfg{cfg}", "fwd_tap64p", f"igemm_fwd_tap64p_kernel<{P_CFG[cfg]}, true, false", "dgrad", (2, 23, 23),
         [128], 320, ("bnr",), regime="narrow", opts=o)
    case(f"tap64p_convt_shuffle_cfg{cfg}", "fwd_tap64p", kn, "fwd", (2, 19, 19), [128], 256, ("bias", "stats", "shuffle"),
         regime="narrow", opts=o, kh=1, kw=1, pad=0, cps=64)
    case(f"tap64p_convt_shuffle_wide_cfg{cfg}", "fwd_tap64p", kn, "fwd", (2, 19, 19), [128], 256, ("bias", "shuffle"),
         opts=o, kh=1, kw=1, pad=0, cps=64)
    case(f"tap64p_convt_dgrad_cfg{cfg}", "fwd_tap64p", kn, "convt_dgrad", (2, 21, 21), [64], 256, (), opts=o, cps=64)

# w4 (test_fwd_w4_matches W4_CASES)
for grid in (None, 3):
    o = dict(fwd_tap64=2, fwd_halo=0, fwd_w4=1)
    if grid:
        o.update(tap64_persist_grid=grid, fwd_w4_grid=grid)
    case(f"w4_one_chunk_stats_g{grid}", "fwd_w4", "igemm_fwd_w4_kernel<true", "fwd", (2, 32, 64), [64], 256,
         ("stats",) + (("acc0",) if grid else ()), regime="narrow", opts=o)
    case(f"w4_concat_relu_g{grid}", "fwd_w4", "igemm_fwd_w4_kernel<false", "fwd", (2, 32, 64), [64, 128], 256,
         ("bias", "relu"), opts=o)
    case(f"w4_up2_concat_stats_g{grid}", "fwd_w4", "igemm_fwd_w4_kernel<true", "fwd", (2, 16, 32), [128, 128], 256,
         ("stats",), regime="narrow", opts=o, up=True)

# halo (option halo_persist = 0) and halop: (2, 8, 32) one patch per image, every side a border; (1, 16, 64) patch
# seams in both directions; (2, 32, 64) on a 3-block grid; one / two chunks; epilogues 0-6
H_SHAPES = {"1patch": (2, 8, 32), "seams": (1, 16, 64)}
H_EPIS = {"plain": ((), "wide"), "stats": (("bias", "stats"), "narrow"), "relu": (("bias", "relu"), "wide"),
          "relu_stats": (("bias", "relu", "stats", "acc0"), "narrow"), "mask_add": (("mask", "add"), "wide"),
          "drop": (("bias", "relu", "drop"), "wide")}
H_EPI_IDX = {"plain": "0", "stats": "1", "relu": "2", "relu_stats": "3", "mask_add": "4", "drop": "5"}
for sname, shp in H_SHAPES.items():
    for parts, nout in (([64], 64), ([128], 128), ([64, 64], 64), ([64], 40), ([64], 128)):
        tag = f"{'x'.join(map(str, parts))}_{nout}_{sname}"
        for ename, (epi, reg) in H_EPIS.items():
            if sname == "1patch" and ename in ("plain", "relu_stats"):
                continue
            if nout == 40 and ename not in ("stats", "relu"):
                continue
            case(f"halop_{tag}_{ename}", "fwd_halop", "igemm_fwd_halop_kernel<false", "fwd", shp, parts, nout, epi,
                 regime=reg, kfields={4: H_EPI_IDX[ename]})
            if sname == "seams" and ename in ("stats", "relu", "mask_add", "drop"):
                case(f"halo_{tag}_{ename}", "fwd_halo", "igemm_fwd_halo_kernel<", "fwd", shp, parts, nout, epi, regime=reg,
                     opts=dict(halo_persist=0))
case("halop_split_stats", "fwd_halop", "igemm_fwd_halop_kernel<false, 1, 64", "fwd", (1, 16, 64), [64], 128,
     ("bias", "stats", "split"), regime="narrow", split=64)
case("halop_split_masks", "fwd_halop", "igemm_fwd_halop_kernel<false, 1, 64", "fwd", (1, 16, 64), [64], 128,
     ("mask", "mask2", "split"), split=64, kfields={4: "4"})
case("halop_2ch_split_relu", "fwd_halop", "igemm_fwd_halop_kernel<false, 2, 32", "fwd", (2, 8, 32), [64, 64], 128,
     ("bias", "relu", "split"), split=64)
case("halo_split_relu", "fwd_halo", "igemm_fwd_halo_kernel<", "fwd", (1, 16, 64), [64], 128, ("bias", "relu", "split"),
     split=64, opts=dict(halo_persist=0))
for parts, nout in (([64], 64), ([128], 64), ([64, 64], 128)):
    tag = f"{'x'.join(map(str, parts))}_{nout}"
    if len(parts) == 1:   # (the data gradient of the layer: dY has its Nout channels, the launch its Cin columns)
        case(f"halop_bnr_{tag}", "fwd_halop", "igemm_fwd_halop_kernel<true", "dgrad", (1, 16, 64), [nout], sum(parts),
             ("bnr", "acc0"), regime="narrow")
    case(f"halop_g3_{tag}_stats", "fwd_halop", "igemm_fwd_halop_kernel<false", "fwd", (2, 32, 64), parts, nout,
         ("bias", "stats"), regime="narrow", opts=dict(halo_persist_grid=3))
    case(f"halop_g3_{tag}_relu", "fwd_halop", "igemm_fwd_halop_kernel<false", "fwd", (2, 32, 64), parts, nout,
         ("bias", "relu"), opts=dict(halo_persist_grid=3))
    # test_halop_pipelined_epilogue_matches / test_halop_swp_matches / test_halop_wide_store_matches / claimed
    case(f"halop_pipe2_{tag}", "fwd_halop", "igemm_fwd_halop_kernel<false", "fwd", (2, 32, 64), parts, nout,
         ("bias", "stats"), regime="narrow", opts=dict(halop_pipe=2, halop_swp=0, halo_persist_grid=3), kfields={3: "true"})
    case(f"halop_swp1_{tag}", "fwd_halop", "igemm_fwd_halop_kernel<false", "fwd", (2, 32, 64), parts, nout,
         ("bias", "relu"), opts=dict(halop_swp=1, halo_persist_grid=3), kfields={7: "true"})
    for wide in (0, 2):
        case(f"halop_wide{wide}_{tag}", "fwd_halop", "igemm_fwd_halop_kernel<false", "fwd", (2, 32, 64), parts, nout,
             ("bias", "relu", "stats"), regime="narrow", opts=dict(halop_wide=wide),
             kfields={5: "true" if wide else "false"})
    case(f"halop_claim_{tag}", "fwd_halop", "igemm_fwd_halop_kernel<false", "fwd", (2, 32, 64), parts, nout,
         ("bias", "relu"), opts=dict(halop_claim=1, halo_persist_grid=7), kfields={6: "true"})
case("halo_bnr_64", "fwd_halo", "igemm_fwd_halo_kernel<", "dgrad", (1, 16, 64), [64], 64, ("bnr",), regime="narrow",
     opts=dict(halo_persist=0), kfields={4: "true"})
case("halo_bnr_mask_add", "fwd_halo", "igemm_fwd_halo_kernel<", "dgrad", (1, 16, 64), [128], 64,
     ("bnr", "mask", "add"), regime="narrow", kfields={4: "true"})
case("halop_fold", "fwd_halop", "igemm_fwd_halop_kernel<false", "fwd", (1, 16, 64), [64], 64, ("bias", "stats", "fold"),
     regime="narrow")
case("halop_up_1ch", "fwd_halop", "igemm_fwd_halop_kernel<false, 1, 64", "fwd", (2, 16, 32), [64], 64,
     ("bias", "relu", "stats"), regime="narrow", opts=dict(halo_persist_grid=3), up=True)
case("halop_up_2ch", "fwd_halop", "igemm_fwd_halop_kernel<false, 2, 32", "fwd", (2, 16, 32), [128], 64, ("bias", "relu"),
     up=True)
# BatchNorm on load with the activation stored too (test_conv_bn_on_load_with_act_out): EPI 6, and the two-launch form
case("halop_bnload_64", "fwd_halop", "igemm_fwd_halop_kernel<false, 1, 64, true, 6", "fwd", (1, 16, 64), [64], 64,
     ("bnload", "stats"), regime="narrow")
case("halop_bnload_64_g3", "fwd_halop", "igemm_fwd_halop_kernel<false, 1, 64, true, 6", "fwd", (1, 32, 64), [64], 64,
     ("bnload", "stats", "acc0"), regime="narrow", opts=dict(halo_persist_grid=3))
case("bnload_two_launch_128", "fwd_halop", "igemm_fwd_halop_kernel<false, 2, 32", "fwd", (1, 16, 64), [128], 128,
     ("bnload", "stats"), regime="narrow")

# f32 forward: zero tails (test_f32_zero_tail_forms ZTAIL_CASES), column skip, the persistent f32 halo form
for name, reals, nout, nreal, up, epi, zt in (("1src_both", [44], 64, 44, False, ("bias", "relu", "stats"), 3),
                                              ("2src_both_mask_add", [44, 44], 64, 44, False, ("mask", "add"), 3),
                                              ("1src_ntail", [64], 64, 44, False, ("bias", "relu", "stats"), 2),
                                              ("1src_up2_both", [44], 64, 44, True, ("bias", "relu", "stats"), 3),
                                              ("1src_ktail_n128", [44], 128, 0, False, ("bias", "relu", "stats"), 1)):
    shp = (2, 6, 10) if up else (2, 12, 20)
    case(f"f32_ztail_{name}", "fwd_tap64", f"igemm_fwd_tap64_kernel<4, {nout // 64}, 64,", "fwd", shp, [64] * len(reals),
         nout, epi, dts=("f32",), regime="narrow" if "stats" in epi else "wide",
         opts=dict(fwd_halo=0, tap64_persist=0, tap64p_f32=0, fwd_tap64=3 if nout == 128 else 1), kfields={7: str(zt + 3)},
         up=up, real=(reals[0], reals[1] if len(reals) > 1 else 0, nreal))
for nout in (96, 352):
    for skip in (1, 0):
        case(f"f32_skip{skip}_n{nout}_tap64p", "fwd_tap64p", "igemm_fwd_tap64p_kernel<256, 128, 3", "fwd", (1, 16, 64), [96],
             nout, ("bias", "relu", "stats"), dts=("f32",), regime="narrow",
             opts=dict(f32_skip=skip, tap64p_f32=1, fwd_tap64=3))
        case(f"f32_skip{skip}_n{nout}_tap64", "fwd_tap64", "igemm_fwd_tap64_kernel<4, 2, 64", "fwd", (1, 16, 64), [96],
             nout, ("bias", "relu"), dts=("f32",), opts=dict(f32_skip=skip, tap64p_f32=0, fwd_tap64=3))
F32P = "igemm_fwd_tap64p_kernel<256, 128, 3, false, true, false, false, true, -1>"
for i, (mode, parts, nout, up, split) in enumerate((("plain", [96], 96, False, 0), ("concat", [64, 128], 192, False, 0),
                                                     ("up", [192], 96, True, 0), ("split", [96, 96], 192, False, 96),
                                                     ("n352", [352], 352, False, 0))):
    grid, _, claim = P_AXES[i]
    o = dict(tap64p_f32=1, tap64p_claim=min(claim, 1), fwd_tap64=3)
    if grid:
        o["tap64_persist_grid"] = grid
    shp = (1, 8, 32) if up else (1, 16, 64)
    epi = ("bias", "stats") + (("split",) if split else ("relu",))
    case(f"f32_tap64p_{mode}", "fwd_tap64p", F32P, "fwd", shp, parts, nout, epi, dts=("f32",), regime="narrow", opts=o,
         up=up, split=split)
    case(f"f32_tap64p_{mode}_wide", "fwd_tap64p", F32P, "fwd", shp, parts, nout, epi[:1] + epi[2:], dts=("f32",), opts=o,
         up=up, split=split)

# data gradients through the packers (pack_weights mode 1 / 2), f32
case("dgrad_f32_tap64", "fwd_tap64", "igemm_fwd_tap64_kernel<", "dgrad", (2, 16, 16), [64], 64, ("add", "mask"),
     dts=("f32",), dil=2)
case("convt_dgrad_f32", "fwd_tap64", "igemm_fwd_tap64_kernel<", "convt_dgrad", (2, 8, 8), [64], 128, (), dts=("f32",),
     cps=64)
case("convt_shuffle_f32", "fwd_tap64", "igemm_fwd_tap64_kernel<", "fwd", (2, 8, 8), [128], 256, ("bias", "shuffle"),
     dts=("f32",), kh=1, kw=1, pad=0, cps=64)

# weight gradient, bf16
case("wg_glds", "wgrad_glds", "igemm_wgrad_glds_kernel<128, 128>", "wgrad", (2, 16, 16), [48], 88, ("dB",), dil=2)
case("wg_glds_acc0", "wgrad_glds", "igemm_wgrad_glds_kernel<64, 256>", "wgrad", (2, 16, 16), [48, 48], 48, ("dB", "acc0"))
case("wg_glds_bna_two_launch", "wgrad_glds", "igemm_wgrad_glds_kernel<128, 128>", "wgrad", (2, 16, 16), [48], 88, ("bna", "dB"))
case("wg_glds_up", "wgrad_glds", "igemm_wgrad_glds_kernel<64, 256>", "wgrad", (2, 8, 8), [88], 48, ("dB",), up=True)
WT_TILE = {2: "2, 4, 128", 3: "2, 4, 64", 4: "1, 4, 64"}
for cfg in (2, 3, 4):   # test_wgrad_tap64_configs: ragged M, and row-aligned images (the stage-origin gather path)
    for nout in (64, 192):
        case(f"wg_tap64_cfg{cfg}_ragged_n{nout}", "wgrad_tap64", f"igemm_wgrad_tap64_kernel<{WT_TILE[cfg]}, false, false>",
             "wgrad", (2, 23, 23), [128], nout, ("dB",) + (("acc0",) if nout == 64 else ()), opts=dict(wgrad_tap64=cfg))
    case(f"wg_tap64_cfg{cfg}_rowaligned", "wgrad_tap64", f"igemm_wgrad_tap64_kernel<{WT_TILE[cfg]}, false, true>", "wgrad",
         (1, 16, 64), [128], 64, ("dB",), opts=dict(wgrad_tap64=cfg, wgrad_halop=0))
case("wg_tap64_defer", "wgrad_tap64", "igemm_wgrad_tap64_kernel<", "wgrad", (2, 32, 64), [64], 64, ("dB", "defer", "acc0"),
     opts=dict(wgrad_halop=0))
case("wg_tap64_convt", "wgrad_tap64", "igemm_wgrad_tap64_kernel<", "wgrad", (2, 8, 8), [128], 256, ("dB", "shuffle"),
     kh=1, kw=1, pad=0, cps=64)
case("wg_cin8", "wgrad_cin8", "igemm_wgrad_cin8_kernel<false>", "wgrad", (3, 8, 32), [8], 64, ("dB",))
case("wg_cin8_acc0_g5", "wgrad_cin8", "igemm_wgrad_cin8_kernel<false>", "wgrad", (3, 16, 32), [8], 64, ("acc0",),
     opts=dict(wgrad_cin8_grid=5))
case("wg_cin8_bna_nodz", "wgrad_cin8", "igemm_wgrad_cin8_kernel<true>", "wgrad", (2, 8, 32), [8], 64, ("bna", "nodz"))
# test_wgrad_persistent_halo: the tap-pair default and the one-tap-per-wave forms
HP = [("pair", {}, "igemm_wgrad_halopair_kernel<6, 0>", "wgrad_halopair"),
      ("pf", dict(wgrad_halop_pair=0), "igemm_wgrad_halop_kernel<8, false, 4, false, true>", "wgrad_halop"),
      ("plain", dict(wgrad_halop_pair=0, wgrad_halop_pf=0), "igemm_wgrad_halop_kernel<8, false, 4, false, false>", "wgrad_halop"),
      ("pf_spread8", dict(wgrad_halop_pair=0, wgrad_halop_spread=8), "igemm_wgrad_halop_kernel<8, false, 8, false, true>",
       "wgrad_halop"),
      ("spread8", dict(wgrad_halop_pair=0, wgrad_halop_spread=8, wgrad_halop_pf=0),
       "igemm_wgrad_halop_kernel<8, false, 8, true, false>", "wgrad_halop"),
      ("waves9", dict(wgrad_halop_pair=0, wgrad_halop_spread=8, wgrad_halop_waves=9),
       "igemm_wgrad_halop_kernel<9, false, 8, true, false>", "wgrad_halop")]
for shp, parts, nout in (((1, 32, 96), [64], 64), ((2, 16, 64), [128, 64], 128), ((3, 16, 32), [64], 64)):
    for name, o, kn, fam in HP:
        if name in ("pf_spread8", "spread8") and nout == 128:
            continue
        case(f"wg_halo_{name}_{'x'.join(map(str, parts))}_{nout}_{shp[0]}", fam, kn, "wgrad", shp, parts, nout,
             ("dB",) + (("acc0",) if name in ("pair", "plain") else ()), opts=o)
case("wg_halopair_defer", "wgrad_halopair", "igemm_wgrad_halopair_kernel<6, 0>", "wgrad", (2, 32, 64), [64], 64,
     ("dB", "defer", "acc0"))
case("wg_halopair_up", "wgrad_halopair", "igemm_wgrad_halopair_kernel<6, 0>", "wgrad", (2, 8, 16), [64], 64, ("dB",), up=True)
case("wg_halop_claim", "wgrad_halop", "igemm_wgrad_halop_kernel<8, false, 4, true, false>", "wgrad", (2, 32, 64), [64], 64,
     ("dB",), opts=dict(wgrad_halop_claim=1, wgrad_halop_grid=7))
# fused BatchNorm-backward apply (test_wgrad_bn_apply_fused): M a power of two, dgamma / dbeta multiples of it
case("wg_bna_fused_64", "wgrad_halop", "igemm_wgrad_halop_kernel<8, true", "wgrad", (2, 16, 32), [64], 64, ("bna", "dB"))
case("wg_bna_fused_nodz", "wgrad_halop", "igemm_wgrad_halop_kernel<8, true", "wgrad", (2, 16, 32), [64], 64, ("bna", "nodz"))
case("wg_bna_fused_2ch", "wgrad_halop", "igemm_wgrad_halop_kernel<8, true", "wgrad", (2, 16, 32), [64, 64], 64,
     ("bna", "dB", "acc0"), opts=dict(wgrad_bna_maxch=2))
case("wg_bna_two_launch_2ch", "wgrad_halopair", "igemm_wgrad_halopair_kernel<6, 0>", "wgrad", (2, 16, 32), [64, 64], 64,
     ("bna", "dB"))
case("wg_bna_two_launch_tap64", "wgrad_tap64", "igemm_wgrad_tap64_kernel<", "wgrad", (2, 16, 16), [64], 64, ("bna", "dB"))
case("wg_bna_two_launch_f32", "wgrad_halo_f32", "igemm_wgrad_halo_f32_kernel<", "wgrad", (1, 16, 32), [64], 64,
     ("bna", "dB"), dts=("f32",))

# weight gradient, f32 (WF32_CASES, test_wgrad_f32_input_layer, test_wgrad_f32_halo, F32_DIL_WGRAD_CASES)
O32 = dict(wgrad_f32=1, wgrad_f32_halo=0)
case("wg_f32_plain_n96", "wgrad_f32", "igemm_wgrad_f32_kernel<", "wgrad", (2, 12, 20), [64], 96, ("dB",), dts=("f32",), opts=O32)
case("wg_f32_concat_n64", "wgrad_f32", "igemm_wgrad_f32_kernel<", "wgrad", (1, 20, 36), [32, 64], 64, ("dB", "acc0"),
     dts=("f32",), opts=O32)
case("wg_f32_dil4_n48", "wgrad_f32", "igemm_wgrad_f32_kernel<", "wgrad", (2, 16, 16), [96], 48, ("dB",), dts=("f32",),
     opts=O32, dil=4)
case("wg_f32_up2_n128", "wgrad_f32", "igemm_wgrad_f32_kernel<", "wgrad", (2, 6, 10), [64], 128, ("dB",), dts=("f32",),
     opts=O32, up=True)
case("wg_f32_ragged_n40", "wgrad_f32", "igemm_wgrad_f32_kernel<", "wgrad", (1, 13, 23), [32], 40, ("dB",), dts=("f32",),
     opts=O32)
case("wg_f32_convt_c32", "wgrad_f32", "igemm_wgrad_f32_kernel<", "wgrad", (2, 8, 16), [64], 128, ("dB", "shuffle"),
     dts=("f32",), opts=O32, kh=1, kw=1, pad=0, cps=32)
case("wg_f32_generic", "wgrad_generic", "igemm_wgrad_kernel<float>", "wgrad", (1, 13, 23), [32], 40, ("dB",), dts=("f32",))
case("wg_in1_ragged", "wgrad_in1_f32", "wgrad_in1_f32_kernel", "wgrad", (1, 40, 56), [8], 64, ("dB",), dts=("f32",),
     real=(1, 0, 48))
case("wg_in1_acc0", "wgrad_in1_f32", "wgrad_in1_f32_kernel", "wgrad", (2, 32, 32), [8], 64, ("dB", "acc0"), dts=("f32",),
     real=(1, 0, 64))
case("wg_in1_defer", "wgrad_in1_f32", "wgrad_in1_f32_kernel", "wgrad", (2, 32, 32), [8], 64, ("dB", "defer"), dts=("f32",),
     real=(1, 0, 64))
for name, shp, parts, nout, up in (("c64_64", (2, 32, 64), [64], 64, False), ("c96_96_ragged_n", (1, 16, 64), [96], 96, False),
                                   ("concat_64_64", (2, 16, 32), [64, 64], 64, False), ("up2_96_64", (2, 16, 32), [96], 64, True)):
    case(f"wg_f32_halo_{name}", "wgrad_halo_f32", "igemm_wgrad_halo_f32_kernel<", "wgrad", shp, parts, nout,
         ("dB",) + (("acc0",) if up else ()), dts=("f32",), up=up)
for reals, nout, nreal in (([44], 64, 44), ([44, 44], 64, 44), ([12], 64, 20), ([64, 44], 64, 40)):
    case(f"wg_f32_halo_zt_{'x'.join(map(str, reals))}_n{nreal}", "wgrad_halo_f32", "igemm_wgrad_halo_f32_kernel<", "wgrad",
         (1, 32, 64), [64] * len(reals), nout, ("dB",), dts=("f32",), opts=dict(wgrad_f32_bias=1),
         real=(reals[0], reals[1] if len(reals) > 1 else 0, nreal))
case("wg_f32_dil2", "wgrad_halo_f32_dil", "igemm_wgrad_halo_f32_dil_kernel<1>", "wgrad", (1, 32, 64), [64], 64, ("dB",),
     dts=("f32",), dil=2)
case("wg_f32_dil4_ragged_n", "wgrad_halo_f32_dil", "igemm_wgrad_halo_f32_dil_kernel<1>", "wgrad", (2, 16, 128), [96], 96,
     ("dB", "acc0"), dts=("f32",), dil=4)
case("wg_f32_dil8_split2", "wgrad_halo_f32_dil", "igemm_wgrad_halo_f32_dil_kernel<2>", "wgrad", (1, 32, 128), [64], 64,
     ("dB",), dts=("f32",), dil=8)
case("wg_f32_dil16_split8", "wgrad_halo_f32_dil", "igemm_wgrad_halo_f32_dil_kernel<8>", "wgrad", (1, 64, 64), [32], 96,
     ("dB",), dts=("f32",), dil=16)


# ------------------------------------------------------------------------------------------------------- operands
REGIMES = {"wide": (8, 4), "narrow": (2, 1)}
GEOM_KEYS = ("dil", "up", "kh", "kw", "pad", "stride", "Ho", "Wo")


def data_key(c, dtn):
    """What the operands and the reference depend on: not the id, the options or the expected kernel, so the rows of
    an option axis share one reference (lru_cache below)."""
    return (c["kind"], c["shape"], c["parts"], c["nout"], c["epi"], c["regime"], dtn, tuple(sorted(c["geom"].items())))


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).float()


def _choice(g, n, values):
    return torch.tensor(values, dtype=torch.float32)[torch.randint(0, len(values), (n,), generator=g)]


def _weights(g, rows, cols, regime):
    if regime == "wide":
        return _ints(g, (rows, cols), -4, 4)
    return _ints(g, (rows, cols), -1, 1) * (torch.rand(rows, cols, generator=g) < 0.25)


def _sizes(kind, shape, geom):
    N, H, W = shape
    up = bool(geom.get("up"))
    kh, kw, dil, stride = geom.get("kh", 3), geom.get("kw", 3), geom.get("dil", 1), geom.get("stride", 1)
    pad = geom.get("pad", dil * (kh // 2))
    Ho = geom.get("Ho", CR.out_size(H, up=up, stride=stride, k=kh, dil=dil, pad=pad))
    Wo = geom.get("Wo", CR.out_size(W, up=up, stride=stride, k=kw, dil=dil, pad=pad))
    return N, H, W, Ho, Wo, kh, kw


@functools.lru_cache(maxsize=6)
def prepare(key):
    """(operands as CPU f32 tensors, reference dict) of one data key; asserts the exactness condition."""
    kind, shape, parts, nout, epi, regime, dtn, geom_items = key
    geom = dict(geom_items)
    dt = DT[dtn]
    g = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
    amax, _ = REGIMES[regime]
    bmax = 8 if regime == "wide" else 2
    split, cps, real = geom.pop("split", 0), geom.pop("cps", 0), geom.pop("real", None)
    N, H, W, Ho, Wo, kh, kw = _sizes(kind, shape, geom)
    inp = {}
    if kind == "wgrad":
        return _prepare_wgrad(key, g, geom, split, cps, real)
    grid = 1.0
    if kind == "fwd":
        srcs = [_ints(g, (N, H, W, p), -amax, amax) for p in parts]
        K = kh * kw * sum(parts)
        Wt = torch.zeros(round_up(nout, 64), round_up(K, 32))
        Wt[:nout, :K] = _weights(g, nout, K, regime)
        if real is not None:   # the hints' contract: pad channels of the sources and their weight columns are zeros
            off = 0
            for s, p, r in zip(srcs, parts, real[:2]):
                s[..., r:] = 0
                for t in range(kh * kw):
                    Wt[:, t * sum(parts) + off + r: t * sum(parts) + off + p] = 0
                off += p
            if real[2]:
                Wt[real[2]:] = 0
        inp.update(srcs=srcs, W=Wt)
    else:   # data gradients: dY and the MASTER weights of the forward layer; parts = (channels of dY,), nout = Cin_s
        cy, cin_s = parts[0], nout
        if kind == "dgrad":
            dY = _ints(g, (N, H, W, cy), -amax, amax)
            Wm = torch.zeros(round_up(cy, 64), round_up(kh * kw * cin_s, 32))
            Wm[:cy, :kh * kw * cin_s] = _weights(g, cy, kh * kw * cin_s, regime)
            gemm = CR.conv_dgrad(dY, Wm, cy, cin_s, Hs=H, Ws=W, kh=kh, kw=kw, dil=geom.get("dil", 1))
            Ho, Wo = H, W
        else:       # ConvTranspose: shape is the low-resolution grid, dY lives at twice that
            dY = _ints(g, (N, 2 * H, 2 * W, cps), -amax, amax)
            Wm = torch.zeros(round_up(4 * cps, 64), round_up(cin_s, 32))
            Wm[:4 * cps, :cin_s] = _weights(g, 4 * cps, cin_s, regime)
            gemm = CR.convt_dgrad(dY, Wm, cps, cin_s)
            Ho, Wo = H, W
        inp.update(dY=dY, Wm=Wm)
    n1 = split if split else nout
    kw_ref = dict(round_to=dt, relu="relu" in epi, bn_stats="stats" in epi)
    if "bias" in epi:
        nb = cps if "shuffle" in epi else nout
        inp["bias"] = _ints(g, (nb,), -bmax, bmax)
        if real is not None and real[2]:
            inp["bias"][real[2]:] = 0
        kw_ref["bias"] = inp["bias"]
    if "drop" in epi:
        kw_ref.update(dropout_rate=0.5, dropout_seed=DROP_SEED)
    if "shuffle" in epi:
        kw_ref.update(out_mode=1, shuffle_c=cps)
    if split:
        kw_ref.update(out_mode=2, split_c=split)
    if "add" in epi:
        inp["addend"] = _ints(g, (N, Ho, Wo, n1), -amax, amax)
        kw_ref["addend"] = inp["addend"]
    if "mask" in epi:
        inp["mask"] = _ints(g, (N, Ho, Wo, n1), -2, 2)
        kw_ref.update(mask=inp["mask"], mask_scale=2.0)
    if "mask2" in epi:
        inp["mask2"] = _ints(g, (N, Ho, Wo, nout - n1), -2, 2)
        kw_ref.update(mask2=inp["mask2"], mask2_scale=0.5)
    if "accum" in epi:
        inp["accum"] = _ints(g, (N, Ho, Wo, n1), -8, 8)
        kw_ref["accum"] = inp["accum"]
    if "bnr" in epi:
        inp["bnr"] = (_ints(g, (N, Ho, Wo, nout), -4, 4), _choice(g, nout, [0.5, 1.0, 2.0, -1.0]), _ints(g, (nout,), -2, 2),
                      _ints(g, (nout,), -2, 2), _choice(g, nout, [0.5, 1.0, 2.0]))
        kw_ref["bn_reduce"] = inp["bnr"]
    if "bnload" in epi:
        inp["bnload"] = (_choice(g, parts[0], [0.5, 1.0, 2.0, -1.0]), _ints(g, (parts[0],), -2, 2))
        kw_ref["bn_load"] = [inp["bnload"]]
        grid = 0.5
    nstat = cps if "shuffle" in epi else nout
    inp["base"] = _ints(g, (2, nstat), -8, 8) if "acc0" in epi else torch.zeros(2, nstat)
    if kind == "fwd":
        ref = CR.conv_fwd(inp["srcs"], inp["W"], nout, **kw_ref, **geom)
    else:
        ref = CR.conv_fwd([], None, nout, gemm=gemm, **kw_ref)
    if "drop" in epi:   # the value before the dropout decision, for the kept-set assertion
        nd = dict(kw_ref)
        nd.update(dropout_rate=0.0)
        ref["v_nodrop"] = (CR.conv_fwd(inp["srcs"], inp["W"], nout, **nd, **geom) if kind == "fwd" else
                           CR.conv_fwd([], None, nout, gemm=gemm, **nd))["v"]
    # the exactness condition
    assert CR.exact(ref["A_out"], grid=grid), (key, float(ref["A_out"].max()))
    if "stats" in epi:
        b = inp["base"].double().abs()
        assert CR.exact(ref["A_stats"][0] + b[0], grid=grid) and CR.exact(ref["A_stats"][1] + b[1], grid=grid * grid), \
            (key, float(ref["A_stats"][1].max()))
    if "bnr" in epi:
        b = inp["base"].double().abs()
        assert CR.exact(ref["A_bnr"][0] + b[0], grid=0.5) and CR.exact(ref["A_bnr"][1] + b[1]), key
    return inp, ref


def _prepare_wgrad(key, g, geom, split, cps, real):
    kind, shape, parts, nout, epi, regime, dtn, _ = key
    dt = DT[dtn]
    N, H, W, Ho, Wo, kh, kw = _sizes(kind, shape, geom)
    srcs = [_ints(g, (N, H, W, p), -8, 8) for p in parts]
    K = kh * kw * sum(parts)
    inp = dict(srcs=srcs)
    bn_apply = None
    if "bna" in epi:
        M = N * Ho * Wo
        assert M & (M - 1) == 0, "bn_apply cases need a power-of-two pixel count"
        inp["bna"] = (2 * _ints(g, (N, Ho, Wo, nout), -4, 4), _ints(g, (N, Ho, Wo, nout), -4, 4),
                      _choice(g, nout, [0.5, 1.0, 2.0, -1.0]), _ints(g, (nout,), -2, 2), _ints(g, (nout,), -2, 2),
                      _choice(g, nout, [0.5, 1.0, 2.0]), _choice(g, nout, [1.0, 2.0]),
                      M * _choice(g, nout, [-4.0, 0.0, 4.0]), M * _choice(g, nout, [-2.0, 0.0, 2.0]), float(M))
        bn_apply = inp["bna"]
        dY = None
    elif "shuffle" in epi:
        dY = _ints(g, (N, 2 * Ho, 2 * Wo, cps), -8, 8)
    else:
        dY = _ints(g, (N, Ho, Wo, nout), -8, 8)
    if real is not None:
        for s, r in zip(srcs, real[:2]):
            s[..., r:] = 0
        if real[2]:
            dY[..., real[2]:] = 0
    inp["dY"] = dY
    nb = cps if "shuffle" in epi else nout
    inp["baseW"] = _ints(g, (nout, K), -8, 8) if "acc0" in epi else torch.zeros(nout, K)
    inp["baseB"] = _ints(g, (nb,), -8, 8) if "acc0" in epi else torch.zeros(nb)
    ref = CR.conv_wgrad(srcs, dY, nout, shuffle_c=cps if "shuffle" in epi else 0, bn_apply=bn_apply, round_to=dt, **geom)
    assert CR.exact(ref["A_dW"] + inp["baseW"].double().abs(), ref["A_dB"] + inp["baseB"].double().abs()), key
    if bn_apply is not None:   # every term of dz an integer: exact in f32 in any evaluation order
        t = CR.E.bn_bwd_apply_terms(*[CR.f64(x) for x in bn_apply[:9]], bn_apply[9])
        assert all(bool((x == x.round()).all()) for x in t), key
    return inp, ref


# ------------------------------------------------------------------------------------------------------- the runs
@contextlib.contextmanager
def options(opts):
    """Native options for one launch; every one goes back to its default (None) afterwards. Split-K of the tap64
    launcher is off unless the row turns it on: small launches would otherwise take it and change the form."""
    from adipose_amd import ops
    o = dict(tap64_ksplit=0)
    o.update(opts)
    try:
        for k, v in o.items():
            ops.set_option(k, v)
        yield
    finally:
        for k in o:
            ops.set_option(k, None)


def guarded(shape, nreal, dt, value=None):
    """A device NHWC tensor of channel stride nreal + 8 inside a sentinel-filled buffer with 256 + stride elements
    behind it. Returns (the whole buffer, the view, the tail)."""
    N, H, W = shape
    stride = nreal + 8
    n = N * H * W * stride
    buf = torch.full((n + stride + 256,), SENT, dtype=dt, device=DEV)
    view = buf[:n].view(N, H, W, stride)
    if value is not None:
        view[..., :nreal] = value.to(DEV, dt)
    return buf, view, buf[n:]


def guarded_vec(n, value):
    v = torch.full((n + 8,), SENT, dtype=torch.float32, device=DEV)
    v[:n] = value.to(DEV)
    return v


def check_map(view, tail, nreal, ref, what):
    CR.assert_exact(view[..., :nreal], ref, what, sentinel=SENT,
                    guard=torch.cat([view[..., nreal:].reshape(-1), tail]))


def check_vec(vec, n, ref, what):
    CR.assert_exact(vec[:n], ref, what, sentinel=SENT, guard=vec[n:])


def check_kernel(c, dtn, kname):
    from adipose_amd import ops
    want = c["kernel"][dtn] if isinstance(c["kernel"], dict) else c["kernel"]
    assert kname.startswith(want), f"{c['id']}: launched {kname}, expected {want}"
    fields = kname[kname.index("<") + 1:kname.rindex(">")].split(", ") if "<" in kname else []
    for i, text in c["kfields"].items():
        if i == "ksplit":
            assert ops.get_option("tap64_ksplit_last") >= text, (kname, ops.get_option("tap64_ksplit_last"))
        else:
            assert fields[i] == text, f"{c['id']}: template argument {i} of {kname} is not {text}"


def run_fwd(c, dtn):
    from adipose_amd import _lib, ops
    dt = DT[dtn]
    inp, ref = prepare(data_key(c, dtn))
    kind, epi, nout, parts = c["kind"], c["epi"], c["nout"], c["parts"]
    geom = dict(c["geom"])
    split, cps, real = geom.pop("split", 0), geom.pop("cps", 0), geom.pop("real", None)
    N, H, W, Ho, Wo, kh, kw = _sizes(kind, c["shape"], geom)
    dev = lambda t, d=dt: t.to(DEV, d).contiguous()   # noqa: E731
    n1 = split if split else nout
    with options(c["opts"]):
        if kind == "fwd":
            srcs, Wd = [dev(s) for s in inp["srcs"]], dev(inp["W"])
        else:   # the device path of a data gradient: repack the f32 master weights, then a forward launch over dY
            Ho, Wo = H, W
            srcs, cy, cin_s = [dev(inp["dY"])], parts[0], nout
            Wm = dev(inp["Wm"], torch.float32)
            if kind == "dgrad":
                Wd = torch.zeros(round_up(cin_s, 64), round_up(kh * kw * cy, 32), dtype=dt, device=DEV)
                ops.pack_weights(Wm, Wd, 1, taps=kh * kw, cin_s=cin_s, nout=cy)
            else:
                Wd = torch.zeros(round_up(cin_s, 64), round_up(4 * cps, 32), dtype=dt, device=DEV)
                ops.pack_weights(Wm, Wd, 2, taps=1, cin_s=cin_s, nout=4 * cps)
                geom.update(kh=2, kw=2, pad=0, stride=2, Ho=H, Wo=W)
        kw_ = dict(geom)
        if "shuffle" in epi:
            obuf, out, otail = guarded((N, 2 * Ho, 2 * Wo), cps, dt)
            kw_.update(out_mode=1, shuffle_c=cps)
        else:
            obuf, out, otail = guarded((N, Ho, Wo), n1, dt)
        if split:
            o2buf, out2, o2tail = guarded((N, Ho, Wo), nout - n1, dt)
            kw_.update(out_mode=2, out2=out2, split_c=split)
        if len(srcs) > 1:
            kw_["srcB"] = srcs[1]
        if "bias" in epi:
            kw_["bias"] = dev(inp["bias"], torch.float32)
        if "relu" in epi:
            kw_["relu"] = True
        if "drop" in epi:
            kw_.update(dropout_rate=0.5, dropout_seed=DROP_SEED)
        if "add" in epi:
            kw_["addend"] = guarded((N, Ho, Wo), n1, dt, inp["addend"])[1]
        if "mask" in epi:
            kw_.update(mask=dev(inp["mask"]), mask_scale=2.0)
        if "mask2" in epi:
            kw_.update(mask2=dev(inp["mask2"]), mask2_scale=0.5)
        if "accum" in epi:
            abuf, acc, atail = guarded((N, Ho, Wo), n1, torch.float32, inp["accum"])
            kw_["accum"] = acc
        nstat = cps if "shuffle" in epi else nout
        s1, s2 = guarded_vec(nstat, inp["base"][0]), guarded_vec(nstat, inp["base"][1])
        if "stats" in epi:
            kw_["bn_stats"] = (s1, s2)
            if "fold" in epi:
                kw_["defer_fold"] = True
        if "bnr" in epi:
            z, sc, sh, mu, ist = inp["bnr"]
            zd = guarded((N, Ho, Wo), nout, dt, z)[1]
            vec = [guarded_vec(nout, t) for t in (sc, sh, mu, ist)]
            kw_["bn_reduce"] = (zd, *vec, s1, s2)      # (dgamma, dbeta) = (s1, s2)
        if "bnload" in epi:
            kw_["bnA"] = tuple(dev(t, torch.float32) for t in inp["bnload"])
            act = torch.full_like(srcs[0], SENT)
            kw_["act_out"] = act
        if real is not None:
            kw_["real"] = real
        ops.conv_fwd(srcs[0], Wd, nout, out=out, **kw_)
        kname = _lib.lib().adp_last_kernel().decode()
        if "fold" in epi:
            M = N * Ho * Wo
            assert M & (M - 1) == 0
            one = torch.ones(nstat, device=DEV)
            fin = [torch.full((nstat,), SENT, device=DEV) for _ in range(4)]   # scale, shift, mean, invstd
            ops.bn_finalize(M, s1[:nstat], s2[:nstat], one, one, 1e-3, 0.0, *fin, fold=True)
        torch.cuda.synchronize()
    check_kernel(c, dtn, kname)
    check_map(out, otail, cps if "shuffle" in epi else n1, ref["out"], "out")
    if split:
        check_map(out2, o2tail, nout - n1, ref["out2"], "out2")
    if "accum" in epi:
        check_map(acc, atail, n1, ref["accum"], "accum")
    base = inp["base"].double()
    if "stats" in epi:
        check_vec(s1, nstat, base[0] + ref["stats"][0], "sum")
        check_vec(s2, nstat, base[1] + ref["stats"][1], "sum of squares")
        if "fold" in epi:
            CR.assert_exact(fin[2], (base[0] + ref["stats"][0]) / (N * Ho * Wo), "finalized mean")
    if "bnr" in epi:
        check_vec(s1, nstat, base[0] + ref["bnr"][0], "dgamma")
        check_vec(s2, nstat, base[1] + ref["bnr"][1], "dbeta")
    if "bnload" in epi:
        CR.assert_exact(act, ref["act"][0], "act_out")
    if "drop" in epi:   # the kept set is the host's adp_uniform mask; kept values are rt(2 * relu(ref))
        pos = ref["v_nodrop"] > 0
        got = CR.f64(out[..., :n1])
        CR.assert_exact((got != 0) & pos, ref["keep"] & pos, "kept set")
        CR.assert_exact(got[ref["keep"]], CR.rt(2.0 * ref["v_nodrop"], dt)[ref["keep"]], "kept values")


def run_wgrad(c, dtn):
    from adipose_amd import _lib, ops
    dt = DT[dtn]
    inp, ref = prepare(data_key(c, dtn))
    epi, nout, parts = c["epi"], c["nout"], c["parts"]
    geom = dict(c["geom"])
    geom.pop("split", 0)
    cps, real = geom.pop("cps", 0), geom.pop("real", None)
    N, H, W, Ho, Wo, kh, kw = _sizes("wgrad", c["shape"], geom)
    K = kh * kw * sum(parts)
    dev = lambda t, d=dt: t.to(DEV, d).contiguous()   # noqa: E731
    with options(c["opts"]):
        srcs = [dev(s) for s in inp["srcs"]]
        dW = torch.full((round_up(nout, 64), round_up(K, 32)), WSENT, device=DEV)
        dW[:nout, :K] = inp["baseW"].to(DEV)
        nb = cps if "shuffle" in epi else nout
        dB = guarded_vec(nb, inp["baseB"]) if "dB" in epi else None
        kw_ = dict(geom)
        if len(srcs) > 1:
            kw_["srcB"] = srcs[1]
        if "shuffle" in epi:
            kw_["shuffle_c"] = cps
        if real is not None:
            kw_["real"] = real
        dz = dztail = None
        if "bna" in epi:
            b = inp["bna"]
            kw_["bn_apply"] = (dev(b[0]), dev(b[1])) + tuple(dev(t, torch.float32) for t in b[2:9]) + (b[9],)
            if "nodz" in epi:
                dY = None
            else:
                n = N * Ho * Wo * nout
                dzbuf = torch.full((n + 256,), SENT, dtype=dt, device=DEV)
                dY, dztail = dzbuf[:n].view(N, Ho, Wo, nout), dzbuf[n:]
                dz = dY
        else:
            dY = dev(inp["dY"])
        if "defer" in epi:
            ops.wgrad_defer(True)
        try:
            ops.conv_wgrad(srcs[0], dY, dW, nout, dB=dB, **kw_)
            kname = _lib.lib().adp_last_kernel().decode()
        finally:
            if "defer" in epi:
                ops.wgrad_flush()
        torch.cuda.synchronize()
    check_kernel(c, dtn, kname)
    CR.assert_exact(dW[:nout, :K], inp["baseW"].double() + ref["dW"], "dW", sentinel=WSENT,
                    guard=torch.cat([dW[nout:].reshape(-1), dW[:nout, K:].reshape(-1)]))
    if dB is not None:
        check_vec(dB, nb, inp["baseB"].double() + ref["dB"], "dB")
    if dz is not None:
        CR.assert_exact(dz, ref["dz"], "dz", sentinel=SENT, guard=dztail)


PARAMS = [pytest.param(c, dtn, id=f"{c['id']}-{dtn}") for c in CASES for dtn in c["dts"]]


@pytest.mark.parametrize("c,dtn", PARAMS)
def test_conv_exact(c, dtn):
    """One row of CASES in one dtype: the launch must report the row's kernel and equal the float64 reference bit
    for bit, with every sentinel intact."""
    try:
        (run_wgrad if c["kind"] == "wgrad" else run_fwd)(c, dtn)
    except AssertionError:
        raise
    except Exception as e:   # a device fault ends the session: nothing more is launched on a faulted GPU
        if any(w in str(e).lower() for w in ("illegal memory", "hip error", "hiperror", "launch failure", "device-side")):
            pytest.exit(f"GPU fault in {c['id']}-{dtn}: {e}", returncode=3)
        raise


# ---------------------------------------------------- fused statistics on real-valued data, derived gates
# Exact integers prove the indexing; how far the f32 partial sums drift needs real values. The weights are one-hot
# (GEMM column n copies channel n % Cin of the centre tap), so the accumulator is exact and v = f32(x + bias[n]) is
# known bit for bit: x ~ N(0, 1) rounded to the storage type, bias 0 on even and 3 on odd channels (mean / std of the
# output 0 and 3). The device sums are held to the float64 sums of those same values within DESIGN section 6's
# (K + 8) * 2^-24 * A, A the float64 sum of |terms|, K the longest f32 chain in front of the f64 accumulator, read
# from each form's code:
#   tap64 (epi_rows + epi_bn_flush, conv_common.h): a thread walks rows tid / GPR, + RSTEP, ... of every row group of
#       its BM x BN tile (GPR = BN / 8, RSTEP = NTH / GPR): BM / RSTEP additions; epi_bn_flush adds the RSTEP
#       threads of a column group through LDS; then one f64 atomic per block. K = BM / RSTEP + RSTEP.
#       256 x 64 tile, 256 threads: GPR = 8, RSTEP = 32, K = 8 + 32 = 40.
#   tap64p (register epilogue, conv_fwd_tap64p.hip): s1 / s2 are zeroed per tile and channel quad; a lane adds its
#       2 * MIQ rows (MIQ = TM / 32: 8 rows of the 256 x 256 tile, 4 of the 256 x 128 one), row16_sum adds the 16
#       pixel lanes in 4 steps, then p_lds_add adds into sacc, which is f64. K = 2 * MIQ + 4 = 12 / 8 whatever the
#       number of tiles a block walks: the f32 chain does not grow with the pixels per block.
#   w4 (conv_fwd_w4.hip): the same scheme, 8 rows per lane and channel quad, sacc f64. K = 8 + 4 = 12.
#   halop (conv_fwd_halo.hip): s1 / s2 live across ALL tiles of a block (zeroed once, flushed after the tile loop):
#       a lane adds 2 pixels (mf = 0, 1 of its wave's 32-pixel patch row) per tile, then row16_sum's 4 steps and
#       one f64 atomic per wave. K = 2 * ceil(T / G) + 4, T the patches of one output block, G the blocks per output
#       block. This is the one form whose f32 chain grows with the pixels per block.
#   cin8 (conv_fwd_cin8.hip): s1 / s2 live across all 16-pixel groups a wave takes (UNR = 4 per pass, passes
#       nwaves * UNR apart), one pixel per lane and group, then row16_sum and one f64 atomic per wave.
#       K = 4 * ceil(groups / (4 * nwaves)) + 4, groups = ceil(M / 16), nwaves = 4 * ceil(min(ceil(groups / 4), 2048) / 4):
#       8 up to 131 072 pixels, 132 on the bench step's 4 x 1024^2 input layer.
# Long chains: one block per output block on 8 192 - 16 384 pixels. halop: T = 64 patches, G = 1: K = 132; the bench
# step (unet_bn, batch 4, 1024^2, BASELINE.json configs) has T = 4 * 128 * 32 = 16 384 patches on 128 blocks per
# output block for its 128-channel level-0 launches: 128 tiles, K = 260, and 64 tiles (K = 132) for 64 -> 64.
# tap64p / w4: K stays 12 on one block as on 256.
GATE_CASES = []


def gate_case(id, family, kernel, shape, cin, nout, K, dtn="bf16", opts=None):
    GATE_CASES.append(dict(id=id, family=family, kernel=kernel, shape=shape, cin=cin, nout=nout, K=K, dtn=dtn,
                           opts=dict(opts or {}), exact=False))


def halop_chain(shape, grid):
    patches = shape[0] * (shape[1] // 8) * (shape[2] // 32)
    g = max(1, min(patches, grid))
    return 2 * -(-patches // g) + 4


T64_GATE = dict(fwd_tap64=5, tap64_persist=0, fwd_halo=0, tap64_mask_lds=0)
gate_case("gate_tap64_256x64", "fwd_tap64", "igemm_fwd_tap64_kernel<4, 1, 64,", (1, 23, 23), 128, 192, 256 // 32 + 32,
          opts=T64_GATE)
gate_case("gate_tap64_256x64_f32", "fwd_tap64", "igemm_fwd_tap64_kernel<4, 1, 64,", (1, 23, 23), 128, 192, 256 // 32 + 32,
          dtn="f32", opts=T64_GATE)
P_GATE = dict(fwd_tap64=2, fwd_halo=0, fwd_w4=0)
gate_case("gate_tap64p_256", "fwd_tap64p", "igemm_fwd_tap64p_kernel<256, 256, 2, false, true", (2, 32, 64), 64, 256,
          2 * 4 + 4, opts=P_GATE)
gate_case("gate_tap64p_128", "fwd_tap64p", "igemm_fwd_tap64p_kernel<256, 128, 3, false, true", (2, 32, 64), 64, 128,
          2 * 2 + 4, opts=dict(fwd_tap64=3, fwd_halo=0, fwd_w4=0))
gate_case("gate_tap64p_256_long_chain", "fwd_tap64p", "igemm_fwd_tap64p_kernel<256, 256, 2, false, true", (2, 64, 64), 64,
          256, 2 * 4 + 4, opts=dict(P_GATE, tap64_persist_grid=1))
W4_GATE = dict(fwd_tap64=2, fwd_halo=0, fwd_w4=1)
gate_case("gate_w4", "fwd_w4", "igemm_fwd_w4_kernel<true", (2, 32, 64), 64, 256, 8 + 4, opts=W4_GATE)
gate_case("gate_w4_long_chain", "fwd_w4", "igemm_fwd_w4_kernel<true", (2, 64, 64), 64, 256, 8 + 4,
          opts=dict(W4_GATE, tap64_persist_grid=1, fwd_w4_grid=1))
# halo, non-persistent (epi_rows over the 8 patch rows of 32 pixels, 512 threads, BN = 64: GPR = 8): a thread with a row
# adds one per patch row, 8 additions; epi_bn_flush adds NTH / GPR = 64 LDS lanes. K = 8 + 64 = 72.
gate_case("gate_halo", "fwd_halo", "igemm_fwd_halo_kernel<", (1, 16, 64), 64, 64, 8 + 512 // 8, opts=dict(halo_persist=0))
gate_case("gate_halop", "fwd_halop", "igemm_fwd_halop_kernel<false, 1, 64", (1, 16, 64), 64, 64,
          halop_chain((1, 16, 64), 256))
gate_case("gate_halop_long_chain", "fwd_halop", "igemm_fwd_halop_kernel<false, 1, 64", (4, 64, 64), 64, 64,
          halop_chain((4, 64, 64), 1), opts=dict(halo_persist_grid=1))


def cin8_chain(M):
    groups = -(-M // 16)
    nwaves = 4 * -(-max(1, min(-(-groups // 4), 2048)) // 4)
    return 4 * -(-groups // (4 * nwaves)) + 4


gate_case("gate_cin8", "fwd_cin8", "igemm_fwd_cin8_kernel<", (2, 32, 32), 8, 64, cin8_chain(2048), opts=dict(cin8_pf=0))
gate_case("gate_cin8_16k", "fwd_cin8", "igemm_fwd_cin8_kernel<", (4, 64, 64), 8, 64, cin8_chain(16384), opts=dict(cin8_pf=0))
assert cin8_chain(2048) == 8 and cin8_chain(16384) == 8 and cin8_chain(4 * 1024 * 1024) == 132
assert halop_chain((1, 16, 64), 256) == 6 and halop_chain((4, 64, 64), 1) == 132 and halop_chain((4, 1024, 1024), 128) == 260


@functools.lru_cache(maxsize=2)
def gate_operands(shape, cin, nout, dtn):
    N, H, W = shape
    dt = DT[dtn]
    g = torch.Generator().manual_seed(zlib.crc32(repr((shape, cin, nout, dtn)).encode()))
    x = torch.randn(N, H, W, cin, generator=g).to(dt).float()
    Wt = torch.zeros(round_up(nout, 64), round_up(9 * cin, 32))
    n = torch.arange(nout)
    Wt[n, 4 * cin + n % cin] = 1.0
    bias = 3.0 * (n % 2).float()
    ref = CR.conv_fwd([x], Wt, nout, bias=bias, bn_stats=True, round_to=dt, v_round=torch.float32)
    return x, Wt, bias, ref


@pytest.mark.parametrize("c", GATE_CASES, ids=[c["id"] for c in GATE_CASES])
def test_fused_statistics_within_derived_gate(c):
    """Sum, sum of squares and var = q / n - mean^2 of a fused bn_stats launch on real-valued data against the
    float64 sums of the very values the device summed, within (K + 8) * 2^-24 * A with K derived above. The stored
    output is bit-equal too (one f32 addition, then the store's rounding). Prints error / gate for DESIGN section 6."""
    from adipose_amd import _lib, ops
    dt = DT[c["dtn"]]
    N, H, W = c["shape"]
    nout, K = c["nout"], c["K"]
    x, Wt, bias, ref = gate_operands(c["shape"], c["cin"], nout, c["dtn"])
    with options(c["opts"]):
        obuf, out, otail = guarded((N, H, W), nout, dt)
        s1, s2 = guarded_vec(nout, torch.zeros(nout)), guarded_vec(nout, torch.zeros(nout))
        ops.conv_fwd(x.to(DEV, dt), Wt.to(DEV, dt), nout, out=out, bias=bias.to(DEV), bn_stats=(s1, s2))
        kname = _lib.lib().adp_last_kernel().decode()
        torch.cuda.synchronize()
    assert kname.startswith(c["kernel"]), kname
    check_map(out, otail, nout, ref["out"], "out")
    (s, q), (As, Aq) = ref["stats"], ref["A_stats"]
    rs = CR.assert_sum_gate(s1[:nout], s, As, K, "sum")
    rq = CR.assert_sum_gate(s2[:nout], q, Aq, K, "sum of squares")
    CR.assert_exact(torch.cat([s1[nout:], s2[nout:]]), torch.full((16,), SENT), "vector tails")
    # var = q / n - mean^2: its error is at most dq / n + 2 |mean| ds / n (+ ds^2 / n^2, far below)
    n = float(N * H * W)
    sd, qd = CR.f64(s1[:nout]), CR.f64(s2[:nout])
    var_d, var_r = qd / n - (sd / n) ** 2, q / n - (s / n) ** 2
    gate_v = CR.sum_gate(K, Aq) / n + 2.0 * (s / n).abs() * CR.sum_gate(K, As) / n
    rv = float(((var_d - var_r).abs() / gate_v).max())
    print(f"GATE {c['id']} K={K} sum={rs:.3f} sqsum={rq:.3f} var={rv:.3f}")
    assert rv <= 1.0, rv


# The fused BatchNorm-backward reduction on real-valued data: dgamma = sum db * (z - mean) * invstd and dbeta = sum db,
# db = the STORED gradient where z * scale + shift > 0. The stored gradient is read back, so the float64 sums of the
# very values the device summed need no exact GEMM: operands are plain randn. Every kernel evaluates a term in at
# most three f32 roundings (inside the + 8). A is the sum of |terms| of the expression the form evaluates: tap64, halo
# and tap64p compute db * (z - mean) * invstd, so A = sum |db (z - mean) invstd|; halop computes
# db * (z * invstd - mean * invstd), whose two parts cancel, so they count separately: A = sum |db| (|z| + |mean|) |invstd|.
# K, from each form's code:
#   tap64 (epi_rows_bnr, and the LDS-staged epilogue of option tap64_bnr_lds, which walks the same rows in the same
#       order): BM / RSTEP rows per thread + RSTEP LDS lanes; 256 x 256 tile, 512 threads: GPR = 32, RSTEP = 16, K = 32.
#   halo (non-persistent, epi_rows_bnr over the 8 patch rows of 32 pixels, 512 threads, BN = 64: GPR = 8): one row per
#       patch row for the threads that have one, 8 additions, + NTH / GPR = 64 LDS lanes. K = 72.
#   tap64p and halop: as their statistics above (per tile and channel quad; across all tiles of the block).
BNR_GATE_CASES = []


def bnr_gate_case(id, family, kernel, shape, cin, nout, K, opts=None):
    BNR_GATE_CASES.append(dict(id=id, family=family, kernel=kernel, shape=shape, cin=cin, nout=nout, K=K,
                               opts=dict(opts or {}), exact=False, split_xhat=family == "fwd_halop"))


for lds in (0, 1):
    bnr_gate_case(f"gate_bnr_tap64_lds{lds}", "fwd_tap64", "igemm_fwd_tap64_kernel<2, 4, 128, true, true,", (1, 24, 40), 256,
                  192, 256 // 16 + 16, opts=dict(tap64_bnr_lds=lds, fwd_tap64=2, fwd_halo=0))
bnr_gate_case("gate_bnr_tap64p_256x128", "fwd_tap64p", "igemm_fwd_tap64p_kernel<256, 128, 3, true, false", (2, 23, 23), 128,
              320, 2 * 2 + 4, opts=dict(tap64_persist=1, fwd_tap64=2, tap64p_cfg=2))
bnr_gate_case("gate_bnr_halo", "fwd_halo", "igemm_fwd_halo_kernel<", (1, 16, 64), 64, 64, 8 + 512 // 8,
              opts=dict(halo_persist=0))
bnr_gate_case("gate_bnr_halop", "fwd_halop", "igemm_fwd_halop_kernel<true, 1, 64", (1, 16, 64), 64, 64,
              halop_chain((1, 16, 64), 256))
bnr_gate_case("gate_bnr_halop_long_chain", "fwd_halop", "igemm_fwd_halop_kernel<true, 1, 64", (4, 64, 64), 64, 64,
              halop_chain((4, 64, 64), 1), opts=dict(halo_persist_grid=1))


@pytest.mark.parametrize("c", BNR_GATE_CASES, ids=[c["id"] for c in BNR_GATE_CASES])
def test_fused_bn_reduce_within_derived_gate(c):
    """dgamma / dbeta of a fused bn_reduce launch (bf16) on real-valued data against the float64 sums over the
    gradient the launch stored, within (K + 8) * 2^-24 * A. Prints error / gate for DESIGN section 6."""
    from adipose_amd import _lib, ops
    dt = torch.bfloat16
    N, H, W = c["shape"]
    cin, nout, K = c["cin"], c["nout"], c["K"]
    g = torch.Generator().manual_seed(zlib.crc32(c["id"].encode()))
    x = torch.randn(N, H, W, cin, generator=g).to(DEV, dt)
    Wt = (torch.randn(round_up(nout, 64), 9 * cin, generator=g) * 0.05).to(DEV, dt)
    z = (torch.randn(N, H, W, nout, generator=g) * 2).to(dt)
    sc, ist = torch.rand(nout, generator=g) + 0.5, torch.rand(nout, generator=g) + 0.5
    sh, mu = torch.rand(nout, generator=g) - 0.5, torch.randn(nout, generator=g) * 0.5
    with options(c["opts"]):
        obuf, out, otail = guarded((N, H, W), nout, dt)
        zd = guarded((N, H, W), nout, dt, z)[1]
        dg, db = guarded_vec(nout, torch.zeros(nout)), guarded_vec(nout, torch.zeros(nout))
        ops.conv_fwd(x, Wt, nout, out=out, bn_reduce=(zd, sc.to(DEV), sh.to(DEV), mu.to(DEV), ist.to(DEV), dg, db))
        kname = _lib.lib().adp_last_kernel().decode()
        torch.cuda.synchronize()
    assert kname.startswith(c["kernel"]), kname
    stored = CR.f64(out[..., :nout])
    CR.assert_exact(torch.cat([out[..., nout:].reshape(-1), otail, dg[nout:], db[nout:]]),
                    torch.full((N * H * W * 8 + otail.numel() + 16,), SENT), "guards")
    ref_dg, ref_db = CR.E.bn_bwd_reduce(stored, z, sc, sh, mu, ist)
    dbv = torch.where(CR.E.gate(z, sc, sh), stored, torch.zeros((), dtype=torch.float64)).abs()
    A_db = dbv.reshape(-1, nout).sum(0)
    xabs = CR.f64(z).abs() + CR.f64(mu).abs() if c["split_xhat"] else (CR.f64(z) - CR.f64(mu)).abs()
    A_dg = (dbv * xabs * CR.f64(ist).abs()).reshape(-1, nout).sum(0)
    rb_ = CR.assert_sum_gate(db[:nout], ref_db, A_db, K, "dbeta")
    rg = CR.assert_sum_gate(dg[:nout], ref_dg, A_dg, K, "dgamma")
    print(f"GATE {c['id']} K={K} dbeta={rb_:.3f} dgamma={rg:.3f}")
