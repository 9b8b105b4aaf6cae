#!/usr/bin/env python3
"""Microbenchmark of the bit-packed morphology calls (csrc/morph.hip): pack, dilate_bits, erode_bits, unpack and the
whole closing (u8 -> u8, and f32 + threshold -> f32), HIP-event timed on warm calls, at (8, 1024, 1024) and
(1, 8192, 8192), for adipocyte masks (data.synthetic_tile; the 8192^2 map is 8 x 8 different 1024^2 tiles side by side)
and the ellipse of k = 3, 5, 15, 31. One JSON line per size and k with the median over rounds of each call in
microseconds, the traffic floor of the closing at the HBM rate given by --hbm-gbps (u8 -> u8: 1 + 1 + 4/8 B per pixel,
the input, the output and the plane written and read twice; f32 -> f32: 4 + 4 + 4/8 B) and the ratio to it, and a
baseline that is none of the library's code, in the same process: the rect closing of the same k by
torch.nn.functional.max_pool2d(x, k, 1, k // 2) and its negation on a float plane (its -inf padding is the same
"outside takes no part" border; for odd k it equals close(..., shape="rect"), which is checked here on the way).

    python tools/bench_morph.py --sizes 8x1024x1024,1x8192x8192
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def adipocyte_masks(N, H, W):
    import numpy as np

    from adipose_amd.data import synthetic_tile
    T = 1024
    out = np.zeros((N, H, W), np.uint8)
    k = 0
    for n in range(N):
        for y in range(0, H, T):
            for x in range(0, W, T):
                _, m = synthetic_tile(np.random.default_rng(k), size=T, channels=1)
                out[n, y:y + T, x:x + T] = (m > 0.5)[:H - y, :W - x]
                k += 1
    return out


def timed(torch, fn, rounds, reps):
    """Microseconds per call: per round one warm call, then `reps` calls between two events."""
    out = []
    for _ in range(rounds):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps * 1e3)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--sizes", default="8x1024x1024,1x8192x8192")
    p.add_argument("--ks", default="3,5,15,31")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--baseline-rounds", type=int, default=3)
    p.add_argument("--baseline-reps", type=int, default=1)
    p.add_argument("--hbm-gbps", type=float, default=6300.0, help="HBM rate for the traffic floor (GB/s)")
    p.add_argument("--no-baseline", action="store_true")
    args = p.parse_args()
    import torch
    import torch.nn.functional as F

    import _adipose_pkg  # noqa: F401
    from adipose_amd import morphology as mo

    if not torch.cuda.is_available():
        raise SystemExit("bench_morph.py needs a GPU: there is nothing to time without one")
    for size in args.sizes.split(","):
        N, H, W = (int(v) for v in size.split("x"))
        host = adipocyte_masks(N, H, W)
        m = torch.from_numpy(host).cuda()
        prob = m.float() * 0.5 + 0.25   # 0.75 in the cells, 0.25 outside: the same mask at thr = 0.5
        bits = mo.pack(m)
        assert torch.equal(mo.pack(prob, threshold=0.5), bits)
        for k in (int(v) for v in args.ks.split(",")):
            rows = mo.footprint_rows(k, "ellipse")
            calls = {
                "pack": lambda: mo.pack(m),
                "pack_f32": lambda: mo.pack(prob, threshold=0.5),
                "dilate_bits": lambda: mo.dilate_bits(bits, W, rows),
                "erode_bits": lambda: mo.erode_bits(bits, W, rows),
                "unpack": lambda: mo.unpack(bits, W),
                "unpack_f32": lambda: mo.unpack(bits, W, torch.float32),
                "close_u8": lambda: mo.close(m, k),
                "close_f32": lambda: mo.close(prob, k, threshold=0.5, dtype=torch.float32),
            }
            line = {"size": size, "mask": "adipocyte", "k": k, "shape": "ellipse",
                    "distinct_extents": len(set(zip(*rows))), "foreground": round(float(host.mean()), 4),
                    "rounds": args.rounds, "reps": args.reps}
            for name, fn in calls.items():
                t = timed(torch, fn, args.rounds, args.reps)
                line[f"{name}_us"] = round(statistics.median(t), 1)
                line[f"{name}_us_min"] = round(min(t), 1)
            px = N * H * W
            for name, per_px in (("close_u8", 2.5), ("close_f32", 8.5)):
                floor = per_px * px / args.hbm_gbps / 1e3
                line[f"{name}_floor_us"] = round(floor, 1)
                line[f"{name}_over_floor"] = round(line[f"{name}_us"] / floor, 2)
            line["pixels_changed"] = int((mo.close(m, k) != m).sum().item())
            if not args.no_baseline:
                x = m.float()[:, None]

                def pool_close():
                    return -F.max_pool2d(-F.max_pool2d(x, k, 1, k // 2), k, 1, k // 2)

                t = timed(torch, pool_close, args.baseline_rounds, args.baseline_reps)
                line["maxpool_rect_close_us"] = round(statistics.median(t), 1)
                line["maxpool_rect_close_us_min"] = round(min(t), 1)
                line["close_u8_over_maxpool"] = round(line["close_u8_us"] / line["maxpool_rect_close_us"], 4)
                if k % 2:
                    line["rect_equals_maxpool"] = bool(torch.equal(
                        mo.close(m, k, "rect", dtype=torch.float32), pool_close()[:, 0]))
                del x
            print(json.dumps(line), flush=True)
        del m, prob, bits


if __name__ == "__main__":
    main()
