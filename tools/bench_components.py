#!/usr/bin/env python3
"""Microbenchmark of the connected-component calls (csrc/components.hip): label, areas, filter, table and shape, HIP-event
timed on warm calls, at (8, 1024, 1024) and (1, 8192, 8192), for adipocyte masks (data.synthetic_tile; the 8192^2 map
is 8 x 8 different 1024^2 tiles side by side) and the contention / chain-length worst cases: all-foreground, the
4-connected checkerboard and the one-pixel serpentine. One JSON line per size and mask with the median over rounds of
each call in microseconds, their sum, the traffic floor of label + filter (1 + 4 + 4 + 1 B per pixel) at the HBM
rate given by --hbm-gbps, and scipy.ndimage.label on the host for the same input where scipy is present.

    python tools/bench_components.py --sizes 8x1024x1024,1x8192x8192
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def masks(name, N, H, W):
    import numpy as np
    if name == "adipocyte":
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
    if name == "ones":
        return np.ones((N, H, W), np.uint8)
    if name == "checkerboard":
        yy, xx = np.ogrid[0:H, 0:W]
        return np.broadcast_to(((yy + xx) % 2 == 0).astype(np.uint8), (N, H, W)).copy()
    if name == "serpentine":
        m = np.zeros((H, W), np.uint8)
        m[0::2] = 1
        m[1::4, -1] = 1
        m[3::4, 0] = 1
        return np.broadcast_to(m, (N, H, W)).copy()
    raise ValueError(name)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--sizes", default="8x1024x1024,1x8192x8192")
    p.add_argument("--masks", default="adipocyte,ones,checkerboard,serpentine")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--max-rows", type=int, default=4096)
    p.add_argument("--min-px", type=int, default=64)
    p.add_argument("--hbm-gbps", type=float, default=6300.0, help="HBM rate for the traffic floor (GB/s)")
    p.add_argument("--no-scipy", action="store_true")
    args = p.parse_args()
    import numpy as np
    import torch

    import _adipose_pkg  # noqa: F401
    from adipose_amd import components as cc

    for size in args.sizes.split(","):
        N, H, W = (int(v) for v in size.split("x"))
        for name in args.masks.split(","):
            conn = 4 if name == "checkerboard" else 8
            host = masks(name, N, H, W)
            m = torch.from_numpy(host).cuda()
            lab = cc.label(m, conn)
            area = cc.areas(lab)
            calls = {
                "label": lambda: cc.label(m, conn),
                "areas": lambda: cc.areas(lab),
                "filter": lambda: cc.filter_small(lab, area, args.min_px),
                "table": lambda: cc.table(lab, args.max_rows),
                "shape": lambda: cc.shape_table(lab, args.max_rows),
            }
            res = {k: [] for k in calls}
            for _ in range(args.rounds):
                for k, fn in calls.items():
                    fn()   # warm (and the workspace has its size)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.reps):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    res[k].append(e0.elapsed_time(e1) / args.reps * 1e3)
            _, counts = cc.table(lab, 0)
            line = {"size": size, "mask": name, "connectivity": conn, "components": int(counts.sum().item()),
                    "foreground": round(float(host.mean()), 4)}
            for k in calls:
                line[f"{k}_us"] = round(statistics.median(res[k]), 1)
                line[f"{k}_us_min"] = round(min(res[k]), 1)
            line["sum_us"] = round(sum(line[f"{k}_us"] for k in calls), 1)
            floor_bytes = 10 * N * H * W
            line["floor_bytes_label_filter"] = floor_bytes
            line["floor_us"] = round(floor_bytes / args.hbm_gbps / 1e3, 1)
            line["label_filter_over_floor"] = round((line["label_us"] + line["filter_us"]) / line["floor_us"], 2)
            if name == "ones":   # atomics issued per address by the areas call: one per tile of 64 x 256 of an image
                line["area_atomics_per_address"] = -(-H // 64) * -(-W // 256)
                line["shape_atomics_per_address"] = -(-H // cc.SHAPE_TILE_ROWS) * -(-W // cc.SHAPE_TILE_COLS)
            if not args.no_scipy:
                try:
                    import scipy.ndimage as ndi
                    st = np.ones((3, 3), int) if conn == 8 else None
                    t0 = time.perf_counter()
                    for n in range(N):
                        ndi.label(host[n], structure=st)
                    line["scipy_label_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                except ImportError:
                    pass
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
