#!/usr/bin/env python3
"""Microbenchmark of the CLAHE calls (csrc/clahe.hip): clahe_hist, clahe_lut, clahe_apply and the whole clahe (u8 -> u8),
HIP-event timed on warm calls, at (1, 6144, 6144) on a 16 x 16 grid with clip limit 3.0 (a whole ECM image, as
preprocess_small_MS_SIMs.py enhances it) and at (8, 1024, 1024) on 8 x 8 with 2.0 (a batch of tiles, enhance_clahe's
defaults). Each case runs on a seeded random image and on a constant image: the constant image is the worst case of the
histogram's LDS atomics (every lane counts the same bin) and the best case of its merging of equal values.

One JSON line per case and image with the median over rounds of each stage and of the whole call in microseconds, the
effective GB/s of the whole call against 3 bytes per pixel (the image read twice, by the histogram and by the
interpolation, and written once), and two yardsticks that are none of the library's code, from the same run: a device
uint8 -> uint8 copy of the same size (torch's copy_: 2 bytes per pixel, the floor of any pass that reads and writes the
image) and the numpy path on the host (skipped with --no-host; it is checked against the device on the way).

    python tools/bench_clahe.py
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = (((1, 6144, 6144), 16, 3.0), ((8, 1024, 1024), 8, 2.0))


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
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--no-host", action="store_true", help="skip the numpy path on the host")
    args = p.parse_args()
    import numpy as np
    import torch

    import _adipose_pkg  # noqa: F401
    from adipose_amd import contrast as ct

    if not torch.cuda.is_available():
        raise SystemExit("bench_clahe.py needs a GPU: there is nothing to time without one")
    for shape, grid, clip in CASES:
        N, H, W = shape
        g = (grid, grid)
        _, _, th, tw = ct.clahe_geometry(H, W, g)
        images = {"random": np.random.default_rng(N * 7 + H).integers(0, 256, shape, dtype=np.uint8),
                  "constant": np.full(shape, 243, np.uint8)}
        for kind, host in images.items():
            d = torch.from_numpy(host).cuda()
            hist = ct.clahe_hist(d, g)
            lut = ct.clahe_lut(hist, th * tw, clip)
            other = torch.empty_like(d)
            calls = {
                "hist": lambda: ct.clahe_hist(d, g),
                "lut": lambda: ct.clahe_lut(hist, th * tw, clip),
                "apply": lambda: ct.clahe_apply(d, lut, g),
                "clahe": lambda: ct.clahe(d, clip, g),
                "copy_u8": lambda: other.copy_(d),
            }
            line = {"size": "x".join(map(str, shape)), "image": kind, "grid": grid, "clip_limit": clip, "tile": [th, tw],
                    "rounds": args.rounds, "reps": args.reps}
            for name, fn in calls.items():
                t = timed(torch, fn, args.rounds, args.reps)
                line[f"{name}_us"] = round(statistics.median(t), 1)
                line[f"{name}_us_min"] = round(min(t), 1)
            px = N * H * W
            line["clahe_gbps_3B_per_px"] = round(3 * px / line["clahe_us"] / 1e3, 1)
            line["copy_gbps_2B_per_px"] = round(2 * px / line["copy_u8_us"] / 1e3, 1)
            line["clahe_over_copy"] = round(line["clahe_us"] / line["copy_u8_us"], 2)
            if not args.no_host:
                t0 = time.perf_counter()
                want = ct.clahe_np(host, clip, g)
                line["numpy_host_us"] = round((time.perf_counter() - t0) * 1e6, 1)
                line["equals_numpy"] = bool(np.array_equal(ct.clahe(d, clip, g).cpu().numpy(), want))
                line["numpy_over_clahe"] = round(line["numpy_host_us"] / line["clahe_us"], 1)
                del want
            print(json.dumps(line), flush=True)
            del d, hist, lut, other


if __name__ == "__main__":
    main()
