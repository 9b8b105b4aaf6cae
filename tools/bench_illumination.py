#!/usr/bin/env python3
"""Microbenchmark of the gray-scale morphology calls (csrc/graymorph.hip) and the background corrections built on them
(illumination.py): erode and open by the ellipses of 31 and 301, the disc of radius 100, the 512 x 1 line and the
301 x 301 rectangle, and the three corrections at the reference's defaults (rolling ball r = 100, banding 1 x 512,
top-hat 301), HIP-event timed on warm calls, at (8, 1024, 1024) and (1, 6144, 6144), for histology-like gray tiles
(data.synthetic_tile; the 6144^2 image is 6 x 6 different 1024^2 tiles side by side under a smooth illumination ramp).
One JSON line per size and case with the median over rounds in microseconds, beside two baselines that are none of the
library's code, in the same process: a u8 copy of the plane (the traffic floor of any pass), and, for the odd
rectangle, the same erosion / opening by torch.nn.functional.max_pool2d on a float plane, in its separable form
((k, 1) then (1, k); its -inf padding is the same "outside takes no part" border), which is checked for equality with the
rect result on the way.

    python tools/bench_illumination.py --sizes 8x1024x1024,1x6144x6144
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def gray_images(N, H, W):
    import numpy as np

    from adipose_amd.data import synthetic_tile
    T = 1024
    out = np.zeros((N, H, W), np.float32)
    k = 0
    for n in range(N):
        for y in range(0, H, T):
            for x in range(0, W, T):
                img, _ = synthetic_tile(np.random.default_rng(k), size=T, channels=1)
                out[n, y:y + T, x:x + T] = np.asarray(img, np.float32).reshape(T, T)[:H - y, :W - x]
                k += 1
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = 0.75 + 0.25 * (yy / max(H - 1, 1)) * (xx / max(W - 1, 1))   # uneven illumination
    return np.clip(np.rint(out * ramp[None]), 0, 255).astype(np.uint8)


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
    p.add_argument("--sizes", default="8x1024x1024,1x6144x6144")
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--no-baseline", action="store_true")
    args = p.parse_args()
    import torch
    import torch.nn.functional as F

    import _adipose_pkg  # noqa: F401
    from adipose_amd import illumination as il

    if not torch.cuda.is_available():
        raise SystemExit("bench_illumination.py needs a GPU: there is nothing to time without one")
    foots = [("ellipse31", il.ellipse_rows(31)), ("ellipse301", il.ellipse_rows(301)), ("disc100", il.disc_rows(100)),
             ("line512x1", il.rect_rows(512, 1)), ("rect301x301", il.rect_rows(301, 301))]
    # what a user without the device path does today: the numpy path on the host, one 1024^2 tile
    import time
    one = gray_images(1, 1024, 1024)
    t0 = time.perf_counter()
    il.open_np(one, il.ellipse_rows(301))
    print(json.dumps({"size": "1x1024x1024", "case": "numpy open ellipse301 (host)",
                      "us": round((time.perf_counter() - t0) * 1e6, 1)}), flush=True)
    for size in args.sizes.split(","):
        N, H, W = (int(v) for v in size.split("x"))
        m = torch.from_numpy(gray_images(N, H, W)).cuda()
        copy_us = round(statistics.median(timed(torch, lambda: m.clone(), args.rounds, 20)), 1)

        def emit(case, fn, **extra):
            t = timed(torch, fn, args.rounds, args.reps)
            line = {"size": size, "case": case, "us": round(statistics.median(t), 1), "us_min": round(min(t), 1),
                    "u8_copy_us": copy_us, "rounds": args.rounds, "reps": args.reps}
            line["over_copy"] = round(line["us"] / copy_us, 1)
            line.update(extra)
            print(json.dumps(line), flush=True)
            return line

        for name, rows in foots:
            lo, hi = rows[0], rows[1]
            info = {"rows": len(lo), "offsets": sum(h - l for l, h in zip(lo, hi))}
            e = emit(f"erode {name}", lambda: il.erode(m, rows), **info)
            o = emit(f"open {name}", lambda: il.open(m, rows), **info)
            if name == "rect301x301" and not args.no_baseline:
                k = 301
                x = m.float()[:, None]

                def pool_max(v):
                    return F.max_pool2d(F.max_pool2d(v, (k, 1), 1, (k // 2, 0)), (1, k), 1, (0, k // 2))

                def pool_erode():
                    return -pool_max(-x)

                def pool_open():
                    return pool_max(-pool_max(-x))

                same = bool(torch.equal(il.erode(m, rows, torch.float32), pool_erode()[:, 0])
                            and torch.equal(il.open(m, rows, torch.float32), pool_open()[:, 0]))
                for case, fn, ours in (("max_pool2d erode rect301x301", pool_erode, e), ("max_pool2d open rect301x301", pool_open, o)):
                    t = timed(torch, fn, 2, 1)
                    print(json.dumps({"size": size, "case": case, "us": round(statistics.median(t), 1), "us_min": round(min(t), 1),
                                      "ours_us": ours["us"], "ours_over_maxpool": round(ours["us"] / statistics.median(t), 3),
                                      "rect_equals_maxpool": same}), flush=True)
                del x
        emit("rolling_ball r=100", lambda: il.rolling_ball(m, 100))
        emit("remove_banding 1x512", lambda: il.remove_banding_morphological(m, 1, 512))
        emit("tophat_correction 301", lambda: il.tophat_correction(m, 301))
        f = m.float()
        emit("rolling_ball r=100 f32 in/out", lambda: il.rolling_ball(f, 100))
        del m, f


if __name__ == "__main__":
    main()
