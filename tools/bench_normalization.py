#!/usr/bin/env python3
"""Microbenchmark of the statistical gray-image steps (csrc/graynorm.hip, normalization.py): the four device entry
points (column_stats, column_normalize, zscore, percentile), their library calls one by one (the statistics pass
adp_gray_colstats, the element-wise adp_gray_colnorm, the histogram adp_clahe_hist on a 1 x 1 grid, the table pass
adp_gray_normalize), and the two composed CLI settings (--banding-method column with --normalization-method percentile
or zscore, i.e. GrayNormalization called as a whole), HIP-event timed on warm calls, at (8, 1024, 1024) and
(1, 6144, 6144), for histology-like gray tiles (data.synthetic_tile; the 6144^2 image is 6 x 6 different 1024^2 tiles
side by side under a smooth illumination ramp and a column-wise banding profile). One JSON line per size and case with
the median over rounds in microseconds, beside a u8 copy of the plane in the same process (the traffic floor of a pass
that reads and writes a byte per pixel) and the numpy path on the host for one 1024^2 tile. Every device result is
checked for equality with the numpy path on the way.

    python tools/bench_normalization.py --sizes 8x1024x1024,1x6144x6144
"""
import argparse
import json
import os
import statistics
import sys
import time

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
    bands = 1 + 0.1 * np.sin(np.arange(W) / 7.0)                       # vertical banding
    return np.clip(np.rint(out * ramp[None] * bands[None, None, :]), 0, 255).astype(np.uint8)


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
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--no-check", action="store_true", help="skip the comparison with the numpy path")
    args = p.parse_args()
    import numpy as np
    import torch

    import _adipose_pkg  # noqa: F401
    from adipose_amd import normalization as nm
    from adipose_amd._lib import call, ptr, stream_ptr

    if not torch.cuda.is_available():
        raise SystemExit("bench_normalization.py needs a GPU: there is nothing to time without one")
    cases = [("column_normalize preserve_global", lambda t: nm.column_normalize(t, True), lambda a: nm.column_normalize_np(a, True)),
             ("column_normalize to 0..255", lambda t: nm.column_normalize(t, False), lambda a: nm.column_normalize_np(a, False)),
             ("zscore", nm.zscore, nm.normalize_zscore_np),
             ("percentile 1-99", nm.percentile, nm.normalize_percentile_np)]
    composed = [("cli: column + percentile", nm.GrayNormalization(True, True, "percentile")),
                ("cli: column + zscore", nm.GrayNormalization(True, True, "zscore"))]
    # what a user without the device path does: the numpy path on the host, one 1024^2 tile
    one = gray_images(1, 1024, 1024)[0]
    for name, _, np_fn in [("column_stats", None, nm.column_stats_np)] + cases:
        t0 = time.perf_counter()
        np_fn(one)
        print(json.dumps({"size": "1x1024x1024", "case": f"numpy {name} (host)",
                          "us": round((time.perf_counter() - t0) * 1e6, 1)}), flush=True)
    for size in args.sizes.split(","):
        N, H, W = (int(v) for v in size.split("x"))
        host = gray_images(N, H, W)
        m = torch.from_numpy(host).cuda()
        copy_us = round(statistics.median(timed(torch, lambda: m.clone(), args.rounds, args.reps)), 1)

        def emit(case, fn, **extra):
            t = timed(torch, fn, args.rounds, args.reps)
            line = {"size": size, "case": case, "us": round(statistics.median(t), 1), "us_min": round(min(t), 1),
                    "u8_copy_us": copy_us, "rounds": args.rounds, "reps": args.reps}
            line["over_copy"] = round(line["us"] / copy_us, 2)
            line.update(extra)
            print(json.dumps(line), flush=True)

        # the library calls one by one, on buffers allocated once
        s = stream_ptr()
        sums = torch.empty((N, W, 2), dtype=torch.int64, device="cuda")
        mm = torch.empty((N, W, 2), dtype=torch.int32, device="cuda")
        col = torch.empty((N, W, 2), dtype=torch.float64, device="cuda")
        glob = torch.empty((N, 4), dtype=torch.float64, device="cuda")
        hist = torch.empty((N, 256), dtype=torch.int32, device="cuda")
        out = torch.empty_like(m)
        emit("adp_gray_colstats", lambda: call("adp_gray_colstats", N, H, W, ptr(m), 0, ptr(sums), ptr(mm), s), bytes_per_px=1)
        emit("adp_gray_colparams", lambda: call("adp_gray_colparams", N, H, W, ptr(sums), ptr(mm), ptr(col), ptr(glob), s))
        emit("adp_gray_colnorm", lambda: call("adp_gray_colnorm", N, H, W, ptr(m), 0, ptr(col), ptr(glob), 1, ptr(out), 0, s),
             bytes_per_px=2)
        emit("adp_clahe_hist 1x1", lambda: call("adp_clahe_hist", N, H, W, ptr(m), 0, 1, 1, ptr(hist), s), bytes_per_px=1)
        emit("adp_gray_normalize zscore", lambda: call("adp_gray_normalize", N, H * W, ptr(m), 0, ptr(hist), nm.ZSCORE, 1.0, 99.0,
                                                       ptr(out), 0, s), bytes_per_px=2)
        emit("adp_gray_normalize percentile", lambda: call("adp_gray_normalize", N, H * W, ptr(m), 0, ptr(hist), nm.PERCENTILE, 1.0,
                                                           99.0, ptr(out), 0, s), bytes_per_px=2)
        del sums, mm, col, glob, hist, out
        # the entry points
        same = None
        if not args.no_check:
            c, g = nm.column_stats(m)
            wc, wg = nm.column_stats_np(host)
            same = bool(np.array_equal(c.cpu().numpy().view(np.int64), wc.view(np.int64))
                        and np.array_equal(g.cpu().numpy().view(np.int64), wg.view(np.int64)))
        emit("column_stats", lambda: nm.column_stats(m), equals_numpy=same)
        for name, d_fn, np_fn in cases:
            same = None if args.no_check else bool(np.array_equal(d_fn(m).cpu().numpy(), np_fn(host)))
            emit(name, lambda: d_fn(m), equals_numpy=same)
        f = m.float()
        emit("column_normalize preserve_global f32 in/out", lambda: nm.column_normalize(f, True))
        emit("percentile 1-99 f32 in/out", lambda: nm.percentile(f))
        del f
        for name, gn in composed:
            emit(name, lambda: gn(m))
        del m


if __name__ == "__main__":
    main()
