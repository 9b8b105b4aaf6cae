#!/usr/bin/env python3
"""Microbenchmark of the unsharp mask (csrc/sharpen.hip, sharpen.py): the library call adp_gray_sharpen on buffers
allocated once, per sigma (default 1, 4 and 16: radius 4 and 16 are the fused launch, radius 64 the two launches through
the plane of row sums) with uint8 in and out, adp_gray_blur (the int64 sums), the entry point sharpen() with float32 in
and out as the predictor calls it, and, from the same run, adp_gray_colnorm at the same shape: an existing kernel with
the same traffic of one byte in and one byte out per pixel. HIP-event timed on warm calls for histology-like gray tiles
(data.synthetic_tile). One JSON line per size and case with the median over rounds in microseconds and the bytes per
second of the pixel traffic (bytes_per_px x pixels / time; the two-launch form also writes and reads 4-byte row sums,
counted in its bytes_per_px), beside a u8 copy of the plane in the same process and the numpy path on the host for one
1024^2 tile. Every device result is checked for equality with the numpy path on the way.

    python tools/bench_sharpen.py --sizes 8x1024x1024 --sigmas 1,4,16
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
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


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
    p.add_argument("--sizes", default="8x1024x1024")
    p.add_argument("--sigmas", default="1,4,16")
    p.add_argument("--amount", type=float, default=0.5)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--no-check", action="store_true", help="skip the comparison with the numpy path")
    args = p.parse_args()
    import numpy as np
    import torch

    import _adipose_pkg  # noqa: F401
    from adipose_amd import normalization as nm
    from adipose_amd import sharpen as sh
    from adipose_amd._lib import call, ptr, stream_ptr

    if not torch.cuda.is_available():
        raise SystemExit("bench_sharpen.py needs a GPU: there is nothing to time without one")
    sigmas = [float(v) for v in args.sigmas.split(",")]
    one = gray_images(1, 1024, 1024)[0]
    for sigma in sigmas:
        t0 = time.perf_counter()
        sh.sharpen_np(one, sigma, args.amount)
        print(json.dumps({"size": "1x1024x1024", "case": f"numpy sharpen sigma {sigma:g} (host)",
                          "us": round((time.perf_counter() - t0) * 1e6, 1)}), flush=True)
    for size in args.sizes.split(","):
        N, H, W = (int(v) for v in size.split("x"))
        host = gray_images(N, H, W)
        m = torch.from_numpy(host).cuda()
        copy_us = round(statistics.median(timed(torch, lambda: m.clone(), args.rounds, args.reps)), 1)

        def emit(case, fn, bytes_per_px=None, **extra):
            t = timed(torch, fn, args.rounds, args.reps)
            line = {"size": size, "case": case, "us": round(statistics.median(t), 1), "us_min": round(min(t), 1),
                    "u8_copy_us": copy_us, "rounds": args.rounds, "reps": args.reps}
            line["over_copy"] = round(line["us"] / copy_us, 2)
            if bytes_per_px is not None:
                line["bytes_per_px"] = bytes_per_px
                line["GB_per_s"] = round(bytes_per_px * N * H * W / line["us"] / 1e3, 1)
            line.update(extra)
            print(json.dumps(line), flush=True)

        s = stream_ptr()
        out = torch.empty_like(m)
        # the yardstick: adp_gray_colnorm, one byte in and one byte out per pixel
        col, glob = nm.column_stats(m)
        emit("adp_gray_colnorm", lambda: call("adp_gray_colnorm", N, H, W, ptr(m), 0, ptr(col), ptr(glob), 1, ptr(out), 0, s),
             bytes_per_px=2)
        del col, glob
        rowbuf = torch.empty((N, H, W), dtype=torch.int32, device="cuda")
        Sout = torch.empty((N, H, W), dtype=torch.int64, device="cuda")
        f = m.float()
        for sigma in sigmas:
            q = sh.taps(sigma)
            r, qa = len(q) - 1, sh._taps_arg(q)
            launches = 1 if r <= sh.FUSED_RMAX else 2
            same = None
            if not args.no_check:
                same = bool(np.array_equal(sh.sharpen(m, sigma, args.amount).cpu().numpy(), sh.sharpen_np(host, sigma, args.amount)))
            emit(f"adp_gray_sharpen sigma {sigma:g}", lambda: call("adp_gray_sharpen", N, H, W, ptr(m), 0, qa, r, args.amount,
                                                                    ptr(rowbuf), ptr(out), 0, s),
                 bytes_per_px=2 if launches == 1 else 11, radius=r, launches=launches, equals_numpy=same)
            emit(f"adp_gray_blur sigma {sigma:g}", lambda: call("adp_gray_blur", N, H, W, ptr(m), 0, qa, r, ptr(rowbuf), ptr(Sout), s),
                 bytes_per_px=9 if launches == 1 else 17, radius=r, launches=launches)
            emit(f"sharpen() sigma {sigma:g} f32 in/out", lambda: sh.sharpen(f, sigma, args.amount),
                 bytes_per_px=8 if launches == 1 else 20, radius=r, launches=launches)
        del m, f, out, rowbuf, Sout


if __name__ == "__main__":
    main()
