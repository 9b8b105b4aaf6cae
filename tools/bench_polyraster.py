#!/usr/bin/env python3
"""Microbenchmark of the polygon rasteriser (csrc/polyraster.hip, annotations.py) on a synthetic slide: SIZE x SIZE
(default 8192^2) with POLYGONS (default 3000) ellipse-like outlines of 40 .. 200 vertices, semi-axes 15 .. 160 pixels,
some of them across the slide's border. Three figures, in microseconds per call, as one JSON line each:

  adp_poly_raster  the library call on device buffers uploaded once (memset of the plane, toggle, row scan, boundary),
                   HIP-event timed: per round one warm call, then `reps` calls between two events; the median over the
                   rounds.
  numpy path       rasterize_np on the same polygons on this box's host; a host clock, the median over the rounds.
  floor            a memset of the plane plus one pass that reads and writes it (zero_ and an in-place bitwise_not of the
                   packed plane), timed the same way as the call: what zeroing and scanning a plane of this size costs
                   with no polygon in it.

The device result is checked for equality with the numpy path's on the way.

    python tools/bench_polyraster.py --size 8192 --polygons 3000
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def synthetic_polygons(np, size, count, seed=0):
    rng = np.random.default_rng(seed)
    polys = []
    for _ in range(count):
        n = int(rng.integers(40, 201))
        a, b = rng.uniform(15, 160, 2)
        cx, cy = rng.uniform(-40, size + 40, 2)
        t = np.sort(rng.uniform(0, 2 * np.pi, n)) + rng.uniform(0, 2 * np.pi)
        rad = 1.0 + 0.08 * rng.standard_normal(n)
        polys.append(np.stack([np.rint(cx + a * rad * np.cos(t)), np.rint(cy + b * rad * np.sin(t))], axis=1).astype(np.int64))
    return polys


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--size", type=int, default=8192)
    p.add_argument("--polygons", type=int, default=3000)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--reps", type=int, default=50)
    p.add_argument("--host-rounds", type=int, default=3)
    args = p.parse_args()
    import numpy as np
    import torch

    import _adipose_pkg  # noqa: F401
    from adipose_amd import annotations as an
    from adipose_amd import morphology as mo
    from adipose_amd._lib import call, ptr, stream_ptr

    if not torch.cuda.is_available():
        raise SystemExit("bench_polyraster.py needs a GPU: there is nothing to time without one")
    S = args.size
    polys = synthetic_polygons(np, S, args.polygons)
    xy, poly_off, img_off = an._flatten([polys])
    P, V = len(poly_off) - 1, len(xy)
    d_xy = torch.from_numpy(xy.astype(np.int32)).cuda()
    d_po = torch.from_numpy(poly_off.astype(np.int32)).cuda()
    d_io = torch.from_numpy(img_off.astype(np.int32)).cuda()
    bits = torch.empty((1, S, (S + 63) // 64), dtype=torch.int64, device="cuda")
    s = stream_ptr()
    size = f"{S}x{S}, {P} polygons, {V} edges"

    def device():
        call("adp_poly_raster", 1, S, S, ptr(d_xy), ptr(d_po), ptr(d_io), P, V, ptr(bits), s)

    def floor():
        bits.zero_()
        bits.bitwise_not_()

    device()
    got = bits.cpu().numpy().view(np.uint64)
    ht, want = [], None
    for _ in range(args.host_rounds):
        t0 = time.perf_counter()
        want = an.rasterize_np([polys], S, S)
        ht.append((time.perf_counter() - t0) * 1e6)
    same = bool(np.array_equal(got, mo.pack_np(want)))
    t = timed(torch, device, args.rounds, args.reps)
    us = statistics.median(t)
    print(json.dumps({"size": size, "case": "adp_poly_raster", "us": round(us, 1), "us_min": round(min(t), 1),
                      "ns_per_edge": round(us * 1e3 / max(V, 1), 2), "coverage": round(float(want.mean()), 3),
                      "rounds": args.rounds, "reps": args.reps, "equals_numpy": same}), flush=True)
    hus = statistics.median(ht)
    print(json.dumps({"size": size, "case": "rasterize_np (host)", "us": round(hus, 1), "us_min": round(min(ht), 1),
                      "rounds": args.host_rounds}), flush=True)
    ft = timed(torch, floor, args.rounds, args.reps)
    fus = statistics.median(ft)
    print(json.dumps({"size": size, "case": "floor (memset + one read-write pass of the plane)", "us": round(fus, 1),
                      "us_min": round(min(ft), 1), "plane_MB": round(bits.numel() * 8 / 1e6, 1)}), flush=True)


if __name__ == "__main__":
    main()
