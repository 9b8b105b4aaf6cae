#!/usr/bin/env python3
"""Microbenchmark of the per-tile fat counts (csrc/tilefat.hip, tile_classification.py) for N tiles of SIZE x SIZE
(default 8 of 1024^2): three figures, each in microseconds per tile, as one JSON line each:

  adp_fat_counts   the library call on device buffers allocated once (memset of the N x 32 result bytes and one launch),
                   HIP-event timed: per round one warm call, then `reps` calls between two events; the median over the
                   rounds. bytes_per_px = 5 (one float32 map and one uint8 mask are read) gives GB_per_s.
  host path        the same four integers the only way they could be had before the kernel: .cpu() of the float32 maps
                   and of the masks, then fat_counts_ref (numpy); a host clock around it (the copy synchronises), the
                   median over the rounds.
  copy bound       5 bytes per pixel over the device copy rate measured in the same run (clone of a float32 plane of the
                   same size: it reads and writes, so its rate is 8 bytes per pixel over its time).

The device result is checked for equality with the host path's on the way. Histology-like probability maps do not
matter to a counting kernel; the maps are seeded uniform values, the masks seeded 0 / 255.

    python tools/bench_tilefat.py --tiles 8 --size 1024
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


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--tiles", type=int, default=8)
    p.add_argument("--size", type=int, default=1024)
    p.add_argument("--threshold", type=float, default=0.5)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--reps", type=int, default=500)
    p.add_argument("--host-rounds", type=int, default=5)
    args = p.parse_args()
    import numpy as np
    import torch

    import _adipose_pkg  # noqa: F401
    from adipose_amd import tile_classification as tc
    from adipose_amd._lib import call, ptr, stream_ptr

    if not torch.cuda.is_available():
        raise SystemExit("bench_tilefat.py needs a GPU: there is nothing to time without one")
    N, S = args.tiles, args.size
    n_px = S * S
    rng = np.random.default_rng(0)
    maps = torch.from_numpy(rng.random((N, S, S), dtype=np.float32)).cuda()
    masks = torch.from_numpy(((rng.random((N, S, S)) < 0.3) * 255).astype(np.uint8)).cuda()
    out = torch.empty((N, 4), dtype=torch.int64, device="cuda")
    cut_raw, cut_scaled = tc.gt_cuts(args.threshold)
    thr, s = float(np.float32(args.threshold)), stream_ptr()
    size = f"{N}x{S}x{S}"

    def device():
        call("adp_fat_counts", N, n_px, ptr(maps), thr, ptr(masks), cut_raw, cut_scaled, ptr(out), s)

    def host():
        return tc.fat_counts_ref(maps.cpu().numpy(), masks.cpu().numpy(), args.threshold)

    device()
    same = bool(np.array_equal(out.cpu().numpy().view(np.uint64), host()))
    t = timed(torch, device, args.rounds, args.reps)
    us = statistics.median(t)
    print(json.dumps({"size": size, "case": "adp_fat_counts", "us_per_tile": round(us / N, 2), "us": round(us, 1),
                      "us_min": round(min(t), 1), "bytes_per_px": 5, "GB_per_s": round(5 * N * n_px / us / 1e3, 1),
                      "rounds": args.rounds, "reps": args.reps, "equals_host": same}), flush=True)
    # one plane at a time: what each costs (a block then issues one atomic, or up to three)
    for case, a, b, bpp in (("adp_fat_counts, maps only", maps, None, 4), ("adp_fat_counts, masks only", None, masks, 1)):
        t = timed(torch, lambda: call("adp_fat_counts", N, n_px, ptr(a), thr, ptr(b), cut_raw, cut_scaled, ptr(out), s),
                  args.rounds, args.reps)
        us1 = statistics.median(t)
        print(json.dumps({"size": size, "case": case, "us_per_tile": round(us1 / N, 2), "us": round(us1, 1),
                          "bytes_per_px": bpp, "GB_per_s": round(bpp * N * n_px / us1 / 1e3, 1)}), flush=True)
    ht = []
    for _ in range(args.host_rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host()
        ht.append((time.perf_counter() - t0) * 1e6)
    hus = statistics.median(ht)
    print(json.dumps({"size": size, "case": ".cpu() + fat_counts_ref (host)", "us_per_tile": round(hus / N, 1),
                      "us": round(hus, 1), "us_min": round(min(ht), 1), "rounds": args.host_rounds}), flush=True)
    ct = timed(torch, lambda: maps.clone(), args.rounds, args.reps)
    cus = statistics.median(ct)
    rate = 8 * N * n_px / cus / 1e3   # GB/s: a clone reads and writes 4 bytes per pixel
    print(json.dumps({"size": size, "case": "copy bound (5 bytes per pixel at the clone's rate)",
                      "us_per_tile": round(5 * n_px / rate / 1e3, 2), "clone_us": round(cus, 1),
                      "clone_GB_per_s": round(rate, 1)}), flush=True)


if __name__ == "__main__":
    main()
