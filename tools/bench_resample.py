#!/usr/bin/env python3
"""Microbenchmark of the Pillow-exact resampling (csrc/resample.hip, resample.py): the library call adp_resample_u8 on
buffers and tables made once, for an 8192^2 gray and RGB image and four target sizes -- the ECM case (a few pixels off
in each extent), 2 x up, 1 / 4 and 1 / 16 down -- in both forms: the two launches through an intermediate (option
resample_fused = 0) and the fused launch (1; where its footprint does not admit the size the line says so and is not
timed). HIP-event timed on warm calls; a call includes the upload of its coefficient tables. One JSON line per case
with the median over rounds in milliseconds, the bytes moved (input + output, and the intermediate written and read in
the two-launch form), GB/s, and PIL.Image.resize's time on the host for the same call. Every device result is checked
for equality with Pillow's on the way.

    python tools/bench_resample.py --size 8192 --filter lanczos
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
    """Milliseconds per call: per round one warm call, then `reps` calls between two events."""
    out = []
    for _ in range(rounds):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--size", type=int, default=8192, help="the source is size x size")
    p.add_argument("--filter", default="lanczos")
    p.add_argument("--channels", default="1,3")
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--no-pillow", action="store_true", help="skip Pillow's time and the comparison with it")
    args = p.parse_args()
    import numpy as np
    import torch
    from PIL import Image

    import _adipose_pkg  # noqa: F401
    from adipose_amd import ops
    from adipose_amd import resample as R
    from adipose_amd._lib import call, ptr, stream_ptr

    if not torch.cuda.is_available():
        raise SystemExit("bench_resample.py needs a GPU: there is nothing to time without one")
    Image.MAX_IMAGE_PIXELS = None
    S, f = args.size, args.filter
    targets = [("ecm", (S - 5, S + 3)), ("up 2x", (2 * S, 2 * S)), ("down 1/4", (S // 4, S // 4)), ("down 1/16", (S // 16, S // 16))]
    s = stream_ptr()
    for C in (int(c) for c in args.channels.split(",")):
        host = np.random.default_rng(C).integers(0, 256, (S, S) if C == 1 else (S, S, C), dtype=np.uint8)
        src = torch.from_numpy(host).cuda()
        for name, (Wo, Ho) in targets:
            pil_ms, want = None, None
            if not args.no_pillow:
                im = Image.fromarray(host)
                t0 = time.perf_counter()
                res = im.resize((Wo, Ho), getattr(Image.Resampling, f.upper()))
                pil_ms = round((time.perf_counter() - t0) * 1e3, 1)
                want = np.asarray(res)
            xb, xk, xks = R.coefficients(S, Wo, f)
            yb, yk, yks = R.coefficients(S, Ho, f)
            dst = torch.empty((Ho, Wo) if C == 1 else (Ho, Wo, C), dtype=torch.uint8, device="cuda")
            tmp = torch.empty(S * Wo * C, dtype=torch.uint8, device="cuda")
            fits = R.fused_fits(S, S, C, Ho, Wo, f)
            io = S * S * C + Ho * Wo * C
            for form in (0, 1):
                line = {"size": f"{S}x{S}x{C}", "to": f"{Wo}x{Ho}", "case": name, "filter": f, "taps": [xks, yks],
                        "form": "fused" if form else "two launches", "pillow_ms": pil_ms}
                if form and not fits:
                    line["ms"] = None
                    line["note"] = "the tile's rows do not fit ADP_RESAMPLE_LDS_BYTES: the call takes the two launches"
                    print(json.dumps(line), flush=True)
                    continue
                ops.set_option("resample_fused", form)

                def fn():
                    call("adp_resample_u8", 1, S, S, C, Ho, Wo, ptr(src), R._host_ptr(xb), R._host_ptr(xk), xks, R._host_ptr(yb),
                         R._host_ptr(yk), yks, ptr(tmp), ptr(dst), s)
                t = timed(torch, fn, args.rounds, args.reps)
                moved = io + (0 if form else 2 * S * Wo * C)
                line.update(ms=round(statistics.median(t), 4), ms_min=round(min(t), 4), bytes=moved,
                            GB_per_s=round(moved / statistics.median(t) / 1e6, 1), rounds=args.rounds, reps=args.reps)
                if want is not None:
                    line["equals_pillow"] = bool(np.array_equal(dst.cpu().numpy(), want))
                    line["pillow_over_device"] = round(pil_ms / line["ms"], 1)
                print(json.dumps(line), flush=True)
            ops.set_option("resample_fused", None)
            del dst, tmp
        del src


if __name__ == "__main__":
    main()
