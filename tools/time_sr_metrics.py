#!/usr/bin/env python
"""Time the SR metrics (srbh_amd.sr_metrics: one-read libsrbh kernels) against the same formulas with stock torch ops on the device
(tests/sr_metrics_oracle.py: what a user had before sr_metrics.py existed).

    python tools/time_sr_metrics.py [--out profiles/sr_metrics_bench.txt] [--runs 20] [--batch 8] [--size 256]

Per function: HIP-event time of one call, median of --runs after warm-up, and the number of device kernels one call launches (torch.profiler).
sr is a channels_last tensor (what net_g.forward returns), gt NCHW; B = 8, 3 x 256 x 256 is the SR stage's batch-8 output.  A stock path
the device's libraries cannot run (float64 convolution) is recorded as such, not skipped silently."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from srbh_amd import sr_metrics as M  # noqa: E402
from tests import sr_metrics_oracle as H  # noqa: E402


def time_ms(fn, runs, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
        return str(n) if n else "n/a"
    except Exception as e:      # noqa: BLE001  (a profiler that cannot attach must not lose the timings)
        return "n/a (%s)" % type(e).__name__


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sr_metrics_bench.txt"))
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    args = ap.parse_args()
    assert args.runs >= 20, "the median is taken over at least 20 runs"
    shape = (args.batch, 3, args.size, args.size)
    sr, gt = H.pair(shape, seed=16)
    sr = sr.cuda().contiguous(memory_format=torch.channels_last)
    gt = gt.cuda()
    rows = []
    pairs = [("calculate_psnr_pt", M.calculate_psnr_pt, H.calculate_psnr_pt), ("calculate_ssim_pt", M.calculate_ssim_pt, H.calculate_ssim_pt),
             ("calculate_cpsnr_pt", M.calculate_cpsnr_pt, H.calculate_cpsnr_pt)]
    for name, ours, stock in pairs:
        for y in (False, True):
            cols = []
            for fn in (lambda: ours(sr, gt, 4, y), lambda: stock(sr, gt, 4, y)):
                try:
                    med, lo, hi = time_ms(fn, args.runs)
                    cols.append("%9.3f ms (min %8.3f, max %8.3f), %5s launches" % (med, lo, hi, launches(fn)))
                except RuntimeError as e:
                    cols.append("not runnable on this device: %s" % str(e).splitlines()[0][:90])
            rows.append("%-20s y=%d | libsrbh %s | stock ops %s" % (name, int(y), cols[0], cols[1]))
            print(rows[-1], flush=True)
    q = M.SRQuality(crop_border=4, device="cuda")
    med, lo, hi = time_ms(lambda: q.addBatch(sr, gt), args.runs)
    rows.append("%-20s y=0 | libsrbh %9.3f ms (min %8.3f, max %8.3f), %5s launches | (all three metrics per image, two kernel calls)"
                % ("SRQuality.addBatch", med, lo, hi, launches(lambda: q.addBatch(sr, gt))))
    print(rows[-1], flush=True)
    head = ["SR metrics, %s, crop_border 4, sr channels_last / gt NCHW, fp32; device %s" % (shape, torch.cuda.get_device_name(0)),
            "HIP-event time of one call, median of %d runs after 3 warm-up calls; launches = device kernels of one call (torch.profiler)" % args.runs,
            "stock ops = the same formulas (tests/sr_metrics_oracle.py, float64) on the device", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(head + rows) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
