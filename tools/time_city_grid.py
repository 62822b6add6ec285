#!/usr/bin/env python
"""Time the per-cell counts of a city's grid (city_grid.cell_counts, srbh_cell_counts) against what a user writes without it, in ONE
process.

    python tools/time_city_grid.py [--out profiles/city_grid_bench.txt] [--rounds 5] [--calls 10] [--loop-calls 2]

Workloads: a 4000 x 3000 uint8 footprint mask (the median-city size) with its 3 888 fishnet windows of 64 / 56, and a 7900 x 7900 mask
with its 19 881 windows (the 20 000-cell city of the sizing example).
  (a) cell_counts(mask, pos_dev): one srbh_cell_counts launch (the windows already on the device, as fishgrid_stats leaves them after its
      upload); (a') the same with host windows: validation, upload and launch;
  (b) what a user writes today: torch.stack([(m[y:y+h, x:x+w] > 0).sum() for x, y, w, h in pos]);
  (c) the best stock form: an int64 integral image of (mask > 0) (cumsum twice) and four gathers per window;
  (d) the compare form, cell_counts(mask, pos_dev, other): two rasters, [n_a, n_b, n_and, count].
HIP events around ONE call each (for (b) the whole loop); every side warmed up, then --rounds alternations of --calls calls per side
(--loop-calls for (b)); the median of the rounds' medians with the range of the rounds' medians.  Each call takes the next of several
distinct masks whose sum exceeds the 256 MiB Infinity Cache.  Input GB/s: the windows' bytes (overlaps counted) over the time.  All sides
are checked equal before anything is timed.  Nothing here reads a GeoTIFF: the masks are seeded random blobs made on the device."""
import argparse
import os
import socket
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from srbh_amd import city_grid as CG  # noqa: E402

DEV = "cuda:0"
L3_BYTES = 256 * 2 ** 20


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def rotating(fn, bufs):
    k = [0]

    def call():
        k[0] = (k[0] + 1) % len(bufs)
        return fn(bufs[k[0]])
    return call


def make_mask(H, W, g):
    """blobs at a 64-pixel scale: most cells empty or full, as a settlement footprint is"""
    coarse = torch.rand((H // 64 + 1, W // 64 + 1), generator=g, device=DEV) < 0.35
    m = coarse.repeat_interleave(64, 0).repeat_interleave(64, 1)[:H, :W]
    m = m & (torch.rand((H, W), generator=g, device=DEV) < 0.8)
    return (m.to(torch.uint8) * 255).contiguous()


def measure(title, H, W, nmasks, args, rows, g):
    pos = CG.fishgrid_windows(W, H)
    pos_d = torch.from_numpy(pos.astype(np.int32)).to(DEV)
    pos_l = pos.tolist()
    masks = [make_mask(H, W, g) for _ in range(nmasks)]
    others = [torch.roll(m, 3, 1) for m in masks]
    pairs = list(zip(masks, others))
    assert nmasks * H * W > L3_BYTES
    x0, y0 = (torch.from_numpy(pos[:, k].copy()).to(DEV) for k in (0, 1))
    x1, y1 = x0 + 64, y0 + 64

    def ours(m):
        return CG.cell_counts(m, pos_d)

    def ours_host(m):
        return CG.cell_counts(m, pos)

    def loop(m):
        return torch.stack([(m[y:y + h, x:x + w] > 0).sum() for x, y, w, h in pos_l])

    def integral(m):
        ii = torch.nn.functional.pad((m > 0).to(torch.int64).cumsum(0).cumsum(1), (1, 0, 1, 0))
        return ii[y1, x1] - ii[y0, x1] - ii[y1, x0] + ii[y0, x0]

    def compare(p):
        return CG.cell_counts(p[0], pos_d, p[1])

    want = loop(masks[0])
    got = ours(masks[0])
    assert torch.equal(got[:, 0], want) and torch.equal(integral(masks[0]), want) and torch.equal(ours_host(masks[0]), got)
    assert int(got[:, 3].min()) == 4096 and 0 < int((got[:, 0] >= 20).sum()) < len(pos)
    both = compare(pairs[0])
    assert torch.equal(both[:, 0], want) and torch.equal(both[:, 1], loop(others[0]))
    assert torch.equal(both[:200, 2], torch.stack([((masks[0][y:y + h, x:x + w] > 0) & (others[0][y:y + h, x:x + w] > 0)).sum()
                                                   for x, y, w, h in pos_l[:200]]))
    fns = [rotating(ours, masks), rotating(ours_host, masks), rotating(loop, masks), rotating(integral, masks), rotating(compare, pairs)]
    calls = [args.calls, args.calls, args.loop_calls, args.calls, args.calls]
    for fn in fns:                                                    # every side warmed up
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    med = [[] for _ in fns]
    for _ in range(args.rounds):
        for i, fn in enumerate(fns):
            med[i].append(statistics.median(event_ms(fn) for _ in range(calls[i])))
    a, ah, b, c, d = (statistics.median(m) for m in med)
    wbytes = float((pos[:, 2] * pos[:, 3]).sum())
    names = ["(a)  cell_counts, device windows: one launch      ", "(a') cell_counts, host windows: check + upload    ",
             "(b)  a Python loop of %6d slice / > 0 / sum     " % len(pos), "(c)  int64 integral image + four gathers          ",
             "(d)  cell_counts with a second raster (compare)   "]
    rows.append(title)
    for name, m, v in zip(names, med, (a, ah, b, c, d)):
        rows.append("   %s %10.4f ms (rounds %10.4f .. %10.4f)" % (name, v, min(m), max(m)))
    ma, mb, mc = med[0], med[2], med[3]
    rows += ["   per round (b) / (a): %s -- the kernel is %s" % (" ".join("%.0f" % (x / y) for x, y in zip(mb, ma)),
                                                              "faster than the loop in every round" if all(y < x for x, y in zip(mb, ma))
                                                              else "NOT FASTER than the loop in a round"),
             "   per round (c) / (a): %s -- the rounds' ranges of (a) and (c) %s" % (" ".join("%.1f" % (x / y) for x, y in zip(mc, ma)),
                                                                                  "overlap" if max(ma) >= min(mc) and max(mc) >= min(ma)
                                                                                  else "do not overlap"),
             "   windows' bytes %.1f MB of a %.1f MB mask (overlaps counted): (a) %.0f GB/s, (d) %.0f GB/s over two rasters; %d masks of"
             % (wbytes / 1e6, H * W / 1e6, wbytes / (a * 1e-3) / 1e9, 2 * wbytes / (d * 1e-3) / 1e9, nmasks),
             "   %.1f MB in rotation exceed the 256 MiB Infinity Cache; (c) writes and re-reads 8 bytes x H x W = %.0f MB twice"
             % (H * W / 1e6, 8 * H * W / 1e6), ""]
    for row in rows[-11:]:
        print(row, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "city_grid_bench.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--loop-calls", type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    g = torch.Generator(device=DEV).manual_seed(20)
    rows = []
    measure("1. 4000 x 3000 uint8 mask, 3 888 windows of 64 / 56 (the median-city size)", 3000, 4000, 24, args, rows, g)
    measure("2. 7900 x 7900 uint8 mask, 19 881 windows of 64 / 56 (the 20 000-cell city)", 7900, 7900, 5, args, rows, g)
    prop = torch.cuda.get_device_properties(0)
    head = ["Per-cell counts of a city's grid on the device; device %s (%s, %d CUs, %.0f GB) on host %s; torch %s, HIP %s"
            % (prop.name, getattr(prop, "gcnArchName", "?"), prop.multi_processor_count, prop.total_memory / 2 ** 30, socket.gethostname(),
               torch.__version__, torch.version.hip),
            "one process; HIP events around one call each, all sides warmed up, %d alternations of %d calls per side (%d for the loop), median"
            % (args.rounds, args.calls, args.loop_calls),
            "of the rounds' medians (range of the rounds' medians).  All sides checked equal first.  Not measured: anything that reads a",
            "GeoTIFF or a shapefile; the upload of the mask; uint16 / int16 masks; other window sizes; more than one GPU.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(head + rows) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
