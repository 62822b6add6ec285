#!/usr/bin/env python
"""Time the city summary (city_summary.window_sums / block_sums / value_histogram / city_summary; csrc/srbh_summary.hip) against what a
user writes without it, in ONE process.

    python tools/time_city_summary.py [--out profiles/city_summary_bench.txt] [--rounds 5] [--calls 6] [--loop-calls 2]

Workload: a 16 000 x 12 000 uint16 height raster with a uint8 class raster (a 4000 x 3000 city at 4 x: predict_city's output size).
  1. the per-cell table's launch over the 3 888 fishnet windows of 256 / 224 (the 64 / 56 fishnet of the 4000 x 3000 grid scaled x 4):
     (a) window_sums(height, pos_dev, build); (b) the Python loop a user writes: per window slice, select, sum; (c) the best stock form
     found: int64 integral images (cumsum twice) of the selection, the selected values and their squares, four gathers per window each
     -- it has no max;
  2. block_sums at block 4, 40 and 400: (a) block_sums; (b) window_sums fed the same blocks as windows; (c) the stock
     ``x.view(Hb, block, Wb, block).sum((1, 3))`` form for n, sum and sumsq and ``amax`` for max;
  3. value_histogram(height, 10, 256, build) against torch.bincount of the masked, divided, clamped values;
  4. city_summary whole against the stock expressions (masked mean / std / max, both bincounts, read back).
torch has no comparison or division for uint16, so every stock form starts with ``height.to(torch.int32)``, inside its timed region: it
is what a user has to write.  HIP events around ONE call each (for 1 (b) the whole loop); every side warmed up, then --rounds
alternations of --calls calls per side (--loop-calls for the loop); the median of the rounds' medians with the range of the rounds'
medians.  Each call takes the next of two (height, class) pairs of 576 MB each: more than the 256 MiB Infinity Cache.  GB/s: the input
bytes (for 1: the windows' bytes, overlaps counted) over the time.  All sides are checked equal before anything is timed.  Nothing
here reads a GeoTIFF: the rasters are seeded random blobs made on the device."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from srbh_amd import city_grid as CG  # noqa: E402
from srbh_amd import city_summary as CS  # noqa: E402

DEV = "cuda:0"
L3_BYTES = 256 * 2 ** 20
H, W = 12000, 16000


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
        return fn(*bufs[k[0]])
    return call


def make_pair(g):
    """class blobs at a 64-pixel scale (most of a city holds no building), heights round(10 h) of a skewed distribution up to 200 m,
    zero where nothing was predicted; class 0 with a height remains here and there"""
    coarse = torch.rand((H // 64 + 1, W // 64 + 1), generator=g, device=DEV) < 0.35
    m = coarse.repeat_interleave(64, 0).repeat_interleave(64, 1)[:H, :W] & (torch.rand((H, W), generator=g, device=DEV) < 0.8)
    build = (m.to(torch.uint8) * torch.randint(1, 7, (H, W), generator=g, device=DEV, dtype=torch.uint8)).contiguous()
    h = (torch.rand((H, W), generator=g, device=DEV) ** 3 * 2000).round().to(torch.int16)
    h = torch.where((build > 0) | (torch.rand((H, W), generator=g, device=DEV) < 0.02), h, torch.zeros_like(h))
    return h.contiguous().view(torch.uint16), build


def bench(fns, calls, rounds):
    for fn in fns:                                                    # every side warmed up
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    med = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            med[i].append(statistics.median(event_ms(fn) for _ in range(calls[i])))
    return med


def report(rows, names, med, in_bytes):
    for name, m, nbytes in zip(names, med, in_bytes):
        v = statistics.median(m)
        rows.append("   %-58s %10.4f ms (rounds %10.4f .. %10.4f)%s" % (name, v, min(m), max(m),
                                                                       "  %6.0f GB/s" % (nbytes / (v * 1e-3) / 1e9) if nbytes else ""))
    for i in range(1, len(med)):
        ratio = " ".join("%.1f" % (x / y) for x, y in zip(med[i], med[0]))
        rows.append("   per round %s / (a): %s -- (a) is %s" % (names[i][:4].strip(), ratio, "faster in every round" if all(
            y < x for x, y in zip(med[i], med[0])) else "NOT FASTER in every round"))


def to_i32(h):
    return h.to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "city_summary_bench.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--loop-calls", type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    g = torch.Generator(device=DEV).manual_seed(21)
    pairs = [make_pair(g) for _ in range(2)]
    assert len(pairs) * H * W * 3 > L3_BYTES
    h0, b0 = pairs[0]
    raster_bytes = H * W * 3.0
    rows = []

    def selected(h, b):
        h32 = to_i32(h)
        sel = (h32 > 0) & (b > 0)
        return sel, torch.where(sel, h32, torch.zeros_like(h32)).to(torch.int64)

    # ---- 1. the per-cell table ---------------------------------------------------------------------------------------------------------
    pos = CG.fishgrid_windows(W, H, 256, 224)
    assert pos.shape == (3888, 4)
    pos_d = torch.from_numpy(pos.astype(np.int32)).to(DEV)
    pos_l = pos.tolist()
    x0, y0 = (torch.from_numpy(pos[:, k].copy()).to(DEV) for k in (0, 1))
    x1, y1 = x0 + 256, y0 + 256

    def ours(h, b):
        return CS.window_sums(h, pos_d, b)

    def loop(h, b, windows=pos_l):
        out = []
        for x, y, w, hh in windows:
            hw = to_i32(h[y:y + hh, x:x + w])
            sel = (hw > 0) & (b[y:y + hh, x:x + w] > 0)
            v = torch.where(sel, hw, torch.zeros_like(hw)).to(torch.int64)
            out.append(torch.stack([sel.sum(), v.sum(), (v * v).sum(), v.max()]))
        return torch.stack(out)

    def integral(h, b):
        sel, v = selected(h, b)
        res = []
        for img in (sel.to(torch.int64), v, v * v):
            ii = torch.nn.functional.pad(img.cumsum(0).cumsum(1), (1, 0, 1, 0))
            res.append(ii[y1, x1] - ii[y0, x1] - ii[y1, x0] + ii[y0, x0])
        return torch.stack(res, 1)

    got = ours(h0, b0)
    assert torch.equal(got[:, 1:4], integral(h0, b0)) and torch.equal(got[:200, 1:], loop(h0, b0, pos_l[:200]))
    assert int(got[:, 0].min()) == 65536 and 0 < int((got[:, 1] == 0).sum()) < len(pos)
    med = bench([rotating(ours, pairs), rotating(loop, pairs), rotating(integral, pairs)], [args.calls, args.loop_calls, args.calls], args.rounds)
    wbytes = float((pos[:, 2] * pos[:, 3]).sum()) * 3
    rows.append("1. the per-cell table: 3 888 windows of 256 / 224 over 16 000 x 12 000 (uint16 height, uint8 class)")
    report(rows, ["(a) window_sums, device windows: one launch", "(b) a Python loop of 3 888 slice / select / sum / max",
                  "(c) three int64 integral images + four gathers (no max)"], med, [wbytes, 0, 0])
    rows += ["   windows' bytes %.1f MB of %.1f MB of rasters (overlaps counted)" % (wbytes / 1e6, raster_bytes / 1e6), ""]
    print("\n".join(rows), flush=True)
    nprinted = len(rows)

    # ---- 2. blocks ---------------------------------------------------------------------------------------------------------------------
    for block in (4, 40, 400):
        Hb, Wb = H // block, W // block
        yy, xx = torch.meshgrid(torch.arange(Hb, device=DEV) * block, torch.arange(Wb, device=DEV) * block, indexing="ij")
        bpos = torch.stack([xx, yy, torch.full_like(xx, block), torch.full_like(xx, block)], -1).reshape(-1, 4).to(torch.int32)   # grid_windows' order

        def ours_b(h, b):
            return CS.block_sums(h, block, b)

        def by_windows(h, b):
            return CS.window_sums(h, bpos, b)

        def stock(h, b):
            sel, v = selected(h, b)
            v4 = v.view(Hb, block, Wb, block)
            return torch.stack([sel.view(Hb, block, Wb, block).sum((1, 3)), v4.sum((1, 3)), (v4 * v4).sum((1, 3)), v4.amax((1, 3))])

        got = ours_b(h0, b0)
        assert torch.equal(got, stock(h0, b0)) and torch.equal(got.reshape(4, -1).t(), by_windows(h0, b0)[:, 1:])
        med = bench([rotating(ours_b, pairs), rotating(by_windows, pairs), rotating(stock, pairs)], [args.calls] * 3, args.rounds)
        rows.append("2. block_sums at block %d: %d x %d blocks" % (block, Hb, Wb))
        report(rows, ["(a) block_sums: the rasters read once, one owner per block", "(b) window_sums fed the %d blocks as windows" % (Hb * Wb),
                      "(c) stock: to int32, select, view(Hb, b, Wb, b) sum / amax"], med, [raster_bytes, raster_bytes, 0])
        rows.append("")
        print("\n".join(rows[nprinted:]), flush=True)
        nprinted = len(rows)
        del bpos

    # ---- 3. histogram ------------------------------------------------------------------------------------------------------------------
    ws = torch.empty(CS._lib.lib().srbh_value_hist_ws_bytes(H, W, 256), dtype=torch.uint8, device=DEV)

    def ours_h(h, b):
        return CS.value_histogram(h, 10, 256, b, workspace=ws)

    def stock_h(h, b):
        h32 = to_i32(h)
        return torch.bincount(torch.clamp(h32[(h32 > 0) & (b > 0)] // 10, max=255), minlength=256)

    assert torch.equal(ours_h(h0, b0), stock_h(h0, b0))
    med = bench([rotating(ours_h, pairs), rotating(stock_h, pairs)], [args.calls] * 2, args.rounds)
    rows.append("3. value_histogram(height, 10, 256, build)")
    report(rows, ["(a) value_histogram: two launches", "(b) torch.bincount of the masked, divided, clamped values"], med, [raster_bytes, 0])
    rows.append("")

    # ---- 4. the whole city ---------------------------------------------------------------------------------------------------------------
    def ours_c(h, b):
        return CS.city_summary(h, b)

    def stock_c(h, b):
        h32 = to_i32(h)
        v = h32[(h32 > 0) & (b > 0)]
        d = v.double()
        return {"count": h.numel(), "n": v.numel(), "mean": d.mean().item(), "std": d.std(unbiased=False).item(), "max": int(v.max()),
                "hist": torch.bincount(torch.clamp(v // 10, max=255), minlength=256).cpu().numpy(),
                "class_counts": torch.bincount(b.reshape(-1).to(torch.int64), minlength=7).cpu().numpy()}

    mine, theirs = ours_c(h0, b0), stock_c(h0, b0)
    assert all(mine[k] == theirs[k] for k in ("count", "n", "max")) and np.array_equal(mine["hist"], theirs["hist"])
    assert np.array_equal(mine["class_counts"], theirs["class_counts"])
    assert abs(mine["mean"] - theirs["mean"]) <= 1e-9 * mine["mean"] and abs(mine["std"] - theirs["std"]) <= 1e-9 * mine["std"]
    med = bench([rotating(ours_c, pairs), rotating(stock_c, pairs)], [args.calls] * 2, args.rounds)
    rows.append("4. city_summary(height, build): count, n, mean, std, max, 256-bin histogram, class counts, read back (host time included)")
    report(rows, ["(a) city_summary: block_sums + two histograms + one copy", "(b) stock: masked mean / std / max, two bincounts, .item()"],
           med, [raster_bytes * 2 + H * W, 0])
    rows += ["   (a) reads the height raster twice and the class raster three times: the GB/s counts those bytes", ""]
    print("\n".join(rows[nprinted:]), flush=True)

    prop = torch.cuda.get_device_properties(0)
    head = ["City summary on the device; device %s (%s, %d CUs, %.0f GB); torch %s, HIP %s"
            % (prop.name, getattr(prop, "gcnArchName", "?"), prop.multi_processor_count, prop.total_memory / 2 ** 30, torch.__version__,
               torch.version.hip),
            "one process; HIP events around one call each, all sides warmed up, %d alternations of %d calls per side (%d for the loop), median"
            % (args.rounds, args.calls, args.loop_calls),
            "of the rounds' medians (range of the rounds' medians); two (height, class) pairs of %.0f MB in rotation.  All sides checked equal"
            % (raster_bytes / 1e6),
            "first.  Stock forms convert uint16 to int32 first (torch compares and divides no uint16).  Not measured: uint8 values, other",
            "raster sizes, anything that reads a GeoTIFF, more than one GPU, a raster near the 2^31-pixel limit.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(head + rows) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
