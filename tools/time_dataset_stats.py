#!/usr/bin/env python
"""Time the dataset-statistics kernels (dataset_stats.band_stats / label_histogram) against the stock construction on the same device, in
ONE process.

    python tools/time_dataset_stats.py [--out profiles/dataset_stats_bench.txt] [--rounds 5] [--calls 10]

Sizes: 4 096 tiles of 6 x 64 x 64 uint16, 4 096 tiles of 2 x 64 x 64 float32, 1 024 labels of 256 x 256 uint8.
  (a) stock: bands  x.double(), then amin / amax / mean / std(unbiased=False) over (H, W);
             labels torch.bincount(labels.flatten().long(), minlength=256);
  (b) band_stats(x) (one srbh_band_stats launch) / label_histogram(labels) (srbh_label_hist + its fold).
HIP events around ONE call each; both sides warmed up, then --rounds alternations of --calls calls per side; the median of the rounds' medians
with the range of the rounds' medians.  Each call takes the next of several distinct input buffers whose sum exceeds the 256 MiB Infinity
Cache, so the figures are reads from HBM; (c) repeats (b) on ONE buffer that fits the Infinity Cache.  Bytes moved: the input once (the
outputs are a few hundred KB).  Nothing here reads a GeoTIFF: the inputs are seeded random numbers made on the device."""
import argparse
import os
import socket
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from srbh_amd import dataset_stats as DS  # noqa: E402

DEV = "cuda:0"
HBM_SPEC, HBM_MEASURED = 8.0e12, 6.29e12        # MI355X: HBM3E peak by specification / reached by a float4 copy
L3_BYTES = 256 * 2 ** 20


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def rounds_of(fns, rounds, calls, warmup=3):
    """per case: the rounds' medians"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    med = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            med[i].append(statistics.median(event_ms(fn) for _ in range(calls)))
    return med


def stock_bands(x):
    d = x.double()
    return d.amin((2, 3)), d.amax((2, 3)), d.mean((2, 3)), d.std((2, 3), unbiased=False)


def stock_labels(lab):
    return torch.bincount(lab.flatten().long(), minlength=256)


def rotating(fn, bufs):
    k = [0]

    def call():
        k[0] = (k[0] + 1) % len(bufs)
        fn(bufs[k[0]])
    return call


def measure(title, bufs, stock, stock_bufs, ours, check, args, rows):
    nbytes = bufs[0].numel() * bufs[0].element_size()
    assert nbytes * len(bufs) > L3_BYTES > nbytes
    check(stock(stock_bufs[0]), ours(bufs[0]))
    ma, mb, mc = rounds_of([rotating(stock, stock_bufs), rotating(ours, bufs), rotating(ours, bufs[:1])], args.rounds, args.calls)
    a, b, c = (statistics.median(m) for m in (ma, mb, mc))
    rows += [title,
             "   (a) stock ops, %d buffers in rotation    %9.4f ms (rounds %9.4f .. %9.4f)" % (len(bufs), a, min(ma), max(ma)),
             "   (b) libsrbh,   %d buffers in rotation    %9.4f ms (rounds %9.4f .. %9.4f)" % (len(bufs), b, min(mb), max(mb)),
             "   (c) libsrbh,   one resident buffer      %9.4f ms (rounds %9.4f .. %9.4f)" % (c, min(mc), max(mc)),
             "   per round (a) / (b): %s -- the kernel is %s" % (" ".join("%.1f" % (x / y) for x, y in zip(ma, mb)),
                                                              "faster in every round" if all(y < x for x, y in zip(ma, mb)) else "NOT FASTER in a round"),
             "   input %.1f MB read once: (b) %.0f GB/s = %.0f %% of the 8.0 TB/s HBM peak (%.0f %% of the 6.29 TB/s a copy reaches); %d x %.0f MB"
             % (nbytes / 1e6, nbytes / (b * 1e-3) / 1e9, 100 * nbytes / (b * 1e-3) / HBM_SPEC, 100 * nbytes / (b * 1e-3) / HBM_MEASURED,
                len(bufs), nbytes / 1e6),
             "   in rotation exceed the 256 MiB Infinity Cache: these are reads from HBM; (c) %.0f GB/s with the one buffer left in the Infinity"
             % (nbytes / (c * 1e-3) / 1e9),
             "   Cache by the call before (it fits; the 32 MiB of L2 do not hold it)", ""]
    for row in rows[-9:]:
        print(row, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dataset_stats_bench.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    g = torch.Generator(device=DEV).manual_seed(19)
    rows = []

    def check_bands(want, got):
        stats, count = got
        assert torch.equal(stats[..., 0], want[0]) and torch.equal(stats[..., 1], want[1]) and int(count.min()) == 64 * 64
        assert torch.allclose(stats[..., 2], want[2], rtol=1e-12, atol=0) and torch.allclose(stats[..., 3], want[3], rtol=1e-9, atol=0)

    # uint16 values below 2^15: torch lacks most uint16 ops, so the stock side reads the same bits as int16
    s2 = [torch.randint(0, 10000, (4096, 6, 64, 64), generator=g, device=DEV, dtype=torch.int16) for _ in range(2)]
    measure("1. 4 096 tiles of 6 x 64 x 64 uint16 (Sentinel-2): per image and band min, max, mean, std",
            [t.view(torch.uint16) for t in s2], stock_bands, s2, DS.band_stats, check_bands, args, rows)
    del s2
    s1 = [torch.rand((4096, 2, 64, 64), generator=g, device=DEV) * 24 - 28 for _ in range(3)]
    measure("2. 4 096 tiles of 2 x 64 x 64 float32 (Sentinel-1, decibels)", s1, stock_bands, s1, DS.band_stats, check_bands, args, rows)
    del s1
    lab = []
    for _ in range(5):
        t = torch.rand((1024, 256, 256), generator=g, device=DEV)
        lab.append(torch.where(t < 0.7, torch.zeros_like(t), (t - 0.7) * 850.0).to(torch.uint8))        # mostly 0, a tail up to 255
        del t

    def check_hist(want, got):
        assert torch.equal(want, got)

    measure("3. 1 024 labels of 256 x 256 uint8 (70 % zeros): the 256-bin histogram", lab, stock_labels, lab, DS.label_histogram, check_hist,
            args, rows)
    prop = torch.cuda.get_device_properties(0)
    head = ["Dataset statistics on the device; device %s (%s, %d CUs, %.0f GB) on host %s; torch %s, HIP %s"
            % (prop.name, getattr(prop, "gcnArchName", "?"), prop.multi_processor_count, prop.total_memory / 2 ** 30, socket.gethostname(),
               torch.__version__, torch.version.hip),
            "one process; HIP events around one call each, all sides warmed up, %d alternations of %d calls per side, median of the rounds'"
            % (args.rounds, args.calls),
            "medians (range of the rounds' medians).  Not measured: anything that reads a GeoTIFF; the upload; other tile sizes; the host",
            "arithmetic behind the per-image table.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(head + rows) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
