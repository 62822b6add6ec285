#!/usr/bin/env python
"""Time the inference tile cutter (loader_math.GridTiles, srbh_grid_tiles) against what a user writes without it, in ONE process.

    python tools/time_grid_tiles.py [--out profiles/grid_tiles_bench.txt] [--rounds 5] [--calls 20] [--city-runs 5]

1. One batch: 256 windows of 64 x 64, 6 + 2 bands (uint16 Sentinel-2 of 8 bands, float32 Sentinel-1), stride 48, on a 4 096 x 4 096 raster.
   (a) the stock construction: 256 slices of each raster, torch.stack, .float(), the channel concatenate, normalize_tiles(..., None);
   (b) gt[s:e] -- four distinct slices in rotation, so that every call is a launch and none a hit of the memo.
   HIP events around ONE call each; both warmed up, then --rounds alternations of --calls calls; the median of the rounds' medians with the
   range of the rounds' medians.  Bytes: the tiles written once plus the source pixels of every window read once.
2. One median-size city (45 x 45 = 2 025 cells at stride 48, batch 256, 23 RRDB blocks) through predict_tiles and Mosaic.finalize, fed by
   GridTiles and fed by the resident fp32 tensor of all its tiles: --city-runs alternations, host clock around work that ends in a
   synchronise.  The spread of the tensor form's repeated runs comes first; the GridTiles form is set against it.  Peak device memory
   (torch's allocator) of one city per form, measured with only that form's inputs alive.
Nothing here reads a GeoTIFF: the rasters are seeded random numbers made on the device."""
import argparse
import os
import socket
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from srbh_amd import harness, synth  # noqa: E402
from srbh_amd import loader_math as LM  # noqa: E402
from srbh_amd.mosaic import Mosaic  # noqa: E402

DEV = "cuda:0"
PREDICT_BATCH_MS = 43.6          # one 256-tile batch of the inference workload (README: BASELINE configs[4])
S2_STATS = np.stack([np.zeros(8), np.full(8, 10000.0)])
S1_STATS = np.stack([np.full(2, -32.0), np.full(2, 0.0)])


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def rounds_of(fns, rounds, calls, warmup=5):
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


def rasters(H, W, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    s2 = torch.randint(0, 10000, (8, H, W), generator=g, device=DEV, dtype=torch.int16).view(torch.uint16)
    s1 = torch.rand((2, H, W), generator=g, device=DEV) * 24 - 28
    return s2, s1


def stock_batch(s2, s1, pos, mins, maxs):
    """the parent's cheapest equivalent: a slice per window and raster, stack, cast, concatenate, normalize_tiles"""
    a = torch.stack([s2[:6, y:y + yc, x:x + xc] for x, y, xc, yc in pos]).float()
    b = torch.stack([s1[:, y:y + yc, x:x + xc] for x, y, xc, yc in pos])
    return LM.normalize_tiles(torch.cat([a, b], 1), mins, maxs, None)


def one_batch(args, rows):
    H = W = 4096
    s2, s1 = rasters(H, W, 3)
    pos = LM.grid_windows(W, H, 64, 48)
    first = (len(pos) // 2) // 256 * 256                                      # four batches from the middle of the city
    pos = pos[first:first + 4 * 256]
    gt = LM.GridTiles(s2, s1, pos, S2_STATS, S1_STATS)
    mins = np.concatenate([S2_STATS[0, :6], S1_STATS[0]])
    maxs = np.concatenate([S2_STATS[1, :6], S1_STATS[1]])
    lists = [pos[i:i + 256].tolist() for i in range(0, 1024, 256)]
    note = ""
    try:
        stock_batch(s2, s1, lists[0], mins, maxs)
        s2_stock = s2
    except (RuntimeError, TypeError) as e:                                     # an op torch does not have for uint16: hand it the same bits as int16
        s2_stock = s2.view(torch.int16)                                        # (every value here is below 2^15, so the tiles are the same)
        note = "   (torch refused the uint16 raster in (a): %s -- (a) ran on the same bits viewed as int16)" % str(e).splitlines()[0][:90]
    for i in range(4):                                                         # the two sides compute the same tiles
        assert torch.equal(stock_batch(s2_stock, s1, lists[i], mins, maxs), gt[i * 256:(i + 1) * 256]), i
    k = [0, 0]

    def a_stock():
        k[0] = (k[0] + 1) % 4
        stock_batch(s2_stock, s1, lists[k[0]], mins, maxs)

    def b_cutter():
        k[1] = (k[1] + 1) % 4
        gt[k[1] * 256:(k[1] + 1) * 256]

    ma, mb = rounds_of([a_stock, b_cutter], args.rounds, args.calls)
    written = 256 * 8 * 64 * 64 * 4
    read = 256 * 64 * 64 * (6 * 2 + 2 * 4)
    a, b = statistics.median(ma), statistics.median(mb)
    rows += ["1. one batch: 256 windows of 64 x 64 at stride 48 on a 4 096 x 4 096 raster, uint16 x 8 (6 taken) + float32 x 2 -> (256, 8, 64, 64) fp32",
             "   (a) stock: 2 x 256 slices, stack, .float(), cat, normalize_tiles   %8.4f ms (rounds %8.4f .. %8.4f)" % (a, min(ma), max(ma)),
             "   (b) GridTiles gt[s:e], one srbh_grid_tiles launch                  %8.4f ms (rounds %8.4f .. %8.4f)" % (b, min(mb), max(mb)),
             "   per round (a) / (b): %s -- the cutter is %s" % (" ".join("%.1f" % (x / y) for x, y in zip(ma, mb)),
                                                                "not slower in any round" if all(y <= x for x, y in zip(ma, mb)) else "SLOWER in a round"),
             "   (b) moves %.1f MB written + %.1f MB read (every window's source pixels once; overlapping windows re-read a third of them) = %.1f MB"
             % (written / 1e6, read / 1e6, (written + read) / 1e6),
             "   -> %.0f GB/s at the median; (b) is %.2f %% of the %.1f ms predict batch, (a) %.2f %%"
             % ((written + read) / (b * 1e-3) / 1e9, 100 * b / PREDICT_BATCH_MS, PREDICT_BATCH_MS, 100 * a / PREDICT_BATCH_MS)]
    if note:
        rows.append(note)
    rows.append("")
    for row in rows:
        print(row, flush=True)


def nets(num_block):
    from srbh_amd.models import SRRegress_Cls_feature
    from srbh_amd.rrdbnet import RRDBNet
    net_hr = RRDBNet(3, 3, num_block=num_block)
    net_hr.load_state_dict(synth.rrdbnet_state_dict(num_block=num_block, seed=1337, mode="init"))
    torch.manual_seed(1337)
    model = SRRegress_Cls_feature("efficientnet-b4", in_channels=8, super_in=64, super_mid=16, upscale=4, isaggre=False, chans_build=7)
    return net_hr.to(DEV).eval(), model.to(DEV).eval()


def one_city(args, rows):
    side = 45 * 48 + 16
    pos = LM.grid_windows(side, side, 64, 48)
    assert len(pos) == 2025
    net_hr, model = nets(args.num_block)
    torch.backends.cudnn.benchmark = True                                      # as bench.py's predict workload: MIOpen's solver search in the warm-up
    batch = 256

    def city(tiles, posall):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = Mosaic(4 * side, 4 * side, 7, DEV)
        harness.predict_tiles(net_hr, model, tiles, posall, m, batch=batch, pad_to=32)
        out = m.finalize()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def peak(make):
        """peak bytes of torch's allocator over one city with only what make() returns (and the networks, the graph) alive"""
        tiles, posall = make()
        city(tiles, posall)                                                    # (warm: graph capture, workspaces)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        inputs = sum(t.numel() * t.element_size() for t in ([tiles] if torch.is_tensor(tiles) else [tiles.s2, tiles.s1]))
        torch.cuda.reset_peak_memory_stats()
        _, out = city(tiles, posall)
        return torch.cuda.max_memory_allocated(), base, inputs, [o.cpu() for o in out]      # (on the host: not in the next form's figures)

    def make_gt():
        s2, s1 = rasters(side, side, 5)
        return LM.GridTiles(s2, s1, pos, S2_STATS, S1_STATS), pos

    def make_tensor():
        gt, _ = make_gt()
        return torch.cat([gt[s:s + batch].clone() for s in range(0, len(pos), batch)]), pos.tolist()

    pk_gt, base_gt, in_gt, out_gt = peak(make_gt)
    pk_t, base_t, in_t, out_t = peak(make_tensor)
    same = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(out_gt, out_t))
    del out_gt, out_t
    gt, _ = make_gt()
    tiles, plist = make_tensor()
    for _ in range(2):
        city(tiles, plist)
        city(gt, pos)
    t_t, t_g = [], []
    for _ in range(args.city_runs):
        t_t.append(city(tiles, plist)[0])
        t_g.append(city(gt, pos)[0])
    mt, mg = statistics.median(t_t), statistics.median(t_g)
    n_batches = (len(pos) + batch - 1) // batch
    rows2 = ["2. one city: 2 025 cells (45 x 45 at stride 48 on a %d x %d raster), batch %d, %d RRDB blocks, predict_tiles + Mosaic.finalize, host clock" % (side, side, batch, args.num_block),
             "   resident fp32 tensor, %d runs: %s ms -> median %.2f, spread %.2f .. %.2f (%.2f %% of the median)"
             % (len(t_t), " ".join("%.2f" % t for t in t_t), mt, min(t_t), max(t_t), 100 * (max(t_t) - min(t_t)) / mt),
             "   GridTiles,            %d runs: %s ms -> median %.2f, range %.2f .. %.2f"
             % (len(t_g), " ".join("%.2f" % t for t in t_g), mg, min(t_g), max(t_g)),
             "   GridTiles - tensor at the medians: %+.2f ms (%+.2f %%); the GridTiles median lies %s the tensor form's spread; %d launches of the cutter"
             % (mg - mt, 100 * (mg - mt) / mt, "inside" if min(t_t) <= mg <= max(t_t) else ("BELOW" if mg < min(t_t) else "ABOVE"), n_batches),
             "   (measure 1's figure per launch gives the excess the cutter itself can explain)",
             "   finalised rasters of the two forms bit-identical: %s" % same,
             "   peak device memory over one city (torch allocator; networks, captured graph and workspaces included in both):",
             "     GridTiles:       peak %8.1f MB, of which its inputs (both rasters) %7.1f MB; allocated before the run %8.1f MB" % (pk_gt / 1e6, in_gt / 1e6, base_gt / 1e6),
             "     resident tensor: peak %8.1f MB, of which its inputs (all tiles)    %7.1f MB; allocated before the run %8.1f MB" % (pk_t / 1e6, in_t / 1e6, base_t / 1e6)]
    for row in rows2:
        print(row, flush=True)
    return rows2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_tiles_bench.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--city-runs", type=int, default=5)
    ap.add_argument("--num-block", type=int, default=23)
    ap.add_argument("--skip-city", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    rows = []
    one_batch(args, rows)
    torch.cuda.empty_cache()
    rows2 = ["2. one city: not measured (--skip-city)"] if args.skip_city else one_city(args, [])
    prop = torch.cuda.get_device_properties(0)
    head = ["Inference tiles cut from device rasters; device %s (%s, %d CUs, %.0f GB) on host %s; torch %s, HIP %s"
            % (prop.name, getattr(prop, "gcnArchName", "?"), prop.multi_processor_count, prop.total_memory / 2 ** 30, socket.gethostname(),
               torch.__version__, torch.version.hip),
            "one process; 1: HIP events around one call each, both sides warmed up, %d alternations of %d calls per side, median of the rounds'"
            % (args.rounds, args.calls),
            "medians (range of the rounds' medians); 2: host clock around one city ending in a synchronise, %d alternations.  Not measured: anything"
            % args.city_runs,
            "that reads a GeoTIFF; the upload of the rasters; cities of other sizes; more than one GPU.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(head + rows + rows2) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
