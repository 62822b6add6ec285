#!/usr/bin/env python
"""Time the burn (city_burn.burn; csrc/srbh_burn.hip) against a floor and against what a user has without it, in ONE process.

    python tools/time_city_burn.py [--out profiles/city_burn_bench.txt] [--rounds 5] [--calls 6] [--subset 2000]

Output: a uint16 raster of 12 000 rows x 16 000 columns (tools/time_city_summary.py's shape; 384 MB), two of them in rotation (more
than the 256 MiB Infinity Cache).  Feature sets:
  1. about a million random quadrilaterals of 3..12 pixels: numpy RandomState(7); per feature a centre uniform over the raster, half
     sizes uniform in [1.5, 6] per axis, the four corners moved by uniform [-0.5, 0.5] per axis, rounded to 1/256; values uniform 1..65535;
  2. the 301 zones of about 300 x 300 pixels of tools/time_city_zones.py;
  3. its one zone of 1000 vertices over about half the raster.
Sides:
  (a)  burn with its tables resident (kept on the Zones object after the first call: the steady state); the values are uploaded per call;
  (a0) burn with boxes and tile lists rebuilt on the host and all tables uploaded in the timed region: what the FIRST call costs;
  (b)  the floor: a plain fill_ of the same output bytes;
  (c)  the best stock-torch construction found: fill_, then per feature the crossing test / scatter_add_ / cumsum mask of
       tools/time_city_zones.py over the feature's box and a masked assignment (torch.where into the box's view), in feature order.
       For set 1 it is timed on the first --subset features and SCALED by Z / subset (one Python loop turn and about eight launches per
       feature: the cost is per feature); the scaled number is marked.
HIP events around ONE call each; every side warmed up, then --rounds alternations of --calls calls per side; the median of the rounds'
medians with the range of the rounds' medians.  (a) and (c) are checked equal before anything is timed (set 1: on the subset).  The host
time of feature_edges and burn_tiles for set 1 is reported separately (perf_counter, median of 3)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import time_city_summary as TS  # noqa: E402
import time_city_zones as TZ  # noqa: E402
from srbh_amd import city_burn as CB  # noqa: E402
from srbh_amd import city_zones as CZ  # noqa: E402

DEV = TS.DEV
H, W = TS.H, TS.W


def million(n=1_000_000, seed=7):
    """-> (vertices (4n, 2), ring_off, feature_off, values)"""
    rs = np.random.RandomState(seed)
    c = np.stack([rs.uniform(0, W, size=n), rs.uniform(0, H, size=n)], axis=1)
    half = rs.uniform(1.5, 6.0, size=(n, 1, 2))
    corners = np.array([(-1, -1), (1, -1), (1, 1), (-1, 1)], dtype=np.float64)[None]
    v = c[:, None, :] + corners * half + rs.uniform(-0.5, 0.5, size=(n, 4, 2))
    v = np.round(v.reshape(-1, 2) * 256) / 256
    return v, np.arange(n + 1, dtype=np.int64) * 4, np.arange(n + 1, dtype=np.int64), rs.randint(1, 65536, size=n)


def i16(v):
    """values 0..65535 as the int16 bit patterns torch's ops take"""
    v = np.asarray(v, dtype=np.int64)
    return np.where(v >= 32768, v - 65536, v).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "city_burn_bench.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--subset", type=int, default=2000)
    ap.add_argument("--features", type=int, default=1_000_000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    outs = [torch.empty((H, W), dtype=torch.uint16, device=DEV) for _ in range(2)]
    assert len(outs) * H * W * 2 > TS.L3_BYTES
    rows, nprinted = [], 0

    v, ring_off, feature_off, mvalues = million(args.features)
    host = {"feature_edges": [], "burn_tiles": []}
    for _ in range(3):
        t0 = time.perf_counter()
        mzones = CB.feature_edges(v, ring_off, feature_off)
        t1 = time.perf_counter()
        mtiles = CB.burn_tiles(mzones, H, W)
        t2 = time.perf_counter()
        host["feature_edges"].append(t1 - t0)
        host["burn_tiles"].append(t2 - t1)
    one, many = TZ.zone_sets()
    rs = np.random.RandomState(8)
    sets = (("1. %d random quadrilaterals of 3..12 pixels" % len(mzones), mzones, mvalues, args.subset),
            ("2. 301 zones of about 300 x 300 pixels", CZ.zone_edges(many), rs.randint(1, 65536, size=301), None),
            ("3. one zone of 1000 vertices over about half the raster", CZ.zone_edges(one), np.array([1234]), None))
    for tag, zones, values, subset in sets:
        Z = len(zones)
        n = Z if subset is None else min(subset, Z)
        pos = TZ.boxes(zones)[:n]
        edges = [torch.from_numpy(zones.edges[zones.edge_off[k]:zones.edge_off[k + 1]].astype(np.int64)).to(DEV) for k in range(n)]
        sv = i16(values[:n]).tolist()

        def ours(out):
            return CB.burn(zones, values, out=out)

        def cold(out):
            zones._device_tables.clear()
            return CB.burn(zones, values, out=out)

        def floor(out):
            return out.view(torch.int16).fill_(1)

        def stock(out):
            o = out.view(torch.int16)
            o.fill_(0)
            for e, (x, y, w, h), val in zip(edges, pos.tolist(), sv):
                if w <= 0 or h <= 0 or len(e) == 0:
                    continue
                box = o[y:y + h, x:x + w]
                box.copy_(torch.where(TZ.torch_zone_mask(e, x, x + w, y, y + h), torch.full_like(box, val), box))
            return out

        # equal first: the subset (or the set) burned alone against the stock construction
        if subset is None:
            check = zones
        else:
            check = CZ.Zones(zones.edges[:zones.edge_off[n]], zones.edge_off[:n + 1], zones.bbox[:n])
        a = CB.burn(check, values[:n], out=outs[0]).view(torch.int16).clone()
        assert torch.equal(a, stock(outs[1]).view(torch.int16)), tag
        burned = int((a != 0).sum())
        del a
        bufs = [(o,) for o in outs]
        ncalls = [args.calls, args.calls, args.calls, 2 if Z > 10000 else args.calls]
        med = TS.bench([TS.rotating(ours, bufs), TS.rotating(floor, bufs), TS.rotating(stock, bufs), TS.rotating(cold, bufs)],
                       [ncalls[0], ncalls[1], 1 if subset is not None else 2, ncalls[3]], args.rounds)
        scale = Z / n
        if scale != 1:
            med[2] = [m * scale for m in med[2]]
        NF = len((mtiles if zones is mzones else CB.burn_tiles(zones, H, W))[2])
        rows.append("%s: %d edges, %d (feature, tile) pairs over %d tiles%s" % (tag, len(zones.edges), NF, -(-H // 64) * -(-W // 64),
                                                                               "" if scale == 1 else "; %.2f Mpixel burned by the first %d" % (burned / 1e6, n)))
        nbytes = float(H) * W * 2
        TS.report(rows, ["(a) burn, tables resident: one launch", "(b) floor: fill_ of the same output bytes",
                         "(c) stock: fill_, then per feature crossings, scatter_add, cumsum, where" + ("" if scale == 1 else " -- %d features timed, SCALED x %.0f" % (n, scale)),
                         "(a0) burn, boxes and tile lists rebuilt, tables uploaded in the call"], med, [nbytes, nbytes, 0, nbytes])
        rows.append("")
        print("\n".join(rows[nprinted:]), flush=True)
        nprinted = len(rows)
        del edges

    rows.append("host, set 1 (perf_counter, median of 3): feature_edges %.3f s, burn_tiles %.3f s"
                % (statistics.median(host["feature_edges"]), statistics.median(host["burn_tiles"])))
    prop = torch.cuda.get_device_properties(0)
    head = ["Footprints burned into a raster on the device; device %s (%s, %d CUs, %.0f GB); torch %s, HIP %s"
            % (prop.name, getattr(prop, "gcnArchName", "?"), prop.multi_processor_count, prop.total_memory / 2 ** 30, torch.__version__,
               torch.version.hip),
            "one process; HIP events around one call each, all sides warmed up, %d alternations of %d calls per side (fewer for the stock loops and"
            % (args.rounds, args.calls),
            "for (a0) of set 1), median of the rounds' medians (range of the rounds' medians); two %d x %d uint16 outputs of %.0f MB in rotation."
            % (H, W, H * W * 2 / 1e6),
            "(a) and (c) checked equal first.  GB/s: the output bytes over the time.  Not measured: uint8 outputs, merge \"max\", keep, interior",
            "views, other raster sizes, features with holes or many parts, shapefile reading, more than one GPU.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(head + rows) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
