#!/usr/bin/env python
"""Time the polygon zones (city_zones.zone_sums / urban_centre_table; csrc/srbh_zones.hip) against what a user has without them, in ONE
process.

    python tools/time_city_zones.py [--out profiles/city_zones_bench.txt] [--rounds 5] [--calls 6] [--loop-calls 2]

Workload: the 16 000 x 12 000 uint16 height raster with its uint8 class raster of tools/time_city_summary.py.
  1. ONE zone of 1000 vertices covering about half the raster (an ellipse with a rippled radius);
  2. 301 zones of about 300 x 300 pixels (24-gons with random radii, one per cell of a 21 x 15 grid: they do not overlap);
  3. urban_centre_table(height, build, the 301 zones) whole: sums, 256-bin height histograms, class counts, read back, host time included.
Sides:
  (a) zone_sums with its tables resident (they are kept on the Zones object after the first call: the steady state);
  (a0) zone_sums with the item table rebuilt on the host and all tables uploaded in the timed region: what the FIRST call costs;
  (b) the floor if rasterising were free: window_sums over each zone's bounding box (cut into the bands zone_sums uses, so that one box
      is not one workgroup; the bands added per zone by index_add_ / scatter_reduce_) with a mask raster ALREADY resident that is the
      class raster inside the zones and 0 outside -- no zone is rasterised in the timed region;
  (c) the best stock-torch construction found: per zone, the crossing test of every edge against every row of the bounding box in int64
      ([E, rows]: t by floor_divide), the toggles scattered into [rows, width + 1] and a cumsum along the row (the same parity trick as
      the kernel's, as stock ops), then masked sums of the bounding box.  Its time includes the rasterisation.  A broadcast of every edge
      against every PIXEL ([E, rows, width]) does not fit the memory for workload 1 and was not timed.
For 3: (a) against (c) with two bincounts per zone added; there is no (b) -- nothing existing makes per-window histograms.
HIP events around ONE call each; every side warmed up, then --rounds alternations of --calls calls per side (--loop-calls for the loops
over 301 zones); the median of the rounds' medians with the range of the rounds' medians.  Each call takes the next of two (height, class)
pairs of 576 MB each: more than the 256 MiB Infinity Cache.  All sides are checked equal before anything is timed."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import time_city_summary as TS  # noqa: E402
from srbh_amd import city_summary as CS  # noqa: E402
from srbh_amd import city_zones as CZ  # noqa: E402

DEV = TS.DEV
H, W = TS.H, TS.W


def torch_zone_mask(edges, x0, x1, y0, y1):
    """the zone's pixels of the box [x0, x1) x [y0, y1) by stock ops, exact: edges int64 (E, 4) on the device -> (rows, width) bool"""
    X0, Y0, X1, Y1 = (edges[:, k] for k in range(4))
    up = Y0 > Y1
    X0, X1, Y0, Y1 = torch.where(up, X1, X0), torch.where(up, X0, X1), torch.where(up, Y1, Y0), torch.where(up, Y0, Y1)
    cy = (torch.arange(y0, y1, device=edges.device, dtype=torch.int64) * 256 + 128)[None, :]
    den, dx = (Y1 - Y0)[:, None], (X1 - X0)[:, None]
    cross = (Y0[:, None] <= cy) & (cy < Y1[:, None])
    t = torch.floor_divide(X0[:, None] * den + (cy - Y0[:, None]) * dx + 128 * den - 1, 256 * den.clamp(min=1))
    t = (t.clamp(min=x0, max=x1) - x0).t().contiguous()                  # [rows, E]: the crossing toggles the box's pixels < t
    tog = torch.zeros((y1 - y0, x1 - x0 + 1), dtype=torch.int32, device=edges.device)
    tog.scatter_add_(1, t, cross.t().to(torch.int32))
    c = tog.cumsum(1, dtype=torch.int32)
    return ((c[:, -1:] - c[:, :-1]) & 1).bool()                          # pixel x: the parity of the crossings with t > x


def boxes(zones):
    """each zone's bounding box in pixels, clipped to the raster: (Z, 4) int64 windows (xoff, yoff, xcount, ycount)"""
    out = []
    for xmin, ymin, xmax, ymax in zones.bbox.tolist():
        x0, x1, y0, y1 = max(xmin >> 8, 0), min(-((-xmax) >> 8), W), max((ymin + 127) >> 8, 0), min((ymax + 127) >> 8, H)
        out.append((x0, y0, x1 - x0, y1 - y0))
    return np.array(out, dtype=np.int64)


def zone_sets():
    """the polygons of workloads 1 and 2 -> (one, many)"""
    rs = np.random.RandomState(7)
    a = 2 * np.pi * np.arange(1000) / 1000
    rad = 1 + 0.05 * np.sin(9 * a)
    one = [[np.stack([W / 2 + 0.4 * W * rad * np.cos(a), H / 2 + 0.4 * H * rad * np.sin(a)], axis=1)]]
    many = []
    for k in range(301):
        cx, cy = (k % 21 + 0.5) * (W / 21), (k // 21 + 0.5) * (H / 15)
        b = np.sort(rs.uniform(0, 2 * np.pi, size=24))
        r = 170 * rs.uniform(0.7, 1.0, size=24)
        many.append([np.stack([cx + r * np.cos(b), cy + r * np.sin(b)], axis=1)])
    return one, many


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "city_zones_bench.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--loop-calls", type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    g = torch.Generator(device=DEV).manual_seed(21)
    pairs = [TS.make_pair(g) for _ in range(2)]
    assert len(pairs) * H * W * 3 > TS.L3_BYTES
    one, many = zone_sets()
    rows, nprinted = [], 0
    tables = {}
    for tag, polys, calls in (("1. one zone of 1000 vertices over about half the raster", one, args.calls),
                              ("2. 301 zones of about 300 x 300 pixels", many, args.loop_calls)):
        zones = CZ.zone_edges(polys)
        pos = boxes(zones)
        items = CZ.zone_items(zones, H, W)[0]
        ipos_d, zid = torch.from_numpy(items[:, 1:].copy()).to(DEV), torch.from_numpy(items[:, 0].astype(np.int64)).to(DEV)
        edges = [torch.from_numpy(zones.edges[zones.edge_off[k]:zones.edge_off[k + 1]].astype(np.int64)).to(DEV) for k in range(len(zones))]
        inzone = torch.zeros((H, W), dtype=torch.bool, device=DEV)
        for e, (x, y, w, h) in zip(edges, pos.tolist()):
            inzone[y:y + h, x:x + w] |= torch_zone_mask(e, x, x + w, y, y + h)
        zmasks = [torch.where(inzone, b, torch.zeros_like(b)) for _, b in pairs]       # resident before anything is timed
        area = int(inzone.sum())
        del inzone

        def ours(h, b, zm):
            return CZ.zone_sums(h, zones, b)

        def cold(h, b, zm):
            zones._device_tables.clear()
            return CZ.zone_sums(h, zones, b)

        def floor(h, b, zm):
            s = CS.window_sums(h, ipos_d, zm)                            # the same bands as (a)'s items, then each zone's bands added
            out = torch.zeros((len(zones), 5), dtype=torch.int64, device=DEV).index_add_(0, zid, s)
            out[:, 4] = torch.zeros(len(zones), dtype=torch.int64, device=DEV).scatter_reduce_(0, zid, s[:, 4], "amax")
            return out

        def stock(h, b, zm):
            out = []
            for e, (x, y, w, hh) in zip(edges, pos.tolist()):
                inz = torch_zone_mask(e, x, x + w, y, y + hh)
                h32 = TS.to_i32(h[y:y + hh, x:x + w])
                sel = inz & (h32 > 0) & (b[y:y + hh, x:x + w] > 0)
                v = torch.where(sel, h32, torch.zeros_like(h32)).to(torch.int64)
                out.append(torch.stack([inz.sum(), sel.sum(), v.sum(), (v * v).sum(), v.max()]))
            return torch.stack(out)

        trip = [(h, b, zm) for (h, b), zm in zip(pairs, zmasks)]
        got = ours(*trip[0])
        assert torch.equal(got, stock(*trip[0])) and torch.equal(got[:, 1:], floor(*trip[0])[:, 1:]) and int(got[:, 0].sum()) == area
        assert int(got[:, 1].min()) > 0
        med = TS.bench([TS.rotating(ours, trip), TS.rotating(floor, trip), TS.rotating(stock, trip), TS.rotating(cold, trip)],
                       [args.calls, args.calls, calls, args.calls], args.rounds)
        box_bytes = float((pos[:, 2] * pos[:, 3]).sum()) * 3
        rows.append("%s: %d edges, %d items, %.1f Mpixel in the zones, bounding boxes %.1f Mpixel" % (tag, len(zones.edges), len(items), area / 1e6,
                                                                                                  box_bytes / 3e6))
        TS.report(rows, ["(a) zone_sums, tables resident: two launches", "(b) floor: window_sums of the boxes' bands, mask raster resident",
                         "(c) stock: int64 crossings, scatter_add, cumsum, masked sums", "(a0) zone_sums, tables rebuilt and uploaded in the call"],
                  med, [box_bytes, box_bytes, 0, box_bytes])
        rows.append("")
        print("\n".join(rows[nprinted:]), flush=True)
        nprinted = len(rows)
        tables[tag[0]] = (zones, edges, pos)
        del zmasks, trip

    # ---- 3. the table ----------------------------------------------------------------------------------------------------------------------
    zones, edges, pos = tables["2"]

    def ours_t(h, b):
        return CZ.urban_centre_table(h, b, zones)

    def stock_t(h, b):
        out, hists, classes = [], [], []
        for e, (x, y, w, hh) in zip(edges, pos.tolist()):
            inz = torch_zone_mask(e, x, x + w, y, y + hh)
            h32, bb = TS.to_i32(h[y:y + hh, x:x + w]), b[y:y + hh, x:x + w]
            sel = inz & (h32 > 0) & (bb > 0)
            v = h32[sel].to(torch.int64)
            out.append(torch.stack([inz.sum(), sel.sum(), v.sum(), (v * v).sum(), v.max()]))
            hists.append(torch.bincount(torch.clamp(v // 10, max=255), minlength=256))
            classes.append(torch.bincount(torch.clamp(bb[inz].to(torch.int64), max=6), minlength=7))
        flat = torch.cat([torch.stack(out), torch.stack(hists), torch.stack(classes)], dim=1).cpu().numpy()
        t = CS.heights_from_sums(flat[:, :5])
        t["hist"], t["class_counts"] = flat[:, 5:261], flat[:, 261:]
        return t

    mine, theirs = ours_t(*pairs[0]), stock_t(*pairs[0])
    assert all(np.array_equal(mine[k], theirs[k], equal_nan=True) for k in mine)
    med = TS.bench([TS.rotating(ours_t, pairs), TS.rotating(stock_t, pairs)], [args.calls, args.loop_calls], args.rounds)
    rows.append("3. urban_centre_table(height, build, the 301 zones): mean / std / max / n / count, 256-bin histogram, class counts, read back")
    TS.report(rows, ["(a) urban_centre_table: zone_sums + two zone_histograms + one copy", "(c) stock: (c) of 2 with two bincounts per zone, one copy"],
              med, [0, 0])
    rows.append("")
    print("\n".join(rows[-4:]), flush=True)

    prop = torch.cuda.get_device_properties(0)
    head = ["Polygon zones on the device; device %s (%s, %d CUs, %.0f GB); torch %s, HIP %s"
            % (prop.name, getattr(prop, "gcnArchName", "?"), prop.multi_processor_count, prop.total_memory / 2 ** 30, torch.__version__,
               torch.version.hip),
            "one process; HIP events around one call each, all sides warmed up, %d alternations of %d calls per side (%d for the loops over 301"
            % (args.rounds, args.calls, args.loop_calls),
            "zones), median of the rounds' medians (range of the rounds' medians); two (height, class) pairs of %.0f MB in rotation.  All sides"
            % (H * W * 3 / 1e6),
            "checked equal first.  (a) finds its tables on the Zones object, (a0) builds and uploads them; (b) rasterises nothing (its mask is resident);",
            "GB/s: the bounding boxes' bytes of both rasters over the time.  Not measured: uint8 values, other raster sizes, zones with holes or",
            "many parts, item_pixels other than the default, the histogram kernel alone, shapefile reading, more than one GPU.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(head + rows) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
