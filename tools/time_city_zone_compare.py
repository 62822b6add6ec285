#!/usr/bin/env python
"""Time the urban-centre validation (city_zone_compare.zone_pair_sums / urban_centre_validation; csrc/srbh_zone_compare.hip) against two
floors and against what a user has without it, in ONE process.

    python tools/time_city_zone_compare.py [--out profiles/city_zone_compare_bench.txt] [--rounds 5] [--calls 6] [--loop-calls 2]

Workload: tools/time_city_compare.py's 16 000 x 12 000 triple (uint16 height, uint16 reference with about 82 % zeros, uint8 class) and the
two zone sets of tools/time_city_zones.py:
  1. ONE zone of 1000 vertices covering about half the raster;
  2. 301 zones of about 300 x 300 pixels;
  3. urban_centre_validation(height, ref, build, the 301 zones) whole, read back, host time included.
Sides of 1 and 2:
  (z) zone_pair_sums(height, ref, zones, build) with its tables resident on the Zones object (the steady state);
  (a) zone_sums(height, zones, build) on the same zones: the floor of the rasterising part -- it reads one raster fewer (3 bytes a pixel
      against 5) and keeps four sums, not nine;
  (b) pair_sums(height, ref, the items' bands as plain windows, build): the floor if the zone test were free (it sums the whole boxes, so
      its numbers differ from (z)'s; its count column is checked against the boxes' areas);
  (c) the best stock-torch form found: per zone the crossing test of tools/time_city_zones.py (int64 crossings, scatter_add_, cumsum), then
      masked sums of the bounding box behind .to(int32) (torch does no arithmetic on uint16).
For 3: urban_centre_validation against urban_centre_table plus the stock comparison (c), each with its read-back.
HIP events around ONE call each; every side warmed up, then --rounds alternations of --calls calls per side (--loop-calls for the loops
over 301 zones); the median of the rounds' medians with the range of the rounds' medians.  Each call takes the next of two triples of
960 MB each: more than the 256 MiB Infinity Cache.  (z) and (c) are checked equal before anything is timed."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import time_city_compare as TC  # noqa: E402
import time_city_summary as TS  # noqa: E402
import time_city_zones as TZ  # noqa: E402
from srbh_amd import city_compare as CC  # noqa: E402
from srbh_amd import city_zone_compare as CZC  # noqa: E402
from srbh_amd import city_zones as CZ  # noqa: E402

DEV = TS.DEV
H, W = TS.H, TS.W


def stock_rows(edges, pos, h, r, b):
    """(Z, 10) int64 by stock ops: per zone the crossing mask of its bounding box, then masked sums"""
    out = []
    for e, (x, y, w, hh) in zip(edges, pos.tolist()):
        inz = TZ.torch_zone_mask(e, x, x + w, y, y + hh)
        p32, r32 = TS.to_i32(h[y:y + hh, x:x + w]), TS.to_i32(r[y:y + hh, x:x + w])
        sel = inz & ((p32 > 0) | (r32 > 0)) & (b[y:y + hh, x:x + w] > 0)
        zero = torch.zeros_like(p32)
        p, q = torch.where(sel, p32, zero).to(torch.int64), torch.where(sel, r32, zero).to(torch.int64)
        d = p - q
        out.append(torch.stack([inz.sum(), sel.sum(), d.sum(), d.abs().sum(), (d * d).sum(), p.sum(), q.sum(), (p * p).sum(), (q * q).sum(),
                                (p * q).sum()]))
    return torch.stack(out)


def report(rows, names, med, in_bytes):
    for name, m, nbytes in zip(names, med, in_bytes):
        v = statistics.median(m)
        rows.append("   %-66s %10.4f ms (rounds %10.4f .. %10.4f)%s" % (name, v, min(m), max(m),
                                                                       "  %6.0f GB/s" % (nbytes / (v * 1e-3) / 1e9) if nbytes else ""))
    for i in range(1, len(med)):
        ratio = " ".join("%.2f" % (x / y) for x, y in zip(med[i], med[0]))
        ahead = all(y < x for x, y in zip(med[i], med[0]))
        rows.append("   per round %s / %s: %s -- %s is %s" % (names[i][:3], names[0][:3], ratio, names[0][:3],
                                                               "ahead in every round" if ahead else "NOT AHEAD in every round"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "city_zone_compare_bench.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--loop-calls", type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    g = torch.Generator(device=DEV).manual_seed(21)
    triples = [TC.make_triple(g) for _ in range(2)]
    assert len(triples) * H * W * 5 > TS.L3_BYTES
    zeros = float((triples[0][1].view(torch.int16) == 0).double().mean())
    one, many = TZ.zone_sets()
    rows, nprinted, tables = ["reference raster: %.1f %% zeros" % (100 * zeros), ""], 0, {}
    for tag, polys, calls in (("1. one zone of 1000 vertices over about half the raster", one, args.calls),
                              ("2. 301 zones of about 300 x 300 pixels", many, args.loop_calls)):
        zones = CZ.zone_edges(polys)
        pos = TZ.boxes(zones)
        items = CZ.zone_items(zones, H, W)[0]
        ipos_d = torch.from_numpy(items[:, 1:].copy()).to(DEV)
        edges = [torch.from_numpy(zones.edges[zones.edge_off[k]:zones.edge_off[k + 1]].astype(np.int64)).to(DEV) for k in range(len(zones))]

        def ours(h, r, b):
            return CZC.zone_pair_sums(h, r, zones, b)

        def zsums(h, r, b):
            return CZ.zone_sums(h, zones, b)

        def bands(h, r, b):
            return CC.pair_sums(h, r, ipos_d, b)

        def stock(h, r, b):
            return stock_rows(edges, pos, h, r, b)

        got = ours(*triples[0])
        assert torch.equal(got, stock(*triples[0])) and int(got[:, 1].min()) > 0
        assert torch.equal(got[:, 0], zsums(*triples[0])[:, 0]) and int(bands(*triples[0])[:, 0].sum()) == int((pos[:, 2] * pos[:, 3]).sum())
        area = int(got[:, 0].sum())
        med = TS.bench([TS.rotating(ours, triples), TS.rotating(zsums, triples), TS.rotating(bands, triples), TS.rotating(stock, triples)],
                       [args.calls, args.calls, args.calls, calls], args.rounds)
        box = float((pos[:, 2] * pos[:, 3]).sum())
        rows.append("%s: %d edges, %d items, %.1f Mpixel in the zones, bounding boxes %.1f Mpixel" % (tag, len(zones.edges), len(items), area / 1e6,
                                                                                                  box / 1e6))
        report(rows, ["(z) zone_pair_sums, tables resident: two launches", "(a) floor of the rasterising: zone_sums(height, zones, build)",
                      "(b) floor if the zone test were free: pair_sums of the items' bands", "(c) stock: int64 crossings, scatter_add_, cumsum, masked sums"],
               med, [box * 5, box * 3, box * 5, 0])
        z, a_ = statistics.median(med[0]), statistics.median(med[1])
        rows.append("   bytes of the boxes: (z) reads 5 a pixel, (a) 3: ratio 1.67; time (z) / (a) = %.2f: (z) is %s that ratio" % (
            z / a_, "below" if z / a_ < 1.6 else "above" if z / a_ > 1.74 else "at"))
        rows.append("")
        print("\n".join(rows[nprinted:]), flush=True)
        nprinted = len(rows)
        tables[tag[0]] = (zones, edges, pos)

    # ---- 3. the table ----------------------------------------------------------------------------------------------------------------------
    zones, edges, pos = tables["2"]

    def ours_t(h, r, b):
        return CZC.urban_centre_validation(h, r, b, zones)

    def stock_t(h, r, b):
        t = CZ.urban_centre_table(h, b, zones)
        t.update({k: v for k, v in CC.errors_from_sums(stock_rows(edges, pos, h, r, b).cpu().numpy()).items() if k not in ("n", "count", "fraction")})
        return t

    def table_only(h, r, b):
        return CZ.urban_centre_table(h, b, zones)

    mine, theirs = ours_t(*triples[0]), stock_t(*triples[0])
    assert all(np.array_equal(mine[k], theirs[k], equal_nan=True) for k in theirs)
    med = TS.bench([TS.rotating(ours_t, triples), TS.rotating(table_only, triples), TS.rotating(stock_t, triples)],
                   [args.calls, args.calls, args.loop_calls], args.rounds)
    rows.append("3. urban_centre_validation(height, ref, build, the 301 zones): the centre table and the error measures, read back")
    report(rows, ["(z) urban_centre_validation: four calls, one cat, one copy", "(t) urban_centre_table alone (no comparison)",
                  "(c) urban_centre_table + the stock comparison (c) of 2, two copies"], med, [0, 0, 0])
    rows.append("")
    print("\n".join(rows[nprinted:]), flush=True)

    prop = torch.cuda.get_device_properties(0)
    head = ["Urban-centre validation on the device; device %s (%s, %d CUs, %.0f GB); torch %s, HIP %s"
            % (prop.name, getattr(prop, "gcnArchName", "?"), prop.multi_processor_count, prop.total_memory / 2 ** 30, torch.__version__,
               torch.version.hip),
            "one process; HIP events around one call each, all sides warmed up, %d alternations of %d calls per side (%d for the loops over 301"
            % (args.rounds, args.calls, args.loop_calls),
            "zones), median of the rounds' medians (range of the rounds' medians); two (height, reference, class) triples of %.0f MB in rotation."
            % (H * W * 5 / 1e6),
            "(z) and (c) checked equal first.  (a) reads one raster fewer and keeps four sums; (b) tests no zone and sums whole boxes.  GB/s: the",
            "bounding boxes' bytes of the rasters a side reads over its time.  Not measured: uint8 heights, other raster sizes, item_pixels other",
            "than the default, the first call (tables built and uploaded: profiles/city_zones_bench.txt (a0)), more than one GPU.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(head + rows) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
