#!/usr/bin/env python
"""Two builds of libsrbh against each other on the city kernels: same integers, same speed.

    python tools/ab_raster_walk.py --parent-lib /path/to/parent/libsrbh.so [--group rect|zones] [--rounds 9] [--bits-out ...] [--bench-out ...]

Both libraries (one ABI) are loaded into ONE process; the Python layer of this tree drives either.  Two groups of entries (--group; both
by default): "rect", the rectangle kernels of csrc/srbh_cells.hip and csrc/srbh_summary.hip -- workloads, rasters and method of
tools/time_city_grid.py and tools/time_city_summary.py (their make_mask / make_pair / event_ms / rotating are imported) --, and "zones",
the zone and pair kernels of csrc/srbh_zones.hip, csrc/srbh_compare.hip and csrc/srbh_zone_compare.hip (zone_sums, zone_histogram,
zone_pair_sums, pair_sums, class_sums) on tools/time_city_compare.py's triple and tools/time_city_zones.py's two zone sets.
  bits   every entry on every element-size pairing: sha256 of the result of either library, which must be equal;
  bench  HIP events around one call each, every side warmed up, buffers in rotation beyond the 256 MiB Infinity Cache, --rounds
         alternations (the side that goes first alternates too) of the tools' calls per side; per line the rounds' medians, their median
         and the verdict: the tree's median must not lie above the parent's by more than the parent's own spread (largest minus smallest
         round median)."""
import argparse
import ctypes
import hashlib
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import time_city_compare as TC  # noqa: E402
import time_city_grid as TG  # noqa: E402
import time_city_summary as TS  # noqa: E402
import time_city_zones as TZ  # noqa: E402
from srbh_amd import _lib  # noqa: E402
from srbh_amd import city_compare as CC  # noqa: E402
from srbh_amd import city_grid as CG  # noqa: E402
from srbh_amd import city_summary as CS  # noqa: E402
from srbh_amd import city_zone_compare as CZC  # noqa: E402
from srbh_amd import city_zones as CZ  # noqa: E402

DEV = "cuda:0"
LIBS = {}


def load(path):
    lib = ctypes.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def on(side, fn):
    def call(*a):
        _lib._lib = LIBS[side]
        return fn(*a)
    return call


def digest(t):
    if isinstance(t, dict):
        t = np.concatenate([np.asarray([t["count"], t["n"], t["max"]], dtype=np.int64), t["hist"], t["class_counts"],
                            np.asarray([t["mean"], t["std"]], dtype=np.float64).view(np.int64)])
    elif isinstance(t, tuple):                                          # (class_sums: the rows and bad)
        t = torch.cat([x.reshape(-1) for x in t]).cpu().numpy()
    else:
        t = t.cpu().numpy()
    return hashlib.sha256(np.ascontiguousarray(t).tobytes()).hexdigest()[:16]


def as_dtype(t, dtype):
    """a seeded uint8 / uint16 raster as another element type: uint8 -> 257 v (both bytes count), uint16 -> v >> 3 (heights stay below 256)"""
    if t.dtype == dtype:
        return t
    if t.dtype == torch.uint8:
        return (t.to(torch.int32) * 257).to(torch.int16).view(dtype)
    return (t.view(torch.int16) >> 3).to(torch.uint8)


def both(rows, name, fn, *a):
    d = {side: digest(on(side, fn)(*a)) for side in ("parent", "tree")}
    rows.append("%-72s %s %s %s" % (name, d["parent"], d["tree"], "equal" if d["parent"] == d["tree"] else "DIFFERENT"))
    print(rows[-1], flush=True)
    return d["parent"] == d["tree"]


def zone_workloads():
    """-> [(tag, Zones)] of tools/time_city_zones.py's two sets, and time_city_compare's fishnet as device windows"""
    one, many = TZ.zone_sets()
    pos_d = torch.from_numpy(CG.fishgrid_windows(TC.W, TC.H, 256, 224).astype(np.int32)).to(DEV)
    return [("one zone of 1000 vertices", CZ.zone_edges(one)), ("301 zones", CZ.zone_edges(many))], pos_d


def bits_zones(rows):
    ok = True
    h16, r16, b8 = TC.make_triple(torch.Generator(device=DEV).manual_seed(23))
    sets, pos_d = zone_workloads()
    for tv in (torch.uint16, torch.uint8):
        for tm in (None, torch.uint8, torch.uint16):
            v, m = as_dtype(h16, tv), None if tm is None else as_dtype(b8, tm)
            for ztag, zones in sets:
                tag = "%s / %s, %s" % (tv, tm, ztag)
                ok &= both(rows, "zone_sums %s" % tag, CZ.zone_sums, v, zones, m)
                ok &= both(rows, "zone_histogram %s, 10, 256" % tag, CZ.zone_histogram, v, zones, 10, 256, m)
            for tr in (torch.uint16, torch.uint8):
                r = as_dtype(r16, tr)
                tag = "%s / %s / %s" % (tv, tr, tm)
                for ztag, zones in sets:
                    ok &= both(rows, "zone_pair_sums %s, %s" % (tag, ztag), CZC.zone_pair_sums, v, r, zones, m)
                ok &= both(rows, "pair_sums %s, %d windows" % (tag, len(pos_d)), CC.pair_sums, v, r, pos_d, m)
                ok &= both(rows, "class_sums %s, C = %d" % (tag, TC.C), CC.class_sums, v, r, TC.EDGES, m)
                del r
            del v, m
    return ok


def bits(rows, groups):
    ok = True
    if "rect" in groups:
        ok &= bits_rect(rows)
    if "zones" in groups:
        ok &= bits_zones(rows)
    rows.append("ALL EQUAL" if ok else "SOME DIFFER")
    return ok


def bits_rect(rows):
    ok = True
    g = torch.Generator(device=DEV).manual_seed(20)
    for H, W in ((3000, 4000), (7900, 7900)):
        pos_d = torch.from_numpy(CG.fishgrid_windows(W, H).astype(np.int32)).to(DEV)
        m8 = TG.make_mask(H, W, g)
        o8 = torch.roll(m8, 3, 1)
        for ta in (torch.uint8, torch.uint16):
            for tb in (None, torch.uint8, torch.uint16):
                a, b = as_dtype(m8, ta), None if tb is None else as_dtype(o8, tb)
                ok &= both(rows, "cell_counts %d x %d %s / %s, %d windows" % (H, W, ta, tb, len(pos_d)), CG.cell_counts, a, pos_d, b)
        a, b = as_dtype(m8, torch.uint16).view(torch.int16), as_dtype(o8, torch.uint16).view(torch.int16)
        ok &= both(rows, "cell_counts %d x %d int16 / int16, the value itself, threshold -1" % (H, W), lambda: CG.cell_counts(a, pos_d, b, -1, False))
    del m8, o8, a, b
    g = torch.Generator(device=DEV).manual_seed(21)
    h16, b8 = TS.make_pair(g)
    H, W = h16.shape
    pos_d = torch.from_numpy(CG.fishgrid_windows(W, H, 256, 224).astype(np.int32)).to(DEV)
    for tv in (torch.uint16, torch.uint8):
        for tm in (None, torch.uint8, torch.uint16):
            v, m = as_dtype(h16, tv), None if tm is None else as_dtype(b8, tm)
            tag = "%d x %d %s / %s" % (H, W, tv, tm)
            ok &= both(rows, "window_sums %s, %d windows" % (tag, len(pos_d)), CS.window_sums, v, pos_d, m)
            for block in (4, 40, 400):
                ok &= both(rows, "block_sums %s, block %d" % (tag, block), CS.block_sums, v, block, m)
            ok &= both(rows, "value_histogram %s, 10, 256" % tag, CS.value_histogram, v, 10, 256, m)
            del v, m
    ok &= both(rows, "city_summary %d x %d uint16 / uint8" % (H, W), CS.city_summary, h16, b8)
    return ok


def bench_line(rows, name, fn, bufs, calls, rounds):
    sides = {s: TS.rotating(on(s, fn), bufs) for s in ("parent", "tree")}
    for s in sides.values():                                          # every side warmed up
        for _ in range(2):
            s()
    torch.cuda.synchronize()
    med = {"parent": [], "tree": []}
    for r in range(rounds):
        for side in (("parent", "tree") if r % 2 == 0 else ("tree", "parent")):
            med[side].append(statistics.median(TS.event_ms(sides[side]) for _ in range(calls)))
    p, t = statistics.median(med["parent"]), statistics.median(med["tree"])
    spread = max(med["parent"]) - min(med["parent"])
    ok = t <= p + spread
    rows += ["%s" % name,
             "   parent rounds: %s" % " ".join("%.4f" % x for x in med["parent"]),
             "   tree rounds:   %s" % " ".join("%.4f" % x for x in med["tree"]),
             "   parent %.4f ms, tree %.4f ms (%+.2f %%), parent's spread %.4f ms (%.2f %%): %s"
             % (p, t, 100 * (t - p) / p, spread, 100 * spread / p, "PASS" if ok else "FAIL")]
    print("\n".join(rows[-4:]), flush=True)
    return ok


def bench_zones(rows, rounds):
    ok = True
    g = torch.Generator(device=DEV).manual_seed(23)
    triples = [TC.make_triple(g) for _ in range(2)]
    assert len(triples) * TC.H * TC.W * 5 > TC.L3_BYTES
    small = [(as_dtype(h, torch.uint8), as_dtype(r, torch.uint8), b) for h, r, b in triples]      # the forms with 16 pixels to a group
    sets, pos_d = zone_workloads()
    lib = _lib.lib()
    cws = torch.empty(lib.srbh_pair_class_ws_bytes(TC.H, TC.W, TC.C), dtype=torch.uint8, device=DEV)
    for ztag, zones in sets:
        NI = len(CZ.zone_items(zones, TC.H, TC.W)[0])
        ws = torch.empty(max(lib.srbh_zone_hist_ws_bytes(NI, 256), lib.srbh_zone_pair_ws_bytes(NI)), dtype=torch.uint8, device=DEV)
        for ttag, bufs in (("uint16 height and reference, uint8 class", triples), ("uint8 height and reference, uint8 class", small)):
            tag = "%s, %d items, %s" % (ztag, NI, ttag)
            ok &= bench_line(rows, "zone_sums(height, zones, build), " + tag, lambda h, r, b: CZ.zone_sums(h, zones, b, workspace=ws), bufs, 6, rounds)
            ok &= bench_line(rows, "zone_histogram(height, zones, 10, 256, build), " + tag,
                             lambda h, r, b: CZ.zone_histogram(h, zones, 10, 256, b, workspace=ws), bufs, 6, rounds)
            ok &= bench_line(rows, "zone_pair_sums(height, ref, zones, build), " + tag,
                             lambda h, r, b: CZC.zone_pair_sums(h, r, zones, b, workspace=ws), bufs, 6, rounds)
    for ttag, bufs in (("uint16 height and reference, uint8 class", triples), ("uint8 height and reference, uint8 class", small)):
        ok &= bench_line(rows, "pair_sums(height, ref, %d windows of 256 / 224, build), %s" % (len(pos_d), ttag),
                         lambda h, r, b: CC.pair_sums(h, r, pos_d, b), bufs, 6, rounds)
        ok &= bench_line(rows, "class_sums(height, ref, edges, build), C = %d, %s" % (TC.C, ttag),
                         lambda h, r, b: CC.class_sums(h, r, TC.EDGES, b, workspace=cws), bufs, 6, rounds)
    return ok


def bench(rows, rounds, groups):
    ok = True
    if "rect" in groups:
        ok &= bench_rect(rows, rounds)
    if "zones" in groups:
        ok &= bench_zones(rows, rounds)
    rows.append("ALL PASS" if ok else "SOME FAIL")
    return ok


def bench_rect(rows, rounds):
    ok = True
    g = torch.Generator(device=DEV).manual_seed(20)
    for H, W, nmasks in ((3000, 4000, 24), (7900, 7900, 5)):
        pos_d = torch.from_numpy(CG.fishgrid_windows(W, H).astype(np.int32)).to(DEV)
        masks = [TG.make_mask(H, W, g) for _ in range(nmasks)]
        pairs = [(m, torch.roll(m, 3, 1)) for m in masks]
        assert nmasks * H * W > TG.L3_BYTES
        tag = "%d x %d uint8, %d windows of 64 / 56" % (H, W, len(pos_d))
        ok &= bench_line(rows, "cell_counts, one raster, " + tag, lambda m, o: CG.cell_counts(m, pos_d), pairs, 10, rounds)
        ok &= bench_line(rows, "cell_counts, two rasters, " + tag, lambda m, o: CG.cell_counts(m, pos_d, o), pairs, 10, rounds)
        if nmasks == 24:
            pairs16 = [(as_dtype(m, torch.uint16), as_dtype(o, torch.uint16)) for m, o in pairs]
            tag = tag.replace("uint8", "uint16")
            ok &= bench_line(rows, "cell_counts, one raster, " + tag, lambda m, o: CG.cell_counts(m, pos_d), pairs16, 10, rounds)
            ok &= bench_line(rows, "cell_counts, two rasters, " + tag, lambda m, o: CG.cell_counts(m, pos_d, o), pairs16, 10, rounds)
            del pairs16
        del masks, pairs
    g = torch.Generator(device=DEV).manual_seed(21)
    pairs = [TS.make_pair(g) for _ in range(2)]
    H, W = TS.H, TS.W
    pos_d = torch.from_numpy(CG.fishgrid_windows(W, H, 256, 224).astype(np.int32)).to(DEV)
    ws = torch.empty(_lib.lib().srbh_value_hist_ws_bytes(H, W, 256), dtype=torch.uint8, device=DEV)
    tag = "%d x %d uint16 height, uint8 class" % (H, W)
    ok &= bench_line(rows, "window_sums, %d windows of 256 / 224, %s" % (len(pos_d), tag), lambda h, b: CS.window_sums(h, pos_d, b), pairs, 6, rounds)
    for block in (4, 40, 400):
        ok &= bench_line(rows, "block_sums, block %d, %s" % (block, tag), lambda h, b: CS.block_sums(h, block, b), pairs, 6, rounds)
    ok &= bench_line(rows, "value_histogram(height, 10, 256, build), " + tag, lambda h, b: CS.value_histogram(h, 10, 256, b, workspace=ws), pairs, 6, rounds)
    ok &= bench_line(rows, "city_summary(height, build) whole, host time included, " + tag, CS.city_summary, pairs, 6, rounds)
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--bits-out", default=os.path.join(ROOT, "profiles", "raster_walk_bits.txt"))
    ap.add_argument("--bench-out", default=os.path.join(ROOT, "profiles", "raster_walk_bench.txt"))
    ap.add_argument("--only", choices=["bits", "bench"], default=None)
    ap.add_argument("--group", choices=["rect", "zones"], default=None, help="one group of entries (default: both)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    LIBS["parent"], LIBS["tree"] = load(args.parent_lib), load(_lib.LIB_PATH)
    prop = torch.cuda.get_device_properties(0)
    dev = "device %s (%s, %d CUs); torch %s, HIP %s" % (prop.name, getattr(prop, "gcnArchName", "?"), prop.multi_processor_count,
                                                        torch.__version__, torch.version.hip)
    ok = True
    for part, out, head in (("bits", args.bits_out, "City kernels, parent library against this tree's: sha256 (first 16 hex digits) of every "
                             "result, parent then tree; " + dev),
                            ("bench", args.bench_out, "City kernels, parent library against this tree's in one process, %d alternations; "
                             "ms per call, medians of the tools' calls per round; " % args.rounds + dev)):
        if args.only in (None, part):
            rows = [head, ""]
            groups = (args.group,) if args.group else ("rect", "zones")
            ok &= bits(rows, groups) if part == "bits" else bench(rows, args.rounds, groups)
            os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
            with open(out, "w") as fh:
                fh.write("\n".join(rows) + "\n")
            print("wrote", out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
