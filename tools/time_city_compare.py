#!/usr/bin/env python
"""Time the city comparison (city_compare.pair_sums / class_sums / city_validation; csrc/srbh_compare.hip) against a floor -- an existing
kernel of this library that reads the same bytes less one raster -- and against what a user writes without it, in ONE process.

    python tools/time_city_compare.py [--out profiles/city_compare_bench.txt] [--rounds 5] [--calls 6] [--variant-lib PATH]

Workload: 16 000 x 12 000 rasters (uint16 predicted height, uint16 reference height, uint8 class): predict_city's output size.  The
reference raster is 82 % zeros, like the reference's label histogram.
  1. pair_sums over the 3 888 fishnet windows of 256 / 224: (a) pair_sums(height, ref, pos, build); (b) the floor window_sums(height, pos,
     build), which reads the same windows less one raster; (c) the best stock form found: int64 integral images (cumsum twice) of the
     selection, d, |d|, d^2, p, r, p^2, r^2 and p r, four gathers per window each;
  2. class_sums(height, ref, edges, build), C = 7: (a) every pixel compared -- almost all of them hit class 0, the contended case; (b) the
     same under mode "ref", threshold 0; (c) the floor value_histogram(height, 10, 256, build); (d) / (e) the stock forms of (a) / (b):
     torch.bincount of class_ref * C + class_pred plus seven masked reductions; with --variant-lib, (f) / (g): (a) / (b) through another
     build of the library (the in-LDS scheme that was NOT kept: -DSRBH_PAIR_CLASS_DIRECT=1, one LDS update per pixel and table entry);
  3. city_validation whole, host time and read-back included, against the stock expressions.
torch does no arithmetic on uint16, so every stock form starts with ``.to(torch.int32)``, inside its timed region: it is what a user has
to write.  HIP events around ONE call each; every side warmed up, then --rounds alternations of --calls calls per side; the median of the
rounds' medians with the range of the rounds' medians.  Each call takes the next of two triples of 960 MB each: more than the 256 MiB
Infinity Cache.  All sides are checked equal before anything is timed.  Nothing here reads a GeoTIFF: the rasters are seeded random
blobs made on the device."""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from srbh_amd import _lib  # noqa: E402
from srbh_amd import city_compare as CC  # noqa: E402
from srbh_amd import city_grid as CG  # noqa: E402
from srbh_amd import city_summary as CS  # noqa: E402

DEV = "cuda:0"
L3_BYTES = 256 * 2 ** 20
H, W = 12000, 16000
EDGES = CC.DEFAULT_EDGES
C = len(EDGES)


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


def make_triple(g):
    """class blobs at a 64-pixel scale, predicted heights round(10 h) of a skewed distribution up to 200 m, zero where nothing was
    predicted; the reference: the prediction +- 5 m on 18 % of the pixels (inside the blobs), zero elsewhere"""
    coarse = torch.rand((H // 64 + 1, W // 64 + 1), generator=g, device=DEV) < 0.35
    m = coarse.repeat_interleave(64, 0).repeat_interleave(64, 1)[:H, :W] & (torch.rand((H, W), generator=g, device=DEV) < 0.8)
    build = (m.to(torch.uint8) * torch.randint(1, 7, (H, W), generator=g, device=DEV, dtype=torch.uint8)).contiguous()
    h = (torch.rand((H, W), generator=g, device=DEV) ** 3 * 2000).round().to(torch.int16)
    h = torch.where((build > 0) | (torch.rand((H, W), generator=g, device=DEV) < 0.02), h, torch.zeros_like(h))
    noise = torch.randint(-50, 51, (H, W), generator=g, device=DEV, dtype=torch.int16)
    ref = torch.where((build > 0) & (torch.rand((H, W), generator=g, device=DEV) < 0.72), torch.clamp(h + noise, min=0), torch.zeros_like(h))
    return h.contiguous().view(torch.uint16), ref.contiguous().view(torch.uint16), build


def bench(fns, calls, rounds):
    for fn in fns:                                                    # every side warmed up
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    med = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            med[i].append(statistics.median(event_ms(fn) for _ in range(calls)))
    return med


def report(rows, names, med, in_bytes):
    for name, m, nbytes in zip(names, med, in_bytes):
        v = statistics.median(m)
        rows.append("   %-66s %10.4f ms (rounds %10.4f .. %10.4f)%s" % (name, v, min(m), max(m),
                                                                       "  %6.0f GB/s" % (nbytes / (v * 1e-3) / 1e9) if nbytes else ""))


def verdict(rows, what, mine, other, byte_ratio=None):
    """`mine` against `other`, round by round"""
    ratio = " ".join("%.3g" % (x / y) for x, y in zip(mine, other))
    ahead = all(x < y for x, y in zip(mine, other))
    extra = "" if byte_ratio is None else "; it reads %.2f x the bytes" % byte_ratio
    rows.append("   %s: time ratio per round %s (median %.3g)%s -- %s" % (what, ratio, statistics.median(mine) / statistics.median(other), extra,
                                                                         "ahead in every round" if ahead else "NOT ahead"))


def to_i32(t):
    return t.to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "city_compare_bench.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--variant-lib", default=None, help="another build of libsrbh.so whose srbh_pair_class_sums is timed beside the tree's")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    g = torch.Generator(device=DEV).manual_seed(23)
    triples = [make_triple(g) for _ in range(2)]
    assert len(triples) * H * W * 5 > L3_BYTES
    h0, r0, b0 = triples[0]
    zeros = float((r0.view(torch.int16) == 0).double().mean())
    assert 0.80 < zeros < 0.84, zeros
    rows = ["reference raster: %.1f %% zeros" % (100 * zeros), ""]

    # ---- 1. the per-cell table ---------------------------------------------------------------------------------------------------------
    pos = CG.fishgrid_windows(W, H, 256, 224)
    assert pos.shape == (3888, 4)
    pos_d = torch.from_numpy(pos.astype(np.int32)).to(DEV)
    x0, y0 = (torch.from_numpy(pos[:, k].copy()).to(DEV) for k in (0, 1))
    x1, y1 = x0 + 256, y0 + 256

    def ours(h, r, b):
        return CC.pair_sums(h, r, pos_d, b)

    def floor(h, r, b):
        return CS.window_sums(h, pos_d, b)

    def integral(h, r, b):
        p32, r32 = to_i32(h), to_i32(r)
        sel = ((p32 > 0) | (r32 > 0)) & (b > 0)
        p64, r64 = torch.where(sel, p32, 0).to(torch.int64), torch.where(sel, r32, 0).to(torch.int64)
        d = p64 - r64
        res = []
        for img in (sel.to(torch.int64), d, d.abs(), d * d, p64, r64, p64 * p64, r64 * r64, p64 * r64):
            ii = torch.nn.functional.pad(img.cumsum(0).cumsum(1), (1, 0, 1, 0))
            res.append(ii[y1, x1] - ii[y0, x1] - ii[y1, x0] + ii[y0, x0])
            del ii, img
        return torch.stack(res, 1)

    got = ours(h0, r0, b0)
    assert torch.equal(got[:, 1:], integral(h0, r0, b0))
    assert torch.equal(CC.pair_sums(h0, r0, pos_d, b0, mode="pred")[:, [0, 1, 5, 7]], floor(h0, r0, b0)[:, :4])
    assert int(got[:, 0].min()) == 65536 and 0 < int((got[:, 1] == 0).sum()) < len(pos)
    med = bench([rotating(ours, triples), rotating(floor, triples), rotating(integral, triples)], args.calls, args.rounds)
    px = float((pos[:, 2] * pos[:, 3]).sum())
    rows.append("1. pair_sums: 3 888 windows of 256 / 224 over 16 000 x 12 000 (uint16 height, uint16 reference, uint8 class)")
    report(rows, ["(a) pair_sums, device windows: one launch", "(b) floor: window_sums(height, pos, build) over the same windows",
                  "(c) stock: nine int64 integral images + four gathers each"], med, [px * 5, px * 3, 0])
    verdict(rows, "(a) against the floor (b)", med[0], med[1], 5 / 3)
    verdict(rows, "(a) against the stock form (c)", med[0], med[2])
    rows += ["   windows' bytes %.1f MB of %.1f MB of rasters (overlaps counted)" % (px * 5 / 1e6, H * W * 5 / 1e6), ""]
    print("\n".join(rows), flush=True)
    nprinted = len(rows)

    # ---- 2. the classes ------------------------------------------------------------------------------------------------------------------
    lib = _lib.lib()
    ws = torch.empty(lib.srbh_pair_class_ws_bytes(H, W, C) // 8, dtype=torch.int64, device=DEV)
    hws = torch.empty(lib.srbh_value_hist_ws_bytes(H, W, 256), dtype=torch.uint8, device=DEV)
    edges_t = torch.tensor(EDGES[1:], dtype=torch.int32, device=DEV)

    def ours_all(h, r, b):
        return CC.class_sums(h, r, EDGES, b, workspace=ws)[0]

    def ours_ref(h, r, b):
        return CC.class_sums(h, r, EDGES, b, mode="ref", ref_threshold=0, workspace=ws)[0]

    def floor_h(h, r, b):
        return CS.value_histogram(h, 10, 256, b, workspace=hws)

    def stock(h, r, b, ref_only):
        p32, r32, b64 = to_i32(h), to_i32(r), b.to(torch.int64)
        if ref_only:
            sel = r32 > 0
            p32, r32, b64 = p32[sel], r32[sel], b64[sel]
        cr = torch.bucketize(r32, edges_t, right=True)
        cm = torch.bincount((cr * C + b64).reshape(-1), minlength=C * C).reshape(C, C)
        d = (p32 - r32).to(torch.int64)
        out = []
        for c in range(C):                                            # seven masked reductions
            dc = d[cr == c]
            out.append(torch.stack([torch.tensor(dc.numel(), device=DEV), dc.sum(), dc.abs().sum(), (dc * dc).sum()]))
        return torch.cat([torch.stack(out), cm], 1)

    variant = None
    if args.variant_lib:
        vlib = ctypes.CDLL(args.variant_lib)
        vfn = vlib.srbh_pair_class_sums
        vfn.restype, vfn.argtypes = _lib.SIGNATURES["srbh_pair_class_sums"]
        e_arr = (ctypes.c_int * C)(*EDGES)

        def variant(h, r, b, mode, rthr):
            out = torch.empty(C * (4 + C) + 1, dtype=torch.int64, device=DEV)
            rc = vfn(h.data_ptr(), 1, W, r.data_ptr(), 1, W, b.data_ptr(), 3, W, H, W, e_arr, C, mode, -1, rthr, -1, out.data_ptr(), ws.data_ptr(),
                     _lib.stream_ptr())
            assert rc == 0, rc
            return out[:-1].view(C, 4 + C)

    a_all, a_ref = ours_all(h0, r0, b0), ours_ref(h0, r0, b0)
    assert torch.equal(a_all, stock(h0, r0, b0, False)) and torch.equal(a_ref, stock(h0, r0, b0, True))
    assert int(a_all[:, 0].sum()) == H * W and a_all[0, 0] > 0.8 * H * W and (a_ref[1:, 0] > 0).all()
    sides = [rotating(ours_all, triples), rotating(ours_ref, triples), rotating(floor_h, triples),
             rotating(lambda h, r, b: stock(h, r, b, False), triples), rotating(lambda h, r, b: stock(h, r, b, True), triples)]
    names = ["(a) class_sums, every pixel compared (contended: 82 % class 0)", "(b) class_sums, mode \"ref\", threshold 0",
             "(c) floor: value_histogram(height, 10, 256, build)", "(d) stock form of (a): bucketize, bincount, seven masked reductions",
             "(e) stock form of (b)"]
    nbytes = [H * W * 5.0, H * W * 5.0, H * W * 3.0, 0, 0]
    if variant:
        assert torch.equal(variant(h0, r0, b0, 0, -1), a_all) and torch.equal(variant(h0, r0, b0, 2, 0), a_ref)
        sides += [rotating(lambda h, r, b: variant(h, r, b, 0, -1), triples), rotating(lambda h, r, b: variant(h, r, b, 2, 0), triples)]
        names += ["(f) (a) through the variant library (scheme not kept)", "(g) (b) through the variant library (scheme not kept)"]
        nbytes += [H * W * 5.0, H * W * 5.0]
    med = bench(sides, args.calls, args.rounds)
    rows.append("2. class_sums(height, ref, edges, build), C = %d, edges %s" % (C, list(EDGES)))
    report(rows, names, med, nbytes)
    verdict(rows, "(a) against the floor (c)", med[0], med[2], 5 / 3)
    verdict(rows, "(b) against the floor (c)", med[1], med[2], 5 / 3)
    verdict(rows, "(a) against its stock form (d)", med[0], med[3])
    verdict(rows, "(b) against its stock form (e)", med[1], med[4])
    if variant:
        verdict(rows, "(a) kept scheme against the variant (f)", med[0], med[5])
        verdict(rows, "(b) kept scheme against the variant (g)", med[1], med[6])
    rows.append("")
    print("\n".join(rows[nprinted:]), flush=True)
    nprinted = len(rows)

    # ---- 3. the whole city -----------------------------------------------------------------------------------------------------------------
    def ours_c(h, r, b):
        return CC.city_validation(h, r, b)

    def stock_c(h, r, b):
        rows_ = stock(h, r, b, False)
        p, q = to_i32(h).double(), to_i32(r).double()
        d = p - q
        n = float(d.numel())
        vals = torch.stack([d.mean(), d.abs().mean(), (d * d).mean().sqrt(), p.mean(), q.mean(),
                            ((p - p.mean()) * (q - q.mean())).mean() / (p.std(unbiased=False) * q.std(unbiased=False))]).cpu().tolist()
        t = rows_.cpu().numpy()
        nn = np.maximum(t[:, 0], 1).astype(np.float64)
        return {"stats": np.stack([np.sqrt(t[:, 3] / nn) * t[:, 0], t[:, 2].astype(np.float64), t[:, 1].astype(np.float64)], 1), "cm": t[:, 4:],
                "vals": vals, "n": n}

    mine, theirs = ours_c(h0, r0, b0), stock_c(h0, r0, b0)
    assert np.array_equal(mine["seg"].getConfusionMatrix().cpu().numpy(), theirs["cm"].astype(np.float64))
    assert np.allclose(mine["height"].stats.cpu().numpy(), theirs["stats"], rtol=1e-12, atol=0)
    for k, v in zip(("me", "mae", "rmse", "mean_pred", "mean_ref", "r"), theirs["vals"]):
        assert abs(mine["sums"][k][0] - v) <= 1e-9 * max(abs(v), 1.0), (k, mine["sums"][k][0], v)
    med = bench([rotating(ours_c, triples), rotating(stock_c, triples)], args.calls, args.rounds)
    rows.append("3. city_validation(height, ref, build): HeightMetric, SegmentationMetric and the whole raster's measures, read back (host time included)")
    report(rows, ["(a) city_validation: class_sums + pair_sums + one copy", "(b) stock: (2d) + float64 means, rmse and Pearson r, read back"],
           med, [H * W * 9.0, 0])
    verdict(rows, "(a) against the stock expressions (b)", med[0], med[1])
    rows += ["   (a) reads the two height rasters twice and the class raster once: the GB/s counts those bytes", ""]
    print("\n".join(rows[nprinted:]), flush=True)

    prop = torch.cuda.get_device_properties(0)
    head = ["City comparison on the device; device %s (%s, %d CUs, %.0f GB); torch %s, HIP %s"
            % (prop.name, getattr(prop, "gcnArchName", "?"), prop.multi_processor_count, prop.total_memory / 2 ** 30, torch.__version__,
               torch.version.hip),
            "one process; HIP events around one call each, all sides warmed up, %d alternations of %d calls per side, median of the rounds'"
            % (args.rounds, args.calls),
            "medians (range of the rounds' medians); two (height, reference, class) triples of %.0f MB in rotation.  All sides checked equal"
            % (H * W * 5 / 1e6),
            "first.  Stock forms convert uint16 to int32 first (torch does no arithmetic on uint16).  Not measured: uint8 heights, other raster",
            "sizes, other C, more than one GPU, anything that reads a file.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(head + rows) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
