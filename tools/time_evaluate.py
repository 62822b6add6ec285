#!/usr/bin/env python
"""Time the height-stage evaluation (srbh_amd.evaluate / harness.evaluate_tiles) against the path it replaces, in ONE process.

    python tools/time_evaluate.py [--out profiles/evaluate_bench.txt] [--runs 20] [--batch 64] [--tiles 128] [--tile-batch 32] [--blocks 23]

1. One batch of head outputs, B = 64, C = 7, 256 x 256 (height (B,1,H,W), logits channels_last as the head returns them, int64 labels):
   the fused ``HeightEvaluation.add`` (one srbh_eval_sums launch + its fold) against the reference loop body built from the code that was
   here before it: ``argmax`` + ``SegmentationMetric.addBatch`` + ``HeightMetric.addBatch`` + the two RMSE expressions of train.py:333-335 /
   :444 -- WITHOUT the reference's per-batch ``.item()``, which would only add a synchronisation to the replaced side.  The two are timed
   alternately (fused, replaced, fused, ...), HIP events around one call each, median / min / max of --runs after warm-up; once as plain
   calls (host included) and once as 10 calls replayed from a HIP graph (device time only).  Two copies of the batch are used in turn, so
   that a call does not find its inputs in the 256 MB last-level cache.  Achieved bytes/s
   = the algorithmic bytes (4 C + 4 + 4 + 8 per pixel) over the fused median; the MI355X's HBM peak is 8 TB/s.
2. ``evaluate_tiles`` per tile (captured graph per full batch, fused add) against the eager loop a user had before (eager forward per batch,
   the replaced scoring path, the reference's ``rmse.item()`` per batch): host clock around a whole pass ending in a synchronisation,
   alternated, median of --runs passes."""
import argparse
import os
import socket
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from srbh_amd import harness, synth  # noqa: E402
from srbh_amd.evaluate import HeightEvaluation  # noqa: E402
from srbh_amd.metrics import AverageMeter, HeightMetric, SegmentationMetric  # noqa: E402

DEV = "cuda:0"
HBM_PEAK = 8.0e12
GRAPH_REPS = 10


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def alternate(fns, runs, clock, warmup=3):
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(runs):
        for i, fn in enumerate(fns):
            ts[i].append(clock(fn))
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def fmt(s):
    return "%9.3f ms (min %8.3f, max %8.3f)" % s


def replaced_scoring(seg, hm, height, logits, ref, label):
    """the reference loop body between the forward and the progress bar (train.py:443-449, :333-335) on the classes that were here before"""
    ypred = height.squeeze(1)
    loss = torch.mean((ypred - ref) ** 2)
    rmse = torch.sqrt(((ypred - ref) ** 2).mean())
    build_pred = logits.argmax(1)
    seg.addBatch(build_pred, label)
    hm.addBatch(ypred, ref, label)
    return loss, rmse


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evaluate_bench.txt"))
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--tiles", type=int, default=128)
    ap.add_argument("--tile-batch", type=int, default=32)
    ap.add_argument("--blocks", type=int, default=23)
    args = ap.parse_args()
    assert args.runs >= 20, "the median is taken over at least 20 runs"
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    B, C, S = args.batch, 7, 256
    g = torch.Generator().manual_seed(17)
    label = torch.randint(0, C, (B, S // 8, S // 8), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2).to(DEV)
    ref = (torch.randint(0, 60, (B, S, S), generator=g).to(DEV) * (label > 0)).float()
    height = ref[:, None] + torch.randn((B, 1, S, S), generator=g).to(DEV) * 3
    logits = (torch.randn((B, C, S, S), generator=g) * 2).to(DEV).contiguous(memory_format=torch.channels_last)
    # two copies of the batch, used in turn: 2 x 185 MB do not fit the 256 MB last-level cache, so a call does not find its inputs there
    sets = [(height, logits, ref, label), tuple(t.clone(memory_format=torch.preserve_format) for t in (height, logits, ref, label))]
    sets_nchw = [(h, lg.contiguous(), r, lb) for h, lg, r, lb in sets]
    turn = [0]

    def batch_of(which):
        turn[0] ^= 1
        return which[turn[0]]

    rows = []

    ev = HeightEvaluation(C, DEV)
    seg, hm = SegmentationMetric(C, device=DEV), HeightMetric(C, device=DEV)

    def fused():
        ev.reset()
        ev.add(*batch_of(sets))

    def replaced():
        replaced_scoring(seg, hm, *batch_of(sets))

    f, r = alternate([fused, replaced], args.runs, event_ms)
    nbytes = B * S * S * (4 * C + 4 + 4 + 8)
    rows += ["1. scoring one batch: B = %d, C = %d, %d x %d, logits channels_last, int64 labels; two copies of the batch used in turn" % (B, C, S, S),
             "   fused HeightEvaluation.add (srbh_eval_sums + fold)        %s" % fmt(f),
             "   replaced: argmax + SegmentationMetric.addBatch + HeightMetric.addBatch + 2 RMSE expressions  %s" % fmt(r),
             "   ratio replaced / fused (medians) %.2f; algorithmic bytes %.1f MB -> %.0f GB/s at the fused median = %.1f %% of the 8 TB/s HBM peak"
             % (r[0] / f[0], nbytes / 1e6, nbytes / (f[0] * 1e-3) / 1e9, 100.0 * nbytes / (f[0] * 1e-3) / HBM_PEAK),
             "   (the fused time includes the fold kernel and the allocation of the per-batch result and workspace tensors)"]

    def fused_nchw():
        ev.reset()
        ev.add(*batch_of(sets_nchw))

    (fn,) = alternate([fused_nchw], args.runs, event_ms)
    rows += ["   fused, NCHW logits                                        %s" % fmt(fn)]

    # the same calls without the host between them: REPS calls captured into one HIP graph, HIP events around a replay, per call
    def replayed(fn):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(GRAPH_REPS):
                fn()
        return graph.replay

    gf, gr, gn = alternate([replayed(fused), replayed(replaced), replayed(fused_nchw)], args.runs, event_ms)
    per = lambda s: tuple(v / GRAPH_REPS for v in s)      # noqa: E731
    rows += ["   device time per call inside a replayed HIP graph of %d calls (no host between the launches):" % GRAPH_REPS,
             "   fused, channels_last logits                               %s" % fmt(per(gf)),
             "   fused, NCHW logits                                        %s" % fmt(per(gn)),
             "   replaced                                                  %s" % fmt(per(gr)),
             "   ratio replaced / fused (medians) %.2f; %.0f GB/s at the fused median = %.1f %% of the 8 TB/s HBM peak"
             % (gr[0] / gf[0], nbytes / (gf[0] / GRAPH_REPS * 1e-3) / 1e9, 100.0 * nbytes / (gf[0] / GRAPH_REPS * 1e-3) / HBM_PEAK), ""]
    for row in rows:
        print(row, flush=True)

    from srbh_amd.models import SRRegress_Cls_feature
    from srbh_amd.rrdbnet import RRDBNet
    net_hr = RRDBNet(3, 3, num_block=args.blocks)
    net_hr.load_state_dict(synth.rrdbnet_state_dict(num_block=args.blocks, seed=4, mode="stress"))
    net_hr = net_hr.to(DEV).eval()
    torch.manual_seed(12)
    model = SRRegress_Cls_feature("efficientnet-b4", in_channels=8, super_in=64, super_mid=16, upscale=4, isaggre=False, chans_build=C).to(DEV).eval()
    N, tb = args.tiles, args.tile_batch
    tiles = synth.tiles(N, 8, 64, seed=23).to(DEV)
    tl = torch.randint(0, C, (N, S // 8, S // 8), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2).to(DEV)
    tr = (torch.randint(0, 60, (N, S, S), generator=g).to(DEV) * (tl > 0)).float()

    def with_graph():
        harness.evaluate_tiles(net_hr, model, tiles, tr, tl, batch=tb, num_class=C).result()

    @torch.no_grad()
    def eager_loop():
        acc_total = AverageMeter()
        seg2, hm2 = SegmentationMetric(C, device=DEV), HeightMetric(C, device=DEV)
        for s in range(0, N, tb):
            x = tiles[s:s + tb]
            out = model(x, harness.features_for_head(net_hr, x[:, :3], model=model))
            _, rmse = replaced_scoring(seg2, hm2, out[0], out[1], tr[s:s + tb], tl[s:s + tb])
            acc_total.update(rmse.item(), x.size(0))
        seg2.check_range()

    w, e = alternate([with_graph, eager_loop], args.runs, wall_ms, warmup=2)
    rows += ["2. a validation pass over %d tiles in batches of %d (RRDBNet with %d blocks + efficientnet-b4 height model), host clock, per TILE" % (N, tb, args.blocks),
             "   harness.evaluate_tiles(...).result()                      %s" % fmt(tuple(v / N for v in w)),
             "   eager loop: forward + replaced scoring + rmse.item() per batch  %s" % fmt(tuple(v / N for v in e)),
             "   ratio eager / evaluate_tiles (medians) %.2f" % (e[0] / w[0])]
    for row in rows[-4:]:
        print(row, flush=True)
    prop = torch.cuda.get_device_properties(0)
    head = ["Height-stage evaluation; device %s (%s, %d CUs, %.0f GB) on host %s; torch %s, HIP %s"
            % (prop.name, getattr(prop, "gcnArchName", "?"), prop.multi_processor_count, prop.total_memory / 2 ** 30, socket.gethostname(),
               torch.__version__, torch.version.hip),
            "one process; the two sides of each comparison timed alternately; median (min, max) of %d runs after warm-up" % args.runs, ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(head + rows) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
