#!/usr/bin/env python
"""Time srgan.PerceptualLoss forward + input gradient: the stock path (MIOpen fp32 convolutions) against libsrbh = "f16" (srbh_wconv3x3 +
csrc/srbh_vgg.hip), seeded VGG19 weights, cuts [2, 7, 16, 25, 34], L1.

    python tools/time_perceptual.py [--out profiles/perceptual_bench.txt] [--rounds 5] [--runs 5] [--batch 8] [--size 256]
    python tools/time_perceptual.py --only mode --runs 3 --out ""      # one path only: the program to put behind `rocprofv3 --kernel-trace --stats --`
    python tools/time_perceptual.py --trainer [--out profiles/perceptual_trainer_bench.txt]      # one whole RealESRGAN iteration with the term on

Both paths are warmed up first (MIOpen's first-use search, the mode's packs and plane buffers are outside every window), then alternated in one
process --rounds times (at least 5); a round times --runs calls of each path with HIP events.  Reported: the median of the rounds' medians and
the range over all calls.  The per-layer table lists the FLOPs of each conv by shape, 2 * 9 * Cin * Cout * H * W * B, three passes each (output,
target, data gradient; the first conv has no data gradient worth counting: 3 channels): divide by the kernel times of a rocprofv3 run."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from srbh_amd import srgan  # noqa: E402


def seeded_state_dict():
    torch.manual_seed(1905)
    f = srgan.vgg19_features()
    with torch.no_grad():
        for p_ in f.parameters():
            p_.mul_(3.0)
    return {"features." + k: v.clone() for k, v in f.state_dict().items()}


def one_call(pl, x, gt):
    x.grad = None
    pl(x, gt).backward()


def timed(fn, runs):
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def trainer(args):
    """RealESRGAN.optimize_parameters (23 blocks, `mixed`, batch x 3 x 64 x 64 -> 256 x 256) with the perceptual term on, free running (one
    synchronisation per --runs iterations), stock VGG stack against SRBH_SR_VGG=libsrbh, alternated in one process after a warm-up of both"""
    import time
    from srbh_amd import rrdbnet_autograd as RA
    from srbh_amd.rrdbnet import RealESRGAN
    dev = "cuda:0"
    RA.set_train_precision("mixed")
    torch.manual_seed(3)
    m = RealESRGAN(3, 3, num_block=23, device=dev, is_train=True, vgg19_weights=seeded_state_dict())
    g = torch.Generator().manual_seed(9)
    gt = torch.nn.functional.interpolate(torch.rand((args.batch, 3, args.size // 8, args.size // 8), generator=g), scale_factor=8, mode="bilinear").to(dev)
    lq = torch.nn.functional.avg_pool2d(gt, 4)

    def run(path, n):
        if path == "mode":
            os.environ["SRBH_SR_VGG"] = "libsrbh"
        else:
            os.environ.pop("SRBH_SR_VGG", None)
            m.cri_perceptual.libsrbh = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            m.feed_data({"lq": lq, "gt": gt})
            m.optimize_parameters()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    for path in ("stock", "mode"):
        run(path, 3)
    per = {"stock": [], "mode": []}
    for _ in range(args.rounds):
        for path in per:
            per[path].append(run(path, args.runs))
    rows = ["RealESRGAN.optimize_parameters with l_g_percep, 23 blocks, mixed, batch %d, %dx%d output; device %s" % (args.batch, args.size, args.size, torch.cuda.get_device_name(0)),
            "wall time per iteration, free running; %d rounds alternating the paths, %d iterations per round, after 3 warm-up iterations of each" % (args.rounds, args.runs), ""]
    for k, v in per.items():
        rows.append("%-6s median %9.3f ms   rounds %s" % (k, statistics.median(v), " ".join("%.3f" % t for t in v)))
    rows.append("mode - stock = %+.3f ms" % (statistics.median(per["mode"]) - statistics.median(per["stock"])))
    print("\n".join(rows), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(rows) + "\n")
        print("wrote", args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "perceptual_bench.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--only", choices=["stock", "mode"], default=None)
    ap.add_argument("--trainer", action="store_true")
    args = ap.parse_args()
    if args.trainer:
        if args.out == os.path.join(ROOT, "profiles", "perceptual_bench.txt"):
            args.out = os.path.join(ROOT, "profiles", "perceptual_trainer_bench.txt")
        return trainer(args)
    assert args.only or args.rounds >= 5, "the two paths are alternated at least five times"
    dev = "cuda:0"
    g = torch.Generator()
    g.manual_seed(16)
    shape = (args.batch, 3, args.size, args.size)
    x = torch.rand(*shape, generator=g).to(dev).requires_grad_(True)
    gt = torch.rand(*shape, generator=g).to(dev)
    sd = seeded_state_dict()
    paths = {}
    if args.only != "mode":
        paths["stock"] = srgan.PerceptualLoss(state_dict=sd).to(dev)
    if args.only != "stock":
        paths["mode"] = srgan.PerceptualLoss(state_dict=sd).to(dev)
        paths["mode"].libsrbh = "f16"
    for pl in paths.values():                       # warm-up of BOTH before any window
        for _ in range(3):
            one_call(pl, x, gt)
    torch.cuda.synchronize()
    per = {k: [] for k in paths}
    for _ in range(args.rounds):
        for k, pl in paths.items():
            per[k].append(timed(lambda: one_call(pl, x, gt), args.runs))
    rows = ["PerceptualLoss forward + input gradient, %s, cuts [2, 7, 16, 25, 34], L1; device %s" % (shape, torch.cuda.get_device_name(0)),
            "HIP-event time of one call; %d rounds alternating the paths, %d calls per round, after 3 warm-up calls of each" % (args.rounds, args.runs), ""]
    med = {}
    for k, rounds in per.items():
        meds = [statistics.median(r) for r in rounds]
        flat = [t for r in rounds for t in r]
        med[k] = statistics.median(meds)
        rows.append("%-6s median of round medians %9.3f ms   round medians %s   all calls %.3f .. %.3f ms"
                    % (k, med[k], " ".join("%.3f" % m for m in meds), min(flat), max(flat)))
    if len(med) == 2:
        rows.append("mode / stock = %.3f" % (med["mode"] / med["stock"]))
    rows += ["", "conv FLOPs by shape (2 * 9 * Cin * Cout * H * W * B), one pass:"]
    plan, _, _ = srgan._vgg_plan(paths.get("mode") or paths["stock"])
    h = w = args.size
    total = 0.0
    for conv, cut, pool, idx in plan:
        fl = 2.0 * 9 * conv.in_channels * conv.out_channels * h * w * args.batch
        total += fl
        rows.append("  conv %2d  %3d -> %3d  %3dx%-3d  %8.3f GFLOP" % (idx, conv.in_channels, conv.out_channels, h, w, fl / 1e9))
        if pool:
            h, w = h // 2, w // 2
    rows.append("  one pass %.1f GFLOP, a call (output, target, data gradient) ~%.1f GFLOP" % (total / 1e9, 3 * total / 1e9))
    for k in med:
        rows.append("  %-6s %.1f TFLOP/s over the whole call" % (k, 3 * total / 1e12 / (med[k] / 1e3)))
    print("\n".join(rows), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(rows) + "\n")
        print("wrote", args.out)


if __name__ == "__main__":
    main()
