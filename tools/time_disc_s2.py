#!/usr/bin/env python
"""Time the discriminator's three 4x4 / stride 2 / pad 1 convs (SR/rrdbnet_arch.py:262-264), forward + data gradient + weight gradient: the
stock path (MIOpen fp32 convolutions) against UNetDiscriminatorSN.libsrbh_s2 = "f16" (srgan._DiscConvS2Fn, csrc/srbh_disc.hip), per conv at the
trainer's shapes (num_feat 64, 256 x 256 input: 64 -> 128 at 256x256, 128 -> 256 at 128x128, 256 -> 512 at 64x64), spectral norm included.

    python tools/time_disc_s2.py [--out profiles/disc_s2_bench.txt] [--rounds 5] [--runs 5] [--batch 8]
    python tools/time_disc_s2.py --only mode --runs 3 --out ""      # one path only: the program to put behind `rocprofv3 --kernel-trace --stats --`
    python tools/time_disc_s2.py --trainer [--out profiles/disc_s2_trainer_bench.txt]      # one whole RealESRGAN iteration, variable unset / set

Both paths are warmed up first (MIOpen's first-use search is outside every window), then alternated in one process --rounds times (at least 5);
a round times --runs calls of each path with HIP events.  Reported: the median of the rounds' medians and the range over all calls.  FLOPs of
one pass: 2 * 16 * Cin * Cout * Ho * Wo * B; a call is three passes."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from srbh_amd import srgan  # noqa: E402

DEV = "cuda:0"


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
    """RealESRGAN.optimize_parameters (23 blocks, `mixed`, batch x 3 x 64 x 64 -> 256 x 256), free running (one synchronisation per --runs
    iterations), SRBH_SR_DISC_S2 unset against libsrbh, alternated in one process after a warm-up of both"""
    import time
    from srbh_amd import rrdbnet_autograd as RA
    from srbh_amd.rrdbnet import RealESRGAN
    RA.set_train_precision("mixed")
    torch.manual_seed(3)
    m = RealESRGAN(3, 3, num_block=23, device=DEV, is_train=True)
    g = torch.Generator().manual_seed(9)
    gt = torch.nn.functional.interpolate(torch.rand((args.batch, 3, 32, 32), generator=g), scale_factor=8, mode="bilinear").to(DEV)
    lq = torch.nn.functional.avg_pool2d(gt, 4)

    def run(path, n):
        if path == "mode":
            os.environ["SRBH_SR_DISC_S2"] = "libsrbh"
        else:
            os.environ.pop("SRBH_SR_DISC_S2", None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            m.feed_data({"lq": lq, "gt": gt})
            m.optimize_parameters()
        torch.cuda.synchronize()
        assert m.net_d.libsrbh_s2 == ("f16" if path == "mode" else None)
        return (time.perf_counter() - t0) / n * 1e3

    for path in ("stock", "mode"):
        run(path, 3)
    per = {"stock": [], "mode": []}
    for _ in range(args.rounds):
        for path in per:
            per[path].append(run(path, args.runs))
    rows = ["RealESRGAN.optimize_parameters, 23 blocks, mixed, batch %d, 256x256 output; device %s" % (args.batch, torch.cuda.get_device_name(0)),
            "stock = SRBH_SR_DISC_S2 unset, mode = SRBH_SR_DISC_S2=libsrbh (conv1..conv3 of the discriminator on csrc/srbh_disc.hip)",
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
    default_out = os.path.join(ROOT, "profiles", "disc_s2_bench.txt")
    ap.add_argument("--out", default=default_out)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--only", choices=["stock", "mode"], default=None)
    ap.add_argument("--trainer", action="store_true")
    args = ap.parse_args()
    if args.trainer:
        if args.out == default_out:
            args.out = os.path.join(ROOT, "profiles", "disc_s2_trainer_bench.txt")
        return trainer(args)
    assert args.only or args.rounds >= 5, "the two paths are alternated at least five times"
    torch.manual_seed(5)
    net = srgan.UNetDiscriminatorSN(3, num_feat=64).train().to(DEV)
    g = torch.Generator()
    g.manual_seed(16)
    B = args.batch
    convs = [("conv1", net.conv1, 256), ("conv2", net.conv2, 128), ("conv3", net.conv3, 64)]
    fns = {"stock": lambda conv, t: conv(t), "mode": srgan._disc_conv4x4s2}
    if args.only:
        fns = {args.only: fns[args.only]}
    cases = []
    for name, conv, hw in convs:
        x = torch.randn(B, conv.in_channels, hw, hw, generator=g).to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        gy = torch.randn(B, conv.out_channels, hw // 2, hw // 2, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
        cases.append((name, conv, x, gy))

    def one_call(fn, conv, x, gy, wgrad):
        x.grad = None
        conv.weight_orig.grad = None
        conv.weight_orig.requires_grad_(wgrad)      # (False: the generator's GAN term through the frozen discriminator)
        fn(conv, x).backward(gy)

    for name, conv, x, gy in cases:                 # warm-up of BOTH, with and without the weight gradient, before any window
        for fn in fns.values():
            for wgrad in (True, False):
                for _ in range(3):
                    one_call(fn, conv, x, gy, wgrad)
    torch.cuda.synchronize()
    rows = ["UNetDiscriminatorSN(num_feat=64) conv1..conv3 (4x4 / stride 2 / pad 1, spectral norm), forward + data gradient + weight gradient, batch %d; device %s"
            % (B, torch.cuda.get_device_name(0)),
            "stock = conv(x) (MIOpen fp32), mode = srgan._disc_conv4x4s2 (fp16 / bf16 operands on csrc/srbh_disc.hip; staging, packs and depth-to-space included)",
            "HIP-event time of one call; %d rounds alternating the paths, %d calls per round, after 3 warm-up calls of each" % (args.rounds, args.runs), ""]
    total = {(k, wg): 0.0 for k in fns for wg in (True, False)}
    for name, conv, x, gy in cases:
        fl = 2.0 * 16 * conv.in_channels * conv.out_channels * gy.shape[2] * gy.shape[3] * B
        rows.append("%s  %3d -> %3d  %dx%d -> %dx%d   %.1f GFLOP per pass" % (name, conv.in_channels, conv.out_channels, x.shape[2], x.shape[3], gy.shape[2], gy.shape[3], fl / 1e9))
        for wgrad in (True, False):
            npass = 3 if wgrad else 2
            rows.append("  forward + data gradient%s (%d passes)" % (" + weight gradient" if wgrad else "", npass))
            per = {k: [] for k in fns}
            for _ in range(args.rounds):
                for k, fn in fns.items():
                    per[k].append(timed(lambda: one_call(fn, conv, x, gy, wgrad), args.runs))
            med = {}
            for k, rounds in per.items():
                meds = [statistics.median(r) for r in rounds]
                flat = [t for r in rounds for t in r]
                med[k] = statistics.median(meds)
                total[(k, wgrad)] += med[k]
                rows.append("    %-6s median of round medians %8.3f ms   round medians %s   all calls %.3f .. %.3f ms   %.1f TFLOP/s over the call"
                            % (k, med[k], " ".join("%.3f" % m for m in meds), min(flat), max(flat), npass * fl / 1e12 / (med[k] / 1e3)))
            if len(med) == 2:
                rows.append("    mode / stock = %.3f" % (med["mode"] / med["stock"]))
    rows += ["", "sums over the three convs; one trainer iteration runs them through three discriminator passes (the generator's GAN term: forward + data",
             "gradient; the real and the fake pass: forward + both gradients), i.e. 2 x (all three) + 1 x (forward + data gradient):"]
    for k in fns:
        a, b = total[(k, True)], total[(k, False)]
        rows.append("%-6s forward + both gradients %.3f ms, forward + data gradient %.3f ms, per trainer iteration %.3f ms" % (k, a, b, 2 * a + b))
    print("\n".join(rows), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(rows) + "\n")
        print("wrote", args.out)


if __name__ == "__main__":
    main()
