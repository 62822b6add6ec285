#!/usr/bin/env python
"""Time act(conv_k(t)) for conv4..conv8 of the discriminator (SR/rrdbnet_arch.py:265-269: 3x3 / stride 1 / pad 1, spectral norm, LeakyReLU 0.2),
forward + data gradient + weight gradient: the path the module runs with libsrbh = "f16" (srgan._DiscConvFn on the head's kernels in slices of 64
output channels + stock leaky_relu) against UNetDiscriminatorSN.libsrbh_wide = "f16" (srgan._DiscConvWideFn, csrc/srbh_disc3.hip), per conv at
the trainer's shapes (num_feat 64, 256 x 256 input: 512 -> 256 at 64x64, 256 -> 128 at 128x128, 128 -> 64 and 64 -> 64 at 256x256).  Staging,
packs, LeakyReLU and its backward are inside the window on both sides.

    python tools/time_disc_wide.py [--out profiles/disc_wide_bench.txt] [--rounds 5] [--runs 5] [--batch 8]
    python tools/time_disc_wide.py --only mode --runs 3 --out ""      # one path only: the program to put behind `rocprofv3 --kernel-trace --stats --`
    python tools/time_disc_wide.py --trainer [--out profiles/disc_wide_trainer_bench.txt]      # one whole RealESRGAN iteration, variable unset / set

Both paths are warmed up first, then alternated in one process --rounds times (at least 5); a round times --runs calls of each path with HIP
events.  Reported: the median of the rounds' medians, the round medians and the range over all calls.  The weight-gradient kernels are also timed
alone: srbh_wgrad3x3_b16 against cout / 64 calls of srbh_act16_wgrad_b16 on the same planes.  FLOPs of one pass: 2 * 9 * Cin * Cout * H * W * B."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from srbh_amd import _lib, srgan  # noqa: E402

DEV = "cuda:0"
VAR = "SRBH_SR_DISC_WIDE"


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
    iterations), SRBH_SR_DISC_WIDE unset against libsrbh, alternated in one process after a warm-up of both"""
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
            os.environ[VAR] = "libsrbh"
        else:
            os.environ.pop(VAR, None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            m.feed_data({"lq": lq, "gt": gt})
            m.optimize_parameters()
        torch.cuda.synchronize()
        assert m.net_d.libsrbh_wide == ("f16" if path == "mode" else None)
        return (time.perf_counter() - t0) / n * 1e3

    for _ in range(2):                              # (with one warm-up of each the first timed round was an outlier: 140 ms against 107 .. 111)
        for path in ("unset", "mode"):
            run(path, 3)
    per = {"unset": [], "mode": []}
    for _ in range(args.rounds):
        for path in per:
            per[path].append(run(path, args.runs))
    others = " ".join("%s=%s" % (k, os.environ[k]) for k in ("SRBH_SR_DISC", "SRBH_SR_DISC_S2", "SRBH_SR_VGG") if k in os.environ) or "none set"
    rows = ["RealESRGAN.optimize_parameters, 23 blocks, mixed, batch %d, 256x256 output; device %s" % (args.batch, torch.cuda.get_device_name(0)),
            "unset = %s unset, mode = %s=libsrbh (act(conv4..conv8) of the discriminator on csrc/srbh_disc3.hip); other SR-stage variables: %s" % (VAR, VAR, others),
            "wall time per iteration, free running; %d rounds alternating the paths, %d iterations per round, after two alternations of 3 warm-up iterations of each" % (args.rounds, args.runs), ""]
    for k, v in per.items():
        rows.append("%-6s median %9.3f ms   rounds %s" % (k, statistics.median(v), " ".join("%.3f" % t for t in v)))
    rows.append("mode - unset = %+.3f ms; the two sets of rounds %s" % (statistics.median(per["mode"]) - statistics.median(per["unset"]),
                                                                       "do not overlap" if max(per["mode"]) < min(per["unset"]) or max(per["unset"]) < min(per["mode"]) else "OVERLAP"))
    print("\n".join(rows), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(rows) + "\n")
        print("wrote", args.out)


def wgrad_alone(conv, x, gy, args):
    """srbh_wgrad3x3_b16 against cout / 64 calls of srbh_act16_wgrad_b16 on the same fp16 / bf16 planes; reduce kernels included on both sides"""
    L, sp = _lib.lib(), _lib.stream_ptr
    B, Cc, H, W = x.shape
    Oc = conv.out_channels
    X = torch.zeros(L.srbh_act16_bytes(B, Cc, H, W), dtype=torch.uint8, device=DEV)
    Gp = torch.zeros(L.srbh_act16_bytes(B, Oc, H, W), dtype=torch.uint8, device=DEV)
    xn, gn = x.detach().permute(0, 2, 3, 1).contiguous(), gy.permute(0, 2, 3, 1).contiguous()
    _lib.check(L.srbh_nhwc32_to_act16(xn.data_ptr(), X.data_ptr(), B, Cc, H, W, Cc // 32, 0, 1.0, 0, sp()), "stage x")
    _lib.check(L.srbh_nhwc32_to_act16(gn.data_ptr(), Gp.data_ptr(), B, Oc, H, W, Oc // 32, 0, 1.0, 1, sp()), "stage g")
    dw = torch.empty((Oc, Cc, 3, 3), device=DEV)
    ws = torch.empty(L.srbh_wgrad3x3_ws_bytes(Oc, Cc, B, H, W) // 4, device=DEV)
    ws16 = torch.empty(L.srbh_hwgrad_ws_bytes(min(64, Oc), Cc, 3) // 4, device=DEV)

    def new():
        _lib.check(L.srbh_wgrad3x3_b16(X.data_ptr(), Cc // 32, Cc, Gp.data_ptr(), Oc // 32, Oc, B, H, W, dw.data_ptr(), ws.data_ptr(), sp()), "wgrad3x3_b16")

    def old():
        for lo in range(0, Oc, 64):
            _lib.check(L.srbh_act16_wgrad_b16(X.data_ptr(), Cc // 32, Cc, Gp.data_ptr(), Oc // 32, lo, min(64, Oc - lo), B, H, W,
                                              dw[lo:].data_ptr(), ws16.data_ptr(), sp()), "act16_wgrad_b16")

    fns = {"act16_wgrad_b16 x %d" % ((Oc + 63) // 64): old, "wgrad3x3_b16": new}
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    per = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            per[k].append(statistics.median(timed(fn, args.runs)))
    fl = 2.0 * 9 * Cc * Oc * H * W * B
    return ["    weight gradient alone: %-22s median of round medians %8.3f ms   round medians %s   %.1f TFLOP/s"
            % (k, statistics.median(v), " ".join("%.3f" % m for m in v), fl / 1e12 / (statistics.median(v) / 1e3)) for k, v in per.items()]


def main():
    ap = argparse.ArgumentParser()
    default_out = os.path.join(ROOT, "profiles", "disc_wide_bench.txt")
    ap.add_argument("--out", default=default_out)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--only", choices=["parent", "mode"], default=None)
    ap.add_argument("--trainer", action="store_true")
    args = ap.parse_args()
    if args.trainer:
        if args.out == default_out:
            args.out = os.path.join(ROOT, "profiles", "disc_wide_trainer_bench.txt")
        return trainer(args)
    assert args.only or args.rounds >= 5, "the two paths are alternated at least five times"
    torch.manual_seed(5)
    net = srgan.UNetDiscriminatorSN(3, num_feat=64).train().to(DEV)
    g = torch.Generator()
    g.manual_seed(16)
    B = args.batch
    convs = [("conv4", net.conv4, 64), ("conv5", net.conv5, 128), ("conv6", net.conv6, 256), ("conv7", net.conv7, 256), ("conv8", net.conv8, 256)]
    parent = lambda conv, t: F.leaky_relu(srgan._disc_conv3x3(conv, t, True), 0.2)      # noqa: E731
    fns = {"parent": parent, "mode": lambda conv, t: srgan._disc_conv3x3_act(conv, t, parent)}
    if args.only:
        fns = {args.only: fns[args.only]}
    cases = []
    for name, conv, hw in convs:
        x = torch.randn(B, conv.in_channels, hw, hw, generator=g).to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        gy = torch.randn(B, conv.out_channels, hw, hw, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
        cases.append((name, conv, x, gy))

    def one_call(fn, conv, x, gy, wgrad):
        x.grad = None
        conv.weight_orig.grad = None
        conv.weight_orig.requires_grad_(wgrad)      # (False: the generator's GAN term through the frozen discriminator)
        y = fn(conv, x)
        y.backward(gy)
        return y

    for name, conv, x, gy in cases:                 # warm-up of BOTH, with and without the weight gradient, before any window
        for k, fn in fns.items():
            y = one_call(fn, conv, x, gy, True)
            assert ("DiscConvWide" in type(y.grad_fn).__name__) == (k == "mode"), (k, type(y.grad_fn).__name__)
            for wgrad in (True, False):
                for _ in range(3):
                    one_call(fn, conv, x, gy, wgrad)
    torch.cuda.synchronize()
    rows = ["UNetDiscriminatorSN(num_feat=64) act(conv4..conv8) (3x3 / stride 1 / pad 1, spectral norm, LeakyReLU 0.2), forward + data gradient + weight gradient, batch %d; device %s"
            % (B, torch.cuda.get_device_name(0)),
            "parent = leaky_relu(srgan._disc_conv3x3(f16)) (head kernels in slices of 64 output channels + stock LeakyReLU), mode = srgan._disc_conv3x3_act",
            "(fp16 / bf16 operands on csrc/srbh_disc3.hip and srbh_wconv3x3; staging, packs, LeakyReLU and its backward included on both sides)",
            "HIP-event time of one call; %d rounds alternating the paths, %d calls per round, after 3 warm-up calls of each" % (args.rounds, args.runs), ""]
    total = {(k, wg): 0.0 for k in fns for wg in (True, False)}
    rounds_sum = {(k, wg): [0.0] * args.rounds for k in fns for wg in (True, False)}
    for name, conv, x, gy in cases:
        fl = 2.0 * 9 * conv.in_channels * conv.out_channels * gy.shape[2] * gy.shape[3] * B
        rows.append("%s  %3d -> %3d  %dx%d   %.1f GFLOP per pass" % (name, conv.in_channels, conv.out_channels, x.shape[2], x.shape[3], fl / 1e9))
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
                rounds_sum[(k, wgrad)] = [a + b for a, b in zip(rounds_sum[(k, wgrad)], meds)]
                rows.append("    %-6s median of round medians %8.3f ms   round medians %s   all calls %.3f .. %.3f ms   %.1f TFLOP/s over the call"
                            % (k, med[k], " ".join("%.3f" % m for m in meds), min(flat), max(flat), npass * fl / 1e12 / (med[k] / 1e3)))
            if len(med) == 2:
                rows.append("    mode / parent = %.3f" % (med["mode"] / med["parent"]))
        if not args.only:
            rows += wgrad_alone(conv, x, gy, args)
    rows += ["", "sums over the five convs; one trainer iteration runs them through three discriminator passes (the generator's GAN term: forward + data",
             "gradient; the real and the fake pass: forward + both gradients), i.e. 2 x (all five) + 1 x (forward + data gradient):"]
    for k in fns:
        a, b = total[(k, True)], total[(k, False)]
        rows.append("%-6s forward + both gradients %.3f ms, forward + data gradient %.3f ms, per trainer iteration %.3f ms" % (k, a, b, 2 * a + b))
    if len(fns) == 2:
        for wg in (True, False):
            pm, mm = rounds_sum[("parent", wg)], rounds_sum[("mode", wg)]
            rows.append("per-round sums, forward + %s: parent %s | mode %s -> %s" % ("both gradients" if wg else "data gradient", " ".join("%.3f" % t for t in pm),
                        " ".join("%.3f" % t for t in mm), "mode lower, the two sets do not overlap" if max(mm) < min(pm) else
                        ("mode HIGHER, the two sets do not overlap" if max(pm) < min(mm) else "the two sets OVERLAP")))
    print("\n".join(rows), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(rows) + "\n")
        print("wrote", args.out)


if __name__ == "__main__":
    main()
