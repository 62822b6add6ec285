#!/usr/bin/env python
"""Time the device-side training augmentation (loader_math.train_batch / sr_pair) against the un-augmented prep it sits beside, in ONE
process.

    python tools/time_augment.py [--out profiles/augment_bench.txt] [--rounds 5] [--calls 20]

Height stage, batch 64 (8 bands of 64 x 64, labels 256 x 256) and SR stage, batch 8 (3 bands, 64 x 64 / 256 x 256).  Three cases each:
  (a) the parent's un-augmented prep: normalize_tiles + LabelPrep (SR stage: normalize_tiles of LR and of HR);
  (b) train_batch / sr_pair with drawn parameters -- table build on the host, the pinned staging buffer and its upload included;
  (c) the two augmentation kernels alone on parameters that are already on the device, outputs allocated beforehand.
HIP events around ONE call each; every case is warmed up, then --rounds alternations (a, b, c, a, b, c, ...) of --calls calls per case.
Reported: the median of the rounds' medians and the range of the rounds' medians, plus GB/s over the bytes each side must move (inputs
read once, outputs written once; the parameter tables are counted for (b) and (c)).  Also the host time of one (b) call without a
synchronisation (what the thread that queues the training step pays) and of Augment.draw.  There is no parent path for the augmented
batch: (a) computes something else (no gather), and is here as the floor the new path has to stay near."""
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

from srbh_amd import _lib, harness  # noqa: E402
from srbh_amd import loader_math as LM  # noqa: E402

DEV = "cuda:0"
HBM_PEAK = 8.0e12


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def host_us(fn, n=50):
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e6)
    torch.cuda.synchronize()
    return statistics.median(ts)


def rounds_of(fns, rounds, calls, warmup=5):
    """per case: (median of round medians, min and max of the round medians)"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    med = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            med[i].append(statistics.median(event_ms(fn) for _ in range(calls)))
    return [(statistics.median(m), min(m), max(m)) for m in med]


def line(name, s, nbytes):
    return "   %-64s %8.4f ms (rounds %8.4f .. %8.4f)  %6.1f MB -> %6.0f GB/s" % (name, s[0], s[1], s[2], nbytes / 1e6, nbytes / (s[0] * 1e-3) / 1e9)


def nbytes_of(*tensors):
    return sum(t.numel() * t.element_size() for t in tensors)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_bench.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--sr-batch", type=int, default=8)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    L = _lib.lib()
    aug = LM.Augment()
    gen = torch.Generator().manual_seed(17)
    mins = np.linspace(-100, 50, 8)
    maxs = mins + np.linspace(1500, 2600, 8)
    rows = []

    # ---- height stage ------------------------------------------------------------------------------------------------------------
    B = args.batch
    raw = (torch.rand(B, 8, 64, 64, generator=gen) * 3000 - 200).to(DEV)
    lab = torch.randint(0, 256, (B, 256, 256), generator=gen, dtype=torch.uint8).to(DEV)
    prep = LM.LabelPrep(harness.HIR, harness.CLASS_WEIGHT, DEV)
    params = aug.draw(B, gen)
    dp = aug.to_device(params, 256, 256, DEV, (mins.astype(np.float32), (maxs - mins).astype(np.float32)))
    outs = LM.train_batch(raw, lab, mins, maxs, prep, params)
    lr, hf, ha, build, wt, wa = (torch.empty_like(t) for t in outs)
    st = _lib.stream_ptr

    def a_parent():
        LM.normalize_tiles(raw, mins, maxs, (0, 1))
        prep(lab)

    def b_train_batch():
        LM.train_batch(raw, lab, mins, maxs, prep, params)

    def c_kernels():
        L.srbh_aug_image(raw.data_ptr(), B, 8, 64, 64, 4, lr.data_ptr(), 4, dp.flip.data_ptr(), dp.perm.data_ptr(), dp.tables.data_ptr(),
                         dp.consts[0].data_ptr(), dp.consts[1].data_ptr(), 0.0, 1.0, 1, st())
        L.srbh_aug_label_prep(lab.data_ptr(), B, 256, 256, dp.flip.data_ptr(), dp.perm.data_ptr(), dp.tables.data_ptr(), prep.lut.data_ptr(),
                              prep.cw.data_ptr(), build.data_ptr(), hf.data_ptr(), wt.data_ptr(), ha.data_ptr(), wa.data_ptr(), None, st())

    data = nbytes_of(raw, lab, *outs)
    par = nbytes_of(dp.tables, dp.perm, dp.flip)
    a, b, c = rounds_of([a_parent, b_train_batch, c_kernels], args.rounds, args.calls)
    rows += ["1. height stage: batch %d, 8 bands 64 x 64 fp32, labels 256 x 256 uint8 -> the TrainStep 6-tuple" % B,
             line("(a) un-augmented prep of the parent: normalize_tiles + LabelPrep", a, data),
             line("(b) train_batch, drawn parameters (tables, staging, upload included)", b, data + par),
             line("(c) srbh_aug_image + srbh_aug_label_prep alone", c, data + par),
             "   (b) / (a) = %.2f, (c) / (a) = %.2f at the medians; the 8 TB/s HBM peak would move (c)'s bytes in %.4f ms (the batch fits the"
             % (b[0] / a[0], c[0] / a[0], (data + par) / HBM_PEAK * 1e3),
             "   256 MB last-level cache, so part of this traffic never reaches HBM)",
             "   host time of one (b) call, no synchronisation: %.0f us; of one (a) call: %.0f us; Augment.draw(%d): %.0f us; Augment.tables: %.0f us"
             % (host_us(b_train_batch), host_us(a_parent), B, host_us(lambda: aug.draw(B, gen)), host_us(lambda: aug.tables(params, 256, 256))), ""]
    for row in rows:
        print(row, flush=True)

    # ---- SR stage ----------------------------------------------------------------------------------------------------------------
    Bs = args.sr_batch
    raw_lr = (torch.rand(Bs, 3, 64, 64, generator=gen) * 3000 - 200).to(DEV)
    raw_hr = (torch.rand(Bs, 3, 256, 256, generator=gen) * 255).to(DEV)
    hmn, hmx = np.zeros(3), np.full(3, 255.0)
    sp = aug.draw(Bs, gen)
    sdp = aug.to_device(sp, 256, 256, DEV, (mins[:3].astype(np.float32), (maxs - mins)[:3].astype(np.float32), hmn.astype(np.float32),
                                           (hmx - hmn).astype(np.float32)))
    lq, gt = (torch.empty_like(t) for t in LM.sr_pair(raw_lr, raw_hr, mins[:3], maxs[:3], hmn, hmx, sp))

    def sa_parent():
        LM.normalize_tiles(raw_lr, mins[:3], maxs[:3], (0, 1))
        LM.normalize_tiles(raw_hr, hmn, hmx, None)

    def sb_pair():
        LM.sr_pair(raw_lr, raw_hr, mins[:3], maxs[:3], hmn, hmx, sp)

    def sc_kernels():
        for src, dst, up, k, clamp in ((raw_lr, lq, 4, 0, 1), (raw_hr, gt, 1, 2, 0)):
            L.srbh_aug_image(src.data_ptr(), Bs, 3, src.shape[2], src.shape[3], up, dst.data_ptr(), up, sdp.flip.data_ptr(), sdp.perm.data_ptr(),
                             sdp.tables.data_ptr(), sdp.consts[k].data_ptr(), sdp.consts[k + 1].data_ptr(), 0.0, 1.0, clamp, st())

    data = nbytes_of(raw_lr, raw_hr, lq, gt)
    par = nbytes_of(sdp.tables, sdp.perm, sdp.flip)
    a, b, c = rounds_of([sa_parent, sb_pair, sc_kernels], args.rounds, args.calls)
    rows2 = ["2. SR stage: batch %d, LR 3 x 64 x 64 and HR 3 x 256 x 256 fp32 -> (lq, gt)" % Bs,
             line("(a) un-augmented: normalize_tiles of LR and of HR", a, data),
             line("(b) sr_pair, drawn parameters (tables, staging, upload included)", b, data + par),
             line("(c) the two srbh_aug_image launches alone", c, data + par),
             "   (b) / (a) = %.2f, (c) / (a) = %.2f at the medians; host time of one (b) call, no synchronisation: %.0f us; of one (a) call: %.0f us"
             % (b[0] / a[0], c[0] / a[0], host_us(sb_pair), host_us(sa_parent))]
    for row in rows2:
        print(row, flush=True)
    prop = torch.cuda.get_device_properties(0)
    head = ["Training augmentation on the device; device %s (%s, %d CUs, %.0f GB) on host %s; torch %s, HIP %s"
            % (prop.name, getattr(prop, "gcnArchName", "?"), prop.multi_processor_count, prop.total_memory / 2 ** 30, socket.gethostname(),
               torch.__version__, torch.version.hip),
            "one process; HIP events around one call each; every case warmed up, then %d alternations of %d calls per case;" % (args.rounds, args.calls),
            "median of the rounds' medians (range of the rounds' medians); MB = bytes the side must move, GB/s = those over the median", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(head + rows + rows2) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
