#!/usr/bin/env python
"""Generate tests/golden/g17_evaluate.npz from the *imported reference* metrics.py.

    python tools/make_golden_evaluate.py --reference <checkout of the reference project>

The reference's validation / test loops (train.py:315-344 vtest_epoch, :427-486 vtest_epoch2) need its data loader and both networks; what
they do with the networks' outputs does not.  This script imports the reference's own metrics.py (AverageMeter, SegmentationMetric,
HeightMetric; pandas is its one import beyond torch / numpy, as for g11 in tools/make_golden.py) and executes the loop body -- the lines
between the forward and the progress bar, and the issave block's two array expressions -- on the seeded synthetic head outputs of
tests/evaluate_oracle.fixture_inputs(), grouped into loader batches of 1, 3 and 4 over the 10 images.  Stored: the inputs and every recorded
result (data only).  Before writing, tests/evaluate_oracle.evaluate (float64) is pinned against the reference: confusion matrices bit-exact,
every float within 1e-5 relative (the reference subtracts and squares in fp32)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import evaluate_oracle as E  # noqa: E402

TOL = 1e-5


def import_reference(ref_dir):
    sys.modules.setdefault("pandas", __import__("pandas"))
    sys.path.insert(0, ref_dir)
    import metrics
    return metrics


def reference_loop(R, height, logits, ref, label, ref_batch, classes):
    """train.py:429-449 with the loader and the networks replaced by slices of the given outputs, plus vtest_epoch's two meters (:317-336)"""
    losses, acc, acc_total = R.AverageMeter(), R.AverageMeter(), R.AverageMeter()
    acc_seg = R.SegmentationMetric(classes, "cpu")
    acc_he = R.HeightMetric(classes, "cpu")
    with torch.no_grad():
        for s in range(0, height.shape[0], ref_batch):
            ypred, y_true, build = height[s:s + ref_batch], ref[s:s + ref_batch], label[s:s + ref_batch].long()
            build_pred = logits[s:s + ref_batch]
            n = ypred.size(0)
            loss = torch.mean((ypred - y_true) ** 2)
            losses.update(loss.item(), n)
            rmse = torch.sqrt(((ypred - y_true) ** 2).mean())
            acc.update(rmse, n)
            acc_total.update(rmse.item(), n)
            build_pred = build_pred.argmax(1)
            acc_seg.addBatch(build_pred, build)
            acc_he.addBatch(ypred, y_true, build)
    f64 = lambda v: np.asarray(v.numpy() if torch.is_tensor(v) else v, dtype=np.float64)      # noqa: E731
    return {"loss": f64(losses.avg), "rmse": f64(acc.avg), "acc_total": f64(acc_total.avg), "cm": f64(acc_seg.getConfusionMatrix()),
            "hm_stats": f64(acc_he.stats), "hm_count": f64(acc_he.getCount()), "oa": f64(acc_seg.OverallAccuracy()),
            "iou": f64(acc_seg.IntersectionOverUnion()), "mfwiou": f64(acc_seg.mFWIoU()), "hm_each": f64(acc_he.getAvgEach()),
            "hm_balance": f64(acc_he.getAvgBalance()), "hm_all": f64(acc_he.getAvgAll())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="directory of the reference project (holds metrics.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g17_evaluate.npz"))
    args = ap.parse_args()
    R = import_reference(args.reference)
    height, logits, ref, label = E.fixture_inputs()
    C = E.NUM_CLASS
    per_image = [set(np.unique(label[b].numpy()).tolist()) for b in range(label.shape[0])]
    assert any(len(s) <= C - 2 for s in per_image) and any(len(s) == 1 for s in per_image)
    assert 0.015 <= E.tie_fraction(logits) <= 0.03, E.tie_fraction(logits)
    assert float(height.min()) < 0 and int((height * 10 % 1 == 0.5).sum()) > 50
    out = {"in_height": height.numpy(), "in_logits": logits.numpy(), "in_ref": ref.numpy(), "in_label": label.numpy()}
    # the two rasters of issave=True (train.py:464-466, :476), image by image
    qh, cl = [], []
    for k in range(height.shape[0]):
        tmp = height[k].squeeze().cpu().numpy().copy()
        tmp[tmp < 0] = 0
        qh.append((np.round(tmp * 10)).astype("uint16"))
        cl.append(logits[k:k + 1].argmax(1)[0].cpu().numpy().astype("uint8"))
    out["q_height"], out["cls_map"] = np.stack(qh), np.stack(cl)
    worst = 0.0
    for rb in E.REF_BATCHES:
        got = reference_loop(R, height, logits, ref, label, rb, C)
        want = E.evaluate(height, logits, ref, label, rb, C)
        want.update(E.derived(want["cm"], want["hm_stats"], want["hm_count"]))
        assert np.array_equal(got["cm"], want["cm"].numpy()), f"ref_batch {rb}: confusion matrices differ"
        assert np.array_equal(got["hm_count"], want["hm_count"].numpy())
        for k, v in got.items():
            scale = want["hm_stats"][:, 1:2].expand(-1, 3) if k == "hm_stats" else None      # sum d cancels: relative to sum |d|
            err = E.rel_err(want[k], v, scale=scale)
            worst = max(worst, err)
            assert err <= TOL, f"ref_batch {rb}, {k}: oracle vs reference {err:.3e} > {TOL}"
            out[f"rb{rb}_{k}"] = v
        print(f"  ref_batch {rb}: loss {float(got['loss']):.6f} rmse {float(got['rmse']):.6f} OA {float(got['oa']):.4f}")
    print(f"  pinned: confusion matrices bit-exact, largest relative gap oracle (float64) vs reference (fp32) = {worst:.2e} (bound {TOL})")
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
