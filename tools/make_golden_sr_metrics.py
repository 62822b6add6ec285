#!/usr/bin/env python
"""Generate tests/golden/g16_sr_metrics.npz from the *imported reference* SR/psnr_ssim.py.

    python tools/make_golden_sr_metrics.py --reference <checkout of the reference project>

The reference module imports cv2, clip, open_clip and lpips at its top; none of them is needed by the three tensor metrics.  clip,
open_clip and lpips are served as empty stub modules; cv2 as a stub whose only function is getGaussianKernel(ksize, sigma): the normalised
exp(-(i - (ksize-1)/2)^2 / (2 sigma^2)) column, which is OpenCV's own formula for sigma > 0 (_ssim_pth, :367, is its one caller here).

The script runs the reference's calculate_psnr_pt / calculate_ssim_pt / calculate_cpsnr_pt on the CPU over
tests/sr_metrics_oracle.fixture_cases() and stores their outputs (float64) -- data only.  The inputs come from
tests/sr_metrics_oracle.fixture_inputs() (np.random.RandomState(16): a 3x3-smoothed uniform ground truth, sr = gt + 0.05 N(0, 1): PSNR
~26 dB, SSIM ~0.85, neither formula saturates).  The two small pairs are stored whole; of the two large ones (0.7 MB as fp32, more than the
fixture may weigh) a [::5, ::5] subsample of every plane is stored, which the CPU test compares with the regenerated inputs bit for bit."""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import sr_metrics_oracle as H  # noqa: E402

SUBSAMPLE = 5
WHOLE = ("s11", "s12")


def import_reference(ref_dir):
    for name in ("clip", "open_clip", "lpips"):
        sys.modules.setdefault(name, types.ModuleType(name))
    cv2 = types.ModuleType("cv2")

    def getGaussianKernel(ksize, sigma):
        assert sigma > 0
        x = np.arange(ksize, dtype=np.float64) - (ksize - 1) / 2.0
        g = np.exp(-(x * x) / (2.0 * sigma * sigma))
        return (g / g.sum()).reshape(ksize, 1)

    cv2.getGaussianKernel = getGaussianKernel
    sys.modules["cv2"] = cv2
    sys.path.insert(0, os.path.join(ref_dir, "SR"))
    import psnr_ssim
    return psnr_ssim


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="directory of the reference project (holds SR/psnr_ssim.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g16_sr_metrics.npz"))
    args = ap.parse_args()
    R = import_reference(args.reference)
    inputs = H.fixture_inputs()
    out = {}
    for name, (sr, gt) in inputs.items():
        cut = (slice(None),) * 4 if name in WHOLE else (slice(None), slice(None), slice(None, None, SUBSAMPLE), slice(None, None, SUBSAMPLE))
        out[f"in_{name}_sr"] = sr.numpy()[cut]
        out[f"in_{name}_gt"] = gt.numpy()[cut]
    fns = {"psnr": R.calculate_psnr_pt, "ssim": R.calculate_ssim_pt, "cpsnr": R.calculate_cpsnr_pt}
    for name, crop, y, which in H.fixture_cases():
        sr, gt = inputs[name]
        for metric in which:
            v = fns[metric](sr, gt, crop_border=crop, test_y_channel=y)
            v = np.asarray(v.numpy() if torch.is_tensor(v) else v, dtype=np.float64)
            out[H.case_key(name, crop, y, metric)] = v
            print(f"  {H.case_key(name, crop, y, metric):28s} {np.array2string(v, precision=6)}")
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
