"""float64 stock-op restatement of the reference's SR metrics  --  TEST INFRASTRUCTURE ONLY.

``calculate_psnr_pt`` / ``calculate_ssim_pt`` / ``calculate_cpsnr_pt`` of reference SR/psnr_ssim.py (:203-232, :283-318 + :352-382,
:443-490) written out with plain torch ops, for the shapes tests/golden/g16_sr_metrics.npz does not carry (the fixture itself holds the
imported reference's outputs; tests/test_sr_metrics_cpu.py pins this file against it).  Runs wherever its inputs live: the tests use it on
the CPU, tools/time_sr_metrics.py on the device as the stock-op path a user had before sr_metrics.py.

``y_order`` chooses how the three-term fp32 luma sum of rgb2ycbcr_pt (:135-137) is evaluated: "matmul" is the reference's own expression
(torch.matmul: the order of the three terms is the BLAS's business), "ltr" adds r, g, b terms left to right with separate fp32
multiplies and adds (what csrc/srbh_sr_metrics.hip does), "rtl" right to left (the other order, for the sensitivity measurement)."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

MAX_OFFSET = 8
Y_WEIGHTS = (65.481, 128.553, 24.966)


def gaussian_window(ksize=11, sigma=1.5):
    """cv2.getGaussianKernel(ksize, sigma) for sigma > 0: normalised exp(-(i - (ksize-1)/2)^2 / (2 sigma^2)), float64 (ksize,)"""
    g = [math.exp(-((i - (ksize - 1) / 2.0) ** 2) / (2.0 * sigma * sigma)) for i in range(ksize)]
    s = sum(g)
    return torch.tensor([v / s for v in g], dtype=torch.float64)


def y_channel(img, y_order="matmul"):
    """rgb2ycbcr_pt(img, y_only=True) (:135-143): fp32 in, fp32 (n, 1, h, w) out"""
    img = img.float()
    if y_order == "matmul":
        weight = torch.tensor([[Y_WEIGHTS[0]], [Y_WEIGHTS[1]], [Y_WEIGHTS[2]]]).to(img)
        out = torch.matmul(img.permute(0, 2, 3, 1), weight).permute(0, 3, 1, 2) + 16.0
    else:
        t = [img[:, k:k + 1] * Y_WEIGHTS[k] for k in range(3)]
        out = ((t[0] + t[1]) + t[2] if y_order == "ltr" else (t[2] + t[1]) + t[0]) + 16.0
    return out / 255.


def _prepare(img, img2, crop_border, test_y_channel, y_order):
    assert img.shape == img2.shape, (img.shape, img2.shape)
    if crop_border != 0:
        img = img[:, :, crop_border:-crop_border, crop_border:-crop_border]
        img2 = img2[:, :, crop_border:-crop_border, crop_border:-crop_border]
    if test_y_channel:
        img, img2 = y_channel(img, y_order), y_channel(img2, y_order)
    return img.to(torch.float64), img2.to(torch.float64)


def mse_pt(img, img2, crop_border=0, test_y_channel=False, y_order="matmul"):
    """the per-image MSE behind calculate_psnr_pt (:231), (n,) float64"""
    a, b = _prepare(img, img2, crop_border, test_y_channel, y_order)
    return torch.mean((a - b) ** 2, dim=[1, 2, 3])


def calculate_psnr_pt(img, img2, crop_border=0, test_y_channel=False, y_order="matmul"):
    return 10. * torch.log10(1. / (mse_pt(img, img2, crop_border, test_y_channel, y_order) + 1e-8))


def calculate_ssim_pt(img, img2, crop_border=0, test_y_channel=False, y_order="matmul"):
    a, b = _prepare(img, img2, crop_border, test_y_channel, y_order)
    a, b = a * 255., b * 255.
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    g = gaussian_window()
    ch = a.size(1)
    window = torch.outer(g, g).view(1, 1, 11, 11).expand(ch, 1, 11, 11).to(a.device)

    def conv(x):
        return F.conv2d(x, window, stride=1, padding=0, groups=ch)

    mu1, mu2 = conv(a), conv(b)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = conv(a * a) - mu1_sq
    sigma2_sq = conv(b * b) - mu2_sq
    sigma12 = conv(a * b) - mu1_mu2
    cs_map = (2 * sigma12 + c2) / (sigma1_sq + sigma2_sq + c2)
    ssim_map = ((2 * mu1_mu2 + c1) / (mu1_sq + mu2_sq + c1)) * cs_map
    return ssim_map.mean([1, 2, 3])


def cpsnr_offset_mse(img, img2, crop_border=0, test_y_channel=False, y_order="matmul"):
    """the bias-corrected MSE of the WHOLE batch at each of the 81 offsets, in the reference's loop order (index ro * 9 + co): (81,) float64"""
    a, b = _prepare(img, img2, crop_border, test_y_channel, y_order)
    height, width = a.shape[-2:]
    ch_, cw_ = height - MAX_OFFSET, width - MAX_OFFSET
    out = []
    for ro in range(MAX_OFFSET + 1):
        for co in range(MAX_OFFSET + 1):
            cur1 = a[:, :, ro:, co:][:, :, 0:ch_, 0:cw_].clone()
            cur2 = b[:, :, (MAX_OFFSET - ro):, (MAX_OFFSET - co):][:, :, 0:ch_, 0:cw_].clone()
            for k in range(a.shape[1]):
                bias = torch.mean(cur1[:, k] - cur2[:, k])
                cur2[:, k] += bias
            out.append(torch.mean(torch.square(cur1 - cur2)))
    return torch.stack(out)


def calculate_cpsnr_pt(img, img2, crop_border=0, test_y_channel=False, y_order="matmul"):
    """0-dim float64: 10 log10(255^2 / best_mse), inf where best_mse == 0 (:488-490)"""
    best = cpsnr_offset_mse(img, img2, crop_border, test_y_channel, y_order).min()
    if best == 0:
        return torch.tensor(float("inf"), dtype=torch.float64)
    return 10. * torch.log10(255. * 255. / best)


FIXTURE_SEED = 16
FIXTURE_SHAPES = {"s40x48": (2, 3, 40, 48), "s11": (1, 1, 11, 11), "s67x130": (3, 3, 67, 130), "s12": (1, 3, 12, 12)}


def fixture_cases():
    """[(shape name, crop_border, test_y_channel, metrics the remaining window allows)] of tests/golden/g16_sr_metrics.npz: every shape with
    crop 0 and crop 4 where anything is left to measure, with test_y_channel where C == 3"""
    cases = []
    for name, (n, c, h, w) in FIXTURE_SHAPES.items():
        for crop in (0, 4):
            side = min(h, w) - 2 * crop
            which = [m for m, need in (("psnr", 1), ("ssim", 11), ("cpsnr", MAX_OFFSET + 1)) if side >= need]
            for y in ((False, True) if c == 3 else (False,)):
                if which:
                    cases.append((name, crop, y, tuple(which)))
    return cases


def case_key(name, crop, y, metric):
    return f"{name}_crop{crop}_y{int(y)}_{metric}"


def fixture_inputs():
    """{shape name: (sr, gt)}: the fixture's inputs, regenerated from ONE np.random.RandomState(FIXTURE_SEED) consumed in the order of
    FIXTURE_SHAPES (the legacy generator's stream is frozen across numpy versions; the fixture stores the two small pairs whole and a
    subsample of the two large ones, which tests/test_sr_metrics_cpu.py compares bit for bit)"""
    import numpy as np
    rs = np.random.RandomState(FIXTURE_SEED)
    return {name: pair(shape, rs) for name, shape in FIXTURE_SHAPES.items()}


def pair(shape, seed, noise=0.05):
    """(sr, gt) as the fixture makes them: gt = uniform noise smoothed by a 3x3 mean, sr = gt + noise * N(0, 1); fp32 NCHW.  seed: an int
    or a np.random.RandomState to draw from"""
    import numpy as np
    rs = seed if isinstance(seed, np.random.RandomState) else np.random.RandomState(seed)
    n, c, h, w = shape
    u = rs.uniform(0.0, 1.0, (n, c, h + 2, w + 2))
    gt = sum(u[:, :, i:i + h, j:j + w] for i in range(3) for j in range(3)) / 9.0
    sr = gt + noise * rs.standard_normal(gt.shape)
    return torch.from_numpy(sr.astype(np.float32)), torch.from_numpy(gt.astype(np.float32))
