"""GPU: srbh_amd.sr_metrics (csrc/srbh_sr_metrics.hip) against the reference's fixture and the float64 restatement.

Tolerances.  Without test_y_channel both sides start from the same fp32 values and do everything behind them in float64; only the order of
at most ~1e6 additions differs, and the cancellations in sigma^2 and in sum d^2 - (sum d)^2 / N are bounded by 1e-11 against C2 = 58.5 and an
MSE >= 1e-4 on these inputs: 1e-9 absolute on SSIM, 1e-9 relative on the MSE behind PSNR and cPSNR (derived, not measured).

With test_y_channel the reference's three-term fp32 luma sum goes through torch.matmul, whose order is not defined.  Measured on the CPU with
tests/sr_metrics_oracle.py, the largest change of each metric over the fixture's test_y_channel entries between the two orders of that sum
(y_order "ltr" vs "rtl"): PSNR 2.11e-7 dB, SSIM 1.66e-8, cPSNR 7.19e-7 dB.  The fixture entries with test_y_channel are allowed 50 x that.
Against the helper the kernel's own order is known (y_order="ltr": separate fp32 multiplies and adds, correctly rounded division -- the
same fp32 values), so those comparisons keep the 1e-9 bounds."""
import math

import numpy as np
import pytest
import torch

from tests import sr_metrics_oracle as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
Y_MEASURED = {"psnr": 2.11e-7, "ssim": 1.66e-8, "cpsnr": 7.19e-7}       # see the module docstring
Y_TOL = {k: 50 * v for k, v in Y_MEASURED.items()}
TOL = 1e-9


def M():
    from srbh_amd import sr_metrics
    return sr_metrics


def mse_of(metric, value):
    """the MSE behind a PSNR (10 log10(1 / (mse + 1e-8))) or cPSNR (10 log10(255^2 / mse)) value, float64 numpy"""
    v = np.asarray(value, dtype=np.float64)
    return 10.0 ** (-v / 10.0) - 1e-8 if metric == "psnr" else 255.0 ** 2 / 10.0 ** (v / 10.0)


def check(metric, got, want, y_tol=False, what=""):
    got = np.asarray(got.detach().cpu().numpy() if torch.is_tensor(got) else got, dtype=np.float64)
    want = np.asarray(want.detach().cpu().numpy() if torch.is_tensor(want) else want, dtype=np.float64)
    assert got.shape == want.shape, (what, metric, got.shape, want.shape)
    if y_tol or metric == "ssim":
        err, bound = float(np.max(np.abs(got - want))), (Y_TOL[metric] if y_tol else TOL)
    else:
        err, bound = float(np.max(np.abs(mse_of(metric, got) / mse_of(metric, want) - 1.0))), TOL
    print(f"{what} {metric}: err {err:.3e} (bound {bound:.1e})")
    assert err <= bound, (what, metric, err, bound, got, want)


def run_all(sr, gt, crop, y, which=("psnr", "ssim", "cpsnr")):
    m = M()
    fns = {"psnr": m.calculate_psnr_pt, "ssim": m.calculate_ssim_pt, "cpsnr": m.calculate_cpsnr_pt}
    out = {k: fns[k](sr, gt, crop_border=crop, test_y_channel=y) for k in which}
    for k, v in out.items():
        assert v.dtype == torch.float64 and v.is_cuda and v.shape == (() if k == "cpsnr" else (sr.shape[0],)), (k, v.shape, v.dtype)
    return out


def helper_all(sr, gt, crop, y, which=("psnr", "ssim", "cpsnr")):
    fns = {"psnr": H.calculate_psnr_pt, "ssim": H.calculate_ssim_pt, "cpsnr": H.calculate_cpsnr_pt}
    return {k: fns[k](sr, gt, crop, y, "ltr") for k in which}


def on_device(sr, gt, sr_cl=True, gt_cl=False):
    sr, gt = sr.to(DEV), gt.to(DEV)
    if sr_cl:
        sr = sr.contiguous(memory_format=torch.channels_last)
    if gt_cl:
        gt = gt.contiguous(memory_format=torch.channels_last)
    return sr, gt


@pytest.fixture(scope="module")
def g16(golden_dir):
    import os
    return dict(np.load(os.path.join(golden_dir, "g16_sr_metrics.npz")))


@pytest.fixture(scope="module")
def inputs():
    return H.fixture_inputs()


def test_every_fixture_entry_channels_last_sr_against_nchw_gt(g16, inputs):
    for name, crop, y, which in H.fixture_cases():
        sr, gt = on_device(*inputs[name])
        assert name == "s11" or not sr.is_contiguous()      # (a one-channel tensor is both layouts at once)
        got = run_all(sr, gt, crop, y, which)
        for m in which:
            check(m, got[m], g16[H.case_key(name, crop, y, m)], y_tol=y, what=f"{name} crop {crop} y {int(y)}")


# the kernels' tiles: PSNR / SSIM 16 rows x 32 columns of pixels; cPSNR 32 x 32 positions of the (H-8) x (W-8) window, at most 16 workgroups per
# (image, channel), so more than 16 tiles make a workgroup walk several
STRADDLE = [
    ((1, 1, 13, 21), 0, False),       # smaller than a tile in both dimensions
    ((3, 3, 17, 33), 0, False),       # PSNR / SSIM tile + 1 in both dimensions
    ((3, 3, 41, 41), 0, False),       # cPSNR window 33 x 33: tile + 1; not a multiple of the PSNR / SSIM tile
    ((3, 3, 41, 41), 0, True),        # the same through the luma path
    ((1, 3, 50, 75), 4, False),       # a crop view (42 x 67 left), no multiple of any tile
    ((1, 3, 50, 75), 4, True),
    ((1, 1, 140, 150), 0, False),     # cPSNR window 132 x 142: 25 tiles on 16 workgroups
    ((3, 1, 16, 32), 0, False),       # exactly one PSNR / SSIM tile
]


@pytest.mark.parametrize("shape,crop,y", STRADDLE)
def test_tile_straddling_shapes_against_the_helper(shape, crop, y):
    sr_c, gt_c = H.pair(shape, seed=sum(shape) + crop)
    sr, gt = on_device(sr_c, gt_c)
    got = run_all(sr, gt, crop, y)
    want = helper_all(sr_c, gt_c, crop, y)
    for m in got:
        check(m, got[m], want[m], what=f"{shape} crop {crop} y {int(y)}")
    # the same numbers whatever the layout of either image, bit for bit (the sums do not depend on the strides)
    sr2, gt2 = on_device(sr_c, gt_c, sr_cl=False, gt_cl=True)
    again = run_all(sr2, gt2, crop, y)
    assert all(torch.equal(got[m], again[m]) for m in got)


def test_crop_is_the_view_not_a_copy():
    """crop_border = 4 equals the uncropped call on the cropped view made contiguous, bit for bit"""
    sr, gt = on_device(*H.pair((2, 3, 44, 52), seed=5))
    a = run_all(sr, gt, 4, False)
    b = run_all(sr[:, :, 4:-4, 4:-4].contiguous(), gt[:, :, 4:-4, 4:-4].contiguous(), 0, False)
    assert all(torch.equal(a[m], b[m]) for m in a)


def test_identical_images_saturate_as_the_reference_does():
    sr, _ = on_device(*H.pair((2, 3, 40, 48), seed=2))
    got = run_all(sr, sr.clone(memory_format=torch.contiguous_format), 0, False)
    assert got["psnr"].tolist() == [80.0, 80.0]                    # the 1e-8 floor
    assert float((got["ssim"] - 1.0).abs().max()) <= 1e-12
    assert math.isinf(float(got["cpsnr"])) and float(got["cpsnr"]) > 0
    got = run_all(sr, sr.clone(), 0, True)
    assert got["psnr"].tolist() == [80.0, 80.0] and float((got["ssim"] - 1.0).abs().max()) <= 1e-12 and math.isinf(float(got["cpsnr"]))


def test_one_position_window_gives_inf_as_the_reference_does():
    """(1, 3, 9, 9): a 1x1 cPSNR window; removing the bias removes everything"""
    sr_c, gt_c = H.pair((1, 3, 9, 9), seed=9)
    assert math.isinf(float(H.calculate_cpsnr_pt(sr_c, gt_c)))
    got = M().calculate_cpsnr_pt(*on_device(sr_c, gt_c))
    assert got.is_cuda and got.dtype == torch.float64 and math.isinf(float(got)) and float(got) > 0


def test_cpsnr_finds_a_true_optimum():
    """gt shifted by (3, 5) pixels and +0.1 brighter: the search (relative shifts are even: 2 ro - 8) lands next to it, on the offset the helper
    finds, and removes the brightness.  The gain is measured like for like: against 10 log10(255^2 / mse) of the plain, unshifted pair."""
    _, canvas = H.pair((1, 3, 70, 72), seed=35)
    rs = np.random.RandomState(36)
    sr_c = canvas[:, :, 0:64, 0:64] + torch.from_numpy((0.05 * rs.standard_normal((1, 3, 64, 64))).astype(np.float32))
    gt_c = (canvas[:, :, 3:67, 5:69] + 0.1).contiguous()
    sr, gt = on_device(sr_c, gt_c)
    m = M()
    mse = m.cpsnr_offset_mse(sr, gt)
    want_mse = H.cpsnr_offset_mse(sr_c, gt_c)
    assert mse.shape == (81,) and int(mse.argmin()) == int(want_mse.argmin())
    ro, co = divmod(int(mse.argmin()), 9)
    assert abs((2 * ro - 8) - 3) == 1 and abs((2 * co - 8) - 5) == 1, (ro, co)        # gt[r, c] ~ sr[r + 3, c + 5] + 0.1
    check("cpsnr", m.calculate_cpsnr_pt(sr, gt), H.calculate_cpsnr_pt(sr_c, gt_c), what="shifted")
    assert float(np.max(np.abs(mse.cpu().numpy() / want_mse.numpy() - 1.0))) <= TOL
    plain = 10.0 * math.log10(255.0 ** 2 / float(mse_of("psnr", m.calculate_psnr_pt(sr, gt).cpu().numpy())[0]))
    gain = float(m.calculate_cpsnr_pt(sr, gt)) - plain
    print(f"cPSNR {float(m.calculate_cpsnr_pt(sr, gt)):.3f} dB, plain {plain:.3f} dB, gain {gain:.3f} dB at offset {(ro, co)}")
    assert gain > 3.0, gain


def test_bit_reproducible_and_independent_of_the_batch():
    m = M()
    sr, gt = on_device(*H.pair((3, 3, 67, 130), seed=7))
    q = m.SRQuality(device=DEV)
    a, b = run_all(sr, gt, 0, False), run_all(sr, gt, 0, False)
    assert all(torch.equal(a[k], b[k]) for k in a)
    va, vb = q.batch_values(sr, gt), q.batch_values(sr, gt)
    assert va.shape == (3, 3) and torch.equal(va, vb)
    alone = q.batch_values(sr[1:2], gt[1:2])               # image 1 sent alone (views into the same memory)
    assert torch.equal(alone[:, 0], va[:, 1])
    alone_c = q.batch_values(sr[1:2].contiguous(), gt[1:2].clone())
    assert torch.equal(alone_c[:, 0], va[:, 1])
    assert torch.equal(m.calculate_psnr_pt(sr[1:2], gt[1:2])[0], a["psnr"][1]) and torch.equal(m.calculate_ssim_pt(sr[1:2], gt[1:2])[0], a["ssim"][1])
    # SSIM alone == SSIM next to PSNR (the same kernel form); PSNR alone runs without the window pass and its halo, so its workgroups add
    # their pixels in another order: equal to rounding, not bit for bit
    assert torch.equal(va[1], a["ssim"]) and float((va[0] / a["psnr"] - 1.0).abs().max()) <= 1e-13
    assert torch.equal(m.calculate_cpsnr_pt(sr[1:2], gt[1:2]), va[2, 1])


def test_srquality_over_two_batches_is_the_mean_of_the_per_image_values():
    m = M()
    b1 = on_device(*H.pair((2, 3, 40, 48), seed=11))
    b2 = on_device(*H.pair((3, 3, 40, 48), seed=12))
    for crop, y in ((0, False), (4, True)):
        q = m.SRQuality(crop_border=crop, test_y_channel=y, device=DEV)
        vals = {"psnr": [], "ssim": [], "cpsnr": []}
        for sr, gt in (b1, b2):
            q.addBatch(sr, gt)
            vals["psnr"] += m.calculate_psnr_pt(sr, gt, crop, y).tolist()
            vals["ssim"] += m.calculate_ssim_pt(sr, gt, crop, y).tolist()
            vals["cpsnr"] += [float(m.calculate_cpsnr_pt(sr[i:i + 1], gt[i:i + 1], crop, y)) for i in range(sr.shape[0])]
        res = q.result()
        assert res["count"] == 5 and set(res) == {"psnr", "ssim", "cpsnr", "count"}
        for k, v in vals.items():
            assert res[k].is_cuda and res[k].dtype == torch.float64
            assert abs(float(res[k]) - float(np.mean(v))) <= 1e-12 * abs(float(np.mean(v))), (k, float(res[k]), np.mean(v))
        # and the per-image cPSNR is the helper's function at n = 1
        sr, gt = b1
        check("cpsnr", m.calculate_cpsnr_pt(sr[1:2], gt[1:2], crop, y), H.calculate_cpsnr_pt(sr[1:2].cpu(), gt[1:2].cpu(), crop, y, "ltr"),
              what=f"n=1 crop {crop} y {int(y)}")
    q.reset()
    assert q.result()["count"] == 0


def test_realesrgan_validate_equals_srquality_fed_with_predict():
    from srbh_amd.rrdbnet import RealESRGAN
    m = M()
    torch.manual_seed(3)
    net = RealESRGAN(3, 3, num_block=1, device=DEV, is_train=True)
    pairs = []
    for seed, n in ((21, 2), (22, 1)):
        _, gt = H.pair((n, 3, 128, 128), seed=seed)
        pairs.append((torch.nn.functional.avg_pool2d(gt, 4), gt))          # 32 x 32 inputs, CPU tensors as a loader hands them over
    got = net.validate(iter(pairs), crop_border=4, test_y_channel=False)
    q = m.SRQuality(crop_border=4, device=DEV)
    for lq, gt in pairs:
        sr = net.predict(lq)
        assert sr.shape == gt.shape
        q.addBatch(sr, gt.to(DEV))
    want = q.result()
    assert set(got) == {"psnr", "ssim", "cpsnr", "count"} and got["count"] == 3 == want["count"]
    for k in ("psnr", "ssim", "cpsnr"):
        assert isinstance(got[k], float) and math.isfinite(got[k]) and got[k] == float(want[k]), (k, got[k], float(want[k]))


def test_other_dtypes_are_cast_and_the_device_is_required():
    m = M()
    sr, gt = on_device(*H.pair((1, 3, 24, 24), seed=4))
    want = run_all(sr.half().float(), gt.double().float(), 0, False)
    got = run_all(sr.half(), gt.double(), 0, False)
    assert all(torch.equal(got[k], want[k]) for k in got)
    with pytest.raises(RuntimeError, match="GPU only"):
        m.calculate_psnr_pt(sr, gt.cpu())
