"""CPU: the SR metrics' fixture, their stock-op restatement, the import shim and the argument checks of srbh_amd.sr_metrics.
No kernel is launched here (the kernels: tests/test_gpu_sr_metrics.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import sr_metrics_oracle as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "super-resolution-building-height-estimation_amd")


@pytest.fixture(scope="module")
def g16(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g16_sr_metrics.npz")))


@pytest.fixture(scope="module")
def inputs():
    return H.fixture_inputs()


def test_fixture_inputs_regenerate_bit_for_bit(g16, inputs):
    """the fixture stores the small pairs whole and every 5th row / column of the large ones: the seeded generator gives the same fp32 values"""
    for name, (sr, gt) in inputs.items():
        for tag, t in (("sr", sr), ("gt", gt)):
            want = g16[f"in_{name}_{tag}"]
            got = t.numpy() if want.shape == tuple(t.shape) else t.numpy()[:, :, ::5, ::5]
            assert want.dtype == np.float32 and np.array_equal(got, want), (name, tag)


def test_fixture_is_small_and_complete(g16, golden_dir):
    size = os.path.getsize(os.path.join(golden_dir, "g16_sr_metrics.npz"))
    assert size < os.path.getsize(os.path.join(golden_dir, "g10_losses.npz")), size
    keys = {H.case_key(name, crop, y, m) for name, crop, y, which in H.fixture_cases() for m in which}
    assert keys == {k for k in g16 if not k.startswith("in_")}
    # every shape with crop 0; crop 4 wherever something is left; Y wherever there are three channels; the one-position SSIM case
    assert {"s40x48_crop4_y1_cpsnr", "s11_crop0_y0_ssim", "s67x130_crop4_y1_ssim", "s12_crop0_y1_cpsnr", "s12_crop4_y1_psnr",
            "s11_crop4_y0_psnr"} <= keys and "s12_crop4_y0_ssim" not in keys
    assert 24.0 < float(g16["s40x48_crop0_y0_psnr"].mean()) < 28.0 and 0.7 < float(g16["s40x48_crop0_y0_ssim"].mean()) < 0.95   # neither saturates


def test_oracle_helper_equals_the_reference_fixture(g16, inputs):
    """tests/sr_metrics_oracle.py against the imported reference's outputs, 1e-9 on every entry.  Without test_y_channel only the float64
    summation order differs (observed: <= 3e-14); with it the helper computes Y with the reference's own expression (y_order="matmul")."""
    fns = {"psnr": H.calculate_psnr_pt, "ssim": H.calculate_ssim_pt, "cpsnr": H.calculate_cpsnr_pt}
    worst = 0.0
    for name, crop, y, which in H.fixture_cases():
        sr, gt = inputs[name]
        for m in which:
            got = fns[m](sr, gt, crop_border=crop, test_y_channel=y).numpy()
            want = g16[H.case_key(name, crop, y, m)]
            assert got.dtype == np.float64 and got.shape == want.shape, (name, crop, y, m)
            err = float(np.max(np.abs(got - want)))
            worst = max(worst, err)
            assert err <= 1e-9, (name, crop, y, m, err)
    print(f"helper vs reference fixture: worst |diff| = {worst:.2e}")


def test_y_orders_of_the_helper_are_the_same_luma_to_rounding(inputs):
    sr, _ = inputs["s40x48"]
    a, b, c = (H.y_channel(sr, o) for o in ("matmul", "ltr", "rtl"))
    assert a.shape == (2, 1, 40, 48) and a.dtype == torch.float32
    assert float((a - b).abs().max()) <= 2e-7 and float((c - b).abs().max()) <= 2e-7      # a few fp32 ulp of values in [16/255, 1)


def test_gaussian_window_is_opencvs_formula():
    g = H.gaussian_window()
    assert g.dtype == torch.float64 and abs(float(g.sum()) - 1.0) < 1e-15 and torch.equal(g, g.flip(0))
    assert abs(float(g[5] / g[4]) - float(np.exp(1.0 / 4.5))) < 1e-14          # exp(-0) / exp(-1 / (2 * 1.5^2))


def test_dropin_import_path_resolves_to_sr_metrics(tmp_path):
    code = ("import sys; sys.path.insert(0, %r);"
            "from SR.psnr_ssim import calculate_psnr_pt, calculate_ssim_pt, calculate_cpsnr_pt;"
            "import srbh_amd.sr_metrics as m;"
            "assert calculate_psnr_pt is m.calculate_psnr_pt and calculate_ssim_pt is m.calculate_ssim_pt;"
            "assert calculate_cpsnr_pt is m.calculate_cpsnr_pt;"
            "assert not ({'cv2', 'clip', 'open_clip', 'lpips'} & set(sys.modules)); print('ok')") % os.path.join(PKG, "dropin")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(tmp_path))
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr


def test_cpu_tensors_raise_and_bad_arguments_raise_value_error():
    from srbh_amd import sr_metrics as M
    from srbh_amd.rrdbnet import RealESRGAN
    x = torch.rand(2, 3, 24, 24)
    fns = (M.calculate_psnr_pt, M.calculate_ssim_pt, M.calculate_cpsnr_pt)
    for fn in fns:
        with pytest.raises(RuntimeError, match="GPU only"):
            fn(x, x.clone())
        with pytest.raises(ValueError):
            fn(x, torch.rand(2, 3, 24, 25))                       # mismatched shapes
        with pytest.raises(ValueError):
            fn(torch.rand(1, 2, 24, 24), torch.rand(1, 2, 24, 24))      # C not in {1, 3}
        with pytest.raises(ValueError):
            fn(torch.rand(1, 1, 24, 24), torch.rand(1, 1, 24, 24), test_y_channel=True)
        with pytest.raises(ValueError):
            fn(x[0], x[0])                                        # not (n, c, h, w)
    with pytest.raises(ValueError):
        M.calculate_ssim_pt(x, x, crop_border=7)                  # 10x10 left: no 11x11 window
    with pytest.raises(ValueError):
        M.calculate_cpsnr_pt(x, x, crop_border=8)                 # 8x8 left: no 9x9 offsets
    with pytest.raises(ValueError):
        M.calculate_psnr_pt(x, x, crop_border=12)                 # nothing left
    with pytest.raises(RuntimeError, match="GPU only"):
        M.calculate_ssim_pt(x, x, crop_border=6)                  # 12x12 is enough: only the device is missing
    q = M.SRQuality(device="cpu")
    with pytest.raises(ValueError):
        q.addBatch(torch.rand(1, 3, 10, 10), torch.rand(1, 3, 10, 10))
    with pytest.raises(RuntimeError, match="GPU only"):
        q.addBatch(x, x)
    assert q.result()["count"] == 0
    assert callable(RealESRGAN.validate)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """the C ABI's own checks (nothing reaches a device: every call returns SRBH_ERR_ARG first) and the workspace queries"""
    from srbh_amd import _lib
    _lib.build()
    L = _lib.lib()
    ok, neg = (C.c_long * 4)(3 * 24 * 24, 24 * 24, 24, 1), (C.c_long * 4)(3 * 24 * 24, 24 * 24, -24, 1)
    p = C.c_void_p(4096)       # never dereferenced
    assert L.srbh_sr_psnr_ssim_sums(p, ok, p, ok, 1, 2, 24, 24, 0, p, p, p, None) != 0            # C = 2
    assert L.srbh_sr_psnr_ssim_sums(p, ok, p, ok, 1, 1, 24, 24, 1, p, p, p, None) != 0            # y_only with C = 1
    assert L.srbh_sr_psnr_ssim_sums(p, ok, p, neg, 1, 3, 24, 24, 0, p, p, p, None) != 0           # negative stride
    assert L.srbh_sr_psnr_ssim_sums(p, ok, p, ok, 1, 3, 10, 24, 0, p, p, p, None) != 0            # SSIM below 11 rows
    assert L.srbh_sr_psnr_ssim_sums(p, ok, p, ok, 1, 3, 24, 24, 0, None, None, p, None) != 0      # nothing asked for
    assert L.srbh_sr_psnr_ssim_sums(p, ok, p, ok, 1, 3, 24, 24, 0, p, p, None, None) != 0         # no workspace
    assert b"srbh_sr_psnr_ssim_sums" in L.srbh_last_error()
    assert L.srbh_sr_cpsnr_sums(p, ok, p, ok, 1, 3, 8, 24, 0, p, p, p, None) != 0                 # below 9 rows
    assert L.srbh_sr_cpsnr_sums(p, None, p, ok, 1, 3, 24, 24, 0, p, p, p, None) != 0              # no strides
    assert L.srbh_sr_cpsnr_sums(p, ok, p, ok, 1, 3, 24, 24, 0, p, None, p, None) != 0             # no output
    assert b"srbh_sr_cpsnr_sums" in L.srbh_last_error()
    # psnr/ssim: one [sq, ssim] pair of doubles per 16x32 tile and image; cpsnr: 81 x 2 doubles per workgroup, at most 16 per (image, channel)
    assert L.srbh_sr_psnr_ssim_ws_bytes(2, 40, 48) == 2 * (3 * 2) * 2 * 8
    assert L.srbh_sr_psnr_ssim_ws_bytes(1, 17, 33) == 1 * (2 * 2) * 2 * 8
    assert L.srbh_sr_cpsnr_ws_bytes(2, 3, 40, 48, 0) == 2 * 3 * 2 * 162 * 8       # 32 x 40 window: 1 x 2 tiles
    assert L.srbh_sr_cpsnr_ws_bytes(2, 3, 40, 48, 1) == 2 * 1 * 2 * 162 * 8
    assert L.srbh_sr_cpsnr_ws_bytes(8, 3, 256, 256, 0) == 8 * 3 * 16 * 162 * 8    # 64 tiles, capped at 16 workgroups
    assert L.srbh_sr_cpsnr_ws_bytes(1, 3, 8, 24, 0) == 0 and L.srbh_sr_psnr_ssim_ws_bytes(0, 24, 24) == 0
