"""Quality metrics of the SR stage on libsrbh reductions: PSNR, SSIM and cPSNR (reference SR/psnr_ssim.py).

``calculate_psnr_pt`` (:203-232), ``calculate_ssim_pt`` (:283-318 with ``_ssim_pth`` :352-382) and ``calculate_cpsnr_pt``
(:443-490) under the reference's names and signatures, plus ``SRQuality``, an accumulator over validation batches modelled on
``metrics.HeightMetric``.  Each function is ONE read of its two images (csrc/srbh_sr_metrics.hip: tile + halo of both in LDS,
float64 behind the fp32 loads, ordered partial sums -- bit-reproducible) where the reference runs five float64 grouped 11x11
convolutions (SSIM) or 81 clone-and-reduce iterations (cPSNR).  The kernels return sums; the few scalar operations around them
(mean, log10, bias-corrected MSE, best offset) are float64 torch ops on the device, so no function synchronises with the host.

The images are read where they are: a ``channels_last`` network output, an NCHW target and the ``crop_border`` view all go to the
kernels through their strides, without a ``.contiguous()`` copy.  GPU only; non-fp32 inputs are cast with ``.float()``."""
import ctypes as C

import torch

from . import _lib

MAX_OFFSET = 8      # calculate_cpsnr_pt's max_offset (:467): offsets (ro, co) in 0..8 x 0..8
_NOFF = (MAX_OFFSET + 1) ** 2


def _views(img, img2, crop_border, test_y_channel, min_side, what):
    """the two (n, c, h, w) views the kernels read, after every check that needs no device (ValueError before any launch)"""
    if img.dim() != 4 or img2.dim() != 4:
        raise ValueError(f"{what}: images must be (n, c, h, w) tensors (got {tuple(img.shape)}, {tuple(img2.shape)})")
    if img.shape != img2.shape:
        raise ValueError(f"{what}: image shapes are different: {tuple(img.shape)}, {tuple(img2.shape)}")
    c = int(img.shape[1])
    if c not in (1, 3):
        raise ValueError(f"{what}: images must have 1 or 3 channels (got {c})")
    if test_y_channel and c != 3:
        raise ValueError(f"{what}: test_y_channel needs 3 channels (got {c})")
    crop_border = int(crop_border)
    if crop_border < 0:
        raise ValueError(f"{what}: crop_border must not be negative (got {crop_border})")
    h, w = int(img.shape[2]) - 2 * crop_border, int(img.shape[3]) - 2 * crop_border
    if img.shape[0] < 1 or h < min_side or w < min_side:
        raise ValueError(f"{what}: at least one image of {min_side}x{min_side} pixels is needed after the crop (got {img.shape[0]} of {h}x{w})")
    if not (img.is_cuda and img2.is_cuda):
        raise RuntimeError("srbh SR metrics run on the GPU only (no CPU fallback)")
    if img.device != img2.device:
        raise RuntimeError(f"{what}: images are on different devices ({img.device}, {img2.device})")
    if img.dtype != torch.float32:
        img = img.float()
    if img2.dtype != torch.float32:
        img2 = img2.float()
    if crop_border:
        img = img[:, :, crop_border:-crop_border, crop_border:-crop_border]
        img2 = img2[:, :, crop_border:-crop_border, crop_border:-crop_border]
    return img, img2


def _strides(t):
    return (C.c_long * 4)(*t.stride())


def _psnr_ssim_sums(a, b, y_only, want_sq, want_ssim):
    """(sq, ssim): per-image float64 sums (None where not asked for) and the element counts they are means over"""
    n, c, h, w = a.shape
    L = _lib.lib()
    out = torch.empty((2, n), dtype=torch.float64, device=a.device)
    ws = torch.empty(L.srbh_sr_psnr_ssim_ws_bytes(n, h, w), dtype=torch.uint8, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(L.srbh_sr_psnr_ssim_sums(a.data_ptr(), _strides(a), b.data_ptr(), _strides(b), n, c, h, w, int(y_only),
                                            out[0].data_ptr() if want_sq else None, out[1].data_ptr() if want_ssim else None,
                                            ws.data_ptr(), _lib.stream_ptr()), "srbh_sr_psnr_ssim_sums")
    return (out[0] if want_sq else None), (out[1] if want_ssim else None)


def _cpsnr_sums(a, b, y_only):
    """(sd, sqd): float64 (n, ce, 81) sums of d and d^2 per image, effective channel and offset ro * 9 + co"""
    n, c, h, w = a.shape
    ce = 1 if y_only else c
    L = _lib.lib()
    out = torch.empty((2, n, ce, _NOFF), dtype=torch.float64, device=a.device)
    ws = torch.empty(L.srbh_sr_cpsnr_ws_bytes(n, c, h, w, int(y_only)), dtype=torch.uint8, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(L.srbh_sr_cpsnr_sums(a.data_ptr(), _strides(a), b.data_ptr(), _strides(b), n, c, h, w, int(y_only),
                                        out[0].data_ptr(), out[1].data_ptr(), ws.data_ptr(), _lib.stream_ptr()), "srbh_sr_cpsnr_sums")
    return out[0], out[1]


def _psnr_from(sq, elems):
    return 10. * torch.log10(1. / (sq / elems + 1e-8))       # psnr_ssim.py:231-232


def _offset_mse(sd, sqd, count):
    """bias-corrected MSE per offset (psnr_ssim.py:479-484) from sums over a set of images: sd, sqd (..., ce, 81) summed over the set, `count`
    elements per channel.  Subtracting the channel's mean difference from d leaves sum d^2 - (sum d)^2 / count; rounding can take that
    below the 0 the reference's explicit subtraction cannot go below, hence the clamp."""
    ce = sd.shape[-2]
    return (sqd - sd * sd / count).clamp_min(0.0).sum(-2) / (ce * count)


def _cpsnr_from(best_mse):
    # psnr_ssim.py:488-490, with the `== 0 -> inf` branch taken on the device (the quotient is +inf there already; the where states it)
    return torch.where(best_mse == 0, float("inf"), 10. * torch.log10(255. * 255. / best_mse))


def calculate_psnr_pt(img, img2, crop_border=0, test_y_channel=False, **kwargs):
    """PSNR per image (psnr_ssim.py:203-232): images in [0, 1], shape (n, 3/1, h, w) -> (n,) float64, 10 log10(1 / (mse + 1e-8))."""
    a, b = _views(img, img2, crop_border, test_y_channel, 1, "calculate_psnr_pt")
    sq, _ = _psnr_ssim_sums(a, b, test_y_channel, True, False)
    n, c, h, w = a.shape
    return _psnr_from(sq, (1 if test_y_channel else c) * h * w)


def calculate_ssim_pt(img, img2, crop_border=0, test_y_channel=False, **kwargs):
    """SSIM per image (psnr_ssim.py:283-318): images in [0, 1], shape (n, 3/1, h, w) -> (n,) float64, the mean of the SSIM map over the
    channels and the (h-10) x (w-10) positions of the 11x11 Gaussian window."""
    a, b = _views(img, img2, crop_border, test_y_channel, 11, "calculate_ssim_pt")
    _, ss = _psnr_ssim_sums(a, b, test_y_channel, False, True)
    n, c, h, w = a.shape
    return ss / ((1 if test_y_channel else c) * (h - 10) * (w - 10))


def cpsnr_offset_mse(img, img2, crop_border=0, test_y_channel=False):
    """the (81,) float64 bias-corrected MSE of the batch at every offset of calculate_cpsnr_pt's search (index ro * 9 + co: img cropped
    from (ro, co), img2 from (8 - ro, 8 - co)); calculate_cpsnr_pt takes its minimum."""
    a, b = _views(img, img2, crop_border, test_y_channel, MAX_OFFSET + 1, "calculate_cpsnr_pt")
    sd, sqd = _cpsnr_sums(a, b, test_y_channel)
    n, _, h, w = a.shape
    return _offset_mse(sd.sum(0), sqd.sum(0), n * (h - MAX_OFFSET) * (w - MAX_OFFSET))


def calculate_cpsnr_pt(img, img2, crop_border=0, test_y_channel=False, **kwargs):
    """cPSNR of PROBA-V (psnr_ssim.py:443-490): PSNR maximised over 9 x 9 translations with the brightness bias of each channel removed.
    ONE value for the whole batch, as in the reference (bias and MSE are means over all n images): a 0-dim float64 tensor,
    10 log10(255^2 / best_mse).

    Quirk kept from the reference: the peak is 255^2 although the images are in [0, 1], so the value sits 48.13 dB above a PSNR of the
    same error.  Difference from the reference: where best_mse == 0 the reference returns the Python float ``inf``; here the result stays
    a device tensor holding ``inf`` (chosen with torch.where: no host synchronisation)."""
    return _cpsnr_from(cpsnr_offset_mse(img, img2, crop_border, test_y_channel).min())


class SRQuality:
    """PSNR / SSIM / cPSNR over a validation set, accumulated on the device (modelled on metrics.HeightMetric).  ``addBatch(sr, gt)`` adds
    the per-image values of a batch -- cPSNR per image is the PROBA-V definition, i.e. calculate_cpsnr_pt at n = 1 -- in two kernel calls
    (both images are read once for PSNR + SSIM and once for cPSNR); ``result()`` returns their means over the images seen."""

    def __init__(self, crop_border=0, test_y_channel=False, device="cuda"):
        self.crop_border = crop_border
        self.test_y_channel = test_y_channel
        self.device = device
        self.reset()

    def reset(self):
        self.sums = torch.zeros(3, dtype=torch.float64, device=self.device)      # psnr, ssim, cpsnr
        self.count = 0

    def batch_values(self, sr, gt):
        """(3, n) float64: psnr, ssim, cpsnr of each image of the batch"""
        a, b = _views(sr, gt, self.crop_border, self.test_y_channel, 11, "SRQuality")
        n, c, h, w = a.shape
        ce = 1 if self.test_y_channel else c
        sq, ss = _psnr_ssim_sums(a, b, self.test_y_channel, True, True)
        sd, sqd = _cpsnr_sums(a, b, self.test_y_channel)
        best = _offset_mse(sd, sqd, (h - MAX_OFFSET) * (w - MAX_OFFSET)).min(-1).values
        return torch.stack([_psnr_from(sq, ce * h * w), ss / (ce * (h - 10) * (w - 10)), _cpsnr_from(best)])

    def addBatch(self, sr, gt):
        v = self.batch_values(sr, gt)
        self.sums += v.sum(1).to(self.sums.device)
        self.count += int(v.shape[1])

    def result(self):
        """{"psnr", "ssim", "cpsnr"}: 0-dim float64 device tensors, means over the images; "count": the number of images"""
        m = self.sums / max(self.count, 1)
        return {"psnr": m[0], "ssim": m[1], "cpsnr": m[2], "count": self.count}
