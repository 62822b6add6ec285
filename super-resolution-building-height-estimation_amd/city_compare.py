"""How good a predicted city is against a reference height raster on the same grid: exact integer sums on the device, the error
measures from them on the host.

The reference validates loose float tiles (``vtest_epoch2``: ``HeightMetric`` per height class, ``SegmentationMetric`` of the class map;
here ``evaluate.evaluate_tiles`` / ``HeightEvaluation``) and, for rasters, one file at a time through cv2 (``cal_rmse``,
demo_preprocess_height_v2.py:1389-1406: a height product against the label, RMSE over the pixels where they differ) or one shapefile
feature and one GDAL window read at a time (the ``compare_twotiff_valid*`` family).  Here, over ``harness.predict_city``'s ``(height
uint16, class uint8)`` and a reference height raster on the same grid:

* ``pair_sums``        per window ``[count, n, sd, sad, sdd, sp, sr, spp, srr, spr]`` for thousands of windows in ONE libsrbh launch;
* ``errors_from_sums`` / ``cell_errors``  the per-cell agreement table (n, count, fraction, me, mae, rmse, means, Pearson r, r2) from those
  integers, on the host, each a correctly rounded quotient of exact integers;
* ``class_sums``       per height class of the reference ``[n, sd, sad, sdd]`` and the confusion matrix of the classes, whole raster;
* ``city_validation``  the city-scale ``vtest_epoch2``: a filled ``metrics.HeightMetric`` and ``metrics.SegmentationMetric``;
* ``block_errors``     the agreement at an aggregated scale (block 40 = 100 m, 400 = 1 km), from two ``city_summary.block_sums`` calls.

``p`` is the predicted raster, ``r`` the reference, ``d = p - r``.  A pixel is COMPARED when it lies inside the raster (and the window),
the pair test of ``mode`` holds -- with ``P := p > pred_threshold`` and ``R := r > ref_threshold``: ``"any"`` P or R, ``"both"`` P and R,
``"ref"`` R, ``"pred"`` P -- and (no mask or ``mask > mask_threshold``).  Thresholds lie in -1..65535; -1 makes a test always true.  The
kernels (csrc/srbh_compare.hip) work in integers only, so every sum is exact and bit-equal between runs.  Everything stays in RASTER
UNITS: predict_city's height is ``round(10 h)``, the caller brings the reference to the same units, nothing here divides by ten.

GPU only.  The same sums per polygon zone (a per-urban-centre RMSE) are ``city_zone_compare``'s.  Rasters of another resolution and
warping, int16 and float rasters, GeoTIFFs and shapefiles are out of scope."""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from .city_grid import _check_rasters, _check_windows, _on_device, _workspace
from .city_summary import _SUM_TYPES, _int_rows, block_sums

__all__ = ["pair_sums", "errors_from_sums", "cell_errors", "class_sums", "city_validation", "block_errors", "MODES", "DEFAULT_EDGES"]

MODES = {"any": 0, "both": 1, "ref": 2, "pred": 3}                       # include/srbh.h SRBH_PAIR_*
DEFAULT_EDGES = (0, 30, 120, 210, 300, 600, 900)                          # ten times the reference's hir (train.py:55), raster units
MAX_CLASSES = 16
_TILE = 256                                                               # city_validation's whole-raster row: one window per 256 x 256 tile
_WHAT = "uint16 or uint8 (int16 and float rasters are out of scope)"


# ---- argument handling --------------------------------------------------------------------------------------------------------------------
# city_summary's argument path: everything that can be judged without a device is judged first (and is testable without one); the device is
# asked for last.
def _rasters(fn, pred, ref, mask, mode, pred_threshold, ref_threshold, mask_threshold):
    """the checks that need no device: shapes, types, strides, the mode's name, thresholds -> (H, W, mode, pthr, rthr, mthr)"""
    if ref is None:
        raise ValueError(f"{fn}: ref must be an (H, W) tensor (got None)")
    H, W = _check_rasters(fn, ("pred", "ref"), pred, ref, _SUM_TYPES, _WHAT)
    if mask is not None:
        _check_rasters(fn, ("pred", "mask"), pred, mask, _SUM_TYPES, _WHAT)
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError(f"{fn}: mode={mode!r} is none of {tuple(MODES)}")
    thr = [int(pred_threshold), int(ref_threshold), int(mask_threshold)]
    if not all(-1 <= t <= 65535 for t in thr):
        raise ValueError(f"{fn}: a threshold {tuple(thr)} outside -1..65535")
    return (H, W, MODES[mode], *thr)


def _device_rasters(fn, pred, ref, mask):
    pred, rs_p, ref, rs_r = _on_device(fn, ("pred", "ref"), pred, ref)
    mask, rs_m = _on_device(fn, ("mask", None), mask, None)[:2]
    return pred, rs_p, ref, rs_r, mask, rs_m


def _abi(pred, rs_p, ref, rs_r, mask, rs_m, H, W):
    """the eleven leading arguments of both entries of csrc/srbh_compare.hip"""
    return (pred.data_ptr(), _SUM_TYPES[pred.dtype], rs_p, ref.data_ptr(), _SUM_TYPES[ref.dtype], rs_r,
            None if mask is None else mask.data_ptr(), 0 if mask is None else _SUM_TYPES[mask.dtype], rs_m, H, W)


def _edges(fn, edges):
    try:
        e = [v for v in edges]
    except TypeError:
        raise ValueError(f"{fn}: edges={edges!r} must be a sequence of integers") from None
    if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in e):
        raise ValueError(f"{fn}: edges={edges!r} must be integers")
    e = [int(v) for v in e]
    if not 2 <= len(e) <= MAX_CLASSES:
        raise ValueError(f"{fn}: {len(e)} edges; the number of classes C must lie in 2..{MAX_CLASSES}")
    if e[0] != 0:
        raise ValueError(f"{fn}: edges[0]={e[0]} must be 0")
    if any(b <= a for a, b in zip(e, e[1:])) or e[-1] > 2 ** 31 - 2:
        raise ValueError(f"{fn}: edges={e} must be strictly ascending int32 values")
    return e


# ---- the kernels ----------------------------------------------------------------------------------------------------------------------------
def pair_sums(pred, ref, pos, mask=None, mode="any", pred_threshold=0, ref_threshold=0, mask_threshold=0):
    """-> device (N, 10) int64 ``[count, n, sd, sad, sdd, sp, sr, spp, srr, spr]`` per window, one srbh_pair_sums launch on the current
    stream.  ``pred`` / ``ref`` / ``mask``: (H, W) device tensors of uint16 or uint8, read in place (stride 1 along W, any row stride).
    ``pos``: host (N, 4) windows (xoff, yoff, xcount, ycount), validated to lie inside the raster and uploaded; a device int32 (N, 4)
    tensor is used as is (the kernel sums only what lies inside the raster).  ``count`` = the window's pixels inside the raster, ``n`` =
    the compared ones; over those ``sd`` = sum of d = pred - ref, ``sad`` of |d|, ``sdd`` of d^2, ``sp`` / ``sr`` of pred / ref, ``spp``
    / ``srr`` / ``spr`` of pred^2, ref^2 and pred ref -- raster units, exact."""
    H, W, mode, pthr, rthr, mthr = _rasters("pair_sums", pred, ref, mask, mode, pred_threshold, ref_threshold, mask_threshold)
    pos = _check_windows("pair_sums", pos, W, H, pred.device)
    pred, rs_p, ref, rs_r, mask, rs_m = _device_rasters("pair_sums", pred, ref, mask)
    pos_dev, n = pos.to(pred.device).contiguous(), pos.shape[0]
    out = torch.empty((n, 10), dtype=torch.int64, device=pred.device)
    with torch.cuda.device(pred.device):
        _lib.check(_lib.lib().srbh_pair_sums(*_abi(pred, rs_p, ref, rs_r, mask, rs_m, H, W), pos_dev.data_ptr(), n, mode, pthr, rthr, mthr,
                                             out.data_ptr(), _lib.stream_ptr()), "srbh_pair_sums")
    return out


def class_sums(pred, ref, edges, build=None, mode="any", pred_threshold=-1, ref_threshold=-1, mask_threshold=-1, workspace=None):
    """-> (device (C, 4 + C) int64, device 0-dim int64 ``bad``): per class c of the REFERENCE ``[n, sd, sad, sdd, cm[c][0..C-1]]`` over the
    compared pixels of the whole raster (the defaults compare every pixel).  ``edges``: C ascending integers, edges[0] == 0, 2 <= C <= 16;
    the class of a value is the number of k >= 1 with value >= edges[k].  The predicted class is the value of ``build`` when it is given
    (it also masks under ``mask_threshold``; the default -1 switches that off), else the class of ``pred``; a compared pixel with
    build >= C enters the four sums, no column of cm, and ``bad``.  ``workspace``: optional device buffer of at least
    srbh_pair_class_ws_bytes bytes to reuse between calls (its content does not matter)."""
    H, W, mode, pthr, rthr, mthr = _rasters("class_sums", pred, ref, build, mode, pred_threshold, ref_threshold, mask_threshold)
    e = _edges("class_sums", edges)
    C = len(e)
    _workspace("class_sums", workspace)
    pred, rs_p, ref, rs_r, build, rs_m = _device_rasters("class_sums", pred, ref, build)
    workspace = _workspace("class_sums", workspace, _lib.lib().srbh_pair_class_ws_bytes(H, W, C), pred.device)
    out = torch.empty(C * (4 + C) + 1, dtype=torch.int64, device=pred.device)
    with torch.cuda.device(pred.device):
        _lib.check(_lib.lib().srbh_pair_class_sums(*_abi(pred, rs_p, ref, rs_r, build, rs_m, H, W), (ctypes.c_int * C)(*e), C, mode, pthr,
                                                   rthr, mthr, out.data_ptr(), workspace.data_ptr(), _lib.stream_ptr()),
                   "srbh_pair_class_sums")
    return out[:-1].view(C, 4 + C), out[-1]


# ---- the error measures from the integers ------------------------------------------------------------------------------------------------
def _errors(count, n, sd, sad, sdd, sp, sr, spp, srr, spr):
    """one row in Python integers -> (fraction, me, mae, rmse, mean_pred, mean_ref, r, r2).  int / int is correctly rounded, so every
    quotient is rounded once; the variances and the covariance are formed exactly (n spp - sp^2: no cancellation, however close the
    values lie) before the one conversion."""
    nan = math.nan
    fraction = n / count if count else nan
    if n == 0:
        return (fraction,) + (nan,) * 7
    vp, vr, cov = n * spp - sp * sp, n * srr - sr * sr, n * spr - sp * sr
    r = cov / math.sqrt(vp * vr) if vp and vr else nan
    r2 = (vr - n * sdd) / vr if vr else nan                             # 1 - n sdd / vr as ONE quotient
    return fraction, sd / n, sad / n, math.sqrt(sdd / n), sp / n, sr / n, r, r2


_FLOATS = ("fraction", "me", "mae", "rmse", "mean_pred", "mean_ref", "r", "r2")


def errors_from_sums(sums):
    """(N, 10) integers ``[count, n, sd, sad, sdd, sp, sr, spp, srr, spr]`` (pair_sums' rows, on the host) -> dict of numpy arrays, one
    entry per window: ``n``, ``count`` int64; float64 in raster units ``fraction = n / count``, ``me = sd / n``, ``mae = sad / n``,
    ``rmse = sqrt(sdd / n)``, ``mean_pred``, ``mean_ref``, Pearson ``r = (n spr - sp sr) / sqrt((n spp - sp^2)(n srr - sr^2))`` and
    ``r2 = 1 - n sdd / (n srr - sr^2)`` (the coefficient of determination of pred as a predictor of ref).  NaN where n == 0 (count == 0
    for fraction) or the variance in a denominator is 0."""
    rows = _int_rows("errors_from_sums", sums, ("count", "n", "sd", "sad", "sdd", "sp", "sr", "spp", "srr", "spr"))
    out = {"n": np.array([r[1] for r in rows], dtype=np.int64), "count": np.array([r[0] for r in rows], dtype=np.int64)}
    vals = [_errors(*r) for r in rows]
    for k, name in enumerate(_FLOATS):
        out[name] = np.array([v[k] for v in vals], dtype=np.float64)
    return out


def cell_errors(height, ref, pos, build=None, **kw):
    """The per-cell agreement table of a fishnet (city_grid.fishgrid_windows) over a predicted city and a reference height raster:
    errors_from_sums of pair_sums(height, ref, pos, build, **kw) -- by default the pixels where either height is > 0 and, with ``build``,
    class > 0.  One launch and one device-to-host copy of N x 10 int64.  Raster units."""
    return errors_from_sums(pair_sums(height, ref, pos, build, **kw).cpu().numpy())


def fill_metrics(class_rows, bad, device):
    """(C, 4 + C) Python / numpy integers (class_sums' rows on the host) -> (metrics.HeightMetric, metrics.SegmentationMetric) filled as
    HeightEvaluation.result() fills them, the raster as one batch: per class stats = [sqrt(sdd / n) n (0 for a class without pixels),
    sad, sd], count = n; confusionMatrix[reference class, predicted class]"""
    from .metrics import HeightMetric, SegmentationMetric
    rows = [[int(v) for v in r] for r in np.asarray(class_rows).tolist()]
    C = len(rows)
    hm, seg = HeightMetric(C, device=device), SegmentationMetric(C, device=device)
    stats = [[math.sqrt(sdd / n) * n if n else 0.0, float(sad), float(sd)] for n, sd, sad, sdd, *_ in rows]
    hm.stats += torch.tensor(stats, dtype=torch.float64).to(device)
    hm.count += torch.tensor([[float(r[0])] for r in rows], dtype=torch.float64).to(device)
    seg.confusionMatrix += torch.tensor([r[4:] for r in rows], dtype=torch.float64).to(device)
    if bad:
        seg._bad |= torch.ones((), dtype=torch.int64, device=device)
    return hm, seg


def city_validation(height, ref_height, build=None, edges=DEFAULT_EDGES):
    """The city-scale vtest_epoch2: every pixel of the predicted ``height`` against ``ref_height`` (both in raster units), by the height
    classes ``edges`` of the reference.  -> dict: ``"height"`` a filled metrics.HeightMetric (per class sqrt(sdd / n) n, sad, sd and the
    count n: getAvgEach() gives rmse / mae / me per class); ``"seg"`` a filled metrics.SegmentationMetric, confusion matrix [reference
    class, predicted class], the predicted class being ``build``'s value when it is given, else the class of ``height``; ``"sums"`` the
    whole raster's errors_from_sums row (every pixel compared); ``"bad"`` the number of pixels with build >= C (seg.check_range() raises
    when it is not 0).  Two kernels and a fold; the device results are read back once."""
    rows, bad = class_sums(height, ref_height, edges, build)
    H, W = height.shape
    # the whole raster's row: a window is ONE workgroup, so the raster is cut into tiles (device windows, clipped by the kernel) and the
    # tiles' rows are added in int64 on the device
    ys, xs = torch.meshgrid(torch.arange(0, H, _TILE, dtype=torch.int32, device=rows.device),
                            torch.arange(0, W, _TILE, dtype=torch.int32, device=rows.device), indexing="ij")
    tiles = torch.stack([xs, ys, torch.full_like(xs, _TILE), torch.full_like(xs, _TILE)], -1).reshape(-1, 4)
    whole = pair_sums(height, ref_height, tiles, None, "any", -1, -1).sum(0)
    C = rows.shape[0]
    flat = torch.cat([rows.reshape(-1), bad.reshape(1), whole.reshape(-1)]).cpu().numpy()
    class_rows, nbad = flat[:C * (4 + C)].reshape(C, 4 + C), int(flat[C * (4 + C)])
    hm, seg = fill_metrics(class_rows, nbad, height.device)
    return {"height": hm, "seg": seg, "sums": errors_from_sums(flat[C * (4 + C) + 1:].reshape(1, 10)), "bad": nbad}


def block_errors(pred, ref, block, mask=None):
    """The agreement at an aggregated scale: the rasters cut into block x block cells (city_summary.block_sums, two calls with
    value_threshold=-1: every pixel, or those with mask > 0), D_b = sum_pred,b - sum_ref,b in exact int64 on the device, over the blocks
    where either sum is non-zero.  The block means are mp_b = sum_pred,b / n_b, mr_b = sum_ref,b / n_b and e_b = D_b / n_b (n_b = the
    block's summed pixels), each one float64 division of exactly converted integers.  -> dict of device tensors: ``n_blocks`` int64;
    float64 ``me`` = mean e_b, ``mae`` = mean |e_b|, ``rmse`` = sqrt(mean e_b^2), Pearson ``r`` of (mp_b, mr_b) from the raw moments, and
    ``sums`` = [sum e, sum |e|, sum e^2, sum mp, sum mr, sum mp^2, sum mr^2, sum mp mr].  NaN without blocks.  Python only."""
    a, b = block_sums(pred, block, mask, value_threshold=-1), block_sums(ref, block, mask, value_threshold=-1)
    sp, sr, n = a[1].reshape(-1), b[1].reshape(-1), a[0].reshape(-1)
    d = sp - sr                                                       # exact int64
    use = (sp != 0) | (sr != 0)                                        # (n_b > 0 there)
    nb = n.double().clamp_min(1.0)                                     # (sums < 2^47, n < 2^31: exact in float64)
    zero = torch.zeros((), dtype=torch.float64, device=d.device)
    e, mp, mr = (torch.where(use, t.double() / nb, zero) for t in (d, sp, sr))
    s = torch.stack([e.sum(), e.abs().sum(), (e * e).sum(), mp.sum(), mr.sum(), (mp * mp).sum(), (mr * mr).sum(), (mp * mr).sum()])
    k = use.sum()
    kd = k.double()
    var = (kd * s[5] - s[3] * s[3]) * (kd * s[6] - s[4] * s[4])
    return {"n_blocks": k, "me": s[0] / kd, "mae": s[1] / kd, "rmse": torch.sqrt(s[2] / kd), "r": (kd * s[7] - s[3] * s[4]) / torch.sqrt(var),
            "sums": s}
