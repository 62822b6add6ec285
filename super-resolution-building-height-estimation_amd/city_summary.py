"""What a city's predicted rasters are turned into: per-cell and per-block height sums and the height histogram, on the device.

The reference publishes none of its 2.5 m rasters as the result but the step behind them: "the mean and std of building height in each
urban center" (datasetglobe/urbanarea_meanstd.xls, README "Testing on 301 urban centers", Figure 11) and the distribution of predicted
heights (Figure 10); its per-cell bookkeeping (``Fishgrid_stats``, ``zonal_stats``, demo_preprocess_height_v2.py:450-570, :1143-1186)
goes one shapefile feature and one GDAL window read at a time.  Here, over ``harness.predict_city``'s ``(height uint16, class uint8)``:

* ``window_sums``      per window ``[count, n, sum, sumsq, max]`` for thousands of overlapping windows in ONE libsrbh launch;
* ``block_sums``       the same sums for every non-overlapping block x block cell, the raster read once: a 10 m / 100 m / 1 km product;
* ``value_histogram``  the selected pixels counted by ``min(v // bin_width, nbins - 1)``;
* ``heights_from_sums`` / ``cell_heights``  the per-cell table (n, count, fraction, mean, std, max) from those integers, on the host;
* ``aggregate_city``   per-block rasters n, count, max, mean, fraction, density on the device;
* ``city_summary``     the whole raster's count, n, mean, std, max, histogram and class counts.

A pixel is SELECTED when it lies inside the raster, ``value > value_threshold`` and (no mask or ``mask > mask_threshold``); the defaults
select ``height > 0`` and, with a class raster, ``build > 0``.  The kernels (csrc/srbh_summary.hip) work in integers only, so every sum
is exact and bit-equal between runs.  Every result stays in RASTER UNITS: predict_city's height is ``round(10 h)``, so a mean of 87.3
is 8.73 m -- nothing here divides by ten.

GPU only.  Polygon zones and their rasterisation, GeoTIFFs, the .xls, float or int16 rasters and per-window class histograms are out of
scope."""
import math

import numpy as np
import torch

from . import _lib
from .city_grid import _check_rasters, _check_windows, _on_device, _workspace

__all__ = ["window_sums", "block_sums", "value_histogram", "heights_from_sums", "cell_heights", "aggregate_city", "city_summary"]

_SUM_TYPES = {torch.uint16: 1, torch.uint8: 3}                            # include/srbh.h SRBH_GRID_U16 / _U8
MAX_BINS = 4096


# ---- argument handling --------------------------------------------------------------------------------------------------------------------
# city_grid's argument path: everything that can be judged without a device is judged first (and is testable without one); the device is
# asked for last.
_NAMES = ("value", "mask")


def _rasters(fn, value, mask, value_threshold, mask_threshold):
    """the checks that need no device: shapes, types, strides, thresholds -> (H, W, vthr, mthr)"""
    H, W = _check_rasters(fn, _NAMES, value, mask, _SUM_TYPES, "uint16 or uint8 (int16 and float rasters are out of scope)")
    vthr, mthr = int(value_threshold), int(mask_threshold)
    if not (-1 <= vthr <= 65535 and -1 <= mthr <= 65535):
        raise ValueError(f"{fn}: a threshold ({vthr}, {mthr}) outside -1..65535")
    return H, W, vthr, mthr


def _bins(fn, bin_width, nbins):
    """a histogram's division judged -> (bin_width, nbins) as ints"""
    for name, v, hi in (("bin_width", bin_width, 65535), ("nbins", nbins, MAX_BINS)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= hi:
            raise ValueError(f"{fn}: {name}={v!r} outside 1..{hi}")
    return int(bin_width), int(nbins)


def _abi(value, rs_v, mask, rs_m, H, W):
    """the eight leading arguments every entry of csrc/srbh_summary.hip takes"""
    return (value.data_ptr(), _SUM_TYPES[value.dtype], rs_v, None if mask is None else mask.data_ptr(),
            0 if mask is None else _SUM_TYPES[mask.dtype], rs_m, H, W)


# ---- the kernels ----------------------------------------------------------------------------------------------------------------------------
def window_sums(value, pos, mask=None, value_threshold=0, mask_threshold=0):
    """-> device (N, 5) int64 ``[count, n, sum, sumsq, max]`` per window, one srbh_window_sums launch on the current stream.
    ``value`` / ``mask``: (H, W) device tensors of uint16 or uint8, read in place (stride 1 along W, any row stride).  ``pos``: host
    (N, 4) windows (xoff, yoff, xcount, ycount), validated to lie inside the raster and uploaded; a device int32 (N, 4) tensor is used
    as is (the kernel sums only what lies inside the raster).  ``count`` = the window's pixels inside the raster, ``n`` = the selected
    ones, ``sum`` / ``sumsq`` / ``max`` over the selected pixels in raster units (0 when n == 0)."""
    H, W, vthr, mthr = _rasters("window_sums", value, mask, value_threshold, mask_threshold)
    pos = _check_windows("window_sums", pos, W, H, value.device)
    value, rs_v, mask, rs_m = _on_device("window_sums", _NAMES, value, mask)
    pos_dev, n = pos.to(value.device).contiguous(), pos.shape[0]
    out = torch.empty((n, 5), dtype=torch.int64, device=value.device)
    with torch.cuda.device(value.device):
        _lib.check(_lib.lib().srbh_window_sums(*_abi(value, rs_v, mask, rs_m, H, W), pos_dev.data_ptr(), n, vthr, mthr, out.data_ptr(),
                                               _lib.stream_ptr()), "srbh_window_sums")
    return out


def block_sums(value, block, mask=None, value_threshold=0, mask_threshold=0):
    """-> device (4, Hb, Wb) int64 planes ``n, sum, sumsq, max`` of the block x block cells cut from the top-left corner (Hb = ceil(H /
    block), Wb = ceil(W / block); edge blocks hold what lies inside the raster), one srbh_block_sums launch that reads each raster once.
    Raster units."""
    H, W, vthr, mthr = _rasters("block_sums", value, mask, value_threshold, mask_threshold)
    block = _block("block_sums", block)
    value, rs_v, mask, rs_m = _on_device("block_sums", _NAMES, value, mask)
    out = torch.empty((4, -(-H // block), -(-W // block)), dtype=torch.int64, device=value.device)
    with torch.cuda.device(value.device):
        _lib.check(_lib.lib().srbh_block_sums(*_abi(value, rs_v, mask, rs_m, H, W), min(block, 2 ** 31 - 1), vthr, mthr, out.data_ptr(),
                                              _lib.stream_ptr()), "srbh_block_sums")
    return out


def _block(fn, block):
    if isinstance(block, bool) or not isinstance(block, (int, np.integer)) or block < 1:
        raise ValueError(f"{fn}: block={block!r} must be an integer >= 1")
    return int(block)


def value_histogram(value, bin_width=1, nbins=256, mask=None, value_threshold=0, mask_threshold=0, workspace=None):
    """-> device (nbins,) int64: the selected pixels counted by ``min(value // bin_width, nbins - 1)``, exact.  ``value_histogram(height,
    10, 256, build)`` is a predicted city's histogram in the 256-bin layout of bh_stats_*.txt (one bin per metre, the last bin open);
    ``value_histogram(build, 1, 7, value_threshold=-1)`` gives the class counts.  ``workspace``: optional device buffer of at least
    srbh_value_hist_ws_bytes bytes to reuse between calls (its content does not matter)."""
    H, W, vthr, mthr = _rasters("value_histogram", value, mask, value_threshold, mask_threshold)
    bin_width, nbins = _bins("value_histogram", bin_width, nbins)
    value, rs_v, mask, rs_m = _on_device("value_histogram", _NAMES, value, mask)
    workspace = _workspace("value_histogram", workspace, _lib.lib().srbh_value_hist_ws_bytes(H, W, nbins), value.device, align=4)
    hist = torch.empty(nbins, dtype=torch.int64, device=value.device)
    with torch.cuda.device(value.device):
        _lib.check(_lib.lib().srbh_value_hist(*_abi(value, rs_v, mask, rs_m, H, W), vthr, mthr, bin_width, nbins, hist.data_ptr(),
                                              workspace.data_ptr(), _lib.stream_ptr()), "srbh_value_hist")
    return hist


# ---- the paper's numbers from the integers ---------------------------------------------------------------------------------------------------
def _mean_std(n, s, q):
    """(mean, population std) of n values with sum s and sum of squares q, from Python integers: each is ONE correctly rounded division
    (int / int is correctly rounded) -- no cancellation, however close the values lie -- and one correctly rounded square root"""
    if n == 0:
        return math.nan, math.nan
    return s / n, math.sqrt((n * q - s * s) / (n * n))


def _int_rows(fn, sums, columns):
    """an (N, K) integer table on the host, K = len(columns) -> its rows as lists of Python integers, or ValueError"""
    sums = np.asarray(sums)
    if sums.ndim != 2 or sums.shape[1] != len(columns) or not np.issubdtype(sums.dtype, np.integer):
        raise ValueError(f"{fn}: needs (N, {len(columns)}) integers [{', '.join(columns)}] (got {sums.dtype} {sums.shape})")
    return [[int(v) for v in r] for r in sums.tolist()]


def heights_from_sums(sums):
    """(N, 5) integers ``[count, n, sum, sumsq, max]`` (window_sums' rows, on the host) -> dict of numpy arrays, one entry per window:
    ``n``, ``count``, ``max`` int64; ``fraction = n / count``, ``mean = sum / n`` and ``std``, the population standard deviation
    sqrt((n sumsq - sum^2) / n^2), float64 in raster units.  n == 0 gives NaN for mean and std, count == 0 for fraction."""
    rows = _int_rows("heights_from_sums", sums, ("count", "n", "sum", "sumsq", "max"))
    out = {"n": np.array([r[1] for r in rows], dtype=np.int64), "count": np.array([r[0] for r in rows], dtype=np.int64),
           "max": np.array([r[4] for r in rows], dtype=np.int64)}
    out["fraction"] = np.array([r[1] / r[0] if r[0] else math.nan for r in rows], dtype=np.float64)
    ms = [_mean_std(r[1], r[2], r[3]) for r in rows]
    out["mean"] = np.array([m for m, _ in ms], dtype=np.float64)
    out["std"] = np.array([s for _, s in ms], dtype=np.float64)
    return out


def cell_heights(height, pos, build=None):
    """The per-cell table of a fishnet (city_grid.fishgrid_windows) over a predicted city: heights_from_sums of window_sums(height, pos,
    build) -- the pixels with height > 0 and, with ``build``, class > 0.  One launch and one device-to-host copy of N x 5 int64.  Raster
    units (predict_city's height is round(10 h))."""
    return heights_from_sums(window_sums(height, pos, build).cpu().numpy())


def aggregate_city(height, block, build=None):
    """A coarser product of a predicted city: dict of device (Hb, Wb) rasters over the block x block cells (block 4: 10 m, 40: 100 m,
    400: 1 km at 2.5 m pixels).  ``n`` (selected pixels), ``count`` (the block's pixels, from geometry) and ``max`` int64; ``mean = sum /
    n`` (NaN where n == 0), ``fraction = n / count`` and ``density = sum / count`` (the mean over ALL pixels of the block) float64, each
    one division of exactly converted integers.  Raster units."""
    s = block_sums(height, block, build)
    block = int(block)
    H, W = height.shape
    ys = torch.arange(s.shape[1], dtype=torch.int64, device=s.device) * block
    xs = torch.arange(s.shape[2], dtype=torch.int64, device=s.device) * block
    count = torch.clamp(H - ys, max=block)[:, None] * torch.clamp(W - xs, max=block)[None, :]
    n, total = s[0], s[1].double()                                       # (sum < 2^47: exact in float64)
    return {"n": n, "count": count, "max": s[3], "mean": total / n.double(), "fraction": n.double() / count.double(),
            "density": total / count.double()}


def city_summary(height, build=None, bin_width=10, nbins=256, num_class=7):
    """The whole raster's numbers, as the reference reports them per urban centre: dict of ``count`` (pixels), ``n`` (selected: height
    > 0 and, with ``build``, class > 0), ``mean``, ``std`` (population), ``max`` -- Python numbers in raster units --, ``hist`` ((nbins,)
    int64 numpy: value_histogram(height, bin_width, nbins, build)) and ``class_counts`` ((num_class,) int64 numpy, the last class open;
    None without ``build``).  Block partials are added in int64 on the device; one small result is read back at the end."""
    s = block_sums(height, 256, build)
    parts = [s[:3].sum(dim=(1, 2)), s[3].max().reshape(1), value_histogram(height, bin_width, nbins, build)]
    if build is not None:
        parts.append(value_histogram(build, 1, num_class, value_threshold=-1))
    r = [int(v) for v in torch.cat(parts).cpu().tolist()]
    mean, std = _mean_std(r[0], r[1], r[2])
    return {"count": int(height.shape[0]) * int(height.shape[1]), "n": r[0], "mean": mean, "std": std, "max": r[3],
            "hist": np.array(r[4:4 + nbins], dtype=np.int64),
            "class_counts": None if build is None else np.array(r[4 + nbins:], dtype=np.int64)}
