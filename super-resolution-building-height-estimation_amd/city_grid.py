"""Which cells of a city are predicted at all: the reference's fishnet and its per-cell built-up counts, on the device.

The reference lays a fishnet of FULL window x window cells over a city's raster (generate_WSF_mask_Globeheight_grid.py:275-449,
``Fishgridnew_bound(tif, window_size=64, offset=56)``), counts the World-Settlement-Footprint pixels of every cell
(demo_preprocess_height_v2.py:1143-1186, ``Fishgrid_stats(..., condition=(0, 20, 4096))``) and predicts the cells with ``isv > 0`` only
(BH_loader.py:908-929, ``generateindex(shp, geotrans, validname='isv')``); its training samples were chosen by comparing two footprint
rasters cell by cell (``compare_twotiff_valid`` / ``compare_twotiff_valid_iou``, demo_preprocess_height_v2.py:740-933).  Here

* ``fishgrid_windows``  the fishnet in pixel space, in the reference's feature order (host, numpy);
* ``cell_counts``       per window ``[n_a, n_b, n_and, count]`` for thousands of overlapping windows in ONE libsrbh launch
                        (csrc/srbh_cells.hip), exact integers, no host synchronisation;
* ``fishgrid_stats`` / ``compare_cells`` / ``valid_windows``  the reference's fields and flags from those counts, under its names;
* ``city_windows``      the three steps in one call, for handing straight to ``harness.predict_city`` / ``loader_math.GridTiles``.

Quirks kept because the reference has them: the corner cell is written a second time when only one of the two remainders is non-zero;
a window is cast ``.astype(numpy.uint8)`` BEFORE it is compared (``as_uint8=True``: uint16 256 counts as 0, int16 -1 as 255); the IoU
of two empty cells is 0 / 0 = NaN, and NaN passes no threshold.

GPU only.  Shapefiles, GeoTIFFs, the urban-centre polygon intersection, warping the second raster onto the first one's grid and float
rasters are out of scope: both rasters are taken to lie on the grid the windows index."""
import numpy as np
import torch

from . import _lib
from .loader_math import check_windows

__all__ = ["fishgrid_windows", "cell_counts", "stats_from_counts", "compare_from_counts", "fishgrid_stats", "compare_cells", "valid_windows",
           "city_windows"]

_CELL_TYPES = {torch.uint16: 1, torch.int16: 2, torch.uint8: 3}            # include/srbh.h SRBH_GRID_U16 / _I16 / _U8
_CELL_WHAT = "uint8, uint16 or int16 (a float's cast to uint8 is not defined outside 0..255)"


# ---- the fishnet (generate_WSF_mask_Globeheight_grid.py:275-449) ------------------------------------------------------------------------
def fishgrid_windows(width, height, window=64, offset=56, unique=False):
    """(N, 4) int64 windows (xoff, yoff, xcount, ycount) of Fishgridnew_bound over a width x height raster, in the order the reference
    writes its features: the regular cells column by column, then -- where the raster is not covered exactly -- a column flush with the
    right edge, a row flush with the bottom edge, and the corner cell.  Every window is window x window and inside the raster; every
    pixel is covered.  The corner cell repeats the last cell of the extra column (or row) when only one remainder is non-zero: the
    reference writes that duplicate, so it is kept unless ``unique=True`` (exact repeats dropped, the first kept)."""
    width, height, window, offset = int(width), int(height), int(window), int(offset)
    if width < window or height < window or offset < 1 or offset > window:
        raise ValueError(f"fishgrid_windows: needs width, height >= window and 1 <= offset <= window (got {width}, {height}, window "
                         f"{window}, offset {offset}): the reference would write cells outside the raster")
    cols, rows = (width - window) // offset + 1, (height - window) // offset + 1
    diff_col, diff_row = width - ((cols - 1) * offset + window), height - ((rows - 1) * offset + window)
    xy = [(c * offset, r * offset) for c in range(cols) for r in range(rows)]
    if diff_col > 0:
        xy += [(width - window, r * offset) for r in range(rows)]
    if diff_row > 0:
        xy += [(c * offset, height - window) for c in range(cols)]
    if diff_col > 0 or diff_row > 0:
        xy.append((width - window, height - window))
    if unique:
        xy = list(dict.fromkeys(xy))
    pos = np.empty((len(xy), 4), dtype=np.int64)
    pos[:, :2], pos[:, 2:] = np.array(xy, dtype=np.int64).reshape(-1, 2), window
    return pos


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------------
# The argument path of every raster entry (here and in city_summary): ``fn`` is the caller's name, ``names`` what it calls its two
# rasters, ``types`` its dtype table and ``what`` that table in words.  Everything that can be judged without a device is judged first
# (and is testable without one); the device is asked for last.
def _check_rasters(fn, names, a, b, types, what):
    """the checks of one or two rasters (``b`` may be None) that need no device: shapes, types, strides -> (H, W)"""
    for name, t in list(zip(names, (a, b)))[:1 if b is None else 2]:
        if not (torch.is_tensor(t) and t.dim() == 2):
            raise ValueError(f"{fn}: {name} must be an (H, W) tensor (got {getattr(t, 'shape', type(t))})")
        if t.dtype not in types:
            raise TypeError(f"{fn}: {name} is {t.dtype}; the rasters are {what}")
        if min(t.shape) < 1:
            raise ValueError(f"{fn}: {name} {tuple(t.shape)} is empty")
        if t.shape[1] > 1 and t.stride(1) != 1:
            raise ValueError(f"{fn}: {name} has stride {t.stride(1)} along W; it must be 1 (a band or a crop is fine, a transpose is not)")
    H, W = a.shape
    if b is not None and (tuple(b.shape) != (H, W) or b.device != a.device):
        raise ValueError(f"{fn}: {names[1]} {tuple(b.shape)} on {b.device} does not match {names[0]}'s {H} x {W} raster on {a.device}")
    if H * W >= 2 ** 31:
        raise ValueError(f"{fn}: a raster of {H} x {W} pixels; counts are formed in 32 bits, so H * W must stay below 2^31")
    return H, W


def _check_windows(fn, pos, W, H, device):
    """``pos`` judged without a device -> (N, 4) int32 windows, N > 0: the device tensor itself, or the host windows, validated to lie
    inside the raster, for the caller to upload"""
    if torch.is_tensor(pos) and pos.is_cuda:
        if pos.dtype != torch.int32 or pos.dim() != 2 or pos.shape[1] != 4 or pos.device != device:
            raise ValueError(f"{fn}: a device pos must be an (N, 4) int32 tensor on {device} (got {pos.dtype} {tuple(pos.shape)} on "
                             f"{pos.device})")
    else:
        try:
            pos = torch.from_numpy(check_windows(pos, W, H, tile=max(W, H)).astype(np.int32))
        except ValueError as e:
            raise ValueError(f"{fn}: {e}") from None
    if pos.shape[0] == 0:
        raise ValueError(f"{fn}: no windows")
    return pos


def _on_device(fn, names, a, b):
    """checked rasters -> (a, its row stride, b or None, its row stride), read in place; refuses host tensors"""
    out = []
    for name, t in zip(names, (a, b)):
        if t is None:
            out += [None, 0]
            continue
        if not t.is_cuda:
            raise RuntimeError(f"{fn} (libsrbh): {name} must be a device tensor -- there is no CPU path")
        t = t.detach()
        if t.shape[0] > 1 and t.stride(0) < t.shape[1]:             # (an expanded row: rows that overlap cannot be read in place)
            t = t.contiguous()
        out += [t, max(t.stride(0), t.shape[1])]
    return out


def _workspace(fn, workspace, need=0, device=None, align=8):
    """the buffer an entry hands to libsrbh: ``workspace`` itself, judged, or a new one of ``need`` bytes where it is None.  Without
    ``device`` -- an entry's early call, before it asks for a device -- only what needs none is judged: a contiguous device tensor"""
    if workspace is None:
        return None if device is None else torch.empty(max(need, 8), dtype=torch.uint8, device=device)
    ok = torch.is_tensor(workspace) and workspace.is_cuda and workspace.is_contiguous()
    if ok and device is not None:
        ok = workspace.device == device and workspace.numel() * workspace.element_size() >= need and workspace.data_ptr() % align == 0
    if not ok:
        size = "" if device is None else f" of at least {need} bytes on {device}, aligned to {align}"
        raise ValueError(f"{fn}: workspace must be a contiguous device buffer{size}")
    return workspace


def cell_counts(mask, pos, other=None, threshold=0, as_uint8=True):
    """-> device (N, 4) int64 ``[n_a, n_b, n_and, count]`` per window, one srbh_cell_counts launch on the current stream.
    ``mask`` / ``other``: (H, W) device tensors of uint8, uint16 or int16, read in place (stride 1 along W, any row stride: one band of
    a (C, H, W) raster or a crop is not copied).  ``pos``: host (N, 4) windows (xoff, yoff, xcount, ycount), validated to lie inside the
    raster and uploaded; a device int32 (N, 4) tensor is used as is (the kernel counts only what lies inside the raster).
    ``count`` = the window's pixels inside the raster, ``n_a`` = those with f(mask) > threshold, ``n_b`` the same for ``other``, ``n_and``
    both (0 without ``other``); f = the value's low eight bits (``as_uint8``, the reference's ``.astype(numpy.uint8)``) or the value."""
    H, W = _check_rasters("cell_counts", ("mask", "other"), mask, other, _CELL_TYPES, _CELL_WHAT)
    threshold = int(threshold)
    if not -32768 <= threshold <= 65535:
        raise ValueError(f"cell_counts: threshold={threshold} outside -32768..65535")
    pos = _check_windows("cell_counts", pos, W, H, mask.device)
    mask, rs_a, other, rs_b = _on_device("cell_counts", ("mask", "other"), mask, other)
    pos_dev, n = pos.to(mask.device).contiguous(), pos.shape[0]
    out = torch.empty((n, 4), dtype=torch.int64, device=mask.device)
    with torch.cuda.device(mask.device):
        _lib.check(_lib.lib().srbh_cell_counts(mask.data_ptr(), _CELL_TYPES[mask.dtype], rs_a,
                                               None if other is None else other.data_ptr(),
                                               0 if other is None else _CELL_TYPES[other.dtype], rs_b, H, W, pos_dev.data_ptr(), n,
                                               threshold, 1 if as_uint8 else 0, out.data_ptr(), _lib.stream_ptr()), "srbh_cell_counts")
    return out


# ---- the reference's fields and flags from the counts -------------------------------------------------------------------------------------
def stats_from_counts(counts, condition=(0, 20, 4096)):
    """Fishgrid_stats' three fields from (N, 4) host counts [n_a, n_b, n_and, count] (demo_preprocess_height_v2.py:1174-1176)"""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1, 4)
    s, c = counts[:, 0].copy(), counts[:, 3].copy()
    return {"sum": s, "count": c, "isv": ((s >= condition[1]) & (c >= condition[2])).astype(np.int64)}


def compare_from_counts(counts, isv=None, condition=(0, 2000, 65536, 0.3), metric="iou"):
    """compare_twotiff_valid (metric 'absdiff', :802-823) / compare_twotiff_valid_iou (metric 'iou', :897-925) from (N, 4) host counts"""
    if metric not in ("iou", "absdiff"):
        raise ValueError(f"compare_cells: metric must be 'iou' or 'absdiff' (got {metric!r})")
    counts = np.asarray(counts, dtype=np.int64).reshape(-1, 4)
    n_a, n_b, n_and, count = (counts[:, k] for k in range(4))
    done = np.ones(len(counts), dtype=bool) if isv is None else np.asarray(isv).reshape(-1) != 0
    if done.shape[0] != len(counts):
        raise ValueError(f"compare_cells: isv has {done.shape[0]} entries for {len(counts)} windows")
    absdiff = n_a + n_b - 2 * n_and
    with np.errstate(divide="ignore", invalid="ignore"):
        diou = 1 - n_and / (n_a + n_b - n_and).astype(np.float64)           # calculate_iou :732-736: 0 / 0.0 = NaN for two empty cells
        isv3 = diou <= condition[3] if metric == "iou" else absdiff / count <= condition[3]
    isv2 = (n_b >= condition[1]) & (count >= condition[2])
    out = {"vrt_sum": n_b, "vrt_count": count, "absdiff": absdiff, "isv2": isv2, "isv3": isv3, "isv4": isv2 & isv3}
    out = {k: np.where(done, v, 0).astype(np.int64) for k, v in out.items()}      # (the reference skips a row with isv == 0)
    out["diou"] = np.where(done, diou, np.nan)
    return out


def fishgrid_stats(mask, pos, condition=(0, 20, 4096), as_uint8=True):
    """Fishgrid_stats over a device raster: {'sum', 'count', 'isv'} numpy int64 arrays, one entry per window; ``sum`` = the window's
    pixels with value > condition[0], ``count`` its size, ``isv = (sum >= condition[1]) & (count >= condition[2])``.  One launch and
    one device-to-host copy of N x 4 int64."""
    return stats_from_counts(cell_counts(mask, pos, None, condition[0], as_uint8).cpu().numpy(), condition)


def compare_cells(ref_mask, other_mask, pos, isv=None, condition=(0, 2000, 65536, 0.3), metric="iou", as_uint8=True):
    """compare_twotiff_valid_iou (``metric='iou'``) / compare_twotiff_valid (``metric='absdiff'``) over two device rasters on one grid:
    numpy arrays ``vrt_sum`` (built-up pixels of other_mask), ``vrt_count``, ``absdiff`` (pixels where the two binary masks differ),
    ``diou`` = 1 - IoU (float64; NaN where both cells are empty, and then isv3 = 0), ``isv2 = (vrt_sum >= c[1]) & (vrt_count >= c[2])``,
    ``isv3 = diou <= c[3]`` or ``absdiff / vrt_count <= c[3]``, ``isv4 = isv2 & isv3``.  Rows with ``isv == 0`` are skipped as in the
    reference: 0 in the integer fields, NaN in diou."""
    counts = cell_counts(ref_mask, pos, other_mask, condition[0], as_uint8).cpu().numpy()
    return compare_from_counts(counts, isv, condition, metric)


def valid_windows(pos, flags):
    """pos[flags > 0], order kept (generateindex(..., validname=...), BH_loader.py:910-911)"""
    pos, flags = np.asarray(pos), np.asarray(flags).reshape(-1)
    if pos.ndim != 2 or pos.shape[0] != flags.shape[0]:
        raise ValueError(f"valid_windows: {flags.shape[0]} flags for windows of shape {pos.shape}")
    return pos[flags > 0]


def city_windows(width, height, mask, window=64, offset=56, condition=(0, 20, 4096)):
    """The cells of a city the reference predicts: Fishgridnew_bound's fishnet over the width x height raster, kept where the footprint
    ``mask`` (device, (height, width)) has isv > 0.  (N, 4) int64, ready for predict_city / GridTiles."""
    if not torch.is_tensor(mask) or mask.dim() != 2 or tuple(mask.shape) != (int(height), int(width)):
        raise ValueError(f"city_windows: mask {getattr(mask, 'shape', type(mask))} is not the ({height}, {width}) raster")
    pos = fishgrid_windows(width, height, window, offset)
    return valid_windows(pos, fishgrid_stats(mask, pos, condition)["isv"])
