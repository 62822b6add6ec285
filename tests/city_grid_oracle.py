"""A literal numpy restatement of the reference's city grid: the layout of Fishgridnew_bound in pixel space
(generate_WSF_mask_Globeheight_grid.py:275-449), the per-window counts of Fishgrid_stats and compare_twotiff_valid(_iou)
(demo_preprocess_height_v2.py:1143-1186, :740-933) and their flags.  One window at a time, slices and .sum() as the reference writes
them; tests/golden/g20_city_grid.npz (tools/make_golden_city_grid.py) pins it against the reference's own functions."""
import numpy as np


def fishgrid_windows(width, height, window=64, offset=56):
    """the four steps of Fishgridnew_bound: regular cells column-major, the right column, the bottom row, the corner cell"""
    cols = (width - window) // offset + 1
    rows = (height - window) // offset + 1
    diff_col = width - ((cols - 1) * offset + window)
    diff_row = height - ((rows - 1) * offset + window)
    pos = []
    for c in range(cols):
        for r in range(rows):
            pos.append((c * offset, r * offset, window, window))
    if diff_col > 0:
        for r in range(rows):
            pos.append((width - window, r * offset, window, window))
    if diff_row > 0:
        for c in range(cols):
            pos.append((c * offset, height - window, window, window))
    if diff_col > 0 or diff_row > 0:
        pos.append((width - window, height - window, window, window))
    return np.array(pos, dtype=np.int64).reshape(-1, 4)


def _binary(m, x, y, w, h, thr, as_uint8):
    """the window's pixels inside the raster, compared as the reference compares them (:1172-1173)"""
    H, W = m.shape
    x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + w, W), min(y + h, H)
    if w <= 0 or h <= 0 or x1 <= x0 or y1 <= y0:
        return np.zeros((0, 0), dtype=bool)
    cut = m[y0:y1, x0:x1]
    if as_uint8:
        cut = cut.astype(np.uint8)
    return cut.astype(np.int64) > thr


def cell_counts(mask, pos, other=None, threshold=0, as_uint8=True):
    """(N, 4) int64 [n_a, n_b, n_and, count], one window at a time"""
    out = np.zeros((len(pos), 4), dtype=np.int64)
    for i, (x, y, w, h) in enumerate(np.asarray(pos).tolist()):
        a = _binary(mask, x, y, w, h, threshold, as_uint8)
        out[i, 0], out[i, 3] = a.sum(), a.size
        if other is not None:
            b = _binary(other, x, y, w, h, threshold, as_uint8)
            out[i, 1], out[i, 2] = b.sum(), (a & b).sum()
    return out


def fishgrid_stats(mask, pos, condition=(0, 20, 4096), as_uint8=True):
    """Fishgrid_stats' fields, feature by feature"""
    res = {k: np.zeros(len(pos), dtype=np.int64) for k in ("sum", "count", "isv")}
    for i, (x, y, w, h) in enumerate(np.asarray(pos).tolist()):
        out_data = _binary(mask, x, y, w, h, condition[0], as_uint8).astype(np.uint8)
        isum, icount = out_data.sum(), out_data.size
        res["sum"][i], res["count"][i] = isum, icount
        res["isv"][i] = 1 if (isum >= condition[1]) and (icount >= condition[2]) else 0
    return res


def compare_cells(ref_mask, other_mask, pos, isv=None, condition=(0, 2000, 65536, 0.3), metric="iou", as_uint8=True):
    """compare_twotiff_valid (metric 'absdiff') / compare_twotiff_valid_iou (metric 'iou'), feature by feature; a row with isv == 0 is
    skipped: 0 in the integer fields, NaN in diou"""
    n = len(pos)
    res = {k: np.zeros(n, dtype=np.int64) for k in ("vrt_sum", "vrt_count", "absdiff", "isv2", "isv3", "isv4")}
    res["diou"] = np.full(n, np.nan)
    for i, (x, y, w, h) in enumerate(np.asarray(pos).tolist()):
        if isv is not None and isv[i] == 0:
            continue
        d1 = _binary(ref_mask, x, y, w, h, condition[0], as_uint8).astype(np.uint8)
        d2 = _binary(other_mask, x, y, w, h, condition[0], as_uint8).astype(np.uint8)
        isum, icount = d2.sum(), d2.size
        ivalid2 = 1 if (isum >= condition[1]) and (icount >= condition[2]) else 0
        diff = (d1 != d2).astype(np.uint8).sum()
        with np.errstate(divide="ignore", invalid="ignore"):
            overlap, union = d2 * d1, (d2 + d1) > 0
            diou = 1 - overlap.sum() / float(union.sum())
            ivalid3 = int(diou <= condition[3]) if metric == "iou" else int((diff / icount) <= condition[3])
        res["vrt_sum"][i], res["vrt_count"][i], res["absdiff"][i] = isum, icount, diff
        res["isv2"][i], res["isv3"][i], res["isv4"][i] = ivalid2, ivalid3, 1 if (ivalid2 == 1 and ivalid3 == 1) else 0
        res["diou"][i] = diou
    return res
