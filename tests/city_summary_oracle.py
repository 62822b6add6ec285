"""The city summary in numpy and Python integers, one window and one block at a time: what srbh_window_sums, srbh_block_sums and
srbh_value_hist must return, and the host numbers made from them.  A helper of tests/test_city_summary_cpu.py and
tests/test_gpu_city_summary.py, not a test.  The reference has no program for this step (its urbanarea_meanstd.xls is a result), so
nothing here is pinned by a fixture: the definitions are the ones include/srbh.h states, written as literally as numpy allows."""
import math
from fractions import Fraction

import numpy as np


def _selected(value, mask, x, y, w, h, vthr, mthr):
    """(the window's values inside the raster, which of them are selected)"""
    H, W = value.shape
    x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + w, W), min(y + h, H)
    if w <= 0 or h <= 0 or x1 <= x0 or y1 <= y0:
        return np.zeros((0, 0), dtype=np.int64), np.zeros((0, 0), dtype=bool)
    v = value[y0:y1, x0:x1].astype(np.int64)
    sel = v > vthr
    if mask is not None:
        sel &= mask[y0:y1, x0:x1].astype(np.int64) > mthr
    return v, sel


def _five(v, sel):
    s = v[sel]                                                          # int64: a sum of squares of < 2^31 values below 2^16 stays below 2^63
    return [int(v.size), int(s.size), int(s.sum()), int((s * s).sum()), int(s.max()) if s.size else 0]


def window_sums(value, pos, mask=None, vthr=0, mthr=0):
    """(N, 5) int64 [count, n, sum, sumsq, max], one window at a time, Python integers"""
    return np.array([_five(*_selected(value, mask, x, y, w, h, vthr, mthr)) for x, y, w, h in np.asarray(pos).tolist()],
                    dtype=np.int64).reshape(-1, 5)


def block_sums(value, block, mask=None, vthr=0, mthr=0):
    """(4, Hb, Wb) int64 planes n, sum, sumsq, max, one block at a time"""
    H, W = value.shape
    Hb, Wb = -(-H // block), -(-W // block)
    out = np.zeros((4, Hb, Wb), dtype=np.int64)
    for by in range(Hb):
        for bx in range(Wb):
            out[:, by, bx] = _five(*_selected(value, mask, bx * block, by * block, block, block, vthr, mthr))[1:]
    return out


def bin_index(v, bin_width, nbins):
    return np.minimum(np.asarray(v, dtype=np.int64) // bin_width, nbins - 1)


def value_hist(value, bin_width=1, nbins=256, mask=None, vthr=0, mthr=0):
    v, sel = _selected(value, mask, 0, 0, value.shape[1], value.shape[0], vthr, mthr)
    return np.bincount(bin_index(v[sel], bin_width, nbins), minlength=nbins).astype(np.int64)


def _round(fr):
    """a Fraction to the nearest float64: Fraction.__float__ is int / int, which Python rounds correctly"""
    return float(fr)


def mean_std(n, s, q):
    """exact rational mean and variance, each rounded once; the std is the correctly rounded root of the rounded variance"""
    if n == 0:
        return math.nan, math.nan
    mean = Fraction(s, n)
    var = Fraction(q, n) - mean * mean
    return _round(mean), math.sqrt(_round(var))


def heights(sums):
    """the per-window table from (N, 5) integers, in Fractions"""
    rows = [[int(v) for v in r] for r in np.asarray(sums).tolist()]
    ms = [mean_std(r[1], r[2], r[3]) for r in rows]
    return {"n": np.array([r[1] for r in rows], dtype=np.int64), "count": np.array([r[0] for r in rows], dtype=np.int64),
            "max": np.array([r[4] for r in rows], dtype=np.int64),
            "fraction": np.array([_round(Fraction(r[1], r[0])) if r[0] else math.nan for r in rows], dtype=np.float64),
            "mean": np.array([m for m, _ in ms], dtype=np.float64), "std": np.array([s for _, s in ms], dtype=np.float64)}


def aggregate(value, block, mask=None):
    """aggregate_city's rasters: numpy float64 divisions of the exact integers"""
    s = block_sums(value, block, mask)
    H, W = value.shape
    ys, xs = np.arange(s.shape[1]) * block, np.arange(s.shape[2]) * block
    count = (np.minimum(H - ys, block)[:, None] * np.minimum(W - xs, block)[None, :]).astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return {"n": s[0], "count": count, "max": s[3], "mean": s[1].astype(np.float64) / s[0].astype(np.float64),
                "fraction": s[0].astype(np.float64) / count.astype(np.float64), "density": s[1].astype(np.float64) / count.astype(np.float64)}


def summary(value, mask=None, bin_width=10, nbins=256, num_class=7):
    H, W = value.shape
    count, n, s, q, mx = _five(*_selected(value, mask, 0, 0, W, H, 0, 0))
    mean, std = mean_std(n, s, q)
    return {"count": count, "n": n, "mean": mean, "std": std, "max": mx, "hist": value_hist(value, bin_width, nbins, mask),
            "class_counts": None if mask is None else value_hist(mask, 1, num_class, None, -1)}


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))
