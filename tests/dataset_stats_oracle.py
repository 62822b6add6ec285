"""Exact restatement of srbh_amd.dataset_stats' per-image pass (a helper, not a test): numpy + fractions.

A band's valid pixels -- neither NaN nor equal to nodata -- are turned into integers over one power-of-two denominator (every float32,
uint16 and int16 value is such a rational), so count, min, max, the mean S / n and the population variance (n Q - S^2) / n^2 are EXACT
rationals; each is rounded to float64 once.  A table row is {min, max, mean, sqrt(var)}: the project's statement of what GDAL's
ComputeStatistics(False) is understood to return (GDAL itself is not available here).  Labels: np.bincount."""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53


def valid_values(band, nodata=None):
    """the valid pixels of a band as a flat array of its own dtype, row-major"""
    v = np.asarray(band).reshape(-1)
    keep = np.ones(v.shape, dtype=bool)
    if v.dtype.kind == "f":
        keep &= ~np.isnan(v)
    if nodata is not None:
        keep &= v.astype(np.float64) != float(nodata)
    return v[keep]


def band_exact(band, nodata=None):
    """-> dict(count, min, max, mean, var): count int, min / max float (None when count == 0), mean / var Fractions"""
    v = valid_values(band, nodata)
    n = int(v.size)
    if n == 0:
        return dict(count=0, min=None, max=None, mean=None, var=None)
    if v.dtype.kind in "iu":
        ints, den = [int(x) for x in v], 1
    else:
        ratios = [float(x).as_integer_ratio() for x in v]
        den = max(d for _, d in ratios)
        ints = [a * (den // d) for a, d in ratios]
    s, q = sum(ints), sum(a * a for a in ints)
    return dict(count=n, min=float(v.min()), max=float(v.max()), mean=Fraction(s, n * den), var=Fraction(n * q - s * s, n * n * den * den))


def band_row(band, nodata=None):
    """(row (4,) float64 {min, max, mean, std}, count): the exact mean and variance rounded once to float64, std = sqrt of that variance;
    four NaNs when no pixel is valid"""
    e = band_exact(band, nodata)
    if e["count"] == 0:
        return np.full(4, np.nan), 0
    return np.array([e["min"], e["max"], float(e["mean"]), math.sqrt(float(e["var"]))], dtype=np.float64), e["count"]


def table(images, nodata=None):
    """images (N, C, H, W) -> (stats (N, C, 4) float64, count (N, C) int64), band_stats' layout"""
    images = np.asarray(images)
    n, c = images.shape[:2]
    stats, count = np.empty((n, c, 4)), np.empty((n, c), dtype=np.int64)
    for i in range(n):
        for b in range(c):
            stats[i, b], count[i, b] = band_row(images[i, b], nodata)
    return stats, count


def variance_bound(n, mean, var):
    """error bound of the corrected two-pass variance in float64 (Chan, Golub & LeVeque 1983): 2 [(n + 2) u var + (n u)^2 (mean^2 + var)]"""
    return 2.0 * ((n + 2) * U * var + (n * U) ** 2 * (mean * mean + var))


def label_histogram(labels):
    return np.bincount(np.asarray(labels, dtype=np.uint8).reshape(-1), minlength=256).astype(np.int64)
