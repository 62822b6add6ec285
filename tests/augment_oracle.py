"""CPU oracle of the training augmentation  --  TEST INFRASTRUCTURE ONLY.

numpy, integer index arithmetic, float64 values.  The chain is materialised literally, one whole-image step after the other, the way
the reference's loader runs it (BH_loader.py:353-369, :731-750): nearest x`up` with np.repeat, the flip with slicing, the 2 x 2 grid
shuffle with four block copies, the rotation with the fixed-point tables and the REFLECT_101 fold, then the normalisation with the
fp32 mins / ranges the kernel gets, the decimation ``[::step, ::step]`` and ``oracle.loader_oracle.label_prep`` on the augmented
label.  Shares no code with srbh_amd.loader_math: both are written from the definition and are fed the same parameter VALUES.

`dtype` of the image functions is the type the VALUES are computed in: float64 is the oracle the kernels are measured against;
float32 runs the same literal chain in the kernel's own precision, which for identity parameters (every weight 0 or 1) is
``loader_oracle.normalize`` bit for bit."""
import math

import numpy as np

from oracle import loader_oracle as LO


def flip(img, code):
    """img (..., H, W); bit 0 reverses the columns, bit 1 the rows"""
    if code & 1:
        img = img[..., :, ::-1]
    if code & 2:
        img = img[..., ::-1, :]
    return img


def grid_shuffle(img, perm):
    """destination cell i takes source cell perm[i]; cells of H/2 x W/2, row-major"""
    H, W = img.shape[-2:]
    hh, wh = H // 2, W // 2
    out = np.empty_like(img)
    for i in range(4):
        s = int(perm[i])
        out[..., (i // 2) * hh:(i // 2 + 1) * hh, (i % 2) * wh:(i % 2 + 1) * wh] = \
            img[..., (s // 2) * hh:(s // 2 + 1) * hh, (s % 2) * wh:(s % 2 + 1) * wh]
    return out


def matrix(angle, H, W):
    """the inverse map's six float64 coefficients: sx = M0 x + M1 y + M2, sy = M3 x + M4 y + M5"""
    a, b = math.cos(math.radians(angle)), math.sin(math.radians(angle))
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    return a, -b, cx - a * cx + b * cy, b, a, cy - b * cx - a * cy


def tables(angle, H, W):
    """int64 ax[W], bx[W], X0[H], Y0[H]; angle None = not rotated = the identity tables"""
    x, y = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    if angle is None:
        return (1024 * np.arange(W, dtype=np.int64), np.zeros(W, dtype=np.int64), np.zeros(H, dtype=np.int64),
                1024 * np.arange(H, dtype=np.int64))
    m = matrix(angle, H, W)
    r = lambda v: np.rint(v).astype(np.int64)          # noqa: E731  (ties to even)
    return r(m[0] * x * 1024), r(m[3] * x * 1024), r((m[1] * y + m[2]) * 1024), r((m[4] * y + m[5]) * 1024)


def reflect101(i, n):
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i >= n, p - i, i)


def coords_nearest(angle, H, W):
    ax, bx, X0, Y0 = tables(angle, H, W)
    return (X0[:, None] + ax[None, :] + 512) >> 10, (Y0[:, None] + bx[None, :] + 512) >> 10


def coords_bilinear(angle, H, W):
    """X, Y in 1/32 px: integer part X >> 5, fraction (X & 31) / 32"""
    ax, bx, X0, Y0 = tables(angle, H, W)
    return (X0[:, None] + ax[None, :] + 16) >> 5, (Y0[:, None] + bx[None, :] + 16) >> 5


def rotate_nearest(img, angle):
    H, W = img.shape[-2:]
    X, Y = coords_nearest(angle, H, W)
    return img[..., reflect101(Y, H), reflect101(X, W)]


def rotate_bilinear(img, angle, dtype=np.float64):
    """img (..., H, W) -> (value, S): the bilinear sample and the same combination of |img| (the scale of its rounding error)"""
    H, W = img.shape[-2:]
    X, Y = coords_bilinear(angle, H, W)
    fx, fy = ((X & 31) / 32.0).astype(dtype), ((Y & 31) / 32.0).astype(dtype)
    x0, x1, y0, y1 = reflect101(X >> 5, W), reflect101((X >> 5) + 1, W), reflect101(Y >> 5, H), reflect101((Y >> 5) + 1, H)
    one = dtype(1)
    w = ((one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy)
    v = img.astype(dtype)
    c = (v[..., y0, x0], v[..., y0, x1], v[..., y1, x0], v[..., y1, x1])
    val = w[0] * c[0] + w[1] * c[1] + w[2] * c[2] + w[3] * c[3]
    S = w[0] * np.abs(c[0]) + w[1] * np.abs(c[1]) + w[2] * np.abs(c[2]) + w[3] * np.abs(c[3])
    return val, S


def aug_image(raw, up, step, code, perm, angle, mins=None, ranges=None, datarange=None, dtype=np.float64):
    """one sample raw (C, Hs, Ws) -> (out, bound_scale): out (C, Hs up / step, Ws up / step) in `dtype`; bound_scale is
    (S + |min_c|) / range_c (S alone without normalisation), what the test multiplies by 2^-21.  mins / ranges: the fp32 arrays the
    kernel gets."""
    g = np.repeat(np.repeat(np.asarray(raw), up, axis=-2), up, axis=-1)
    g = grid_shuffle(flip(g, code), perm)
    v, S = rotate_bilinear(g, angle, dtype)
    scale = S.astype(np.float64)
    if mins is not None:
        mn, rg = np.asarray(mins, dtype=np.float32).astype(dtype)[:, None, None], np.asarray(ranges, dtype=np.float32).astype(dtype)[:, None, None]
        v = (v - mn) / rg
        scale = (scale + np.abs(mn.astype(np.float64))) / rg.astype(np.float64)
        if datarange is not None:
            v = np.clip(v, dtype(datarange[0]), dtype(datarange[1]))
    return v[:, ::step, ::step], scale[:, ::step, ::step]


def aug_label(height_u8, code, perm, angle):
    return np.ascontiguousarray(rotate_nearest(grid_shuffle(flip(np.asarray(height_u8), code), perm), angle))


def aug_label_prep(height_u8, code, perm, angle, hir, heightweight):
    """one sample (H, W) uint8 -> (label, (height, height_aggre, build, weight, weight_aggre) as loader_oracle.label_prep)"""
    lab = aug_label(height_u8, code, perm, angle)
    return lab, LO.label_prep(lab, hir, heightweight)
