"""CPU oracle of the inference tile cutter  --  TEST INFRASTRUCTURE ONLY.

``cell`` is a literal numpy restatement of the reference's gridimgLoader.__getitem__ (BH_loader.py:965-990): the two window reads, the
transpose to H W C, the band cut, the concatenate, the cast to float32, ``(v - min) / range`` and the transpose back.  In the reference
the subtraction is a float32 torch tensor minus a float64 numpy array, which promotes to float64; the division stays in float64 and
the assignment back into the float32 tensor rounds ONCE.  So the reference's value is the float64 quotient rounded to float32, which is
what ``cell`` returns and ``cell64`` returns unrounded (tests/golden/g18_grid_tiles.npz pins both statements against the reference's
own code).  ``tile`` is this project's batch form: the cell in the top-left corner of a tile x tile square of +0.0.

Shares no code with srbh_amd.loader_math."""
import numpy as np


def norms(s2_stats, s1_stats, nchans):
    """(mins, ranges) float64 over the concatenated bands, as gridimgLoader.__init__ forms them (:956-961); s1_stats None: no Sentinel-1"""
    n2 = np.array(s2_stats, dtype=np.float64)[:, :nchans]
    n2[1] -= n2[0]
    if s1_stats is None:
        return n2[0].copy(), n2[1].copy()
    n1 = np.array(s1_stats, dtype=np.float64).reshape(2, -1)
    n1[1] -= n1[0]
    return np.concatenate([n2[0], n1[0]]), np.concatenate([n2[1], n1[1]])


def read_window(raster, xoff, yoff, xcount, ycount):
    """gdal's ReadAsArray(xoff, yoff, xcount, ycount) of a (C, H, W) array: (C, ycount, xcount); the window must lie inside the raster"""
    C, H, W = raster.shape
    assert 0 <= xoff and 0 <= yoff and xcount >= 1 and ycount >= 1 and xoff + xcount <= W and yoff + ycount <= H, (xoff, yoff, xcount, ycount)
    return raster[:, yoff:yoff + ycount, xoff:xoff + xcount]


def _raw(s2, s1, pos, nchans):
    xoff, yoff, xcount, ycount = (int(v) for v in pos)
    a = read_window(s2, xoff, yoff, xcount, ycount).transpose((1, 2, 0))[:, :, :nchans]       # H W C, band cut (:969-971)
    if s1 is None:
        return a.astype("float32")
    b = read_window(s1, xoff, yoff, xcount, ycount).transpose((1, 2, 0))                      # (:976-977)
    return np.concatenate((a, b), axis=-1).astype("float32")                                     # (:980-981)


def cell64(s2, s1, pos, s2_stats, s1_stats, nchans):
    """(C, ycount, xcount) float64: (float32(v) - min) / range in float64, unrounded"""
    mn, rg = norms(s2_stats, s1_stats, nchans)
    img = _raw(s2, s1, pos, nchans)
    return np.transpose((img.astype(np.float64) - mn) / rg, axes=(2, 0, 1))                      # (:982-983, :988)


def cell(s2, s1, pos, s2_stats, s1_stats, nchans):
    """what gridimgLoader.__getitem__ returns as `img`: cell64 rounded once to float32"""
    return cell64(s2, s1, pos, s2_stats, s1_stats, nchans).astype(np.float32)


def tile(s2, s1, pos, s2_stats, s1_stats, nchans, tile_side):
    """(C, tile, tile) float32: the cell in [:ycount, :xcount], +0.0 everywhere else"""
    c = cell(s2, s1, pos, s2_stats, s1_stats, nchans)
    out = np.zeros((c.shape[0], tile_side, tile_side), dtype=np.float32)
    out[:, :c.shape[1], :c.shape[2]] = c
    return out


def bound(s2, s1, pos, s2_stats, s1_stats, nchans):
    """(C, ycount, xcount) float64: 2^-23 (|v| + |min_c|) / range_c, the error two correctly rounded fp32 operations may leave (each at
    most 2^-24 of a magnitude no larger than (|v| + |min|) / range; the conversion of v to float32 is exact).  It holds where min_c and
    range_c are float32 values, which the callers see to."""
    mn, rg = norms(s2_stats, s1_stats, nchans)
    img = np.abs(_raw(s2, s1, pos, nchans).astype(np.float64))
    return np.transpose(2.0 ** -23 * (img + np.abs(mn)) / np.abs(rg), axes=(2, 0, 1))
