"""The city comparison in numpy int64 and Python integers, one window and one class at a time: what srbh_pair_sums and
srbh_pair_class_sums must return, the host numbers made from them, and the inputs the GPU tests run on.  A helper of
tests/test_city_compare_cpu.py and tests/test_gpu_city_compare.py, not a test.  The reference has no program for the exact rule (cal_rmse
reads files through cv2, vtest_epoch2 works on float tiles), so nothing here is pinned by a fixture: the definitions are the ones
include/srbh.h states, written as literally as numpy allows.

``mistake`` turns ONE rule into a plausible wrong one; tests/test_city_compare_cpu.py asserts that each of them changes the result on the
GPU tests' own inputs (the oracle is not blind to them)."""
import math
from fractions import Fraction

import numpy as np

MODES = ("any", "both", "ref", "pred")
MISTAKES = ("r_minus_p", "no_abs", "gt_at_edge", "cm_transposed", "or_in_both", "mask_on_count")


# ---- the rule -------------------------------------------------------------------------------------------------------------------------------
def _clip(shape, x, y, w, h):
    H, W = shape
    x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + w, W), min(y + h, H)
    if w <= 0 or h <= 0 or x1 <= x0 or y1 <= y0:
        return None
    return slice(y0, y1), slice(x0, x1)


def _compared(p, r, m, mode, pthr, rthr, mthr, mistake=None):
    P, R = p > pthr, r > rthr
    if mode == "any":
        sel = P | R
    elif mode == "both":
        sel = (P | R) if mistake == "or_in_both" else (P & R)
    elif mode == "ref":
        sel = R.copy()
    elif mode == "pred":
        sel = P.copy()
    else:
        raise ValueError(mode)
    if m is not None:
        sel &= m > mthr
    return sel


def _ten(p, r, sel, count, mistake=None):
    p, r = p[sel], r[sel]
    d = r - p if mistake == "r_minus_p" else p - r
    ad = d if mistake == "no_abs" else np.abs(d)
    return [int(count), int(p.size), int(d.sum()), int(ad.sum()), int((d * d).sum()), int(p.sum()), int(r.sum()), int((p * p).sum()),
            int((r * r).sum()), int((p * r).sum())]


def pair_sums(pred, ref, pos, mask=None, mode="any", pthr=0, rthr=0, mthr=0, mistake=None):
    """(N, 10) int64 [count, n, sd, sad, sdd, sp, sr, spp, srr, spr], one window at a time"""
    out = []
    for x, y, w, h in np.asarray(pos).tolist():
        c = _clip(pred.shape, x, y, w, h)
        if c is None:
            out.append([0] * 10)
            continue
        p, r = pred[c].astype(np.int64), ref[c].astype(np.int64)
        m = None if mask is None else mask[c].astype(np.int64)
        sel = _compared(p, r, m, mode, pthr, rthr, mthr, mistake)
        count = p.size
        if mistake == "mask_on_count" and m is not None:
            count = int((m > mthr).sum())
        out.append(_ten(p, r, sel, count, mistake))
    return np.array(out, dtype=np.int64).reshape(-1, 10)


def class_of(v, edges, mistake=None):
    """the number of k in 1 .. C - 1 with v >= edges[k]"""
    v = np.asarray(v, dtype=np.int64)
    c = np.zeros(v.shape, dtype=np.int64)
    for e in list(edges)[1:]:
        c += (v > e) if mistake == "gt_at_edge" else (v >= e)
    return c


def class_sums(pred, ref, edges, build=None, mode="any", pthr=-1, rthr=-1, mthr=-1, mistake=None):
    """((C, 4 + C) int64 rows [n, sd, sad, sdd, cm[c][0..C-1]], bad), one class at a time"""
    C = len(edges)
    p, r = pred.astype(np.int64), ref.astype(np.int64)
    m = None if build is None else build.astype(np.int64)
    sel = _compared(p, r, m, mode, pthr, rthr, mthr, mistake)
    c = class_of(r, edges, mistake)
    pc = m if m is not None else class_of(p, edges, mistake)
    rows = np.zeros((C, 4 + C), dtype=np.int64)
    for k in range(C):
        s = sel & (c == k)
        rows[k, :4] = _ten(p, r, s, 0, mistake)[1:5]
        for j in range(C):
            rows[k, 4 + j] = int((s & (pc == j)).sum())
    if mistake == "cm_transposed":
        rows[:, 4:] = rows[:, 4:].T.copy()
    return rows, int((sel & (pc >= C)).sum())


# ---- the host numbers -------------------------------------------------------------------------------------------------------------------------
def errors(sums):
    """errors_from_sums in Fractions: every quotient exact, rounded once (Fraction.__float__ is int / int, which Python rounds
    correctly); r = (n spr - sp sr) / sqrt((n spp - sp^2)(n srr - sr^2)) with the integers formed exactly before the one conversion"""
    rows = [[int(v) for v in r] for r in np.asarray(sums).tolist()]
    names = ("fraction", "me", "mae", "rmse", "mean_pred", "mean_ref", "r", "r2")
    cols = {k: [] for k in names}
    for count, n, sd, sad, sdd, sp, sr, spp, srr, spr in rows:
        cols["fraction"].append(float(Fraction(n, count)) if count else math.nan)
        if n == 0:
            for k in names[1:]:
                cols[k].append(math.nan)
            continue
        vp, vr, cov = n * spp - sp * sp, n * srr - sr * sr, n * spr - sp * sr
        cols["me"].append(float(Fraction(sd, n)))
        cols["mae"].append(float(Fraction(sad, n)))
        cols["rmse"].append(math.sqrt(float(Fraction(sdd, n))))
        cols["mean_pred"].append(float(Fraction(sp, n)))
        cols["mean_ref"].append(float(Fraction(sr, n)))
        cols["r"].append(cov / math.sqrt(vp * vr) if vp and vr else math.nan)
        cols["r2"].append(float(1 - Fraction(n * sdd, vr)) if vr else math.nan)
    out = {"n": np.array([r[1] for r in rows], dtype=np.int64), "count": np.array([r[0] for r in rows], dtype=np.int64)}
    out.update({k: np.array(v, dtype=np.float64) for k, v in cols.items()})
    return out


def metric_tables(rows):
    """(HeightMetric stats (C, 3), count (C, 1), confusion matrix (C, C)) as float64 numpy from the class rows, as HeightEvaluation.result()
    fills them with the raster as one batch: sqrt(sdd / n) n (0 without pixels), sad, sd"""
    rows = [[int(v) for v in r] for r in np.asarray(rows).tolist()]
    stats = np.array([[math.sqrt(float(Fraction(r[3], r[0]))) * r[0] if r[0] else 0.0, float(r[2]), float(r[1])] for r in rows], dtype=np.float64)
    return stats, np.array([[float(r[0])] for r in rows], dtype=np.float64), np.array([r[4:] for r in rows], dtype=np.float64)


def block_errors(pred, ref, block, mask=None):
    """numpy float64: the block means over the blocks where either sum is non-zero; {"n_blocks", "sums" (8,), "me", "mae", "rmse", "r"}"""
    H, W = pred.shape
    e, mp, mr = [], [], []
    for y in range(0, H, block):
        for x in range(0, W, block):
            c = (slice(y, min(y + block, H)), slice(x, min(x + block, W)))
            sel = np.ones(pred[c].shape, dtype=bool) if mask is None else mask[c] > 0
            sp, sr, n = int(pred[c][sel].astype(np.int64).sum()), int(ref[c][sel].astype(np.int64).sum()), int(sel.sum())
            if sp or sr:
                e.append(np.float64(sp - sr) / np.float64(n))
                mp.append(np.float64(sp) / np.float64(n))
                mr.append(np.float64(sr) / np.float64(n))
    e, mp, mr = (np.array(v, dtype=np.float64) for v in (e, mp, mr))
    terms = [e, np.abs(e), e * e, mp, mr, mp * mp, mr * mr, mp * mr]
    s = np.array([math.fsum(t) for t in terms], dtype=np.float64)
    k = np.float64(len(e))
    with np.errstate(divide="ignore", invalid="ignore"):
        return {"n_blocks": len(e), "sums": s, "abs_sums": np.array([math.fsum(np.abs(t)) for t in terms]), "me": s[0] / k, "mae": s[1] / k,
                "rmse": np.sqrt(s[2] / k), "r": (k * s[7] - s[3] * s[4]) / np.sqrt((k * s[5] - s[3] * s[3]) * (k * s[6] - s[4] * s[4]))}


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ---- the inputs of the GPU tests ----------------------------------------------------------------------------------------------------------------
H0, W0 = 70, 131
THRESHOLD_VALUES = (0, 1, 6, 7, 254, 255, 256, 65534, 65535)


def raster(dtype, H, W, seed, zeros=0.5, top=None):
    """`zeros` of the pixels are 0; both ends of the type (or 0 and `top`) are present"""
    rs = np.random.RandomState(seed)
    top = np.iinfo(dtype).max if top is None else top
    a = rs.randint(0, top + 1, size=(H, W)).astype(dtype)
    a[rs.rand(H, W) < zeros] = 0
    a[0, 0], a[-1, -1], a[0, -1], a[-1, 0] = top, top, 1, top - 1
    return a


def triple(tp, tr, tm, H=H0, W=W0, seed=1):
    """(pred, ref, mask or None) of the element types given; about a quarter of the reference equals the prediction"""
    p, r = raster(tp, H, W, seed), raster(tr, H, W, seed + 100)
    same = np.random.RandomState(seed + 200).rand(H, W) < 0.25
    r[same] = np.minimum(p[same].astype(np.int64), np.iinfo(tr).max).astype(tr)
    return p, r, None if tm is None else raster(tm, H, W, seed + 300, zeros=0.3)


def edge_windows(H, W):
    """xoff 0..17 x xcount 1..40 (a stride of widths, every one of them once) x ycount 1, 3 and H; the same flush with the right edge;
    the four corner pixels; the whole raster"""
    pos = []
    for xoff in range(18):
        for i, xcount in enumerate(range(1 + xoff % 3, 41, 3)):
            for ycount, yoff in ((1, (xoff * 7 + xcount) % H), (3, (xoff * 5 + xcount) % (H - 2)), (H, 0)):
                pos.append((xoff, yoff, xcount, ycount))
                pos.append((W - xcount - (xoff + i) % 3, yoff, xcount, ycount))
    pos += [(0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1), (0, 0, W, H), (0, 0, W, 1), (0, H - 1, W, 1),
            (0, 0, 1, H), (W - 1, 0, 1, H), (0, 0, 40, H), (W - 40, 0, 40, H)]
    return np.array(pos, dtype=np.int64)


def threshold_case():
    """small rasters of the values next to every threshold the tests use, and their windows"""
    rs = np.random.RandomState(5)
    v = np.array(THRESHOLD_VALUES, dtype=np.uint16)
    p, r = v[rs.randint(0, len(v), size=(29, 37))], v[rs.randint(0, len(v), size=(29, 37))]
    m = np.array((0, 1, 6, 7, 254, 255), dtype=np.uint8)[rs.randint(0, 6, size=(29, 37))]
    p[0, :len(v)], r[1, :len(v)] = v, v
    pos = np.array([(0, 0, 37, 29), (0, 0, len(v), 2), (5, 3, 19, 11), (36, 28, 1, 1)] + [(i, 0, 1, 2) for i in range(len(v))])
    return p, r, m, pos


def class_case(name):
    """(pred, ref, build) uint16, uint16, uint8 for the class tests; heights around the default edges, on / one below / one above them"""
    near = np.array([0, 1, 29, 30, 31, 119, 120, 121, 209, 210, 211, 299, 300, 301, 599, 600, 601, 899, 900, 901, 65535], dtype=np.uint16)
    H, W = {"7x9": (7, 9), "131x70": (H0, W0), "300x300": (300, 300), "zeros": (H0, W0)}[name]
    rs = np.random.RandomState(H * 1000 + W)
    if name == "zeros":
        return np.zeros((H, W), np.uint16), np.zeros((H, W), np.uint16), np.zeros((H, W), np.uint8)
    p, r = near[rs.randint(0, len(near), size=(H, W))], near[rs.randint(0, len(near), size=(H, W))]
    r[rs.rand(H, W) < 0.6] = 0                                         # the label histogram is mostly zeros
    p[(r == 0) & (rs.rand(H, W) < 0.7)] = 0
    b = rs.randint(0, 7, size=(H, W)).astype(np.uint8)
    b[rs.rand(H, W) < 0.05] = rs.randint(7, 256)                       # classes beyond the table of C = 7
    return p, r, b


CLASS_EDGES = {2: (0, 1), 7: (0, 30, 120, 210, 300, 600, 900), 16: (0, 1, 29, 30, 31, 120, 121, 210, 300, 301, 600, 601, 900, 901, 40000, 65535)}
EMPTY_CLASS_EDGES = (0, 30, 120, 210, 300, 600, 650, 700, 900)        # no value of class_case lies in [650, 700): class 6 has no pixel
