"""Oracle and case tables of the two ends of the product: the inference epilogue (csrc/srbh_mosaic.hip: srbh_mosaic_accumulate,
srbh_mosaic_finalize) and the loader's plain kernels (csrc/srbh_loader.hip: srbh_label_prep, srbh_normalize_clamp)  --  TEST INFRASTRUCTURE.

The mosaic functions are an integer restatement of include/srbh.h's contract (numpy integers and float64, one tile at a time);
tests/test_io_ends_cpu.py pins them against oracle/mosaic_oracle.py (the literal restatement of the reference's lines) and the reference's
own fixture tests/golden/g12_mosaic.npz.  `label_prep` and `normalize` are batch-shaped calls of oracle/loader_oracle.py, nothing restated.

Inputs for which exactness can be demanded.  Everything in the epilogue is integer work or a single correctly rounded fp32 operation except
the class quantum rintf(e_c / s * 255).  The kernel computes, per pixel (eps = 2^-24, every fl() one fp32 rounding):
    m   = max_c z_c                                    exact
    d_c = fl(z_c - m)                                  ONE rounding, the same one torch.softmax makes: the oracle takes d in fp32 too
    e_c = expf(d_c)                                    ASSUMED good to 2 ulp = 4 eps relative (the toolchain ships no accuracy table; the
                                                       same assumption tests/test_gpu_train_glue.py makes)
    s   = fl(..fl(fl(e_0 + e_1) + e_2).. + e_{C-1})    positive terms: 4 eps from the exponentials and C - 1 adds of one eps each
    t_c = fl(fl(e_c / s) * 255)                        4 + (C + 3) from the operands, one rounding each for quotient and product
so t_c is within (C + 9) eps RELATIVE of the float64 value p_c * 255 <= 255 to first order; the second-order terms ((C + 9)^2 eps^2) and
the float64 oracle's own error (2^-29 of that) are covered by one more eps.  An entry whose float64 value lies at least
    DELTA(C) = 255 (C + 10) 2^-24
from every .5 boundary therefore rounds to the oracle's integer whatever the order of the sum or the last bits of expf.  `clean_logits`
draws z = 3 randn and redraws every pixel that has an entry inside DELTA until none is left; the quantised class sums of such inputs have
ONE right answer and the GPU tests demand it at every entry.  (C = 1: e = s = 1, the quantum is 255 exactly.)

Why DELTA is the derived bound and not twice it (255 (2C + 10) 2^-24 was proposed with these tests).  About 0.05 % of the ENTRIES of a
3 randn draw lie inside DELTA, 0.09 % inside twice DELTA, whatever C is; a pixel is redrawn when any of its C entries does, so the share of
redrawn PIXELS grows with C: measured over 400 000 pixels 0.29 % / 0.77 % / 0.84 % at C = 7 / 15 / 16 with DELTA, 0.43 % / 1.31 % / 1.41 %
with twice DELTA.  The inputs are to stay the random draw -- fewer than 1 % of the pixels redrawn, asserted in tests/test_io_ends_cpu.py --,
which twice DELTA cannot meet at C >= 11.  For the same reason C = 15 and 16 are run on samples large enough (57 344 pixels) for that share
to be a property of the draw and not of the seed.
"""
import functools
import os
import zlib
from collections import namedtuple

import numpy as np
import torch

from oracle import loader_oracle as LO

EPS32 = 2.0 ** -24
M16, M8 = 0xFFFF, 0xFF


def delta(C):
    return 255.0 * (C + 10) * EPS32


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


# ---- the two quanta ---------------------------------------------------------------------------------------------------------------------
def height_quanta(h):
    """np.round(fl32(max(h, 0) * 10)) mod 2^16 as int64: the fp32 product and the half-even rounding the kernel and the reference both use"""
    h = np.asarray(h, dtype=np.float32)
    hv = np.where(h < 0, np.float32(0), h).astype(np.float32)
    t = hv * np.float32(10)
    assert t.dtype == np.float32
    return np.round(t).astype(np.int64) & M16


def class_quanta(z):
    """z (..., C) fp32 logits -> (round(p * 255) int64, margin float64): p the float64 softmax of the FP32 differences d = fl32(z - max z);
    margin = |frac(p * 255) - 0.5|, the distance of an entry from the nearest rounding boundary"""
    z = np.asarray(z, dtype=np.float32)
    d = z - z.max(axis=-1, keepdims=True)
    assert d.dtype == np.float32
    e = np.exp(d.astype(np.float64))
    t = e / e.sum(axis=-1, keepdims=True) * 255.0
    return np.round(t).astype(np.int64), np.abs(t - np.floor(t) - 0.5)


def class_quanta_fp32(z):
    """a numpy-fp32 emulation of the kernel's own order (expf of the library at hand, the sum in class order 0 .. C - 1)"""
    z = np.asarray(z, dtype=np.float32)
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    s = np.zeros(z.shape[:-1], dtype=np.float32)
    for c in range(z.shape[-1]):
        s = s + e[..., c]
    t = e / s[..., None] * np.float32(255)
    assert t.dtype == np.float32
    return np.round(t).astype(np.int64)


# ---- srbh_mosaic_accumulate / srbh_mosaic_finalize ----------------------------------------------------------------------------------------
Acc = namedtuple("Acc", "res_h res_b res_w margin")


def mosaic_accumulate(height, logits_nhwc, pos, H, W, state=None):
    """height (B, th, tw) fp32, logits (B, th, tw, C) fp32, pos (B, 4) = (xoff, yoff, xcount, ycount) in MOSAIC PIXELS, state = the three
    uint32 accumulators to add onto (None: zeros).  Pixel (x, y) of tile b lands at (xoff + x, yoff + y) iff x < xcount, y < ycount and the
    target is inside [0, W) x [0, H).  Returns uint32 (H, W), (C, H, W), (H, W) and the margin of every entry (B, th, tw, C)."""
    height, logits_nhwc = np.asarray(height, dtype=np.float32), np.asarray(logits_nhwc, dtype=np.float32)
    B, th, tw, C = logits_nhwc.shape
    assert height.shape == (B, th, tw)
    pos = np.asarray(pos, dtype=np.int64).reshape(B, 4)
    if state is None:
        state = (np.zeros((H, W), np.uint32), np.zeros((C, H, W), np.uint32), np.zeros((H, W), np.uint32))
    res_h, res_b, res_w = (np.asarray(s).astype(np.uint32).astype(np.int64) for s in state)
    hq = height_quanta(height)
    bq, margin = class_quanta(logits_nhwc)
    for b in range(B):
        xoff, yoff, xcount, ycount = (int(v) for v in pos[b])
        x0, x1 = max(0, -xoff), min(tw, xcount, W - xoff)
        y0, y1 = max(0, -yoff), min(th, ycount, H - yoff)
        if x1 <= x0 or y1 <= y0:
            continue
        ys, xs = slice(yoff + y0, yoff + y1), slice(xoff + x0, xoff + x1)
        res_h[ys, xs] += hq[b, y0:y1, x0:x1]
        res_w[ys, xs] += 1
        res_b[:, ys, xs] += bq[b, y0:y1, x0:x1].transpose(2, 0, 1)
    m32 = 0xFFFFFFFF
    return Acc((res_h & m32).astype(np.uint32), (res_b & m32).astype(np.uint32), (res_w & m32).astype(np.uint32), margin)


def added_mask(pos, th, tw, H, W):
    """(B, th, tw) bool: the tile pixels that mosaic_accumulate adds somewhere"""
    pos = np.asarray(pos, dtype=np.int64).reshape(-1, 4)
    x, y = np.arange(tw)[None, None, :], np.arange(th)[None, :, None]
    xo, yo, xc, yc = (pos[:, k][:, None, None] for k in range(4))
    return (x < xc) & (y < yc) & (xo + x >= 0) & (xo + x < W) & (yo + y >= 0) & (yo + y < H)


def mosaic_finalize(res_h, res_b, res_w, C):
    """literal from include/srbh.h and oracle/mosaic_oracle.py:30-35: sums masked to 16 bits, the weight to 8; np.argmax takes the first
    maximum; height = np.round(h / w) in float64 where w8 > 0, else the masked h.  -> (uint16 (H, W), uint8 (H, W))"""
    h16 = (np.asarray(res_h).astype(np.uint32) & M16).astype(np.uint16)
    b16 = (np.asarray(res_b).astype(np.uint32) & M16).astype(np.uint16)
    w8 = (np.asarray(res_w).astype(np.uint32) & M8).astype(np.uint8)
    assert b16.shape[0] == C
    build = np.argmax(b16, axis=0).astype(np.uint8)
    h = h16.copy()
    mask = w8 > 0
    h[mask] = np.round(h16[mask].astype(np.float64) / w8[mask].astype(np.float64)).astype(np.uint16)
    return h, build


# ---- logits with one right answer ---------------------------------------------------------------------------------------------------------
def _draw_randn3(gen, n, C):
    return torch.randn(n, C, generator=gen) * 3


Clean = namedtuple("Clean", "z rounds first_inside redrawn")


def clean_pixels(n, C, key, draw=_draw_randn3, fp16=False, max_rounds=8):
    """(n, C) fp32 logits from `draw` and the seeded generator of `key`; every pixel with an entry whose margin is below delta(C) is redrawn
    from the same generator until none is left.  fp16: every draw is rounded to fp16 first (the values a half tensor hands to the kernel).
    -> Clean(z read-only numpy, redraw rounds used, entries inside delta on the first draw, pixels that were ever redrawn)"""
    gen = _gen("clean", key, n, C, fp16)
    rnd = (lambda t: t.half().float()) if fp16 else (lambda t: t)
    z = rnd(draw(gen, n, C)).numpy().astype(np.float32)
    first, ever = None, np.zeros(n, dtype=bool)
    for rounds in range(max_rounds + 1):
        inside = class_quanta(z)[1] < delta(C)
        if first is None:
            first = int(inside.sum())
        bad = inside.any(axis=-1)
        if not bad.any():
            z.setflags(write=False)
            return Clean(z, rounds, first, int(ever.sum()))
        ever |= bad
        z[bad] = rnd(draw(gen, int(bad.sum()), C)).numpy()
    raise AssertionError(f"clean_pixels{key}: entries inside delta after {max_rounds} redraw rounds")


@functools.lru_cache(maxsize=None)
def clean_logits(C, B, th, tw, fp16=False, key="acc"):
    c = clean_pixels(B * th * tw, C, (key, C, B, th, tw), fp16=fp16)
    return c._replace(z=c.z.reshape(B, th, tw, C))


# ---- accumulate: the case table -----------------------------------------------------------------------------------------------------------
CITY_H, CITY_W = 40, 52                       # mosaic pixels
AccCase = namedtuple("AccCase", "name C th tw B")
# B th tw: 240 (below one workgroup), 272 / 288 / 800 (a ragged last workgroup of 16 / 32 / 32), 448, 2240, 2880, 8192 and 57 344 (several)
ACC_CASES = (AccCase("c1_4x4_b15", 1, 4, 4, 15), AccCase("c2_4x4_b17", 2, 4, 4, 17), AccCase("c7_4x4_b28", 7, 4, 4, 28),
             AccCase("c7_8x20_b5", 7, 8, 20, 5), AccCase("c2_12x8_b3", 2, 12, 8, 3), AccCase("c7_12x8_b30", 7, 12, 8, 30),
             AccCase("c1_8x20_b14", 1, 8, 20, 14), AccCase("c7_64x64_b2", 7, 64, 64, 2), AccCase("c15_64x64_b14", 15, 64, 64, 14),
             AccCase("c16_64x64_b14", 16, 64, 64, 14))
WINDOW_KINDS = ("full", "cropped", "xcount0", "count1", "count_over", "hang_left", "hang_top", "hang_right", "hang_bottom", "out_left",
                "out_top", "out_right", "out_bottom", "count_negative")


def windows(B, th, tw, H, W, key, first=0):
    """(B, 4) int64 pixel windows, tile b of kind WINDOW_KINDS[(first + b) % 14]; offsets stay within one tile of the city"""
    gen = _gen("win", key, B, th, tw)
    r = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=gen))      # noqa: E731  (inclusive)
    out = []
    for b in range(B):
        kind = WINDOW_KINDS[(first + b) % len(WINDOW_KINDS)]
        xoff, yoff, xc, yc = r(0, max(0, W - tw)), r(0, max(0, H - th)), tw, th
        if kind == "cropped":
            xc, yc = r(min(2, tw - 1), tw - 1), r(min(2, th - 1), th - 1)
        elif kind == "xcount0":
            xc = 0
        elif kind == "count1":
            xc = yc = 1
        elif kind == "count_over":
            xc, yc = tw + 3, th + 5
        elif kind == "hang_left":
            xoff = -r(1, tw - 1)
        elif kind == "hang_top":
            yoff = -r(1, th - 1)
        elif kind == "hang_right":
            xoff = W - r(1, tw - 1)
        elif kind == "hang_bottom":
            yoff = H - r(1, th - 1)
        elif kind == "out_left":
            xoff = -tw
        elif kind == "out_top":
            yoff = -th - r(0, th - 1) // 2
        elif kind == "out_right":
            xoff = W + r(0, tw - 1)
        elif kind == "out_bottom":
            yoff = H
        elif kind == "count_negative":
            yc = -3
        out.append([xoff, yoff, xc, yc])
    return np.array(out, dtype=np.int64)


# heights that must survive: a negative, -0.0, x10 ties on even and odd floors, the largest value the reference's cast defines
SPECIAL_HEIGHTS = (-0.0, -3.7, 0.05, 0.15, 0.25, 12.25, 12.35, 2000.0, 6553.5, 6553.45, 0.0, 100.05)


@functools.lru_cache(maxsize=None)
def heights(B, th, tw, key="acc"):
    """8 randn + 3 (a third negative), every third pixel one of SPECIAL_HEIGHTS or a random k.05 (a x10 tie wherever fp32 keeps it one)"""
    gen = _gen("heights", key, B, th, tw)
    h = (torch.randn(B * th * tw, generator=gen) * 8 + 3).numpy().astype(np.float32)
    k = torch.randint(0, 65535, (B * th * tw,), generator=gen).numpy()
    tie = ((k.astype(np.float64) + 0.5) / 10.0).astype(np.float32)
    i = np.arange(h.size)
    h = np.where(i % 3 == 1, tie, h)
    sp = np.array(SPECIAL_HEIGHTS, dtype=np.float32)
    h = np.where(i % 3 == 2, sp[(i // 3) % sp.size], h).astype(np.float32)
    h = h.reshape(B, th, tw)
    h.setflags(write=False)
    return h


def start_state(C, H, W, key):
    """seeded random accumulators below 2^15, int64 numpy (res_h, res_b, res_w)"""
    gen = _gen("state", key, C, H, W)
    return tuple(torch.randint(0, 1 << 15, s, generator=gen).numpy() for s in ((H, W), (C, H, W), (H, W)))


AccInputs = namedtuple("AccInputs", "height logits pos state want")


@functools.lru_cache(maxsize=None)
def acc_inputs(case):
    c = case
    z = clean_logits(c.C, c.B, c.th, c.tw).z
    h = heights(c.B, c.th, c.tw)
    pos = windows(c.B, c.th, c.tw, CITY_H, CITY_W, c.name, first=ACC_CASES.index(c) * 5)
    state = start_state(c.C, CITY_H, CITY_W, c.name)
    return AccInputs(h, z, pos, state, mosaic_accumulate(h, z, pos, CITY_H, CITY_W, state))


# ---- the order of the softmax sum: the one case kept INSIDE the margin, with a right answer of its own ------------------------------------------
def order_case(C, big_first):
    """logits of one pixel: two classes at 0, the other C - 2 >= 5 at -17, the pair first or last.  e = 1, 1 and C - 2 values t = expf(-17) =
    4.1e-8 < 2^-23 -- whatever expf's last bits.  include/srbh.h: s is the fp32 sum in class order 0 .. C - 1.  Pair first: 1 + 1 = 2, and
    every + t is below half an ulp of 2 (2^-23) and is lost: s = 2, e / s * 255 = 127.5 exactly, rintf gives 128 (half to even).  Pair last:
    the (C - 2) t >= 2.0e-7 add up first, 1 + that rounds to 1 + 2^-22, + 1 is 2 + 2^-22 exactly: e / s * 255 < 127.5 gives 127.  A sum in
    descending order swaps the two answers; the float64 value is 127.4999.., 1e-5 below the boundary, so the float64 oracle says 127 for both
    and is NOT the expected value here.  -> (z (C,) fp32, quanta (C,) int64)"""
    assert C >= 7
    z = np.full(C, -17.0, dtype=np.float32)
    pair = (0, 1) if big_first else (C - 2, C - 1)
    z[list(pair)] = 0.0
    q = np.zeros(C, dtype=np.int64)
    q[list(pair)] = 128 if big_first else 127
    return z, q


# ---- through mosaic.Mosaic: windows in LR CELLS (add multiplies by 4), tiles of 2 x 2 cells = 8 x 8 pixels ----------------------------------
WRAPPER = AccCase("wrapper", 7, 8, 8, 28)


@functools.lru_cache(maxsize=None)
def wrapper_inputs(fp16=False):
    """-> (height (B, 8, 8), logits NHWC, pos in cells (B, 4)); fp16: both tensors hold fp16-representable values"""
    c = WRAPPER
    h = heights(c.B, c.th, c.tw, "wrapper")
    if fp16:
        h = torch.from_numpy(h.copy()).half().float().numpy()
        h.setflags(write=False)
    z = clean_logits(c.C, c.B, c.th, c.tw, fp16=fp16, key="wrapper").z
    return h, z, windows(c.B, c.th // 4, c.tw // 4, CITY_H // 4, CITY_W // 4, "wrapper")


# ---- wrap-around: tiny tiles stacked on one window, from zero mosaics ------------------------------------------------------------------------
WRAP_POS = (5, 7)
WRAP_CASES = ("weight", "height", "class")


def _draw_dominant(gen, n, C):
    """class 0 at about 225 / 255, class 1 at about 30 / 255, class 2 nowhere: 300 x 225 wraps to 1964, below 300 x 30"""
    assert C == 3
    return torch.tensor([2.0, 0.0, -9.0]) + 0.02 * torch.randn(n, C, generator=gen)


@functools.lru_cache(maxsize=None)
def wrap_inputs(name):
    """-> AccInputs from ZERO mosaics (state None)"""
    th = tw = 4
    x, y = WRAP_POS
    if name == "weight":        # 256 full tiles and 44 of two columns: weight 300 (-> 44) in columns 0, 1 and 256 (-> 0) in columns 2, 3
        B, C = 300, 2
        pos = np.array([[x, y, tw, th]] * 256 + [[x, y, 2, th]] * 44, dtype=np.int64)
        h = heights(B, th, tw, "wrap_weight")
        z = clean_logits(C, B, th, tw, key="wrap_weight").z
    elif name == "height":      # 4 x 20 000 = 80 000
        B, C = 4, 2
        pos = np.array([[x, y, tw, th]] * B, dtype=np.int64)
        h = np.full((B, th, tw), 2000.0, dtype=np.float32)
        z = clean_logits(C, B, th, tw, key="wrap_height").z
    else:
        B, C = 300, 3
        pos = np.array([[x, y, tw, th]] * B, dtype=np.int64)
        h = heights(B, th, tw, "wrap_class")
        z = clean_pixels(B * th * tw, C, "wrap_class", draw=_draw_dominant).z.reshape(B, th, tw, C)
    return AccInputs(h, z, pos, None, mosaic_accumulate(h, z, pos, CITY_H, CITY_W))


# ---- finalize on crafted accumulators ------------------------------------------------------------------------------------------------------
FIN_SHAPES = ((1, 1), (5, 51), (16, 16), (1, 257), (25, 40))          # H W = 1, 255, 256, 257, 1000
FIN_C = (1, 2, 7, 16, 20)
# (masked height sum, masked weight): w = 0 and w = 256 -> 0 with h != 0; the half-even ties of h / 2; quotients just off a tie with w = 255;
# w in 1, 3, 255
FIN_HW = ((1234, 0), (40000, 256), (1, 2), (3, 2), (5, 2), (7, 2), (65535, 2), (255 * 7 + 127, 255), (255 * 7 + 128, 255), (65535, 1),
          (65535, 3), (65534, 255), (4, 3), (5, 3), (127, 254), (381, 254), (0, 0), (0, 5))
FIN_HW_WANT = (1234, 40000, 0, 2, 2, 4, 32768, 7, 8, 65535, 21845, 257, 1, 2, 0, 2, 0, 0)
FIN_ARGMAX = ("all_equal", "tie_low_last", "last_only", "tie_after_mask", "order_after_mask")


def finalize_inputs(C, H, W):
    """crafted uint32 accumulators: pixel i takes row i % 18 of FIN_HW and class pattern (i // 18) % 5 of FIN_ARGMAX over a random background
    of small class sums (ties are frequent); EVERY entry then gets random bits above its mask, which no output may depend on"""
    gen = _gen("fin", C, H, W)
    n = H * W
    ri = lambda hi, shape: torch.randint(0, hi, shape, generator=gen).numpy().astype(np.int64)      # noqa: E731
    i = np.arange(n)
    hw = np.array(FIN_HW, dtype=np.int64)[i % len(FIN_HW)]
    h, w = hw[:, 0].copy(), hw[:, 1].copy()
    b = ri(4, (C, n)) + 65532 * (ri(8, (C, n)) == 0)                  # small values with frequent ties; some entries near 2^16
    lo, last = min(1, C - 1), C - 1
    high_b = ri(1 << 16, (C, n))
    kind = (i // len(FIN_HW)) % len(FIN_ARGMAX)
    for k, name in enumerate(FIN_ARGMAX):
        sel = kind == k
        if name == "all_equal":
            b[:, sel] = 77
        elif name == "tie_low_last":
            b[:, sel] = ri(100, (C, int(sel.sum())))
            b[lo, sel] = b[last, sel] = 500
        elif name == "last_only":
            b[:, sel] = ri(100, (C, int(sel.sum())))
            b[last, sel] = 65535
        elif name == "tie_after_mask":        # raw: the last class is far larger; masked: a tie that the first of the two wins
            b[:, sel] = ri(100, (C, int(sel.sum())))
            b[lo, sel] = b[last, sel] = 300
            high_b[lo, sel], high_b[last, sel] = 0, 3
        elif name == "order_after_mask":      # raw: class 0 is largest; masked: the last class
            b[:, sel] = 1
            b[last, sel] = 2
            high_b[:, sel] = 0
            high_b[0, sel] = 2 if C > 1 else 0
    res_h = (h + (ri(1 << 16, (n,)) << 16)).astype(np.uint32).reshape(H, W)
    res_w = (w + (ri(1 << 23, (n,)) << 9)).astype(np.uint32).reshape(H, W)       # (bit 8 stays with w: 256 is a value of the table)
    res_b = (b + (high_b << 16)).astype(np.uint32).reshape(C, H, W)
    return res_h, res_b, res_w


# ---- the loader's plain kernels -----------------------------------------------------------------------------------------------------------
HIR256 = (0, 3, 12, 21, 30, 60, 90, 256)
HIR255 = (0, 3, 12, 21, 30, 60, 90, 255)          # 255 falls in no class: its LUT entry stays 0
# arbitrary fp32 bit patterns: a negative, a subnormal, values that are not bf16-representable
CLASS_WEIGHTS = np.array([0.1, -2.5, 1e-40, 3.0000002, 1e30, 3.14159274, 0.333333343], dtype=np.float32)
PREP_SHAPES = ((1, 4, 4), (3, 8, 12), (2, 20, 36), (5, 64, 68))
PREP_KINDS = ("mixed", "one_below", "all255")


def prep_labels(shape, kind="mixed"):
    """(B, H, W) uint8.  mixed: random 0..255; cell k (row-major over all images) with k % 3 == 1 is constant at a class edge of hir (a sum
    that is an exact multiple of 16), with k % 3 == 2 the same with one label one lower (a sum one below the multiple: the truncation
    decides the class); a permutation of 0..255 at the head of image 0 where it fits; the last image of several all 255."""
    B, H, W = shape
    gen = _gen("labels", shape, kind)
    lab = torch.randint(0, 256, shape, generator=gen).numpy().astype(np.uint8)
    edges = np.array([3, 12, 21, 30, 60, 90, 255, 1], dtype=np.uint8)
    if kind == "all255":
        lab[:] = 255
        return lab
    cells = lab.reshape(B, H // 4, 4, W // 4, 4).transpose(0, 1, 3, 2, 4).reshape(-1, 16).copy()
    k = np.arange(cells.shape[0])
    exact = k % 3 == 1 if kind == "mixed" else np.zeros_like(k, dtype=bool)
    below = k % 3 == 2 if kind == "mixed" else np.ones_like(k, dtype=bool)          # one_below: every cell
    for sel in (exact, below):
        cells[sel] = edges[(k[sel] // 3) % edges.size][:, None]
    cells[below, 5] -= 1
    lab = cells.reshape(B, H // 4, W // 4, 4, 4).transpose(0, 1, 3, 2, 4).reshape(B, H, W).copy()
    if kind == "mixed" and H * W >= 256:
        lab[0].reshape(-1)[:256] = torch.randperm(256, generator=gen).numpy().astype(np.uint8)
    if kind == "mixed" and B > 1:
        lab[-1] = 255
    return lab


def label_prep(height_u8, hir, class_weight):
    """batch form of oracle/loader_oracle.label_prep: (B, H, W) uint8 -> build int64, height_f, weight (B, H, W), height_aggre, weight_aggre
    (B, H/4, W/4), in the C ABI's order of outputs"""
    cw = np.asarray(class_weight, dtype=np.float32)
    rows = [LO.label_prep(np.ascontiguousarray(h), hir, cw) for h in np.asarray(height_u8)]
    hf, ha, b, w, wa = (torch.stack([r[k] for r in rows]) for k in range(5))
    B, H, W = hf.shape
    return b, hf, w, ha.reshape(B, H // 4, W // 4), wa.reshape(B, H // 4, W // 4)


NORM_SHAPES = ((3, 5, 1, 1), (2, 8, 7, 9), (1, 1, 16, 16), (1, 3, 600, 600))
NORM_CLAMPS = ((0.0, 1.0), (-1.0, 1.0), (0.25, 0.75), None)
NORM_GRID_CAP = 4096 * 256                      # normalize_clamp_kernel's grid: at most 4096 workgroups of 256


def norm_bands(C):
    """(mins, ranges) fp32: band 0 the identity (0, 1) -- inputs land on the bounds exactly --, band 1 of range 0, the rest general; a lone
    band is general"""
    gen = _gen("bands", C)
    mins = (torch.rand(C, generator=gen) * 300 - 200).numpy().astype(np.float32)
    ranges = (torch.rand(C, generator=gen) * 2000 + 500).numpy().astype(np.float32)
    if C > 1:
        mins[0], ranges[0] = 0.0, 1.0
        ranges[1] = 0.0
    return mins, ranges


def norm_specials(lo, hi):
    f = np.float32
    inf = f(np.inf)
    v = [f(-0.0), inf, -inf, f(np.nan), f(1e-41), f(-1e-41), f(0.0), f(1.0), f(0.5)]
    for b in (lo, hi):
        v += [f(b), np.nextafter(f(b), inf), np.nextafter(f(b), -inf)]
    return np.array(v, dtype=np.float32)


def norm_inputs(shape, clamp):
    """src (B, C, H, W) fp32: uniform over [-200, 2800) like raw band values, but in band 0 (identity) uniform over [-0.5, 1.5) and in band 1
    (range 0) equal to the band's min in a third of the elements; every 5th element of the head of each band plane, and of the tail of the
    tensor, one of norm_specials (the bounds and one ulp either side of them, -0.0, +-inf, NaN, a subnormal)"""
    B, C, H, W = shape
    gen = _gen("norm", shape, clamp)
    mins, ranges = norm_bands(C)
    x = (torch.rand(shape, generator=gen) * 3000 - 200).numpy().astype(np.float32)
    lo, hi = clamp if clamp else (0.0, 1.0)
    sp = norm_specials(lo, hi)
    if C > 1:
        x[:, 0] = (torch.rand((B, H, W), generator=gen) * 2 - 0.5).numpy()
        third = torch.randint(0, 3, (B, H, W), generator=gen).numpy() == 0
        x[:, 1] = np.where(third, mins[1], x[:, 1])
    planes = x.reshape(B * C, H * W)
    k = min(H * W, 5 * sp.size)
    idx = np.arange(0, k, 5) if H * W > 1 else np.arange(1)
    for p in range(B * C):
        planes[p, idx] = sp[(np.arange(idx.size) + p) % sp.size]
    flat = x.reshape(-1)
    if flat.size > NORM_GRID_CAP:
        flat[-k::5] = sp[: len(flat[-k::5])]
    return x, mins, ranges


def normalize(src, mins, ranges, clamp):
    """batch form of oracle/loader_oracle.normalize (fp32 arithmetic on the CPU: two IEEE operations and the clip by assignment).  The
    oracle takes (mins, maxs) and forms the range itself in fp32: maxs is handed over in float64 so that its range IS `ranges`, checked."""
    mins, ranges = np.asarray(mins, dtype=np.float32), np.asarray(ranges, dtype=np.float32)
    maxs = mins.astype(np.float64) + ranges.astype(np.float64)
    assert np.array_equal((maxs - mins.astype(np.float64)).astype(np.float32).view(np.int32), ranges.view(np.int32))
    dr = tuple(float(v) for v in clamp) if clamp else None
    return torch.stack([LO.normalize(torch.from_numpy(np.ascontiguousarray(s)), mins.astype(np.float64), maxs, dr) for s in np.asarray(src)])


def bits(t):
    """fp32 tensor / array -> int32 numpy view: the sign of zero and the payload of a NaN count"""
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def golden(name):
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name))
