"""float64 restatement of the kernels that decide whether training is right (csrc/srbh_loss.hip, csrc/srbh_optim.hip) and of the
elementwise glue on the SR trainer's backward path (csrc/srbh_aux.hip)  --  TEST INFRASTRUCTURE ONLY.

One plain torch function per entry point, evaluated in float64 on the device its inputs live on (the CPU, except for the one case that
is too large to move), each written from the contract in include/srbh.h and the reference formulas it cites, not from the kernels.
Every function returns its result together with B, the first-order bound of an fp32 evaluation of the header's formula in units of
eps = 2^-24: the sum over the expression's terms of (fp32 roundings on the term's path) x |term|.  tests/test_gpu_train_glue.py asserts
|got - want| <= eps * B; tests/test_train_glue_cpu.py pins this file against float64 autograd, torch.optim.Adam and oracle/loss_oracle.py.
Below the functions: the dispatch arithmetic of those entry points restated as plain constants and small functions (grid caps, trips of a
capped grid, the Adam kernel's path, conv_first's form), so that the GPU case tables can be held to the forms they were chosen for.
No device code here."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

EPS32 = 2.0 ** -24           # unit roundoff of fp32
ULP_EXP = ULP_LOG = 2        # expf / logf: ASSUMED 2 ulp each (no device-math accuracy table ships with the toolchain); 1 ulp = 2 eps
TINY = 2.0 ** -126 / EPS32   # the smallest normal fp32 in units of eps: below it a result carries an ABSOLUTE error of up to this much (gradual
#                              underflow or a flush to zero alike), whatever its relative bound says -- an exponential 88 or more below the maximum


def _d(t):
    return t.detach().to(torch.float64)


def _f32(x):
    """a Python float as the fp32 value the C ABI (or the Adam table) carries"""
    return float(torch.tensor(x, dtype=torch.float32))


# ---- losses and metrics ---------------------------------------------------------------------------------------------------------------
def wmse_sum(p, t, w=None):
    """srbh_wmse_sum: sum_i w_i (p_i - t_i)^2.  Returns (sum, B): per term 3 roundings (the difference, two products) and at most
    FLUSH fp32 adds before the partial turns double"""
    d = _d(p) - _d(t)
    term = d * d if w is None else _d(w) * d * d
    return float(term.sum()), float((3 + FLUSH) * term.abs().sum())


def wmse_grad(p, t, w, gscale):
    """srbh_wmse_grad: grad_i = gscale * 2 w_i (p_i - t_i).  Returns (grad, B): one product chain, 3 roundings"""
    g = 2.0 * _f32(gscale) * (_d(p) - _d(t))
    if w is not None:
        g = g * _d(w)
    return g, 3 * g.abs()


def _softmax_parts(z):
    """z (B, C, HW) -> log-softmax, softmax, d = z - max, log(sum exp d), all float64"""
    z = _d(z)
    d = z - z.max(1, keepdim=True).values
    lse = torch.log(torch.exp(d).sum(1, keepdim=True))
    ls = d - lse
    return ls, torch.exp(ls), d, lse


def _rel_softmax(C, s, d):
    """per class, the relative error of an fp32 softmax value in eps: its own expf and the rounding of its argument (|d| eps), the
    sum's (the s-weighted mean of the same, C - 1 adds), the reciprocal and the product"""
    own = _own(d)
    return own + (s * own).sum(1, keepdim=True) + (C - 1) + 2


def _own(d):
    """an exponential's own relative error in eps: expf's ULP_EXP ulp and the rounding of its argument; a class at -inf has the exact
    softmax value 0 and carries none"""
    return 2 * ULP_EXP + torch.where(d.isfinite(), d.abs(), torch.zeros_like(d))


def cedice_sums(z, y, w=None):
    """srbh_cedice_sums: [sum w nll, sum pb tb, sum pb, sum tb] with nll = -log softmax_y, pb = 1 - s_0, tb = (y > 0); a label outside
    [0, C) makes sum 0 NaN and counts in the others by tb alone.  z (B, C, HW), y (B, HW) int64, w (B, HW) or None.
    Returns (sums[4], B[4]); the accumulation itself is double, so B is the sum of the per-pixel bounds"""
    Bn, C, HW = z.shape
    ls, s, d, lse = _softmax_parts(z)
    ok = (y >= 0) & (y < C)
    yc = y.clamp(0, C - 1).unsqueeze(1)
    nll = -ls.gather(1, yc).squeeze(1)
    dy = d.gather(1, yc).squeeze(1)
    wt = torch.ones_like(nll) if w is None else _d(w)
    nll_sum = (wt * nll).sum() if bool(ok.all()) else torch.tensor(float("nan"), dtype=torch.float64, device=z.device)
    tb = (y > 0).to(torch.float64)
    s0 = s[:, 0]
    pb = 1.0 - s0
    sums = torch.stack([nll_sum, (pb * tb).sum(), pb.sum(), tb.sum()])
    # nll = logf(se) - d_y: se's relative error moves log(se) absolutely; logf's own ULP_LOG ulp; d_y's rounding; the difference; times w
    rel_se = (s * _own(d)).sum(1) + (C - 1)
    lse = lse.squeeze(1)
    b_nll = wt.abs() * (rel_se + 2 * ULP_LOG * lse.abs() + dy.abs() + 2 * nll.abs())
    b_pb = s0 * _rel_softmax(C, s, d)[:, 0] + pb.abs()
    return sums, torch.stack([b_nll.sum(), (b_pb * tb).sum(), b_pb.sum(), torch.zeros_like(nll_sum)])


def cedice_grad(z, y, w, g3):
    """srbh_cedice_grad: dlogits = g3[0] d(sum w nll) + g3[1] d(sum pb tb) + g3[2] d(sum pb):
        dz_c = g0 w (s_c - [c == y]) + (g1 tb + g2) s_0 (s_c - [c == 0]).
    A label outside [0, C) has no one-hot class (the pinned behaviour, include/srbh.h): its CE term is g0 w s_c, its tb is (y > 0).
    Returns (dz (B, C, HW), B)"""
    Bn, C, HW = z.shape
    _, s, d, _ = _softmax_parts(z)
    g0, g1, g2 = (_f32(float(v)) for v in g3)
    cls = torch.arange(C, device=z.device).view(1, C, 1)
    oh = (cls == y.unsqueeze(1)).to(torch.float64)
    o0 = (cls == 0).to(torch.float64)
    wt = (torch.ones(y.shape, dtype=torch.float64, device=z.device) if w is None else _d(w)).unsqueeze(1)
    tb = (y > 0).to(torch.float64).unsqueeze(1)
    s0 = s[:, :1]
    gd = (g1 * tb + g2) * s0
    a, b = g0 * wt * (s - oh), gd * (s - o0)
    rel = _rel_softmax(C, s, d)
    ba = (g0 * wt).abs() * (s * rel + (s - oh).abs()) + 2 * a.abs()
    bb = gd.abs() * (s * rel + (s - o0).abs()) + (rel[:, :1] + 3) * b.abs()
    # every softmax value (its exponential, its product) and every product behind it may underflow: an absolute floor
    floor = 2 * TINY * ((g0 * wt).abs() + gd.abs() + (g1 * tb + g2).abs() + 3)
    return a + b, ba + bb + (a + b).abs() + floor


def height_sums(p, r, cls, num_class):
    """srbh_height_metric_sums: per class k [sum d^2, sum |d|, sum d, count], d = p - r over cls == k; other values of cls are skipped.
    Returns (out (num_class, 4), B): the kernel is double throughout, so B = (n + 2) 2^-53 sum|term| in units of eps"""
    d = (_d(p) - _d(r)).reshape(-1)
    cls = cls.reshape(-1)
    out = torch.zeros(num_class, 4, dtype=torch.float64)
    mag = torch.zeros(num_class, 4, dtype=torch.float64)
    for k in range(num_class):
        dk = d[cls == k]
        out[k] = torch.stack([(dk * dk).sum(), dk.abs().sum(), dk.sum(), torch.tensor(float(dk.numel()), dtype=torch.float64)])
        mag[k] = torch.stack([(dk * dk).sum(), dk.abs().sum(), dk.abs().sum(), torch.tensor(0.0, dtype=torch.float64)])
    return out, mag * ((d.numel() + 2) * 2.0 ** -53 / EPS32)


def confusion(pred, label, num_class):
    """srbh_confusion_add: cm[label][pred] += 1 over the pairs with both values in [0, num_class).  Returns (cm int64, bad flag)"""
    pred, label = pred.reshape(-1), label.reshape(-1)
    ok = (pred >= 0) & (pred < num_class) & (label >= 0) & (label < num_class)
    cm = torch.zeros(num_class * num_class, dtype=torch.int64)
    cm.index_add_(0, label[ok] * num_class + pred[ok], torch.ones(int(ok.sum()), dtype=torch.int64))
    return cm.view(num_class, num_class), int(not bool(ok.all()))


# ---- Adam -----------------------------------------------------------------------------------------------------------------------------
def adam(p, g, m, v, lr, wd, inv_bc1, inv_sqrt_bc2, beta1, beta2, eps, table_f32=True):
    """srbh_adam_step on one tensor: g += wd p; m = lerp(m, g, 1 - beta1); v = beta2 v + (1 - beta2) g^2;
    p -= lr inv_bc1 m / (sqrt(v) inv_sqrt_bc2 + eps).  beta, 1 - beta and eps are the doubles the caller passes; lr, wd, inv_bc1 and
    inv_sqrt_bc2 the fp32 table values (table_f32 = False: as given, to compare with float64 torch.optim.Adam).  Returns (p', m', v', Bp, Bm, Bv, M): the B's by first-order propagation g' -> m', v' -> p'
    (derivation: the docstring of tests/test_gpu_train_glue.py), M = |p| + step (|m| + (1 - beta1) |g' - m|) / denom"""
    p, g, m, v = _d(p), _d(g), _d(m), _d(v)
    lr, wd, inv_bc1, isb2 = (_f32(x) if table_f32 else float(x) for x in (lr, wd, inv_bc1, inv_sqrt_bc2))
    omb1, omb2 = 1.0 - beta1, 1.0 - beta2
    g1 = g + wd * p
    bg = g.abs() + (wd * p).abs()                                              # one fused rounding
    lerp = omb1 * (g1 - m)
    m1 = m + lerp
    bm = omb1 * bg + 3 * lerp.abs() + m1.abs()                                  # difference, (1 - beta1) as fp32, product; the sum
    q = omb2 * g1 * g1
    v1 = beta2 * v + q
    bv = 2 * omb2 * g1.abs() * bg + 4 * v1                                      # (1 - beta2), beta2 as fp32, two products, the fused sum
    s = torch.sqrt(v1)
    bs = torch.where(v1 > 0, bv / (2 * s.clamp_min(1e-300)), torch.zeros_like(s)) + s
    den = s * isb2 + eps
    bden = isb2 * bs + 3 * den                                                  # product, eps as fp32, sum
    r = m1 / den
    br = bm / den + r.abs() * bden / den + r.abs()
    step = lr * inv_bc1
    upd = step * r
    p1 = p - upd
    bp = step * br + 2 * upd.abs() + p1.abs()                                   # lr inv_bc1, the product; the difference
    M = p.abs() + step * (m.abs() + lerp.abs()) / den
    return p1, m1, v1, bp, bm, bv, M


# ---- SR glue --------------------------------------------------------------------------------------------------------------------------
def axpby(a, x, b, y):
    """srbh_axpby_f32: dst = a x + b y in fp32.  The header's formula leaves one choice open, whether b y is rounded before the sum or
    fused into it, so both fp32 results are returned (float32 tensors): (separate, fused).  y None: fl(a x), both the same.
    IEEE: 0 * inf and 0 * nan are NaN, so a == 0 does NOT clear a non-finite x (nor b == 0 a non-finite y)"""
    a, b = _f32(a), _f32(b)
    ax = (a * _d(x)).float()                  # (24 x 24 bits: the double product is exact, one rounding)
    if y is None:
        return ax, ax
    by = b * _d(y)
    return (ax.double() + by.float().double()).float(), (ax.double() + by).float()


def lrelu_bwd(g, y, slope):
    """srbh_lrelu_bwd_f32: g * (y > 0 ? 1 : slope) from the saved OUTPUT y, as fp32 (one exact product, one rounding).  +0, -0 and
    negative y take the slope; the smallest positive subnormal is > 0"""
    mul = torch.where(y > 0, torch.ones((), dtype=torch.float64), torch.tensor(_f32(slope), dtype=torch.float64))
    return (_d(g) * mul).float()


def up2_bwd(g):
    """srbh_up2_bwd_nhwc_f32: g [B][2Ho][2Wo][C] -> the sum of each 2 x 2 block [B][Ho][Wo][C].  Returns (out, B = 2 sum|term|)"""
    g = _d(g)
    Bn, H2, W2, C = g.shape
    blk = g.view(Bn, H2 // 2, 2, W2 // 2, 2, C)
    return blk.sum((2, 4)), 2 * blk.abs().sum((2, 4))


def act16_channel_sum(raw, chunk0, nchunk):
    """srbh_act16_channel_sum: raw [B][chunks][H+2][W+2][32] of fp16 / bf16 (the stored values, halo included) -> per-channel sums over
    the INTERIOR of planes chunk0 .. chunk0 + nchunk.  Returns (sums [nchunk * 32], sum|x|)"""
    x = _d(raw[:, chunk0:chunk0 + nchunk, 1:-1, 1:-1])
    return x.sum((0, 2, 3)).reshape(-1), x.abs().sum((0, 2, 3)).reshape(-1)


def act16_sum_roundings(B, H, W):
    """fp32 adds on a channel's path: a thread's terms, 4 shuffle adds, 4 LDS atomics, one global atomic per block"""
    npix = B * H * W
    gx = grid(npix, CAP_CSUM)
    return math.ceil(npix / (gx * 64)) + 4 + 4 + gx


def conv_first(x, w, bias):
    """srbh_conv_first_f32: 3x3 pad-1 conv with bias, NCHW in, NHWC [B][H][W][64] out.  Returns (out, B): cin * 9 fused
    multiply-adds on top of the bias, each bounded by the sum of the absolute terms"""
    b = None if bias is None else _d(bias)
    out = F.conv2d(_d(x), _d(w), b, 1, 1)
    mag = F.conv2d(_d(x).abs(), _d(w).abs(), None if b is None else b.abs(), 1, 1)
    return out.permute(0, 2, 3, 1).contiguous(), (9 * x.shape[1]) * mag.permute(0, 2, 3, 1).contiguous()


# ---- the dispatch facts the case tables rely on ---------------------------------------------------------------------------------------
BLOCK = 256
CAP_LOSS, CAP_METRIC = 2048, 512        # grid_for; the height sums and the confusion matrix
CAP_AXPBY, CAP_ELT4, CAP_CSUM = 2048, 4096, 1024     # axpby; lrelu / up2 (float4 items); channel sum (blocks of 64 pixels x 4 octets)
ADAM_CHUNK = 4096
FLUSH = 64                              # wmse_sum turns its fp32 partial double every 64 terms
MAXC = 16
CONV_FIRST_MAX_CIN = 56
LDS_DEFAULT = 65536                     # dynamic LDS above this needs the opt-in attribute


def grid(items, cap, block=BLOCK):
    return max(1, min(cap, (items + block - 1) // block))


def trips(items, cap, block=BLOCK):
    """grid-stride trips of the busiest thread"""
    return math.ceil(items / (grid(items, cap, block) * block))


def wmse_flushes(n):
    return trips(n, CAP_LOSS) // FLUSH


def adam_path(ptrs, n):
    """the form the Adam kernel takes on a tensor: "scalar" when any of p / g / m / v is off a 16-byte boundary, else "vector", with a
    scalar tail when n % 4 != 0"""
    if any(int(a) % 16 for a in ptrs):
        return "scalar"
    return "vector+tail" if n % 4 else "vector"


def adam_chunks(sizes):
    """the (tensor, slice) list of a table"""
    return [(i, s) for i, n in enumerate(sizes) for s in range((n + ADAM_CHUNK - 1) // ADAM_CHUNK)]


def conv_first_form(cin):
    """(kernel, dynamic LDS bytes, opt-in needed) -- None for a refused cin"""
    if not 1 <= cin <= CONV_FIRST_MAX_CIN:
        return None
    lds = cin * 9 * 64 * 4
    return ("cin3" if cin == 3 else "runtime", lds, lds > LDS_DEFAULT)


def conv_first_ragged(W):
    """pixels of a row's last 4-pixel group that lie past the row's end"""
    return (4 - W % 4) % 4
