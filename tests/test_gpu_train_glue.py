"""The kernels that decide whether training is right -- the loss sums and their gradients, the validation metrics (csrc/srbh_loss.hip),
the Adam update (csrc/srbh_optim.hip) -- and the elementwise glue on the SR trainer's backward path (axpby, LeakyReLU backward, the
adjoint of nearest-x2, the per-channel sums of ACT16 planes, conv_first: csrc/srbh_aux.hip), each entry point on its own through the
C ABI against the float64 functions of tests/train_glue_oracle.py, at the smallest shapes at which each form of its dispatch can still go
wrong: a second grid-stride trip of every capped grid, the fp32 partial's flush in wmse_sum, NCHW / channels_last / padded logits, 2..16
classes, the scalar / vector / vector-with-tail paths of the Adam kernel at every chunk edge, both conv_first kernels with the LDS opt-in
and a ragged last pixel group, and every refusal.  tests/test_train_glue_cpu.py proves by arithmetic that the case tables below reach those
forms, and that the oracle equals float64 autograd / torch.optim.Adam.

Inputs are independent fp32 random tensors (not bf16- or fp16-representable), made on the CPU, never another kernel's output.  Every
output lives in guard-filled storage with slack on both sides, every input is compared with its clone afterwards
(tests/gpu_util.GuardedBuffers); accumulating outputs start from non-zero contents.

Bounds, from the arithmetic of the header's formulas (eps = 2^-24), never from the kernels: |got - want| <= eps * B, B the sum over the
expression's terms of k x |term|, k the fp32 roundings on the term's path (the oracle returns B beside each result):
  wmse_sum        k = 3 + 64: the difference and two products per term, at most 64 fp32 adds before the partial turns double
  wmse_grad       k = 3 on |grad|
  cedice          expf / logf ASSUMED 2 ulp (= 4 eps) each: the toolchain ships no device-math accuracy table.  A softmax value carries
                  (4 + |d_c|) eps of its own exponential (d = z - max, rounded once), the same s-weighted for the sum, C - 1 adds, the
                  reciprocal and the product; nll adds 4 eps |log se|, the rounding of d_y, the difference and the product with w; pb the
                  difference from 1.  The sums accumulate in double: 2^-18 eps (|prior| + sum|term|) for at most 2 048 double atomics.
                  The gradient: both terms' factors (2 and rel(s_0) + 3 roundings) and the final sum; plus an absolute floor of a few
                  2^-126 times the factors: an exponential 88 or more below the maximum is subnormal or zero in fp32, its softmax value
                  and the products behind it carry the absolute error of the format's underflow, not a relative one (the +-80 logits).
  height sums     double throughout: (n + 2) 2^-53 sum|term|; counts, the confusion matrix and the flag are integer-exact
  Adam            first order through g' -> m', v' -> p' (u = eps; every fl() one rounding; beta2, 1 - beta, eps reach the kernel as fp32):
                    g' = fma(wd, p, g)                        dg  <= u (|g| + |wd p|)
                    m' = m + fl(fl(g' - m) (1 - beta1))       dm  <= (1 - beta1) dg + 3u |(1 - beta1)(g' - m)| + u |m'|
                    v' = fma(v, beta2, fl(fl((1-beta2) g') g'))   dv <= 2 (1 - beta2) |g'| dg + 4u v'
                    s = sqrtf(v')                             ds  <= dv / (2 s) + u s
                    den = fl(fl(s isb2) + eps)                dden <= isb2 ds + 3u den
                    r = fl(m' / den)                          dr  <= dm / den + |r| dden / den + u |r|
                    p' = fl(p - fl(fl(lr inv_bc1) r))         dp  <= lr inv_bc1 dr + 2u |upd| + u |p'|
                  The inputs keep v >= 1e-6 g^2 (and no wd with beta2 = 0), so dp stays below 64 eps (|p| + step (|m| + |lerp|) / den):
                  asserted on the CPU.  The rows g = m = v = 0 are bit-exact.
  axpby           bit-exact against fl(fl(a x) + fl(b y)) or against fl(fl(a x) + b y), the same form for every element: the header's
                  formula leaves the contraction of the second product open; no ulp of slack is needed.  0 * inf = NaN is pinned.
  lrelu           bit-exact
  up2_bwd         2 eps sum|term| (three fp32 adds, pairwise)
  act16 sums      k = a thread's terms + 4 shuffle adds + 4 LDS atomics + gridDim.x global atomics, on sum|x|
  conv_first      k = 9 cin fused multiply-adds on |bias| + sum|x||w|; rb / rc bit-equal to ra, out16 the RNE fp16 of ra bit for bit,
                  border, further planes and slack of the ACT16 buffer untouched.  The bf16 plane form of conv_first is not reachable
                  through the C ABI (the trunk's entry selects it): it is left to the trunk's tests (tests/test_gpu_trunk_bf16.py).
Each test prints `TGLUE <entry> <case>: <error / (eps B)> (stock <the fp32 torch chain on the device, same unit>)`; FRAC holds the
fraction of the derived bound an entry is held to.

Measured on an MI355X, error / (eps B), largest over the cases of each entry point (the stock fp32 torch chain on the device beside it):
  srbh_wmse_sum            5.0e-3 (n = 1; the flush case 1.1e-4; stock 1.7e-2)   derived k = 67 was loose by 200 x: held to 4 x = 2.02e-2
  srbh_wmse_grad           0.92 of k = 3   (stock 0.88)
  srbh_cedice_sums         0.34   (stock 0.52)
  srbh_cedice_grad         0.76, at the +-80 logits   (stock 1.41: fp32 autograd misses the bound there)
  srbh_height_metric_sums  n <= 300: exact (inputs on a 1/64 grid: order-independent double sums); n = 131 142, full-mantissa inputs:
                           1.2e-4 (stock, in fp32: 3e5)   loose by 8 400 x (a bound linear in n on double atomics): held to 4 x = 4.8e-4
  srbh_confusion_add       exact
  srbh_adam_step           0.996 in every alignment form (stock 0.996): p' just above a power of two, where the last rounding alone is
                           eps |p'| -- the bound's leading term is attained; derived k stays
  optim.Adam on views      2.7e-2 of 64 eps per step   loose by 38 x: held to 4 x = 0.107
  srbh_axpby_f32           bit-exact; the second product is FUSED into the sum (fl(fl(a x) + b y)) in every case where the forms differ
  srbh_lrelu_bwd_f32       bit-exact (the smallest subnormal counts as > 0)
  srbh_up2_bwd_nhwc_f32    0.94 of 2 eps sum|term|   (stock 1.39: torch's sum takes another order)
  srbh_act16_channel_sum   1.7e-2 (stock 2.9e-2)   loose by 60 x: held to 4 x = 6.7e-2
  srbh_conv_first_f32      0.34 of k = 9 cin   (stock 0.18); rb / rc / out16 / untouched bytes bit-exact
Four derived bounds were loose by more than 10 x and now stand at 4 x the measurement (FRAC below); no bound was widened.  One bound was
wrong as first derived and was corrected before any figure was taken: the CE gradient's lacked the underflow floor above (at the +-80
logits an exponential is subnormal in fp32; the kernel's absolute error there is below 1e-43).

Mutation check (scratch builds of the kernels, never committed; "older" = tests/test_losses_metrics.py, test_gpu_adam.py, test_sr_stage.py):
  wmse_sum's `if (++k == 64)` flush without its add          test_wmse_sum_flush; older files pass
  `i += blockDim.x` in axpby_kernel's grid-stride loop       test_axpby[2097164-dst_is_x / dst_is_y]; older files pass
  `c == 1` for `c == 0` in the Dice gradient term            test_cedice_grad (all 99), test_cedice_out_of_range_label; test_losses_metrics.py
                                                             catches it as well (3 tests)
  the flush skipping a class whose sum d is 0.0 altogether   test_height_metric_sums, every nc >= 3 at n = 200 (one block) and most at 300 /
  (its d^2, |d| and count dropped with it)                   131 142 (8 of 9); older files pass
  1 - beta1 and 1 - beta2 swapped in the scalar path only    test_adam_step (the 4 unaligned forms x the 5 rows with beta1 != beta2),
                                                             test_adam_wrapper_on_unaligned_views; older files pass
  conv_first reading in[p + kx - 1] in a row's last group    test_conv_first (all 180); older files pass
  act16_channel_sum reading the halo row                     test_act16_channel_sum (all 34); test_sr_stage.py catches it as well (6 tests)"""
import functools
import zlib
from collections import namedtuple

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import train_glue_oracle as O
from tests.gpu_util import GuardedBuffers as Buffers
from tests.gpu_util import act16_alloc, act16_raw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = O.EPS32
# the fraction of the derived bound eps * B each entry point is held to: 1.0, or 4 x the largest measured where the derived bound was loose
# by more than 10 x (the 4 x allows for the run-to-run variation of atomic order)
FRAC = dict(wmse_sum=0.0202, wmse_grad=1.0, cedice_sums=1.0, cedice_grad=1.0, height=4.8e-4, adam=1.0, adam_wrapper=0.107, up2=1.0,
            act16_sum=0.067, conv_first=1.0)
MEASURED = dict(wmse_sum=5.03e-3, wmse_grad=0.919, cedice_sums=0.338, cedice_grad=0.758, height=1.19e-4, adam=0.996, adam_wrapper=2.66e-2,
                up2=0.943, act16_sum=1.67e-2, conv_first=0.343)
assert all(FRAC[k] <= 1.0 and (FRAC[k] == 1.0 if MEASURED[k] >= 0.1 else FRAC[k] <= 4.1 * MEASURED[k]) for k in FRAC)
BIG = 2048 * 256 + 70               # work items of one capped loss grid and a ragged rest


def _lib():
    from srbh_amd import _lib as m
    return m, m.lib()


def _p(t):
    return None if t is None else t.data_ptr()


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _ratio(got, want, B):
    """max |got - want| / (eps B); where B == 0 the two must be equal"""
    got, want, B = got.detach().double().cpu(), want.double().cpu(), B.double().cpu()
    err = (got - want).abs()
    B = B.expand_as(err)
    zero = B == 0
    assert bool((err[zero] == 0).all()), "a value whose bound is zero is not exact"
    return float((err[~zero] / (EPS * B[~zero])).max()) if bool((~zero).any()) else 0.0


def _bits_equal(a, b):
    it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def _report(entry, case, err, stock):
    print(f"TGLUE {entry} {case}: {err:.3e} (stock {stock:.3e}; held to {FRAC.get(entry, 0.0):.3e})")


def _refused(rc, bufs, name):
    _, L = _lib()
    assert rc != 0, f"{name}: accepted"
    bufs.verify(written=False)
    assert name.encode() in L.srbh_last_error(), L.srbh_last_error()


def _guard_intact(buf, v):
    lo = (v.data_ptr() - buf.data_ptr()) // buf.element_size()
    return bool(buf[:lo].isnan().all()) and bool(buf[lo + v.numel():].isnan().all())


# ---- srbh_wmse_sum / srbh_wmse_grad ---------------------------------------------------------------------------------------------------------
WMSE_N = (1, 255, 257, 1000, BIG)
WMSE_FLUSH_N = 64 * (2048 * 256) + 2048 * 256 + 70
WMSE_GSCALE = (1.0, -0.37, 0.0)
PRIOR = 3.25
DBL = 2.0 ** -18                    # at most 2 048 double atomics on (|prior| + sum|term|), in units of eps


@functools.lru_cache(maxsize=None)
def wmse_inputs(n):
    gen = _gen("wmse", n)
    return torch.randn(n, generator=gen) * 3, torch.randn(n, generator=gen) * 3 + 0.5, torch.rand(n, generator=gen) * 2 + 0.01


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("n", WMSE_N)
def test_wmse_sum(n, weighted):
    m, L = _lib()
    p, t, w = wmse_inputs(n)
    bufs = Buffers()
    dp, dt = bufs.inp(p), bufs.inp(t)
    dw = bufs.inp(w) if weighted else None
    out = bufs.out((1,), dtype=torch.float64, fill=torch.tensor([PRIOR], dtype=torch.float64))
    m.check(L.srbh_wmse_sum(_p(dp), _p(dt), _p(dw), n, _p(out), m.stream_ptr()), "wmse_sum")
    bufs.verify()
    want, B = O.wmse_sum(p, t, w if weighted else None)
    B += DBL * (PRIOR + B / (3 + O.FLUSH))
    d = dp - dt
    stock = float(((d * d * dw) if weighted else d * d).sum())
    err = abs(float(out) - PRIOR - want) / (EPS * B)
    _report("wmse_sum", (n, weighted), err, abs(stock - want) / (EPS * B))
    assert err <= FRAC["wmse_sum"]


def test_wmse_sum_flush():
    """the only case in which a thread's fp32 partial reaches its 64-term flush: 65 trips of the capped grid and a ragged rest.  Made on
    the device, the float64 oracle evaluated there too (the same functions)"""
    m, L = _lib()
    n = WMSE_FLUSH_N
    gen = torch.Generator(device=DEV).manual_seed(64)
    p = torch.randn(n, generator=gen, device=DEV) * 3
    t = torch.randn(n, generator=gen, device=DEV) * 3 + 0.5
    w = torch.rand(n, generator=gen, device=DEV) * 2 + 0.01
    sums = (float(p.double().sum()), float(t.double().sum()), float(w.double().sum()))
    bufs = Buffers()
    out = bufs.out((1,), dtype=torch.float64, fill=torch.tensor([PRIOR], dtype=torch.float64))
    m.check(L.srbh_wmse_sum(_p(p), _p(t), _p(w), n, _p(out), m.stream_ptr()), "wmse_sum")
    bufs.verify()
    assert sums == (float(p.double().sum()), float(t.double().sum()), float(w.double().sum())), "an input was written"
    want, B = O.wmse_sum(p, t, w)
    B += DBL * (PRIOR + B / (3 + O.FLUSH))
    d = p - t
    stock = float((d * d * w).sum())
    err = abs(float(out) - PRIOR - want) / (EPS * B)
    _report("wmse_sum", (n, "flush"), err, abs(stock - want) / (EPS * B))
    assert err <= FRAC["wmse_sum"]


@pytest.mark.parametrize("gscale", WMSE_GSCALE)
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("n", WMSE_N)
def test_wmse_grad(n, weighted, gscale):
    m, L = _lib()
    p, t, w = wmse_inputs(n)
    bufs = Buffers()
    dp, dt, dg = bufs.inp(p), bufs.inp(t), bufs.inp(torch.tensor([gscale]))
    dw = bufs.inp(w) if weighted else None
    grad = bufs.out((n,))
    m.check(L.srbh_wmse_grad(_p(dp), _p(dt), _p(dw), n, _p(dg), _p(grad), m.stream_ptr()), "wmse_grad")
    bufs.verify()
    want, B = O.wmse_grad(p, t, w if weighted else None, gscale)
    stock = 2 * dg * (dp - dt) * (dw if weighted else 1.0)
    err = _ratio(grad, want, B)
    _report("wmse_grad", (n, weighted, gscale), err, _ratio(stock, want, B))
    assert err <= FRAC["wmse_grad"]


# ---- srbh_cedice_sums / srbh_cedice_grad ------------------------------------------------------------------------------------------------------
CE = namedtuple("CE", "C B HW form weighted labels logits g3")
CE_FORMS = ("nchw", "channels_last", "padded")
CE_SMALL = ((1, 1), (2, 37), (3, 256))
CE_BIG = (2, 2048 * 128 + 35)
CE_G3 = ("ce", "dice_pt", "dice_p", "random")
CE_LOGITS = ("target_200_below", "all_equal", "minus_inf", "pm80")


def ce(C, B, HW, form="nchw", weighted=True, labels="all", logits="randn", g3="random"):
    return CE(C, B, HW, form, weighted, labels, logits, g3)


CE_CASES = ([ce(C, B, HW, form, wt) for C in (2, 3, 7, 16) for B, HW in CE_SMALL for form in CE_FORMS for wt in (True, False)] +
            [ce(7, *CE_BIG, form) for form in CE_FORMS] +
            [ce(7, 2, 37, labels=lb) for lb in ("zero", "nonzero")] + [ce(2, 3, 256, "padded", labels=lb) for lb in ("zero", "nonzero")] +
            [ce(7, 1, 64, form, logits=lg) for lg in CE_LOGITS for form in ("nchw", "padded")])
CE_G3_CASES = [ce(C, 2, 37, form, g3=g) for C in (2, 7) for form in CE_FORMS for g in CE_G3[:3]]       # (CE_CASES all take the random g3)
CE_PRIOR = (3.25, -1.5, 0.75, 2.0)
FILL = 777.0                       # what the gap elements of a padded layout hold


def ce_layout(form, B, C, HW):
    """(elements of the allocation, batch / channel / pixel strides)"""
    if form == "nchw":
        return B * C * HW, C * HW, HW, 1
    if form == "channels_last":
        return B * C * HW, C * HW, 1, C
    cs = 2 * HW + 3
    bs = C * cs + 11
    return B * bs, bs, cs, 2


@functools.lru_cache(maxsize=None)
def ce_inputs(case):
    """logits (B, C, HW), labels (B, HW), weight (B, HW), g3 -- CPU tensors"""
    C, B, HW = case.C, case.B, case.HW
    gen = _gen("ce", C, B, HW, case.labels, case.logits)
    z = torch.randn((B, C, HW), generator=gen) * 2.5
    if case.labels == "zero":
        y = torch.zeros((B, HW), dtype=torch.int64)
    elif case.labels == "nonzero":
        y = torch.randint(1, C, (B, HW), generator=gen)
    else:
        y = torch.randint(0, C, (B, HW), generator=gen)
        if B * HW >= C:
            y.view(-1)[:C] = torch.arange(C)                   # every class is there
        if case.labels == "out_of_range":
            y.view(-1)[C:C + 3] = torch.tensor([-1, C, 100])
    if case.logits == "target_200_below":
        z.scatter_(1, y.unsqueeze(1), -200.0 + torch.rand((B, 1, HW), generator=gen))
    elif case.logits == "all_equal":
        z[:] = 1.7
    elif case.logits == "minus_inf":
        z.scatter_(1, ((y + 1) % C).unsqueeze(1), float("-inf"))
    elif case.logits == "pm80":
        z = (torch.rand((B, C, HW), generator=gen) * 2 - 1) * 80.0
    w = torch.rand((B, HW), generator=gen) * 2 + 0.01
    g3 = {"ce": [1.0, 0.0, 0.0], "dice_pt": [0.0, 1.0, 0.0], "dice_p": [0.0, 0.0, 1.0]}.get(case.g3)
    g3 = torch.tensor(g3) if g3 else torch.randn(3, generator=gen)
    return z, y, w, g3


def _ce_store(case, z):
    total, bs, cs, ps = ce_layout(case.form, case.B, case.C, case.HW)
    store = torch.full((total,), FILL)
    store.as_strided((case.B, case.C, case.HW), (bs, cs, ps)).copy_(z)
    return store, (bs, cs, ps)


def _ce_call_sums(case, C_arg=None):
    m, L = _lib()
    z, y, w, _ = ce_inputs(case)
    store, (bs, cs, ps) = _ce_store(case, z)
    bufs = Buffers()
    dz, dy = bufs.inp(store), bufs.inp(y, dtype=torch.int64)
    dw = bufs.inp(w) if case.weighted else None
    prior = torch.tensor(CE_PRIOR, dtype=torch.float64)
    out_buf, out = Buffers._carve((4,), 0, torch.float64)          # (sum 0 may be NaN on purpose: its guards are checked by hand)
    out.copy_(prior)
    rc = L.srbh_cedice_sums(_p(dz), case.B, case.C if C_arg is None else C_arg, case.HW, bs, cs, ps, _p(dy), _p(dw), _p(out), m.stream_ptr())
    return rc, bufs, out_buf, out, prior, (dz.as_strided((case.B, case.C, case.HW), (bs, cs, ps)), dy, dw)


@pytest.mark.parametrize("case", CE_CASES, ids=lambda c: "-".join(map(str, c)))
def test_cedice_sums(case):
    m, _ = _lib()
    z, y, w, _ = ce_inputs(case)
    rc, bufs, out_buf, out, prior, (vz, dy, dw) = _ce_call_sums(case)
    m.check(rc, "cedice_sums")
    bufs.verify()
    assert _guard_intact(out_buf, out)
    want, B = O.cedice_sums(z, y, w if case.weighted else None)
    B = B + DBL * (prior.abs() + B) * (B > 0)                  # (B >= sum|term| for each of the three)
    assert bool(want.isfinite().all())
    s0 = vz.softmax(1)[:, 0]
    tb = (dy > 0).float()
    cev = F.cross_entropy(vz, dy, reduction="none")
    stock = torch.stack([(cev * dw if dw is not None else cev).sum(), ((1 - s0) * tb).sum(), (1 - s0).sum(), tb.sum()])
    err = _ratio(out.cpu() - prior, want, B)
    _report("cedice_sums", tuple(case), err, float(((stock.double().cpu() - want).abs()[:3] / (EPS * B[:3])).max()))
    assert err <= FRAC["cedice_sums"]


def _ce_call_grad(case, C_arg=None):
    m, L = _lib()
    z, y, w, g3 = ce_inputs(case)
    store, (bs, cs, ps) = _ce_store(case, z)
    bufs = Buffers()
    dz, dy, dg = bufs.inp(store), bufs.inp(y, dtype=torch.int64), bufs.inp(g3)
    dw = bufs.inp(w) if case.weighted else None
    out = bufs.out((store.numel(),), fill=torch.full((store.numel(),), FILL))
    rc = L.srbh_cedice_grad(_p(dz), case.B, case.C if C_arg is None else C_arg, case.HW, bs, cs, ps, _p(dy), _p(dw), _p(dg), _p(out), m.stream_ptr())
    return rc, bufs, out, (bs, cs, ps), (dz, dy, dw, dg)


def _ce_check_grad(case, out, strides):
    z, y, w, g3 = ce_inputs(case)
    shape = (case.B, case.C, case.HW)
    got = out.cpu()
    gap = torch.ones(got.numel(), dtype=torch.bool)
    gap.as_strided(shape, strides).fill_(False)
    assert bool((got[gap] == FILL).all()), "the gradient kernel wrote between the logits"
    want, B = O.cedice_grad(z, y, w if case.weighted else None, g3)
    assert bool(want.isfinite().all())
    return got.as_strided(shape, strides), want, B


@pytest.mark.parametrize("case", CE_CASES + CE_G3_CASES, ids=lambda c: "-".join(map(str, c)))
def test_cedice_grad(case):
    m, _ = _lib()
    rc, bufs, out, strides, (dz, dy, dw, dg) = _ce_call_grad(case)
    m.check(rc, "cedice_grad")
    bufs.verify()
    got, want, B = _ce_check_grad(case, out, strides)
    # stock: fp32 autograd on the device over the scalar g3 . sums
    vz = dz.as_strided((case.B, case.C, case.HW), strides).clone().requires_grad_()
    cev = F.cross_entropy(vz, dy, reduction="none")
    pb, tb = 1 - vz.softmax(1)[:, 0], (dy > 0).float()
    (dg[0] * (cev * dw if dw is not None else cev).sum() + dg[1] * (pb * tb).sum() + dg[2] * pb.sum()).backward()
    err = _ratio(got, want, B)
    _report("cedice_grad", tuple(case), err, _ratio(vz.grad, want, B))
    assert err <= FRAC["cedice_grad"]


CE_OOR = [ce(7, 2, 37, form, labels="out_of_range") for form in CE_FORMS]


@pytest.mark.parametrize("case", CE_OOR, ids=lambda c: c.form)
def test_cedice_out_of_range_label(case):
    """labels -1, C and 100: sum 0 is NaN, sums 1-3 count the pixel by tb = (y > 0) alone; the gradient at such a pixel is the softmax
    with no one-hot class, g0 w s_c + (g1 tb + g2) s_0 (s_c - [c == 0]) -- finite, as include/srbh.h states it"""
    m, _ = _lib()
    z, y, w, _ = ce_inputs(case)
    assert int(((y < 0) | (y >= case.C)).sum()) == 3
    rc, bufs, out_buf, out, prior, _ = _ce_call_sums(case)
    m.check(rc, "cedice_sums")
    bufs.verify()
    assert _guard_intact(out_buf, out)
    want, B = O.cedice_sums(z, y, w)
    got = out.cpu() - prior
    assert bool(got[0].isnan()) and bool(want[0].isnan())
    err = _ratio(got[1:], want[1:], (B + DBL * (prior.abs() + B) * (B > 0))[1:])
    rc, bufs, gout, strides, _ = _ce_call_grad(case)
    m.check(rc, "cedice_grad")
    bufs.verify()
    gg, gw, gB = _ce_check_grad(case, gout, strides)
    gerr = _ratio(gg, gw, gB)
    _report("cedice_sums", tuple(case), err, 0.0)
    _report("cedice_grad", tuple(case), gerr, 0.0)
    assert err <= FRAC["cedice_sums"] and gerr <= FRAC["cedice_grad"]


@pytest.mark.parametrize("C", [1, 17])
def test_cedice_refuses_class_counts(C):
    case = ce(7, 2, 37)
    rc, bufs, out_buf, out, prior, _ = _ce_call_sums(case, C_arg=C)
    assert torch.equal(out.cpu(), prior) and _guard_intact(out_buf, out)
    _refused(rc, bufs, "srbh_cedice_sums")
    rc, bufs, _, _, _ = _ce_call_grad(case, C_arg=C)
    _refused(rc, bufs, "srbh_cedice_grad")


# ---- srbh_height_metric_sums / srbh_confusion_add ---------------------------------------------------------------------------------------------
METRIC_NC = (1, 3, 7, 16)
METRIC_N = (1, 200, 300, 512 * 256 + 70)      # 200: ONE block, where the flush's skip of a class whose sum d is 0.0 is certain to act


@functools.lru_cache(maxsize=None)
def height_inputs(nc, n):
    """pred, ref, cls; for nc >= 3 and n >= 200: class 1 is absent, class nc - 1 has d = +-0.5 in equal numbers (sum d exactly 0 in any
    order), and the values -1 and nc are present.  Up to n = 300 the heights are 13-bit values on a 1/64 grid (neither fp16 nor bf16 holds
    them): every double sum is then exact in ANY order of the atomics, and the test asserts equality -- with full-mantissa inputs the same
    case gave 0 in one run and 7.5e-4 of the bound in the next, by the order of its two blocks' atomics alone"""
    gen = _gen("height", nc, n)
    if n <= 300:
        ref = torch.randint(-4096, 4097, (n,), generator=gen).float() / 64
        pred = ref + torch.randint(-640, 641, (n,), generator=gen).float() / 64
    else:
        ref = torch.randn(n, generator=gen) * 10 + 12
        pred = ref + torch.randn(n, generator=gen) * 3
    if n == 1:
        return pred, ref, torch.zeros(1, dtype=torch.int64)
    cls = torch.randint(-1, nc + 1, (n,), generator=gen)
    cls[:3] = torch.tensor([-1, nc, 0])
    if nc >= 3:
        cls[cls == 1] = 0
        idx = (cls == nc - 1).nonzero().view(-1)
        if idx.numel() % 2:
            cls[idx[-1]] = 0
            idx = idx[:-1]
        ref[idx] = torch.randint(-64, 65, (idx.numel(),), generator=gen).float() / 8
        pred[idx] = ref[idx] + torch.tensor([0.5, -0.5]).repeat(idx.numel() // 2)
    return pred, ref, cls


def _height_call(nc_arg, nc, n):
    m, L = _lib()
    pred, ref, cls = height_inputs(nc, n)
    bufs = Buffers()
    dp, dr, dc = bufs.inp(pred), bufs.inp(ref), bufs.inp(cls, dtype=torch.int64)
    prior = (torch.arange(nc * 4, dtype=torch.float64) + 1).view(nc, 4) * 0.5
    out = bufs.out((nc, 4), dtype=torch.float64, fill=prior)
    rc = L.srbh_height_metric_sums(_p(dp), _p(dr), _p(dc), n, nc_arg, _p(out), m.stream_ptr())
    return rc, bufs, out, prior, (dp, dr, dc)


@pytest.mark.parametrize("n", METRIC_N)
@pytest.mark.parametrize("nc", METRIC_NC)
def test_height_metric_sums(nc, n):
    m, _ = _lib()
    pred, ref, cls = height_inputs(nc, n)
    rc, bufs, out, prior, (dp, dr, dc) = _height_call(nc, nc, n)
    m.check(rc, "height_metric_sums")
    bufs.verify()
    want, B = O.height_sums(pred, ref, cls, nc)
    got = out.cpu() - prior
    assert torch.equal(got[:, 3], want[:, 3]), "counts are integer-exact"
    B = B + DBL * (prior.abs() + B / ((n + 2) * 2.0 ** -53 / EPS)) * (B > 0)          # (B / its factor = sum|term|)
    if nc >= 3 and n >= 200:
        assert want[1, 3] == 0 and torch.equal(out.cpu()[1], prior[1]), "the absent class"
        k = nc - 1
        assert want[k, 3] >= 2 and want[k, 2] == 0 and want[k, 0] == 0.25 * want[k, 3]
        assert float(got[k, 2]) == 0.0 and float(got[k, 0]) == float(want[k, 0]) and float(got[k, 1]) == float(want[k, 1])
    d = dp - dr
    stock = torch.stack([torch.stack([(d[dc == k] ** 2).sum(), d[dc == k].abs().sum(), d[dc == k].sum(), (dc == k).sum().float()]) for k in range(nc)])
    err = _ratio(got, want, B)
    _report("height", (nc, n), err, float(((stock.double().cpu() - want).abs() / (EPS * B).clamp_min(1e-300))[:, :3].max()))
    assert err <= FRAC["height"] and (n > 300 or err == 0.0)


@functools.lru_cache(maxsize=None)
def confusion_inputs(nc, n, clean):
    gen = _gen("confusion", nc, n, clean)
    lo, hi = (0, nc) if clean else (-1, nc + 1)
    pred, label = torch.randint(lo, hi, (n,), generator=gen), torch.randint(lo, hi, (n,), generator=gen)
    if not clean:
        pred[0], label[0] = (nc, 0) if n > 1 else (-1, 0)
        if n > 1:
            pred[1], label[1] = 0, -1
    return pred, label


def _confusion_call(nc_arg, nc, n, clean, flag0):
    m, L = _lib()
    pred, label = confusion_inputs(nc, n, clean)
    bufs = Buffers()
    dp, dl = bufs.inp(pred, dtype=torch.int64), bufs.inp(label, dtype=torch.int64)
    prior = (torch.arange(nc * nc, dtype=torch.int64) * 3 + 1).view(nc, nc)
    cm = bufs.out((nc, nc), dtype=torch.int64, fill=prior)
    flag = bufs.out((1,), dtype=torch.int64, fill=torch.tensor([flag0], dtype=torch.int64))     # an int in the low half of 8 zero bytes
    rc = L.srbh_confusion_add(_p(dp), _p(dl), n, nc_arg, _p(cm), _p(flag), m.stream_ptr())
    return rc, bufs, cm, flag, prior


@pytest.mark.parametrize("flag0", [0, 1])
@pytest.mark.parametrize("clean", [True, False])
@pytest.mark.parametrize("n", METRIC_N)
@pytest.mark.parametrize("nc", METRIC_NC)
def test_confusion_add(nc, n, clean, flag0):
    m, _ = _lib()
    pred, label = confusion_inputs(nc, n, clean)
    rc, bufs, cm, flag, prior = _confusion_call(nc, nc, n, clean, flag0)
    m.check(rc, "confusion_add")
    bufs.verify()
    want, bad = O.confusion(pred, label, nc)
    assert bad == (0 if clean else 1)
    assert torch.equal(cm.cpu() - prior, want)
    assert flag.cpu().view(torch.int32).tolist() == [max(bad, flag0), 0]
    print(f"TGLUE confusion {(nc, n, clean, flag0)}: exact")


@pytest.mark.parametrize("nc", [0, 17])
def test_metrics_refuse_class_counts(nc):
    rc, bufs, _, _, _ = _height_call(nc, 16, 300)
    _refused(rc, bufs, "srbh_height_metric_sums")
    rc, bufs, _, _, _ = _confusion_call(nc, 16, 300, True, 0)
    _refused(rc, bufs, "srbh_confusion_add")


# ---- srbh_adam_step -----------------------------------------------------------------------------------------------------------------------
ADAM_SIZES = (1, 3, 4, 5, 4095, 4096, 4097, 8192, 12289)
ADAM_NULL_AT, ADAM_EMPTY_AT = 4, 7          # table positions of the entry without a gradient and of the entry with n = 0
ADAM_FORMS = ("aligned", "p", "g", "m", "v")                 # which of the four arrays sits one float past a 16-byte boundary
HP = namedtuple("HP", "wd t beta1 beta2")
ADAM_HP = (HP(0.0, 1, 0.9, 0.999), HP(1e-4, 2, 0.9, 0.999), HP(1e-4, 1000, 0.9, 0.999), HP(0.0, 100000, 0.9, 0.999), HP(1e-4, 1, 0.9, 0.999),
           HP(0.0, 2, 0.0, 0.0))
ADAM_LR = (1e-3, 2.5e-4)
ADAM_EPS = 1e-8
ADAM_SCALES = (1e-3, 1.0, 1e3, 0.1, 30.0)
EDGE = 8                                     # rows [0, 8): g = m = v = 0;  rows [8, 16): v = 0, g != 0 -- in every tensor of >= 4095 elements


def adam_table_sizes():
    """the n of every table entry, the skipped ones included"""
    sizes = list(ADAM_SIZES)
    sizes.insert(ADAM_NULL_AT, 100)
    sizes.insert(ADAM_EMPTY_AT, 0)
    return sizes


@functools.lru_cache(maxsize=None)
def adam_inputs(hp):
    """per table entry (p, g, m, v, lr): g's scale runs from 1e-3 to 1e3 over the tensors, v >= 0.25 scale^2 >= 1e-6 g^2"""
    rows = []
    for i, n in enumerate(adam_table_sizes()):
        gen = _gen("adam", i, n)
        sc = ADAM_SCALES[i % len(ADAM_SCALES)]
        nn_ = max(n, 4)                                        # (the n = 0 entry still points at real memory)
        p = torch.randn(nn_, generator=gen)
        g = torch.randn(nn_, generator=gen) * sc
        mm = torch.randn(nn_, generator=gen) * sc * 0.5
        v = ((0.5 + torch.rand(nn_, generator=gen)) * sc) ** 2
        if n >= 4095:
            g[:EDGE], mm[:2 * EDGE], v[:2 * EDGE] = 0.0, 0.0, 0.0
            g[EDGE:2 * EDGE] = sc * (1 + torch.rand(EDGE, generator=gen)) * torch.tensor([1.0, -1.0]).repeat(EDGE // 2)
        rows.append((p, g, mm, v, ADAM_LR[i % 2]))
    return rows


def _adam_run(form, hp, order=None, nchunks=None, beta1=None, eps=None):
    """one launch over the whole table.  Returns (rc, buffers, [(p, m, v) device views], chunk list)"""
    m, L = _lib()
    from srbh_amd.optim import _ENTRY
    assert L.srbh_adam_chunk() == O.ADAM_CHUNK
    sizes = adam_table_sizes()
    bufs = Buffers()
    tab = np.zeros(len(sizes), dtype=_ENTRY)
    dev = []
    off = {k: int(form == k) for k in "pgmv"}
    for i, (n, (p, g, mm, v, lr)) in enumerate(zip(sizes, adam_inputs(hp))):
        dp, dm, dv = (bufs.out(t.shape, off[k], fill=t) for k, t in (("p", p), ("m", mm), ("v", v)))
        dg = None if i == ADAM_NULL_AT else bufs.inp(g, off["g"])
        dev.append((dp, dm, dv))
        tab[i] = (_p(dp), _p(dg) or 0, _p(dm), _p(dv), n, lr, hp.wd, 1.0 / (1.0 - hp.beta1 ** hp.t), 1.0 / np.sqrt(1.0 - hp.beta2 ** hp.t))
    chunks = O.adam_chunks(sizes) + [(ADAM_EMPTY_AT, 0)]
    if order is not None:
        chunks = [chunks[j] for j in order]
    dtab = bufs.inp(torch.from_numpy(tab.view(np.uint8).copy()), dtype=torch.uint8)
    dch = torch.tensor(chunks, dtype=torch.int32, device=DEV).reshape(-1)
    rc = L.srbh_adam_step(_p(dtab), _p(dch), len(chunks) if nchunks is None else nchunks, hp.beta1 if beta1 is None else beta1, hp.beta2,
                          ADAM_EPS if eps is None else eps, m.stream_ptr())
    return rc, bufs, dev, tab


@pytest.mark.parametrize("hp", ADAM_HP, ids=lambda h: "-".join(map(str, h)))
@pytest.mark.parametrize("form", ADAM_FORMS)
def test_adam_step(form, hp):
    m, _ = _lib()
    rc, bufs, dev, tab = _adam_run(form, hp)
    m.check(rc, "adam_step")
    bufs.verify()
    worst = stock_worst = 0.0
    for i, (n, (p, g, mm, v, lr)) in enumerate(zip(adam_table_sizes(), adam_inputs(hp))):
        dp, dm, dv = (t.cpu() for t in dev[i])
        if i in (ADAM_NULL_AT, ADAM_EMPTY_AT):
            assert _bits_equal(dp, p) and _bits_equal(dm, mm) and _bits_equal(dv, v), "a skipped entry was touched"
            continue
        assert O.adam_path([tab[i][k] for k in "pgmv"], n) == ("scalar" if form != "aligned" else ("vector+tail" if n % 4 else "vector"))
        assert all(_bits_equal(a[n:], b[n:]) for a, b in ((dp, p), (dm, mm), (dv, v))), "a write past the tensor's n elements"
        dp, dm, dv, p, g, mm, v = (t[:n] for t in (dp, dm, dv, p, g, mm, v))
        p1, m1, v1, bp, bm, bv, _ = O.adam(p, g, mm, v, lr, hp.wd, tab[i]["inv_bc1"], tab[i]["inv_sqrt_bc2"], hp.beta1, hp.beta2, ADAM_EPS)
        worst = max(worst, _ratio(dp, p1, bp), _ratio(dm, m1, bm), _ratio(dv, v1, bv))
        if n >= 4095:
            if hp.wd == 0:
                assert _bits_equal(dp[:EDGE], p[:EDGE]) and bool((dm[:EDGE] == 0).all()) and bool((dv[:EDGE] == 0).all()), "g = m = v = 0 moved p"
        # stock: the same chain in fp32 torch on the device
        sp, sg, sm, sv = (t.to(DEV) for t in (p, g, mm, v))
        sg = sg + hp.wd * sp
        sm = sm + (sg - sm) * (1 - hp.beta1)
        sv = sv * hp.beta2 + (1 - hp.beta2) * sg * sg
        sp = sp - (lr * float(tab[i]["inv_bc1"])) * (sm / (sv.sqrt() * float(tab[i]["inv_sqrt_bc2"]) + ADAM_EPS))
        stock_worst = max(stock_worst, _ratio(sp, p1, bp), _ratio(sm, m1, bm), _ratio(sv, v1, bv))
    _report("adam", (form,) + tuple(hp), worst, stock_worst)
    assert worst <= FRAC["adam"]


def test_adam_chunk_order_does_not_matter():
    hp = ADAM_HP[1]
    n = len(O.adam_chunks(adam_table_sizes())) + 1
    order = torch.randperm(n, generator=_gen("order")).tolist()
    assert order != sorted(order)
    rc0, b0, dev0, _ = _adam_run("aligned", hp)
    rc1, b1, dev1, _ = _adam_run("aligned", hp, order=order)
    assert rc0 == 0 and rc1 == 0
    b0.verify()
    b1.verify()
    for a, b in zip(dev0, dev1):
        assert all(_bits_equal(x.cpu(), y.cpu()) for x, y in zip(a, b))


@pytest.mark.parametrize("what", ["nchunks", "beta1", "eps"])
def test_adam_refusals(what):
    kw = dict(nchunks=dict(nchunks=0), beta1=dict(beta1=1.0), eps=dict(eps=-1e-8))[what]
    rc, bufs, _, _ = _adam_run("aligned", ADAM_HP[0], **kw)
    _refused(rc, bufs, "srbh_adam_step")


WRAP = ((1, (5,)), (7, (17, 241)), (4107, (33,)))        # (offset in floats, shape): views of one flat buffer, no offset a multiple of 4
WRAP_LR, WRAP_WD, WRAP_STEPS = 1e-3, 1e-4, 3


def test_adam_wrapper_on_unaligned_views():
    """srbh_amd.optim.Adam over contiguous views of one flat buffer at odd offsets -- the way the kernel's scalar path is reached in
    practice -- 3 steps against float64 torch.optim.Adam on copies.  Bound: 64 eps per step on |p| + the sum of the reference's updates"""
    from srbh_amd.optim import Adam
    gen = _gen("wrap")
    flat = torch.randn(4107 + 33 + 4, generator=gen).to(DEV)
    ps = [torch.nn.Parameter(flat[o:o + int(np.prod(s))].view(s)) for o, s in WRAP]
    assert all(p.is_contiguous() and p.data_ptr() % 16 != 0 for p in ps)
    ref = [torch.nn.Parameter(p.detach().cpu().double().clone()) for p in ps]
    opt, ropt = Adam(ps, lr=WRAP_LR, weight_decay=WRAP_WD), torch.optim.Adam(ref, lr=WRAP_LR, weight_decay=WRAP_WD)
    moved = [torch.zeros_like(r) for r in ref]
    gsum = [torch.zeros_like(r) for r in ref]                   # sum over the steps of |(1 - beta1) g'|: what exp_avg's terms add up to at most
    for step in range(WRAP_STEPS):
        for i, (p, r) in enumerate(zip(ps, ref)):
            g = torch.randn(p.shape, generator=gen) * ADAM_SCALES[(i + step) % 3]
            p.grad, r.grad = g.to(DEV), g.double()
        before = [r.detach().clone() for r in ref]
        gsum = [gs + 0.1 * (r.grad + WRAP_WD * b).abs() for gs, r, b in zip(gsum, ref, before)]
        opt.step()
        ropt.step()
        moved = [mv + (r.detach() - b).abs() for mv, r, b in zip(moved, ref, before)]
    worst = max(_ratio(p, r.detach(), 64 * WRAP_STEPS * (r.detach().abs() + mv)) for p, r, mv in zip(ps, ref, moved))
    for p, r, gs in zip(ps, ref, gsum):
        st, rst = opt.state[p], ropt.state[r]
        worst = max(worst, _ratio(st["exp_avg"], rst["exp_avg"], 64 * WRAP_STEPS * gs),
                    _ratio(st["exp_avg_sq"], rst["exp_avg_sq"], 64 * WRAP_STEPS * rst["exp_avg_sq"].abs().clamp_min(1e-30)))
    _report("adam_wrapper", WRAP, worst, 0.0)
    assert worst <= FRAC["adam_wrapper"]


# ---- srbh_axpby_f32 / srbh_lrelu_bwd_f32 ---------------------------------------------------------------------------------------------------------
AXPBY_N = (4, 1020, 4 * (2048 * 256) + 12)
LRELU_N = (4, 1020, 4 * (4096 * 256) + 12)
AXPBY_MODES = ("plain", "y_null", "dst_is_x", "dst_is_y", "a0_nonfinite_x", "b0_nonfinite_y")
SPECIALS = (0.0, -0.0, 2.0 ** -149, -1.5, -(2.0 ** -149), 3.0)


@functools.lru_cache(maxsize=None)
def eltwise_inputs(n):
    gen = _gen("eltwise", n)
    return torch.randn(n, generator=gen) * 3, torch.randn(n, generator=gen) * 5 + 1


@pytest.mark.parametrize("mode", AXPBY_MODES)
@pytest.mark.parametrize("n", AXPBY_N)
def test_axpby(n, mode):
    m, L = _lib()
    x, y = eltwise_inputs(n)
    a, b = 0.7310585975646973 + 2 ** -20, -1.3
    if "nonfinite" in mode:
        x, y = x.clone(), y.clone()
        t = x if mode[0] == "a" else y
        t[:3] = torch.tensor([float("inf"), float("-inf"), float("nan")])
        t[-3:] = torch.tensor([float("nan"), float("inf"), float("-inf")])       # (n = 4: element 3 and elements 1, 2 again)
        a, b = (0.0, b) if mode[0] == "a" else (a, 0.0)
    bufs = Buffers()
    if mode == "dst_is_x":
        dx = dst = bufs.out((n,), fill=x)
        dy = bufs.inp(y)
    elif mode == "dst_is_y":
        dy = dst = bufs.out((n,), fill=y)
        dx = bufs.inp(x)
    else:
        dx, dy = bufs.inp(x), None if mode == "y_null" else bufs.inp(y)
        dst_buf, dst = Buffers._carve((n,), 0)                  # (NaN results on purpose in two modes: guards checked by hand)
    if "nonfinite" in mode:                                    # (an input that holds a NaN is compared by its bits: NaN != NaN)
        held = [(v, c) for v, c in bufs.inputs if bool(c.isnan().any())]
        bufs.inputs = [(v, c) for v, c in bufs.inputs if not bool(c.isnan().any())]
        assert len(held) == 1
    m.check(L.srbh_axpby_f32(_p(dst), a, _p(dx), b, _p(dy), n, m.stream_ptr()), "axpby")
    bufs.verify()
    if "nonfinite" in mode:
        assert _bits_equal(*held[0]), "an input was written"
    if not mode.startswith("dst_is"):
        assert _guard_intact(dst_buf, dst)
    sep, fused = O.axpby(a, x, b, None if mode == "y_null" else y)
    got = dst.cpu()
    nan = sep.isnan()
    assert torch.equal(got.isnan(), nan) and int(nan.sum()) == ((4 if n == 4 else 6) if "nonfinite" in mode else 0), "0 * inf, 0 * nan are NaN (IEEE)"
    got, sep, fused = (torch.where(nan, torch.zeros_like(t), t) for t in (got, sep, fused))
    is_sep, is_fused = _bits_equal(got, sep), _bits_equal(got, fused)
    print(f"TGLUE axpby {(n, mode)}: bit-exact, second product {'fused' if is_fused and not is_sep else 'rounded' if is_sep and not is_fused else 'either'}")
    assert is_sep or is_fused


@pytest.mark.parametrize("slope", [0.2, 0.0])
@pytest.mark.parametrize("n", LRELU_N)
def test_lrelu_bwd(n, slope):
    m, L = _lib()
    g, y = eltwise_inputs(n)
    y = y.clone()
    y[:len(SPECIALS)][:n] = torch.tensor(SPECIALS)[:n]
    if n > 1020:
        y[-len(SPECIALS):] = torch.tensor(SPECIALS)               # (also in the second grid-stride trip)
    bufs = Buffers()
    dg, dy = bufs.out((n,), fill=g), bufs.inp(y)
    m.check(L.srbh_lrelu_bwd_f32(_p(dg), _p(dy), slope, n, m.stream_ptr()), "lrelu_bwd")
    bufs.verify()
    assert _bits_equal(dg.cpu(), O.lrelu_bwd(g, y, slope))
    print(f"TGLUE lrelu_bwd {(n, slope)}: bit-exact")


@pytest.mark.parametrize("n", [3, 1022])
def test_eltwise_refuse_ragged_n(n):
    m, L = _lib()
    x, y = eltwise_inputs(1024)
    bufs = Buffers()
    dx, dy, dst = bufs.inp(x), bufs.inp(y), bufs.out((1024,))
    _refused(L.srbh_axpby_f32(_p(dst), 1.0, _p(dx), 1.0, _p(dy), n, m.stream_ptr()), bufs, "srbh_axpby_f32")
    bufs = Buffers()
    dg, dy = bufs.out((1024,), fill=x), bufs.inp(y)
    _refused(L.srbh_lrelu_bwd_f32(_p(dg), _p(dy), 0.2, n, m.stream_ptr()), bufs, "srbh_lrelu_bwd_f32")


# ---- srbh_up2_bwd_nhwc_f32 ---------------------------------------------------------------------------------------------------------------------
UP2_CASES = ((1, 1, 1, 4), (2, 3, 5, 8), (1, 7, 2, 64), (3, 5, 3, 12), (1, 513, 512, 16))


@pytest.mark.parametrize("case", UP2_CASES, ids=lambda c: "x".join(map(str, c)))
def test_up2_bwd(case):
    m, L = _lib()
    B, Ho, Wo, C = case
    g = torch.randn((B, 2 * Ho, 2 * Wo, C), generator=_gen("up2", case)) * 2
    bufs = Buffers()
    dg, out = bufs.inp(g), bufs.out((B, Ho, Wo, C))
    m.check(L.srbh_up2_bwd_nhwc_f32(_p(dg), _p(out), B, Ho, Wo, C, m.stream_ptr()), "up2_bwd")
    bufs.verify()
    want, Bd = O.up2_bwd(g)
    stock = dg.view(B, Ho, 2, Wo, 2, C).sum((2, 4))
    err = _ratio(out, want, Bd)
    _report("up2", case, err, _ratio(stock, want, Bd))
    assert err <= FRAC["up2"]


def test_up2_bwd_refuses_ragged_channels():
    m, L = _lib()
    bufs = Buffers()
    dg, out = bufs.inp(torch.randn(1, 4, 4, 6)), bufs.out((1, 2, 2, 6))
    _refused(L.srbh_up2_bwd_nhwc_f32(_p(dg), _p(out), 1, 2, 2, 6, m.stream_ptr()), bufs, "srbh_up2_bwd_nhwc_f32")


# ---- srbh_act16_channel_sum ----------------------------------------------------------------------------------------------------------------------
CSUM_PLANES = ((1, 0, 1), (6, 0, 1), (6, 2, 3), (6, 5, 1))         # (chunks_total, chunk0, nchunk)
CSUM_SHAPES = ((1, 1, 1), (1, 7, 9), (2, 8, 8), (3, 5, 43))
CSUM_BIG = (1, 512, 513)
CSUM_CASES = [(bf, pl, sh) for bf in (0, 1) for pl in CSUM_PLANES for sh in CSUM_SHAPES] + [(bf, (1, 0, 1), CSUM_BIG) for bf in (0, 1)]
HALO = 3.0e4                        # what the halo pixels and the planes outside the range hold (finite in fp16)


def _csum_call(bf, planes, shape, chunk0=None):
    m, L = _lib()
    ct, c0, nc = planes
    B, H, W = shape
    dt = torch.bfloat16 if bf else torch.float16
    buf = act16_alloc(B, ct, H, W, DEV)
    raw = act16_raw(buf, B, ct, H, W, dt)
    raw.fill_(HALO)
    vals = (torch.randn((B, nc, H, W, 32), generator=_gen("csum", bf, planes, shape)) * 4 + 0.3).to(dt)      # (the CPU's RNE conversion)
    raw[:, c0:c0 + nc, 1:-1, 1:-1] = vals.to(DEV)             # a same-type copy: the stored 16-bit values are exactly `vals`
    keep = buf.clone()
    bufs = Buffers()
    out = bufs.out((nc * 32,), fill=torch.full((nc * 32,), 1.0e9))
    rc = L.srbh_act16_channel_sum(_p(buf), B, H, W, ct, c0 if chunk0 is None else chunk0, nc, bf, _p(out), m.stream_ptr())
    return rc, bufs, out, buf, keep, raw


@pytest.mark.parametrize("case", CSUM_CASES, ids=lambda c: f"{'bf16' if c[0] else 'fp16'}-{c[1]}-{c[2]}".replace(" ", ""))
def test_act16_channel_sum(case):
    m, _ = _lib()
    bf, planes, shape = case
    rc, bufs, out, buf, keep, raw = _csum_call(*case)
    m.check(rc, "act16_channel_sum")
    bufs.verify()
    assert torch.equal(buf, keep), "the planes were written"
    want, mag = O.act16_channel_sum(raw.cpu(), planes[1], planes[2])
    Bd = O.act16_sum_roundings(*shape) * mag
    stock = raw[:, planes[1]:planes[1] + planes[2], 1:-1, 1:-1].float().sum((0, 2, 3)).reshape(-1)
    err = _ratio(out, want, Bd)
    _report("act16_sum", case, err, _ratio(stock, want, Bd))
    assert err <= FRAC["act16_sum"]


def test_act16_channel_sum_refuses_plane_range():
    rc, bufs, _, _, _, _ = _csum_call(0, (6, 2, 3), (1, 7, 9), chunk0=4)
    _refused(rc, bufs, "srbh_act16_channel_sum")


# ---- srbh_conv_first_f32 -------------------------------------------------------------------------------------------------------------------------
CF_CIN = (1, 3, 4, 12, 48, 56)
CF_HW = ((1, 1), (2, 3), (5, 4), (3, 5), (4, 9), (2, 6))          # W % 4 = 1, 3, 0, 1, 1, 2: (2, 6) is there for the residue 2
CF_OUTS = ("ra", "ra_rb_rc", "out16_2", "out16_6", "all")       # all: ra + rb + rc + out16 with 2 planes
CF = namedtuple("CF", "cin H W B bias outs")
CF_CASES = [CF(cin, H, W, (1, 3)[(i + j + k) % 2], (i + k) % 2 == 0, outs)
            for i, cin in enumerate(CF_CIN) for j, (H, W) in enumerate(CF_HW) for k, outs in enumerate(CF_OUTS)]


@functools.lru_cache(maxsize=None)
def cf_inputs(cin, H, W, B):
    gen = _gen("cf", cin, H, W, B)
    return (torch.randn((B, cin, H, W), generator=gen) * 2, torch.randn((64, cin, 3, 3), generator=gen) * (0.5 / cin ** 0.5),
            torch.randn(64, generator=gen))


def _cf_call(case, cin_arg=None, ct_arg=None):
    m, L = _lib()
    x, w, bias = cf_inputs(case.cin, case.H, case.W, case.B)
    B, H, W = case.B, case.H, case.W
    bufs = Buffers()
    dx, dw = bufs.inp(x), bufs.inp(w)
    db = bufs.inp(bias) if case.bias else None
    ra = rb = rc = o16 = pattern = None
    ct = 0
    if case.outs in ("ra", "ra_rb_rc", "all") or ct_arg is not None:
        ra = bufs.out((B, H, W, 64))
    if case.outs in ("ra_rb_rc", "all"):
        rb, rc = bufs.out((B, H, W, 64)), bufs.out((B, H, W, 64))
    if case.outs in ("out16_2", "out16_6", "all") or ct_arg is not None:
        ct = 6 if case.outs == "out16_6" else 2
        o16 = act16_alloc(B, ct, H, W, DEV)
        pattern = ((torch.arange(o16.numel(), dtype=torch.int64) * 37 + 11) % 251).to(torch.uint8).to(DEV)
        o16.copy_(pattern)
    rc_ = L.srbh_conv_first_f32(_p(dx), _p(dw), _p(db), B, case.cin if cin_arg is None else cin_arg, H, W, _p(ra), _p(rb), _p(rc), _p(o16),
                                ct if ct_arg is None else ct_arg, m.stream_ptr())
    return rc_, bufs, (ra, rb, rc, o16, pattern, ct), (dx, dw, db)


@pytest.mark.parametrize("case", CF_CASES, ids=lambda c: "-".join(map(str, c)))
def test_conv_first(case):
    m, _ = _lib()
    x, w, bias = cf_inputs(case.cin, case.H, case.W, case.B)
    B, H, W = case.B, case.H, case.W
    rc_, bufs, (ra, rb, rc, o16, pattern, ct), (dx, dw, db) = _cf_call(case)
    m.check(rc_, "conv_first")
    bufs.verify()
    want, Bd = O.conv_first(x, w, bias if case.bias else None)
    stock = F.conv2d(dx, dw, db, 1, 1).permute(0, 2, 3, 1)
    if ra is None:                                           # out16 alone: the fp32 values come from a second call on the same inputs
        rc2, bufs2, (ra, _, _, _, _, _), _ = _cf_call(case._replace(outs="ra"))
        m.check(rc2, "conv_first")
        bufs2.verify()
    err = _ratio(ra, want, Bd)
    _report("conv_first", tuple(case), err, _ratio(stock, want, Bd))
    assert err <= FRAC["conv_first"]
    if rb is not None:
        assert _bits_equal(rb.cpu(), ra.cpu()) and _bits_equal(rc.cpu(), ra.cpu())
    if o16 is not None:
        expect = pattern.clone()
        half = ra.half().view(B, H, W, 2, 32).permute(0, 3, 1, 2, 4)            # torch's RNE conversion of the fp32 values this call wrote
        act16_raw(expect, B, ct, H, W, torch.float16)[:, :2, 1:-1, 1:-1] = half
        assert torch.equal(o16, expect), "out16: not the RNE fp16 of ra, or a write to the border / a further plane / the slack"


def test_conv_first_refusals():
    case = CF(3, 2, 3, 1, True, "all")
    rc_, bufs, (_, _, _, o16, pattern, _), _ = _cf_call(case._replace(cin=56), cin_arg=57)
    assert torch.equal(o16, pattern)
    _refused(rc_, bufs, "srbh_conv_first_f32")
    rc_, bufs, (_, _, _, o16, pattern, _), _ = _cf_call(case, ct_arg=1)
    assert torch.equal(o16, pattern)
    _refused(rc_, bufs, "srbh_conv_first_f32")


def test_no_error_pending():
    torch.cuda.synchronize()
    assert float(torch.ones(8, device=DEV).sum()) == 8.0
