"""GPU: every kernel instantiation the head's host code can select is launched once, and each launch is pinned to ITS form.

The head entry points (srbh_hconv_f32 / _h16, srbh_hconv_entry_h16, srbh_hblock16_eval, srbh_hbwd16) turn run-time flags -- operand type, which
tensors hold 16-bit elements, which epilogue -- into template arguments.  test_gpu_head_walk.py runs 9 of the 28 hconv16_kernel forms, 2 of the 4
hconv_up forms and 3 entry forms; a flag that reaches the wrong template argument in one of the others would pass it.  Here the C entry points
are driven through the ctypes structs of srbh_amd._lib, one launch per form:

  hconv16_kernel<OPT, S16, IO, BS, NIN>   28: 16 plain (operand type x 16-bit source x 16-bit residual x 16-bit output), 4 backward-statistics,
                                              8 narrow-input
  hconv_up_kernel<S16, O16>                4
  hconv_entry_kernel<OPT, O16, S16>        6      hconv_entry64_kernel<O16>  2
  hblock16_kernel<O16>                     2      hbwd16_kernel<BS, MASK>    6
  hconv_f32_kernel<NOB, KS, 1, OPT>       18 (the forms reachable without SRBH_HCONV_RPW), at the walk shape and at a ragged one

Shape (B, H, W) = (3, 8, 128): 12 tiles of 4 x 64 (2 x 2 per image): image, tile row and tile column are all non-trivial; tiles_per_xcd = 2,
the sixth XCD's range is clipped by the tile count and the last two are empty.  The template also runs (2, 6, 72): partial tiles in both
directions, channel counts that leave its vectorised staging.

Each case asserts
  * the path counter of its form (and no other head form);
  * the kernel that ran, from torch.profiler's kernel names (one profiler session per test, the launches in order).  The names carry the template
    arguments ("hconv16_kernel<2, 1, 3, 0, 0>"): they are asserted; should a profiler build report base names only, the base name is asserted;
  * the result against a float64 evaluation of the same rounded operands under the bounds test_gpu_head_walk.py holds that kernel to (TOL_CONV,
    TOL_HBLOCK, TOL_HBWD_DX, check_16, check_sum with its K and caps -- imported, none invented here).

Sharpness.  Outputs are pre-filled with NaN, residuals are not zero, pre-affines are not the identity, masks switch 20 - 80 % of the elements,
fp16 and bf16 operand roundings are 8 x apart.  test_references_tell_neighbouring_forms_apart (no GPU) evaluates the float64 reference of the
neighbouring form wherever the neighbour is arithmetic (other operand type, residual / pre-affine / post-affine / mask dropped, statistics of
the unmasked values) and holds it to > 20 x the bound; a neighbour that reads or writes a tensor with the wrong element size (S16, IO, O16,
NIN), or a weight pack of another layout (NOB, KS), produces garbage or leaves NaN, which no bound lets through.
"""
import ctypes as C
import re

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_head_walk import (TOL_CONV, TOL_HBLOCK, TOL_HBWD_DX, bn_sums, both, chan, check_16, check_f32, check_sum, fold, moments,
                                      pow2, rel, rnd)

gpu = pytest.mark.gpu
DEV = "cuda:0"
SHAPE, RAGGED = (3, 8, 128), (2, 6, 72)
T16 = {1: torch.float16, 2: torch.bfloat16}
SHARP = 20.0                                   # a neighbouring form's reference is at least this many bounds away
DROP = (1, slice(4, 8), slice(64, 128))        # the tile (image 1, tile row 1, tile column 1) the sums' sharpness check removes
HEAD_FORMS = ("hconv16", "hconv_template", "entry_fused", "entry_split", "hconv_up", "hbwd16", "hblock16")


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------------
def dev(t, dtype=None):
    """NCHW host tensor -> NHWC (channels_last) device tensor"""
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous(memory_format=torch.channels_last)


def vec(t):
    return None if t is None else t.float().to(DEV).contiguous()


def nan_out(B, c, h, w, dtype):
    return torch.full((B, c, h, w), float("nan"), dtype=dtype, device=DEV).contiguous(memory_format=torch.channels_last)


def ptr(t):
    return None if t is None else t.data_ptr()


def pack16(w, bf16, perm=None):
    from srbh_amd import _lib
    L = _lib.lib()
    cout, cin, ks, _ = w.shape
    wc = w.float().to(DEV).contiguous()
    if perm is not None:
        wc = wc.index_select(0, perm).contiguous()
    buf = torch.empty(L.srbh_hpack_h16_bytes(cout, cin, ks) // 2, dtype=torch.float16, device=DEV)
    _lib.check(L.srbh_hpack_conv_h16(wc.data_ptr(), cout, cin, ks, 0, int(bf16), buf.data_ptr(), _lib.stream_ptr()), "hpack_conv_h16")
    return buf


def pack32(w):
    from srbh_amd import _lib
    L = _lib.lib()
    cout, cin, ks, _ = w.shape
    wc = w.float().to(DEV).contiguous()
    buf = torch.empty(L.srbh_hpack_bytes(cout, cin, ks) // 4, dtype=torch.float32, device=DEV)
    _lib.check(L.srbh_hpack_conv_f32(wc.data_ptr(), cout, cin, ks, 0, buf.data_ptr(), _lib.stream_ptr()), "hpack_conv_f32")
    return buf


def pad16(b, perm=None):
    if b is None:
        return None
    out = torch.zeros((b.numel() + 15) // 16 * 16, dtype=torch.float32, device=DEV)
    out[:b.numel()] = b.to(DEV) if perm is None else b.to(DEV).index_select(0, perm)
    return out


def stats_buf(c16=16):
    from srbh_amd import _lib
    return torch.full((_lib.lib().srbh_bn_stats_bytes(c16) // 8,), 7.0, dtype=torch.float64, device=DEV)      # (not clean: the call zeroes it)


class kernels_of:
    """with kernels_of("hconv16_kernel") as k: ...launches... ; k.names = the matching device kernels in launch order"""

    def __init__(self, *bases):
        self.bases, self.names = bases, []

    def __enter__(self):
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        self.prof = profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA])
        self.prof.__enter__()
        return self

    def __exit__(self, et, ev, tb):
        torch.cuda.synchronize()
        self.prof.__exit__(et, ev, tb)
        if et is None:
            evs = [e for e in self.prof.events() if any(b + "<" in e.name or e.name.endswith(b) or b + "(" in e.name for b in self.bases)
                   and "hip" not in e.name[:3].lower()]
            evs = [e for e in evs if str(e.device_type).endswith("CUDA")]
            self.names = [e.name for e in sorted(evs, key=lambda e: e.time_range.start)]
        return False


def require(cond, what):
    assert cond, what


def kernel_form(name):
    """'void (anonymous namespace)::hconv16_kernel<2, 1, 3, 0, 0>(HParams)' -> ('hconv16_kernel', (2, 1, 3, 0, 0)); arguments None if absent"""
    m = re.search(r"(\w+_kernel)(?:<([-\d, ]+)>)?", name)
    assert m, name
    return m.group(1), (tuple(int(v) for v in m.group(2).split(",")) if m.group(2) else None)


class Recorder:
    """collects the failures of a test's cases, so that one report names every form that went wrong"""

    def __init__(self):
        self.errs, self.launched = [], []

    def launch(self, case, base, args, counters, fn):
        """fn() launches ONE head kernel; its path counters are asserted here, its kernel name after the profiler session (check_names)"""
        from srbh_amd import _lib
        _lib.path_counters(reset=True)
        out = fn()
        got = _lib.path_counters(reset=True)
        want = {k: counters.get(k, 0) for k in HEAD_FORMS}
        if {k: got[k] for k in HEAD_FORMS} != want:
            self.errs.append(f"{case}: path counters {got}, wanted {want}")
        self.launched.append((case, base, tuple(args)))
        return out

    def check(self, case, fn):
        try:
            fn()
        except (AssertionError, RuntimeError) as e:
            self.errs.append(f"{case}: {type(e).__name__} {str(e)[:400]}")

    def check_names(self, names):
        if len(names) != len(self.launched):
            self.errs.append(f"{len(self.launched)} launches, {len(names)} kernels in the profile: {names}")
            return
        for (case, base, args), name in zip(self.launched, names):
            gb, ga = kernel_form(name)
            if gb != base or (ga is not None and ga[:len(args)] != args):
                self.errs.append(f"{case}: ran {name}, wanted {base}<{', '.join(map(str, args))}>")

    def done(self):
        assert not self.errs, "\n".join(self.errs)


# ---- srbh_hconv_*: one description per case, evaluated on the host (ref) and launched (run) ------------------------------------------------
class Conv:
    """A conv call: host operands (NCHW), the flags, and the float64 / fp32 evaluation of the same rounded operands."""

    def __init__(self, opt, shape, c0, cout, ks=3, c1=0, src16=False, res=None, res16=False, res2=False, out16=False, pre=False, post=False,
                 relu=False, lrelu=False, bias=True, stats=False, bstat=False, ps2=0, seed=1, wmax=0.3):
        B, Hh, Ww = shape
        self.opt, self.shape, self.c0, self.c1, self.cout, self.ks = opt, shape, c0, c1, cout, ks
        self.src16, self.res16, self.out16, self.relu, self.lrelu, self.ps2, self.stats, self.bstat = src16, res16, out16, relu, lrelu, ps2, stats, bstat
        t16 = T16.get(opt)
        self.x0 = rnd((B, c0, Hh, Ww), seed)
        if src16:
            self.x0 = self.x0.to(t16)
        self.x1 = rnd((B, c1, Hh, Ww), seed + 1) if c1 else None
        if c1 and src16:
            self.x1 = self.x1.to(t16)
        self.w = rnd((cout, c0 + c1, ks, ks), seed + 2, -wmax, wmax)
        self.bias = rnd((cout,), seed + 3) if bias else None
        self.pre = (pow2(c0, seed + 4), rnd((c0,), seed + 5, -0.2, 0.2)) if pre else None
        self.post = (rnd((cout,), seed + 6, 0.5, 1.5), rnd((cout,), seed + 7, -0.2, 0.2)) if post else None
        self.res = None
        if res:
            self.res = rnd((B, cout, Hh, Ww), seed + 8)
            if res16:
                self.res = self.res.to(t16)
        self.res2 = rnd((B, cout, Hh, Ww), seed + 9) if res2 else None
        if bstat:
            self.c = rnd((B, 16, Hh, Ww), seed + 10)
            self.mean, self.invstd = rnd((16,), seed + 11, -0.1, 0.1), rnd((16,), seed + 12, 0.5, 1.5)
            self.mask = (rnd((16,), seed + 13, 0.5, 1.5), rnd((16,), seed + 14, -0.2, 0.2))

    def ref(self, dt, opt=None, pre=True, post=True, res=True):
        """the conv of the rounded operands in element type dt; the keyword arguments evaluate a NEIGHBOURING form instead"""
        opt = self.opt if opt is None else opt
        a = self.x0.float()
        if self.pre and pre:
            a = torch.relu(a * chan(self.pre[0]) + chan(self.pre[1]))
        xin = torch.cat([a] + ([self.x1.float()] if self.c1 else []), 1)
        w = self.w
        if opt:
            xin, w = xin.to(T16[opt]), w.to(T16[opt])
        y = F.conv2d(xin.to(dt), w.to(dt), None if self.bias is None else self.bias.to(dt), 1, w.shape[-1] // 2)
        if self.post and post:
            y = y * chan(self.post[0]).to(dt) + chan(self.post[1]).to(dt)
        if self.res is not None and res:
            y = y * 0.5 + self.res.to(dt)
            if self.res2 is not None:
                y = y * 2.0 + self.res2.to(dt)
        if self.lrelu:
            y = torch.where(y >= 0, y, y * 0.2)
        if self.relu:
            y = torch.relu(y)
        return F.pixel_shuffle(y, 2) if self.ps2 else y

    def args(self, keep):
        """the srbh_hconv_args of the call and its output / statistics tensors (`keep` holds every device tensor until the launch is over)"""
        from srbh_amd import _lib
        from srbh_amd import hrfuse as H
        B, Hh, Ww = self.shape
        a = _lib.HConvArgs()
        x0, x1 = dev(self.x0), (dev(self.x1) if self.c1 else None)
        perm = H._up_perm(torch.device(DEV)) if self.ps2 == 2 else None
        w = pack32(self.w) if self.opt == 0 else pack16(self.w, self.opt == 2, perm)
        bias, res, res2 = pad16(self.bias, perm), (dev(self.res) if self.res is not None else None), (dev(self.res2) if self.res2 is not None else None)
        pre, post = [vec(t) for t in self.pre or ()], [pad16(t) for t in self.post or ()]
        a.src0, a.c0, a.src1, a.c1 = ptr(x0), self.c0, ptr(x1), self.c1
        if pre:
            a.pre_scale, a.pre_shift, a.pre_relu = ptr(pre[0]), ptr(pre[1]), 1
        a.w, a.bias, a.cout, a.ksize = ptr(w), ptr(bias), self.cout, self.ks
        a.B, a.H, a.W, a.pixelshuffle2 = B, Hh, Ww, self.ps2
        odt = T16[self.opt] if self.out16 else torch.float32
        out = nan_out(B, self.cout // 4, 2 * Hh, 2 * Ww, odt) if self.ps2 else nan_out(B, self.cout, Hh, Ww, odt)
        a.out = ptr(out)
        if post:
            a.post_scale, a.post_shift = ptr(post[0]), ptr(post[1])
        if res is not None:
            a.res1, a.res1_ld, a.res1_scale = ptr(res), self.cout, 0.5
        if res2 is not None:
            a.res2, a.res2_ld, a.res2_scale = ptr(res2), self.cout, 2.0
        a.post_relu, a.post_lrelu = int(self.relu), int(self.lrelu)
        a.io_h16 = (1 if self.src16 else 0) | (2 if self.c1 and self.src16 else 0) | (4 if self.res is not None and self.res16 else 0) | (8 if self.out16 else 0)
        st = None
        extra = []
        if self.stats or self.bstat:
            st = stats_buf()
            a.stats, a.stats_clean = ptr(st), 0
        if self.bstat:
            extra = [dev(self.c), vec(self.mean), vec(self.invstd), vec(self.mask[0]), vec(self.mask[1])]
            a.bstat_c, a.bstat_mean, a.bstat_invstd, a.bstat_ms, a.bstat_mh = [ptr(t) for t in extra]
        keep.extend([x0, x1, w, bias, res, res2, pre, post, out, st, extra])
        return a, out, st

    def run(self, keep):
        from srbh_amd import _lib
        L = _lib.lib()
        a, out, st = self.args(keep)
        if self.opt == 0:
            _lib.check(L.srbh_hconv_f32(C.byref(a), _lib.stream_ptr()), "hconv_f32")
        else:
            _lib.check(L.srbh_hconv_h16(C.byref(a), int(self.opt == 2), _lib.stream_ptr()), "hconv_h16")
        return out, st

    def check_out(self, name, got, form, cap=4096, th=4, tw=64):
        want, host = both(self.ref)
        if self.out16:
            check_16(name, got, want, host, T16[self.opt], form, "dispatch", cap=cap, th=th, tw=tw)
        else:
            check_f32(name, got, want, TOL_CONV, form, "dispatch", cap=cap, th=th, tw=tw)

    def bstat_sums(self, y, c, dt, masked=True):
        return bn_sums(y, c.to(dt), self.mean.to(dt), self.invstd.to(dt), self.mask if masked else None)


def drop(t):
    b, rows, cols = DROP
    return t[b:b + 1, :, rows, cols]


def hconv16_cases():
    """(name, template arguments <OPT, S16, IO, BS, NIN>, Conv)"""
    out = []
    for opt in (1, 2):
        for s16 in (0, 1):
            for r16 in (0, 1):
                for o16 in (0, 1):          # plain: pre-affine + ReLU, bias, post-affine, residual (fp32 or 16-bit), ReLU
                    out.append((f"plain opt{opt} s{s16} r{r16} o{o16}", (opt, s16, r16 | o16 << 1, 0, 0),
                                Conv(opt, SHAPE, 16, 16, src16=bool(s16), res=True, res16=bool(r16), out16=bool(o16), pre=True, post=True, relu=True,
                                     seed=10 * opt + s16)))
    for s16 in (0, 1):
        for o16 in (0, 1):                  # backward statistics: bf16 operands, the sums of the masked output
            out.append((f"bstat s{s16} o{o16}", (2, s16, o16 << 1, 1, 0), Conv(2, SHAPE, 16, 16, src16=bool(s16), out16=bool(o16), bias=False, bstat=True, seed=40 + s16)))
    for opt in (1, 2):
        for r16 in (0, 1):
            for o16 in (0, 1):              # narrow input: 7 fp32 channels at pixel stride 7 (12 beside a 16-bit tensor: the host wants c0 % 4 == 0 there)
                out.append((f"nin opt{opt} r{r16} o{o16}", (opt, 0, r16 | o16 << 1, 0, 1),
                            Conv(opt, SHAPE, 12 if r16 or o16 else 7, 16, res=True, res16=bool(r16), out16=bool(o16), post=True, relu=True, seed=50 + opt)))
    return out


def template_cases(shape):
    """(name, template arguments <NOB, KS, RPW, OPT>, Conv): two sources, pre-affine, bias, both residuals, LeakyReLU; NOB 4 = the PixelShuffle conv"""
    c0, c1 = (8, 4) if shape == SHAPE else (6, 3)
    out = []
    for opt in (0, 1, 2):
        for nob, cout in ((1, 12), (2, 24), (4, 64)):
            for ks in (3, 1):
                out.append((f"template {shape} opt{opt} nob{nob} ks{ks}", (nob, ks, 1, opt),
                            Conv(opt, shape, c0, cout, ks=ks, c1=c1, pre=True, res=nob != 4, res2=nob != 4, lrelu=True, ps2=int(nob == 4), seed=60 + nob + ks,
                                 wmax=1.0)))          # (weights of the residuals' size: the operand rounding stays visible behind them)
    return out


@gpu
def test_hconv16_all_28_forms():
    cases, keep, R = hconv16_cases(), [], Recorder()
    assert len({c[1] for c in cases}) == 28
    with kernels_of("hconv16_kernel") as k:
        outs = [R.launch(name, "hconv16_kernel", targs, {"hconv16": 1}, lambda cv=cv: cv.run(keep)) for name, targs, cv in cases]
    R.check_names(k.names)
    for (name, targs, cv), (got, st) in zip(cases, outs):
        R.check(name, lambda: cv.check_out(name, got, "hconv16"))
        if cv.bstat:
            def sums():
                w64, h32 = both(cv.ref)
                s64, s32 = cv.bstat_sums(w64, cv.c, torch.float64), cv.bstat_sums(h32, cv.c, torch.float32)
                check_sum(name + " sums", fold(st), s64, s32, s64 - cv.bstat_sums(drop(w64), drop(cv.c), torch.float64), "stats", "dispatch")
            R.check(name + " sums", sums)
    R.done()


@gpu
def test_hconv_up_all_4_forms():
    cases = [(f"up s{s16} o{o16}", (s16, o16), Conv(1, SHAPE, 16, 64, src16=bool(s16), out16=bool(o16), ps2=2, seed=70 + s16)) for s16 in (0, 1) for o16 in (0, 1)]
    keep, R = [], Recorder()
    with kernels_of("hconv_up_kernel") as k:
        outs = [R.launch(name, "hconv_up_kernel", targs, {"hconv_up": 1}, lambda cv=cv: cv.run(keep)) for name, targs, cv in cases]
    R.check_names(k.names)
    for (name, _, cv), (got, _) in zip(cases, outs):
        R.check(name, lambda: cv.check_out(name, got, "hconv_up", th=8, tw=128))
    R.done()


@gpu
@pytest.mark.parametrize("shape", [SHAPE, RAGGED], ids=["walk_shape", "ragged"])
def test_hconv_template_all_18_forms(shape):
    import os
    assert os.environ.get("SRBH_HCONV_RPW", "1") != "2"
    cases, keep, R = template_cases(shape), [], Recorder()
    assert len({c[1] for c in cases}) == 18
    with kernels_of("hconv_f32_kernel") as k:
        outs = [R.launch(name, "hconv_f32_kernel", targs, {"hconv_template": 1}, lambda cv=cv: cv.run(keep)) for name, targs, cv in cases]
    R.check_names(k.names)
    th, tw = (4, 64) if shape == SHAPE else (shape[1], shape[2])        # (ragged: no whole tiles -- one window per image)
    for (name, _, cv), (got, _) in zip(cases, outs):
        R.check(name, lambda: cv.check_out(name, got, "hconv16", th=th * (2 if cv.ps2 else 1), tw=tw * (2 if cv.ps2 else 1)))
    R.done()


# ---- srbh_hconv_entry_h16 -----------------------------------------------------------------------------------------------------------------
def entry_cases():
    """(name, kernel, template arguments, conv1 3x3, downsample 1x1 over the same sources): post-affines, conv1's ReLU, BatchNorm sums of both"""
    out = []
    for opt, s16 in ((1, 0), (2, 0), (1, 1)):
        for o16 in (0, 1):
            mk = lambda ks, post_relu, seed: Conv(opt, SHAPE, 16, 16, ks=ks, c1=16, src16=bool(s16), out16=bool(o16), post=True, relu=post_relu,      # noqa: E731
                                                  stats=True, seed=seed)
            out.append((f"entry opt{opt} s{s16} o{o16}", "hconv_entry_kernel", (opt, o16, s16), mk(3, True, 80 + opt + s16), mk(1, False, 80 + opt + s16)))
    for o16 in (0, 1):
        mk = lambda ks, post_relu: Conv(1, SHAPE, 64, 16, ks=ks, src16=True, out16=bool(o16), post=True, relu=post_relu, stats=True, seed=90)      # noqa: E731
        out.append((f"entry64 o{o16}", "hconv_entry64_kernel", (o16,), mk(3, True), mk(1, False)))
    for _, _, _, c1, ds in out:          # one input: the downsample conv reads conv1's sources (its own weights, bias and post-affine)
        ds.x0, ds.x1 = c1.x0, c1.x1
        ds.w, ds.bias, ds.post = rnd(tuple(ds.w.shape), 97, -0.3, 0.3), rnd((16,), 98), (rnd((16,), 99, 0.5, 1.5), rnd((16,), 100, -0.2, 0.2))
    return out


def run_entry(c1, ds, keep):
    from srbh_amd import _lib
    a1, o1, s1 = c1.args(keep)
    a2, o2, s2 = ds.args(keep)
    a2.src0, a2.src1 = a1.src0, a1.src1
    _lib.check(_lib.lib().srbh_hconv_entry_h16(C.byref(a1), C.byref(a2), int(c1.opt == 2), _lib.stream_ptr()), "hconv_entry_h16")
    return o1, s1, o2, s2


@gpu
def test_hconv_entry_all_8_forms():
    import os
    assert os.environ.get("SRBH_HCONV_ENTRY64", "1") != "0"
    cases, keep, R = entry_cases(), [], Recorder()
    with kernels_of("hconv_entry_kernel", "hconv_entry64_kernel") as k:
        outs = [R.launch(name, base, targs, {"entry_fused": 1}, lambda c1=c1, ds=ds: run_entry(c1, ds, keep)) for name, base, targs, c1, ds in cases]
    R.check_names(k.names)
    for (name, base, _, c1, ds), (o1, s1, o2, s2) in zip(cases, outs):
        cap = 256 if base == "hconv_entry64_kernel" else None
        for tag, cv, got, st in (("conv1", c1, o1, s1), ("downsample", ds, o2, s2)):
            R.check(f"{name} {tag}", lambda: cv.check_out(f"{name} {tag}", got, "entry_fused", cap=cap))

            def sums():
                w64, h32 = both(cv.ref)
                check_sum(f"{name} {tag} sums", fold(st), moments(w64), moments(h32), moments(w64) - moments(drop(w64)), "stats", "dispatch")
            R.check(f"{name} {tag} sums", sums)
    R.done()


# ---- srbh_hblock16_eval -------------------------------------------------------------------------------------------------------------------
class Block:
    def __init__(self, seed=110):
        B, Hh, Ww = SHAPE
        self.x = (rnd((B, 16, Hh, Ww), seed) * 0.7).half()
        self.w1, self.w2 = rnd((16, 16, 3, 3), seed + 1, -0.3, 0.3), rnd((16, 16, 3, 3), seed + 2, -0.3, 0.3)
        self.s1, self.h1 = rnd((16,), seed + 3, 0.5, 1.5), rnd((16,), seed + 4, -0.3, 0.3)
        self.s2, self.h2 = rnd((16,), seed + 5, 0.5, 1.5), rnd((16,), seed + 6, -0.3, 0.3)

    def ref(self, dt, bn1=True, identity=True):
        x = self.x.to(dt)
        a1 = F.conv2d(x, self.w1.half().to(dt), None, 1, 1)
        if bn1:
            a1 = a1 * chan(self.s1).to(dt) + chan(self.h1).to(dt)
        a1 = torch.relu(a1).half().to(dt)
        y = F.conv2d(a1, self.w2.half().to(dt), None, 1, 1) * chan(self.s2).to(dt) + chan(self.h2).to(dt)
        return torch.relu(y + x) if identity else torch.relu(y)

    def run(self, o16, keep):
        from srbh_amd import _lib
        B, Hh, Ww = SHAPE
        a = _lib.HBlock16Args()
        t = [dev(self.x), pack16(self.w1, False), pack16(self.w2, False), vec(self.s1), vec(self.h1), vec(self.s2), vec(self.h2)]
        out = nan_out(B, 16, Hh, Ww, torch.float16 if o16 else torch.float32)
        a.x, a.w1, a.w2, a.scale1, a.shift1, a.scale2, a.shift2 = [ptr(v) for v in t]
        a.out, a.out_h16, a.B, a.H, a.W = ptr(out), o16, B, Hh, Ww
        keep.extend(t + [out])
        _lib.check(_lib.lib().srbh_hblock16_eval(C.byref(a), _lib.stream_ptr()), "hblock16_eval")
        return out


@gpu
def test_hblock16_both_forms():
    blk, keep, R = Block(), [], Recorder()
    with kernels_of("hblock16_kernel") as k:
        outs = [R.launch(f"hblock16 o{o16}", "hblock16_kernel", (o16,), {"hblock16": 1}, lambda o16=o16: blk.run(o16, keep)) for o16 in (0, 1)]
    R.check_names(k.names)
    want, host = both(blk.ref)
    R.check("hblock16 fp32", lambda: check_f32("hblock16 fp32", outs[0], want, TOL_HBLOCK, "hblock16", "dispatch"))
    R.check("hblock16 fp16", lambda: check_16("hblock16 fp16", outs[1], want, host, torch.float16, "hblock16", "dispatch"))
    R.done()


# ---- srbh_hbwd16 --------------------------------------------------------------------------------------------------------------------------
def dgrad64(dc, w, dt):
    """conv^T(dc, W) of the bf16-rounded operands"""
    return F.conv2d(dc.bfloat16().to(dt), w.bfloat16().to(dt).transpose(0, 1).flip(2, 3), None, 1, 1)


def wgrad_of(xin, g, dt):
    return torch.nn.grad.conv2d_weight(xin.bfloat16().to(dt), (16, 16, 3, 3), g.bfloat16().to(dt), padding=1)


def wgrad_tile(xin, g):
    """the float64 contribution of the DROP tile (with its halo: zero outside the image)"""
    b, rows, cols = DROP
    xw = F.pad(xin.bfloat16().double(), (1, 1, 1, 1))[b:b + 1, :, rows.start:rows.stop + 2, cols.start:cols.stop + 2]
    return torch.nn.grad.conv2d_weight(xw, (16, 16, 3, 3), drop(g.bfloat16()).double(), padding=0)


def run_hbwd16(bs, mask):
    """one srbh_hbwd16 launch of form <bs, mask>; returns what the checks need (device results, host operands)"""
    from srbh_amd import _lib
    from srbh_amd import hrfuse as H
    from tests.test_gpu_hbwd16 import _case
    L = _lib.lib()
    B, Hh, Ww = SHAPE
    gy, c, x, mean, invstd, consts, mk, w = _case(B, Hh, Ww, 120 + bs, bool(mask))
    s1, h1 = pow2(16, 131).to(DEV), rnd((16,), 132, -0.2, 0.2).to(DEV)
    m1, i1 = rnd((16,), 133, -0.1, 0.1).to(DEV), rnd((16,), 134, 0.5, 1.5).to(DEV)
    pre = (s1, h1) if bs == 1 else None                       # the conv2 form: conv2's input is relu(bn1(c1)), folded
    res = dev(rnd((B, 16, Hh, Ww), 135) * 1e-3, torch.bfloat16) if bs != 1 else None
    o16 = bs != 0
    a = _lib.HBwd16Args()
    a.g, a.c, a.mean, a.invstd = ptr(gy), ptr(c), ptr(mean), ptr(invstd)
    a.coef, a.k1, a.k2 = [ptr(t) for t in consts]
    if mk is not None:
        a.mask_scale, a.mask_shift = ptr(mk[0]), ptr(mk[1])
    a.x = ptr(x)
    if pre:
        a.pre_scale, a.pre_shift, a.pre_relu = ptr(s1), ptr(h1), 1
    wp = torch.empty(L.srbh_hpack_h16_bytes(16, 16, 3) // 2, dtype=torch.float16, device=DEV)
    _lib.check(L.srbh_hpack_conv_h16(w.contiguous().data_ptr(), 16, 16, 3, 1, 1, wp.data_ptr(), _lib.stream_ptr()), "hpack(T, bf16)")
    a.w, a.B, a.H, a.W = ptr(wp), B, Hh, Ww
    dx = nan_out(B, 16, Hh, Ww, torch.bfloat16 if o16 else torch.float32)
    a.dx, a.dx_b16, a.res = ptr(dx), int(o16), ptr(res)
    st = bc = pattern = active = None
    if bs == 1:                                               # sums for bn1 over conv1's output x, masked by its ReLU
        st, bc = stats_buf(), x
        a.bstat_c, a.bstat_mean, a.bstat_invstd, a.bstat_ms, a.bstat_mh = ptr(x), ptr(m1), ptr(i1), ptr(s1), ptr(h1)
    if bs == 2:                                               # the previous block's closing ReLU as bits, sums for its bn2
        st, bc = stats_buf(), dev(rnd((B, 16, Hh, Ww), 136))
        out_p, pattern = H.bn_add_relu(bc, torch.ones(16, device=DEV), torch.zeros(16, device=DEV), dev(rnd((B, 16, Hh, Ww), 137) * 0.5), want_bits=True)
        active = out_p > 0
        a.bstat_c, a.bstat_mean, a.bstat_invstd, a.relu_bits = ptr(bc), ptr(m1), ptr(i1), ptr(pattern)
    if st is not None:
        a.stats, a.stats_clean = ptr(st), 0
    dw = torch.full((16, 16, 3, 3), float("nan"), dtype=torch.float32, device=DEV)
    ws = torch.empty(L.srbh_hwgrad_ws_bytes(16, 16, 3) // 4, dtype=torch.float32, device=DEV)
    a.dw, a.ws = ptr(dw), ptr(ws)
    # dc as the apply kernel hands it over (bf16), the operand both contractions of the fused pass round to
    dc = H.empty_nhwc(B, 16, Hh, Ww, DEV, torch.bfloat16)
    _lib.check(L.srbh_bn_bwd_apply_io(ptr(gy), ptr(c), ptr(mean), ptr(invstd), a.mask_scale, a.mask_shift, ptr(consts[0]), ptr(consts[1]), ptr(consts[2]),
                                      ptr(dc), B * Hh * Ww, 16, 4 | 1, _lib.stream_ptr()), "apply")
    _lib.check(L.srbh_hbwd16(C.byref(a), _lib.stream_ptr()), "hbwd16")
    torch.cuda.synchronize()
    return dict(bs=bs, mask=mk, dx=dx, dw=dw, st=st, dc=dc.float().cpu(), x=x.cpu(), c=c.cpu(), w=w.cpu(), s1=s1.cpu(), h1=h1.cpu(), m1=m1.cpu(), i1=i1.cpu(),
                res=None if res is None else res.cpu(), bc=None if bc is None else bc.cpu(), active=None if active is None else active.cpu(), keep=(a, wp, ws, pattern))


def hbwd16_refs(r, dt):
    """(dx, the operand x' of the weight gradient) of a run_hbwd16 result in element type dt"""
    xp = torch.relu(r["x"] * chan(r["s1"]) + chan(r["h1"])) if r["bs"] == 1 else r["x"]
    dx = dgrad64(r["dc"], r["w"], dt) + (r["res"].to(dt) if r["res"] is not None else 0)
    if r["bs"] == 2:
        dx = torch.where(r["active"], dx, torch.zeros_like(dx))
    return dx, xp


@gpu
def test_hbwd16_all_6_forms():
    R, runs = Recorder(), []
    with kernels_of("hbwd16_kernel") as k:
        for bs in (0, 1, 2):
            for mask in (0, 1):
                runs.append((f"hbwd16 bs{bs} m{mask}", R.launch(f"hbwd16 bs{bs} m{mask}", "hbwd16_kernel", (bs, mask), {"hbwd16": 1}, lambda: run_hbwd16(bs, mask))))
    R.check_names(k.names)
    for name, r in runs:
        (want, xp), (host, _) = hbwd16_refs(r, torch.float64), hbwd16_refs(r, torch.float32)
        if r["bs"] == 0:
            R.check(name + " dx", lambda: check_f32(name + " dx", r["dx"], want, TOL_HBWD_DX, "hbwd16", "dispatch"))
        else:
            R.check(name + " dx", lambda: check_16(name + " dx", r["dx"], want, host, torch.bfloat16, "hbwd16", "dispatch"))
        if r["mask"] is not None:
            frac = float((r["c"] * chan(r["mask"][0].cpu()) + chan(r["mask"][1].cpu()) <= 0).float().mean())
            R.check(name + " mask", lambda: require(0.2 < frac < 0.8, frac))
        R.check(name + " dw", lambda: check_sum(name + " dw", r["dw"], wgrad_of(xp, r["dc"], torch.float64), wgrad_of(xp, r["dc"], torch.float32),
                                                wgrad_of(xp, r["dc"], torch.float64) - wgrad_tile(xp, r["dc"]), "hbwd16", "dispatch"))
        if r["bs"] == 1:           # over the fp32 values, masked by conv1's ReLU (s1, h1)

            def sums():
                mk = (r["s1"], r["h1"])
                s64 = bn_sums(want, r["bc"].double(), r["m1"].double(), r["i1"].double(), mk)
                s32 = bn_sums(host, r["bc"], r["m1"], r["i1"], mk)
                part = bn_sums(drop(want), drop(r["bc"]).double(), r["m1"].double(), r["i1"].double(), mk)
                check_sum(name + " sums", fold(r["st"]), s64, s32, s64 - part, "stats", "dispatch")
            R.check(name + " sums", sums)
        if r["bs"] == 2:           # over the bf16 values the kernel wrote (what the consumer reads)

            def sums():
                d = r["dx"].cpu()
                s64 = bn_sums(d.double(), r["bc"].double(), r["m1"].double(), r["i1"].double(), None)
                s32 = bn_sums(d.float(), r["bc"], r["m1"], r["i1"], None)
                part = bn_sums(drop(d.double()), drop(r["bc"]).double(), r["m1"].double(), r["i1"].double(), None)
                check_sum(name + " sums", fold(r["st"]), s64, s32, s64 - part, "stats", "dispatch")
            R.check(name + " sums", sums)
            R.check(name + " zeros", lambda: require(float((r["dx"].float() == 0).float().mean()) > 0.2, "the closing ReLU masks nothing"))
    R.done()


# ---- sharpness, on the host ------------------------------------------------------------------------------------------------------------------
def test_references_tell_neighbouring_forms_apart():
    """the float64 reference of the neighbouring form is > SHARP x the bound away (TOL_CONV for the convs: a 16-bit output's step is larger, so
    for those the distance is also held to > SHARP half-steps of the type, 2^-11 / 2^-8 relative)"""
    def far(name, a, b, bound=TOL_CONV):
        d = rel(a, b)
        assert d > SHARP * bound, (name, d)

    for name, targs, cv in hconv16_cases() + template_cases(SHAPE) + template_cases(RAGGED):
        want = cv.ref(torch.float64)
        out_step = 0.0 if not cv.out16 else (2.0 ** -11 if cv.opt == 1 else 2.0 ** -8)
        bound = max(TOL_CONV, out_step)
        if cv.opt and not cv.out16:          # (with a 16-bit output the other operand type also writes the other element type)
            far(name + " other operand type", cv.ref(torch.float64, opt=3 - cv.opt), want)
        if "template" in name:
            far(name + " fp32 <-> 16-bit operands", cv.ref(torch.float64, opt=0 if cv.opt else 1), want)
        if cv.pre:
            far(name + " no pre-affine", cv.ref(torch.float64, pre=False), want, bound)
        if cv.post:
            far(name + " no post-affine", cv.ref(torch.float64, post=False), want, bound)
        if cv.res is not None:
            far(name + " no residual", cv.ref(torch.float64, res=False), want, bound)
        if cv.bstat:
            s = cv.bstat_sums(want, cv.c, torch.float64)
            far(name + " unmasked sums", cv.bstat_sums(want, cv.c, torch.float64, masked=False), s, 1e-4)
            far(name + " plain moments", moments(want), s, 1e-4)
    for name, base, targs, c1, ds in entry_cases():
        for cv in (c1, ds):
            want = cv.ref(torch.float64)
            if not cv.out16:
                far(name + " other operand type", cv.ref(torch.float64, opt=3 - cv.opt), want)
            far(name + " no post-affine", cv.ref(torch.float64, post=False), want, max(TOL_CONV, 2.0 ** -8 if cv.out16 else 0.0))
        far(name + " the two convs", c1.ref(torch.float64), ds.ref(torch.float64), 2.0 ** -8)
    blk = Block()
    far("hblock16 no bn1", blk.ref(torch.float64, bn1=False), blk.ref(torch.float64), 2.0 ** -11)
    far("hblock16 no identity", blk.ref(torch.float64, identity=False), blk.ref(torch.float64), 2.0 ** -11)
    # an fp16 and a bf16 reading of the same 16-bit output differ (the element type follows the operand type)
    y = hconv16_cases()[0][2].ref(torch.float32)
    far("fp16 bits read as bf16", y.half().view(torch.bfloat16).float(), y, 2.0 ** -8)
