"""GPU: the head kernels' persistent tile walk with MORE than one tile per workgroup, held to kernel tolerance.

hconv16_kernel, hconv_up_kernel, both hconv_entry kernels, hblock16_kernel, hwgrad16_kernel and hbwd16_kernel share one walk (4 x 64 tiles, a
contiguous run of ceil(ntiles / 8) tiles per XCD, workgroup j of an XCD takes tiles j, j + per_xcd, ...; next tile -- or next two -- in flight
while one is multiplied; weight-gradient / BatchNorm sums kept per lane over the walk).  Their small-shape tests run one tile per workgroup, the
whole-model tests walk but at fp16-operand tolerances (1e-3 .. 3e-2).  Here:

  shape A = (60, 12, 320): 900 tiles, 113 per XCD (109 in the last): 1 and 2 tiles per workgroup at either cap;
  shape B = (161, 12, 320): 2 415 tiles, 302 per XCD (301 in the last): 3 and 4 at cap 768, 4 and 5 at cap 512.

15 tiles per image (5 columns x 3 rows): a workgroup's successive tiles change tile column, tile row and image, XCD runs begin mid-image and
mid-row.  Every case first asserts -- from the cap the library reports (srbh_head_wgs_cap) -- the tiles-per-workgroup counts it is meant to
produce, and from srbh_path_counters that the intended kernel form ran; an environment knob that changes either makes the case FAIL.

Reference: float64 on the host of the same operation on the same rounded operands (rounded where the kernel rounds).  Pre-affines use
power-of-two scales: x * scale is exact, so the kernel's fused multiply-add and torch's mul-then-add round alike.
  * fp32 outputs: rel-L2 of the whole tensor AND of the worst 4 x 64 tile <= the kernel's small-shape bound (5e-6 head convs, 2e-5 hblock16,
    1e-5 hbwd16 dx); the message of a failing tile names XCD, workgroup and trip.
  * 16-bit outputs: against the float64 result rounded once: every element equal or one step of the type away, at most 2 % differ (whole
    tensor and per tile); the host's own fp32 evaluation must differ in <= 0.5 % and never by more than a step.  "One step" is the type's
    spacing at max(|want|, |got|, rms(want)): an element that cancels to near zero still carries the fp32 summation error of its rms-sized
    partial sums (~1e-7 rms), which spans several of the tiny spacings down there -- the host's fp32 conv against float64 is up to 7 (fp16)
    and 25 (bf16) spacings-at-the-value off at these shapes, and never more than one spacing-at-rms.
  * sums over pixels (weight gradients, forward and backward BatchNorm sums): floor = rel-L2(host fp32 evaluation, float64) of the same
    formula; bound = min(K * floor, the kernel's small-shape bound), K the smallest of 2 / 4 / 8 that holds on an MI355X for every case with a
    factor 1.5 to spare (the convention of test_gpu_trunk_parity.py); and the bound is SHARP: <= 0.1 x what one dropped interior tile moves
    the float64 result (from host values alone).

Measured on an MI355X (both shapes; A and B agree to the digits shown unless two values are given):
  fp32 outputs, whole tensor / worst tile: hconv16 forward forms 6.7 .. 7.8e-8 / 7.1e-8 .. 1.1e-7 (narrow outputs included), data-gradient
    forms 5.4 .. 5.7e-8 / 5.9 .. 6.3e-8, narrow inputs 0.95 .. 3.7e-8 / 1.5 .. 4.1e-8; hconv_up 7.3e-8 / 7.7e-8; entry kernels 4.2e-8 .. 1.7e-7 /
    4.4e-8 .. 1.8e-7 (bound 5e-6 for all of these); hbwd16 conv1 dx 6.8e-8 / 7.4e-8 (1e-5); hblock16 2.0e-6 (A), 1.8e-6 (B) / 1.86e-5 (2e-5) --
    its worst tile is one where the float64 graph rounds a few elements of the fp16 intermediate a1 the other way; the host's own fp32
    evaluation of the block is 1.80e-5 off on ITS worst tile, so that margin belongs to the reference, not to the walk.
  16-bit outputs, share of differing elements (host fp32 vs float64 in brackets), never more than one step: hconv16 fp16 residual + output
    2.3e-4 (4.8e-4), bf16 data gradient 3.7 .. 4.0e-5 (5.3e-5); hbwd16 conv2 dx 4.5e-5 (5.9e-5), conv1_bits dx 3.4 .. 3.7e-5 (6.1e-5); hblock16
    fp16 3.6e-4 (6.2e-4); hconv_up fp16 4.7e-4 (9.9e-4); worst tile 5.6e-3 (hblock16), else <= 2.2e-3.
  sums, got / floor = ratio:  forward BatchNorm sums of hconv16 3.2e-9 / 1.0e-7 (A), 2.0e-7 (B) = 0.03, 0.02; of the entry kernels
    0.7 .. 1.8e-9 / 0.9 .. 1.3e-7 = 0.01 .. 0.02;  backward sums of hconv16 (bstat) 8.4e-8 / 1.8e-7, 2.8e-7 = 0.46, 0.30; of hbwd16 conv2
    4.1e-8 / 9.3e-8 = 0.44 (A), 5.8e-8 / 7.8e-8 = 0.75 (B); of hbwd16 conv1_bits 1.3e-8 / 4.9e-8 = 0.26, 1.1e-8 / 5.3e-8 = 0.21;
    hwgrad16 (three forms) 1.2 .. 1.4e-7 / 0.8 .. 1.2e-6 = 0.11 .. 0.16 (A), / 1.4 .. 2.2e-6 = 0.06 .. 0.09 (B);  hbwd16 dw, conv2 form
    8.0e-8 / 2.0e-7 = 0.39, 7.4e-8 / 2.5e-7 = 0.30, conv1 forms 1.5e-7 / 4.2e-7 = 0.36, 1.8e-7 / 6.9e-7 = 0.26.
  The largest ratio is 0.75, so K = 2 (2 / 0.75 = 2.7 >= 1.5) for every kind of sum; K * floor is then 1.0e-7 .. 4.4e-6, at most 0.001 of what the
  dropped tile moves the float64 result (4.2e-4 for the forward sums at B .. 3.6e-2 for a weight gradient at A).  No case failed: no defect found.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = {"A": (60, 12, 320), "B": (161, 12, 320)}
DEFAULT_CAP = {"hconv16": 768, "entry_fused": 768, "wgrad16": 768, "hconv_up": 768, "hbwd16": 512, "hblock16": 512}
COUNTS = {("A", 768): {1, 2}, ("A", 512): {1, 2}, ("B", 768): {3, 4}, ("B", 512): {4, 5}}
ENTRY64_WGS = 256                # the whole-row entry kernel: 32 workgroups per XCD (include/srbh.h, srbh_head_wgs_cap)
TOL_CONV, TOL_HBLOCK, TOL_HBWD_DX = 5e-6, 2e-5, 1e-5         # the kernels' small-shape bounds (test_gpu_head_f16 / _hblock16 / _hbwd16)
CAP_SUM = {"wgrad16": 5e-6, "hbwd16": 1e-4, "stats": 1e-4}   # small-shape bounds of the sums: K * floor may not exceed them
K_SUM = {"wgrad16": 2, "hbwd16": 2, "stats": 2}              # chosen from the MI355X ratios in the docstring
DROP = (1, 2)                    # the interior tile (tile row, tile column) whose contribution the sharpness check removes (image B // 2)


# ---- the walk ---------------------------------------------------------------------------------------------------------------------------
def ntiles_of(key):
    B, Hh, Ww = SHAPES[key]
    return B * (Hh // 4) * (Ww // 64)


def walk_geometry(ntiles, cap, at_least_one=False):
    """(tiles per XCD, workgroups per XCD) of the launch code: per_xcd = min(ceil(ntiles / 8), cap / 8)"""
    per = (ntiles + 7) // 8
    wgs = cap // 8 if cap >= 8 else (1 if at_least_one else 0)
    return per, min(per, wgs)


def walk_counts(ntiles, cap, at_least_one=False):
    """the set of tiles-per-workgroup counts of a walk over `ntiles` tiles under workgroup cap `cap`"""
    per, wgs = walk_geometry(ntiles, cap, at_least_one)
    counts = set()
    for xcd in range(8):
        n = max(0, min(per, ntiles - xcd * per))
        counts.update(len(range(j, n, wgs)) for j in range(wgs))
    return counts


def tile_owner(t, ntiles, cap):
    """tile index -> 'XCD x, workgroup j, trip k' of the walk"""
    per, wgs = walk_geometry(ntiles, cap, True)
    xcd, r = divmod(t, per)
    return f"XCD {xcd}, workgroup {r % wgs} of it, trip {r // wgs}"


def test_walk_counts_helper_on_the_documented_shapes():
    assert ntiles_of("A") == 900 and ntiles_of("B") == 2415
    for (key, cap), want in COUNTS.items():
        assert walk_counts(ntiles_of(key), cap) == want, (key, cap)
    assert walk_counts(900, 256) == {3, 4}                       # the whole-row entry kernel at A
    # one tile per workgroup: the 512-tile hblock16 case of test_gpu_hblock16.py, and any cap above the tile count (idle workgroups in the last XCD)
    assert walk_counts(512, 512) == {1} and walk_counts(900, 4096) == {0, 1} and walk_counts(2415, 4096) == {0, 1}
    # shape A at cap 768: workgroups 0..16 of an XCD walk two tiles, the rest one
    assert [len(range(j, 113, 96)) for j in (0, 16, 17, 95)] == [2, 2, 1, 1]


def walk_cap(form, key):
    """the cap in effect for `form`; asserts that the walk over shape `key` gives the tiles-per-workgroup counts the case is written for"""
    from srbh_amd import _lib
    cap = _lib.head_wgs_cap(form)
    got = walk_counts(ntiles_of(key), cap, form == "hblock16")
    assert got == COUNTS[(key, DEFAULT_CAP[form])], f"{form} at shape {key}: cap {cap} gives {sorted(got)} tiles per workgroup"
    return cap


class ran:
    """with ran(hconv16=1): ... -- exactly these head forms were launched inside the block (and nothing went to the template unless named)"""

    def __init__(self, **forms):
        self.forms = dict(forms)
        self.forms.setdefault("hconv_template", 0)

    def __enter__(self):
        from srbh_amd import _lib
        _lib.path_counters(reset=True)
        return self

    def __exit__(self, et, ev, tb):
        from srbh_amd import _lib
        c = _lib.path_counters(reset=True)
        if et is None:
            for k, v in self.forms.items():
                assert c[k] == v, (k, v, c)
        return False


# ---- operands -----------------------------------------------------------------------------------------------------------------------------
def rnd(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


def pow2(n, seed):
    return 2.0 ** torch.randint(-1, 2, (n,), generator=torch.Generator().manual_seed(seed)).float()


@functools.lru_cache(maxsize=None)
def act(key, seed, c=16, scale=1.0):
    """a (B, c, H, W) uniform(-scale, scale) fp32 host tensor of shape `key` (shared between cases, never written)"""
    B, Hh, Ww = SHAPES[key]
    return rnd((B, c, Hh, Ww), seed) * scale


def nhwc(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def conv_of(cin, cout, ks=3, bias=True, seed=3):
    conv = torch.nn.Conv2d(cin, cout, ks, 1, ks // 2, bias=bias)
    with torch.no_grad():
        conv.weight.copy_(rnd(tuple(conv.weight.shape), seed, -0.3, 0.3))
        if bias:
            conv.bias.copy_(rnd((cout,), seed + 1))
    return conv


def chan(v):
    return v.view(1, -1, 1, 1)


def drop_window(key):
    """(image, rows, cols) of the dropped interior tile"""
    B, _, _ = SHAPES[key]
    return B // 2, slice(DROP[0] * 4, DROP[0] * 4 + 4), slice(DROP[1] * 64, DROP[1] * 64 + 64)


# ---- checks -------------------------------------------------------------------------------------------------------------------------------
def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def per_tile(t, th, tw):
    B, Cc, Hh, Ww = t.shape
    return t.permute(0, 2, 3, 1).reshape(B, Hh // th, th, Ww // tw, tw, Cc)


def check_f32(name, got, want, bound, form, key, cap=None, th=4, tw=64):
    """whole-tensor and worst-tile rel-L2 of an fp32 output against the float64 reference"""
    from srbh_amd import _lib
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape), (got.dtype, got.shape, want.shape)
    want = want.to(got.device)
    d = got.detach().double() - want
    whole = float(d.norm() / want.norm())
    dt = per_tile(d, th, tw).square().sum((2, 4, 5)).sqrt()
    wt = per_tile(want, th, tw).square().sum((2, 4, 5)).sqrt()
    rt = (dt / wt.clamp_min(1e-300)).flatten()
    worst = int(rt.argmax())
    where = tile_owner(worst, rt.numel(), cap or _lib.head_wgs_cap(form))
    print(f"FIG {name} {key}: whole {whole:.3e} worst tile {float(rt[worst]):.3e} (tile {worst}: {where}) bound {bound:.1e}")
    assert whole <= bound, (name, key, whole)
    assert float(rt[worst]) <= bound, f"{name} {key}: tile {worst} ({where}) rel-L2 {float(rt[worst]):.3e}"


def spacing(v, dtype):
    """the spacing of `dtype` (fp16 / bf16, normal range) at magnitude v > 0 (float64): 2^(exponent of v - mantissa bits), from v's own bits"""
    e = (v.view(torch.int64) >> 52) & 0x7FF
    return ((e - (10 if dtype == torch.float16 else 7)) << 52).view(torch.float64)


def steps_off(a, w, rms, dtype):
    a, w = a.double().contiguous(), w.double().contiguous()
    return (a - w).abs() / spacing(torch.maximum(torch.maximum(a.abs(), w.abs()), rms).contiguous(), dtype)


def check_16(name, got, want64, host32, dtype, form, key, cap=None, th=4, tw=64):
    """a 16-bit output against the float64 reference rounded once; host32 = the host's fp32 evaluation (its share of flips caps the reference)"""
    from srbh_amd import _lib
    assert got.dtype == dtype and tuple(got.shape) == tuple(want64.shape), (got.dtype, got.shape)
    want64, host32 = want64.to(got.device), host32.to(got.device)
    want = want64.to(dtype)
    rms = want64.square().mean().sqrt()
    s_host = steps_off(host32.to(dtype), want, rms, dtype)
    share_host = float((s_host > 0).double().mean())
    assert float(s_host.max()) <= 1.0 and share_host <= 0.005, (name, key, float(s_host.max()), share_host)
    s = steps_off(got.detach(), want, rms, dtype)
    share = float((s > 0).double().mean())
    st = per_tile((s > 0).double(), th, tw).mean((2, 4, 5)).flatten()
    worst = int(st.argmax())
    where = tile_owner(worst, st.numel(), cap or _lib.head_wgs_cap(form))
    far = per_tile(s, th, tw).amax((2, 4, 5)).flatten()
    print(f"FIG {name} {key}: differing {share:.3e} (host fp32 {share_host:.3e}) max steps {float(s.max()):.2f} worst tile share "
          f"{float(st[worst]):.3e} (tile {worst}: {where})")
    assert float(s.max()) <= 1.0, f"{name} {key}: {float(s.max()):.1f} steps off in tile {int(far.argmax())} ({tile_owner(int(far.argmax()), far.numel(), cap or _lib.head_wgs_cap(form))})"
    assert share <= 0.02, (name, key, share)
    assert float(st[worst]) <= 0.02, f"{name} {key}: tile {worst} ({where}) differs in {float(st[worst]):.3e} of its elements"


def check_sum(name, got, want64, host32, dropped64, kind, key):
    """a sum over pixels: bound = min(K * floor, small-shape bound), and the bound is sharp against one dropped tile"""
    floor = rel(host32.cpu(), want64.cpu())
    bound = min(K_SUM[kind] * floor, CAP_SUM[kind])
    moved = rel(dropped64, want64)
    want64, dropped64 = want64.cpu(), dropped64.cpu()
    g = rel(got.detach().cpu(), want64)
    print(f"FIG {name} {key}: got {g:.3e} floor {floor:.3e} got/floor {g / floor:.2f} bound {bound:.3e} dropped tile {moved:.3e}")
    assert floor > 0 and bound <= 0.1 * moved, (name, key, bound, moved)
    assert g <= bound, (name, key, g, bound)


def fold(stats):
    """[NSLOT][2][16] partial sums -> [2][16]"""
    return stats.view(-1, 2, 16).sum(0)


def moments(y):
    return torch.stack([y.sum((0, 2, 3)), (y * y).sum((0, 2, 3))])


def bn_sums(dz, c, mean, invstd, mask):
    """sum dz', sum dz' * xhat per channel in the element type of the arguments (dz' = dz where c * ms + mh > 0)"""
    if mask is not None:
        keep = (c.double() * chan(mask[0]).double() + chan(mask[1]).double()) > 0        # exact sign of the kernel's fma(c, ms, mh)
        dz = torch.where(keep, dz, torch.zeros_like(dz))
    xhat = (c - chan(mean)) * chan(invstd)
    return torch.stack([dz.sum((0, 2, 3)), (dz * xhat).sum((0, 2, 3))])


def both(fn):
    """fn(dtype) evaluated in float64 and in fp32"""
    return fn(torch.float64), fn(torch.float32)


# ---- hconv16_kernel: forward forms --------------------------------------------------------------------------------------------------------
FWD_CASES = {
    # name: (16-bit source, pre-affine + ReLU, post scale/shift + ReLU, fp16 residual, fp16 output, statistics)
    "f32src_pre_stats": (False, True, False, False, False, True),      # depth-1 walk, forward statistics epilogue
    "f32src_post": (False, False, True, False, False, False),
    "h16src_post": (True, False, True, False, False, False),           # depth-2 walk, the source staged as it is
    "h16src_pre": (True, True, False, False, False, False),            # depth-2 walk through the widen / transform / round path
    "h16src_res16_out16": (True, False, True, True, True, False),
}


@gpu
@pytest.mark.parametrize("key", ["A", "B"])
@pytest.mark.parametrize("case", list(FWD_CASES))
def test_hconv16_forward_forms(case, key):
    from srbh_amd import hrfuse as H
    s16, pre, post, res16, o16, stats = FWD_CASES[case]
    walk_cap("hconv16", key)
    conv = conv_of(16, 16)
    x = act(key, 5).half() if s16 else act(key, 5)
    scale, shift = pow2(16, 7), rnd((16,), 8, -0.2, 0.2)
    psc, psh = rnd((16,), 9, 0.5, 1.5), rnd((16,), 10, -0.2, 0.2)
    res = act(key, 6).half() if res16 else None
    a = x.float()
    if pre:
        a = torch.relu(a * chan(scale) + chan(shift))
    xr, wr = a.half(), conv.weight.detach().half()

    def ref(dt):
        y = F.conv2d(xr.to(dt), wr.to(dt), conv.bias.detach().to(dt), 1, 1)
        if post:
            y = y * chan(psc).to(dt) + chan(psh).to(dt)
        if res is not None:
            y = y + res.to(dt)
        return torch.relu(y) if post else y

    want, host = both(ref)
    with H.head_precision("f16"), torch.no_grad(), ran(hconv16=1):
        conv = conv.to(DEV)
        got, st = H.hconv([nhwc(x)], conv, H._PackedConv(), pre=(scale.to(DEV), shift.to(DEV), True) if pre else None,
                          post=(psc.to(DEV), psh.to(DEV)) if post else None, post_relu=post, res=nhwc(res) if res is not None else None,
                          want_stats=stats, out_h16=o16)
        torch.cuda.synchronize()
    if o16:
        check_16(case, got, want, host, torch.float16, "hconv16", key)
    else:
        check_f32(case, got, want, TOL_CONV, "hconv16", key)
    if stats:
        b, rows, cols = drop_window(key)
        wd = want.to(DEV)
        check_sum(case + " sums", fold(st), moments(wd), moments(host), moments(wd) - moments(wd[b:b + 1, :, rows, cols]), "stats", key)


@gpu
@pytest.mark.parametrize("key", ["A", "B"])
@pytest.mark.parametrize("cout", [7, 1])
def test_hconv16_narrow_output(cout, key):
    """conv_last's 16 -> 7 / 16 -> 1 forms: scalar stores of the channels that exist"""
    from srbh_amd import hrfuse as H
    walk_cap("hconv16", key)
    conv = conv_of(16, cout)
    x = act(key, 5)
    want = F.conv2d(x.half().double(), conv.weight.detach().half().double(), conv.bias.detach().double(), 1, 1)
    with H.head_precision("f16"), torch.no_grad(), ran(hconv16=1):
        got, _ = H.hconv([nhwc(x)], conv.to(DEV), H._PackedConv())
        torch.cuda.synchronize()
    check_f32(f"narrow_out{cout}", got, want, TOL_CONV, "hconv16", key)


# ---- hconv16_kernel: bf16 data-gradient forms ---------------------------------------------------------------------------------------------
def dgrad_ref(g, weight, dt):
    """conv^T(g, W) of the bf16-rounded operands as a conv with the transposed + flipped weight"""
    wt = weight.detach().bfloat16().to(dt).transpose(0, 1).flip(2, 3)
    return F.conv2d(g.bfloat16().to(dt), wt, None, 1, 1)


DGRAD_CASES = {
    # name: (bf16 dY in memory, skip gradient, bf16 output, backward-statistics epilogue)
    "dgrad": (False, False, False, False),
    "dgrad_g16_skip": (True, True, False, False),
    "dgrad_g16_out16": (True, False, True, False),
    "dgrad_g16_bstat": (True, False, False, True),
}


@gpu
@pytest.mark.parametrize("key", ["A", "B"])
@pytest.mark.parametrize("case", list(DGRAD_CASES))
def test_hconv16_data_gradient_forms(case, key):
    from srbh_amd import hrfuse as H
    from srbh_amd import hrfuse_autograd as HA
    g16, skip, o16, bstat = DGRAD_CASES[case]
    walk_cap("hconv16", key)
    conv = conv_of(16, 16, bias=False)
    g = act(key, 17, scale=1e-3)
    g = g.bfloat16() if g16 else g
    res = act(key, 18, scale=1e-3).bfloat16() if skip else None
    want, host = both(lambda dt: dgrad_ref(g, conv.weight, dt) + (res.to(dt) if skip else 0))
    c = act(key, 19)
    mean, invstd = rnd((16,), 20, -0.1, 0.1), rnd((16,), 21, 0.5, 1.5)
    mask = (rnd((16,), 22, 0.5, 1.5), rnd((16,), 23, -0.2, 0.2))
    with H.head_precision("f16"), torch.no_grad(), ran(hconv16=1):
        st = HA._stats_buf(16, DEV) if bstat else None
        cd = nhwc(c)
        bs = (cd, mean.to(DEV), invstd.to(DEV), mask[0].to(DEV), mask[1].to(DEV), st) if bstat else None
        if bstat:
            assert HA.bstat_fusable(nhwc(g), conv.weight, cd)
        got = HA.conv_dgrad(nhwc(g), conv.weight.detach().to(DEV), HA._PackedGrad(), res=nhwc(res) if skip else None, out_b16=o16, bstat=bs)
        torch.cuda.synchronize()
    if o16:
        check_16(case, got, want, host, torch.bfloat16, "hconv16", key)
    else:
        check_f32(case, got, want, TOL_CONV, "hconv16", key)
    if bstat:
        b, rows, cols = drop_window(key)
        wd, c64, dmask = want.to(DEV), cd.double(), (mask[0].to(DEV), mask[1].to(DEV))
        s64 = bn_sums(wd, c64, mean.to(DEV).double(), invstd.to(DEV).double(), dmask)
        s32 = bn_sums(host, c, mean, invstd, mask)
        part = bn_sums(wd[b:b + 1, :, rows, cols], c64[b:b + 1, :, rows, cols], mean.to(DEV).double(), invstd.to(DEV).double(), dmask)
        frac = float(((c.double() * chan(mask[0]).double() + chan(mask[1]).double()) > 0).double().mean())
        assert 0.2 < frac < 0.8, frac
        check_sum(case + " sums", fold(st), s64, s32, s64 - part, "stats", key)


@gpu
@pytest.mark.parametrize("key", ["A", "B"])
@pytest.mark.parametrize("cout_fwd", [7, 1])
def test_hconv16_narrow_input_data_gradient(cout_fwd, key):
    """dX = conv^T(dY[7 or 1], W): fp32 source of < 16 channels, four guarded scalar loads per staging unit"""
    from srbh_amd import hrfuse as H
    from srbh_amd import hrfuse_autograd as HA
    walk_cap("hconv16", key)
    conv = conv_of(16, cout_fwd, bias=False)
    g = act(key, 24, c=cout_fwd, scale=1e-3)
    want = dgrad_ref(g, conv.weight, torch.float64)
    with H.head_precision("f16"), torch.no_grad(), ran(hconv16=1):
        got = HA.conv_dgrad(nhwc(g), conv.weight.detach().to(DEV), HA._PackedGrad())
        torch.cuda.synchronize()
    check_f32(f"narrow_in{cout_fwd}", got, want, TOL_CONV, "hconv16", key)


# ---- hwgrad16_kernel ----------------------------------------------------------------------------------------------------------------------
def wgrad_refs(xin, g, key):
    """(float64, host fp32, float64 without the dropped tile) weight gradient of the bf16-rounded (xin, g)"""
    b, rows, cols = drop_window(key)
    xb, gb = xin.bfloat16(), g.bfloat16()
    w64, w32 = both(lambda dt: torch.nn.grad.conv2d_weight(xb.to(dt), (16, 16, 3, 3), gb.to(dt), padding=1))
    xwin = xb[b:b + 1, :, rows.start - 1:rows.stop + 1, cols.start - 1:cols.stop + 1].double()        # (an interior tile: its halo exists)
    part = torch.nn.grad.conv2d_weight(xwin, (16, 16, 3, 3), gb[b:b + 1, :, rows, cols].double(), padding=0)
    return w64, w32, w64 - part


@gpu
@pytest.mark.parametrize("key", ["A", "B"])
@pytest.mark.parametrize("case", ["f32", "f32_pre", "x16_g16"])
def test_hwgrad16_forms(case, key):
    from srbh_amd import hrfuse as H
    from srbh_amd import hrfuse_autograd as HA
    walk_cap("wgrad16", key)
    x, g = act(key, 15), act(key, 17, scale=1e-3)
    scale, shift = pow2(16, 7), rnd((16,), 8, -0.2, 0.2)
    if case == "x16_g16":
        x, g = x.half(), g.bfloat16()
    xin = torch.relu(x.float() * chan(scale) + chan(shift)) if case == "f32_pre" else x.float()
    w64, w32, wdrop = wgrad_refs(xin, g, key)
    with H.head_precision("f16"), torch.no_grad(), ran(wgrad16=1, wgrad_b16_generic=0, wgrad_f32=0):
        got = HA.conv_wgrad([nhwc(x)], (scale.to(DEV), shift.to(DEV), True) if case == "f32_pre" else None, nhwc(g), 16, 3)
        torch.cuda.synchronize()
    check_sum("hwgrad16 " + case, got, w64, w32, wdrop, "wgrad16", key)


# ---- hbwd16_kernel ------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("key", ["A", "B"])
@pytest.mark.parametrize("form", ["conv2", "conv1", "conv1_bits"])
def test_hbwd16_forms(form, key):
    """conv2 form: statistics epilogue, bf16 dx, folded pre-affine; conv1 form: ReLU mask, skip gradient, fp32 dx; conv1_bits: the conv1 form
    whose dx + skip gradient goes on through the previous block's closing ReLU (relu_bits) as bf16, summed for that block's bn2 over the
    values it wrote.  Against the three launches it replaces (the conditions of test_gpu_hbwd16.py) and against float64 on the bf16 dc those
    launches hand over."""
    from srbh_amd import hrfuse as H
    from srbh_amd import hrfuse_autograd as HA
    from tests.test_gpu_hbwd16 import _case, _separate
    walk_cap("hbwd16", key)
    B, Hh, Ww = SHAPES[key]
    conv2 = form == "conv2"
    gy, c, x, mean, invstd, consts, mask, w = _case(B, Hh, Ww, 31 if conv2 else 32, not conv2)
    gen = torch.Generator().manual_seed(99)
    s1, h1 = pow2(16, 7).to(DEV), (torch.randn(16, generator=gen) * 0.2).to(DEV)
    m1, i1 = (torch.randn(16, generator=gen) * 0.1).to(DEV), (torch.rand(16, generator=gen) + 0.5).to(DEV)
    pre = (s1, h1, True) if conv2 else None
    bits = form == "conv1_bits"
    res = None if conv2 else nhwc(act(key, 18, scale=1e-3).bfloat16())
    with H.head_precision("f16"), torch.no_grad():
        assert HA.hbwd16_ok(c, x, w)
        st_a, st_b = (HA._stats_buf(16, DEV), HA._stats_buf(16, DEV)) if conv2 else (HA._stats_buf(16, DEV) if bits else None, None)
        bstat = (x, m1, i1, s1, h1, st_a) if conv2 else None
        pattern = active = c2p = None
        if bits:          # the previous block: out' = relu(bn2'(c2') + idt'), its activity pattern as bits
            c2p = nhwc(act(key, 33))
            out_p, pattern = H.bn_add_relu(c2p, torch.ones(16, device=DEV), torch.zeros(16, device=DEV), nhwc(act(key, 34) * 0.5), want_bits=True)
            active = out_p > 0
            assert 0.2 < float(active.float().mean()) < 0.8
            bstat = (c2p, m1, i1, None, None, st_a)
        with ran(hbwd16=1):
            dx, dw = HA.hbwd16(gy, c, mean, invstd, consts, mask, x, pre, w, HA._PackedGrad(), res=res, out_b16=conv2 or bits, bstat=bstat,
                               relu_bits=pattern)
        dc, dx_r, dw_r = _separate(gy, c, mean, invstd, consts, mask, x, pre, w, res, conv2, (x, m1, i1, s1, h1, st_b) if conv2 else None)
        torch.cuda.synchronize()
    # the three launches (near-identical: rare one-step flips of the apply arithmetic)
    if conv2:
        assert rel(dx.float(), dx_r.float()) <= 2e-3 and float((dx.float() != dx_r.float()).float().mean()) <= 0.02
        assert rel(fold(st_a), fold(st_b)) <= 1e-4
    elif not bits:
        assert rel(dx, dx_r) <= 1e-4
    assert rel(dw, dw_r) <= 1e-4
    # float64 on the same rounded operands
    dch, xh, wh = dc.cpu(), x.cpu(), w.cpu()
    xp = torch.relu(xh * chan(s1.cpu()) + chan(h1.cpu())) if conv2 else xh
    want, host = both(lambda dt: dgrad_ref(dch, wh, dt) + (res.cpu().to(dt) if res is not None else 0))
    if bits:
        keep = active.cpu()
        want, host = torch.where(keep, want, torch.zeros_like(want)), torch.where(keep, host, torch.zeros_like(host))
    if conv2 or bits:
        check_16(f"hbwd16 {form} dx", dx, want, host, torch.bfloat16, "hbwd16", key)
    else:
        check_f32("hbwd16 conv1 dx", dx, want, TOL_HBWD_DX, "hbwd16", key)
    if not conv2:
        frac = float((c * chan(mask[0]) + chan(mask[1]) <= 0).float().mean())
        assert 0.2 < frac < 0.8, frac
    if bits:          # the sums are taken over the bf16 values the kernel wrote (what the consumer reads)
        assert float((dx.float() == 0).float().mean()) > 0.2
        b, rows, cols = drop_window(key)
        d64 = dx.double()
        s64 = bn_sums(d64, c2p.double(), m1.double(), i1.double(), None)
        s32 = bn_sums(dx.float().cpu(), c2p.cpu(), m1.cpu(), i1.cpu(), None)
        part = bn_sums(d64[b:b + 1, :, rows, cols], c2p.double()[b:b + 1, :, rows, cols], m1.double(), i1.double(), None)
        check_sum("hbwd16 conv1_bits sums", fold(st_a), s64, s32, s64 - part, "stats", key)
    w64, w32, wdrop = wgrad_refs(xp, dch, key)
    check_sum(f"hbwd16 {form} dw", dw, w64, w32, wdrop, "hbwd16", key)
    if conv2:
        b, rows, cols = drop_window(key)
        mk = (s1.cpu(), h1.cpu())
        wd, x64 = want.to(DEV), x.double()
        s64 = bn_sums(wd, x64, m1.double(), i1.double(), (s1, h1))
        s32 = bn_sums(host, xh, m1.cpu(), i1.cpu(), mk)
        part = bn_sums(wd[b:b + 1, :, rows, cols], x64[b:b + 1, :, rows, cols], m1.double(), i1.double(), (s1, h1))
        check_sum("hbwd16 conv2 sums", fold(st_a), s64, s32, s64 - part, "stats", key)


# ---- hblock16_kernel ----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("key", ["A", "B"])
@pytest.mark.parametrize("out_h16", [True, False])
def test_hblock16_forms(out_h16, key):
    """the float64 graph of the block on the fp16-rounded operands, and the two-launch chain under the conditions of test_gpu_hblock16.py"""
    from srbh_amd import hrfuse as H
    from tests.test_gpu_hblock16 import _block
    walk_cap("hblock16", key)
    walk_cap("hconv16", key)                       # (the two-launch chain walks too)
    blk = _block(5)
    x = (act(key, 5) * 0.7).half()
    xd = nhwc(x)
    outs = {}
    with torch.no_grad(), H.head_precision("f16"):
        for fused in (True, False):
            H.HBLOCK16 = fused
            try:
                with ran(hblock16=1 if fused else 0, hconv16=0 if fused else 2):
                    outs[fused] = blk.forward_nhwc([xd], out_h16=out_h16)
                    torch.cuda.synchronize()
            finally:
                H.HBLOCK16 = True
    got, chain = outs[True], outs[False].float()
    d = (got.float() - chain).abs()
    assert bool((d <= 2.0 ** -9 * chain.abs().clamp_min(1.0)).all()), float(d.max())
    assert float(d.norm() / chain.norm()) <= 1e-4
    if out_h16:
        assert float((d > 0).float().mean()) <= 0.02, float((d > 0).float().mean())

    def ref(dt):
        b = _block(5).cpu().to(dt)
        with torch.no_grad():
            w1, w2 = b.conv1.weight.half().to(dt), b.conv2.weight.half().to(dt)
            a1 = F.relu(b.bn1(F.conv2d(x.to(dt), w1, padding=1))).half().to(dt)
            return F.relu(b.bn2(F.conv2d(a1, w2, padding=1)) + x.to(dt))

    want, host = both(ref)
    if out_h16:
        check_16("hblock16 fp16", got, want, host, torch.float16, "hblock16", key)
    else:
        check_f32("hblock16 fp32", got, want, TOL_HBLOCK, "hblock16", key)


# ---- hconv_up_kernel ----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("key", ["A", "B"])
@pytest.mark.parametrize("io16", [False, True])
def test_hconv_up_forms(io16, key, monkeypatch):
    """conv 16 -> 64 + PixelShuffle(2) on the persistent kernel: bit for bit the template's result, and the float64 conv of the rounded operands
    (a 4 x 64 input tile is an 8 x 128 output tile)"""
    from srbh_amd import hrfuse as H
    walk_cap("hconv_up", key)
    conv = conv_of(16, 64)
    x = act(key, 5).half() if io16 else act(key, 5)
    want, host = both(lambda dt: F.pixel_shuffle(F.conv2d(x.half().to(dt), conv.weight.detach().half().to(dt), conv.bias.detach().to(dt), 1, 1), 2))
    conv = conv.to(DEV)
    xd = nhwc(x)
    outs = {}
    with H.head_precision("f16"), torch.no_grad():
        for flag in (True, False):
            monkeypatch.setattr(H, "HCONV_UP", flag)
            with ran(hconv_up=1 if flag else 0, hconv_template=0 if flag else 1):
                outs[flag], _ = H.hconv([xd], conv, H._PackedConv(), ps2=True, out_h16=io16)
                torch.cuda.synchronize()
    assert torch.equal(outs[True], outs[False])
    if io16:
        check_16("hconv_up fp16", outs[True], want, host, torch.float16, "hconv_up", key, th=8, tw=128)
    else:
        check_f32("hconv_up fp32", outs[True], want, TOL_CONV, "hconv_up", key, th=8, tw=128)


# ---- hconv_entry kernels (shape A: tiles that change column; the aligned multi-tile case is in test_gpu_feature_h16.py) ----------------------
@gpu
@pytest.mark.parametrize("c0,c1,whole_row", [(16, 16, False), (64, 16, False), (64, 0, True)])
def test_hconv_entry_forms(c0, c1, whole_row):
    """conv1 (3x3) + downsample[0] (1x1) over one input in one pass: the chunked kernel at 32 and 80 input channels (fp32 sources, BatchNorm
    sums), the whole-row kernel on a 64-channel fp16 source -- which must also equal, bit for bit, the chunked kernel fed the same values as
    fp32.  Whether a 64-channel fp16 source takes the whole-row kernel is not counted separately: the knob that switches it off must be unset."""
    import os
    from srbh_amd import hrfuse as H
    key = "A"
    if whole_row:
        assert os.environ.get("SRBH_HCONV_ENTRY64", "1") != "0"
        assert walk_counts(ntiles_of(key), ENTRY64_WGS) == {3, 4}
    cap = walk_cap("entry_fused", key)
    conv1, convd = conv_of(c0 + c1, 16, 3, bias=False, seed=3), conv_of(c0 + c1, 16, 1, bias=False, seed=4)
    x0 = (act(key, 5, c=c0) * 0.7).half() if whole_row else act(key, 5, c=c0)
    x1 = act(key, 6, c=c1) if c1 else None
    xin = torch.cat([x0.float()] + ([x1] if c1 else []), 1).half()
    r1 = both(lambda dt: F.conv2d(xin.to(dt), conv1.weight.detach().half().to(dt), None, 1, 1))
    rd = both(lambda dt: F.conv2d(xin.to(dt), convd.weight.detach().half().to(dt), None, 1, 0))
    conv1, convd = conv1.to(DEV), convd.to(DEV)
    srcs = [nhwc(x0)] + ([nhwc(x1)] if c1 else [])
    with H.head_precision("f16"), torch.no_grad(), ran(entry_fused=2 if whole_row else 1, entry_split=0):
        a = H.hconv_entry(srcs, conv1, H._PackedConv(), convd, H._PackedConv(), want_stats=True)
        if whole_row:
            b = H.hconv_entry([nhwc(x0.float())], conv1, H._PackedConv(), convd, H._PackedConv(), want_stats=True)
        torch.cuda.synchronize()
    if whole_row:
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    wcap = ENTRY64_WGS if whole_row else cap
    bi, rows, cols = drop_window(key)
    for name, out, st, (want, host) in (("conv1", a[0], a[1], r1), ("downsample", a[2], a[3], rd)):
        check_f32(f"entry{c0 + c1} {name}", out, want, TOL_CONV, "entry_fused", key, cap=wcap)
        wd = want.to(DEV)
        check_sum(f"entry{c0 + c1} {name} sums", fold(st), moments(wd), moments(host), moments(wd) - moments(wd[bi:bi + 1, :, rows, cols]), "stats", key)
