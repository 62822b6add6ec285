"""The plane kernels of the VGG19 perceptual loss (csrc/srbh_vgg.hip) one at a time through the C ABI, against torch on the SAME 16-bit values,
bit for bit: input normalisation + conversion, ReLU, ReLU + 2x2 max-pool (odd sizes: 5 -> 2), its backward with torch's first-maximum tie rule
(windows with equal maxima included), and the one-read feature distance (float64 sum at 1e-12 relative, gradient planes bit-equal, two runs
bit-identical).  Borders stay zero everywhere: the kernels write interiors only."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from srbh_amd import _lib
from tests import gpu_util as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def rnd(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


def bits(t):
    return t.contiguous().view(torch.int16).cpu()


def planes_f16(t):
    """(B, C, H, W) fp32 holding fp16-representable values -> fp16 ACT16 planes"""
    return G.act16_from_nchw_x16(t.to(DEV), bf16=0)


def planes_b16(t):
    return G.act16_from_nchw_x16(t.to(DEV), bf16=1)


@pytest.mark.parametrize("norm,rng", [(True, False), (False, True), (True, True), (False, False)])
def test_input_conversion(norm, rng):
    B, H, W = 2, 9, 70
    x = rnd((B, 3, H, W), 1, -1.0 if rng else 0.0, 1.0).to(DEV)
    buf = G.act16_alloc(B, 1, H, W, DEV)
    buf.view(torch.int16)[:] = 0x3c00                      # stale ones everywhere: the kernel must write all 32 channels of the interior ...
    raw = G.act16_raw(buf, B, 1, H, W, torch.int16)
    raw[:, :, 0] = 0; raw[:, :, -1] = 0; raw[:, :, :, 0] = 0; raw[:, :, :, -1] = 0      # ... and only the interior
    mean, std = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    _lib.check(_lib.lib().srbh_vgg_input_f16(x.data_ptr(), buf.data_ptr(), B, H, W, mean if norm else None, std if norm else None, int(rng),
                                             _lib.stream_ptr()), "vgg_input_f16")
    torch.cuda.synchronize()
    want = x.cpu()
    if rng:
        want = (want + 1.0) / 2.0
    if norm:
        want = (want - torch.tensor(MEAN).view(1, 3, 1, 1)) / torch.tensor(STD).view(1, 3, 1, 1)
    got = G.act16_planes(buf, B, 1, H, W, torch.float16)
    assert torch.equal(bits(got[:, :3]), bits(want.half()))
    assert not bool(bits(got[:, 3:]).any()) and G.border_is_zero(buf, B, 1, H, W)


def _with_ties(shape, seed):
    """fp16-representable values, many exact ties and all-negative windows: a coarse grid of values"""
    return (rnd(shape, seed) * 4).round() / 4 + 0.0        # (+ 0.0: no negative zeros, whose ReLU torch leaves as -0.0 and the kernel stores as 0.0)


@pytest.mark.parametrize("B,Cc,H,W", [(2, 64, 5, 5), (1, 32, 8, 70), (1, 128, 3, 2), (2, 32, 48, 40)])
@pytest.mark.parametrize("pool", [0, 1])
def test_relu_pool_and_backward(B, Cc, H, W, pool):
    ch = Cc // 32
    s = _with_ties((B, Cc, H, W), 3) if (H, W) != (48, 40) else rnd((B, Cc, H, W), 3).half().float()
    sp = planes_f16(s)
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    out = G.act16_alloc(B, ch, Ho, Wo, DEV)
    L = _lib.lib()
    _lib.check(L.srbh_vgg_relu_pool_f16(sp.data_ptr(), out.data_ptr(), B, ch, H, W, pool, _lib.stream_ptr()), "vgg_relu_pool_f16")
    torch.cuda.synchronize()
    want = F.relu(s)
    if pool:
        want = F.max_pool2d(want, 2, 2)
    assert torch.equal(bits(G.act16_planes(out, B, ch, Ho, Wo, torch.float16)), bits(want.half()))
    assert G.border_is_zero(out, B, ch, Ho, Wo)

    # backward: g_z = [add] + (saved > 0) * route(g), against autograd of the same chain on the same values (float64: one rounding to bf16 here too)
    g = G.b16(rnd((B, Cc, Ho, Wo), 4))
    for with_add in (False, True):
        add = G.b16(rnd((B, Cc, H, W), 5)) if with_add else None
        gz = G.act16_alloc(B, ch, H, W, DEV)
        gp, ap = planes_b16(g), (None if add is None else planes_b16(add))       # (held: a temporary's memory would be handed to the next one)
        _lib.check(L.srbh_vgg_relu_pool_bwd_b16(gp.data_ptr(), sp.data_ptr(), None if ap is None else ap.data_ptr(), gz.data_ptr(),
                                                B, ch, H, W, pool, _lib.stream_ptr()), "vgg_relu_pool_bwd_b16")
        torch.cuda.synchronize()
        sv = s.double().requires_grad_(True)
        y = F.relu(sv)
        if pool:
            y = F.max_pool2d(y, 2, 2)
        (routed,) = torch.autograd.grad(y, sv, g.double())
        routed = torch.where(s > 0, routed, torch.zeros_like(routed))          # (relu'(0) = 0 in torch as well: stated, not assumed)
        want_g = (routed + (add.double() if with_add else 0)).float().to(torch.bfloat16)
        got = G.act16_planes(gz, B, ch, H, W, torch.bfloat16)
        zero_sign = lambda t: torch.where(t == 0, torch.zeros_like(t), t)      # noqa: E731  (-0.0 from 0 * g and +0.0 are the same gradient)
        assert torch.equal(bits(zero_sign(got.float().cpu()).to(torch.bfloat16)), bits(zero_sign(want_g.float()).to(torch.bfloat16)))
        assert G.border_is_zero(gz, B, ch, H, W)


@pytest.mark.parametrize("l2", [0, 1])
@pytest.mark.parametrize("B,Cc,H,W", [(2, 64, 24, 20), (1, 512, 3, 2), (2, 64, 48, 40)])
def test_feature_distance_and_its_gradient(B, Cc, H, W, l2):
    ch = Cc // 32
    a, b = rnd((B, Cc, H, W), 6, -4, 4).half().float(), rnd((B, Cc, H, W), 7, -4, 4).half().float()
    b[0, :, 0] = a[0, :, 0]                                  # d == 0 on a whole row: sign(0) = 0
    pa, pb = planes_f16(a), planes_f16(b)
    L = _lib.lib()
    n = a.numel()
    wgt = 0.1
    coef = wgt / n
    gscale = (2.0 if l2 else 1.0) * wgt / n
    ws = torch.empty(max(1, L.srbh_vgg_dist_ws_bytes(B, ch, H, W) // 8), dtype=torch.float64, device=DEV)
    runs = []
    for _ in range(2):
        acc = torch.full((1,), 123.0, dtype=torch.float64, device=DEV)
        grad = G.act16_alloc(B, ch, H, W, DEV)
        _lib.check(L.srbh_vgg_dist(pa.data_ptr(), pb.data_ptr(), B, ch, H, W, l2, coef, 0, acc.data_ptr(), gscale, grad.data_ptr(), ws.data_ptr(),
                                   _lib.stream_ptr()), "vgg_dist")
        _lib.check(L.srbh_vgg_dist(pa.data_ptr(), pb.data_ptr(), B, ch, H, W, l2, coef, 1, acc.data_ptr(), gscale, None, ws.data_ptr(),
                                   _lib.stream_ptr()), "vgg_dist(accumulate)")
        torch.cuda.synchronize()
        runs.append((float(acc), G.act16_planes(grad, B, ch, H, W, torch.bfloat16).cpu().clone()))
        assert G.border_is_zero(grad, B, ch, H, W)
    d = a.double() - b.double()
    s = float((d * d).sum() if l2 else d.abs().sum())
    want = 2 * coef * s                                       # overwritten once, accumulated once
    print(f"vgg_dist l2={l2} {B}x{Cc}x{H}x{W}: {runs[0][0]!r} vs float64 {want!r}")
    assert abs(runs[0][0] - want) <= 1e-12 * abs(want)
    gs = torch.tensor(gscale, dtype=torch.float32)
    want_g = (gs * (a - b) if l2 else gs * torch.sign(a - b)).to(torch.bfloat16)
    assert torch.equal(bits(runs[0][1]), bits(want_g))
    assert runs[0][0] == runs[1][0] and torch.equal(bits(runs[0][1]), bits(runs[1][1]))


def test_dx_scaling():
    B, H, W = 2, 7, 9
    g = rnd((B, H, W, 3), 8).to(DEV)
    go = torch.tensor([0.37], device=DEV)
    std = (C.c_float * 3)(*STD)
    for norm, rng in ((True, False), (False, True), (True, True)):
        dx = torch.empty((B, 3, H, W), device=DEV)
        _lib.check(_lib.lib().srbh_vgg_dx_nchw(g.data_ptr(), dx.data_ptr(), B, H, W, std if norm else None, int(rng), go.data_ptr(), _lib.stream_ptr()), "dx")
        torch.cuda.synchronize()
        want = g.permute(0, 3, 1, 2).cpu()
        if norm:
            want = want / torch.tensor(STD).view(1, 3, 1, 1)
        if rng:
            want = want / 2.0
        assert torch.equal(dx.cpu(), want * go.cpu())
