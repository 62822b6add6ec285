"""The discriminator's 4x4 / stride 2 / pad 1 convs on libsrbh (csrc/srbh_disc.hip, UNetDiscriminatorSN.libsrbh_s2 = "f16"): staging, packs,
the three products through the C ABI, argument checks, the module and the trainer.

Products are compared with the float64 product of the SAME rounded operands (tests/disc_s2_oracle.py) under the derived elementwise bound
    |y - y64| <= K 2^-23 conv(|a|, |b|),     K = addends per output element (forward 16 C, data gradient 4 O, weight gradient B Ho Wo):
products of two 16-bit operands are exact in fp32, any summation tree of K fp32 additions stays inside K u, and u is taken as 2^-23 because the
matrix unit's internal accumulation is not documented as round-to-nearest per addition.  Every element is compared.  The largest observed
ratio (error / bound) per product is printed; measured on an MI355X over the four shapes: forward 1.5e-3, data gradient 2.8e-3, weight
gradient 6.0e-2 (its K is as small as 16 there)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import srbh_oracle as O
from srbh_amd import _lib
from tests import disc_s2_oracle as D
from tests import gpu_util as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -23


def sp():
    return _lib.stream_ptr()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16).cpu(), b.contiguous().view(torch.int16).cpu())


def stage_s(x, bf=0):
    """x (B, C, H, W) on the device -> the planes of S"""
    B, Cc, H, W = x.shape
    buf = G.act16_alloc(B, 4 * Cc // 32, H // 2 + 1, W // 2 + 1, DEV)
    _lib.check(_lib.lib().srbh_s2d_nhwc32_to_act16(nhwc(x).data_ptr(), buf.data_ptr(), B, Cc, H, W, bf, sp()), "s2d")
    return buf


def stage_g(g, bf=1):
    B, Oc, Ho, Wo = g.shape
    buf = G.act16_alloc(B, Oc // 32, Ho + 2, Wo + 2, DEV)
    _lib.check(_lib.lib().srbh_nhwc32_to_act16_framed(nhwc(g).data_ptr(), buf.data_ptr(), B, Oc, Ho, Wo, bf, sp()), "framed")
    return buf


def pack(w, tf, bf):
    Oc, Cc = w.shape[:2]
    L = _lib.lib()
    buf = torch.zeros(L.srbh_wpack2x2_bytes(Oc, 4 * Cc), dtype=torch.uint8, device=DEV)
    _lib.check(L.srbh_pack_conv4x4s2(w.contiguous().data_ptr(), Oc, Cc, tf, bf, buf.data_ptr(), sp()), "pack_conv4x4s2")
    return buf


def wconv2x2(planes, cin, wp, cout, B, H, W, bf, out=None, **kw):
    a = _lib.WConvArgs()
    a.in_, a.in_chunks_total, a.in_chunk0, a.in_chunks = planes.data_ptr(), cin // 32, 0, cin // 32
    a.w, a.cout, a.B, a.H, a.W, a.bf16 = wp.data_ptr(), cout, B, H, W, bf
    if out is not None:
        a.out32, a.out32_c = out.data_ptr(), cout
    for k, v in kw.items():
        setattr(a, k, v)
    _lib.check(_lib.lib().srbh_wconv2x2(C.byref(a), sp()), "wconv2x2")
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def cases():
    """per shape: fp32 x, w, g on the CPU and the three float64 products with their bound scales -- computed once, never modified"""
    out = {}
    for shp in D.SHAPES:
        B, Cc, Oc, H, W = shp
        gen = torch.Generator()
        gen.manual_seed(Cc * 7 + H)
        x = torch.randn(B, Cc, H, W, generator=gen)
        w = torch.randn(Oc, Cc, 4, 4, generator=gen) * 0.05
        g = torch.randn(B, Oc, H // 2, W // 2, generator=gen)
        out[shp] = dict(x=x, w=w, g=g, fwd=D.forward(x, w), ds=D.dgrad_ds(g, w), dw=D.wgrad(x, g))
    return out


def check_bound(name, got, want, scale, K):
    got, bound = got.double(), K * U * scale
    err = (got - want).abs()
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"[disc_s2] {name}: K={K} max |err| {float(err.max()):.3e}, largest err / bound {ratio:.3e}")
    assert bool((err <= bound).all()), (name, ratio)
    return ratio


@pytest.mark.parametrize("shp", D.SHAPES)
def test_staging_is_bit_exact(shp, cases):
    B, Cc, Oc, H, W = shp
    c = cases[shp]
    Hs, Ws = H // 2 + 1, W // 2 + 1
    buf = stage_s(c["x"].to(DEV))
    torch.cuda.synchronize()
    want = D.s2d(c["x"]).half()
    assert same_bits(G.act16_to_nchw(buf, B, 4 * Cc, Hs, Ws).half(), want)          # pad-derived zeros included
    assert same_bits(G.act16_planes(buf, B, 4 * Cc // 32, Hs, Ws, torch.float16), want)
    assert G.border_is_zero(buf, B, 4 * Cc // 32, Hs, Ws)
    # the framed gradient planes, bf16: the data at (1, 1) of an (Ho+2) x (Wo+2) interior, the ring zero
    Ho, Wo = H // 2, W // 2
    gb = stage_g(c["g"].to(DEV))
    torch.cuda.synchronize()
    want_g = torch.nn.functional.pad(c["g"], (1, 1, 1, 1)).to(torch.bfloat16)
    assert same_bits(G.act16_planes(gb, B, Oc // 32, Ho + 2, Wo + 2, torch.bfloat16), want_g)
    assert G.border_is_zero(gb, B, Oc // 32, Ho + 2, Wo + 2)
    # a used buffer is written again in full: the ring too
    G.act16_raw(gb, B, Oc // 32, Ho + 2, Wo + 2, torch.int16)[:, :, 1:-1, 1:-1] = 0x3F80
    _lib.check(_lib.lib().srbh_nhwc32_to_act16_framed(nhwc(c["g"].to(DEV)).data_ptr(), gb.data_ptr(), B, Oc, Ho, Wo, 1, sp()), "framed")
    torch.cuda.synchronize()
    assert same_bits(G.act16_planes(gb, B, Oc // 32, Ho + 2, Wo + 2, torch.bfloat16), want_g)


@pytest.mark.parametrize("shp", D.SHAPES)
def test_d2s_is_the_exact_permutation(shp):
    B, Cc, Oc, H, W = shp
    gen = torch.Generator()
    gen.manual_seed(3)
    ds = torch.randn(B, 4 * Cc, H // 2 + 1, W // 2 + 1, generator=gen)
    gb = G.GuardedBuffers()
    src = gb.inp(nhwc(ds))
    dx = gb.out((B, H, W, Cc))
    _lib.check(_lib.lib().srbh_d2s_nhwc32(src.data_ptr(), dx.data_ptr(), B, Cc, H, W, sp()), "d2s")
    gb.verify()
    assert torch.equal(dx.permute(0, 3, 1, 2).cpu(), D.d2s(ds))


@pytest.mark.parametrize("shp", D.SHAPES)
def test_forward_product(shp, cases):
    B, Cc, Oc, H, W = shp
    c = cases[shp]
    gb = G.GuardedBuffers()
    out = gb.out((B, H // 2, W // 2, Oc))
    wconv2x2(stage_s(c["x"].to(DEV)), 4 * Cc, pack(c["w"].to(DEV), 0, 0), Oc, B, H // 2, W // 2, 0, out=out)
    gb.verify()
    want, scale = c["fwd"]
    check_bound(f"forward {shp}", out.permute(0, 3, 1, 2).cpu(), want, scale, 16 * Cc)


@pytest.mark.parametrize("shp", D.SHAPES)
def test_data_gradient_product(shp, cases):
    B, Cc, Oc, H, W = shp
    c = cases[shp]
    Ho, Wo = H // 2, W // 2
    gb = G.GuardedBuffers()
    ds = gb.out((B, Ho + 1, Wo + 1, 4 * Cc))
    wconv2x2(stage_g(c["g"].to(DEV)), Oc, pack(c["w"].to(DEV), 1, 1), 4 * Cc, B, Ho + 1, Wo + 1, 1, out=ds)
    gb.verify()
    want, scale = c["ds"]
    check_bound(f"data gradient {shp}", ds.permute(0, 3, 1, 2).cpu(), want, scale, 4 * Oc)
    dx = torch.empty((B, H, W, Cc), device=DEV)
    _lib.check(_lib.lib().srbh_d2s_nhwc32(ds.data_ptr(), dx.data_ptr(), B, Cc, H, W, sp()), "d2s")
    assert torch.equal(dx.permute(0, 3, 1, 2).cpu(), D.d2s(ds.permute(0, 3, 1, 2).cpu()))


@pytest.mark.parametrize("shp", D.SHAPES)
def test_weight_gradient_product_and_determinism(shp, cases):
    B, Cc, Oc, H, W = shp
    c = cases[shp]
    Ho, Wo = H // 2, W // 2
    L = _lib.lib()
    S, Gp = stage_s(c["x"].to(DEV)), stage_g(c["g"].to(DEV))
    nws = L.srbh_wgrad4x4s2_ws_bytes(Oc, Cc, B, Ho, Wo)
    assert nws > 0 and nws % 4 == 0
    res = []
    for fill in (float("nan"), 3.0):                         # (the workspace needs no initialisation)
        gb = G.GuardedBuffers()
        dw = gb.out((Oc, Cc, 4, 4))
        ws = gb.out((nws // 4,), fill=torch.full((nws // 4,), fill))
        _lib.check(L.srbh_wgrad4x4s2_b16(S.data_ptr(), Gp.data_ptr(), B, Cc, Oc, Ho, Wo, dw.data_ptr(), ws.data_ptr(), sp()), "wgrad4x4s2_b16")
        gb.verify()                                          # (every workspace slot is written, none beyond)
        res.append(dw.cpu().clone())
    assert torch.equal(res[0], res[1])
    want, scale = c["dw"]
    check_bound(f"weight gradient {shp}", res[0], want, scale, B * Ho * Wo)


def test_both_packs_in_one_launch_equal_the_single_packs(cases):
    shp = D.SHAPES[2]
    B, Cc, Oc, H, W = shp
    w = cases[shp]["w"].to(DEV)
    L = _lib.lib()
    nb = L.srbh_wpack2x2_bytes(Oc, 4 * Cc)
    assert nb == (4 * Cc // 32) * 8 * (Oc // 32) * 1024 == L.srbh_wpack2x2_bytes(4 * Cc, Oc)
    a, b = torch.zeros(nb, dtype=torch.uint8, device=DEV), torch.zeros(nb, dtype=torch.uint8, device=DEV)
    _lib.check(L.srbh_pack_conv4x4s2_pair(w.data_ptr(), Oc, Cc, a.data_ptr(), b.data_ptr(), sp()), "pack pair")
    torch.cuda.synchronize()
    assert torch.equal(a, pack(w, 0, 0)) and torch.equal(b, pack(w, 1, 1))


def test_entry_points_refuse_what_they_cannot_run():
    L = _lib.lib()
    gb = G.GuardedBuffers()
    planes = gb.out((1 << 16,), dtype=torch.uint8)
    out = gb.out((1 << 14,))
    x = torch.zeros(1 << 14, device=DEV)
    with pytest.raises(RuntimeError, match="srbh_s2d_nhwc32_to_act16: C must be a positive multiple of 32"):
        _lib.check(L.srbh_s2d_nhwc32_to_act16(x.data_ptr(), planes.data_ptr(), 1, 16, 8, 8, 0, sp()), "s2d")
    with pytest.raises(RuntimeError, match="srbh_s2d_nhwc32_to_act16: H and W must be even"):
        _lib.check(L.srbh_s2d_nhwc32_to_act16(x.data_ptr(), planes.data_ptr(), 1, 32, 7, 8, 0, sp()), "s2d")
    with pytest.raises(RuntimeError, match="srbh_d2s_nhwc32: H and W must be even"):
        _lib.check(L.srbh_d2s_nhwc32(x.data_ptr(), out.data_ptr(), 1, 32, 7, 8, sp()), "d2s")
    with pytest.raises(RuntimeError, match="srbh_pack_conv4x4s2: O and C must be positive multiples of 32"):
        _lib.check(L.srbh_pack_conv4x4s2(x.data_ptr(), 64, 16, 0, 0, planes.data_ptr(), sp()), "pack")
    with pytest.raises(RuntimeError, match="srbh_wconv2x2: cout must be a multiple of 64"):
        wconv2x2(planes, 32, planes, 96, 1, 4, 4, 0, out=out)
    with pytest.raises(RuntimeError, match="srbh_wconv2x2: null input / weight / out32 pointer"):
        wconv2x2(planes, 32, planes, 64, 1, 4, 4, 0)
    with pytest.raises(RuntimeError, match="srbh_wconv2x2: no bias"):
        wconv2x2(planes, 32, planes, 64, 1, 4, 4, 0, out=out, relu=1)
    with pytest.raises(RuntimeError, match="srbh_wconv2x2: input chunk range"):
        wconv2x2(planes, 32, planes, 64, 1, 4, 4, 0, out=out, in_chunks=0)
    with pytest.raises(RuntimeError, match="srbh_wgrad4x4s2_b16: cout must be a multiple of 64"):
        _lib.check(L.srbh_wgrad4x4s2_b16(planes.data_ptr(), planes.data_ptr(), 1, 32, 96, 4, 4, out.data_ptr(), out.data_ptr(), sp()), "wgrad")
    with pytest.raises(RuntimeError, match="srbh_wgrad4x4s2_b16: C must be a positive multiple of 32"):
        _lib.check(L.srbh_wgrad4x4s2_b16(planes.data_ptr(), planes.data_ptr(), 1, 16, 64, 4, 4, out.data_ptr(), out.data_ptr(), sp()), "wgrad")
    assert L.srbh_wgrad4x4s2_ws_bytes(96 + 8, 32, 1, 4, 4) == 0 and L.srbh_wpack2x2_bytes(0, 32) == 0
    gb.verify(written=False)                                 # no launch happened


def _graph_has(fn, name, seen=None):
    seen = set() if seen is None else seen
    if fn is None or fn in seen:
        return False
    seen.add(fn)
    return name in type(fn).__name__ or any(_graph_has(f, name, seen) for f, _ in fn.next_functions)


def test_module_on_libsrbh_matches_the_stock_graph_in_float64(golden_dir):
    """as tests/test_sr_stage.py's discriminator test, with its thresholds: UNetDiscriminatorSN(3, num_feat=32).train() with libsrbh = "f16" and
    libsrbh_s2 = "f16" on the device against the stock graph in float64 on the CPU from the same state; the new Function really ran; the
    num_feat = 8 fixture net (8 / 16 / 32 input channels: below the 64 the module asks for) keeps the stock op and matches g14 `disc_out`.
    At num_feat = 32 conv1 (32 -> 64) keeps the stock op as well; conv2 (64 -> 128) and conv3 (128 -> 256) take the new path."""
    import os
    from srbh_amd.srgan import UNetDiscriminatorSN
    from tests.test_sr_stage import rand
    torch.manual_seed(5)
    base = UNetDiscriminatorSN(3, num_feat=32, skip_connection=True).train()
    x0, wgt = rand((2, 3, 64, 64), 7, 0.0, 1.0), rand((2, 1, 64, 64), 8)
    res = {}
    for mode in ("cpu64", "s2"):
        m = copy.deepcopy(base)
        if mode == "cpu64":
            m, x, w_ = m.double(), x0.double().clone().requires_grad_(True), wgt.double()
        else:
            m = m.to(DEV)
            m.libsrbh = m.libsrbh_s2 = "f16"
            x, w_ = x0.to(DEV).clone().requires_grad_(True), wgt.to(DEV)
        y = m(x)
        if mode == "s2":
            assert _graph_has(y.grad_fn, "DiscConvS2")
        (y * w_).sum().backward()
        res[mode] = (y.detach().cpu().float(), x.grad.cpu().float(), {k: p.grad.cpu().float() for k, p in m.named_parameters() if p.grad is not None})
    cos = lambda a, b: float((a.double() * b.double()).sum() / (a.double().norm() * b.double().norm()).clamp_min(1e-300))   # noqa: E731
    (y0, gx0, g0), (y1, gx1, g1) = res["cpu64"], res["s2"]
    assert len(g0) == 12 and set(g1) == set(g0)
    print(f"[disc_s2] module: output rel-L2 {O.rel_l2(y1, y0):.3e}, input-gradient cosine {cos(gx1, gx0):.6f}, "
          f"smallest parameter-gradient cosine {min(cos(g1[k], g0[k]) for k in g0):.6f}")
    assert O.rel_l2(y1, y0) <= 5e-3 and cos(gx1, gx0) >= 0.99
    for k in g0:
        assert cos(g1[k], g0[k]) >= 0.99, (k, cos(g1[k], g0[k]))
    g = np.load(os.path.join(golden_dir, "g14_sr_stage.npz"))
    d = UNetDiscriminatorSN(3, num_feat=8, skip_connection=True).eval()
    d.load_state_dict({k[len("disc_sd_"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("disc_sd_")}, strict=True)
    d = d.to(DEV)
    d.libsrbh_s2 = "f16"
    xin = rand((2, 3, 32, 32), 143, 0.0, 1.0).to(DEV).requires_grad_(True)
    y = d(xin)
    assert not _graph_has(y.grad_fn, "DiscConvS2")
    assert O.rel_l2(y.detach().cpu(), torch.from_numpy(g["disc_out"])) <= 2e-5


def test_trainer_runs_the_convs_on_libsrbh(monkeypatch):
    """RealESRGAN(is_train=True) with SRBH_SR_DISC_S2=libsrbh in the `mixed` mode: four iterations on the 128x128 pair of tests/test_sr_stage.py;
    loss_dict keys as upstream, every value finite, the mode set; with the variable unset the attribute is None after an iteration"""
    from srbh_amd import rrdbnet_autograd as RA
    from srbh_amd.rrdbnet import RealESRGAN
    from tests.test_sr_stage import rand
    RA.set_train_precision("mixed")
    try:
        torch.manual_seed(3)
        m = RealESRGAN(3, 3, num_block=1, device=DEV, is_train=True)
        gt = torch.nn.functional.interpolate(rand((2, 3, 16, 16), 9, 0.0, 1.0), scale_factor=8, mode="bilinear")
        lq = torch.nn.functional.avg_pool2d(gt, 4)
        monkeypatch.setenv("SRBH_SR_DISC_S2", "libsrbh")
        for it in range(4):
            m.feed_data({"lq": lq, "gt": gt})
            ld = m.optimize_parameters()
            assert list(ld) == ["l_g_pix", "l_g_gan", "l_d_real", "out_d_real", "l_d_fake", "out_d_fake"]
            assert all(v == v and abs(v) != float("inf") for v in ld.values()), ld
            assert m.net_d.libsrbh_s2 == "f16"
        monkeypatch.delenv("SRBH_SR_DISC_S2")
        m.feed_data({"lq": lq, "gt": gt})
        ld = m.optimize_parameters()
        assert m.net_d.libsrbh_s2 is None and all(v == v for v in ld.values())
    finally:
        RA.set_train_precision("f32")
