"""The discriminator's wide 3x3 convs with LeakyReLU on libsrbh (csrc/srbh_disc3.hip, UNetDiscriminatorSN.libsrbh_wide = "f16"): the masked
gradient staging and the pair pack bit for bit, the three products through the C ABI, argument checks, the module and the trainer.

Products are compared with the float64 product of the SAME rounded operands (tests/disc_wide_oracle.py) under the derived elementwise bound
    |r - r64| <= K 2^-23 conv(|a|, |b|),     K = addends per output element (forward 9 Cin, data gradient 9 Cout, weight gradient B H W):
products of two 16-bit operands are exact in fp32, any summation tree of K fp32 additions stays inside K u, and u is taken as 2^-23 because the
matrix unit's internal accumulation is not documented as round-to-nearest per addition.  The forward adds 2^-23 |y64| for the one fp32 product
of the LeakyReLU (which is 1-Lipschitz: a sign flip near 0 stays inside the bound).  Every element is compared.  The largest observed ratio
(error / bound) per product is printed; measured on an MI355X over the six shapes: forward 1.5e-3, data gradient 3.0e-3, weight gradient
1.5e-2 (at K = 64; 2.7e-5 at K = 6528, 4.8e-5 there with four walkers), the witness srbh_act16_wgrad_b16 1.4e-2."""
import copy
import ctypes as C

import pytest
import torch

from oracle import srbh_oracle as O
from srbh_amd import _lib
from tests import disc_wide_oracle as D
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


def stage_x(x):
    """x (B, C, H, W) on the device -> fp16 planes, as the forward stages them"""
    return G.act16_from_nchw_x16(x, bf16=0)


def stage_gp(g, y, buf=None):
    """bf16 planes of g * (y > 0 ? 1 : 0.2) through the masked staging"""
    B, Oc, H, W = g.shape
    buf = G.act16_alloc(B, Oc // 32, H, W, DEV) if buf is None else buf
    gn, yn = nhwc(g), nhwc(y)                                  # (both alive until the call is issued)
    _lib.check(_lib.lib().srbh_nhwc32_to_act16_lrelu_bwd(gn.data_ptr(), yn.data_ptr(), buf.data_ptr(), B, Oc, H, W, 0.2, 1, sp()), "lrelu_bwd staging")
    torch.cuda.synchronize()
    return buf


def wconv(entry, planes, cin, wp, cout, B, H, W, bf, out=None, **kw):
    a = _lib.WConvArgs()
    a.in_, a.in_chunks_total, a.in_chunk0, a.in_chunks = planes.data_ptr(), cin // 32, 0, cin // 32
    a.w, a.cout, a.B, a.H, a.W, a.bf16 = wp.data_ptr(), cout, B, H, W, bf
    if out is not None:
        a.out32, a.out32_c = out.data_ptr(), cout
    for k, v in kw.items():
        setattr(a, k, v)
    _lib.check(getattr(_lib.lib(), entry)(C.byref(a), sp()), entry)
    torch.cuda.synchronize()


def wgrad3x3(X, Gp, shp, dw, ws):
    B, Cc, Oc, H, W = shp
    _lib.check(_lib.lib().srbh_wgrad3x3_b16(X.data_ptr(), Cc // 32, Cc, Gp.data_ptr(), Oc // 32, Oc, B, H, W, dw.data_ptr(), ws.data_ptr(), sp()), "wgrad3x3_b16")


@pytest.fixture(scope="module")
def cases():
    """per shape: fp32 x, w, g and a saved output ys (with +0 and -0 entries) on the CPU, g' = g * (ys > 0 ? 1 : 0.2), and the three float64
    products with their bound scales -- computed once, never modified"""
    out = {}
    for shp in D.SHAPES:
        B, Cc, Oc, H, W = shp
        gen = torch.Generator()
        gen.manual_seed(Cc * 7 + H)
        x = torch.randn(B, Cc, H, W, generator=gen)
        w = torch.randn(Oc, Cc, 3, 3, generator=gen) * 0.05
        g = torch.randn(B, Oc, H, W, generator=gen)
        ys = torch.randn(B, Oc, H, W, generator=gen)
        ys.view(-1)[::7] = 0.0
        ys.view(-1)[3::11] = -0.0
        gp = D.gprime(g, ys)
        out[shp] = dict(x=x, w=w, g=g, ys=ys, gp=gp, fwd=D.forward(x, w), dx=D.dgrad(gp, w), dw=D.wgrad(x, gp))
    return out


def check_bound(name, got, want, bound):
    got = got.double()
    err = (got - want).abs()
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"[disc_wide] {name}: max |err| {float(err.max()):.3e}, largest err / bound {ratio:.3e}")
    assert bool((err <= bound).all()), (name, ratio)
    return ratio


@pytest.mark.parametrize("shp", D.SHAPES)
def test_masked_staging_is_bit_exact(shp, cases):
    B, Cc, Oc, H, W = shp
    c = cases[shp]
    g, ys = c["g"].to(DEV), c["ys"].to(DEV)
    assert bool((ys == 0).any()) and bool(torch.signbit(ys[ys == 0]).any()) and not bool(torch.signbit(ys[ys == 0]).all())
    want = torch.where(ys > 0, g, g * 0.2).to(torch.bfloat16)            # fp32 on the device, torch's leaky_relu backward rule
    assert same_bits(want, c["gp"].to(torch.bfloat16))
    buf = stage_gp(g, ys)
    assert same_bits(G.act16_planes(buf, B, Oc // 32, H, W, torch.bfloat16), want)
    assert G.border_is_zero(buf, B, Oc // 32, H, W)
    # a used buffer: the interior is rewritten in full, the border kept
    G.act16_raw(buf, B, Oc // 32, H, W, torch.int16)[:, :, 1:-1, 1:-1] = 0x3F80
    stage_gp(g, ys, buf)
    assert same_bits(G.act16_planes(buf, B, Oc // 32, H, W, torch.bfloat16), want)
    assert G.border_is_zero(buf, B, Oc // 32, H, W)


@pytest.mark.parametrize("shp", D.SHAPES)
def test_both_packs_in_one_launch_equal_the_single_packs(shp, cases):
    B, Cc, Oc, H, W = shp
    w = cases[shp]["w"].to(DEV)
    L = _lib.lib()
    nb = L.srbh_wpack16_bytes(Oc, Cc)
    assert nb == L.srbh_wpack16_bytes(Cc, Oc)
    gb = G.GuardedBuffers()
    a, b = gb.out((nb,), dtype=torch.uint8), gb.out((nb,), dtype=torch.uint8)
    _lib.check(L.srbh_pack_conv3x3_pair(w.data_ptr(), Oc, Cc, a.data_ptr(), b.data_ptr(), sp()), "pack pair")
    gb.verify()
    assert torch.equal(a, G.pack_w(w)) and torch.equal(b, G.pack_w_b16(D.wt(w)))


@pytest.mark.parametrize("shp", D.SHAPES)
def test_forward_product_with_leaky_relu(shp, cases):
    B, Cc, Oc, H, W = shp
    c = cases[shp]
    gb = G.GuardedBuffers()
    out = gb.out((B, H, W, Oc))
    wconv("srbh_wconv3x3_lrelu", stage_x(c["x"].to(DEV)), Cc, G.pack_w(c["w"].to(DEV)), Oc, B, H, W, 0, out=out)
    gb.verify()
    want, scale = c["fwd"]
    assert bool((want < 0).any()) and bool((want > 0).any())
    check_bound(f"forward {shp}", out.permute(0, 3, 1, 2).cpu(), want, 9 * Cc * U * scale + U * want.abs())
    # without the LeakyReLU form the same call gives the pre-activation: srbh_wconv3x3 is what it was
    pre = torch.empty((B, H, W, Oc), device=DEV)
    wconv("srbh_wconv3x3", stage_x(c["x"].to(DEV)), Cc, G.pack_w(c["w"].to(DEV)), Oc, B, H, W, 0, out=pre)
    assert torch.equal(torch.where(pre >= 0, pre, pre * 0.2), out)


@pytest.mark.parametrize("shp", D.SHAPES)
def test_data_gradient_product(shp, cases):
    B, Cc, Oc, H, W = shp
    c = cases[shp]
    gb = G.GuardedBuffers()
    dx = gb.out((B, H, W, Cc))
    Gp = stage_gp(c["g"].to(DEV), c["ys"].to(DEV))
    wconv("srbh_wconv3x3", Gp, Oc, G.pack_w_b16(D.wt(c["w"]).to(DEV)), Cc, B, H, W, 1, out=dx)
    gb.verify()
    want, scale = c["dx"]
    check_bound(f"data gradient {shp}", dx.permute(0, 3, 1, 2).cpu(), want, 9 * Oc * U * scale)


def _wgrad_twice(shp, c):
    """two calls, the workspace pre-filled with NaN and with 3.0 (it needs no initialisation); dw and ws inside guards"""
    B, Cc, Oc, H, W = shp
    L = _lib.lib()
    X, Gp = stage_x(c["x"].to(DEV)), stage_gp(c["g"].to(DEV), c["ys"].to(DEV))
    nws = L.srbh_wgrad3x3_ws_bytes(Oc, Cc, B, H, W)
    assert nws > 0 and nws % 4 == 0
    res = []
    for fill in (float("nan"), 3.0):
        gb = G.GuardedBuffers()
        dw = gb.out((Oc, Cc, 3, 3))
        ws = gb.out((nws // 4,), fill=torch.full((nws // 4,), fill))
        wgrad3x3(X, Gp, shp, dw, ws)
        gb.verify()                                          # (every workspace slot is written, none beyond)
        res.append(dw.cpu().clone())
    assert torch.equal(res[0], res[1])
    return res[0], X, Gp


@pytest.mark.parametrize("shp", D.SHAPES)
def test_weight_gradient_product_determinism_and_second_witness(shp, cases):
    B, Cc, Oc, H, W = shp
    c = cases[shp]
    L = _lib.lib()
    want, scale = c["dw"]
    bound = B * H * W * U * scale
    dw, X, Gp = _wgrad_twice(shp, c)
    check_bound(f"weight gradient {shp}", dw, want, bound)
    # the independent witness: srbh_act16_wgrad_b16 (the 16 x 16 block kernel of the trunk's training path) in slices of <= 64 output channels
    parts = []
    for lo in range(0, Oc, 64):
        n = min(64, Oc - lo)
        d = torch.empty((n, Cc, 3, 3), device=DEV)
        ws = torch.empty(L.srbh_hwgrad_ws_bytes(n, Cc, 3) // 4, device=DEV)
        _lib.check(L.srbh_act16_wgrad_b16(X.data_ptr(), Cc // 32, Cc, Gp.data_ptr(), Oc // 32, lo, n, B, H, W, d.data_ptr(), ws.data_ptr(), sp()), "act16_wgrad_b16")
        parts.append(d)
    torch.cuda.synchronize()
    check_bound(f"weight gradient, witness {shp}", torch.cat(parts, 0).cpu(), want, bound)


def test_weight_gradient_with_an_uneven_tile_walk(cases):
    """18 tiles over 4 walkers: workgroups take 5, 5, 4 and 4 tiles.  Inside the bound like the uncapped run; the two need not be bit-equal
    (another summation order)."""
    shp = D.CAPPED
    B, Cc, Oc, H, W = shp
    c = cases[shp]
    L = _lib.lib()
    want, scale = c["dw"]
    full = L.srbh_wgrad3x3_ws_bytes(Oc, Cc, B, H, W)
    assert L.srbh_wgrad3x3_walkers_cap(D.CAP) == 0
    try:
        assert L.srbh_wgrad3x3_ws_bytes(Oc, Cc, B, H, W) * 18 == full * D.CAP
        dw, _, _ = _wgrad_twice(shp, c)
    finally:
        assert L.srbh_wgrad3x3_walkers_cap(0) == D.CAP
    check_bound(f"weight gradient, {D.CAP} walkers {shp}", dw, want, B * H * W * U * scale)


def test_entry_points_refuse_what_they_cannot_run():
    L = _lib.lib()
    gb = G.GuardedBuffers()
    planes = gb.out((1 << 16,), dtype=torch.uint8)
    out = gb.out((1 << 14,))
    x = torch.zeros(1 << 16, device=DEV)
    P, Op, X = planes.data_ptr(), out.data_ptr(), x.data_ptr()
    with pytest.raises(RuntimeError, match="srbh_wgrad3x3_b16: cin must be a positive multiple of 32"):
        _lib.check(L.srbh_wgrad3x3_b16(X, 2, 48, X, 2, 64, 1, 4, 4, Op, Op, sp()), "wgrad")
    with pytest.raises(RuntimeError, match="srbh_wgrad3x3_b16: cout must be 32 or a multiple of 64"):
        _lib.check(L.srbh_wgrad3x3_b16(X, 2, 64, X, 3, 96, 1, 4, 4, Op, Op, sp()), "wgrad")
    with pytest.raises(RuntimeError, match="srbh_wgrad3x3_b16: null pointer"):
        _lib.check(L.srbh_wgrad3x3_b16(X, 2, 64, X, 2, 64, 1, 4, 4, None, Op, sp()), "wgrad")
    with pytest.raises(RuntimeError, match="srbh_wgrad3x3_b16: null pointer"):
        _lib.check(L.srbh_wgrad3x3_b16(None, 2, 64, X, 2, 64, 1, 4, 4, Op, Op, sp()), "wgrad")
    with pytest.raises(RuntimeError, match="srbh_wgrad3x3_b16: channel ranges outside"):
        _lib.check(L.srbh_wgrad3x3_b16(X, 1, 64, X, 2, 64, 1, 4, 4, Op, Op, sp()), "wgrad")
    with pytest.raises(RuntimeError, match="srbh_nhwc32_to_act16_lrelu_bwd: C must be a positive multiple of 32"):
        _lib.check(L.srbh_nhwc32_to_act16_lrelu_bwd(X, X, P, 1, 16, 4, 4, 0.2, 1, sp()), "staging")
    with pytest.raises(RuntimeError, match="srbh_nhwc32_to_act16_lrelu_bwd: null pointer"):
        _lib.check(L.srbh_nhwc32_to_act16_lrelu_bwd(X, None, P, 1, 32, 4, 4, 0.2, 1, sp()), "staging")
    with pytest.raises(RuntimeError, match="srbh_pack_conv3x3_pair: cout and cin must be positive multiples of 32"):
        _lib.check(L.srbh_pack_conv3x3_pair(X, 48, 32, P, P, sp()), "pack")
    with pytest.raises(RuntimeError, match="srbh_pack_conv3x3_pair: null pointer"):
        _lib.check(L.srbh_pack_conv3x3_pair(X, 32, 32, P, None, sp()), "pack")
    with pytest.raises(RuntimeError, match="srbh_wconv3x3_lrelu: cout must be 32 or a multiple of 64"):
        wconv("srbh_wconv3x3_lrelu", planes, 32, planes, 96, 1, 4, 4, 0, out=out)
    with pytest.raises(RuntimeError, match="srbh_wconv3x3_lrelu: no bias"):
        wconv("srbh_wconv3x3_lrelu", planes, 32, planes, 64, 1, 4, 4, 0, out=out, relu=1)
    with pytest.raises(RuntimeError, match="srbh_wconv3x3_lrelu: no output requested"):
        wconv("srbh_wconv3x3_lrelu", planes, 32, planes, 64, 1, 4, 4, 0)
    assert L.srbh_wgrad3x3_ws_bytes(96, 32, 1, 4, 4) == 0 and L.srbh_wgrad3x3_ws_bytes(64, 48, 1, 4, 4) == 0
    gb.verify(written=False)                                 # no launch happened


def _graph_has(fn, name, seen=None):
    seen = set() if seen is None else seen
    if fn is None or fn in seen:
        return False
    seen.add(fn)
    return name in type(fn).__name__ or any(_graph_has(f, name, seen) for f, _ in fn.next_functions)


def test_module_is_as_close_to_float64_as_the_path_it_replaces():
    """UNetDiscriminatorSN(3, num_feat=64).train(), batch 2, 32 x 32, with libsrbh = libsrbh_s2 = libsrbh_wide = "f16" on the device against the
    stock graph in float64 on the CPU from the same state.  The yardstick is the parent's path -- libsrbh = libsrbh_s2 = "f16", libsrbh_wide
    unset -- measured here against the same float64 graph: output rel-L2 and 1 - cosine of the input gradient and of every parameter gradient
    must be at most 2 x its value (same operand precision; the differences are summation order and the fp16 -> bf16 double rounding of x in the
    weight gradient).  state_dict keys are unchanged; a conv carrying a foreign forward hook falls back.
    Measured on an MI355X, wide (parent's path): output rel-L2 9.078e-4 (9.089e-4); input gradient 1 - cos 2.089e-4 (2.042e-4); parameter
    gradients 1 - cos: conv0.weight 2.226e-4 (2.453e-4), conv0.bias 2.469e-4 (2.979e-4), conv1 1.741e-4 (1.858e-4), conv2 2.836e-4 (3.258e-4),
    conv3 3.886e-4 (3.951e-4), conv4 2.979e-4 (2.942e-4), conv5 2.575e-4 (2.758e-4), conv6 1.474e-4 (1.711e-4), conv7 1.655e-4 (1.573e-4),
    conv8 1.579e-4 (1.609e-4), conv9.weight 4.281e-7 (4.329e-7), conv9.bias 0 (0): the largest wide / parent ratio is 1.05."""
    from srbh_amd.srgan import UNetDiscriminatorSN
    from tests.test_sr_stage import rand
    torch.manual_seed(5)
    base = UNetDiscriminatorSN(3, num_feat=64, skip_connection=True).train()
    x0, wgt = rand((2, 3, 32, 32), 7, 0.0, 1.0), rand((2, 1, 32, 32), 8)
    res = {}
    for mode in ("cpu64", "parent", "wide"):
        m = copy.deepcopy(base)
        if mode == "cpu64":
            m, x, w_ = m.double(), x0.double().clone().requires_grad_(True), wgt.double()
        else:
            m = m.to(DEV)
            m.libsrbh = m.libsrbh_s2 = "f16"
            if mode == "wide":
                m.libsrbh_wide = "f16"
            x, w_ = x0.to(DEV).clone().requires_grad_(True), wgt.to(DEV)
        assert list(m.state_dict()) == list(base.state_dict())
        y = m(x)
        if mode != "cpu64":
            assert _graph_has(y.grad_fn, "DiscConvWide") == (mode == "wide")
        (y * w_).sum().backward()
        res[mode] = (y.detach().cpu().double(), x.grad.cpu().double(), {k: p.grad.cpu().double() for k, p in m.named_parameters() if p.grad is not None})
    omc = lambda a, b: 1.0 - float((a * b).sum() / (a.norm() * b.norm()).clamp_min(1e-300))   # noqa: E731
    y0, gx0, g0 = res["cpu64"]
    assert len(g0) == 12 and set(res["wide"][2]) == set(g0) == set(res["parent"][2])
    rows = [("output rel-L2", O.rel_l2(res["wide"][0], y0), O.rel_l2(res["parent"][0], y0)),
            ("input gradient 1-cos", omc(res["wide"][1], gx0), omc(res["parent"][1], gx0))]
    rows += [(f"{k} 1-cos", omc(res["wide"][2][k], g0[k]), omc(res["parent"][2][k], g0[k])) for k in g0]
    for name, wide, parent in rows:
        print(f"[disc_wide] module {name}: wide {wide:.3e}, parent path {parent:.3e}")
    bad = [(name, wide, parent) for name, wide, parent in rows if not wide <= 2.0 * parent]
    assert not bad, bad
    # a foreign forward hook on one conv: that conv takes the stock path with the full hook protocol, the others stay
    m = copy.deepcopy(base).to(DEV)
    m.libsrbh = m.libsrbh_s2 = m.libsrbh_wide = "f16"
    seen = []
    for k in (4, 5, 6, 7, 8):
        getattr(m, f"conv{k}").register_forward_hook(lambda mod, inp, out: seen.append(tuple(out.shape)))
    y = m(x0.to(DEV))
    assert len(seen) == 5 and not _graph_has(y.grad_fn, "DiscConvWide")


def test_trainer_runs_the_convs_on_libsrbh(monkeypatch):
    """RealESRGAN(is_train=True) with SRBH_SR_DISC_WIDE=libsrbh in the `mixed` mode: one iteration on the 128x128 pair of tests/test_sr_stage.py;
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
        monkeypatch.setenv("SRBH_SR_DISC_WIDE", "libsrbh")
        m.feed_data({"lq": lq, "gt": gt})
        ld = m.optimize_parameters()
        assert list(ld) == ["l_g_pix", "l_g_gan", "l_d_real", "out_d_real", "l_d_fake", "out_d_fake"]
        assert all(v == v and abs(v) != float("inf") for v in ld.values()), ld
        assert m.net_d.libsrbh_wide == "f16"
        monkeypatch.delenv("SRBH_SR_DISC_WIDE")
        m.feed_data({"lq": lq, "gt": gt})
        ld = m.optimize_parameters()
        assert m.net_d.libsrbh_wide is None and all(v == v for v in ld.values())
    finally:
        RA.set_train_precision("f32")
