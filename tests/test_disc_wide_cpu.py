"""The discriminator's wide 3x3 convs with LeakyReLU on ACT16 planes, without a device: the products of
tests/disc_wide_oracle.py against F.conv2d(padding=1) + F.leaky_relu(0.2) and their autograd in float64 (they pin the helper the GPU tests
compare the kernels with), the adjoint definition of Wt, the new exports of the built library, and UNetDiscriminatorSN.libsrbh_wide: default
None, no change of the module list or the state_dict, CPU tensors on stock ops whatever the attribute says, an unknown mode refused."""
import copy

import pytest
import torch
import torch.nn.functional as F

from tests import disc_wide_oracle as D

NEW_SYMBOLS = ("srbh_wconv3x3_lrelu", "srbh_nhwc32_to_act16_lrelu_bwd", "srbh_pack_conv3x3_pair", "srbh_wgrad3x3_b16", "srbh_wgrad3x3_ws_bytes",
               "srbh_wgrad3x3_walkers_cap")


@pytest.mark.parametrize("B,C,O,H,W", D.SHAPES)
def test_the_unrounded_products_are_conv_lrelu_and_its_autograd(B, C, O, H, W):
    g = torch.Generator()
    g.manual_seed(B * 1000 + C + H)
    x = torch.randn(B, C, H, W, dtype=torch.float64, generator=g).requires_grad_(True)
    w = (torch.randn(O, C, 3, 3, dtype=torch.float64, generator=g) * 0.05).requires_grad_(True)
    y = F.leaky_relu(F.conv2d(x, w, padding=1), 0.2)
    gy = torch.randn(y.shape, dtype=torch.float64, generator=g)
    y.backward(gy)
    xd, wd = x.detach(), w.detach()
    y2, scale = D.forward(xd, wd, rounded=False)
    assert y2.shape == y.shape and float((y2 - y.detach()).abs().max()) <= 1e-12 * 9 * C and bool((scale >= y2.abs() - 1e-12).all())
    gp = torch.where(y.detach() > 0, gy, gy * 0.2)              # (float64: the rule D.gprime states in fp32)
    dx, _ = D.dgrad(gp, wd, rounded=False)
    dw, _ = D.wgrad(xd, gp, rounded=False)
    assert dx.shape == x.shape and dw.shape == w.shape
    assert float((dx - x.grad).abs().max()) <= 1e-12 * 9 * O      # float64 sums of 9 O (B H W) terms of O(1) in another order
    assert float((dw - w.grad).abs().max()) <= 1e-12 * B * H * W


def test_wt_is_the_adjoint():
    g = torch.Generator()
    g.manual_seed(2)
    w = torch.randn(64, 32, 3, 3, dtype=torch.float64, generator=g)
    x = torch.randn(2, 32, 7, 9, dtype=torch.float64, generator=g)
    r = torch.randn(2, 64, 7, 9, dtype=torch.float64, generator=g)
    Wt = D.wt(w)
    assert Wt.shape == (32, 64, 3, 3) and float(Wt[5, 7, 0, 2]) == float(w[7, 5, 2, 0])
    lhs = (F.conv2d(x, w, padding=1) * r).sum()
    rhs = (x * F.conv2d(r, Wt, padding=1)).sum()
    assert abs(float(lhs - rhs)) <= 1e-9                         # <conv(x, w), r> = <x, conv(r, Wt)>


def test_rounded_products_use_the_contract_operands():
    B, C, O, H, W = D.SHAPES[4]
    g = torch.Generator()
    g.manual_seed(1)
    x, w = torch.randn(B, C, H, W, generator=g), torch.randn(O, C, 3, 3, generator=g) * 0.1
    y, _ = D.forward(x, w)
    z = F.conv2d(x.half().double(), w.half().double(), padding=1)
    assert float((y - torch.where(z >= 0, z, z * D.SLOPE32)).abs().max()) <= 1e-12 and abs(D.SLOPE32 - 0.2) < 2.0 ** -26
    gy = torch.randn(B, O, H, W, generator=g)
    gp = D.gprime(gy, y.float())
    assert gp.dtype == torch.float32 and torch.equal(gp, torch.where(y.float() > 0, gy, gy * 0.2))
    dw, _ = D.wgrad(x, gp)
    want = torch.nn.grad.conv2d_weight(x.half().float().bfloat16().double(), w.shape, gp.bfloat16().double(), padding=1)
    assert float((dw - want).abs().max()) <= 1e-10


def test_the_built_library_exports_the_new_entries():
    from srbh_amd import _lib
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and getattr(L, name) is not None, name
    assert L.srbh_wgrad3x3_ws_bytes(64, 64, 1, 8, 64) > 0 and L.srbh_wgrad3x3_ws_bytes(96, 64, 1, 8, 64) == 0
    assert L.srbh_wgrad3x3_ws_bytes(64, 48, 1, 8, 64) == 0
    # the walker cap: returns the previous value, shrinks the workspace of a many-tile shape, 0 restores the default
    full = L.srbh_wgrad3x3_ws_bytes(64, 64, 2, 24, 136)
    assert L.srbh_wgrad3x3_walkers_cap(D.CAP) == 0
    try:
        assert L.srbh_wgrad3x3_ws_bytes(64, 64, 2, 24, 136) == D.CAP * 2 * 9 * 64 * 32 * 4 < full
    finally:
        assert L.srbh_wgrad3x3_walkers_cap(0) == D.CAP
    assert L.srbh_wgrad3x3_ws_bytes(64, 64, 2, 24, 136) == full


def _run(m, x0):
    x = x0.clone().requires_grad_(True)
    y = m(x)
    y.square().sum().backward()
    return y.detach(), x.grad, {k: p.grad for k, p in m.named_parameters()}


def test_the_attribute_is_off_by_default_and_changes_nothing_on_the_cpu():
    from srbh_amd.srgan import UNetDiscriminatorSN
    assert UNetDiscriminatorSN.libsrbh_wide is None
    torch.manual_seed(5)
    base = UNetDiscriminatorSN(3, num_feat=64, skip_connection=True).train()
    assert base.libsrbh_wide is None
    a, b = copy.deepcopy(base), copy.deepcopy(base)
    b.libsrbh_wide = "f16"
    assert [n for n, _ in a.named_modules()] == [n for n, _ in b.named_modules()]
    assert list(a.state_dict()) == list(b.state_dict()) and list(b.state_dict()) == list(base.state_dict())
    g = torch.Generator()
    g.manual_seed(7)
    x0 = torch.rand(1, 3, 16, 16, generator=g)
    ya, gxa, ga = _run(a, x0)
    yb, gxb, gb = _run(b, x0)
    assert torch.equal(ya, yb) and torch.equal(gxa, gxb)
    assert len(ga) == 12
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k


def test_an_unknown_mode_is_refused():
    from srbh_amd.srgan import UNetDiscriminatorSN
    m = UNetDiscriminatorSN(3, num_feat=8)
    m.libsrbh_wide = "bf16"
    with pytest.raises(ValueError, match="libsrbh_wide: unknown mode 'bf16'"):
        m(torch.zeros(1, 3, 16, 16))
