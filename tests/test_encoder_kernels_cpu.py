"""CPU: tests/encoder_kernels_oracle.py itself -- the float64 functions the GPU tests of csrc/srbh_dwconv.hip and csrc/srbh_enc_eval.hip compare against equal the
stock float64 module chain of encoders.MBConvBlock in eval mode, the depthwise reference equals the padded grouped conv under the
encoder's TF-"same" padding, and the shape lists of tests/test_gpu_dwconv.py have the slice / round / LDS-limit properties they were
chosen for.  No kernel is launched here (the kernels: tests/test_gpu_encoder_kernels.py, tests/test_gpu_dwconv.py)."""
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import encoder_kernels_oracle as O


def _maxrel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("B,C,SQ,H,W", [(2, 6, 3, 4, 5), (3, 17, 1, 7, 2)])
def test_oracle_chain_equals_the_stock_module_chain(B, C, SQ, H, W):
    """affine_act_pool -> se_hidden -> se_gate_scale (and the gate-only variant) == BatchNorm2d.eval() -> SiLU -> adaptive_avg_pool2d ->
    Conv2d 1x1 -> SiLU -> Conv2d 1x1 -> sigmoid -> multiply, all float64, to 1e-12"""
    g = torch.Generator().manual_seed(B * 100 + C)
    bn = nn.BatchNorm2d(C, eps=1e-3).double().eval()
    red, exp = nn.Conv2d(C, SQ, 1).double(), nn.Conv2d(SQ, C, 1).double()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g, dtype=torch.float64) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g, dtype=torch.float64) * 0.3)
        bn.running_mean.copy_(torch.randn(C, generator=g, dtype=torch.float64) * 0.4)
        bn.running_var.copy_(torch.rand(C, generator=g, dtype=torch.float64) + 0.1)
        red.weight.mul_(3.0)
        exp.weight.mul_(3.0)
        x = torch.randn((B, C, H, W), generator=g, dtype=torch.float64) * 1.5 + 0.4
        s = F.silu(bn(x))
        pooled_m = F.adaptive_avg_pool2d(s, 1)
        hidden_m = F.silu(red(pooled_m))
        gate_m = torch.sigmoid(exp(hidden_m))
        want = gate_m * s
    scale, shift = O.bn_eval_scale_shift(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
    y, pooled = O.affine_act_pool(x, scale, shift, 1)
    hidden = O.se_hidden(pooled, red.weight, red.bias)
    gate = O.se_gate(hidden, exp.weight, exp.bias)
    got = O.se_gate_scale(y, hidden, exp.weight, exp.bias)
    assert y.dtype == torch.float64 and got.shape == want.shape
    assert _maxrel(y, s) <= 1e-12 and _maxrel(pooled, pooled_m.flatten(1)) <= 1e-12
    assert _maxrel(hidden, hidden_m.flatten(1)) <= 1e-12 and _maxrel(gate, gate_m.flatten(1)) <= 1e-12
    assert _maxrel(got, want) <= 1e-12
    assert _maxrel(y * gate.view(B, C, 1, 1), want) <= 1e-12          # the gate-only variant: the caller multiplies
    # the other activations and the skip connection
    res = torch.randn(x.shape, generator=g, dtype=torch.float64)
    assert _maxrel(O.affine_act(x, scale, shift, 0, res), bn(x).detach() + res) <= 1e-12
    assert _maxrel(O.affine_act(x, scale, shift, 2), F.relu(bn(x)).detach()) <= 1e-12
    # fp32 inputs are taken to float64 before any arithmetic
    assert O.affine_act(x.float(), scale.float(), shift.float(), 1).dtype == torch.float64
    # a BatchNorm without affine parameters
    s1, h1 = O.bn_eval_scale_shift(None, None, bn.running_mean, bn.running_var, bn.eps)
    assert _maxrel(x * s1.view(1, -1, 1, 1) + h1.view(1, -1, 1, 1), F.batch_norm(x, bn.running_mean, bn.running_var, None, None, False, 0.0, bn.eps)) <= 1e-12


@pytest.mark.parametrize("K,stride", [(3, 1), (3, 2), (5, 1), (5, 2)])
def test_depthwise_oracle_equals_the_padded_grouped_conv(K, stride):
    """dwconv and its autograd gradients == F.conv2d(F.pad(x), groups = C) in float64 under the padding encoders.SamePadConv2d computes
    (even and odd sizes: an odd total pad at stride 2 puts the extra row / column at the bottom / right)"""
    from srbh_amd import encoders
    g = torch.Generator().manual_seed(K * 10 + stride)
    totals = set()
    for H, W in ((8, 8), (7, 10), (9, 6)):
        pad, OH, OW = O.same_geometry(H, W, K, stride)
        for size, lo, hi in ((W, pad[0], pad[1]), (H, pad[2], pad[3])):
            conv = encoders.SamePadConv2d(4, 4, K, size, stride=stride, groups=4, bias=False)
            assert conv._pad == (lo, hi, lo, hi) and conv._depthwise
            totals.add((lo + hi) % 2)
        x, w = torch.randn((2, 5, H, W), generator=g), torch.randn((5, 1, K, K), generator=g)          # fp32, as the GPU tests hand them over
        xf, wf = x.double().requires_grad_(True), w.double().requires_grad_(True)
        want = F.conv2d(F.pad(xf, pad), wf, None, stride, 0, 1, 5)
        assert want.shape == (2, 5, OH, OW) == (2, 5, math.ceil(H / stride), math.ceil(W / stride))
        gy = torch.randn(want.shape, generator=g)
        dx_w, dw_w = torch.autograd.grad(want, (xf, wf), gy.double())
        y, dx, dw = O.dwconv_grads(x, w, stride, pad, gy)
        assert y.dtype == dx.dtype == dw.dtype == torch.float64
        assert torch.equal(y, want.detach()) and torch.equal(dx, dx_w) and torch.equal(dw, dw_w)
        assert torch.equal(O.dwconv(x, w, stride, pad), want.detach())
    if stride == 2:
        assert totals == {0, 1}, totals          # both an even and an odd total pad were in the set


def test_slice_arithmetic_of_the_weight_gradient_cases():
    """splits = min(B, ceil(1024 / C)), slice s = images [B s // splits, B (s + 1) // splits): every shape tests/test_gpu_dwconv.py lists as
    multi-round, uneven or single-slice really is, and takes the LDS-staged weight-gradient kernel whose round loop it is there for"""
    seen = set()
    for (B, C, H, W, K, stride), prop in O.DW_SLICE_CASES:
        splits = O.wgrad_splits(B, C)
        assert splits == min(B, math.ceil(1024 / C))
        bounds = O.slice_bounds(B, splits)
        assert bounds[0][0] == 0 and bounds[-1][1] == B and all(a[1] == b[0] for a, b in zip(bounds, bounds[1:]))
        sizes = [b1 - b0 for b0, b1 in bounds]
        assert min(sizes) >= 1
        _, OH, OW = O.same_geometry(H, W, K, stride)
        P = O.lds_planes(OH * OW)
        assert O.staged("wgrad", H, W, K, stride), (B, C, H, W, K, stride)
        if prop == "multi_round":
            assert splits > 1 and P == 4
            assert all(n > P and n % P != 0 for n in sizes), sizes          # several rounds, the last one ragged
            assert len({n % P for n in sizes}) > 1, sizes                    # and not the same tail in every slice
        elif prop == "uneven":
            assert splits > 1 and set(sizes) == {3, 4} and max(sizes) <= P, (sizes, P)
        else:
            assert prop == "single_slice" and splits == 1 and sizes == [B]
        seen.add(prop)
    assert seen == {"multi_round", "uneven", "single_slice"}
    assert O.wgrad_splits(70, 300) == 4 and [b1 - b0 for b0, b1 in O.slice_bounds(70, 4)] == [17, 18, 17, 18]
    assert O.wgrad_splits(5, 37) == 5          # the ten long-standing geometries: one image per slice


def test_lds_limit_cases_sit_on_the_side_they_claim():
    """the planes of DW_LIMIT_CASES against the byte counts the dispatcher computes: each of forward, input gradient and K = 5 weight gradient
    has a plane just under (within 1 % of) and one over DW_LDS_MAX; the wrap case runs the one-thread-per-output kernels past one grid stride"""
    under, over = {}, {}
    for (B, C, H, W, K, stride), want in O.DW_LIMIT_CASES:
        assert H != W and (B, C) == (2, 3)
        _, OH, OW = O.same_geometry(H, W, K, stride)
        for which in ("fwd", "dgrad", "wgrad"):
            assert O.staged(which, H, W, K, stride) == want[which], (H, W, K, stride, which)
            if which == "wgrad" and K == 3:
                continue                                   # (3x3 over >= 256-pixel planes: never staged, whatever its size)
            n = O.lds_bytes(which, H, W, K, stride, OH, OW)
            d = under if n <= O.DW_LDS_MAX else over
            d[which] = min(d.get(which, 1 << 30), abs(n - O.DW_LDS_MAX))
    for which in ("fwd", "dgrad", "wgrad"):
        assert under[which] <= O.DW_LDS_MAX // 100, (which, under)
        assert which in over
    assert under["fwd"] == 0 and under["dgrad"] == 0       # a plane that needs exactly DW_LDS_MAX bytes is still staged
    assert over["wgrad"] == 12                             # three floats over
    B, C, H, W, K, stride = O.DW_WRAP_CASE
    assert not any(O.staged(which, H, W, K, stride) for which in ("fwd", "dgrad", "wgrad"))
    assert B * C * H * W > O.GRID_CAP_ITEMS
