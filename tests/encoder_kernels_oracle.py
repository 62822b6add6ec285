"""float64 stock-op restatement of the encoder's small kernels (csrc/srbh_dwconv.hip, csrc/srbh_enc_eval.hip, srbh_bn_eval_scale_shift)  --  TEST INFRASTRUCTURE ONLY.

One plain torch function per C-ABI entry point, evaluated in float64 on the CPU whatever the inputs' type, plus the launch
arithmetic of the depthwise dispatcher restated in Python (batch slices of the weight gradient, LDS byte counts of the staged
forms), so that the shape lists below can be held to the properties they were chosen for.  tests/test_encoder_kernels_cpu.py
pins this file against the stock float64 module chain; tests/test_gpu_encoder_kernels.py and tests/test_gpu_dwconv.py compare
the kernels with it.  No device code here.

Layouts as in include/srbh.h: x / y [B][C][...] (any trailing plane shape), scale / shift [C], pooled [B][C], w1 [SQ][C],
hidden [B][SQ], w2 [C][SQ], gate [B][C], depthwise w [C][1][K][K].  act: 0 none, 1 SiLU, 2 ReLU."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F


def _d(t):
    return t.detach().to("cpu", torch.float64)


def _per_channel(v, x):
    return _d(v).view(1, -1, *([1] * (x.dim() - 2)))


def affine_act(x, scale, shift, act, res=None):
    """srbh_affine_act_nchw / srbh_affine_act_add_nchw: act(x * scale[c] + shift[c]) (+ res)"""
    x = _d(x)
    u = x * _per_channel(scale, x) + _per_channel(shift, x)
    u = F.silu(u) if act == 1 else (F.relu(u) if act == 2 else u)
    return u if res is None else u + _d(res)


def affine_act_pool(x, scale, shift, act):
    """srbh_affine_act_pool_nchw: (y, pooled) with pooled[b][c] the mean of y's plane (b, c)"""
    y = affine_act(x, scale, shift, act)
    return y, y.flatten(2).mean(2)


def se_hidden(pooled, w1, b1):
    """srbh_se_hidden: swish(b1 + w1 . pooled[b])"""
    return F.silu(_d(pooled) @ _d(w1).flatten(1).t() + _d(b1))


def se_gate(hidden, w2, b2):
    """srbh_se_gate: sigmoid(b2 + w2 . hidden[b])"""
    return torch.sigmoid(_d(hidden) @ _d(w2).flatten(1).t() + _d(b2))


def se_gate_scale(y, hidden, w2, b2):
    """srbh_se_gate_scale: every plane (b, c) of y times its gate"""
    y = _d(y)
    g = se_gate(hidden, w2, b2)
    return y * g.view(*g.shape, *([1] * (y.dim() - 2)))


def bn_eval_scale_shift(weight, bias, mean, var, eps):
    """srbh_bn_eval_scale_shift: inference BatchNorm as (scale, shift); weight / bias None = 1 / 0"""
    invstd = 1.0 / torch.sqrt(_d(var) + eps)
    scale = invstd if weight is None else _d(weight) * invstd
    shift = -_d(mean) * scale
    return scale, (shift if bias is None else shift + _d(bias))


def dwconv(x, w, stride, pad):
    """srbh_dwconv_fwd: depthwise conv of the zero-padded input; pad = (left, right, top, bottom) as F.pad takes it.  Differentiable in
    x and w when they are float64 leaves (dwconv_grads)"""
    x = x if x.dtype == torch.float64 and x.requires_grad else _d(x)
    w = w if w.dtype == torch.float64 and w.requires_grad else _d(w)
    return F.conv2d(F.pad(x, pad), w, None, stride, 0, 1, x.shape[1])


def dwconv_grads(x, w, stride, pad, gy):
    """(y, dx, dw) of dwconv for the output gradient gy: srbh_dwconv_bwd_data / srbh_dwconv_bwd_weight through autograd on float64"""
    xr, wr = _d(x).requires_grad_(True), _d(w).requires_grad_(True)
    y = dwconv(xr, wr, stride, pad)
    dx, dw = torch.autograd.grad(y, (xr, wr), _d(gy))
    return y.detach(), dx, dw


def same_pad(size, K, stride):
    """TF-"same" padding of one axis as encoders.SamePadConv2d fixes it for a nominal input `size`: (before, after, output size)"""
    out = math.ceil(size / stride)
    total = max((out - 1) * stride + K - size, 0)
    return total // 2, total - total // 2, out


def same_geometry(H, W, K, stride):
    """((left, right, top, bottom), OH, OW) for an H x W plane"""
    pt, pb, OH = same_pad(H, K, stride)
    pl, pr, OW = same_pad(W, K, stride)
    return (pl, pr, pt, pb), OH, OW


# ---- the depthwise dispatcher's arithmetic (csrc/srbh_dwconv.hip: srbh_dwconv_bwd_weight_splits, lds_planes, the `lds` byte counts of
# ---- srbh_dwconv_fwd / _bwd_data / _bwd_weight against DW_LDS_MAX, grid_for) restated ----------------------------------------------
DW_LDS_MAX = 60 * 1024
GRID_CAP_ITEMS = 8192 * 256          # grid_for(): beyond this many work items the 256-thread workgroups take a second grid stride


def wgrad_splits(B, C):
    return max(1, min(B, (1024 + C - 1) // C))


def slice_bounds(B, splits):
    """[(b0, b1)] of the weight gradient's batch slices"""
    return [(B * s // splits, B * (s + 1) // splits) for s in range(splits)]


def lds_planes(out_px):
    return max(1, min(64, 256 // max(out_px, 1)))


def lds_bytes(which, H, W, K, stride, OH, OW):
    """bytes of LDS the staged form of `which` ("fwd", "dgrad", "wgrad") asks for; the dispatcher takes the one-thread-per-output kernel
    when this exceeds DW_LDS_MAX"""
    if which == "fwd":
        return lds_planes(OH * OW) * (((OH - 1) * stride + K) * ((OW - 1) * stride + K) + K * K) * 4
    if which == "dgrad":
        ph, pw = (OH - 1) * stride + 2 * (K - 1) + stride + 1, (OW - 1) * stride + 2 * (K - 1) + stride + 1
        return lds_planes(H * W) * (ph * pw + K * K) * 4
    assert which == "wgrad", which
    return lds_planes(OH * OW) * (((OH - 1) * stride + K) * ((OW - 1) * stride + K) + OH * OW) * 4


def staged(which, H, W, K, stride):
    """does the LDS-staged kernel take this plane under "same" padding (else: the one-thread-per-output kernel)"""
    _, OH, OW = same_geometry(H, W, K, stride)
    ok = lds_bytes(which, H, W, K, stride, OH, OW) <= DW_LDS_MAX
    if which == "wgrad":
        ok = ok and (K == 5 or OH * OW < 256)
    return ok


# ---- shape lists of tests/test_gpu_dwconv.py (B, C, H, W, K, stride), each with the property it is there for; tests/test_encoder_kernels_cpu.py
# ---- asserts that property from the arithmetic above --------------------------------------------------------------------------------
DW_SLICE_CASES = [
    ((70, 300, 8, 8, 5, 1), "multi_round"),        # 4 slices of 17 / 18 images, 4 planes per round: 5 rounds, the last with 1 or 2 planes
    ((70, 300, 16, 16, 3, 2), "multi_round"),
    ((70, 48, 4, 4, 3, 1), "uneven"),              # 22 slices of 3 or 4 images
    ((1, 37, 8, 8, 5, 1), "single_slice"),
    ((3, 1056, 2, 2, 3, 1), "single_slice"),
]

# either side of DW_LDS_MAX = 61 440 bytes (one plane per round at these sizes, B = 2, C = 3); which of the three staged forms still
# takes the plane.  The arithmetic is written out in tests/test_gpu_dwconv.py::test_depthwise_conv_either_side_of_the_lds_limit
DW_LIMIT_CASES = [
    ((2, 3, 117, 127, 3, 1), {"fwd": True, "dgrad": False, "wgrad": False}),
    ((2, 3, 114, 124, 3, 1), {"fwd": True, "dgrad": True, "wgrad": False}),
    ((2, 3, 122, 124, 3, 1), {"fwd": False, "dgrad": False, "wgrad": False}),
    ((2, 3, 114, 127, 5, 2), {"fwd": True, "dgrad": False, "wgrad": False}),
    ((2, 3, 107, 122, 5, 2), {"fwd": True, "dgrad": True, "wgrad": False}),
    ((2, 3, 96, 121, 5, 2), {"fwd": True, "dgrad": True, "wgrad": True}),
    ((2, 3, 98, 119, 5, 2), {"fwd": True, "dgrad": True, "wgrad": False}),
    ((2, 3, 122, 124, 5, 2), {"fwd": False, "dgrad": False, "wgrad": False}),
]

DW_WRAP_CASE = (3, 47, 122, 124, 3, 1)             # one-thread-per-output kernels, more outputs than one grid stride covers
