"""Rounding-exact CPU emulation of the "f16x2" precision mode of the inference RRDBNet  --  TEST INFRASTRUCTURE ONLY.

The trunk is oracle.rrdbnet_emulation's (untouched); the tail (conv_body, conv_up1, conv_up2, conv_hr) follows the contract of
csrc/srbh_ptail_split.hip:

* an fp32 value v travels as ``hi = rne16(v)`` and ``lo' = rne16((v - hi) * 2^11)`` (fp16 both; the subtraction is exact in fp32);
  weights are split the same way;
* a conv is ``M = sum w_hi a_hi``, ``C = sum (w_hi a_lo' + w_lo' a_hi)``, ``y = fp32(M + C * 2^-11) + bias`` (fp32 registers; the order of
  the additions inside the sums is free: ``acc`` = float64 is the exact sum rounded once, float32 torch's CPU order), then ``+ feat``
  (conv_body) or LeakyReLU (up convs), then the fp32 result is split again; conv_hr's result leaves as fp32;
* conv_body's ``hi`` = the fp16 planes the trunk writes (= rne16 of its fp32 output stream), its ``lo'`` from that stream.

Switches for the attribution table of DESIGN.md section 4: ``split_w`` / ``split_a`` (False: that operand has no low part; both False is
oracle.rrdbnet_emulation.rrdbnet_emulated(..., "bf16") bit for bit), ``convs`` (which of the four convs are split), ``body_lo`` (False: conv_body
reads the trunk's planes without a low part), ``lo_scale`` (2^11; 1 = unscaled low parts), ``flush`` (every fp16-subnormal operand -> 0: what a
matrix core that flushed subnormal inputs would see).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import srbh_oracle as O
from oracle.rrdbnet_emulation import _f32, _q16, rrdbnet_emulated

TAIL = ("conv_body", "conv_up1", "conv_up2", "conv_hr")
LO_SCALE = 2048.0
F16_MIN_NORMAL = 2.0 ** -14


def rne16(t):
    """round to fp16 (RNE) and back, dtype kept"""
    return t.float().half().to(t.dtype)


def flush16(t):
    """fp16 subnormals -> 0 (t holds fp16 values)"""
    return torch.where(t.abs() < F16_MIN_NORMAL, torch.zeros_like(t), t)


def split16(v, lo_scale=LO_SCALE, flush=False):
    """(hi, lo') of fp32 values held in any float dtype"""
    v32 = v.float()
    hi = v32.half().float()
    lo = ((v32 - hi) * lo_scale).half().float()
    if flush:
        hi, lo = flush16(hi), flush16(lo)
    return hi.to(v.dtype), lo.to(v.dtype)


def split_conv(w, bias, a_hi, a_lo, acc=torch.float64, split_w=True, lo_scale=LO_SCALE, flush=False):
    """one tail conv of the contract on given operand planes (a_lo None: no low part of the activation): fp32 values in ``acc`` dtype,
    bias added, no epilogue"""
    w_hi, w_lo = split16(w.to(acc), lo_scale, flush)
    if flush:
        a_hi = flush16(a_hi)
        a_lo = None if a_lo is None else flush16(a_lo)
    m = F.conv2d(a_hi.to(acc), w_hi, None, 1, 1)
    c = None
    if a_lo is not None:
        c = F.conv2d(a_lo.to(acc), w_hi, None, 1, 1)
    if split_w:
        c2 = F.conv2d(a_hi.to(acc), w_lo, None, 1, 1)
        c = c2 if c is None else c + c2
    if c is not None:
        m = _f32(c) * (1.0 / lo_scale) + m if acc == torch.float32 else m + c * (1.0 / lo_scale)
    return _f32(_f32(m) + bias.to(acc).view(1, -1, 1, 1))


@torch.no_grad()
def trunk_and_feat(sd, x, trunk="bf16", acc=torch.float64):
    """(feat, xrr, planes): conv_first's fp32 output, the trunk's fp32 output stream and its fp16 planes, as the kernels hold them"""
    feat = _f32(F.conv2d(x.to(acc), sd["conv_first.weight"].to(acc), sd["conv_first.bias"].to(acc), 1, 1))
    xrr = rrdbnet_emulated(sd, x, trunk, acc=acc, stop="trunk").to(acc)
    return feat, xrr, _q16(xrr, "fp16")


@torch.no_grad()
def tail_split(sd, feat, xrr, planes, acc=torch.float64, split_w=True, split_a=True, convs=TAIL, body_lo=True, lo_scale=LO_SCALE, flush=False):
    one = torch.ones((), dtype=acc)
    S = _f32(one * 0.2)

    def lrelu(v):
        return torch.where(v >= 0, v, _f32(v * S))

    def conv(name, hi, lo):
        on = name in convs
        return split_conv(sd[name + ".weight"], sd[name + ".bias"], hi, lo if (on and split_a) else None, acc, on and split_w, lo_scale, flush)

    def planes_of(v):
        hi, lo = split16(v, lo_scale)
        return hi, lo

    lo0 = ((xrr.float() - planes.float()) * lo_scale).half().to(acc) if body_lo else None
    hi, lo = planes_of(_f32(conv("conv_body", planes, lo0) + feat))
    hi, lo = planes_of(lrelu(conv("conv_up1", O.nearest2x(hi), O.nearest2x(lo))))
    hi, lo = planes_of(lrelu(conv("conv_up2", O.nearest2x(hi), O.nearest2x(lo))))
    return conv("conv_hr", hi, lo).float()


@torch.no_grad()
def rrdbnet_emulated_f16x2(sd, x, trunk="bf16", acc=torch.float64, **kw):
    """forward_feature of the f16x2 mode, (B,64,4H,4W) fp32"""
    feat, xrr, planes = trunk_and_feat(sd, x, trunk, acc)
    return tail_split(sd, feat, xrr, planes, acc, **kw)


@torch.no_grad()
def rrdbnet_tail_exact(sd, x, trunk="bf16"):
    """the emulated trunk's fp32 output through an EXACT tail (float64, nothing rounded): what the trunk alone leaves at the final map"""
    acc = torch.float64
    feat, xrr, _ = trunk_and_feat(sd, x, trunk, acc)
    sdd = {k: v.to(acc) for k, v in sd.items()}

    def conv(name, t):
        return F.conv2d(t, sdd[name + ".weight"], sdd[name + ".bias"], 1, 1)

    body = conv("conv_body", xrr) + feat
    u = F.leaky_relu(conv("conv_up1", O.nearest2x(body)), 0.2)
    u = F.leaky_relu(conv("conv_up2", O.nearest2x(u)), 0.2)
    return conv("conv_hr", u)
