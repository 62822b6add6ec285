"""Rounding-exact CPU emulation of libsrbh's inference RRDBNet  --  TEST INFRASTRUCTURE ONLY.

``srbh_oracle.rrdbnet_forward_feature`` says what the network computes; this module says what the KERNELS compute: the
same network with every value rounded where ``srbh_rrdbnet_forward`` (csrc/srbh_rrdbnet.hip) rounds it, written from that
file and the conv epilogue (csrc/srbh_conv3x3_kernel.h):

* conv_first in fp32 -> ``feat``, ``xr``, ``xrr`` (fp32); dense planes 0..1 = RNE of it to the trunk type;
* conv1..conv4 of a dense block: operands = the 16-bit planes and the weights rounded (RNE) to the trunk type, fp32 sum,
  + bias, LeakyReLU (``v >= 0 ? v : v * 0.2f``), RNE to the trunk type;
* conv5: ``y = (conv + bias) * 0.2f + xr`` -> ``xr``; closing an RRDB ``y = y * 0.2f + xrr`` -> ``xrr`` and ``xr``; next
  planes 0..1 = RNE of ``y`` to the trunk type -- except the very last conv5 of a bf16 trunk, which rounds to fp16;
* conv_body (+ ``feat``), conv_up1, conv_up2 (nearest x2, LeakyReLU): fp16 operands, fp16 outputs; conv_hr: fp32 output.

The one thing it does not fix is the ORDER of the additions inside a conv: ``acc`` selects the accumulator (float64 = the
exact sum rounded once, float32 = torch's CPU order).  The matrix cores add in a third order; the distance between the two
emulations is the yardstick for how far a correct kernel may sit from either (tests/test_gpu_trunk_parity.py).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import srbh_oracle as O

_KINDS = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _q16(t, kind):
    """round to a 16-bit type (torch's conversions are RNE) and back; ``None`` = keep"""
    return t if kind is None else t.float().to(_KINDS[kind]).to(t.dtype)


def _f32(t, on=True):
    """an fp32 register / store"""
    return t.float().to(t.dtype) if on else t


@torch.no_grad()
def rrdbnet_emulated(sd, x, trunk="bf16", acc=torch.float64, stop="feature", scale: int = 4):
    """``trunk``: "bf16" (the default inference trunk), "fp16" (SRBH_TRUNK_BF16=0) or None (no rounding anywhere: the plain
    network in ``acc`` precision).  ``stop="trunk"``: the fp32 RRDB-level stream behind the last RRDB (``xrr``, (B,64,H,W));
    ``"feature"``: forward_feature's (B,64,4H,4W); ``"both"``: the pair.  fp32 tensors (``acc`` precision when ``trunk`` is None)."""
    if trunk not in ("bf16", "fp16", None):
        raise ValueError(f"trunk={trunk!r}")
    if stop not in ("trunk", "feature", "both"):
        raise ValueError(f"stop={stop!r}")
    rounding = trunk is not None
    tail = "fp16" if rounding else None
    nb = O.num_blocks_of(sd)
    if nb == 0 and rounding:
        trunk = "fp16"          # (no dense blocks: srbh_rrdbnet_forward writes conv_first's planes as fp16, conv_body reads them)
    one = torch.ones((), dtype=acc)
    S = _f32(one * 0.2) if rounding else one * 0.2          # the kernels' 0.2f

    def f32(t):
        return _f32(t, rounding)

    def conv(name, inp, kind):
        w = _q16(sd[name + ".weight"].to(acc), kind)
        return f32(f32(F.conv2d(inp.to(acc), w, None, 1, 1)) + sd[name + ".bias"].to(acc).view(1, -1, 1, 1))

    def lrelu(v):
        return torch.where(v >= 0, v, f32(v * S))

    x = x.to(acc)
    if scale == 2:
        x = O.pixel_unshuffle(x, 2)
    elif scale == 1:
        x = O.pixel_unshuffle(x, 4)
    feat = f32(F.conv2d(x, sd["conv_first.weight"].to(acc), sd["conv_first.bias"].to(acc), 1, 1))
    xr = xrr = feat
    planes = _q16(feat, trunk)
    for i in range(nb):
        for r in (1, 2, 3):
            p = f"body.{i}.rdb{r}."
            feats = [planes]
            for k in range(1, 5):
                feats.append(_q16(lrelu(conv(f"{p}conv{k}", torch.cat(feats, 1), trunk)), trunk))
            y = f32(conv(p + "conv5", torch.cat(feats, 1), trunk) * S + xr)
            if r == 3:
                y = xrr = f32(y * S + xrr)
            xr = y
            last = i == nb - 1 and r == 3
            planes = _q16(y, "fp16" if (last and rounding) else trunk)
    trunk_out = xrr.float() if rounding else xrr
    if stop == "trunk":
        return trunk_out
    body = _q16(f32(conv("conv_body", planes, tail) + feat), tail)
    u = _q16(lrelu(conv("conv_up1", O.nearest2x(body), tail)), tail)
    u = _q16(lrelu(conv("conv_up2", O.nearest2x(u), tail)), tail)
    out = conv("conv_hr", u, tail)
    out = out.float() if rounding else out
    return (trunk_out, out) if stop == "both" else out
