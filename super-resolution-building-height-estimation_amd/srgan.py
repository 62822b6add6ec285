"""SR-stage (GAN fine-tuning) companions of RRDBNet, SURVEY.md 8f-4: the pieces around the generator that the reference's
``RealESRGAN`` trainer uses (SR/rrdbnet_arch.py:244-303 UNetDiscriminatorSN, :387-434 filter2D / USMSharp; SR/srloss.py:144-249
GANLoss).  They are NOT on the MI355X hot path and stay on stock PyTorch-ROCm ops (VERDICT r01 item 7 allows that); the
generator's forward AND backward run on libsrbh (rrdbnet_autograd.py).  The VGG19 perceptual loss needs torchvision's
pretrained network (absent offline): it is an optional plug-in (``RealESRGAN.cri_perceptual``), not restated."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.utils import spectral_norm

__all__ = ["UNetDiscriminatorSN", "filter2D", "USMSharp", "GANLoss"]


# ---- the discriminator's 3x3 stride-1 convolutions on libsrbh (round 5) --------------------------------------------------------------------
# conv0, conv4 .. conv9 of UNetDiscriminatorSN (SR/rrdbnet_arch.py:256-265,285-301) are 3x3 / stride 1 / padding 1: 74 % of the network's FLOPs.
# They run on the head's convolution kernels (csrc/srbh_head.hip, srbh_head_bwd.hip: forward, data gradient = the forward kernel on transposed +
# flipped weights, weight gradient as a GEMM over pixels) in slices of <= 64 output channels (the kernels' limit), in the precision of the SR-stage
# mode: exact fp32, or fp16 forward / bf16 gradient operands with fp32 accumulation (`precision`).  The three 4x4 stride-2 convs (unless
# `libsrbh_s2` is set, below), LeakyReLU and the skip additions stay stock device ops; with `libsrbh_wide` set, conv4..conv8 leave these kernels for
# the wide plane kernels with the LeakyReLU in their epilogue (further below).  The spectral-norm reparametrisation is torch's own: the hook computes
# `weight = weight_orig / sigma` (with its power iteration in training), the convolution takes that tensor and returns its gradient.
# UNetDiscriminatorSN.libsrbh selects it; the trainer turns it on with the generator's 16-bit operand modes (RealESRGAN.optimize_parameters: 57.5 ->
# 52.2 ms per iteration at batch 8, profiles/r05cs).  Restricting it to the <= 64-channel convs (one launch each) gained nothing.
def _disc_pack(w, cout, cin, transpose, h16, bf16):
    from . import _lib
    L = _lib.lib()
    if h16:
        buf = torch.empty(L.srbh_hpack_h16_bytes(cout, cin, 3) // 2, dtype=torch.float16, device=w.device)
        _lib.check(L.srbh_hpack_conv_h16(w.data_ptr(), cout, cin, 3, int(transpose), int(bf16), buf.data_ptr(), _lib.stream_ptr()), "hpack_conv_h16(disc)")
    else:
        buf = torch.empty(L.srbh_hpack_bytes(cout, cin, 3) // 4, dtype=torch.float32, device=w.device)
        _lib.check(L.srbh_hpack_conv_f32(w.data_ptr(), cout, cin, 3, int(transpose), buf.data_ptr(), _lib.stream_ptr()), "hpack_conv_f32(disc)")
    return buf


def _disc_launch(xn, pack, bias, cout, h16, bf16):
    """one srbh_hconv call: xn NHWC fp32 (B, c0, H, W) -> (B, cout <= 64, H, W) NHWC fp32"""
    import ctypes as C
    from . import _lib
    from . import hrfuse as H
    B, c0, Hh, Ww = xn.shape
    a = _lib.HConvArgs()
    a.src0, a.c0 = xn.data_ptr(), c0
    a.w = pack.data_ptr()
    a.bias = None if bias is None else bias.data_ptr()
    a.cout, a.ksize = cout, 3
    a.B, a.H, a.W = B, Hh, Ww
    out = H.empty_nhwc(B, cout, Hh, Ww, xn.device)
    a.out = out.data_ptr()
    L = _lib.lib()
    if h16:
        _lib.check(L.srbh_hconv_h16(C.byref(a), int(bf16), _lib.stream_ptr()), "hconv_h16(disc)")
    else:
        _lib.check(L.srbh_hconv_f32(C.byref(a), _lib.stream_ptr()), "hconv_f32(disc)")
    return out


class _DiscConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, h16):
        from . import hrfuse as H
        xn = H.to_nhwc(x.detach().float())
        w = weight.detach().float().contiguous()
        cout, cin = w.shape[:2]
        outs = []
        for lo in range(0, cout, 64):
            n = min(64, cout - lo)
            b = None
            if bias is not None:
                b = torch.zeros((n + 15) // 16 * 16, dtype=torch.float32, device=x.device)
                b[:n] = bias.detach().float()[lo:lo + n]
            outs.append(_disc_launch(xn, _disc_pack(w[lo:lo + n].contiguous(), n, cin, False, h16, False), b, n, h16, False))
        ctx.save_for_backward(xn, w)
        ctx.h16, ctx.has_bias = bool(h16), bias is not None
        return outs[0] if len(outs) == 1 else H.to_nhwc(torch.cat(outs, dim=1))

    @staticmethod
    def backward(ctx, g):
        import ctypes as C
        from . import _lib
        from . import hrfuse as H
        xn, w = ctx.saved_tensors
        h16 = ctx.h16
        gn = H.to_nhwc(g.float())
        cout, cin = w.shape[:2]
        L = _lib.lib()
        dx = None
        if ctx.needs_input_grad[0]:          # conv^T: the forward kernel on transposed + flipped weight slices, <= 64 input channels per launch
            parts = []
            for lo in range(0, cin, 64):
                n = min(64, cin - lo)
                parts.append(_disc_launch(gn, _disc_pack(w[:, lo:lo + n].contiguous(), n, cout, True, h16, True), None, n, h16, True))
            dx = parts[0] if len(parts) == 1 else H.to_nhwc(torch.cat(parts, dim=1))
        dw = None
        if ctx.needs_input_grad[1]:
            dws = []
            for lo in range(0, cout, 64):
                n = min(64, cout - lo)
                gs = gn if cout <= 64 else H.to_nhwc(gn[:, lo:lo + n].contiguous(memory_format=torch.channels_last))
                d = torch.empty((n, cin, 3, 3), dtype=torch.float32, device=g.device)
                a = _lib.HWGradArgs()
                a.src0, a.c0 = xn.data_ptr(), cin
                a.dy, a.cout, a.ksize = gs.data_ptr(), n, 3
                a.B, a.H, a.W = xn.shape[0], xn.shape[2], xn.shape[3]
                a.dw = d.data_ptr()
                ws = torch.empty(L.srbh_hwgrad_ws_bytes(n, cin, 3) // 4, dtype=torch.float32, device=g.device)
                a.ws = ws.data_ptr()
                _lib.check((L.srbh_hconv_wgrad_b16 if h16 else L.srbh_hconv_wgrad_f32)(C.byref(a), _lib.stream_ptr()), "hconv_wgrad(disc)")
                dws.append(d)
            dw = dws[0] if len(dws) == 1 else torch.cat(dws, dim=0)
        db = gn.sum(dim=(0, 2, 3)) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        return dx, dw, db, None


def _sn_hooks_by_hand(conv, x):
    """The hook protocol of the discriminator convs on libsrbh.  torch's spectral_norm is a forward PRE-hook that sets conv.weight =
    weight_orig / sigma (one power iteration in training): it is the only hook these paths know how to honour.  A module that carries nothing
    but such pre-hooks gets them called by hand -> True, and the caller reads conv.weight; a module carrying ANY other hook (forward hooks,
    foreign pre-hooks, hooks with kwargs) is left alone -> False, and the caller takes the stock path with the full hook protocol."""
    from torch.nn.utils.spectral_norm import SpectralNorm
    pre = list(conv._forward_pre_hooks.values())
    if (any(not isinstance(h, SpectralNorm) for h in pre) or conv._forward_hooks or conv._backward_hooks or conv._backward_pre_hooks
            or getattr(conv, "_forward_pre_hooks_with_kwargs", None) or getattr(conv, "_forward_hooks_with_kwargs", None)):
        return False
    for hook in pre:
        hook(conv, (x,))
    return True


def _disc_conv3x3(conv, x, h16):
    """conv(x) of a 3x3 stride-1 discriminator conv on libsrbh, under the hook protocol of _sn_hooks_by_hand"""
    if not _sn_hooks_by_hand(conv, x):
        return conv(x)
    return _DiscConvFn.apply(x, conv.weight, conv.bias, h16)


def _wconv(inp, in_chunks, w, bias, cout, B, H, W, bf16=0, relu=0, mask=None, add=None, out16=None, out32=None, out32_c=0,
           entry="srbh_wconv3x3", label="wconv3x3(vgg)"):
    """one call of a wide conv entry point (include/srbh.h: srbh_wconv3x3, srbh_wconv2x2, srbh_wconv3x3_lrelu) on whole plane buffers"""
    import ctypes as C
    from . import _lib
    a = _lib.WConvArgs()
    a.in_, a.in_chunks_total, a.in_chunk0, a.in_chunks = inp.data_ptr(), in_chunks, 0, in_chunks
    a.w, a.bias, a.cout = w.data_ptr(), (None if bias is None else bias.data_ptr()), cout
    a.B, a.H, a.W, a.bf16, a.relu = B, H, W, bf16, relu
    if mask is not None:
        a.mask16, a.mask_chunks_total, a.mask_chunk0 = mask.data_ptr(), cout // 32, 0
    if add is not None:
        a.add16, a.add_chunks_total, a.add_chunk0 = add.data_ptr(), cout // 32, 0
    if out16 is not None:
        a.out16, a.out16_chunks_total, a.out16_chunk0 = out16.data_ptr(), cout // 32, 0
    if out32 is not None:
        a.out32, a.out32_c = out32.data_ptr(), out32_c
    _lib.check(getattr(_lib.lib(), entry)(C.byref(a), _lib.stream_ptr()), label)


# ---- the three 4x4 stride-2 convs on libsrbh (UNetDiscriminatorSN.libsrbh_s2 = "f16") -------------------------------------------------------
# conv1..conv3 (SR/rrdbnet_arch.py:262-264, used at :277-279) are 4x4 / stride 2 / pad 1 without bias: exactly a 2x2-tap VALID conv over the
# space-to-depth image of the zero-padded input (4C channels, (H/2+1) x (W/2+1)) -- no wasted tap, no strided operand read.
# Forward, data gradient and weight gradient run on ACT16 planes through csrc/srbh_disc.hip: fp16 operands forward, bf16 operands in both
# gradients, fp32 accumulation (include/srbh.h states the contract).  Spectral norm rewrites the weight on every training forward, so both packs
# are made per call, in one launch.
class _DiscConvS2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight):
        from . import _lib
        from . import hrfuse as H
        L, sp = _lib.lib(), _lib.stream_ptr
        xn = H.to_nhwc(x.detach().float())
        w = weight.detach().float().contiguous()
        B, Cc, Hh, Ww = xn.shape
        O = w.shape[0]
        Ho, Wo = Hh // 2, Ww // 2
        dev = x.device
        with torch.cuda.device(dev):
            S = torch.zeros(L.srbh_act16_bytes(B, 4 * Cc, Ho + 1, Wo + 1), dtype=torch.uint8, device=dev)
            _lib.check(L.srbh_s2d_nhwc32_to_act16(xn.data_ptr(), S.data_ptr(), B, Cc, Hh, Ww, 0, sp()), "s2d_nhwc32_to_act16(disc)")
            nb = L.srbh_wpack2x2_bytes(O, 4 * Cc)
            w2, wt = torch.empty(nb, dtype=torch.uint8, device=dev), torch.empty(nb, dtype=torch.uint8, device=dev)
            _lib.check(L.srbh_pack_conv4x4s2_pair(w.data_ptr(), O, Cc, w2.data_ptr(), wt.data_ptr(), sp()), "pack_conv4x4s2_pair(disc)")
            out = H.empty_nhwc(B, O, Ho, Wo, dev)
            _wconv(S, Cc // 8, w2, None, O, B, Ho, Wo, out32=out, out32_c=O, entry="srbh_wconv2x2", label="wconv2x2(disc fwd)")
        ctx.save_for_backward(S, wt)
        ctx.geo = (B, Cc, O, Hh, Ww)
        return out

    @staticmethod
    def backward(ctx, g):
        from . import _lib
        from . import hrfuse as H
        L, sp = _lib.lib(), _lib.stream_ptr
        S, wt = ctx.saved_tensors
        B, Cc, O, Hh, Ww = ctx.geo
        Ho, Wo = Hh // 2, Ww // 2
        dev = g.device
        dx = dw = None
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return None, None
        with torch.cuda.device(dev):
            gn = H.to_nhwc(g.float())
            G = torch.zeros(L.srbh_act16_bytes(B, O, Ho + 2, Wo + 2), dtype=torch.uint8, device=dev)
            _lib.check(L.srbh_nhwc32_to_act16_framed(gn.data_ptr(), G.data_ptr(), B, O, Ho, Wo, 1, sp()), "nhwc32_to_act16_framed(disc)")
            if ctx.needs_input_grad[0]:
                ds = torch.empty((B, Ho + 1, Wo + 1, 4 * Cc), dtype=torch.float32, device=dev)
                _wconv(G, O // 32, wt, None, 4 * Cc, B, Ho + 1, Wo + 1, bf16=1, out32=ds, out32_c=4 * Cc, entry="srbh_wconv2x2",
                       label="wconv2x2(disc dgrad)")
                dx = H.empty_nhwc(B, Cc, Hh, Ww, dev)
                _lib.check(L.srbh_d2s_nhwc32(ds.data_ptr(), dx.data_ptr(), B, Cc, Hh, Ww, sp()), "d2s_nhwc32(disc)")
            if ctx.needs_input_grad[1]:
                dw = torch.empty((O, Cc, 4, 4), dtype=torch.float32, device=dev)
                ws = torch.empty(L.srbh_wgrad4x4s2_ws_bytes(O, Cc, B, Ho, Wo) // 4, dtype=torch.float32, device=dev)
                _lib.check(L.srbh_wgrad4x4s2_b16(S.data_ptr(), G.data_ptr(), B, Cc, O, Ho, Wo, dw.data_ptr(), ws.data_ptr(), sp()), "wgrad4x4s2_b16(disc)")
        return dx, dw


def _disc_conv4x4s2(conv, x):
    """conv(x) of a 4x4 / stride 2 / pad 1 discriminator conv on libsrbh (_DiscConvS2Fn), under the hook protocol of _sn_hooks_by_hand: spectral
    norm's pre-hook is called by hand, a module with any other hook takes stock `conv(x)`.  So does every conv or input outside what the kernels
    take (bias, other geometry, in_channels % 64, out_channels % 64, odd H or W, CPU tensors).  The kernels themselves take in_channels % 32
    (include/srbh.h); the module asks for 64, the narrowest conv1 of a discriminator this mode is meant for (num_feat 64: 64 / 128 / 256), so that
    the 8-feature net of fixture g14 -- whose conv3 is 32 -> 64 -- keeps stock fp32 convolutions and its 2e-5 agreement with the reference."""
    ok = (isinstance(conv, nn.Conv2d) and conv.kernel_size == (4, 4) and conv.stride == (2, 2) and conv.padding == (1, 1)
          and conv.dilation == (1, 1) and conv.groups == 1 and conv.bias is None and conv.padding_mode == "zeros"
          and conv.in_channels % 64 == 0 and conv.out_channels % 64 == 0
          and x.dim() == 4 and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0 and x.is_cuda)
    if not ok or not _sn_hooks_by_hand(conv, x):
        return conv(x)
    return _DiscConvS2Fn.apply(x, conv.weight)


# ---- act(conv4..conv8) on ACT16 planes (UNetDiscriminatorSN.libsrbh_wide = "f16") ------------------------------------------------------------
# conv4..conv8 (SR/rrdbnet_arch.py:265-269, used at :285-300) are 3x3 / stride 1 / pad 1 without bias, 64..512 channels, each followed by
# LeakyReLU(0.2).  One autograd function per conv runs conv + activation on csrc/srbh_disc3.hip and the wide conv of the trunk's family
# (DESIGN.md 3.21): the input staged once as fp16 planes, one launch for all output channels with the LeakyReLU in its epilogue; in the backward
# the gradient staged once as bf16 planes with the LeakyReLU derivative applied, the data gradient as the same wide conv on the transposed +
# flipped pack, the weight gradient in one launch (srbh_wgrad3x3_b16).  fp16 operands forward, bf16 operands in both gradients, fp32
# accumulation (include/srbh.h states the contract).  Both packs are made per call, in one launch (spectral norm).
class _DiscConvWideFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight):
        from . import _lib
        from . import hrfuse as H
        L, sp = _lib.lib(), _lib.stream_ptr
        xn = H.to_nhwc(x.detach().float())
        w = weight.detach().float().contiguous()
        B, Cc, Hh, Ww = xn.shape
        O = w.shape[0]
        dev = x.device
        with torch.cuda.device(dev):
            X = torch.zeros(L.srbh_act16_bytes(B, Cc, Hh, Ww), dtype=torch.uint8, device=dev)
            _lib.check(L.srbh_nhwc32_to_act16(xn.data_ptr(), X.data_ptr(), B, Cc, Hh, Ww, Cc // 32, 0, 1.0, 0, sp()), "nhwc32_to_act16(disc wide)")
            nb = L.srbh_wpack16_bytes(O, Cc)
            wf, wt = torch.empty(nb, dtype=torch.uint8, device=dev), torch.empty(nb, dtype=torch.uint8, device=dev)
            _lib.check(L.srbh_pack_conv3x3_pair(w.data_ptr(), O, Cc, wf.data_ptr(), wt.data_ptr(), sp()), "pack_conv3x3_pair(disc wide)")
            y = H.empty_nhwc(B, O, Hh, Ww, dev)
            _wconv(X, Cc // 32, wf, None, O, B, Hh, Ww, out32=y, out32_c=O, entry="srbh_wconv3x3_lrelu", label="wconv3x3_lrelu(disc fwd)")
        ctx.save_for_backward(X, y, wt)
        ctx.geo = (B, Cc, O, Hh, Ww)
        return y

    @staticmethod
    def backward(ctx, g):
        from . import _lib
        from . import hrfuse as H
        L, sp = _lib.lib(), _lib.stream_ptr
        X, y, wt = ctx.saved_tensors
        B, Cc, O, Hh, Ww = ctx.geo
        dev = g.device
        dx = dw = None
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return None, None
        with torch.cuda.device(dev):
            gn = H.to_nhwc(g.float())
            G = torch.zeros(L.srbh_act16_bytes(B, O, Hh, Ww), dtype=torch.uint8, device=dev)
            _lib.check(L.srbh_nhwc32_to_act16_lrelu_bwd(gn.data_ptr(), y.data_ptr(), G.data_ptr(), B, O, Hh, Ww, 0.2, 1, sp()), "nhwc32_to_act16_lrelu_bwd(disc)")
            if ctx.needs_input_grad[0]:
                dx = H.empty_nhwc(B, Cc, Hh, Ww, dev)
                _wconv(G, O // 32, wt, None, Cc, B, Hh, Ww, bf16=1, out32=dx, out32_c=Cc, label="wconv3x3(disc dgrad)")
            if ctx.needs_input_grad[1]:
                dw = torch.empty((O, Cc, 3, 3), dtype=torch.float32, device=dev)
                ws = torch.empty(L.srbh_wgrad3x3_ws_bytes(O, Cc, B, Hh, Ww) // 4, dtype=torch.float32, device=dev)
                _lib.check(L.srbh_wgrad3x3_b16(X.data_ptr(), Cc // 32, Cc, G.data_ptr(), O // 32, O, B, Hh, Ww, dw.data_ptr(), ws.data_ptr(), sp()),
                           "wgrad3x3_b16(disc)")
        return dx, dw


def _disc_conv3x3_act(conv, x, stock):
    """leaky_relu(conv(x), 0.2) of a wide 3x3 stride-1 discriminator conv on libsrbh (_DiscConvWideFn), under the hook protocol of
    _sn_hooks_by_hand: spectral norm's pre-hook is called by hand, a module with any other hook takes `stock(conv, x)` -- what the module did
    without this mode.  So does every conv or input outside what the kernels are meant for (bias, other geometry, in_channels % 64,
    out_channels % 64, CPU tensors): % 64 is the module's gate as in _disc_conv4x4s2, it keeps the 8-feature net of fixture g14 on what it runs
    today (the kernels themselves take in_channels % 32 and 32 output channels, include/srbh.h)."""
    ok = (isinstance(conv, nn.Conv2d) and conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == (1, 1)
          and conv.dilation == (1, 1) and conv.groups == 1 and conv.bias is None and conv.padding_mode == "zeros"
          and conv.in_channels % 64 == 0 and conv.out_channels % 64 == 0 and x.dim() == 4 and x.is_cuda)
    if not ok or not _sn_hooks_by_hand(conv, x):
        return stock(conv, x)
    return _DiscConvWideFn.apply(x, conv.weight)


class _Bilinear2xFn(torch.autograd.Function):
    """F.interpolate(scale_factor=2, mode="bilinear", align_corners=False) on a device tensor through srbh_bilinear2x_nhwc_f32 (the stock backward
    scatters with atomics: 4.5 ms of a 52 ms trainer iteration at batch 8)"""

    @staticmethod
    def forward(ctx, x):
        from . import _lib
        from . import hrfuse as H
        xn = H.to_nhwc(x.detach().float())
        B, Cc, Hh, Ww = xn.shape
        out = H.empty_nhwc(B, Cc, 2 * Hh, 2 * Ww, x.device)
        _lib.check(_lib.lib().srbh_bilinear2x_nhwc_f32(xn.data_ptr(), out.data_ptr(), B, Hh, Ww, Cc, 0, _lib.stream_ptr()), "bilinear2x(fwd)")
        return out

    @staticmethod
    def backward(ctx, g):
        from . import _lib
        from . import hrfuse as H
        gn = H.to_nhwc(g.float())
        B, Cc, H2, W2 = gn.shape
        dx = H.empty_nhwc(B, Cc, H2 // 2, W2 // 2, g.device)
        _lib.check(_lib.lib().srbh_bilinear2x_nhwc_f32(gn.data_ptr(), dx.data_ptr(), B, H2 // 2, W2 // 2, Cc, 1, _lib.stream_ptr()), "bilinear2x(bwd)")
        return dx


class UNetDiscriminatorSN(nn.Module):
    """U-Net discriminator with spectral normalisation; state_dict keys conv0..conv9 (conv1..conv8 carry weight_orig / weight_u /
    weight_v of torch's spectral_norm) as upstream (SR/rrdbnet_arch.py:244-303)."""

    def __init__(self, num_in_ch, num_feat=64, skip_connection=True):
        super().__init__()
        self.skip_connection = skip_connection
        nf = num_feat
        self.conv0 = nn.Conv2d(num_in_ch, nf, 3, 1, 1)
        self.conv1 = spectral_norm(nn.Conv2d(nf, nf * 2, 4, 2, 1, bias=False))
        self.conv2 = spectral_norm(nn.Conv2d(nf * 2, nf * 4, 4, 2, 1, bias=False))
        self.conv3 = spectral_norm(nn.Conv2d(nf * 4, nf * 8, 4, 2, 1, bias=False))
        self.conv4 = spectral_norm(nn.Conv2d(nf * 8, nf * 4, 3, 1, 1, bias=False))
        self.conv5 = spectral_norm(nn.Conv2d(nf * 4, nf * 2, 3, 1, 1, bias=False))
        self.conv6 = spectral_norm(nn.Conv2d(nf * 2, nf, 3, 1, 1, bias=False))
        self.conv7 = spectral_norm(nn.Conv2d(nf, nf, 3, 1, 1, bias=False))
        self.conv8 = spectral_norm(nn.Conv2d(nf, nf, 3, 1, 1, bias=False))
        self.conv9 = nn.Conv2d(nf, 1, 3, 1, 1)

    libsrbh = None          # None: stock convolutions; "f32" / "f16": the 3x3 stride-1 convs on libsrbh in that operand precision (device tensors only)
    libsrbh_s2 = None       # None: stock 4x4 stride-2 convolutions; "f16": conv1..conv3 on libsrbh's 16-bit plane kernels (device tensors only)
    libsrbh_wide = None     # None: act(conv4..conv8) as `libsrbh` says; "f16": conv + LeakyReLU as one function on 16-bit planes (device tensors only)

    def forward(self, x):
        act = lambda t: F.leaky_relu(t, 0.2)
        up = lambda t: F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False)
        if self.libsrbh is not None and x.is_cuda:
            h16 = self.libsrbh == "f16"
            c3 = lambda conv, t: _disc_conv3x3(conv, t, h16)      # noqa: E731
            up = lambda t: _Bilinear2xFn.apply(t) if t.shape[1] % 4 == 0 else F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False)      # noqa: E731
        else:
            c3 = lambda conv, t: conv(t)                           # noqa: E731
        if self.libsrbh_s2 is not None and x.is_cuda:
            if self.libsrbh_s2 != "f16":
                raise ValueError(f"UNetDiscriminatorSN.libsrbh_s2: unknown mode {self.libsrbh_s2!r} (None or 'f16')")
            s2 = _disc_conv4x4s2                                   # (4x4 stride 2 as 2x2 taps on space-to-depth planes)
        else:
            s2 = lambda conv, t: conv(t)                           # noqa: E731  (4x4 stride 2: stock convolutions)
        c3a = lambda conv, t: act(c3(conv, t))                     # noqa: E731  (conv4..conv8 with their activation)
        if self.libsrbh_wide is not None:
            if self.libsrbh_wide != "f16":
                raise ValueError(f"UNetDiscriminatorSN.libsrbh_wide: unknown mode {self.libsrbh_wide!r} (None or 'f16')")
            if x.is_cuda:
                c3a = lambda conv, t: _disc_conv3x3_act(conv, t, lambda c, u: act(c3(c, u)))      # noqa: E731  
        x0 = act(c3(self.conv0, x))
        x1 = act(s2(self.conv1, x0))
        x2 = act(s2(self.conv2, x1))
        x3 = act(s2(self.conv3, x2))
        x4 = c3a(self.conv4, up(x3))
        if self.skip_connection:
            x4 = x4 + x2
        x5 = c3a(self.conv5, up(x4))
        if self.skip_connection:
            x5 = x5 + x1
        x6 = c3a(self.conv6, up(x5))
        if self.skip_connection:
            x6 = x6 + x0
        return c3(self.conv9, c3a(self.conv8, c3a(self.conv7, x6)))


def filter2D(img, kernel):
    """cv2.filter2D on (b,c,h,w) with a (1|b, k, k) kernel, reflect padding (SR/rrdbnet_arch.py:387-409)."""
    k = kernel.size(-1)
    if k % 2 != 1:
        raise ValueError("Wrong kernel size")
    b, c, h, w = img.shape
    img = F.pad(img, (k // 2,) * 4, mode="reflect")
    ph, pw = img.shape[-2:]
    if kernel.size(0) == 1:
        return F.conv2d(img.reshape(b * c, 1, ph, pw), kernel.view(1, 1, k, k)).view(b, c, h, w)
    kern = kernel.view(b, 1, k, k).repeat(1, c, 1, 1).view(b * c, 1, k, k)
    return F.conv2d(img.reshape(1, b * c, ph, pw), kern, groups=b * c).view(b, c, h, w)


def _gaussian_kernel_1d(ksize, sigma):
    """cv2.getGaussianKernel: sigma <= 0 -> 0.3*((ksize-1)*0.5 - 1) + 0.8; exp(-(i-c)^2 / (2 sigma^2)) normalised to sum 1."""
    if sigma <= 0:
        sigma = 0.3 * ((ksize - 1) * 0.5 - 1) + 0.8
    c = (ksize - 1) * 0.5
    g = torch.tensor([math.exp(-((i - c) ** 2) / (2.0 * sigma * sigma)) for i in range(ksize)], dtype=torch.float64)
    return (g / g.sum()).float()


class USMSharp(nn.Module):
    """unsharp masking (SR/rrdbnet_arch.py:412-434): blur with a radius x radius Gaussian, sharpen where |residual|*255 > threshold."""

    def __init__(self, radius=50, sigma=0):
        super().__init__()
        if radius % 2 == 0:
            radius += 1
        self.radius = radius
        g = _gaussian_kernel_1d(radius, sigma)
        self.register_buffer("kernel", torch.outer(g, g).unsqueeze(0))
        self.register_buffer("kernel1d", g.clone(), persistent=False)      # (not in the state_dict: the reference's has `kernel` only)

    def _blur(self, img):
        """filter2D(img, self.kernel).  On a device tensor the Gaussian is applied as its two 1-D factors (the kernel IS their outer product):
        2 x 51 taps instead of 2 601 per pixel -- the 2-D form cost 7 ms per feed_data at batch 8 (tools/sr_iteration_phases.py); same values up
        to fp32 summation order.  CPU tensors keep the 2-D form the reference fixture is compared against."""
        if not img.is_cuda:
            return filter2D(img, self.kernel)
        k = self.kernel1d.numel()
        b, c, h, w = img.shape
        x = F.pad(img, (k // 2,) * 4, mode="reflect").reshape(b * c, 1, h + k - 1, w + k - 1)
        x = F.conv2d(x, self.kernel1d.view(1, 1, 1, k))
        return F.conv2d(x, self.kernel1d.view(1, 1, k, 1)).view(b, c, h, w)

    def forward(self, img, weight=0.5, threshold=10):
        blur = self._blur(img)
        residual = img - blur
        soft_mask = self._blur((residual.abs() * 255 > threshold).float())
        sharp = torch.clip(img + weight * residual, 0, 1)
        return soft_mask * sharp + (1 - soft_mask) * img


# ---- VGG19 perceptual loss (SR/srloss.py:61-143; wired at SR/rrdbnet_arch.py:496-498, used at :559-562) -------------------------------
# The reference builds `torchvision.models.vgg19(weights="IMAGENET1K_V1").features` and downloads its weights.  Neither torchvision nor a
# network exists offline, so the feature stack is restated from the layer table the reference itself prints (SR/srloss.py:8-48: configuration
# "E": 2 x 64, pool, 2 x 128, pool, 4 x 256, pool, 4 x 512, pool, 4 x 512, pool; every conv 3x3 / pad 1 + ReLU, max-pool 2 / 2) and takes the
# weights as a state_dict with torchvision's keys (`features.<i>.weight` / `.bias`, or the bare `<i>.weight` of the `features` module).
# Without one the convolutions keep their random initialisation -- a structure test, not a perceptual metric; RealESRGAN(is_train=True) only
# adds the term when it is handed weights or a ready module.
VGG19_CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512, 512, 512, "M")


def vgg19_features():
    """torchvision.models.vgg19().features: indices 0..36 as listed in SR/srloss.py:8-48"""
    layers, cin = [], 3
    for v in VGG19_CFG:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    return nn.Sequential(*layers)


class VGGFeatureExtractor(nn.Module):
    """SR/srloss.py:61-105: the VGG19 feature stack cut behind `feature_layer` (a list: one nn.Sequential child per cut, keys
    `features.child<i>.<j>.*` as upstream; an int: a single stack), optional ImageNet input normalisation / [-1, 1] -> [0, 1] range map,
    parameters frozen.  state_dict: torchvision's vgg19 weights (see above)."""

    def __init__(self, feature_layer=(2, 7, 16, 25, 34), use_input_norm=True, use_range_norm=False, state_dict=None):
        super().__init__()
        feats = vgg19_features()
        if state_dict is not None:
            sd = {(k[len("features."):] if k.startswith("features.") else k): v for k, v in state_dict.items()
                  if k.startswith("features.") or k.split(".")[0].isdigit()}
            feats.load_state_dict(sd, strict=True)
        self.use_input_norm = use_input_norm
        self.use_range_norm = use_range_norm
        if self.use_input_norm:
            self.register_buffer("mean", torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1))
            self.register_buffer("std", torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1))
        self.list_outputs = isinstance(feature_layer, (list, tuple))
        children = list(feats.children())
        if self.list_outputs:
            self.features = nn.Sequential()
            cuts = [-1] + list(feature_layer)
            for i in range(len(cuts) - 1):
                self.features.add_module("child" + str(i), nn.Sequential(*children[cuts[i] + 1:cuts[i + 1] + 1]))
        else:
            self.features = nn.Sequential(*children[:feature_layer + 1])
        for v in self.features.parameters():
            v.requires_grad = False

    def forward(self, x):
        if self.use_range_norm:
            x = (x + 1.0) / 2.0
        if self.use_input_norm:
            x = (x - self.mean) / self.std
        if self.list_outputs:
            out = []
            for child in self.features.children():
                x = child(x)
                out.append(x.clone())      # (the next child starts with an in-place ReLU)
            return out
        return self.features(x)


# ---- the same loss on libsrbh (PerceptualLoss.libsrbh = "f16") ---------------------------------------------------------------------------
# One call runs the feature stack on the output and on the target, the loss and (when x requires grad) dloss/dx on hand-written kernels:
# csrc/srbh_conv3x3.hip srbh_wconv3x3 (the trunk-family conv for 64..512 channels) and csrc/srbh_vgg.hip (input conversion, ReLU / max-pool
# plane -> plane and its backward, the one-read feature distance).  Activations are fp16 ACT16 planes from the input conversion to the last
# feature, gradients bf16 planes; the arithmetic contract stands in include/srbh.h and DESIGN.md 4.  No stock convolution, no fallback.
def _vgg_plan(pl):
    """[(conv module, is_cut, pool_behind)] of the convs up to the last cut + the cut weights; NotImplementedError for a cut that is no conv"""
    feats = pl.vgg.features
    if pl.vgg.list_outputs:
        layers, cuts = [], []
        for child in feats.children():
            layers += list(child.children())
            cuts.append(len(layers) - 1)
        weights = [float(w) for w in pl.weights[:len(cuts)]]
    else:
        layers = list(feats.children())
        cuts, weights = [len(layers) - 1], [1.0]
    for c in cuts:
        if c < 0 or not isinstance(layers[c], nn.Conv2d):
            raise NotImplementedError(f"PerceptualLoss.libsrbh: cut {c} is not a convolution of vgg19_features() "
                                      f"({type(layers[c]).__name__ if c >= 0 else 'empty'}); the libsrbh mode takes cuts at conv indices only")
    if sorted(set(cuts)) != cuts:
        raise NotImplementedError(f"PerceptualLoss.libsrbh: cuts {cuts} are not strictly increasing")
    plan, i = [], 0
    while i <= cuts[-1]:
        conv = layers[i]
        if not (isinstance(conv, nn.Conv2d) and conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == (1, 1)):
            raise NotImplementedError(f"PerceptualLoss.libsrbh: layer {i} is not a 3x3 / stride 1 / pad 1 convolution")
        j, relu, pool = i + 1, False, False
        while j <= cuts[-1] and not isinstance(layers[j], nn.Conv2d):
            if isinstance(layers[j], nn.ReLU) and not pool:
                relu = True
            elif isinstance(layers[j], nn.MaxPool2d) and relu and not pool:
                pool = True
            else:
                raise NotImplementedError(f"PerceptualLoss.libsrbh: layer {j} does not follow the conv / ReLU / max-pool order of vgg19_features()")
            j += 1
        if j <= cuts[-1] and not relu:
            raise NotImplementedError(f"PerceptualLoss.libsrbh: no ReLU behind conv {i}")
        plan.append((conv, i in cuts, pool, i))
        i = j
    return plan, cuts, weights


def _vgg_packs(pl, device):
    """frozen packs of the plan's convs: fp16 forward packs + fp32 biases, bf16 transposed + flipped packs; keyed by the wcache stamps"""
    from . import _lib, wcache
    plan, cuts, weights = _vgg_plan(pl)
    params = [p for conv, *_ in plan for p in (conv.weight, conv.bias)]
    key = (wcache.gen(*params), tuple((p._version, p.data_ptr()) for p in params), tuple(cuts), str(device))
    cached = pl.__dict__.get("_srbh_vgg_packs")
    if cached is None or cached[0] != key:
        L = _lib.lib()
        convs = []
        for conv, is_cut, pool, idx in plan:
            w = conv.weight.detach().float().contiguous()
            cout, cin = w.shape[:2]
            if cout % 64 or (cin % 32 and cin != 3) or conv.bias is None:
                raise NotImplementedError(f"PerceptualLoss.libsrbh: conv {idx} has {cin} -> {cout} channels")
            fwd = torch.zeros(L.srbh_wpack16_bytes(cout, cin), dtype=torch.uint8, device=device)
            _lib.check(L.srbh_pack_conv3x3_f16(w.data_ptr(), cout, cin, fwd.data_ptr(), _lib.stream_ptr()), "pack_conv3x3_f16(vgg)")
            wt = w.transpose(0, 1).flip(2, 3).contiguous()
            bwd = torch.zeros(L.srbh_wpack16_bytes(cin, cout), dtype=torch.uint8, device=device)
            _lib.check(L.srbh_pack_conv3x3_b16(wt.data_ptr(), cin, cout, bwd.data_ptr(), _lib.stream_ptr()), "pack_conv3x3_b16(vgg)")
            convs.append(dict(fwd=fwd, bwd=bwd, bias=conv.bias.detach().float().contiguous(), cin=cin, cout=cout, cut=is_cut, pool=pool))
        import ctypes as C
        norm = None
        if pl.vgg.use_input_norm:
            norm = ((C.c_float * 3)(*pl.vgg.mean.flatten().tolist()), (C.c_float * 3)(*pl.vgg.std.flatten().tolist()))
        cached = (key, dict(convs=convs, weights=weights, norm=norm))
        pl.__dict__["_srbh_vgg_packs"] = cached
    wcache.keep(cached)
    return cached[1]


class _PlanePool:
    """zero-bordered ACT16 buffers of one (device, batch) per (tag, chunks, H, W): allocated and zeroed once, the kernels write interiors only"""

    def __init__(self, device, B):
        self.device, self.B, self.bufs = device, B, {}

    def get(self, tag, chunks, H, W):
        from . import _lib, wcache
        k = (tag, chunks, H, W)
        b = self.bufs.get(k)
        if b is None:
            b = self.bufs[k] = torch.zeros(_lib.lib().srbh_act16_bytes(self.B, chunks * 32, H, W), dtype=torch.uint8, device=self.device)
        wcache.keep(b)
        return b


class _PerceptualFn(torch.autograd.Function):
    """the whole loss: forward returns the fp32 loss and keeps the fp32 NHWC gradient of the normalised input; backward scales it"""

    @staticmethod
    def forward(ctx, x, gt, pl):
        from . import _lib
        L, sp = _lib.lib(), _lib.stream_ptr
        dev = x.device
        P = _vgg_packs(pl, dev)
        convs, norm = P["convs"], P["norm"]
        B, C3, H0, W0 = x.shape
        if C3 != 3 or tuple(gt.shape) != tuple(x.shape):
            raise ValueError(f"PerceptualLoss.libsrbh: x and gt must be (B, 3, H, W) of one shape (got {tuple(x.shape)}, {tuple(gt.shape)})")
        pools = pl.__dict__.setdefault("_srbh_vgg_planes", {})
        pool = pools.get((str(dev), B))
        if pool is None:
            pool = pools[(str(dev), B)] = _PlanePool(dev, B)
        rng = int(bool(pl.vgg.use_range_norm))
        mean_p, std_p = (norm if norm is not None else (None, None))
        l2 = int(pl.lossfn_type != "l1")
        want_grad = bool(ctx.needs_input_grad[0])

        def features(t, side):
            """planes of every conv ('x': all kept for the backward; 'g': only the cuts are kept, the rest ping-pong)"""
            src = t.detach().float().contiguous()
            a = pool.get("in", 1, H0, W0)
            _lib.check(L.srbh_vgg_input_f16(src.data_ptr(), a.data_ptr(), B, H0, W0, mean_p, std_p, rng, sp()), "vgg_input_f16")
            h, w, ach, out = H0, W0, 1, []
            for j, c in enumerate(convs):
                nch = c["cout"] // 32
                tag = f"{side}{j}" if (side == "x" or c["cut"]) else f"g_pp{j & 1}"
                p = pool.get(tag, nch, h, w)
                _wconv(a, ach, c["fwd"], c["bias"], c["cout"], B, h, w, relu=int(not c["cut"]), out16=p)
                out.append((p, nch, h, w))
                if j + 1 < len(convs):
                    if c["cut"] or c["pool"]:
                        if c["pool"] and (h < 2 or w < 2):
                            raise ValueError(f"PerceptualLoss.libsrbh: a {h}x{w} plane cannot be pooled")
                        ho, wo = (h // 2, w // 2) if c["pool"] else (h, w)
                        a = pool.get(f"a{j & 1}", nch, ho, wo)
                        _lib.check(L.srbh_vgg_relu_pool_f16(p.data_ptr(), a.data_ptr(), B, nch, h, w, int(c["pool"]), sp()), "vgg_relu_pool_f16")
                        h, w = ho, wo
                    else:
                        a = p
                    ach = nch
            return out

        with torch.cuda.device(dev):
            fx, fg = features(x, "x"), features(gt, "g")
            acc = torch.empty(1, dtype=torch.float64, device=dev)
            lg, first, wi = {}, True, 0
            for j, c in enumerate(convs):
                if not c["cut"]:
                    continue
                (px, nch, h, w), (pg, *_) = fx[j], fg[j]
                n = B * c["cout"] * h * w
                wgt = P["weights"][wi]
                wi += 1
                g = pool.get(f"lg{j}", nch, h, w) if want_grad else None
                ws = torch.empty(max(1, L.srbh_vgg_dist_ws_bytes(B, nch, h, w) // 8), dtype=torch.float64, device=dev)
                gscale = (2.0 if l2 else 1.0) * wgt / n
                _lib.check(L.srbh_vgg_dist(px.data_ptr(), pg.data_ptr(), B, nch, h, w, l2, wgt / n, int(not first), acc.data_ptr(), gscale,
                                           None if g is None else g.data_ptr(), ws.data_ptr(), sp()), "vgg_dist")
                lg[j] = g
                first = False
            ctx.geo = None
            if want_grad:
                j = len(convs) - 1
                G = lg[j]
                while j > 0:
                    c, prev = convs[j], convs[j - 1]
                    _, _, h, w = fx[j]
                    pp, pch, ph, pw = fx[j - 1]
                    add = lg.get(j - 1)
                    Gp = pool.get(f"G_pp{j & 1}", pch, ph, pw)
                    if prev["pool"]:
                        T = pool.get("T", pch, h, w)
                        _wconv(G, c["cout"] // 32, c["bwd"], None, c["cin"], B, h, w, bf16=1, out16=T)
                        _lib.check(L.srbh_vgg_relu_pool_bwd_b16(T.data_ptr(), pp.data_ptr(), None if add is None else add.data_ptr(), Gp.data_ptr(),
                                                                B, pch, ph, pw, 1, sp()), "vgg_relu_pool_bwd_b16")
                    else:
                        _wconv(G, c["cout"] // 32, c["bwd"], None, c["cin"], B, h, w, bf16=1, mask=pp, add=add, out16=Gp)
                    G = Gp
                    j -= 1
                g3 = torch.empty((B, H0, W0, 3), dtype=torch.float32, device=dev)
                _wconv(G, convs[0]["cout"] // 32, convs[0]["bwd"], None, 32, B, H0, W0, bf16=1, out32=g3, out32_c=3)
                ctx.save_for_backward(g3)
                ctx.geo = (B, H0, W0, rng, None if norm is None else norm[1])
            return (acc.to(torch.float32) * float(pl.loss_weight)).reshape(())

    @staticmethod
    def backward(ctx, go):
        from . import _lib
        (g3,) = ctx.saved_tensors
        B, H0, W0, rng, std_p = ctx.geo
        dx = torch.empty((B, 3, H0, W0), dtype=torch.float32, device=g3.device)
        gof = go.detach().float().reshape(1).contiguous()
        with torch.cuda.device(g3.device):
            _lib.check(_lib.lib().srbh_vgg_dx_nchw(g3.data_ptr(), dx.data_ptr(), B, H0, W0, std_p, rng, gof.data_ptr(), _lib.stream_ptr()), "vgg_dx_nchw")
        return dx, None, None


class PerceptualLoss(nn.Module):
    """SR/srloss.py:108-143: sum_i weights[i] * L1|MSE(vgg_i(x), vgg_i(gt.detach())) -- times `self.loss_weight`, which upstream pins to 1.0
    whatever the argument says (srloss.py:123: kept, it is the arithmetic the checkpoints were trained with).
    `libsrbh = "f16"` (device tensors only): the feature stack, the loss and its input gradient on libsrbh's 16-bit kernels (_PerceptualFn)."""

    libsrbh = None          # None: stock ops; "f16": fp16 activation planes / bf16 gradient planes on libsrbh, cuts at conv indices only

    def __init__(self, feature_layer=(2, 7, 16, 25, 34), weights=(0.1, 0.1, 1.0, 1.0, 1.0), lossfn_type="l1", use_input_norm=True,
                 use_range_norm=False, loss_weight=1.0, state_dict=None):
        super().__init__()
        self.vgg = VGGFeatureExtractor(feature_layer=feature_layer, use_input_norm=use_input_norm, use_range_norm=use_range_norm,
                                       state_dict=state_dict)
        self.lossfn_type = lossfn_type
        self.weights = list(weights)
        self.lossfn = nn.L1Loss() if lossfn_type == "l1" else nn.MSELoss()
        self.loss_weight = 1.0

    def forward(self, x, gt):
        if self.libsrbh is not None and x.is_cuda:
            if self.libsrbh != "f16":
                raise ValueError(f"PerceptualLoss.libsrbh: unknown mode {self.libsrbh!r} (None or 'f16')")
            return _PerceptualFn.apply(x, gt.detach(), self)
        x_vgg, gt_vgg = self.vgg(x), self.vgg(gt.detach())
        loss = 0.0
        if isinstance(x_vgg, list):
            for i in range(len(x_vgg)):
                loss = loss + self.weights[i] * self.lossfn(x_vgg[i], gt_vgg[i])
        else:
            loss = loss + self.lossfn(x_vgg, gt_vgg.detach())
        return loss * self.loss_weight


class GANLoss(nn.Module):
    """SR/srloss.py:144-249: 'vanilla' (BCE with logits), 'lsgan', 'wgan', 'wgan_softplus', 'hinge'; loss_weight applies to the
    generator only."""

    def __init__(self, gan_type, real_label_val=1.0, fake_label_val=0.0, loss_weight=1.0):
        super().__init__()
        if gan_type not in ("vanilla", "lsgan", "wgan", "wgan_softplus", "hinge"):
            raise NotImplementedError(f"GAN type {gan_type} is not implemented.")
        self.gan_type, self.loss_weight = gan_type, loss_weight
        self.real_label_val, self.fake_label_val = real_label_val, fake_label_val

    def forward(self, input, target_is_real, is_disc=False):
        t = self.gan_type
        if t == "hinge":
            if is_disc:
                loss = F.relu(1 + (-input if target_is_real else input)).mean()
            else:
                loss = -input.mean()
        elif t == "wgan":
            loss = -input.mean() if target_is_real else input.mean()
        elif t == "wgan_softplus":
            loss = F.softplus(-input).mean() if target_is_real else F.softplus(input).mean()
        else:
            target = input.new_full(input.shape, self.real_label_val if target_is_real else self.fake_label_val)
            loss = F.binary_cross_entropy_with_logits(input, target) if t == "vanilla" else F.mse_loss(input, target)
        return loss if is_disc else loss * self.loss_weight
