"""GPU: the head's DEFAULT inference precision -- fp16 operands / fp32 accumulate (srbh_hconv_h16, BASELINE configs[4] "fp16
MFMA").  Two statements: (1) the kernel computes exactly the convolution of the fp16-rounded operands (<= 5e-6 against a
float64 conv of the same rounded values: summation order only), for every shape / fusion the head uses; (2) the whole head
stays inside the north star's tolerance on the height maps: <= 1e-3 relative L2 against the reference fixtures (g7) and the
fp32 CPU oracle.  The strict fp32 mode keeps its 2e-5 tests in test_gpu_head.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import srbh_oracle as O
from oracle import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_HEAD = 1e-3        # north star: height maps within 1e-3 relative of the reference
TOL_KERNEL = 5e-6      # vs the float64 conv of the SAME fp16-rounded operands


def rnd(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


def h16(t):
    return t.half().double()


@pytest.mark.parametrize("c0,c1,cout,ks,ps2,hw", [(16, 0, 16, 3, False, (24, 70)), (16, 16, 16, 3, False, (17, 64)), (64, 0, 16, 3, False, (8, 130)),
                                                   (16, 0, 64, 3, True, (12, 20)), (32, 0, 16, 1, False, (9, 66)), (16, 0, 7, 3, False, (16, 16)),
                                                   (16, 0, 16, 3, False, (8, 128)), (16, 0, 7, 3, False, (8, 64)), (16, 0, 1, 3, False, (4, 128))])
def test_h16_conv_equals_conv_of_rounded_operands(c0, c1, cout, ks, ps2, hw):
    from srbh_amd import hrfuse as H
    Hh, Ww = hw
    conv = torch.nn.Conv2d(c0 + c1, cout, ks, 1, ks // 2, bias=True)
    with torch.no_grad():
        conv.weight.copy_(rnd(tuple(conv.weight.shape), 3, -0.3, 0.3))
        conv.bias.copy_(rnd((cout,), 4))
    x0, x1 = rnd((2, c0, Hh, Ww), 5), (rnd((2, c1, Hh, Ww), 6) if c1 else None)
    scale, shift = rnd((c0,), 7, 0.5, 1.5), rnd((c0,), 8, -0.2, 0.2)
    # reference: pre-affine + ReLU in fp32 (as the kernel does while staging), THEN the fp16 rounding of both operands
    a = torch.relu(x0 * scale[None, :, None, None] + shift[None, :, None, None])
    xin = torch.cat([a] + ([x1] if c1 else []), 1)
    want = F.conv2d(h16(xin), h16(conv.weight), conv.bias.double(), 1, ks // 2).float()
    if ps2:
        want = F.pixel_shuffle(want, 2)
    H.set_head_precision("f16")
    try:
        conv = conv.to(DEV)
        srcs = [H.to_nhwc(x0.to(DEV))] + ([H.to_nhwc(x1.to(DEV))] if c1 else [])
        got, _ = H.hconv(srcs, conv, H._PackedConv(), pre=(scale.to(DEV), shift.to(DEV), True), ps2=ps2)
    finally:
        H.set_head_precision("auto")
    assert got.shape == want.shape
    assert O.rel_l2(got.cpu(), want) <= TOL_KERNEL


def b16(t):
    return t.bfloat16().double()


@pytest.mark.parametrize("c0,c1,cout,ks,pre,hw", [(16, 0, 16, 3, True, (8, 128)), (16, 0, 16, 3, False, (12, 64)), (16, 0, 16, 3, True, (24, 70)), (64, 16, 16, 3, False, (17, 64)), (16, 0, 32, 3, True, (8, 130)),
                                                   (80, 0, 16, 1, False, (9, 66)), (24, 0, 16, 3, False, (16, 16)), (16, 0, 7, 3, False, (16, 16))])
def test_b16_wgrad_equals_wgrad_of_rounded_operands(c0, c1, cout, ks, pre, hw):
    """srbh_hconv_wgrad_b16: exactly the weight gradient of the bf16-rounded (transformed input, dY) pair, fp32-accumulated
    (<= 5e-6 against float64 on the same rounded values); ragged tile edges, the concat, the folded BN+ReLU, a half-filled
    16-channel chunk (cin 24), and the fp32 fallback for a 7-channel output (then: no rounding at all).  The first two shapes
    (W % 64 == 0, H % 4 == 0, 16 -> 16) run the double-buffered hwgrad16_kernel, the others hwgrad_b16_kernel."""
    from srbh_amd import hrfuse as H
    from srbh_amd import hrfuse_autograd as AG
    Hh, Ww = hw
    x0, x1 = rnd((2, c0, Hh, Ww), 15), (rnd((2, c1, Hh, Ww), 16) if c1 else None)
    dy = rnd((2, cout, Hh, Ww), 17) * 1e-6            # per-pixel gradients of a mean loss: below fp16's normal range
    # power-of-two scales: x*scale is exact, so the kernel's fused multiply-add and torch's mul-then-add round identically
    # (a 1-ulp fp32 difference would flip the bf16 rounding of a few inputs: a 2^-9 error each, 1e-5 on the sum)
    scale, shift = 2.0 ** torch.randint(-1, 2, (c0,), generator=torch.Generator().manual_seed(7)).float(), rnd((c0,), 8, -0.2, 0.2)
    a = torch.relu(x0 * scale[None, :, None, None] + shift[None, :, None, None]) if pre else x0
    xin = torch.cat([a] + ([x1] if c1 else []), 1)
    rx, rg = (b16, b16) if cout % 16 == 0 else (lambda t: t.double(), lambda t: t.double())
    w = torch.zeros(cout, c0 + c1, ks, ks, dtype=torch.float64, requires_grad=True)
    F.conv2d(rx(xin), w, None, 1, ks // 2).backward(rg(dy))
    H.set_head_precision("f16")
    try:
        srcs = [H.to_nhwc(x0.to(DEV))] + ([H.to_nhwc(x1.to(DEV))] if c1 else [])
        got = AG.conv_wgrad(srcs, (scale.to(DEV), shift.to(DEV), True) if pre else None, H.to_nhwc(dy.to(DEV)), cout, ks)
    finally:
        H.set_head_precision("auto")
    assert O.rel_l2(got.cpu().double(), w.grad) <= TOL_KERNEL
    # and the rounding itself stays at bf16's level against the unrounded gradient
    w2 = torch.zeros_like(w, requires_grad=True)
    F.conv2d(xin.double(), w2, None, 1, ks // 2).backward(dy.double())
    assert O.rel_l2(got.cpu().double(), w2.grad) <= 6e-3


def test_default_inference_head_within_north_star_tolerance(golden_dir):
    """HRfeature and both HRfuse_residual heads in eval mode under no_grad (-> fp16 operands by default) against the
    fixtures produced by the imported reference."""
    from srbh_amd import hrfuse as H
    from srbh_amd.hrfuse import HRfeature, HRfuse_residual
    assert H._HEAD_PRECISION["mode"] == "auto"
    g = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(golden_dir, "g7_head.npz")).items()}
    sd = synth.hrfeature_state_dict(64, 16, 16, seed=18, mode="stress")
    m = HRfeature(64, 16, 16)
    m.load_state_dict(sd, strict=True)
    x = rnd((2, 64, 16, 16), 108)
    with torch.no_grad():
        assert H.head_h16()
        e = O.rel_l2(m.to(DEV).eval()(x.to(DEV)).cpu(), g["g7_hrfeat_eval"])
    assert 1e-6 < e <= TOL_HEAD, e              # (> 1e-6: the fp16 path really ran)
    for oc in (1, 7):
        sd = synth.hrfuse_residual_state_dict(16, 16, 16, oc, 4, seed=19 + oc, mode="stress")
        m = HRfuse_residual(16, 16, 16, oc, 4)
        m.load_state_dict(sd, strict=True)
        a, b = rnd((2, 16, 4, 4), 109), rnd((2, 16, 16, 16), 110)      # (the fixture's inputs)
        with torch.no_grad():
            ye = m.to(DEV).eval()(a.to(DEV), b.to(DEV)).cpu()
        assert O.rel_l2(ye, O.hrfuse_residual(synth.clone_sd(sd), "", a, b, False)) <= TOL_HEAD, oc
        assert O.rel_l2(ye, g[f"g7_fuse{oc}_eval"]) <= TOL_HEAD, oc


def test_training_graph_stays_exact_fp32():
    """auto mode: a recorded graph (training) keeps the exact-fp32 kernels in forward and backward -- same numbers as the
    explicit strict mode (an fp16-operand conv would differ at the 1e-4 level)."""
    from srbh_amd import hrfuse as H
    from srbh_amd.hrfuse import HRfeature
    outs = []
    for mode in ("auto", "f32"):
        H.set_head_precision(mode)
        torch.manual_seed(3)
        m = HRfeature(64, 16, 16).to(DEV).train()
        x = rnd((2, 64, 24, 40), 9).to(DEV)
        y = m(x)
        y.square().mean().backward()
        outs.append((y.detach().clone(), m[0].conv1.weight.grad.clone()))
    H.set_head_precision("auto")
    # (not torch.equal: the BatchNorm partial sums are double atomics, their order moves the last bit from run to run)
    assert O.rel_l2(outs[0][0].cpu(), outs[1][0].cpu()) <= 1e-6 and O.rel_l2(outs[0][1].cpu(), outs[1][1].cpu()) <= 1e-6


def test_model_eval_default_precision_height_maps():
    """SRRegress_Cls_feature.forward in the default inference precision against the CPU reference (stock-op encoder /
    decoders on CPU + the fp32 oracle head): height / building / aggregated maps <= 1e-3."""
    import copy
    from tests.test_gpu_model import cpu_reference, make_model
    m = make_model(seed=41).eval()
    x = synth.tiles(2, 8, 64, seed=43)
    fea = torch.randn(2, 64, 256, 256, generator=torch.Generator().manual_seed(44)) * 0.5
    with torch.no_grad():
        want = cpu_reference(copy.deepcopy(m), x, fea, False)
        got = m.to(DEV)(x.to(DEV), fea.to(DEV))
    for a, b, name in zip(got, want, ("height", "build", "aggre")):
        assert O.rel_l2(a.cpu(), b) <= TOL_HEAD, name


@pytest.mark.parametrize("width,io16,act", [(96, False, "none"), (128, False, "none"), (128, True, "none"), (128, True, "c1c2")])
def test_mixed_precision_training_gradients_close_to_exact(monkeypatch, width, io16, act):
    """(width 128 + io16: the gradient tensors internal to a block's backward -- dz / dc2 / da1 / dc1 / dd -- are bf16 in memory
    (hrfuse.TRAIN_IO16, the default), same bounds; act "c1c2" (opt-in): the saved activations c1 / c2 / downsample output are fp16 as
    well -- gradients within the same bounds, the training-mode forward 1.5e-3 instead of 1e-3 (stated here, measured 1.1e-3);
    width 96 is not a multiple of the persistent kernels' 64-pixel tiles, so the template kernels and fp32 tensors run.)
    TrainStep's default ("f16": forward convs fp16 operands, data and weight gradients bf16 operands, fp32 accumulation): every
    parameter gradient of the head within 2e-2 relative of the exact-fp32 graph (bf16 keeps 8 mantissa bits: 4e-3 per
    operand, averaged over the 9 x 16 products of a tap sum), outputs within 1e-3; tiny per-pixel gradients (a mean over
    10^5 pixels puts them at 1e-6, below fp16's normal range) must survive -- that is why the data gradients are bf16."""
    from srbh_amd import hrfuse as H
    from srbh_amd import hrfuse_autograd as HA
    from srbh_amd.hrfuse import HRfeature, HRfuse_residual
    monkeypatch.setattr(H, "TRAIN_IO16", io16)
    monkeypatch.setattr(H, "TRAIN_IO16_ACT", act)
    seen = []
    real_bwd = HA.bn_backward
    monkeypatch.setattr(HA, "bn_backward", lambda g, c, *a, **k: (seen.append((g.dtype, c.dtype, k.get("out_b16", False))), real_bwd(g, c, *a, **k))[1])
    res = {}
    for mode in ("f32", "f16"):
        H.set_head_precision(mode)
        torch.manual_seed(5)
        hf, fu = HRfeature(64, 16, 16).to(DEV).train(), HRfuse_residual(16, 16, 16, 1, 4).to(DEV).train()
        x = rnd((2, 64, 64, width), 11).to(DEV)
        lo = rnd((2, 16, 16, width // 4), 12).to(DEV).requires_grad_(True)
        y = fu(lo, hf(x))
        (y.square().mean() * 1e-3).backward()          # small per-pixel gradients on purpose
        res[mode] = (y.detach().cpu(), {k: p.grad.cpu() for k, p in list(hf.named_parameters()) + list(fu.named_parameters())}, lo.grad.cpu())
    H.set_head_precision("auto")
    # the 16-bit tensors really were used (fp16 saved activations, bf16 internal gradients) exactly when asked for
    assert any(c == torch.float16 for _, c, _ in seen) == (act != "none") and any(g == torch.bfloat16 and b for g, _, b in seen) == io16

    def cos(a, b):
        return float((a.double() * b.double()).sum() / (a.double().norm() * b.double().norm()).clamp_min(1e-300))

    assert O.rel_l2(res["f16"][0], res["f32"][0]) <= (1.5e-3 if act != "none" else TOL_HEAD)
    assert float(res["f32"][2].abs().max()) < 6e-5            # the input gradient really is below fp16's normal range
    # train-mode BatchNorm backward subtracts the batch means of dy and dy*xhat: what is left after that cancellation carries
    # the 1e-3 forward difference amplified, so the bound on a gradient is its direction (cosine) plus a loose norm bound
    assert cos(res["f16"][2], res["f32"][2]) >= 0.99 and O.rel_l2(res["f16"][2], res["f32"][2]) <= 0.15
    gmax = max(float(g.norm()) for g in res["f32"][1].values())
    rels = []
    for k, g in res["f32"][1].items():
        if float(g.norm()) > 1e-3 * gmax:
            assert cos(res["f16"][1][k], g) >= 0.99, k
            rels.append(O.rel_l2(res["f16"][1][k], g))
    assert len(rels) > 10 and sorted(rels)[len(rels) // 2] <= 3e-2, sorted(rels)


def test_fp16_activation_chain_within_tolerance(monkeypatch):
    """hrfuse.FP16_ACTIVATIONS (the default since round 3): every conv of the inference head reads / writes fp16 NHWC tensors
    (srbh_hconv_args.io_h16), bn1 + ReLU in conv1's epilogue, fp16 residual stream.  Whole model, eval, no_grad: height / building
    maps within the 1e-3 tolerance of the CPU reference and 1e-3 of the fp32-tensor chain; the public modules still return fp32."""
    import copy
    from srbh_amd import hrfuse as H
    from srbh_amd.hrfuse import HRfeature
    from tests.test_gpu_model import cpu_reference, make_model
    m = make_model(seed=41).eval()
    x = synth.tiles(2, 8, 64, seed=43)
    fea = torch.randn(2, 64, 256, 256, generator=torch.Generator().manual_seed(44)) * 0.5
    with torch.no_grad():
        want = cpu_reference(copy.deepcopy(m), x, fea, False)
        m = m.to(DEV)
        monkeypatch.setattr(H, "FP16_ACTIVATIONS", False)      # the fp32-tensor chain (the default is the fp16 chain since round 3)
        base = m(x.to(DEV), fea.to(DEV))
        monkeypatch.setattr(H, "FP16_ACTIVATIONS", True)
        got = m(x.to(DEV), fea.to(DEV))
        feat = m.hrfeat(fea.to(DEV))
        feat16 = m.hrfeat(fea.to(DEV), out_h16=True)
    assert feat.dtype == torch.float32 and feat16.dtype == torch.float16
    assert O.rel_l2(feat16.float().cpu(), feat.cpu()) <= 1e-3
    for a, b, c, name in zip(got, want, base, ("height", "build", "aggre")):
        assert a.dtype == torch.float32
        assert O.rel_l2(a.cpu(), b) <= TOL_HEAD, name
        d = O.rel_l2(a.cpu(), c.cpu())
        assert d <= TOL_HEAD, name
        if name != "aggre":                      # (aggre comes from decoder1 alone: no head chain in it, and the decoders are deterministic now)
            assert d > 0, name                   # the fp16 chain really ran


@pytest.mark.parametrize("c0,c1,hw,stats", [(64, 0, (8, 64), True), (16, 16, (12, 128), False), (64, 16, (4, 64), True), (16, 0, (8, 70), False)])
def test_block_entry_fused_conv_pair_equals_the_two_convs(c0, c1, hw, stats):
    """srbh_hconv_entry_h16: conv1 (3x3) + downsample[0] (1x1) of a BasicBlock entry over the same (concatenated) input in one pass
    (srbh_hconv_entry_kernel.h) must give the numbers of the two separate fp16-operand convs: outputs <= 1e-6 (same rounding, same
    accumulation order per pixel), BatchNorm partial sums <= 1e-6 relative.  The last shape (W = 70) takes the fallback inside the call."""
    from srbh_amd import hrfuse as H
    Hh, Ww = hw
    conv1 = torch.nn.Conv2d(c0 + c1, 16, 3, 1, 1, bias=False).to(DEV)
    convd = torch.nn.Conv2d(c0 + c1, 16, 1, 1, 0, bias=False).to(DEV)
    with torch.no_grad():
        conv1.weight.copy_(rnd(tuple(conv1.weight.shape), 3, -0.3, 0.3))
        convd.weight.copy_(rnd(tuple(convd.weight.shape), 4, -0.5, 0.5))
    srcs = [H.to_nhwc(rnd((3, c0, Hh, Ww), 5).to(DEV))] + ([H.to_nhwc(rnd((3, c1, Hh, Ww), 6).to(DEV))] if c1 else [])
    sd, hd = rnd((16,), 7, 0.5, 1.5).to(DEV), rnd((16,), 8, -0.2, 0.2).to(DEV)
    H.set_head_precision("f16")
    try:
        a, sa = H.hconv(srcs, conv1, H._PackedConv(), want_stats=stats)
        b, sb = H.hconv(srcs, convd, H._PackedConv(), want_stats=stats, post=None if stats else (sd, hd))
        c1o, s1, d, s2 = H.hconv_entry(srcs, conv1, H._PackedConv(), convd, H._PackedConv(), want_stats=stats, postd=None if stats else (sd, hd))
    finally:
        H.set_head_precision("auto")
    assert O.rel_l2(c1o.cpu(), a.cpu()) <= 1e-6 and O.rel_l2(d.cpu(), b.cpu()) <= 1e-6
    if stats:
        fold = lambda t: t.view(-1, 2, 16).sum(0)
        assert O.rel_l2(fold(s1).cpu(), fold(sa).cpu()) <= 1e-6 and O.rel_l2(fold(s2).cpu(), fold(sb).cpu()) <= 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("c0,c1,x16,g16,shape", [(64, 0, False, False, (2, 20, 72)), (64, 0, True, True, (2, 20, 72)), (16, 16, False, True, (2, 20, 72)),
                                                 (16, 16, False, False, (2, 20, 72)), (32, 0, False, True, (2, 20, 72)),
                                                 (64, 0, True, False, (2, 20, 72)), (64, 0, True, True, (5, 250, 200)), (16, 16, False, True, (5, 250, 200)),
                                                 (48, 0, False, False, (2, 20, 72)), (32, 16, False, True, (2, 20, 72))])
def test_fused_entry_weight_gradients_equal_the_two_separate_calls(c0, c1, x16, g16, shape):
    """srbh_hconv_wgrad_entry_b16 (round 4): conv1's 3x3 and downsample[0]'s 1x1 weight gradients of a BasicBlock entry
    (SR/HRfuse.py:142-159) in ONE pass over the shared input -- the same bf16 products in the same order as the two separate
    srbh_hconv_wgrad_b16 calls: bit-identical results; ragged size included.  The chunk-inner kernel (2 / 4 chunks) and the whole-row
    kernel of the 64-channel fp16 features (its register prefetch of the next tile: 640 tiles on 512 workgroups) are these calls' paths;
    three input chunks (48, 32 + 16) take the chunk-outer fused kernel."""
    from srbh_amd import hrfuse as H
    from srbh_amd import hrfuse_autograd as HA
    dev = "cuda:0"
    g = torch.Generator().manual_seed(c0 + c1)
    B, Hh, Ww = shape                            # (not multiples of the 8 x 64 tile)
    nhwc = lambda t: t.to(dev).contiguous(memory_format=torch.channels_last)        # noqa: E731
    x0 = nhwc(torch.randn((B, c0, Hh, Ww), generator=g))
    if x16:
        x0 = x0.half()
    srcs = [x0] + ([nhwc(torch.randn((B, c1, Hh, Ww), generator=g))] if c1 else [])
    g3 = nhwc(torch.randn((B, 16, Hh, Ww), generator=g) * 1e-3)
    g1 = nhwc(torch.randn((B, 16, Hh, Ww), generator=g) * 1e-3)
    if g16:
        g3, g1 = g3.bfloat16(), g1.bfloat16()
    with H.head_precision("f16"), torch.no_grad():
        d3, d1 = HA.conv_wgrad_entry(srcs, g3, g1, 16)
        r3, r1 = HA.conv_wgrad(srcs, None, g3, 16, 3), HA.conv_wgrad(srcs, None, g1, 16, 1)
    assert torch.equal(d3, r3) and torch.equal(d1, r1)
    assert float(d3.abs().max()) > 0 and float(d1.abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("C,shape,b16", [(16, (2, 24, 72), False), (16, (3, 8, 64), True), (64, (1, 12, 20), False), (4, (2, 5, 7), True)])
def test_relu_bit_pattern_equals_the_fp32_reference_in_the_backward_reduce(C, shape, b16):
    """Round 4: bn_add_relu also writes the block-closing ReLU's activity pattern as bits (srbh_bn_add_relu_bits); the BatchNorm backward's
    reduce pass (srbh_bn_bwd_reduce_io + SRBH_BN_REF_BITS) masks with them instead of reading the fp32 block output: same dz, same dc,
    same dgamma / dbeta, bit for bit; sizes that are not multiples of 64 groups included."""
    from srbh_amd import hrfuse as H
    from srbh_amd import hrfuse_autograd as HA
    dev = "cuda:0"
    B, Hh, Ww = shape
    g = torch.Generator().manual_seed(C + Hh)
    nhwc = lambda t: t.to(dev).contiguous(memory_format=torch.channels_last)        # noqa: E731
    a, idt = nhwc(torch.randn((B, C, Hh, Ww), generator=g)), nhwc(torch.randn((B, C, Hh, Ww), generator=g))
    sa, ha = (torch.rand(C, generator=g) + 0.5).to(dev), (torch.randn(C, generator=g) * 0.1).to(dev)
    out0 = H.bn_add_relu(a, sa, ha, idt)
    out1, bits = H.bn_add_relu(a, sa, ha, idt, want_bits=True)
    assert torch.equal(out0, out1) and bits.dtype == torch.int64
    assert 0.2 < float((out0 > 0).float().mean()) < 0.8
    gy = nhwc(torch.randn((B, C, Hh, Ww), generator=g))
    mean, invstd, gamma = (torch.randn(C, generator=g) * 0.1).to(dev), (torch.rand(C, generator=g) + 0.5).to(dev), (torch.rand(C, generator=g) + 0.5).to(dev)
    r0 = HA.bn_backward(gy, a, mean, invstd, gamma, None, True, relu_ref=out0, out_b16=b16)
    r1 = HA.bn_backward(gy, a, mean, invstd, gamma, None, True, relu_ref=bits, out_b16=b16)
    dc0, dg0, db0, dz0 = r0
    dc1, dg1, db1, dz1 = r1
    assert dz0.dtype == dz1.dtype and torch.equal(dz0, dz1)          # the masked gradient: elementwise, identical
    assert float((dz0.float() == 0).float().mean()) > 0.2            # ... and really masked
    # the sums go through atomics (order-dependent last bits), and dc carries their means: close, not identical
    # (bounded against the LARGEST element: a sum that happens to land near zero carries the same absolute noise as the others, and an
    #  element-wise rtol on it failed once in a few full-suite runs)
    close = lambda u, v, tol: float((u.double() - v.double()).abs().max()) <= tol * float(v.double().abs().max())      # noqa: E731
    assert close(dg0, dg1, 1e-4) and close(db0, db1, 1e-4)
    # dc is elementwise in (dz, c) given the statistics: the two runs differ only through the atomically summed means, so a masking or
    # summation bug in the bit path shows up as a LARGE relative difference -- rel-L2, not a max-normalised bound (round-4 ADVICE)
    rel = float((dc0.double() - dc1.double()).norm() / dc1.double().norm())
    assert dc0.dtype == dc1.dtype and rel <= (5e-3 if b16 else 1e-3), rel


@pytest.mark.gpu
@pytest.mark.parametrize("cout_fwd", [7, 1, 12])
def test_narrow_input_data_gradient_on_the_persistent_kernel(cout_fwd):
    """The data gradients of the 1- / 7-channel output convs (conv_last of the two fuse heads, SR/HRfuse.py:188-189: dX = conv^T(dY[7], W))
    on the persistent 16 -> 16 kernel's narrow-input form (round 4; they ran the template at 0.2 of the HBM roofline): bf16 operands against
    a float64 transposed convolution of the same rounded operands, with a skip gradient added, and the form is COUNTED as hconv16."""
    import torch.nn.functional as F
    from srbh_amd import _lib
    from srbh_amd import hrfuse as H
    from srbh_amd import hrfuse_autograd as HA
    dev = "cuda:0"
    g = torch.Generator().manual_seed(cout_fwd)
    conv = torch.nn.Conv2d(16, cout_fwd, 3, 1, 1).to(dev)
    dy = (torch.randn((2, cout_fwd, 8, 128), generator=g) * 1e-3).to(dev).contiguous(memory_format=torch.channels_last)
    res = torch.randn((2, 16, 8, 128), generator=g).to(dev).contiguous(memory_format=torch.channels_last) * 1e-3
    with H.head_precision("f16"), torch.no_grad():
        _lib.path_counters(reset=True)
        dx = HA.conv_dgrad(dy, conv.weight, HA._PackedGrad())
        dxr = HA.conv_dgrad(dy, conv.weight, HA._PackedGrad(), res=res)
        c = _lib.path_counters(reset=True)
    assert c["hconv16"] == 2 and c["hconv_template"] == 0, c
    b = lambda t: t.detach().bfloat16().double()             # noqa: E731
    want = F.conv_transpose2d(b(dy), b(conv.weight), None, 1, 1)
    rel = lambda a, w: float((a.double() - w).norm() / w.norm())      # noqa: E731
    assert rel(dx, want) <= 2e-6
    assert rel(dxr, want + res.double()) <= 2e-6


@pytest.mark.gpu
@pytest.mark.parametrize("B,hw", [(2, 64), (3, 32), (1, 128), (5, 64)])
def test_upsampler_persistent_kernel_equals_the_template(B, hw, monkeypatch):
    """Round 4: the Upsampler's conv3x3 16 -> 64 + PixelShuffle(2) (SR/HRfuse.py:17-44) on hconv_up_kernel -- persistent walk, weights
    packed sub-pixel-major so that the PixelShuffle store needs no LDS pass (srbh_hconv_args.pixelshuffle2 == 2) -- against the template
    kernel with the standard pack: the same products in the same order, bit-identical, for fp32 and fp16 outputs and fp16 intermediates;
    a 32 x 32 input takes the template for its first conv (W % 64 != 0) and the new kernel for the second; the training-mode forward
    (fp16 operands) goes through the same kernel and its gradients do not change."""
    from srbh_amd import hrfuse as H
    dev = "cuda:0"
    torch.manual_seed(B * 7 + hw)
    up = H.Upsampler(scale=4, n_feats=16).to(dev).eval()
    with torch.no_grad():
        for p in up.parameters():
            p.mul_(3.0)                              # (biases and weights of visible size)
    x = torch.randn((B, 16, hw, hw), device=dev)
    outs = {}
    for flag in (True, False):
        monkeypatch.setattr(H, "HCONV_UP", flag)
        for m in up._packs.values():
            m.key = None
        with torch.no_grad():
            outs[flag] = (up(x), up(x, out_h16=True))
    assert outs[True][0].shape == (B, 16, 4 * hw, 4 * hw) and outs[True][1].dtype == torch.float16
    assert torch.equal(outs[True][0], outs[False][0]) and torch.equal(outs[True][1], outs[False][1])
    assert float(outs[True][0].abs().max()) > 0.1
    # training mode, fp16-operand head: forward through the same kernel, gradients from the unchanged gradient kernels
    res = {}
    for flag in (True, False):
        monkeypatch.setattr(H, "HCONV_UP", flag)
        up.train()
        for p in up.parameters():
            p.grad = None
        xg = x.clone().requires_grad_(True)
        with H.head_precision("f16"):
            y = up(xg)
            y.square().sum().backward()
        res[flag] = (y.detach().clone(), xg.grad.clone(), [p.grad.clone() for p in up.parameters()])
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])
    for a, b in zip(res[True][2], res[False][2]):
        # (weight gradients are deterministic; the bias gradients come out of atomically added partial sums -- order-dependent last bits
        #  of sums of ~1e5 terms, bounded against the LARGEST element: an element-wise rtol failed for small sums in ~1 of 7 runs)
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("B,Hh,Ww,g16", [(2, 20, 72, False), (3, 64, 64, False), (5, 250, 200, False), (2, 24, 64, True)])
def test_upsampler_weight_gradient_with_the_output_blocks_inside_the_walk(B, Hh, Ww, g16):
    """Round 4: the 16 -> 64 weight gradient (the Upsampler convs, SR/HRfuse.py:17-44) on hwgrad_ob_b16_kernel -- X staged once per tile, the
    four dY blocks inside the tile walk -- against float64 products of the SAME bf16-rounded operands (what remains is fp32 summation
    order); ragged sizes, 640 tiles on 512 workgroups, fp32 and bf16 dY."""
    import torch.nn.functional as F
    from srbh_amd import hrfuse as H
    from srbh_amd import hrfuse_autograd as HA
    from srbh_amd import _lib
    dev = "cuda:0"
    g = torch.Generator().manual_seed(B + Ww)
    nhwc = lambda t: t.to(dev).contiguous(memory_format=torch.channels_last)        # noqa: E731
    x = nhwc(torch.randn((B, 16, Hh, Ww), generator=g))
    gy = nhwc(torch.randn((B, 64, Hh, Ww), generator=g) * 1e-2)
    if g16:
        gy = gy.bfloat16()
    with H.head_precision("f16"), torch.no_grad():
        _lib.path_counters(reset=True)
        dw = HA.conv_wgrad([x], None, gy, 64, 3)
        assert _lib.path_counters()["wgrad_b16_generic"] == 1
    xr, gr = x.bfloat16().double(), gy.bfloat16().double()
    w0 = torch.zeros((64, 16, 3, 3), dtype=torch.float64, device=dev, requires_grad=True)
    F.conv2d(xr, w0, padding=1).mul(gr).sum().backward()
    assert dw.shape == (64, 16, 3, 3)
    assert float((dw.double() - w0.grad).norm() / w0.grad.norm()) <= 1e-5


def _upsampler_wgrad(B, Hh, Ww, g16, save_to=None):
    """(the 16 -> 64 weight gradient of seeded, CPU-built inputs -- the same bits in every process --, the names of the hwgrad kernels that ran)"""
    from torch.profiler import ProfilerActivity, profile
    from srbh_amd import hrfuse as H
    from srbh_amd import hrfuse_autograd as HA
    g = torch.Generator().manual_seed(B + Ww)
    nhwc = lambda t: t.to("cuda:0").contiguous(memory_format=torch.channels_last)        # noqa: E731
    x = nhwc(torch.randn((B, 16, Hh, Ww), generator=g))
    gy = nhwc(torch.randn((B, 64, Hh, Ww), generator=g) * 1e-2)
    if g16:
        gy = gy.bfloat16()
    with H.head_precision("f16"), torch.no_grad(), profile(activities=[ProfilerActivity.CUDA]) as prof:
        dw = HA.conv_wgrad([x], None, gy, 64, 3).cpu()
    kernels = sorted({e.key for e in prof.key_averages() if "hwgrad" in e.key and "reduce" not in e.key})
    if save_to:
        torch.save({"dw": dw, "kernels": kernels}, save_to)
    return dw, kernels


@pytest.mark.gpu
@pytest.mark.parametrize("g16", [False, True])
@pytest.mark.parametrize("B,Hh,Ww", [(2, 20, 72), (5, 250, 200)])
def test_output_blocks_inside_the_walk_equal_the_grid_of_output_blocks(B, Hh, Ww, g16, tmp_path):
    """hwgrad_ob_b16_kernel (the four dY blocks inside the tile walk) against hwgrad_b16_kernel with grid.y = 4 (SRBH_WGRAD_OB_INNER=0, read
    once per process: a fresh child): same walk, products and flush, so the 16 -> 64 gradient is the same bits; a ragged shape and 640 tiles
    on 512 workgroups, fp32 and bf16 dY.  Which kernel ran in which process is read from the profiler's kernel names: were the knob
    ignored, the test would compare a kernel with itself."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "dw.pt")
    code = ("import sys; sys.path.insert(0, %r); from tests import test_gpu_head_f16 as T; T._upsampler_wgrad(%d, %d, %d, %r, %r)"
            % (root, B, Hh, Ww, g16, out))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(os.environ, SRBH_WGRAD_OB_INNER="0"), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    dw, kernels = _upsampler_wgrad(B, Hh, Ww, g16)
    ref = torch.load(out)
    assert len(kernels) == 1 and "hwgrad_ob_b16_kernel" in kernels[0], kernels
    assert len(ref["kernels"]) == 1 and "hwgrad_b16_kernel" in ref["kernels"][0], ref["kernels"]
    assert dw.shape == (64, 16, 3, 3) and float(dw.abs().max()) > 0
    assert torch.equal(dw, ref["dw"])


def test_packs_refreshed_behind_the_optimizer_step_equal_the_lazy_packs():
    """hrfuse.PACKS: the fp16 forward packs and bf16 gradient packs of the bias-free head convs register themselves when they are first made;
    optimizer.step() -- through wcache's post-step hook -- rewrites all of them in ONE launch (srbh_hpack_conv_h16_many) and moves their keys
    to the new generation: the next forward finds every pack current (no pack launch) and every buffer equals what the lazy per-conv pack
    makes of the stepped weight, bit for bit."""
    from srbh_amd import _lib, hrfuse as H, hrfuse_autograd as HA
    dev = "cuda:0"
    torch.manual_seed(2)
    m = H.HRfeature(64, 16, 16).to(dev).train()
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    x = torch.randn(2, 64, 64, 64, device=dev).contiguous(memory_format=torch.channels_last)
    H.PACKS.entries.clear()
    H.PACKS.tables.clear()
    with H.head_precision("f16"):
        for it in range(2):
            opt.zero_grad(set_to_none=True)
            m(x).square().mean().backward()
            if it == 0:
                n_reg = len(H.PACKS.entries)
                assert n_reg >= 10, n_reg                      # 6 3x3 convs + the 1x1 downsample, forward and gradient packs
            opt.step()
        torch.cuda.synchronize()
        assert len(H.PACKS.entries) == n_reg                   # the second step's forward / backward found every pack current: nothing re-registered
        checked = 0
        for e in H.PACKS.entries.values():
            cache, p = e["cache"](), e["param"]()
            co, ci, ks, tf, bf = e["args"]
            want = torch.empty_like(e["buf"])
            _lib.check(_lib.lib().srbh_hpack_conv_h16(p.detach().contiguous().data_ptr(), co, ci, ks, tf, bf, want.data_ptr(), _lib.stream_ptr()), "pack")
            torch.cuda.synchronize()
            assert torch.equal(e["buf"].view(torch.int16), want.view(torch.int16))
            assert cache.key == e["rekey"]()                  # current for this state of the weight
            checked += 1
        assert checked == n_reg
