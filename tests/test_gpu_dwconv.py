"""Depthwise conv kernels (csrc/srbh_dwconv.hip) against the float64 oracle of the same operation (tests/encoder_kernels_oracle.py):
forward, input gradient, weight gradient, every (K, stride, static-same padding) combination the EfficientNet-B4 encoder uses, through
the C ABI (autograd Function in encoders.py, and directly for the batch-slice, LDS-limit and grid-stride cases).  Tolerance 1e-5 relative
L2 on each whole tensor (fp32 sums against float64) and 4e-5 on the worst single plane of y and dx and the worst single channel of dw, so
that an error confined to one border or one channel cannot hide in the norm; the weight gradient gives the same bits on a second run.
The error of the stock fp32 op against the same oracle is printed next to each figure.  Then the fused inference forms of the encoder.

Measured on an MI355X, largest error over all depthwise cases, whole tensor / worst plane or channel (the stock fp32 op's beside it):
  srbh_dwconv_fwd         8.8e-8 / 2.6e-7   (stock 1.2e-7 / 1.3e-7)
  srbh_dwconv_bwd_data    6.6e-8 / 2.1e-7   (stock 1.1e-7 / 2.6e-7)
  srbh_dwconv_bwd_weight  1.7e-7 / 3.9e-7   (stock 1.2e-6 / 3.2e-6)"""
import pytest, torch
import torch.nn.functional as F

from tests import encoder_kernels_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _worst_slice(a, b, keep):
    """the largest rel-L2 over the slices indexed by the first `keep` dimensions (planes of y / dx: keep = 2; channels of dw: keep = 1)"""
    a, b = a.detach().double().cpu().flatten(keep), b.detach().double().cpu().flatten(keep)
    return float(((a - b).norm(dim=-1) / b.norm(dim=-1).clamp_min(1e-30)).max())


def _hold(tag, what, got, want, stock, keep):
    """whole-tensor rel-L2 <= TOL and the worst plane / channel <= 4 TOL against the float64 oracle; prints both and the stock fp32 op's"""
    got, stock = got.detach().cpu(), stock.detach().cpu()
    e, w = rel(got, want), _worst_slice(got, want, keep)
    print(f"dwconv {tag} {what}: err {e:.3e}, worst {'plane' if keep == 2 else 'channel'} {w:.3e} (stock fp32 op {rel(stock, want):.3e}, {_worst_slice(stock, want, keep):.3e})")
    assert got.shape == want.shape
    assert e <= TOL, (tag, what, e)
    assert w <= 4 * TOL, (tag, what, w)


def _stock(x, w, stride, pad, gy):
    """(y, dx, dw) of the stock fp32 op on the device"""
    xr, wr = x.detach().clone().requires_grad_(True), w.detach().clone().requires_grad_(True)
    yr = F.conv2d(F.pad(xr, pad), wr, None, stride, 0, 1, x.shape[1])
    dx, dw = torch.autograd.grad(yr, (xr, wr), gy)
    return yr.detach(), dx, dw


def _wgrad_direct(x, gy, K, stride, pad, bufs):
    """srbh_dwconv_bwd_weight through the C ABI into a guarded output, its scratch pre-filled with NaN: a single batch slice must not read
    it, several slices must write every slot before the reduce reads it -- either way dw comes out without a NaN"""
    from srbh_amd import _lib
    L = _lib.lib()
    B, C, H, W = x.shape
    OH, OW = gy.shape[-2:]
    dw = bufs.out((C, 1, K, K))
    ws = torch.full((L.srbh_dwconv_bwd_weight_splits(B, C) * C * K * K,), float("nan"), device=DEV)
    _lib.check(L.srbh_dwconv_bwd_weight(x.data_ptr(), gy.data_ptr(), dw.data_ptr(), ws.data_ptr(), B, C, H, W, K, stride, pad[2], pad[0], OH, OW,
                                        _lib.stream_ptr()), "dwconv_bwd_weight")
    return dw


@pytest.mark.parametrize("K,stride,H,pad", [
    (3, 1, 32, (1, 1, 1, 1)), (3, 2, 32, (0, 1, 0, 1)), (5, 2, 16, (1, 2, 1, 2)), (5, 1, 8, (2, 2, 2, 2)), (3, 1, 4, (1, 1, 1, 1)),
    (5, 2, 4, (1, 2, 1, 2)), (5, 1, 2, (2, 2, 2, 2)), (3, 1, 2, (1, 1, 1, 1)), (5, 2, 7, (2, 2, 2, 2)), (3, 2, 9, (1, 1, 1, 1)),
])
def test_depthwise_conv_matches_stock_op(K, stride, H, pad):
    from srbh_amd.encoders import _DepthwiseConvFn
    from tests.gpu_util import GuardedBuffers
    g = torch.Generator().manual_seed(K * 100 + stride * 10 + H)
    B, C, W = 5, 37, H + (1 if H > 4 else 0)
    x0, w0 = torch.randn((B, C, H, W), generator=g), torch.randn((C, 1, K, K), generator=g) * 0.3
    x, w = x0.to(DEV).requires_grad_(True), w0.to(DEV).requires_grad_(True)
    y = _DepthwiseConvFn.apply(x, w, stride, pad)
    gy0 = torch.randn(y.shape, generator=g)
    gy = gy0.to(DEV)
    y.backward(gy)
    want_y, want_dx, want_dw = O.dwconv_grads(x0, w0, stride, pad, gy0)
    st_y, st_dx, st_dw = _stock(x, w, stride, pad, gy)
    tag = f"K={K} s={stride} {B}x{C}x{H}x{W}"
    _hold(tag, "y", y, want_y, st_y, 2)
    _hold(tag, "dx", x.grad, want_dx, st_dx, 2)
    _hold(tag, "dw", w.grad, want_dw, st_dw, 1)
    bufs = GuardedBuffers()
    dw2 = _wgrad_direct(x.detach(), gy, K, stride, pad, bufs)
    bufs.verify()
    assert torch.equal(dw2, w.grad)          # include/srbh.h: "bwd_weight sums in a fixed order (deterministic)"


def _direct(B, C, H, W, K, stride):
    """forward and both gradients through the C ABI under the encoder's "same" padding, every output guarded, the weight gradient twice;
    held to the oracle"""
    from srbh_amd import _lib
    from tests.gpu_util import GuardedBuffers
    L = _lib.lib()
    pad, OH, OW = O.same_geometry(H, W, K, stride)
    g = torch.Generator().manual_seed(B * 7919 + C * 31 + H * 5 + K + stride)
    x0, w0 = torch.randn((B, C, H, W), generator=g), torch.randn((C, 1, K, K), generator=g) * 0.3
    gy0 = torch.randn((B, C, OH, OW), generator=g)
    bufs = GuardedBuffers()
    x, w, gy = bufs.inp(x0), bufs.inp(w0), bufs.inp(gy0)
    y, dx = bufs.out(gy0.shape), bufs.out(x0.shape)
    geo = (B, C, H, W, K, stride, pad[2], pad[0], OH, OW, _lib.stream_ptr())
    _lib.check(L.srbh_dwconv_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), *geo), "dwconv_fwd")
    _lib.check(L.srbh_dwconv_bwd_data(gy.data_ptr(), w.data_ptr(), dx.data_ptr(), *geo), "dwconv_bwd_data")
    dw = _wgrad_direct(x, gy, K, stride, pad, bufs)
    dw2 = _wgrad_direct(x, gy, K, stride, pad, bufs)
    bufs.verify()
    want_y, want_dx, want_dw = O.dwconv_grads(x0, w0, stride, pad, gy0)
    st_y, st_dx, st_dw = _stock(x, w, stride, pad, gy)
    tag = f"K={K} s={stride} {B}x{C}x{H}x{W}"
    _hold(tag, "y", y, want_y, st_y, 2)
    _hold(tag, "dx", dx, want_dx, st_dx, 2)
    _hold(tag, "dw", dw, want_dw, st_dw, 1)
    assert torch.equal(dw, dw2)


@pytest.mark.parametrize("case,prop", O.DW_SLICE_CASES)
def test_depthwise_weight_gradient_batch_slices(case, prop):
    """the batch slices of srbh_dwconv_bwd_weight beyond one image each: several staging rounds per slice with a ragged last round (70 images
    in 4 slices of 17 / 18, 4 planes per round), slices of 3 and 4 images, and a single slice, which writes dw itself with no reduce
    launch and leaves the scratch alone (tests/test_encoder_kernels_cpu.py holds each shape to its property)"""
    B, C = case[:2]
    from srbh_amd import _lib
    assert _lib.lib().srbh_dwconv_bwd_weight_splits(B, C) == O.wgrad_splits(B, C)
    assert (O.wgrad_splits(B, C) == 1) == (prop == "single_slice")
    _direct(*case)


@pytest.mark.parametrize("case,staged", O.DW_LIMIT_CASES)
def test_depthwise_conv_either_side_of_the_lds_limit(case, staged):
    """Planes just under and over the 61 440 bytes of LDS (15 360 floats) up to which the dispatcher stages a plane; beyond, the
    one-thread-per-output kernels run.  One plane per round at these sizes (P = 1), B = 2, C = 3, "same" padding, OH = ceil(H / s):
      forward          (PH PW + K K) floats, PH = (OH - 1) s + K
        K = 3, s = 1:  (H + 2)(W + 2) + 9;    117 x 127: 119 * 129 + 9 = 15 360 (exactly the limit: staged);  122 x 124: 124 * 126 + 9 = 15 633 (over)
        K = 5, s = 2:  114 x 127 (OH 57, OW 64): 117 * 131 + 25 = 15 352 (under);                               122 x 124 (61, 62): 125 * 127 + 25 = 15 900 (over)
      input gradient   (PH PW + K K) floats, PH = (OH - 1) s + 2 (K - 1) + s + 1
        K = 3, s = 1:  (H + 5)(W + 5) + 9;    114 x 124: 119 * 129 + 9 = 15 360 (exactly the limit);            117 x 127: 122 * 132 + 9 = 16 113 (over)
        K = 5, s = 2:  (2 OH + 9)(2 OW + 9) + 25;  107 x 122 (54, 61): 117 * 131 + 25 = 15 352 (under);          114 x 127 (57, 64): 123 * 137 + 25 = 16 876 (over)
      weight gradient  (PH PW + OH OW) floats, PH = (OH - 1) s + K  (K = 5; a 3 x 3 over >= 256-pixel planes never stages)
        K = 5, s = 2:  96 x 121 (48, 61): 99 * 125 + 48 * 61 = 15 303 (under);   98 x 119 (49, 60): 101 * 123 + 49 * 60 = 15 363 (3 floats over)
    122 x 124 is over the limit for all three at K = 3, s = 1 and at K = 5, s = 2.  tests/test_encoder_kernels_cpu.py checks this table
    against the restated formulas."""
    B, C, H, W, K, stride = case
    assert {k: O.staged(k, H, W, K, stride) for k in staged} == staged
    _direct(*case)


def test_depthwise_fallback_kernels_beyond_one_grid_stride():
    """3 x 47 planes of 122 x 124: the one-thread-per-output kernels with more than 8192 * 256 outputs, so that the capped grid strides"""
    B, C, H, W, K, stride = O.DW_WRAP_CASE
    assert B * C * H * W > O.GRID_CAP_ITEMS and not O.staged("fwd", H, W, K, stride) and not O.staged("dgrad", H, W, K, stride)
    _direct(*O.DW_WRAP_CASE)


def test_encoder_uses_the_kernels_and_agrees_with_the_stock_path():
    from srbh_amd import encoders
    torch.manual_seed(3)
    enc = encoders.get_encoder("efficientnet-b4", in_channels=8, depth=5, weights=None).to(DEV).eval()
    dws = [m for m in enc.modules() if isinstance(m, encoders.SamePadConv2d) and m._depthwise]
    assert len(dws) == 32
    x = torch.rand((3, 8, 64, 64), device=DEV)
    with torch.no_grad():
        a = enc(x)
        for m in dws:
            m._depthwise = False
        b = enc(x)
    for u, v in zip(a, b):
        assert u.shape == v.shape and rel(u, v) <= 1e-5


def test_bad_arguments_are_errors():
    from srbh_amd import _lib
    x = torch.zeros((1, 2, 4, 4), device=DEV)
    w = torch.zeros((2, 1, 7, 7), device=DEV)
    y = torch.zeros((1, 2, 4, 4), device=DEV)
    rc = _lib.lib().srbh_dwconv_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), 1, 2, 4, 4, 7, 1, 3, 3, 4, 4, _lib.stream_ptr())
    assert rc != 0
    with pytest.raises(RuntimeError):
        _lib.check(rc, "dwconv_fwd")


def test_fused_inference_batchnorm_agrees_with_the_stock_path():
    """encoder + U-Net decoder in eval mode: BatchNorm(+SiLU/ReLU) as one libsrbh affine pass vs MIOpen's inference BN"""
    from srbh_amd import encoders
    from srbh_amd import hrfuse as H
    # (exact-fp32 decoder convs: with the round-4 fp16-operand decoder convs a 1e-7 difference between the two BatchNorm paths flips
    #  fp16 roundings downstream and shows as 3e-5 -- this test is about the BatchNorm kernels)
    with H.head_precision("f32"):
        _fused_bn_body()


def _fused_bn_body():
    from srbh_amd import encoders
    torch.manual_seed(5)
    enc = encoders.get_encoder("efficientnet-b4", in_channels=8, depth=5, weights=None).to(DEV)
    dec = encoders.UnetDecoder(enc.out_channels, (256, 128, 64, 32, 16), n_blocks=5, use_batchnorm=True, center=False,
                               attention_type=None).to(DEV)
    x = torch.rand((4, 8, 64, 64), device=DEV)
    enc.train(); dec.train()
    with torch.no_grad():
        for _ in range(2):
            dec(*enc(x))          # non-trivial running statistics
    enc.eval(); dec.eval()
    with torch.no_grad():
        a = dec(*enc(x))
        encoders.FUSED_BN_EVAL = False
        try:
            b = dec(*enc(x))
        finally:
            encoders.FUSED_BN_EVAL = True
    assert rel(a, b) <= 1e-5
    # a parameter update invalidates the cached affine
    with torch.no_grad():
        enc._bn0.weight.mul_(1.5)
        a2 = enc(x)[1]
        encoders.FUSED_BN_EVAL = False
        try:
            b2 = enc(x)[1]
        finally:
            encoders.FUSED_BN_EVAL = True
    assert rel(a2, b2) <= 1e-5



@pytest.mark.parametrize("B,C,H,K,stride", [(3, 24, 32, 3, 1), (2, 40, 32, 5, 2), (5, 96, 16, 3, 2), (7, 50, 8, 5, 1), (33, 48, 4, 5, 1),
                                            (9, 130, 4, 3, 2), (66, 72, 2, 3, 1), (1, 16, 16, 5, 1)])
@pytest.mark.parametrize("pre", [True, False])
def test_fused_inference_depthwise_bn_swish_pool_kernel(B, C, H, K, stride, pre):
    """srbh_dwconv_eval_fwd (round 4): swish(bn0) while staging, depthwise conv, swish(bn1) + per-plane mean in the epilogue == the torch
    chain on the same folded affines; TF-'same' padding of the encoder (odd total padding at stride 2); ragged plane counts per
    workgroup; the pooled means bit-identical between two runs (fixed reduction tree)."""
    import math
    from srbh_amd import _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(B * 131 + C)
    x = torch.randn((B, C, H, H), generator=g).to(DEV)
    w = (torch.randn((C, 1, K, K), generator=g) * 0.3).to(DEV)
    a0, b0, a1, b1 = [(torch.rand(C, generator=g) + 0.5).to(DEV) if i % 2 == 0 else (torch.randn(C, generator=g) * 0.2).to(DEV) for i in range(4)]
    OH = math.ceil(H / stride)
    pad = max((OH - 1) * stride + K - H, 0)
    pt = pad // 2
    assert L.srbh_dwconv_eval_supported(B, C, H, H, K, stride, pt, pt, OH, OH)
    y = torch.empty((B, C, OH, OH), device=DEV)
    pooled = torch.empty((B, C), device=DEV)
    args = (x.data_ptr(), w.data_ptr(), a0.data_ptr() if pre else None, b0.data_ptr() if pre else None, a1.data_ptr(), b1.data_ptr())
    _lib.check(L.srbh_dwconv_eval_fwd(*args, y.data_ptr(), pooled.data_ptr(), B, C, H, H, K, stride, pt, pt, OH, OH, _lib.stream_ptr()), "dwconv_eval_fwd")
    e = F.silu(x * a0.view(1, -1, 1, 1) + b0.view(1, -1, 1, 1)) if pre else x
    z = F.conv2d(F.pad(e.double(), (pt, pad - pt, pt, pad - pt)), w.double(), None, stride, 0, 1, C)
    want = F.silu(z * a1.double().view(1, -1, 1, 1) + b1.double().view(1, -1, 1, 1))
    assert rel(y, want) <= 2e-6
    assert float((pooled.double() - want.mean((2, 3))).abs().max()) <= 1e-5 * float(want.abs().max())
    y2, pooled2 = torch.empty_like(y), torch.empty_like(pooled)
    _lib.check(L.srbh_dwconv_eval_fwd(*args, y2.data_ptr(), pooled2.data_ptr(), B, C, H, H, K, stride, pt, pt, OH, OH, _lib.stream_ptr()), "dwconv_eval_fwd")
    assert torch.equal(y, y2) and torch.equal(pooled, pooled2)


# (the second row: products wide enough for the LDS-tiled forms of csrc/srbh_pwgemm_lds_kernel.h -- 32x128, 64x128, 64x64 incl. K = 56 (not a
#  multiple of the 16-wide K block), a ragged last column tile and 2x2 planes (M = 2688) -- and wide products with few tiles and a deep K, which
#  stay on pw_gemm_kernel's split-K form)
@pytest.mark.parametrize("B,Cin,Cout,HW", [(3, 144, 24, 1024), (2, 240, 40, 256), (5, 672, 112, 16), (7, 2688, 448, 4), (128, 960, 160, 16), (1, 24, 24, 64),
                                           (67, 144, 32, 256), (256, 24, 144, 1024), (255, 160, 960, 16), (130, 56, 336, 64), (256, 1632, 272, 4),
                                           (250, 672, 112, 16), (256, 448, 2688, 4)])
@pytest.mark.parametrize("transposed", [0, 1])
def test_pointwise_conv_with_gate_bn_and_skip_epilogue(B, Cin, Cout, HW, transposed):
    """srbh_pwconv_fwd_epi (round 4): the squeeze-excite gate multiplied into the operand, folded BatchNorm and the skip connection in the
    epilogue == the separate passes; every tile form (16x16 with split K, 16x32, 32x32) through these shapes; each optional part absent."""
    from srbh_amd import _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(Cin + HW)
    x = torch.randn((B, Cin, HW), generator=g).to(DEV)
    w = (torch.randn((Cout, Cin), generator=g) / Cin ** 0.5).to(DEV)
    gate = torch.rand((B, Cin), generator=g).to(DEV)
    sc, sh = (torch.rand(Cout, generator=g) + 0.5).to(DEV), torch.randn(Cout, generator=g).to(DEV)
    res = torch.randn((B, Cout, HW), generator=g).to(DEV)
    wp = w.t().contiguous() if transposed else w
    for use_gate, use_bn, use_res, act in ((1, 1, 1, 0), (1, 1, 0, 0), (0, 1, 0, 1), (0, 0, 0, 0), (1, 0, 1, 2)):
        y = torch.empty((B, Cout, HW), device=DEV)
        _lib.check(L.srbh_pwconv_fwd_epi(x.data_ptr(), wp.data_ptr(), transposed, y.data_ptr(), B, Cin, Cout, HW, gate.data_ptr() if use_gate else None,
                                         sc.data_ptr() if use_bn else None, sh.data_ptr() if use_bn else None, res.data_ptr() if use_res else None,
                                         act, _lib.stream_ptr()), "pwconv_fwd_epi")
        want = torch.einsum("oc,bcp->bop", w.double(), (x * gate.unsqueeze(2)).double() if use_gate else x.double())
        if use_bn:
            want = want * sc.double().view(1, -1, 1) + sh.double().view(1, -1, 1)
        want = F.silu(want) if act == 1 else (F.relu(want) if act == 2 else want)
        if use_res:
            want = want + res.double()
        assert rel(y, want) <= 3e-6, (use_gate, use_bn, use_res, act)


def test_fused_inference_mbconv_block_agrees_with_the_separate_launches():
    """encoders.MBCONV_EVAL (round 4): every MBConv block of EfficientNet-B4 in eval mode as expand | fused middle | SE hidden | SE gate |
    gated project with bn2 + skip == the round-3 chain of separate libsrbh launches; batch sizes 1, 5 and 64; the encoder's launch count
    drops accordingly (path taken in every block)."""
    from srbh_amd import encoders, _lib
    torch.manual_seed(11)
    enc = encoders.get_encoder("efficientnet-b4", in_channels=8, depth=5, weights=None).to(DEV)
    enc.train()
    with torch.no_grad():
        for _ in range(2):
            enc(torch.rand((8, 8, 64, 64), device=DEV))          # non-trivial running statistics
    enc.eval()
    calls = {"n": 0}
    real = encoders.MBConvBlock._eval_fused

    def counting(self, x):
        z = real(self, x)
        calls["n"] += z is not None
        return z
    for B in (1, 5, 64):
        x = torch.rand((B, 8, 64, 64), device=DEV)
        with torch.no_grad():
            encoders.MBConvBlock._eval_fused = counting
            try:
                calls["n"] = 0
                a = enc(x)
            finally:
                encoders.MBConvBlock._eval_fused = real
            assert calls["n"] == 32, calls
            encoders.MBCONV_EVAL = False
            try:
                b = enc(x)
            finally:
                encoders.MBCONV_EVAL = True
        assert len(a) == len(b)
        for u, v in zip(a[1:], b[1:]):
            assert rel(u, v) <= 1e-5, (B, tuple(u.shape), rel(u, v))
    # a training-mode block keeps its training kernels
    enc.train()
    with torch.no_grad():
        assert enc._blocks[3]._eval_fused(torch.rand((2, enc._blocks[3].inp, 16, 16), device=DEV)) is None
