"""CPU: the float64 oracle of the pointwise convolutions (tests/pwconv_oracle.py) checked on its own, and the census of the kernel forms
the EfficientNet-B4 encoder selects.

(a) the oracle against float64 F.conv2d and its autograd at ragged shapes, to 1e-12 relative;
(b) the comparison of tests/test_gpu_pwconv_forms.py is not blind: on the Gaussian operands of its cases an oracle-side slip of the kind a
    kernel makes -- the last k dropped, W read transposed, a channel shifted by one, two images swapped, a weight-gradient sum short by one
    image -- leaves the element-wise bound at at least one element, by the printed factor.  One missing term is |a_k b_k| against a bound of
    about K 2^-23 times K mean|a b|: where K^2 approaches 2^23 (the weight gradients with B HW of 16 384 and more) it need not exceed the
    bound; for those shapes the test asserts that, and that the integer operands (compared with torch.equal) do change;
(c) the census: every 1x1 convolution of the encoder with the plane it sees for a 64x64 tile, at B = 32, 64, 128, 256, forward, data
    gradient and weight gradient: the form the plan queries name is one of those the GPU module runs (libsrbh loads without a device)."""
import pytest
import torch
import torch.nn.functional as F

from tests import pwconv_oracle as O
from tests import test_gpu_pwconv_forms as G

U = O.U


def relerr(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("B,Cin,Cout,HW", [(1, 1, 1, 1), (3, 7, 19, 9), (5, 37, 19, 4), (2, 21, 5, 16)])
def test_oracle_matches_float64_conv2d_and_autograd(B, Cin, Cout, HW):
    g = torch.Generator().manual_seed(B + Cin)
    x = torch.randn((B, Cin, HW), generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn((Cout, Cin), generator=g, dtype=torch.float64, requires_grad=True)
    gate, scale, shift = (torch.rand((B, Cin), generator=g, dtype=torch.float64), torch.rand(Cout, generator=g, dtype=torch.float64) + 0.5,
                          torch.randn(Cout, generator=g, dtype=torch.float64))
    res, dy, dres = (torch.randn((B, Cout, HW), generator=g, dtype=torch.float64), torch.randn((B, Cout, HW), generator=g, dtype=torch.float64),
                     torch.randn((B, Cin, HW), generator=g, dtype=torch.float64))

    def conv(t):
        return F.conv2d(t.view(B, Cin, HW, 1), w.view(Cout, Cin, 1, 1)).view(B, Cout, HW)
    y = conv(x)
    assert relerr(O.fwd(x, w)[0], y.detach()) <= 1e-12
    dx, dw = torch.autograd.grad(y, (x, w), dy)
    assert relerr(O.bwd_data(dy, w)[0], dx) <= 1e-12
    assert relerr(O.bwd_data(dy, w, dres)[0], dx + dres) <= 1e-12
    assert relerr(O.bwd_weight(x, dy)[0], dw) <= 1e-12
    for ug, ub, ur, act in G.EPI_COMBOS + ((1, 1, 1, 1), (0, 0, 1, 2)):
        want = conv(x * gate.unsqueeze(2) if ug else x).detach()
        if ub:
            want = want * scale.view(1, -1, 1) + shift.view(1, -1, 1)
        want = F.silu(want) if act == 1 else (F.relu(want) if act == 2 else want)
        if ur:
            want = want + res
        o = O.fwd_epi(x, w, gate if ug else None, scale if ub else None, shift if ub else None, res if ur else None, act)
        assert relerr(o["y"], want) <= 1e-12, (ug, ub, ur, act)
    # the magnitude sums are the same sums over absolute values
    assert relerr(O.fwd(x, w)[1], O.fwd(x.abs(), w.abs())[0]) <= 1e-12 and relerr(O.bwd_weight(x, dy)[1], O.bwd_weight(x.abs(), dy.abs())[0]) <= 1e-12
    assert relerr(O.bwd_data(dy, w, dres)[1], O.bwd_data(dy.abs(), w.abs(), dres.abs())[0]) <= 1e-12


def test_integer_operands_differ_along_every_axis():
    g = torch.Generator().manual_seed(1)
    for shape in ((1, 3, 1), (257, 4), (9, 69, 4)):
        t = O.ints(shape, g)
        assert float(t.abs().max()) <= 8 and torch.equal(t, t.round())
        for ax in range(len(shape)):
            rows = t.movedim(ax, 0).reshape(shape[ax], -1)
            assert torch.unique(rows, dim=0).shape[0] == shape[ax], (shape, ax)


def test_integer_operands_exist_for_every_case():
    """every shape of the GPU module draws its integer operands (the pairwise-different draw ends), all in [-8, 8]"""
    for v in G.GEMM_FORMS.values():
        for shape in v:
            assert all(float(t.abs().max()) <= 8 and torch.equal(t, t.round()) for t in O.gemm_operands(*shape, "int").values())
    for v in G.WGRAD_FORMS.values():
        for shape, _ in v:
            assert all(float(t.abs().max()) <= 8 for t in O.wgrad_operands(*shape, "int").values())


def _factor(mut, ref, bound):
    return float(((mut - ref).abs() / bound.clamp_min(1e-300)).max())


GEMM_SHAPES = [(key, s) for key, v in G.GEMM_FORMS.items() for s in v]


@pytest.mark.parametrize("key,shape", GEMM_SHAPES, ids=["x".join(map(str, s)) for _, s in GEMM_SHAPES])
def test_gemm_comparison_is_not_blind(key, shape):
    """against the WIDEST bound the GPU module applies at this shape (F = kw fold + gate + fmaf + res)"""
    M, K, HW, B = shape
    ops = O.gemm_operands(M, K, HW, B, "randn")
    a, inp = ops["a"].double(), ops["inp"].double()
    ref, S = O.fwd(inp, a)
    bound = (K + key[2] + 3) * U * S
    muts = {"last k dropped": ref - a[:, K - 1].view(1, M, 1) * inp[:, K - 1].unsqueeze(1)}
    if M > 1 and K > 1:
        muts["W read transposed"] = O.fwd(inp, a.t().contiguous().view(M, K))[0]
    if M > 1:
        muts["channel shifted by one"] = ref.roll(1, dims=1)
    if B > 1:
        sw = ref.clone()
        sw[0], sw[B - 1] = ref[B - 1], ref[0]
        muts["two images swapped"] = sw
    for name, mut in muts.items():
        f = _factor(mut, ref, bound)
        print(f"[pwconv oracle] {shape} {name}: {f:.3g} x the bound")
        assert f > 1, (name, f)
    assert K * K * U < 1          # (every K here is far enough below 2^11.5 for ONE missing term to show)


WGRAD_SHAPES = [(key, s, ns) for key, v in G.WGRAD_FORMS.items() for s, ns in v]


@pytest.mark.parametrize("key,shape,nsplit", WGRAD_SHAPES, ids=["x".join(map(str, s)) for _, s, _ in WGRAD_SHAPES])
def test_wgrad_comparison_is_not_blind(key, shape, nsplit):
    Cout, Cin, B, HW = shape
    Kt = B * HW
    ops = O.wgrad_operands(Cout, Cin, B, HW, "randn")
    ref, S = O.bwd_weight(ops["x"], ops["dy"])
    bound = (Kt + key[1] + nsplit) * U * S
    short = O.bwd_weight(ops["x"][:B - 1], ops["dy"][:B - 1])[0] if B > 1 else torch.zeros_like(ref)
    muts = {"sum short by one image": short, "channel shifted by one": ref.roll(1, dims=0)}
    for name, mut in muts.items():
        f = _factor(mut, ref, bound)
        print(f"[pwconv oracle] wgrad {shape} {name}: {f:.3g} x the bound")
        if name == "sum short by one image" and f <= 1:
            # HW terms of B HW are missing: invisible to the bound once HW / (Kt^2 2^-23) falls to the order of 1 / max-over-mean of |a b|
            assert Kt * Kt * U / HW > 1 / 64, (shape, f)
            io = O.wgrad_operands(Cout, Cin, B, HW, "int")
            assert not torch.equal(O.bwd_weight(io["x"][:B - 1], io["dy"][:B - 1])[0], O.bwd_weight(io["x"], io["dy"])[0]), "only the integer case sees it"
            print(f"[pwconv oracle] wgrad {shape}: one image of {B} is below the Gaussian bound; the integer comparison catches it")
            continue
        assert f > 1, (name, f)


def _pointwise_convs():
    """[(Cin, Cout, HW)] of every 1x1 convolution the encoder runs on libsrbh, with the plane it sees for a 64x64 tile"""
    from srbh_amd import encoders
    torch.manual_seed(0)
    enc = encoders.get_encoder("efficientnet-b4", in_channels=8).eval()
    seen, hooks = [], []
    for m in enc.modules():
        if isinstance(m, encoders.SamePadConv2d) and m._pointwise and m is not enc._conv_head:
            hooks.append(m.register_forward_hook(lambda mod, inp, out: seen.append((mod.weight.shape[1], mod.weight.shape[0], inp[0].shape[2] * inp[0].shape[3]))))
    with torch.no_grad():
        enc(torch.rand(1, 8, 64, 64))
    for h in hooks:
        h.remove()
    return seen


def test_production_shapes_select_covered_forms():
    from srbh_amd import _lib
    _lib.build()
    convs = _pointwise_convs()
    assert len(convs) == 62 and {hw for _, _, hw in convs} == {1024, 256, 64, 16, 4}
    gemm, wg = {}, {}
    for B in (32, 64, 128, 256):
        for Cin, Cout, HW in convs:
            gemm.setdefault(G.gemm_plan(Cout, Cin, HW, B), ("fwd", B, Cin, Cout, HW))
            gemm.setdefault(G.gemm_plan(Cin, Cout, HW, B), ("dgrad", B, Cin, Cout, HW))
            vec, kw, ns = G.wgrad_plan(Cout, Cin, B, HW)
            wg.setdefault((vec, kw), (B, Cin, Cout, HW, ns))
    print("[pwconv census] gemm forms:", sorted(gemm), "wgrad forms:", sorted(wg))
    assert set(gemm) <= G.COVERED_GEMM, {k: v for k, v in gemm.items() if k not in G.COVERED_GEMM}
    assert set(wg) <= G.COVERED_WGRAD, {k: v for k, v in wg.items() if k not in G.COVERED_WGRAD}
    assert any(f == 1 for f, _, _ in gemm) and any(f == 0 and kw == 16 for f, _, kw in gemm)      # (production still runs both families)
    G.plan_queries_refuse()
