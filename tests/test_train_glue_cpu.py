"""CPU: tests/train_glue_oracle.py itself, and the case tables of tests/test_gpu_train_glue.py.

 * the float64 functions the GPU tests compare the loss / metric / Adam / SR-glue kernels with reproduce independent float64 torch:
   F.cross_entropy and autograd over the scalar g3 . sums, torch.optim.Adam over 3 steps with weight decay, F.leaky_relu and
   F.interpolate(mode="nearest") autograd, F.conv2d, and oracle/loss_oracle.py for the losses and metrics built from the sums;
 * by the arithmetic of the dispatch, restated as constants in the oracle, the case tables reach every form they claim: the second
   grid-stride trip of every capped grid, the flush of wmse_sum's fp32 partial, the scalar / vector / vector-with-tail Adam paths at every
   chunk edge, both conv_first kernels, the LDS opt-in, a ragged last pixel group at every residue, more than one block;
 * the Adam inputs keep the derived bound below 64 eps M, and the inputs hold what 16-bit formats do not.
No kernel is launched here."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import loss_oracle as LO
from tests import test_gpu_train_glue as T
from tests import train_glue_oracle as O

D = torch.float64


def _close(a, b, tol=1e-12):
    a, b = torch.as_tensor(a, dtype=D), torch.as_tensor(b, dtype=D)
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


# ---- the oracle against independent float64 torch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("C", [2, 7, 16])
def test_cedice_oracle_equals_cross_entropy_and_autograd(C, weighted):
    gen = torch.Generator().manual_seed(C)
    B, HW = 3, 41
    z = (torch.randn((B, C, HW), generator=gen, dtype=D) * 3).requires_grad_()
    y = torch.randint(0, C, (B, HW), generator=gen)
    w = torch.rand((B, HW), generator=gen, dtype=D) + 0.1 if weighted else None
    g3 = torch.randn(3, generator=gen).double()                       # (fp32 values: the kernel reads floats)
    ce = F.cross_entropy(z, y, reduction="none")
    pb, tb = z.softmax(1)[:, 1:].sum(1), (y > 0).double()
    sums = torch.stack([(ce * w).sum() if weighted else ce.sum(), (pb * tb).sum(), pb.sum(), tb.sum()])
    (g3 * sums[:3]).sum().backward()
    got, B4 = O.cedice_sums(z.detach(), y, w)
    assert _close(got, sums.detach()) and bool((B4[:3] >= got[:3].abs()).all()) and float(B4[3]) == 0.0
    dz, Bd = O.cedice_grad(z.detach(), y, w, g3)
    assert _close(dz, z.grad) and bool((Bd >= dz.abs()).all())
    # the losses the Python mirror builds from the sums (reference selfloss.py through oracle/loss_oracle.py)
    lv = torch.tensor(0.3, dtype=D)
    n = B * HW
    dice = 1 - (2.0 * got[1] + 1.0) / (got[2] + got[3] + 1.0)
    want = LO.ce_dice_adapt_weight(z.detach().view(B, C, HW, 1), y.view(B, HW, 1), None if w is None else w.view(B, HW, 1), lv)
    assert _close((got[0] / n + dice) * torch.exp(-lv) + lv, want)


def test_cedice_oracle_edges():
    """a class at -inf, a target 200 below the maximum: finite results and finite bounds; an out-of-range label: NaN in sum 0 only, no
    one-hot class in the gradient"""
    z = torch.randn((1, 7, 64), generator=torch.Generator().manual_seed(1))
    y = torch.randint(0, 7, (1, 64), generator=torch.Generator().manual_seed(2))
    zi = z.clone().scatter_(1, ((y + 1) % 7).unsqueeze(1), float("-inf"))
    zt = z.clone().scatter_(1, y.unsqueeze(1), -200.0)
    for zz in (zi, zt):
        s, Bs = O.cedice_sums(zz, y, None)
        dz, Bd = O.cedice_grad(zz, y, None, torch.tensor([1.0, 0.5, -0.25]))
        assert all(bool(t.isfinite().all()) for t in (s, Bs, dz, Bd))
        assert _close(s[0], F.cross_entropy(zz.double(), y, reduction="sum"))
    assert bool((O.cedice_grad(zi, y, None, torch.ones(3))[0][zi == float("-inf")] == 0).all())
    yo = y.clone()
    yo[0, :2] = torch.tensor([-1, 7])
    s, _ = O.cedice_sums(z, yo, None)
    assert bool(s[0].isnan()) and bool(s[1:].isfinite().all()) and float(s[3]) == float((yo > 0).sum())
    dz, _ = O.cedice_grad(z, yo, None, torch.tensor([1.0, 0.0, 0.0]))
    assert _close(dz[0, :, :2], z.double().softmax(1)[0, :, :2]) and _close(dz.sum(1)[0, 2:], torch.zeros(62))


def test_wmse_and_metric_oracles_equal_loss_oracle():
    gen = torch.Generator().manual_seed(5)
    p, t, w = torch.randn(500, generator=gen), torch.randn(500, generator=gen), torch.rand(500, generator=gen)
    lv = torch.tensor(-0.2, dtype=D)
    for wt in (w, None):
        s, Bs = O.wmse_sum(p, t, wt)
        assert _close(s / 500 * torch.exp(-lv) + lv, LO.mse_adapt_weight(p.double(), t.double(), None if wt is None else wt.double(), lv))
        assert Bs == pytest.approx((3 + O.FLUSH) * s)
        pg = p.double().requires_grad_()
        (0.37 * (((pg - t.double()) ** 2) * (1.0 if wt is None else wt.double())).sum()).backward()
        assert _close(O.wmse_grad(p, t, wt, O._f32(0.37))[0], pg.grad * (O._f32(0.37) / 0.37))
    nc = 5
    cls = torch.randint(-1, nc + 1, (500,), generator=gen)
    cls[cls == 3] = 0
    out, _ = O.height_sums(p, t, cls, nc)
    stats, count = LO.height_metric_batch(p.double(), t.double(), cls, nc)
    assert torch.equal(out[:, 3], count.view(-1)) and float(out[3, 3]) == 0
    has = out[:, 3] > 0
    assert _close((out[has, 0] / out[has, 3]).sqrt() * out[has, 3], stats[has, 0]) and _close(out[:, 1:3], stats[:, 1:])
    pred, label = torch.randint(0, nc, (500,), generator=gen), torch.randint(0, nc, (500,), generator=gen)
    cm, bad = O.confusion(pred, label, nc)
    assert bad == 0 and torch.equal(cm, LO.confusion_matrix(pred, label, nc))
    pred[7], label[9] = nc, -1
    cm2, bad = O.confusion(pred, label, nc)
    assert bad == 1 and int(cm2.sum()) == 498


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_adam_oracle_equals_torch_adam(wd):
    gen = torch.Generator().manual_seed(9)
    p0 = torch.randn(300, generator=gen, dtype=D)
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([ref], lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    p, m, v = p0.clone(), torch.zeros(300, dtype=D), torch.zeros(300, dtype=D)
    for t in (1, 2, 3):
        g = torch.randn(300, generator=gen, dtype=D)
        ref.grad = g.clone()
        opt.step()
        p, m, v, bp, bm, bv, M = O.adam(p, g, m, v, 3e-3, wd, 1 / (1 - 0.9 ** t), 1 / math.sqrt(1 - 0.999 ** t), 0.9, 0.999, 1e-8, table_f32=False)
        assert _close(p, ref.detach()) and _close(m, opt.state[ref]["exp_avg"]) and _close(v, opt.state[ref]["exp_avg_sq"])
        assert bool((bp >= p.abs()).all()) and bool((bm >= m.abs()).all()) and bool((bv >= v).all())


@pytest.mark.parametrize("slope", [0.25, 0.0, 0.2])
def test_lrelu_and_up2_oracles_equal_autograd(slope):
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(64, generator=gen, dtype=D)
    x[:3] = torch.tensor([0.0, -0.0, -2.0])
    x.requires_grad_()
    G = torch.randn(64, generator=gen)
    y = F.leaky_relu(x, O._f32(slope))
    (y * G.double()).sum().backward()
    got = O.lrelu_bwd(G, y.detach().float(), slope)
    assert got.dtype == torch.float32 and _close(got, x.grad, 2.0 ** -24)
    if slope in (0.25, 0.0):
        assert torch.equal(got.double(), x.grad)                       # (the product is exact)
    tiny = torch.tensor([2.0 ** -149, -(2.0 ** -149), 0.0, -0.0])
    assert O.lrelu_bwd(torch.ones(4), tiny, 0.5).tolist() == [1.0, 0.5, 0.5, 0.5]
    g = torch.randn((2, 6, 10, 8), generator=gen, dtype=D)               # NHWC
    xin = torch.zeros((2, 8, 3, 5), dtype=D, requires_grad=True)
    (F.interpolate(xin, scale_factor=2, mode="nearest") * g.permute(0, 3, 1, 2)).sum().backward()
    out, Bu = O.up2_bwd(g)
    assert _close(out, xin.grad.permute(0, 2, 3, 1)) and bool((Bu >= 2 * out.abs()).all())


def test_conv_axpby_and_channel_sum_oracles():
    gen = torch.Generator().manual_seed(4)
    x, w, b = torch.randn((2, 5, 4, 7), generator=gen), torch.randn((64, 5, 3, 3), generator=gen), torch.randn(64, generator=gen)
    out, Bc = O.conv_first(x, w, b)
    assert out.shape == (2, 4, 7, 64) and _close(out.permute(0, 3, 1, 2), F.conv2d(x.double(), w.double(), b.double(), padding=1))
    assert bool((Bc >= 45 * out.abs()).all())
    # by hand at a corner: only the 2 x 2 taps inside the image
    want = b[9].double() + (x[1, :, :2, :2].double() * w[9, :, 1:, 1:].double()).sum()
    assert _close(out[1, 0, 0, 9], want) and _close(O.conv_first(x, w, None)[0][1, 0, 0, 9], want - b[9].double())
    xs, ys = torch.randn(1000, generator=gen), torch.randn(1000, generator=gen)
    sep, fused = O.axpby(0.3, xs, -1.7, ys)
    exact = O._f32(0.3) * xs.double() + O._f32(-1.7) * ys.double()
    for t in (sep, fused):
        assert t.dtype == torch.float32 and bool(((t.double() - exact).abs() <= 3 * 2.0 ** -24 * (xs.abs() + 2 * ys.abs()).double()).all())
    assert not torch.equal(sep, fused)                                   # the two forms differ somewhere: the test must allow for both
    one, same = O.axpby(0.3, xs, 0.0, None)
    assert torch.equal(one, same) and torch.equal(one, (O._f32(0.3) * xs.double()).float())
    nf = O.axpby(0.0, torch.tensor([float("inf"), 1.0]), 1.0, torch.tensor([1.0, 1.0]))[0]
    assert bool(nf[0].isnan()) and float(nf[1]) == 1.0
    raw = torch.full((2, 4, 5, 6, 32), 3.0e4, dtype=torch.float16)
    vals = torch.randn((2, 2, 3, 4, 32), generator=gen).half()
    raw[:, 1:3, 1:-1, 1:-1] = vals
    s, mag = O.act16_channel_sum(raw, 1, 2)
    assert _close(s, vals.double().sum((0, 2, 3)).reshape(-1)) and _close(mag, vals.double().abs().sum((0, 2, 3)).reshape(-1))


# ---- the case tables reach the forms they claim ----------------------------------------------------------------------------------------------
def test_constants_and_helpers():
    assert (O.CAP_LOSS, O.CAP_METRIC, O.CAP_ELT4, O.CAP_CSUM, O.BLOCK, O.ADAM_CHUNK, O.FLUSH, O.MAXC) == (2048, 512, 4096, 1024, 256, 4096, 64, 16)
    assert (O.CONV_FIRST_MAX_CIN, O.LDS_DEFAULT) == (56, 65536)
    assert O.trips(1, 2048) == 1 and O.trips(2048 * 256, 2048) == 1 and O.trips(2048 * 256 + 1, 2048) == 2 and O.grid(0, 8) == 1


def test_loss_tables_reach_second_trip_and_flush():
    assert [O.trips(n, O.CAP_LOSS) for n in T.WMSE_N] == [1, 1, 1, 1, 2] and T.WMSE_N == (1, 255, 257, 1000, 2048 * 256 + 70)
    assert all(O.wmse_flushes(n) == 0 for n in T.WMSE_N), "no ordinary case reaches the flush"
    assert O.trips(T.WMSE_FLUSH_N, O.CAP_LOSS) == 66 and O.wmse_flushes(T.WMSE_FLUSH_N) == 1
    assert T.WMSE_FLUSH_N % (2048 * 256) == 70                       # ... and only 70 threads take the 66th trip, the rest flush at 64 of 65
    assert set(T.WMSE_GSCALE) == {1.0, -0.37, 0.0}
    cases = T.CE_CASES
    assert {c.C for c in cases} == {2, 3, 7, 16} and {c.form for c in cases} == set(T.CE_FORMS) and {c.weighted for c in cases} == {True, False}
    for C in (2, 3, 7, 16):
        for form in T.CE_FORMS:
            for wt in (True, False):
                assert {(c.B, c.HW) for c in cases if (c.C, c.form, c.weighted) == (C, form, wt)} >= set(T.CE_SMALL)
    big = [c for c in cases if O.trips(c.B * c.HW, O.CAP_LOSS) > 1]
    assert {c.form for c in big} == set(T.CE_FORMS) and all(c.C == 7 and (c.B, c.HW) == (2, 2048 * 128 + 35) for c in big)
    assert {c.labels for c in cases} == {"all", "zero", "nonzero"} and {c.logits for c in cases} == {"randn", *T.CE_LOGITS}
    assert {c.g3 for c in T.CE_G3_CASES} == {"ce", "dice_pt", "dice_p"} and all(c.g3 == "random" for c in cases)
    assert all(c.labels == "out_of_range" and c.C == 7 for c in T.CE_OOR) and {c.form for c in T.CE_OOR} == set(T.CE_FORMS)
    for form in T.CE_FORMS:                                            # the layouts do not overlap; the padded one has gaps everywhere
        total, bs, cs, ps = T.ce_layout(form, 2, 7, 37)
        idx = torch.zeros(total, dtype=torch.int64)
        idx.as_strided((2, 7, 37), (bs, cs, ps)).add_(1)
        assert int(idx.max()) == 1 and int(idx.sum()) == 2 * 7 * 37
        assert (form != "padded") or (ps == 2 and bs > 7 * 37 and cs > ps * 37 and total > 2 * 2 * 7 * 37)


def test_ce_inputs_hold_what_they_claim():
    for case in T.CE_CASES + T.CE_OOR:
        if case.B * case.HW > 10000:
            continue
        z, y, w, g3 = T.ce_inputs(case)
        if case.labels == "all" and case.B * case.HW >= case.C:
            assert set(y.view(-1).tolist()) >= set(range(case.C))
        if case.labels == "zero":
            assert int(y.abs().sum()) == 0
        if case.labels == "nonzero":
            assert int(y.min()) >= 1
        if case.logits == "target_200_below":
            assert float((z.max(1).values - z.gather(1, y.unsqueeze(1)).squeeze(1)).min()) > 190
        if case.logits == "all_equal":
            assert float(z.max()) == float(z.min())
        if case.logits == "minus_inf":
            assert bool(((z == float("-inf")).sum(1) == 1).all()) and bool(z.gather(1, y.unsqueeze(1)).isfinite().all())
        if case.logits == "pm80":
            assert float(z.max()) > 70 and float(z.min()) < -70
        if case.logits == "randn":
            assert not torch.equal(z.bfloat16().float(), z) and not torch.equal(z.half().float(), z)


def test_metric_tables():
    assert T.METRIC_NC == (1, 3, 7, 16) and [O.trips(n, O.CAP_METRIC) for n in T.METRIC_N] == [1, 1, 1, 2]
    assert {1, 300, 512 * 256 + 70} < set(T.METRIC_N) and O.grid(200, O.CAP_METRIC) == 1 and O.grid(300, O.CAP_METRIC) == 2
    for nc in (3, 7, 16):
        for n in T.METRIC_N[1:]:
            pred, ref, cls = T.height_inputs(nc, n)
            assert {-1, nc} <= set(cls.tolist()) and 1 not in set(cls.tolist())
            on_grid = torch.equal(pred * 64, (pred * 64).round()) and torch.equal(ref * 64, (ref * 64).round())
            assert on_grid == (n <= 300)                               # small cases: sums exact in double in any order
            assert not torch.equal(pred.half().float(), pred) and not torch.equal(pred.bfloat16().float(), pred)
            d = (pred.double() - ref.double())[cls == nc - 1]
            assert d.numel() >= 2 and bool((d.abs() == 0.5).all()) and float(d.sum()) == 0.0
    for nc in T.METRIC_NC:
        p, l = T.confusion_inputs(nc, 300, False)
        assert O.confusion(p, l, nc)[1] == 1 and O.confusion(*T.confusion_inputs(nc, 300, True), nc)[1] == 0


def test_adam_tables_reach_every_path_and_keep_the_bound():
    assert T.ADAM_SIZES == (1, 3, 4, 5, 4095, 4096, 4097, 8192, 12289)
    assert [len(O.adam_chunks([n])) for n in T.ADAM_SIZES] == [1, 1, 1, 1, 1, 1, 2, 2, 4]
    sizes = T.adam_table_sizes()
    assert sizes[T.ADAM_NULL_AT] == 100 and sizes[T.ADAM_EMPTY_AT] == 0 and 0 < T.ADAM_NULL_AT < T.ADAM_EMPTY_AT < len(sizes) - 1
    assert {O.adam_path([0, 0, 0, 0], n) for n in T.ADAM_SIZES} == {"vector", "vector+tail"}
    assert O.adam_path([0, 0, 0, 0], 4096) == "vector" and O.adam_path([0, 0, 0, 0], 4097) == "vector+tail"
    for k in range(4):
        assert O.adam_path([4 * (j == k) for j in range(4)], 4096) == "scalar"
    assert T.ADAM_FORMS == ("aligned", "p", "g", "m", "v")
    assert {h.wd for h in T.ADAM_HP} == {0.0, 1e-4} and {h.t for h in T.ADAM_HP} == {1, 2, 1000, 100000}
    assert {(h.beta1, h.beta2) for h in T.ADAM_HP} == {(0.9, 0.999), (0.0, 0.0)} and len(set(T.ADAM_LR)) == 2
    assert min(T.ADAM_SCALES) == 1e-3 and max(T.ADAM_SCALES) == 1e3
    for hp in T.ADAM_HP:
        for i, (n, (p, g, m, v, lr)) in enumerate(zip(sizes, T.adam_inputs(hp))):
            if n == 0:
                continue
            live = v > 0
            assert bool((v[live] >= 1e-6 * g[live] ** 2).all())
            if n >= 4095:
                assert bool((g[:T.EDGE] == 0).all() and (m[:2 * T.EDGE] == 0).all() and (v[:2 * T.EDGE] == 0).all() and (g[T.EDGE:2 * T.EDGE] != 0).all())
            p1, m1, v1, bp, bm, bv, M = O.adam(p[:n], g[:n], m[:n], v[:n], lr, hp.wd, 1 / (1 - hp.beta1 ** hp.t), 1 / math.sqrt(1 - hp.beta2 ** hp.t),
                                               hp.beta1, hp.beta2, T.ADAM_EPS)
            assert bool((bp <= 64 * M).all()), (hp, n, float((bp / M).max()))
            if n >= 4095 and hp.wd == 0:
                assert torch.equal(p1[:T.EDGE], p[:T.EDGE].double()) and float(bm[:T.EDGE].abs().max()) == 0
    assert all(o % 4 for o, _ in T.WRAP) and T.WRAP_STEPS == 3


def test_glue_tables():
    assert [O.trips(n // 4, O.CAP_AXPBY) for n in T.AXPBY_N] == [1, 1, 2] and [O.trips(n // 4, O.CAP_ELT4) for n in T.LRELU_N] == [1, 1, 2]
    assert all(n % 4 == 0 for n in T.AXPBY_N + T.LRELU_N)
    assert [O.trips(B * Ho * Wo * C // 4, O.CAP_ELT4) for B, Ho, Wo, C in T.UP2_CASES] == [1, 1, 1, 1, 2]
    assert {sh for _, _, sh in T.CSUM_CASES} == set(T.CSUM_SHAPES) | {T.CSUM_BIG} and {pl for _, pl, _ in T.CSUM_CASES} == set(T.CSUM_PLANES)
    B, H, W = T.CSUM_BIG
    assert B * H * W > 1024 * 256 and O.grid(B * H * W, O.CAP_CSUM) == 1024 and O.act16_sum_roundings(B, H, W) == 5 + 8 + 1024
    assert {bf for bf, _, sh in T.CSUM_CASES if sh == T.CSUM_BIG} == {0, 1}
    assert T.HALO > 1000 and float(torch.tensor(T.HALO).half()) == T.HALO


def test_conv_first_table():
    cases = T.CF_CASES
    assert {c.cin for c in cases} == set(T.CF_CIN) == {1, 3, 4, 12, 48, 56}
    assert {O.conv_first_form(c)[0] for c in T.CF_CIN} == {"cin3", "runtime"} and O.conv_first_form(3)[0] == "cin3"
    assert [O.conv_first_form(c)[2] for c in T.CF_CIN] == [False, False, False, False, True, True]
    assert O.conv_first_form(28)[2] is False and O.conv_first_form(29)[2] is True and O.conv_first_form(57) is None
    assert {(1, 1), (2, 3), (5, 4), (3, 5), (4, 9)} <= set(T.CF_HW) and {O.conv_first_ragged(W) for _, W in T.CF_HW} == {0, 1, 2, 3}
    for cin in T.CF_CIN:
        mine = [c for c in cases if c.cin == cin]
        assert {c.B for c in mine} == {1, 3} and {c.bias for c in mine} == {True, False} and {c.outs for c in mine} == set(T.CF_OUTS)
        assert {(c.H, c.W) for c in mine} == set(T.CF_HW)
    for outs in T.CF_OUTS:
        mine = [c for c in cases if c.outs == outs]
        assert {c.B for c in mine} == {1, 3} and {c.bias for c in mine} == {True, False} and {c.cin for c in mine} == set(T.CF_CIN)
    assert max(c.B * c.H * ((c.W + 3) // 4) * 16 for c in cases) > O.BLOCK             # more than one block
