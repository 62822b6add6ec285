"""CPU: tests/head_glue_oracle.py itself, and the case tables of tests/test_gpu_head_glue.py.

 * the float64 functions the GPU tests compare the head's BatchNorm / residual kernels with, chained as the training step chains the
   kernels, reproduce float64 autograd over F.batch_norm(training=True) -> (+ identity) -> ReLU, and torch's running statistics;
 * the ReLU bit pattern round-trips;
 * the case tables reach every form of the dispatch they were written for (by the arithmetic of the dispatch, restated in the oracle);
 * the inputs of the GPU tests have the properties that keep them from masking anything (no mask decision near its rounding, active
   fractions away from 0 and 1, a g that bf16 does not hold);
 * six kernel mutations, applied to the ORACLE here: each changes a result by more than the bound of the GPU case named beside it.
No kernel is launched here."""
import pytest
import torch
import torch.nn.functional as F

from tests import head_glue_oracle as O
from tests import test_gpu_head_glue as T

EPS_BN = O._f32(1e-5)          # (as fp32 holds it: the C ABI passes eps and momentum as floats)


def _maxrel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _rows(c):
    return torch.stack([c, c * c], 1)


@pytest.mark.parametrize("momentum", [0.1, 0.01])
@pytest.mark.parametrize("npix,C,residual", [(40, 5, True), (33, 16, True), (40, 5, False)])
def test_oracle_chain_equals_float64_autograd(npix, C, residual, momentum):
    """residual: y = relu(BN_train(c) + idt), the block-closing form (ReLU reference = y, then reduce, finalize, apply);
    otherwise y = relu(BN_train(c)), the bn1 form (the mask is BN's own scale and shift).  c.grad, weight.grad, bias.grad, the saved
    statistics and torch's running statistics, all to 1e-12"""
    gen = torch.Generator().manual_seed(npix * C)
    momentum = O._f32(momentum)
    c = (torch.randn((npix, C), generator=gen, dtype=torch.float64) * 1.5 + 0.7).requires_grad_()
    w = (torch.rand(C, generator=gen, dtype=torch.float64) + 0.5).requires_grad_()
    b = (torch.randn(C, generator=gen, dtype=torch.float64) * 0.3).requires_grad_()
    idt = torch.randn((npix, C), generator=gen, dtype=torch.float64)
    G = torch.randn((npix, C), generator=gen, dtype=torch.float64)
    rm, rv = torch.randn(C, generator=gen, dtype=torch.float64), torch.rand(C, generator=gen, dtype=torch.float64) + 0.5
    rm_t, rv_t = rm.clone(), rv.clone()
    z = F.batch_norm(c.t().reshape(1, C, npix, 1), rm_t, rv_t, w, b, True, momentum, EPS_BN).reshape(C, npix).t()
    y = torch.relu(z + idt) if residual else torch.relu(z)
    (y * G).sum().backward()

    image = O.split_into_slots(_rows(c.detach()), gen)
    assert int((image.abs().sum((1, 2)) == 0).sum()) >= O.NSLOT // 4            # some slots stay empty
    f = O.bn_finalize(image, npix, w, b, EPS_BN, momentum, rm, rv)
    assert _maxrel(f["running_mean"], rm_t) <= 1e-12 and _maxrel(f["running_var"], rv_t) <= 1e-12
    assert _maxrel(f["save_mean"], c.detach().mean(0)) <= 1e-12
    assert _maxrel(f["save_invstd"], 1.0 / torch.sqrt(c.detach().var(0, unbiased=False) + EPS_BN)) <= 1e-12
    if residual:
        out, _ = O.bn_add_relu(c, f["scale"], f["shift"], idt, None, None)
        assert _maxrel(out, y.detach()) <= 1e-12
        s, q, dz, _, _ = O.bn_bwd_sums(G, c, f["save_mean"], f["save_invstd"], relu_ref=out.float())
        k = O.bn_bwd_finalize(s, q, npix, w, f["save_invstd"])
        dc, _ = O.bn_bwd_apply(dz, c, f["save_mean"], f["save_invstd"], None, k["coef"], k["k1"], k["k2"])
        # the same through the bit form of the reference
        s2, q2, dz2, _, _ = O.bn_bwd_sums(G, c, f["save_mean"], f["save_invstd"], relu_ref=O.unpack_relu_bits(O.relu_bits(out.float().reshape(-1)), npix * C // 4).reshape(npix, C)
                                          if (npix * C) % 4 == 0 else out > 0)
        assert torch.equal(s, s2) and torch.equal(q, q2) and torch.equal(dz, dz2)
    else:
        mask = (f["scale"], f["shift"])
        assert float(O.mask_margin(c, mask).min()) > 1e-6          # the fp32 mask decision of the oracle is the float64 one
        s, q, _, _, _ = O.bn_bwd_sums(G, c, f["save_mean"], f["save_invstd"], mask=mask)
        k = O.bn_bwd_finalize(s, q, npix, w, f["save_invstd"])
        dc, _ = O.bn_bwd_apply(G, c, f["save_mean"], f["save_invstd"], mask, k["coef"], k["k1"], k["k2"])
    assert _maxrel(dc, c.grad) <= 1e-12
    assert _maxrel(k["dgamma"], w.grad) <= 1e-12 and _maxrel(k["dbeta"], b.grad) <= 1e-12


def test_oracle_finalize_at_count_one_and_without_parameters():
    """count = 1: the variance is 0 and the running variance takes it as it is (torch itself divides 0 by count - 1 = 0 there); the
    running mean is torch's; gamma / beta None = 1 / 0; a negative variance (cancellation) clamps to 0"""
    gen = torch.Generator().manual_seed(5)
    c = torch.randn((1, 6), generator=gen, dtype=torch.float64) * 50
    rm, rv = torch.randn(6, generator=gen, dtype=torch.float64), torch.rand(6, generator=gen, dtype=torch.float64) + 0.5
    m = O._f32(0.1)
    f = O.bn_finalize(O.split_into_slots(_rows(c), gen), 1, None, None, EPS_BN, m, rm, rv)
    rm_t, rv_t = rm.clone(), rv.clone()
    torch.batch_norm(c.t().reshape(1, 6, 1, 1), None, None, rm_t, rv_t, True, m, EPS_BN, False)
    assert _maxrel(f["running_mean"], rm_t) <= 1e-12
    assert torch.equal(f["running_var"], (1.0 - m) * rv)
    assert _maxrel(f["save_invstd"], torch.full((6,), EPS_BN ** -0.5, dtype=torch.float64)) <= 1e-15
    assert torch.equal(f["scale"], f["save_invstd"]) and _maxrel(f["shift"], -c[0] * f["save_invstd"]) <= 1e-15
    image = torch.zeros((O.NSLOT, 2, 1), dtype=torch.float64)
    image[3, 0, 0], image[9, 1, 0] = 10.0, 24.0                 # mean 2.5, second moment 6 < 6.25
    assert float(O.bn_finalize(image, 4, None, None, EPS_BN, m, None, None)["save_invstd"]) == pytest.approx(EPS_BN ** -0.5, rel=1e-15)


@pytest.mark.parametrize("n4", [1, 63, 64, 65, 130])
def test_relu_bits_round_trip(n4):
    out = torch.randn(n4 * 4, generator=torch.Generator().manual_seed(n4))
    out[::5] = 0.0
    out[1::9] = -0.0
    words = O.relu_bits(out)
    assert words.dtype == torch.int64 and words.numel() == (n4 + 63) // 64 * 4
    assert torch.equal(O.unpack_relu_bits(words, n4), out.view(n4, 4) > 0)
    # the layout, bit by bit: word j of block k, bit l <-> element j of group 64 k + l
    for grp in {0, n4 // 2, n4 - 1}:
        for j in range(4):
            assert ((int(words[(grp // 64) * 4 + j]) >> (grp % 64)) & 1) == int(out[grp * 4 + j] > 0)


def test_elementwise_oracles():
    g = torch.tensor([1.0, float("inf"), float("nan"), 2.0, -3.0])
    ref = torch.tensor([0.0, -0.0, -1.0, 1e-30, 5.0])
    assert torch.equal(O.relu_mask(g, ref), torch.tensor([0.0, 0.0, 0.0, 2.0, -3.0]))
    src = torch.arange(2 * 1 * 2 * 4, dtype=torch.float32).view(2, 1, 2, 4)
    assert torch.equal(O.nearest2x(src), F.interpolate(src.permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(0, 2, 3, 1))
    x = torch.randn(2, 3, 5, 7)
    assert torch.equal(O.nchw_to_nhwc(x), x.permute(0, 2, 3, 1).contiguous())
    d = torch.tensor([[[1.0, -2.0, 4.0], [-0.0, 3.0, 9.0], [7.0, 7.0, 7.0]]])
    out, M = O.aggregate(d, 2)                                   # one 2 x 2 block: sum 2, three elements >= 0 (-0.0 is one of them)
    assert out.shape == (1, 1, 1) and float(out) == pytest.approx(2.0 / 3.0, rel=1e-9) and float(M) == pytest.approx(2.0, rel=1e-9)
    out, _ = O.aggregate(-torch.ones(1, 2, 2), 2)
    assert float(out) == pytest.approx(-4.0 / O._f32(1e-10), rel=1e-12)


# ---- the case tables ------------------------------------------------------------------------------------------------------------------
def test_dispatch_predicates():
    assert [O.generic_block(C) for C in (1, 3, 7, 16, 24, 48, 64)] == [256, 255, 252, 256, 240, 240, 256]
    assert [O.vec_form(C) for C in (1, 3, 4, 7, 8, 12, 16, 24, 32, 48, 64)] == [False, False, True, False, True, False, True, False, True, False, True]
    assert not O.vec_form(16, aligned=False)
    assert [O.fold_idle(C) for C in T.FINALIZE_WIDTHS] == [0, 4, 4, 0, 16, 64, 0]
    assert O.fold_groups(1) == 128 > O.NSLOT
    assert O.trips(2048 * 256) == 1 and O.trips(2048 * 256 + 1) == 2 and O.trips(63) == 1 and O.trips(4096 * 256 + 1, O.GRID_CAP_BAR) == 2


def test_case_tables_reach_every_form():
    forms = [T.reduce_form(c) for c in T.REDUCE_SCALAR + T.REDUCE_VECTOR]
    assert all(T.reduce_form(c)[0] == "scalar" for c in T.REDUCE_SCALAR) and all(T.reduce_form(c)[0] == "reduce4" for c in T.REDUCE_VECTOR)
    # all 16 instantiations of bn_bwd_reduce4_kernel<GB, CH, OB, RB>; the 8 with OB = 1 also with a dz_out to write
    assert {f[1:] for f in forms if f[0] == "reduce4"} == {(g, c, o, r) for g in (0, 1) for c in (0, 1) for o in (0, 1) for r in (0, 1)}
    assert {T.reduce_form(c)[1:] for c in T.REDUCE_VECTOR if c.dz and c.ob} == {(g, c, 1, r) for g in (0, 1) for c in (0, 1) for r in (0, 1)}
    assert all(c.ref is not None for c in T.REDUCE_VECTOR if c.dz)
    # ... each of them also with dz_out NULL behind a ReLU reference, and at both pixel counts
    for k in T.COMBOS:
        for ref in ("f32", "bits"):
            assert {(c.dz, c.npix) for c in T.REDUCE_VECTOR if c.C == 16 and (c.gb, c.ch, c.ob) == k and c.ref == ref} == {(d, n) for d in (False, True) for n in (5, 77)}
    assert {c.C for c in T.REDUCE_VECTOR} == {4, 8, 16, 32, 64}
    assert any(c.cmode == "mask" for c in T.REDUCE_VECTOR) and any(c.cmode == "none" for c in T.REDUCE_VECTOR)
    # the scalar reduce with blocks of 256, 255 (C = 3), 252 (C = 7), 240 (C = 24 and 48), and behind the alignment fallback
    blocks = {(c.C, T.reduce_form(c)[1]) for c in T.REDUCE_SCALAR}
    assert blocks == {(1, 256), (3, 255), (7, 252), (24, 240), (48, 240), (16, 256)}
    assert all(c.mis for c in T.REDUCE_SCALAR if c.C == 16) and O.vec_form(16)
    for C in (1, 3, 7, 24, 48, 16):
        assert {c.cmode for c in T.REDUCE_SCALAR if c.C == C} == set(T.CMODES)
    # all 8 instantiations of bn_bwd_apply4_kernel<GB, CH, OB>, mask on and off; the scalar apply and its fallback
    aforms = {T.apply_form(c)[1:] + (c.mask,) for c in T.APPLY_VECTOR}
    assert aforms == {(g, c, o, m) for g in (0, 1) for c in (0, 1) for o in (0, 1) for m in (False, True)}
    assert all(T.apply_form(c)[0] == "scalar" for c in T.APPLY_SCALAR) and {c.C for c in T.APPLY_SCALAR} == {1, 3, 7, 24, 16}
    assert all(c.mis for c in T.APPLY_SCALAR if c.C == 16)
    assert {c.C for c in T.APPLY_VECTOR if not (c.gb or c.ch or c.ob)} == {4, 8, 16, 32, 64}
    # the fold: widths with 0, 4, 16 and 64 idle threads, and C = 1
    assert {O.fold_idle(C) for C in T.FINALIZE_WIDTHS} == {0, 4, 16, 64} and 1 in T.FINALIZE_WIDTHS and set(T.FINALIZE_COUNTS) == {1000, 1}
    # bn_add_relu: C = 12 (the vector index wraps at a non-power-of-two), every io, with and without i_scale and bits
    assert {(C, io, si, bits) for C, n, io, si, bits in T.BAR_CASES if n in (1, 37)} == \
        {(C, io, si, bits) for C in (4, 12, 16, 64) for io in range(4) for si in (False, True) for bits in (False, True)}


def test_every_capped_grid_has_a_second_trip_and_a_tiny_case():
    """per entry point with a capped grid: one case whose threads take a second grid-stride trip (with a ragged rest), one with fewer
    than 64 work items; no second-trip tensor is larger than 17 MB"""
    def two_and_tiny(items_blocks, cap=O.GRID_CAP):
        t = [O.trips(i, cap, b) for i, b in items_blocks]
        assert 2 in t and max(t) == 2, t
        assert any(i < 64 for i, _ in items_blocks)
        assert all(i % (O.grid(i, cap) * b) != 0 for i, b in items_blocks if O.trips(i, cap, b) == 2)
    plain = lambda c: not (c.gb or c.ch or c.ob or c.ref == "bits")      # noqa: E731
    two_and_tiny([T.reduce_items(c) for c in T.REDUCE_SCALAR])                                                       # srbh_bn_bwd_reduce, scalar
    two_and_tiny([T.reduce_items(c) for c in T.REDUCE_VECTOR if plain(c) and c.ref is None])                         # srbh_bn_bwd_reduce, vector
    two_and_tiny([T.reduce_items(c) for c in T.REDUCE_VECTOR if not plain(c)])                                       # srbh_bn_bwd_reduce_io
    assert any(T.reduce_items(c)[0] < 64 for c in T.REDUCE_VECTOR if plain(c) and c.ref == "f32")                    # srbh_bn_bwd_reduce_relu (same kernel, same grid)
    two_and_tiny([(T.apply_items(c), 256) for c in T.APPLY_SCALAR])                                                  # srbh_bn_bwd_apply, scalar
    two_and_tiny([(T.apply_items(c), 256) for c in T.APPLY_VECTOR if not (c.gb or c.ch or c.ob)])                    # srbh_bn_bwd_apply, vector
    two_and_tiny([(T.apply_items(c), 256) for c in T.APPLY_VECTOR if c.gb or c.ch or c.ob])                          # srbh_bn_bwd_apply_io
    two_and_tiny([(n // 4, 256) for n in T.ELTWISE_N])                                                               # srbh_relu_mask_mul, srbh_add_inplace
    for pick in (lambda io, bits: io == 0 and not bits, lambda io, bits: io != 0 and not bits, lambda io, bits: bits):
        two_and_tiny([(n * C // 4, 256) for C, n, io, si, bits in T.BAR_CASES if pick(io, bits)], O.GRID_CAP_BAR)    # srbh_bn_add_relu, _io, _bits
    big = [c.npix * c.C * 4 for c in T.REDUCE_SCALAR + T.REDUCE_VECTOR + T.APPLY_SCALAR + T.APPLY_VECTOR] + [4 * n for n in T.ELTWISE_N] + \
          [n * C * 4 for C, n, *_ in T.BAR_CASES]
    assert max(big) <= 17e6
    # the spikes sit on both sides of every seam
    pos = T.spike_positions(T.BIG, O.stride(T.BIG))
    assert {0, 2048 * 256 - 1, 2048 * 256, T.BIG - 1} <= set(pos) and 60 <= len(pos) <= 70


# ---- input conditions -------------------------------------------------------------------------------------------------------------------
def _input_keys():
    cases = T.REDUCE_SCALAR + T.REDUCE_VECTOR + T.APPLY_SCALAR + T.APPLY_VECTOR
    return sorted({(c.C, c.npix, c.gb, c.ch) for c in cases})


def test_inputs_do_not_mask_anything():
    """no mask decision within 1e-4 of its terms' magnitude (an fp32 evaluation of c * ms + mh in any order and with or without fma
    decides as float64 does); the mask and the ReLU are active on 20-80 % of every case of 64 elements or more; an fp32 g is not
    bf16-representable; the ReLU reference holds +0.0 and -0.0"""
    for key in _input_keys():
        C, npix, gb, ch = key
        x = T.bwd_inputs(*key)
        margin = O.mask_margin(x.c, (x.ms, x.mh))
        assert int((margin < 1e-4).sum()) == 0, key
        assert torch.equal(x.keep, O._d(x.c) * O._d(x.ms).view(1, -1) + O._d(x.mh).view(1, -1) > 0), key
        if npix * C >= 64:
            assert 0.2 <= float(x.keep.float().mean()) <= 0.8, key
            assert 0.2 <= float((x.ref > 0).float().mean()) <= 0.8, key
            assert bool((x.ref.view(torch.int32) == 0).any()) and bool((x.ref.view(torch.int32) == -2 ** 31).any())
        assert x.g.dtype == (torch.bfloat16 if gb else torch.float32) and x.c.dtype == (torch.float16 if ch else torch.float32)
        if not gb and npix * C >= 64:
            assert float((x.g.bfloat16().float() != x.g).float().mean()) > 0.98, key
        assert float(x.c.float().abs().max()) <= 3.0 + 6 * 2.0 and float(x.invstd.min()) >= 0.4       # offsets up to 3, spreads up to 2


# ---- mutations: what a subtly wrong kernel would give, from the oracle ----------------------------------------------------------------------
def test_mutations_exceed_the_bounds():
    """each figure: (error the mutation causes) / (the bound of the named GPU case), largest over channels or elements; printed"""
    worst = lambda err, M, bound: float((err / (bound * M).clamp_min(1e-300)).max())      # noqa: E731
    # 1. xhat without invstd -- reduce R(16, 77) (q) and apply A(16, 77)
    case = T.R(16, 77)
    x = T.bwd_inputs(16, 77)
    s, q, _, s_abs, q_abs = T.reduce_want(case)
    q_mut = (O._d(x.g) * (O._d(x.c) - O._d(x.mean).view(1, -1))).sum(0)
    m1 = worst((q_mut - q).abs(), q_abs, T.SUM_BOUND)
    want, M = T.apply_want(T.A(16, 77))
    mut, _ = O.bn_bwd_apply(x.g, x.c, x.mean, torch.ones(16), None, x.coef, x.k1, x.k2)
    m1a = worst((mut - want).abs(), M, T.K_APPLY * T.EPS)
    # 2. the sums over the unrounded dz in the bf16-output form -- reduce R(16, 77, 0, 0, 1, "f32", dz)
    case = T.R(16, 77, 0, 0, 1, ref="f32", dz=True)
    s, q, _, s_abs, q_abs = T.reduce_want(case)
    s_u, q_u, _, _, _ = O.bn_bwd_sums(x.g, x.c, x.mean, x.invstd, relu_ref=x.ref, dz_bf16=False)
    m2 = max(worst((s_u - s).abs(), s_abs, T.SUM_BOUND), worst((q_u - q).abs(), q_abs, T.SUM_BOUND))
    # 3. the bit word index off by one quad -- test_bn_add_relu (16, 37, 0, True, True): elements whose bit is then wrong (the test is exact)
    v = T.bar_inputs(16, 37, 0)
    out = O.bn_add_relu(v.a, v.sa, v.ha, v.idt, v.si, v.hi)[0].float()
    words = O.relu_bits(out)
    m3 = int((O.unpack_relu_bits(words.view(-1, 4).roll(1, 1).reshape(-1), 148) != (out.view(148, 4) > 0)).sum())
    # 4. the zero fill skipped -- any reduce case (the buffer holds 7.0 in every slot): R(16, 77)
    s, q, _, s_abs, q_abs = T.reduce_want(T.R(16, 77))
    m4 = worst(torch.full_like(s, 7.0 * O.NSLOT), s_abs, T.SUM_BOUND)
    # 5. the second grid-stride trip dropped -- reduce R(7, 73800): the elements past the first trip are missing from the sums
    #    (the spike cases catch the same exactly; apply / bn_add_relu leave guard NaNs in the output)
    case = T.R(7, 73800)
    x7 = T.bwd_inputs(7, 73800)
    first = O.stride(*T.reduce_items(case)[:1], block=T.reduce_items(case)[1])
    s, q, _, s_abs, q_abs = T.reduce_want(case)
    tail = O._d(x7.g).reshape(-1)[first:]
    ch = torch.arange(first, first + tail.numel()) % 7
    m5 = worst(torch.zeros(7, dtype=torch.float64).index_add_(0, ch, tail).abs(), s_abs, T.SUM_BOUND)
    spikes = T.spike_positions(T.reduce_items(case)[0], first)
    m5s = sum(p >= first for p in spikes)
    # 6. fold_stat_slots ignoring its last group -- test_bn_finalize_and_clear at every width (the images put rows into that group's slots)
    m6 = {}
    for C in T.FINALIZE_WIDTHS:
        v = T.finalize_inputs(C, 1000)
        w = O.bn_finalize(v.image, 1000, v.gamma, v.beta, T.BN_EPS, 0.1, v.rm, v.rv)
        cut = v.image.clone()
        assert all(bool(t.image[k].any()) for t in (v, T.bwd_finalize_inputs(C, 1000)) for k in T.fold_keep(C))
        cut[O.fold_group_slots(C, min(O.fold_groups(C), O.NSLOT) - 1)] = 0          # (C = 1: the last group that owns a slot)
        wm = O.bn_finalize(cut, 1000, v.gamma, v.beta, T.BN_EPS, 0.1, v.rm, v.rv)
        m6[C] = worst((wm["save_mean"] - w["save_mean"]).abs(), w["save_mean"].abs(), T.K_FIN * T.EPS)
    print(f"MUTATION xhat without invstd: reduce {m1:.3g}x, apply {m1a:.3g}x; unrounded dz sums {m2:.3g}x; bit quad off by one: {m3} wrong bits; "
          f"zero fill skipped {m4:.3g}x; second trip dropped {m5:.3g}x and {m5s} spikes lost; fold without its last group {m6}")
    assert m1 > 10 and m1a > 10 and m2 > 1 and m3 > 0 and m4 > 10 and m5 > 1 and m5s >= 2 and min(m6.values()) > 10
