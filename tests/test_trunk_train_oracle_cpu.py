"""The float64 oracle of the SR trunk's training kernels (tests/trunk_train_oracle.py) against float64 autograd of the reference dense block
(SR/rrdbnet_arch.py:136-167), so that it is no restatement of the kernels' reading of the layouts: fed with UNROUNDED planes, its forward planes,
input gradient, every weight gradient and every bias gradient agree with autograd to 1e-12 relative, for one RDB and for two RRDBs with the
RRDB-level skip; its roundings agree with torch.bfloat16 at the tie cases; and its comparison helpers reject three planted mistakes (a tap shifted
by one column, a weight slice from the neighbouring plane, a bias sum without the last tile) by the printed factors."""
import pytest
import torch

from tests import trunk_train_oracle as T

TOL = 1e-12


def _rand(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.rand(*shape, generator=g, dtype=torch.float64) * (hi - lo) + lo


def _params(n_rdb, seed):
    W = [[_rand((co, ci, 3, 3), seed + 10 * i + k, -0.05, 0.05).requires_grad_() for k, (_, co, ci) in enumerate(T.CONV_GEO)] for i in range(n_rdb)]
    b = [[_rand((co,), seed + 500 + 10 * i + k, -0.1, 0.1).requires_grad_() for k, (_, co, _) in enumerate(T.CONV_GEO)] for i in range(n_rdb)]
    return W, b


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _trunk_autograd(x, W, b):
    """RDBs in groups of three with the RRDB-level skip (SR/rrdbnet_arch.py:170-187), or a single RDB"""
    saved, cur = [], x
    if len(W) == 1:
        cur, xs = T.rdb_reference(cur, W[0], b[0])
        return cur, [xs]
    for r0 in range(0, len(W), 3):
        inp = cur
        for i in range(r0, r0 + 3):
            cur, xs = T.rdb_reference(cur, W[i], b[i])
            saved.append(xs)
        cur = cur * 0.2 + inp
    return cur, saved


@pytest.mark.parametrize("n_rdb", [1, 6])
def test_oracle_agrees_with_float64_autograd(n_rdb):
    """B = 1, 8 x 64.  Forward: trunk_streams builds every plane through dense_local from the input alone.  Backward: the same routine on
    G = [g5 | g4 | g3 | g2 | g1] with bwd_weights' stacked slices and the saved planes as masks, the stream started at 0.04 g (one RDB alone has no
    RRDB in front of it: started at 0.2 g, result times 5); wgrad on the planes both left behind, sliced by CONV_GEO / DW_OFF conv by conv."""
    x = _rand((1, 64, 8, 64), 1).requires_grad_()
    W, b = _params(n_rdb, 100)
    out, saved = _trunk_autograd(x, W, b)
    gout = _rand(tuple(out.shape), 2)
    out.backward(gout)
    with torch.no_grad():
        # ---- forward
        fw = T.trunk_streams(None, W, b, x.detach(), generate=lambda v: v)
        worst = _rel(fw[-1]["stream"], out)
        for i in range(n_rdb):
            for k in range(4):
                worst = max(worst, _rel(fw[i]["inner"][k][0], saved[i][k]))
        print(f"forward planes and output vs autograd, {n_rdb} RDB: {worst:.2e}")
        assert worst <= TOL
        # ---- backward: RDBs in reverse
        Wb = [T.bwd_weights(W[i]) for i in reversed(range(n_rdb))]
        masks = [torch.cat(list(reversed(saved[i])), 1) for i in reversed(range(n_rdb))]
        s0 = 0.2 if n_rdb == 1 else 0.04          # (no RRDB close behind a single RDB)
        bw = T.trunk_streams(None, Wb, None, s0 * gout, masks=masks, generate=lambda v: v)
        gin = bw[-1]["stream"] / s0
        e = _rel(gin, x.grad)
        print(f"input gradient vs autograd, {n_rdb} RDB: {e:.2e}")
        assert e <= TOL
        # ---- weight / bias gradients: G buffer k belongs to RDB n_rdb - 1 - k
        worst = 0.0
        for kbuf in range(n_rdb):
            i = n_rdb - 1 - kbuf
            dw, db = T.wgrad(fw[i]["planes"], bw[kbuf]["planes"])
            assert dw.numel() == T.DW_RDB and db.numel() == T.DB_RDB
            for k, (ch0, cout, cin) in enumerate(T.CONV_GEO):
                ew = _rel(dw[T.DW_OFF[k]:T.DW_OFF[k] + cout * cin * 9].view(cout, cin, 3, 3), W[i][k].grad)
                eb = _rel(db[ch0:ch0 + cout], b[i][k].grad)
                assert ew <= TOL and eb <= TOL, (i, k, ew, eb)
                worst = max(worst, ew, eb)
        print(f"weight and bias gradients vs autograd, {n_rdb} RDB: {worst:.2e}")


def test_geometry_tables_are_the_production_ones():
    """the oracle restates (G channel offset, cout, cin, offset into dw_all); the production tables must be the same numbers"""
    from srbh_amd import rrdbnet_autograd as RA
    assert tuple(RA._CONV_GEO) == T.CONV_GEO and tuple(RA._DW_OFF) == T.DW_OFF and RA._DW_RDB == T.DW_RDB == 239616
    off = 0
    for k, (ch0, cout, cin) in enumerate(T.CONV_GEO):
        assert T.DW_OFF[k] == off and ch0 == (0 if k == 4 else 160 - 32 * k) and cin == 64 + 32 * k
        off += cout * cin * 9
    assert off == T.DW_RDB and sum(c for _, c, _ in T.CONV_GEO) == T.DB_RDB


def test_roundings_at_the_tie_cases():
    """bf16_rne / f16_to_bf16 (integer arithmetic on the bits) against torch.bfloat16: ties go to even, 65504 goes to 65536, the smallest fp16
    subnormal and -0.0 survive; then 4096 random fp16 bit patterns."""
    ties = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 65504.0, 2.0 ** -24, -0.0, 0.0]
    want = [1.0, 1 + 2.0 ** -6, -1.0, -(1 + 2.0 ** -6), 65536.0, 2.0 ** -24, -0.0, 0.0]
    h = torch.tensor(ties, dtype=torch.float16)
    assert torch.equal(h.double(), torch.tensor(ties, dtype=torch.float64))          # (all exact in fp16)
    got = T.f16_to_bf16(h)
    assert torch.equal(got, torch.tensor(want, dtype=torch.float64))
    assert torch.equal(got, h.float().to(torch.bfloat16).double())
    assert bool(torch.signbit(got[6])) and not bool(torch.signbit(got[7]))
    g = torch.Generator()
    g.manual_seed(3)
    bits = torch.randint(0, 1 << 16, (4096,), generator=g).to(torch.int32)
    hh = bits.to(torch.int16).view(torch.float16)
    hh = hh[torch.isfinite(hh)]
    assert torch.equal(T.f16_to_bf16(hh), hh.float().to(torch.bfloat16).double())
    f = _rand((4096,), 4, -3.0, 3.0).float()
    assert torch.equal(T.bf16_rne(f), f.to(torch.bfloat16).double())
    assert float(T.half_ulp_f16(torch.tensor([1.0], dtype=torch.float64))) == 2.0 ** -11
    assert float(T.half_ulp_f16(torch.tensor([2.0 ** -15], dtype=torch.float64))) == 2.0 ** -25
    # half an ulp of bf16: 2^-8 in [1, 2), exactly what the ties above are off by; every rounding of the random values stays inside it
    t64 = torch.tensor([1.0, 1 + 2.0 ** -8, 1.999, 2.0, -3.0, 0.0, 2.0 ** -126, 2.0 ** -127, 3e-40], dtype=torch.float64)
    assert T.half_ulp_bf16(t64).tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -7] + [2.0 ** -134] * 4
    assert float((T.bf16_rne(t64) - t64).abs()[1]) == 2.0 ** -8
    assert bool(((T.bf16_rne(f) - f.double()).abs() <= T.half_ulp_bf16(f.double())).all())
    tiny = (f * 2.0 ** -128).float()          # fp32 subnormals: bf16 keeps a spacing of 2^-133 there
    assert bool(((T.bf16_rne(tiny) - tiny.double()).abs() <= T.half_ulp_bf16(tiny.double())).all()) and bool((T.bf16_rne(tiny) != 0).any())
    assert torch.equal(T.bf16_rne(tiny), tiny.to(torch.bfloat16).double())
    assert bool(((T.bf16_rne(f) - f.double()).abs() > 2.0 ** -9 * f.double().abs()).any())          # (2^-9 |x| is NOT a bound of the rounding)


# ---- the comparison helpers reject planted mistakes ------------------------------------------------------------------------------------------
def _rounded_block(seed):
    """one dense block's stored planes as the GPU tests meet them: fp16 forward planes, bf16 gradient planes, B = 1, 8 x 64"""
    D = _rand((1, 192, 8, 64), seed).half()
    Gp = T.bf16_rne(_rand((1, 192, 8, 64), seed + 1).float())
    return D, Gp


def test_comparison_rejects_a_tap_shifted_by_one_column():
    D, Gp = _rounded_block(20)
    Db = T.f16_to_bf16(D)
    dw, db, sw, sb = T.wgrad(Db, Gp, with_scale=True)
    bound = 8 * 64 * T.U * sw
    assert T.ratio(dw, dw, bound) == 0.0
    wrong, _ = T.wgrad(torch.roll(Db, 1, dims=3), Gp)          # every tap reads the column to its left
    r = T.ratio(wrong, dw, bound)
    print(f"tap shifted by one column: err / bound {r:.3e}")
    assert r > 100.0
    with pytest.raises(AssertionError):
        T.check_bound("shifted tap", wrong, dw, bound)


def test_comparison_rejects_a_weight_slice_from_the_neighbouring_plane():
    D, Gp = _rounded_block(30)
    W = [_rand((co, ci, 3, 3), 40 + k, -0.05, 0.05) for k, (_, co, ci) in enumerate(T.CONV_GEO)]
    Wb = [T.bf16_rne(w.float()) for w in T.bwd_weights(W)]
    mask = D[:, 64:].double().flip(1)
    x_in = Gp[:, :64]
    inner, (stream, ssc) = T.dense_local(Gp, Wb, None, mask, x_in)
    # the gradient of X3 built from conv5's slice of X4 (one plane on): same shapes, other numbers
    lo, hi = 128 + 32, 160 + 32
    wrong_w = list(Wb)
    wrong_w[1] = T.bf16_rne(torch.cat([W[4][:, lo:hi].permute(1, 0, 2, 3).flip(2, 3), W[3][:, 128:160].permute(1, 0, 2, 3).flip(2, 3)], 1).float())
    wrong, _ = T.dense_local(Gp, wrong_w, None, mask, x_in)
    for k in range(4):
        ref, sc = inner[k]
        r = T.ratio(wrong[k][0], ref, T.inner_bound(k, sc, ref, T.half_ulp_bf16))
        print(f"weight slice from the neighbouring plane, plane {k + 1}: err / bound {r:.3e}")
        assert (r > 10.0) if k == 1 else (r == 0.0)


def test_comparison_rejects_a_bias_sum_without_the_last_tile():
    D, Gp = _rounded_block(50)
    _, db, _, sb = T.wgrad(T.f16_to_bf16(D), Gp, with_scale=True)
    bound = 8 * 64 * T.U * sb
    short = Gp.clone()
    short[:, :, 4:] = 0          # the image's second 4-row tile never summed
    _, wrong = T.wgrad(T.f16_to_bf16(D), short)
    r = T.ratio(wrong, db, bound)
    print(f"bias sum without the last tile: err / bound {r:.3e}")
    assert r > 100.0
    assert T.ratio(torch.full_like(db, float("nan")), db, bound) == float("inf")          # a NaN never passes
