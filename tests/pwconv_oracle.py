"""float64 oracle of the pointwise (1x1) convolutions of include/srbh.h -- srbh_pwconv_fwd / _fwd_wt / _fwd_epi / _bwd_data / _bwd_data_res /
_bwd_weight -- written from the header's definitions on the CPU, with the magnitude sum an element-wise fp32 bound needs beside every
result, and the operands the form tests (tests/test_gpu_pwconv_forms.py) and the oracle's own self-checks (tests/test_pwconv_oracle_cpu.py)
share.

  forward   y[b][co][p]  = sum_ci w[co][ci] x[b][ci][p]
  epilogue  y = act((sum_ci w[co][ci] (x[b][ci][p] gate[b][ci])) scale[co] + shift[co]) + res[b][co][p]      (every part optional)
  dgrad     dx[b][ci][p] = sum_co w[co][ci] dy[b][co][p]  (+ res[b][ci][p])
  wgrad     dw[co][ci]   = sum_{b, p} dy[b][co][p] x[b][ci][p]

The bound of an fp32 accumulation of K products with F further roundings on its path is (K + F) 2^-23 S with S = sum_k |a_k| |b_k| (the
project's convention: twice the worst case of a sum rounded to nearest in any order, which also covers whatever a matrix instruction does
inside its own reduction)."""
import torch

U = 2.0 ** -23
SILU_LIPSCHITZ = 1.1            # max |d silu / dv| = 1.0998...
SILU_FLOOR = 2.0 ** -121        # where exp(-v) overflows fp32 (v < -88.73) an fp32 SiLU is -0; the true value is below 88.73 / FLT_MAX < 2^-121


def _d(t):
    return None if t is None else t.detach().double().cpu()


def silu(v):
    return v * torch.sigmoid(v)


def _channel_mix(a, t):
    """out[b][m][p] = sum_k a[m][k] t[b][k][p] as ONE float64 matrix product"""
    B, K, HW = t.shape
    return (a @ t.permute(1, 0, 2).reshape(K, B * HW)).view(a.shape[0], B, HW).permute(1, 0, 2).contiguous()


def fwd(x, w, gate=None):
    """x [B][Cin][HW], w [Cout][Cin] (, gate [B][Cin] multiplied into x) -> (y [B][Cout][HW], S): the forward and its magnitude sum"""
    x, w, gate = _d(x), _d(w), _d(gate)
    xg = x if gate is None else x * gate.unsqueeze(2)
    return _channel_mix(w, xg), _channel_mix(w.abs(), xg.abs())


def fwd_epi(x, w, gate=None, scale=None, shift=None, res=None, act=0, product=None):
    """-> dict(y, pre, S, Spre, post): `pre` the value the activation sees, `post` the activation's result (y without res), S the magnitude
    sum of the gated product, Spre = |scale| S + |shift| the one of `pre`.  product: fwd(x, w, gate) if the caller has it already"""
    scale, shift, res = _d(scale), _d(shift), _d(res)
    assert (scale is None) == (shift is None) and act in (0, 1, 2)
    acc, S = fwd(x, w, gate) if product is None else product
    pre, Spre = acc, S
    if scale is not None:
        pre = acc * scale.view(1, -1, 1) + shift.view(1, -1, 1)
        Spre = S * scale.abs().view(1, -1, 1) + shift.abs().view(1, -1, 1)
    post = silu(pre) if act == 1 else (pre.clamp_min(0.0) if act == 2 else pre)
    y = post if res is None else post + res
    return {"y": y, "pre": pre, "S": S, "Spre": Spre, "post": post}


def bwd_data(dy, w, res=None):
    """dy [B][Cout][HW], w [Cout][Cin] -> (dx [B][Cin][HW], S) with S including |res|"""
    dy, w, res = _d(dy), _d(w), _d(res)
    wt = w.t().contiguous()
    dx, S = _channel_mix(wt, dy), _channel_mix(wt.abs(), dy.abs())
    return (dx, S) if res is None else (dx + res, S + res.abs())


def bwd_weight(x, dy):
    """x [B][Cin][HW], dy [B][Cout][HW] -> (dw [Cout][Cin], S)"""
    x, dy = _d(x), _d(dy)
    B, Cin, HW = x.shape
    xm = x.permute(1, 0, 2).reshape(Cin, B * HW)
    dm = dy.permute(1, 0, 2).reshape(dy.shape[1], B * HW)
    return dm @ xm.t(), dm.abs() @ xm.abs().t()


def epi_bound(o, K, F, res, act, c_silu, exact_pre=False):
    """element-wise bound of srbh_pwconv_fwd_epi from the dict of fwd_epi.  F: the roundings on the way to `pre` beside the K products (K
    fold, gate product, fmaf).  act 0 / 2 (the identity and ReLU are exact and 1-Lipschitz): (K + F + [res]) 2^-23 (Spre + |res|).
    act 1: the error of `pre` through SiLU's Lipschitz constant, plus c 2^-23 |silu| for the kernel's own exp and division (+ the fp32
    underflow floor), plus one rounding of the sum with res.
    exact_pre (integer operands: `pre` is exact, but reaches thousands where the Gaussian cases that c was measured on stay below ~10): no
    term for `pre`, and c grows by |pre|: the fast exp is exp2(-v log2 e), the fp32 rounding of that argument is a relative error
    |v| 2^-24 log2(e) ln(2) = |v| 2^-24 of the exponential, twice that with the rounded constant, and SiLU passes at most all of it on."""
    res = _d(res)
    if act != 1:
        return (K + F + (res is not None)) * U * (o["Spre"] + (0.0 if res is None else res.abs()))
    if exact_pre:
        b = (c_silu + o["pre"].abs()) * U * o["post"].abs() + SILU_FLOOR
    else:
        b = SILU_LIPSCHITZ * (K + F) * U * o["Spre"] + c_silu * U * o["post"].abs() + SILU_FLOOR
    return b if res is None else b + U * (o["post"].abs() + res.abs())


# ---- operands ------------------------------------------------------------------------------------------------------------------------------
def _slices_differ(t):
    """every two slices along every axis differ (an exact float64 hash of each slice: integers up to 8 times weights below 2^20)"""
    for ax in range(t.dim()):
        n, rest = t.shape[ax], t.numel() // max(t.shape[ax], 1)
        if n < 2 or 17.0 ** min(rest, 40) < n * n / 4.0:
            continue          # (one slice; or too few values per slice for n different ones to be likely, e.g. the 256 channels of a 2-image gate)
        m = t.movedim(ax, 0).reshape(t.shape[ax], -1).double()
        assert m.shape[1] * 8 * 2.0 ** 20 < 2.0 ** 53
        r = torch.randint(1, 2 ** 20, (m.shape[1],), generator=torch.Generator().manual_seed(ax + 1)).double()
        if torch.unique(m @ r).numel() != t.shape[ax]:
            return False
    return True


def ints(shape, gen, lim=8):
    """integers in [-lim, lim] such that no two images, channels or pixels (slices along any axis) are equal: an index slip of the kernel
    cannot land on an identical operand.  (An axis whose slices are too short for that -- 17^len < n^2 / 4 -- is left to chance.)"""
    for _ in range(200):
        t = torch.randint(-lim, lim + 1, shape, generator=gen).float()
        if _slices_differ(t):
            return t
    raise AssertionError(f"no draw of shape {shape} with pairwise different slices")


def gemm_operands(M, K, HW, B, kind, seed=0):
    """operands of one forward / data-gradient case: a [M][K] (the forward's w, the transpose of the data gradient's), inp [B][K][HW], and the
    epilogue's gate [B][K], scale / shift [M], res [B][M][HW].  kind "int": integers in [-8, 8]; "randn": Gaussian with a / sqrt(K), gates in
    (0, 1), scales in (0.5, 1.5)"""
    g = torch.Generator().manual_seed(seed + 7919 * M + 104729 * K + 31 * HW + B + (0 if kind == "int" else 1 << 20))
    if kind == "int":
        return {"a": ints((M, K), g), "inp": ints((B, K, HW), g), "gate": ints((B, K), g), "scale": torch.randint(-8, 9, (M,), generator=g).float(),
                "shift": torch.randint(-8, 9, (M,), generator=g).float(), "res": ints((B, M, HW), g)}
    return {"a": torch.randn((M, K), generator=g) / K ** 0.5, "inp": torch.randn((B, K, HW), generator=g), "gate": torch.rand((B, K), generator=g),
            "scale": torch.rand(M, generator=g) + 0.5, "shift": torch.randn(M, generator=g), "res": torch.randn((B, M, HW), generator=g)}


def wgrad_operands(Cout, Cin, B, HW, kind, seed=0):
    g = torch.Generator().manual_seed(seed + 7919 * Cout + 104729 * Cin + 31 * HW + B + (0 if kind == "int" else 1 << 20))
    if kind == "int":
        return {"x": ints((B, Cin, HW), g), "dy": ints((B, Cout, HW), g)}
    return {"x": torch.randn((B, Cin, HW), generator=g), "dy": torch.randn((B, Cout, HW), generator=g) / (B * HW) ** 0.5}
