"""float64 restatement of the head's BatchNorm / residual glue kernels (csrc/srbh_head.hip, csrc/srbh_head_bwd.hip)  --  TEST INFRASTRUCTURE ONLY.

One plain torch function per operation, evaluated in float64 on the CPU whatever the inputs' type, each written from the contract in
include/srbh.h (the BatchNorm statistics and residual entries, the head-backward entries), not from the kernels; plus the dispatch
arithmetic of those entry points restated in Python (which form a call takes, its block size, the groups of the one-block fold, the
trips of a capped grid), so that the case tables of tests/test_gpu_head_glue.py can be held to the properties they were chosen for.
tests/test_head_glue_cpu.py pins this file against float64 autograd; tests/test_gpu_head_glue.py compares the kernels with it.
No device code here.

Layouts as in include/srbh.h: tensors NHWC, flattened to [npix][C]; per-channel vectors [C]; the statistics image [64 slots][2][C]
float64 (moment 0: sum, moment 1: the second sum); the ReLU bit buffer: per 64 consecutive 4-channel groups four 64-bit words, word j
bit l = (element j of group 64 k + l is > 0)."""
from __future__ import annotations

import torch

NSLOT = 64
EPS32 = 2.0 ** -24           # unit roundoff of fp32
BF16_REL = 2.0 ** -8         # unit roundoff of bf16 (8 significant bits): |x - bf16(x)| <= 2^-8 |x| under RNE
GRID_CAP, GRID_CAP_BAR, BLOCK = 2048, 4096, 256     # grid_for / grid4_for; bn_add_relu_impl


def _d(t):
    return t.detach().to("cpu", torch.float64)


def _f32(x):
    """a Python float as the fp32 value the C ABI passes"""
    return float(torch.tensor(x, dtype=torch.float32))


# ---- forward ------------------------------------------------------------------------------------------------------------------------
def fold(stats):
    """the two totals of a [64][2][C] statistics image"""
    st = _d(stats).reshape(NSLOT, 2, -1)
    return st[:, 0].sum(0), st[:, 1].sum(0)


def bn_finalize(stats, count, gamma, beta, eps, momentum, rm, rv):
    """srbh_bn_finalize: training-mode BatchNorm statistics.  Returns a dict: scale, shift, save_mean, save_invstd, running_mean,
    running_var (the new running statistics; None without rm / rv) and, for the bounds, the magnitudes M of shift and of the two
    running statistics (sum of the absolute values of the terms)."""
    s, q = fold(stats)
    C = s.numel()
    eps, momentum = _f32(eps), _f32(momentum)
    g = _d(gamma) if gamma is not None else torch.ones(C, dtype=torch.float64)
    b = _d(beta) if beta is not None else torch.zeros(C, dtype=torch.float64)
    mean = s / count
    var = (q / count - mean * mean).clamp_min(0.0)          # biased, clamped at 0
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = g * invstd
    r = dict(scale=scale, shift=b - mean * scale, save_mean=mean, save_invstd=invstd, running_mean=None, running_var=None,
             M_shift=b.abs() + (mean * scale).abs())
    if rm is not None:
        unbiased = var * count / (count - 1) if count > 1 else var
        r["running_mean"] = (1.0 - momentum) * _d(rm) + momentum * mean
        r["running_var"] = (1.0 - momentum) * _d(rv) + momentum * unbiased
        r["M_running_mean"] = ((1.0 - momentum) * _d(rm)).abs() + (momentum * mean).abs()
        r["M_running_var"] = ((1.0 - momentum) * _d(rv)).abs() + (momentum * unbiased).abs()
    return r


def _pc(v):
    return _d(v).view(1, -1)


def bn_add_relu(a, sa, ha, idt, si, hi):
    """srbh_bn_add_relu: relu(a * sa + ha + (idt * si + hi)), si None = the identity path as it is.  a / idt [npix][C].
    Returns (out, M) with M the sum of the absolute values of the terms."""
    a, idt = _d(a), _d(idt)
    t1, t2 = a * _pc(sa), _pc(ha).expand_as(a)
    if si is None:
        t3, t4 = idt, torch.zeros_like(idt)
    else:
        t3, t4 = idt * _pc(si), _pc(hi).expand_as(a)
    return torch.relu(t1 + t2 + t3 + t4), t1.abs() + t2.abs() + t3.abs() + t4.abs()


def relu_bits(out):
    """the activity pattern of `out` (any shape, a multiple of 4 elements, read as consecutive 4-element groups): int64 words
    [ceil(groups / 64) * 4]; the bits of groups past the end are 0 here (unspecified in the kernel's buffer)"""
    act = (out.detach().cpu().reshape(-1, 4) > 0)
    n4 = act.shape[0]
    K = (n4 + 63) // 64
    pad = torch.zeros((K * 64, 4), dtype=torch.bool)
    pad[:n4] = act
    lane = torch.arange(64, dtype=torch.int64).view(1, 64, 1)
    return (pad.view(K, 64, 4).to(torch.int64) << lane).sum(1).reshape(-1)        # distinct bits: the sum is their OR (bit 63 = the sign)


def unpack_relu_bits(words, n4):
    """int64 words of relu_bits' layout -> bool [n4][4]"""
    w = words.detach().cpu().to(torch.int64).view(-1, 1, 4)
    lane = torch.arange(64, dtype=torch.int64).view(1, 64, 1)
    return (((w >> lane) & 1) != 0).reshape(-1, 4)[:n4]


def relu_mask(g, ref):
    """srbh_relu_mask_mul: g where ref > 0, else 0 -- a select (an inf or NaN of g at a masked position gives 0), in g's own type"""
    g, ref = g.detach().cpu(), ref.detach().cpu()
    return torch.where(ref > 0, g, torch.zeros_like(g))


def nearest2x(src):
    """srbh_nearest2x_f32: src [B][H/2][W/2][C] -> [B][H][W][C], out[y][x] = src[y // 2][x // 2]"""
    return src.detach().cpu().repeat_interleave(2, 1).repeat_interleave(2, 2).contiguous()


def nchw_to_nhwc(src):
    return src.detach().cpu().permute(0, 2, 3, 1).contiguous()


def aggregate(data, step):
    """srbh_aggregate: step x step block sums of v and of [v >= 0], their quotient with fp32(1e-10) added to the count; H // step and
    W // step outputs (the ragged rest is not read).  Returns (out, M) with M = sum |v| / (count + 1e-10)."""
    v = _d(data)
    N, H, W = v.shape
    oh, ow = H // step, W // step
    blk = v[:, :oh * step, :ow * step].reshape(N, oh, step, ow, step)
    cnt = (blk >= 0).to(torch.float64).sum((2, 4)) + _f32(1e-10)
    return blk.sum((2, 4)) / cnt, blk.abs().sum((2, 4)) / cnt


# ---- backward -----------------------------------------------------------------------------------------------------------------------
def mask_margin(c, mask):
    """|c * ms + mh| / (|c * ms| + |mh|) per element, float64: how far the mask decision is from the rounding of its fp32 evaluation"""
    ms, mh = mask
    t = _d(c) * _pc(ms)
    return (t + _pc(mh)).abs() / (t.abs() + _pc(mh).abs()).clamp_min(1e-300)


def _masked_dy(g, c, mask, relu_ref, dz_bf16):
    dy, dz = _d(g), None
    if relu_ref is not None:
        ref = relu_ref.detach().cpu()
        dy = torch.where(ref if ref.dtype == torch.bool else ref > 0, dy, torch.zeros_like(dy))
        dz = dy
        if dz_bf16:
            dz = dy.to(torch.float32).to(torch.bfloat16)           # g is fp32 or bf16: the first step is exact, the second is RNE
            dy = dz.to(torch.float64)
    if mask is not None:
        ms, mh = mask
        keep = c.detach().cpu().float() * ms.detach().cpu().float().view(1, -1) + mh.detach().cpu().float().view(1, -1) > 0   # fp32, as the kernel
        dy = torch.where(keep, dy, torch.zeros_like(dy))
    return dy, dz


def bn_bwd_sums(g, c, mean, invstd, mask=None, relu_ref=None, dz_bf16=False):
    """srbh_bn_bwd_reduce / _relu / _io: dy = g where relu_ref > 0 (relu_ref: the fp32 block output, or a bool tensor for the bit form),
    dz = dy (rounded to bf16 with dz_bf16, and then dy is what dz holds); dy = dy * [c * ms + mh > 0] with mask = (ms, mh);
    xhat = (c - mean) * invstd.  g / c [npix][C]; c None: bias gradient, q = 0.
    Returns (s, q, dz, s_abs, q_abs): s = sum dy, q = sum dy * xhat per channel, dz (None without relu_ref), and the sums of |terms|."""
    dy, dz = _masked_dy(g, c, mask, relu_ref, dz_bf16)
    if c is None:
        t = torch.zeros_like(dy)
    else:
        t = dy * ((_d(c) - _pc(mean)) * _pc(invstd))
    return dy.sum(0), t.sum(0), dz, dy.abs().sum(0), t.abs().sum(0)


def bn_bwd_finalize(s, q, count, gamma, invstd):
    """srbh_bn_bwd_finalize: dgamma = q, dbeta = s, coef = gamma * invstd (gamma None = 1), k1 = s / count, k2 = q / count"""
    g = _d(gamma) if gamma is not None else torch.ones_like(s)
    return dict(dgamma=q, dbeta=s, coef=g * _d(invstd), k1=s / count, k2=q / count)


def bn_bwd_apply(g, c, mean, invstd, mask, coef, k1, k2):
    """srbh_bn_bwd_apply / _io: coef * (dy - k1 - xhat * k2).  Returns (out, M), M = |coef| * (|dy| + |k1| + |xhat * k2|)"""
    dy, _ = _masked_dy(g, c, mask, None, False)
    xk = (_d(c) - _pc(mean)) * _pc(invstd) * _pc(k2)
    return _pc(coef) * (dy - _pc(k1) - xk), _pc(coef).abs() * (dy.abs() + _pc(k1).abs() + xk.abs())


def split_into_slots(rows, generator, keep=()):
    """rows [R][2][C] float64 (one row's contribution to the two sums) spread over the 64 slots of a statistics image: every row goes
    to a slot drawn from a random three quarters of the slots, so that some slots stay empty; the slots of `keep` are among the used
    ones and get one of the first rows each (R > len(keep)).  Returns the image [64][2][C] float64; its totals are the rows' totals
    up to float64 rounding."""
    rows = _d(rows)
    perm = [int(k) for k in torch.randperm(NSLOT, generator=generator)]
    used = torch.tensor(list(keep) + [k for k in perm if k not in keep][: NSLOT * 3 // 4 - len(keep)])
    slot = used[torch.randint(0, used.numel(), (rows.shape[0],), generator=generator)]
    if rows.shape[0] > len(keep):
        slot[: len(keep)] = used[: len(keep)]
    return torch.zeros((NSLOT,) + tuple(rows.shape[1:]), dtype=torch.float64).index_add_(0, slot, rows)


# ---- the dispatch of the entry points, restated (plain arithmetic) --------------------------------------------------------------------
def vec_form(C, aligned=True):
    """the 16-byte kernels (bn_bwd_reduce4 / bn_bwd_apply4): C % 4 == 0, C / 4 divides 256, every pointer aligned"""
    return bool(aligned) and C % 4 == 0 and 256 % (C // 4) == 0


def generic_block(C):
    """threads per block of the scalar reduce: a multiple of C, so that a thread stays on one channel"""
    return 256 if 256 % C == 0 else (256 // C) * C


def fold_groups(C):
    """groups of the one-block fold of the statistics image: group g takes slots g, g + G, ..."""
    return 256 // (2 * C)


def fold_idle(C):
    """threads of the fold's block that belong to no group"""
    return 256 - fold_groups(C) * 2 * C


def fold_group_slots(C, group):
    return list(range(group, NSLOT, fold_groups(C)))


def grid(items, cap=GRID_CAP):
    return min(max((items + 255) // 256, 1), cap)


def trips(items, cap=GRID_CAP, block=BLOCK):
    """the most loop trips a thread of the capped grid takes over `items` work items (the grid is sized for 256-thread blocks; the
    scalar reduce then runs it with generic_block(C) threads)"""
    return -(-items // (grid(items, cap) * block))


def stride(items, cap=GRID_CAP, block=BLOCK):
    return grid(items, cap) * block
