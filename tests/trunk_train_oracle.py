"""Float64 oracle of the SR trunk's training kernels (the "fast" mode of rrdbnet_autograd.py): the dense block of SR/rrdbnet_arch.py:136-167
forward and backward, the trunk's fp32 streams, and the weight / bias gradients of its five convs -- torch / numpy on the CPU, nothing imported
from the code under test.

Every conv of the kernels reads STORED 16-bit planes, so a dense block is checked layer by layer: `dense_local` takes the stored planes (as
float64 values) and returns, per layer, the float64 value in front of its 16-bit store.  The backward of a dense block is a dense block on
gradients (G = [g5 | g4 | g3 | g2 | g1], transposed + flipped weight slices stacked along K, the LeakyReLU derivative taken from the saved forward
plane), so one routine serves both directions.

Bounds (the project's form, tests/test_gpu_disc_wide.py): an fp32 sum of K products is within K u sum|a||b| of the float64 sum, u = 2^-23; a value
stored in 16 bits adds half an ulp of that format; an fp32 stream adds the bounds of the convs summed into it and one u |x| per update."""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -23
TINY = 2.0 ** -149          # fp32's spacing below 2^-126: what one product or sum can lose to underflow, whatever its size
# conv1..conv5 of a dense block on the gradient side: (first channel of its output gradient in G = [g5 (64) | g4 | g3 | g2 | g1], cout, cin)
CONV_GEO = ((160, 32, 64), (128, 32, 96), (96, 32, 128), (64, 32, 160), (0, 64, 192))
DW_OFF = (0, 9 * 2048, 9 * (2048 + 3072), 9 * (2048 + 3072 + 4096), 9 * (2048 + 3072 + 4096 + 5120))      # conv_k's OIHW weights in an RDB's slice of dw_all
DW_RDB = 9 * (32 * 64 + 32 * 96 + 32 * 128 + 32 * 160 + 64 * 192)      # 239 616 floats per RDB
DB_RDB = 192


# ---- roundings ------------------------------------------------------------------------------------------------------------------------------
def bf16_rne(x):
    """round-to-nearest-even to bf16, by integer arithmetic on the fp32 bits (x must be exact in fp32: fp32 or fp16 values); float64 result"""
    a = np.ascontiguousarray(torch.as_tensor(x).detach().to(torch.float32).numpy())
    u = a.view(np.uint32).astype(np.uint64)
    low, keep = u & 0xFFFF, u >> 16
    up = (low > 0x8000) | ((low == 0x8000) & ((keep & 1) == 1))
    r = ((keep + up.astype(np.uint64)) << 16).astype(np.uint32)
    return torch.from_numpy(r.view(np.float32).astype(np.float64))


def f16_to_bf16(h):
    """what the weight-gradient kernels do to a saved fp16 plane: fp16 -> fp32 (exact) -> bf16 (RNE)"""
    h = torch.as_tensor(h)
    assert h.dtype == torch.float16
    return bf16_rne(h.float())


def half_ulp_bf16(ref):
    """half an ulp of bf16 (8 significant bits) at `ref`: 2^(floor(log2 |ref|) - 8), between 2^-9 |ref| (just under a power of two) and 2^-8 |ref|
    (at one): what round-to-nearest can be off by -- 1 + 2^-8 goes to 1.  Below 2^-126 (bf16 has fp32's exponent range) the spacing stays 2^-133:
    half of it, 2^-134 -- the tail of an impulse's gradient gets there."""
    a = ref.abs()
    _, e = torch.frexp(a)          # a = m 2^e, m in [0.5, 1)
    return torch.where(a < 2.0 ** -126, torch.full_like(a, 2.0 ** -134), torch.ldexp(torch.ones_like(a), e.clamp_min(-125) - 9))


def half_ulp_f16(ref):
    """half an ulp of fp16 at `ref`: 2^-11 |ref| for normal values, 2^-25 in the subnormal range (|ref| < 2^-14)"""
    return torch.where(ref.abs() < 2.0 ** -14, torch.full_like(ref, 2.0 ** -25), 2.0 ** -11 * ref.abs())


# ---- the reference dense block (ground truth of the CPU tests) ------------------------------------------------------------------------------
def rdb_reference(x, W, b):
    """SR/rrdbnet_arch.py:136-167 in float64: five convs over the growing concatenation, LeakyReLU 0.2 on the first four, 0.2 conv5 + x.
    W, b: lists of conv1..conv5's weight and bias.  Returns (out, [x1, x2, x3, x4])."""
    feats = [x]
    for k in range(4):
        feats.append(F.leaky_relu(F.conv2d(torch.cat(feats, 1), W[k], b[k], 1, 1), 0.2))
    return F.conv2d(torch.cat(feats, 1), W[4], b[4], 1, 1) * 0.2 + x, feats[1:]


def bwd_weights(W):
    """the five gradient convs of a dense block from conv1..conv5's weights: the gradient of plane X_m (dense channels lo:hi) is one conv over
    the first channels of G = [g5 | g4 | g3 | g2 | g1] with the transposed and flipped slices [lo:hi] of every conv that read X_m, stacked along
    the input channels in G's order (conv5 first).  Order: dX4, dX3, dX2, dX1, dx -- the shapes of conv1..conv5."""
    out = []
    for lo, hi, users in ((160, 192, (4,)), (128, 160, (4, 3)), (96, 128, (4, 3, 2)), (64, 96, (4, 3, 2, 1)), (0, 64, (4, 3, 2, 1, 0))):
        out.append(torch.cat([W[k][:, lo:hi].permute(1, 0, 2, 3).flip(2, 3) for k in users], dim=1))
    return out


# ---- one dense block as the kernels run it ----------------------------------------------------------------------------------------------------
def dense_local(planes, weights, bias, mask, stream_in):
    """planes (B, 192, H, W) float64: the stored planes [p0 (64) | p1 | p2 | p3 | p4]; weights: the five convs (cout, 64 + 32 k, 3, 3) as the pack
    rounds them; bias: five vectors, or None (backward); mask: None = forward (LeakyReLU 0.2 behind bias), else (B, 128, H, W): the saved
    forward planes whose signs scale p1..p4 (backward: [X4 | X3 | X2 | X1]; value * (saved > 0 ? 1 : 0.2)); stream_in (B, 64, H, W).
    Returns (inner, stream): inner[k] = (value of p_{k+1} in front of its 16-bit store, sum|a||b|), stream = (0.2 conv5(planes) + stream_in, scale)."""
    inner = []
    for k in range(4):
        cin = 64 + 32 * k
        x, w = planes[:, :cin], weights[k]
        v = F.conv2d(x, w, None if bias is None else bias[k], 1, 1)
        s = F.conv2d(x.abs(), w.abs(), None if bias is None else bias[k].abs(), 1, 1)
        if mask is None:
            v = F.leaky_relu(v, 0.2)            # (1-Lipschitz: the pre-activation's scale bounds it)
        else:
            f = torch.full_like(v, 0.2).masked_fill_(mask[:, 32 * k:32 * k + 32] > 0, 1.0)      # (full_like: 0.2 in v's own precision)
            v, s = v * f, s * f
        inner.append((v, s))
    c5 = F.conv2d(planes, weights[4], None if bias is None else bias[4], 1, 1)
    s5 = F.conv2d(planes.abs(), weights[4].abs(), None if bias is None else bias[4].abs(), 1, 1)
    return inner, (0.2 * c5 + stream_in, 0.2 * s5 + stream_in.abs())


def inner_bound(k, scale, ref, half_ulp):
    """bound of inner plane k (0..3) against its stored value: 9 cin products + the bias, one rounding of the activation, and the 16-bit store
    of an fp32 value that far from `ref` (half an ulp there: the fp32 value may sit in the next binade)"""
    fp32 = (9 * (64 + 32 * k) + 1) * (U * scale + TINY) + U * ref.abs()
    return fp32 + half_ulp(ref.abs() + fp32)


def trunk_streams(rows, weights, bias, x0, masks=None, generate=None):
    """the fp32 streams of a row of dense blocks in float64, by the kernels' recurrences: per RDB x' = 0.2 conv5(stored planes) + x, behind every
    third RDB x = 0.2 x' + x_rrdb (x_rrdb: the stream that entered the RRDB).  rows[i]: RDB i's stored planes (running order); weights[i], bias[i]
    (or None), masks[i] as dense_local takes them.  x0 (B, 64, H, W): the stream entering RDB 0.  generate: None = rows are given; a function =
    rows are BUILT on the way, each plane stored through it (identity: the unrounded chain of the CPU tests).
    Returns per RDB a dict: inner (dense_local's), stream (behind the RDB, RRDB close included), bound (of the fp32 stream against it), rows[i]."""
    x, err = x0, torch.zeros_like(x0)
    x_rrdb, err_rrdb = x, err
    out = []
    for i in range(len(weights)):
        b = None if bias is None else bias[i]
        m = None if masks is None else masks[i]
        if generate is None:
            planes = rows[i]
            inner, (xn, sc) = dense_local(planes, weights[i], b, m, x)
        else:
            planes = torch.zeros(x.shape[0], 192, *x.shape[2:], dtype=x.dtype)
            planes[:, :64] = generate(x)
            for k in range(4):
                planes[:, 64 + 32 * k:96 + 32 * k] = generate(dense_local(planes, weights[i], b, m, x)[0][k][0])
            inner, (xn, sc) = dense_local(planes, weights[i], b, m, x)
        # x' = 0.2 (sum of 9 * 192 products + bias) + x: the conv's bound scaled, one rounding of the product and one of the sum
        err = err + (9 * 192 + 2) * (U * (sc - x.abs()) + TINY) + U * xn.abs()          # (sc - |x| = 0.2 sum|a||b| of conv5)
        x = xn
        if i % 3 == 2:
            x = 0.2 * x + x_rrdb
            err = 0.2 * err + err_rrdb + U * (0.2 * xn.abs() + x_rrdb.abs())
            x_rrdb, err_rrdb = x, err
        out.append({"inner": inner, "stream": x, "bound": err, "planes": planes})
    return out


# ---- weight and bias gradients ------------------------------------------------------------------------------------------------------------------
def wgrad(D_planes, G_planes, with_scale=False):
    """D_planes (B, 192, H, W): the saved planes [x (64) | x1 | x2 | x3 | x4] ALREADY rounded to bf16 (f16_to_bf16), G_planes (B, 192, H, W): the
    gradient planes [g5 (64) | g4 | g3 | g2 | g1]; float64.  dW[co][ci][ky][kx] = sum g[y][x][co] * D[y + ky - 1][x + kx - 1][ci] (zero outside the
    image), db = sum g.  Returns (dw, db) in the layout of one RDB's slice of dw_all (conv1..conv5, OIHW) and db_all (G's channel order);
    with_scale: also the same sums over absolute values."""
    B, _, H, W = D_planes.shape
    Dp = F.pad(D_planes, (1, 1, 1, 1))
    res = []
    for x, g in ((Dp, G_planes),) + (((Dp.abs(), G_planes.abs()),) if with_scale else ()):
        # per tap the shifted planes as (192, pixels) and the gradients as (192, pixels): every block is one matrix product over the pixels
        taps = [x[:, :, ky:ky + H, kx:kx + W].permute(1, 0, 2, 3).reshape(192, -1) for ky in range(3) for kx in range(3)]
        g2 = g.permute(1, 0, 2, 3).reshape(192, -1)
        dw = torch.zeros(DW_RDB, dtype=torch.float64)
        for k, (ch0, cout, cin) in enumerate(CONV_GEO):
            blk = torch.stack([g2[ch0:ch0 + cout] @ t[:cin].T for t in taps], -1)          # (cout, cin, 9): OIHW with the taps as ky * 3 + kx
            dw[DW_OFF[k]:DW_OFF[k] + cout * cin * 9] = blk.reshape(-1)
        res += [dw, g2.sum(1)]
    return tuple(res)


# ---- comparison -----------------------------------------------------------------------------------------------------------------------------------
def ratio(got, want, bound):
    """largest |got - want| / bound over all elements (inf where a non-finite value or an error at a zero bound sits)"""
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    err = (got - want).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return float(r.max())


def check_bound(name, got, want, bound):
    r = ratio(got, want, bound)
    print(f"[trunk_train] {name}: largest err / bound {r:.3e}")
    assert r <= 1.0, (name, r)
    return r
