"""float64 statement of the discriminator's 4x4 / stride 2 / pad 1 convolution as a 2x2-tap valid convolution over the space-to-depth image of
the zero-padded input (include/srbh.h) -- a helper of tests/test_disc_s2_cpu.py and tests/test_gpu_disc_s2.py, not a test.

    S[(2p+q) C + c][u][v]     = xpad[c][2u+p][2v+q]                  xpad = x in a zero ring of 1
    W2[o][(2p+q) C + c][a][b] = w[o][c][2a+p][2b+q]
    y   = valid 2x2 conv of S with W2
    dS  = valid 2x2 conv of gpad (g in a zero ring of 1) with Wt[k][o][a][b] = W2[o][k][1-a][1-b]
    dx  = d2s(dS)                                                    (the adjoint of s2d)
    dW2 = sum over pixels of g S, un-shuffled to OIHW

The three products round their operands as the kernels do (forward fp16 x fp16, data gradient bf16 x bf16, weight gradient bf16(g) x
bf16(fp16(x))) and then run in float64; each also returns conv(|a|, |b|), the scale of the derived error bound K 2^-23 conv(|a|, |b|)."""
import torch
import torch.nn.functional as F

PHASES = [(p, q) for p in (0, 1) for q in (0, 1)]

SHAPES = [                      # (B, C, O, H, W)
    (2, 32, 64, 16, 16),        # one partial tile
    (1, 32, 64, 18, 132),       # output 9 x 66: crosses both tile edges, ragged
    (2, 64, 128, 8, 8),         # two output slices, 8 input chunks
    (1, 256, 512, 8, 8),        # 32 chunks of K, 8 slices; in the data gradient 1024 output channels
]


def s2d(x):
    """(B, C, H, W), H and W even -> (B, 4C, H/2+1, W/2+1)"""
    xp = F.pad(x, (1, 1, 1, 1))
    return torch.cat([xp[:, :, p::2, q::2] for p, q in PHASES], 1)


def w2(w):
    """(O, C, 4, 4) -> (O, 4C, 2, 2)"""
    return torch.cat([w[:, :, p::2, q::2] for p, q in PHASES], 1)


def wt(w):
    """(O, C, 4, 4) -> (4C, O, 2, 2): W2 transposed and flipped"""
    return w2(w).transpose(0, 1).flip(2, 3).contiguous()


def d2s(ds):
    """(B, 4C, U, V) -> (B, C, 2U-2, 2V-2): the adjoint of s2d (inverse permutation, ring cropped)"""
    B, K, U, V = ds.shape
    C = K // 4
    xp = ds.new_zeros(B, C, 2 * U, 2 * V)
    for k, (p, q) in enumerate(PHASES):
        xp[:, :, p::2, q::2] = ds[:, k * C:(k + 1) * C]
    return xp[:, :, 1:-1, 1:-1].contiguous()


def unshuffle_w(dw2):
    """(O, 4C, 2, 2) -> (O, C, 4, 4): the inverse of w2"""
    O, K = dw2.shape[:2]
    C = K // 4
    dw = dw2.new_zeros(O, C, 4, 4)
    for k, (p, q) in enumerate(PHASES):
        dw[:, :, p::2, q::2] = dw2[:, k * C:(k + 1) * C]
    return dw


def h16(t):
    return t.float().half().double()


def b16(t):
    return t.float().to(torch.bfloat16).double()


def forward(x, w, rounded=True):
    """y and conv(|x|, |w|) in float64; rounded: fp16 operands"""
    xs, ws = (h16(x), h16(w)) if rounded else (x.double(), w.double())
    S, W2 = s2d(xs), w2(ws)
    return F.conv2d(S, W2), F.conv2d(S.abs(), W2.abs())


def dgrad_ds(g, w, rounded=True):
    """dS (B, 4C, Ho+1, Wo+1) and its bound scale; rounded: bf16 operands"""
    gs, ws = (b16(g), b16(w)) if rounded else (g.double(), w.double())
    gp, Wt = F.pad(gs, (1, 1, 1, 1)), wt(ws)
    return F.conv2d(gp, Wt), F.conv2d(gp.abs(), Wt.abs())


def dgrad(g, w, rounded=True):
    ds, scale = dgrad_ds(g, w, rounded)
    return d2s(ds), d2s(scale)


def wgrad(x, g, rounded=True):
    """dw (O, C, 4, 4) and its bound scale; rounded: bf16(fp16(x)) and bf16(g)"""
    xs, gs = (b16(x.float().half().float()), b16(g)) if rounded else (x.double(), g.double())
    S = s2d(xs)
    O, K = gs.shape[1], S.shape[1]
    dw2 = torch.nn.grad.conv2d_weight(S, (O, K, 2, 2), gs)
    sc = torch.nn.grad.conv2d_weight(S.abs(), (O, K, 2, 2), gs.abs())
    return unshuffle_w(dw2), unshuffle_w(sc)
