"""float64 statement of the discriminator's wide 3x3 / stride 1 / pad 1 convolutions with LeakyReLU(0.2) (include/srbh.h) -- a
helper of tests/test_disc_wide_cpu.py and tests/test_gpu_disc_wide.py, not a test.

    y  = lrelu(conv(x, w))
    g' = g * (y > 0 ? 1 : 0.2)                                       (torch's leaky_relu backward rule on the saved output, in fp32)
    dx = conv(g', Wt),   Wt[c][o][a][b] = w[o][c][2-a][2-b]
    dw = conv2d_weight(x, g')

The three products round their operands as the kernels do (forward fp16 x fp16, data gradient bf16 x bf16, weight gradient bf16(g') x
bf16(fp16(x))) and then run in float64; each also returns conv(|a|, |b|), the scale of the derived error bound K 2^-23 conv(|a|, |b|)."""
import torch
import torch.nn.functional as F

SLOPE = 0.2
SLOPE32 = float(torch.tensor(SLOPE, dtype=torch.float32))      # the fp32 constant the kernels multiply by

SHAPES = [                      # (B, Cin, Cout, H, W)
    (1, 64, 64, 8, 64),         # one full tile
    (2, 64, 64, 11, 70),        # ragged, crosses both tile edges, two images
    (2, 256, 128, 16, 16),      # two output slices, 8 chunks
    (1, 512, 256, 8, 8),        # conv4's channels: 16 chunks, 4 slices; 512 outputs in the data gradient
    (1, 64, 32, 9, 9),          # the 32-channel output form
    (2, 64, 64, 24, 136),       # 18 tiles; run with the walker cap at 4, so workgroups take 4 or 5 tiles, an uneven walk
]
CAPPED = SHAPES[5]
CAP = 4


def h16(t):
    return t.float().half().double()


def b16(t):
    return t.float().to(torch.bfloat16).double()


def wt(w):
    """(O, C, 3, 3) -> (C, O, 3, 3): transposed and flipped"""
    return w.transpose(0, 1).flip(2, 3).contiguous()


def forward(x, w, rounded=True):
    """y = lrelu(conv(x, w)) and conv(|x|, |w|) in float64; rounded: fp16 operands and the fp32 slope constant"""
    xs, ws = (h16(x), h16(w)) if rounded else (x.double(), w.double())
    z = F.conv2d(xs, ws, padding=1)
    return torch.where(z >= 0, z, z * (SLOPE32 if rounded else SLOPE)), F.conv2d(xs.abs(), ws.abs(), padding=1)


def gprime(g, y):
    """fp32: g * (y > 0 ? 1 : 0.2), the product rounded once in fp32 -- what the masked staging rounds to bf16"""
    g, y = g.float(), y.float()
    return torch.where(y > 0, g, g * SLOPE)


def dgrad(gp, w, rounded=True):
    """dx = conv(g', Wt) and its bound scale; rounded: bf16 operands"""
    gs, ws = (b16(gp), b16(w)) if rounded else (gp.double(), w.double())
    Wt = wt(ws)
    return F.conv2d(gs, Wt, padding=1), F.conv2d(gs.abs(), Wt.abs(), padding=1)


def wgrad(x, gp, rounded=True):
    """dw (O, C, 3, 3) and its bound scale; rounded: bf16(fp16(x)) and bf16(g')"""
    xs, gs = (b16(x.float().half().float()), b16(gp)) if rounded else (x.double(), gp.double())
    shape = (gs.shape[1], xs.shape[1], 3, 3)
    return torch.nn.grad.conv2d_weight(xs, shape, gs, padding=1), torch.nn.grad.conv2d_weight(xs.abs(), shape, gs.abs(), padding=1)
