"""The kernels between the head's convolutions -- BatchNorm statistics and their backward, the residual tail with its ReLU bit pattern,
the ReLU mask, the in-place add, nearest-x2, NCHW -> NHWC and the label aggregate (csrc/srbh_head.hip, csrc/srbh_head_bwd.hip) -- each
entry point on its own through the C ABI against the float64 functions of tests/head_glue_oracle.py, at the smallest shapes at which
each form of their dispatch can still go wrong: the scalar backward reduce with block sizes 256 / 255 / 252 / 240, the alignment
fallbacks, all 16 instantiations of bn_bwd_reduce4_kernel and all 8 of bn_bwd_apply4_kernel, a second grid-stride trip of every capped
grid, the one-block fold of the statistics image at widths that leave 0 / 4 / 16 / 64 threads idle and at C = 1, stale statistics
buffers, the self-cleaning finalize variants, and every refusal.  tests/test_head_glue_cpu.py proves by arithmetic that the case tables
below reach those forms, and that the oracle equals float64 autograd.

Inputs: g is fp32 randn (NOT bf16-representable) unless the case takes a bf16 g; c has per-channel offsets up to 3 and spreads 0.5-2;
mean, invstd, gamma, mask scale / shift, coef, k1, k2 are independent random vectors, not another kernel's output.  Every output lives
in guard-filled storage with slack on both sides, every input is compared with its clone afterwards (tests/gpu_util.GuardedBuffers).

Bounds, from the arithmetic (eps = 2^-24), never from the kernels:
  elementwise fp32 outputs   |got - want| <= k * eps * M per element, M the sum of the absolute values of the expression's terms, k its
                             fp32 roundings: bn_add_relu k = 4; apply k = 8, M = |coef| (|dy| + |k1| + |xhat k2|); aggregate
                             k = step^2 + 2, M = sum|v| / (count + 1e-10); finalize outputs k = 4 (shift: M = |beta| + |mean scale|,
                             running statistics: M = |old| + |new|)
  bf16 outputs               the fp32 bound + 2^-8 |want|; dz_out is bit-equal to the masked g (bf16: to its RNE rounding)
  sums                       read from the statistics image, folded on the host in float64: per channel 2e-5 * sum|term| (a thread's few
                             fp32 terms + at most 256 LDS adds per block ~ 300 eps; double from there on)
  everything else            bit-exact
Each test prints `GLUE <entry point> <case>: <error in units of its bound's M> (stock <the fp32 torch chain on the device>)`.

Measured on an MI355X, error / M, largest over the cases of each entry point (bound; the stock fp32 torch chain on the device beside it):
  srbh_bn_finalize / _clear         1.48e-7  (4 eps = 2.38e-7; the fp32 formula over the fp32 totals: 0.9 -- q/N - mean^2 cancels, which is
                                             why the kernel folds and finishes in double)
  srbh_bn_bwd_finalize / _clear     5.6e-8   (4 eps = 2.38e-7; stock 1.3e-7)
  srbh_bn_add_relu / _io / _bits    1.10e-7 / 1.12e-7 / 1.13e-7   (4 eps = 2.38e-7; stock 1.3e-7 / 1.5e-7 / 1.5e-7); bits exact
  srbh_bn_bwd_apply                 vector 1.74e-7, scalar 1.65e-7   (8 eps = 4.77e-7; stock 2.1e-7 / 1.8e-7)
  srbh_bn_bwd_apply_io              4.75e-7 of 8 eps M + 2^-8 |want| in units of 8 eps (4.77e-7): the bf16 rounding itself, which reaches
                                    its 2^-8 on 2 M elements; stock 4.75e-7
  srbh_bn_bwd_reduce                vector 1.24e-7, scalar 1.22e-7 of sum|term|   (stock 1.29e-7 / 9.4e-8)
  srbh_bn_bwd_reduce_relu / _io     8.0e-8 / 1.40e-7 of sum|term|   (stock 7.4e-8 / 1.33e-7); dz_out bit-equal in every case
  srbh_aggregate                    5.7e-8   (stock 5.3e-8)
  relu_mask_mul, add_inplace, nearest2x, nchw_to_nhwc: bit-exact
Two derived bounds were loose by more than 10x and now stand at 4x the measurement: the sums (2e-5 -> 5.6e-7; the order of a block's
fp32 LDS atomics is not fixed, the figure moved between 1.33e-7 and 1.40e-7 from run to run) and the aggregate (66 eps at step 8 ->
2.3e-7; (step^2 + 2) eps where that is smaller).  No bound was widened."""
import functools
from collections import namedtuple
from types import SimpleNamespace

import pytest
import torch

from tests import head_glue_oracle as O
from tests.gpu_util import GuardedBuffers as Buffers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = O.EPS32
K_BAR, K_APPLY, K_FIN = 4, 8, 4
SUM_DERIVED = 2e-5                  # ~300 eps: a thread's few fp32 terms and at most 256 fp32 LDS adds per block
SUM_BOUND = 5.6e-7                  # 4 x the largest measured (1.40e-7): the derived figure was loose by 143x
AGG_BOUND = 2.3e-7                  # 4 x the largest measured (5.68e-8); the derived (step^2 + 2) eps holds where it is the smaller
assert SUM_BOUND <= SUM_DERIVED
OUT_B16, C_H16, G_B16, REF_BITS, STATS_CLEAN = 1, 2, 4, 8, 16
BIG = 2048 * 256 + 70              # work items of one capped grid (2 048 x 256) and a ragged rest

# ---- case tables (tests/test_head_glue_cpu.py checks what they cover) -----------------------------------------------------------------
# backward reduce: ref None | "f32" | "bits" (the block-closing ReLU), dz: dz_out given, cmode "none" (c NULL) | "c" | "mask",
# mis: g one float past a 16-byte boundary
RCase = namedtuple("RCase", "C npix gb ch ob ref dz cmode mis")


def R(C, npix, gb=0, ch=0, ob=0, ref=None, dz=False, cmode="c", mis=False):
    return RCase(C, npix, gb, ch, ob, ref, dz, cmode, mis)


CMODES = ("none", "c", "mask")
COMBOS = [(gb, ch, ob) for gb in (0, 1) for ch in (0, 1) for ob in (0, 1)]
REFS = [(None, False), ("f32", False), ("f32", True), ("bits", False), ("bits", True)]
REDUCE_SCALAR = ([R(C, n, cmode=m) for C in (1, 3, 7, 24, 48) for n in (1, 50, 1000) for m in CMODES] +
                 [R(7, 73800, cmode=m) for m in CMODES] +
                 [R(16, 50, cmode=m, mis=True) for m in CMODES])
REDUCE_VECTOR = ([R(16, n, *k, ref=ref, dz=dz) for k in COMBOS for ref, dz in REFS for n in (5, 77)] +
                 [R(C, 77, *k, ref=ref, dz=dz) for C in (4, 8, 32, 64) for k in ((0, 0, 0), (1, 1, 1)) for ref, dz in REFS[::2]] +
                 [R(C, 77, cmode="mask") for C in (4, 8, 16, 32, 64)] + [R(16, 77, 1, 1, 0, cmode="mask")] +
                 [R(16, 77, cmode="none"), R(16, 77, gb=1, cmode="none"), R(64, 5, cmode="none")] +
                 [R(4, BIG), R(4, BIG, 1, 1, 1, ref="bits", dz=True)])

# backward apply
ACase = namedtuple("ACase", "C npix gb ch ob mask mis")


def A(C, npix, gb=0, ch=0, ob=0, mask=False, mis=False):
    return ACase(C, npix, gb, ch, ob, mask, mis)


APPLY_SCALAR = ([A(C, n, mask=m) for C in (1, 3, 7, 24) for n in (1, 50, 1000) for m in (False, True)] +
                [A(16, 50, mask=m, mis=True) for m in (False, True)] + [A(1, BIG, mask=True)])
APPLY_VECTOR = ([A(16, n, *k, mask=m) for k in COMBOS for n in (5, 77) for m in (False, True)] +
                [A(C, 77, mask=m) for C in (4, 8, 32, 64) for m in (False, True)] + [A(4, BIG, mask=True), A(4, BIG, 1, 1, 1)])

FINALIZE_WIDTHS = (1, 3, 7, 16, 24, 48, 64)
FINALIZE_COUNTS = (1000, 1)

# residual tail: (C, npix, io, i_scale given, bits)
BAR_BIG = 262144 + 19
BAR_CASES = ([(C, n, io, si, bits) for C in (4, 12, 16, 64) for n in (1, 37) for io in (0, 1, 2, 3) for si in (False, True) for bits in (False, True)] +
             [(16, BAR_BIG, 0, True, False), (16, BAR_BIG, 1, False, False), (16, BAR_BIG, 3, True, True)])
ELTWISE_N = (4, 1020, 4 * (2048 * 256) + 12)


def reduce_form(case):
    """the kernel a reduce case runs: ("scalar", block size) or ("reduce4", GB, CH, OB, RB)"""
    if O.vec_form(case.C, not case.mis):
        return ("reduce4", case.gb, case.ch, case.ob, int(case.ref == "bits"))
    return ("scalar", O.generic_block(case.C))


def reduce_items(case):
    """(work items, block size) of a reduce case's grid"""
    if O.vec_form(case.C, not case.mis):
        return case.npix * (case.C // 4), 256
    return case.npix * case.C, O.generic_block(case.C)


def apply_form(case):
    return ("apply4", case.gb, case.ch, case.ob) if O.vec_form(case.C, not case.mis) else ("scalar", 256)


def apply_items(case):
    return case.npix * (case.C // 4 if O.vec_form(case.C, not case.mis) else case.C)


# ---- inputs (made on the CPU, once per case, never modified) --------------------------------------------------------------------------
def _sign(shape, gen):
    return torch.randint(0, 2, shape, generator=gen).float() * 2 - 1


@functools.lru_cache(maxsize=None)
def bwd_inputs(C, npix, gb=0, ch=0):
    """the tensors and per-channel vectors of one backward case.  The mask's threshold lies inside c's distribution (so that the mask
    is neither all on nor all off); elements whose mask decision is within 1e-3 of its terms' magnitude are moved by 1/16; the
    generator is re-seeded (a fixed sequence) until the active fractions of the mask and of the ReLU are inside 0.2 .. 0.8."""
    for attempt in range(64):
        gen = torch.Generator().manual_seed(1000003 * C + 17 * npix + 5 * (2 * gb + ch) + 7919 * attempt)
        g = torch.randn((npix, C), generator=gen)
        off, spread = (torch.rand(C, generator=gen) * 2 - 1) * 3, 0.5 + 1.5 * torch.rand(C, generator=gen)
        c = torch.randn((npix, C), generator=gen) * spread + off
        x = SimpleNamespace(
            mean=torch.randn(C, generator=gen) * 2, invstd=0.4 + 1.2 * torch.rand(C, generator=gen),
            gamma=(0.5 + torch.rand(C, generator=gen)) * _sign((C,), gen), ms=(0.5 + torch.rand(C, generator=gen)) * _sign((C,), gen),
            coef=torch.randn(C, generator=gen), k1=torch.randn(C, generator=gen) * 0.3, k2=torch.randn(C, generator=gen) * 0.3)
        x.mh = -x.ms * (off + 0.5 * spread * torch.randn(C, generator=gen))
        ref = torch.randn((npix, C), generator=gen)
        ref.view(-1)[::7] = 0.0
        ref.view(-1)[3::11] = -0.0
        x.g = g.to(torch.bfloat16) if gb else g
        c = c.half() if ch else c
        for _ in range(4):
            near = O.mask_margin(c, (x.ms, x.mh)) < 1e-3
            c = torch.where(near, (c.float() + 0.0625).to(c.dtype), c)
        x.c, x.ref = c, ref
        x.keep = c.float() * x.ms.view(1, -1) + x.mh.view(1, -1) > 0
        fm, fr = float(x.keep.float().mean()), float((ref > 0).float().mean())
        if npix * C < 64 or (0.2 <= fm <= 0.8 and 0.2 <= fr <= 0.8):
            break
    # the bit form of the ReLU reference; the bits of the groups past the end are unspecified: all ones here
    n4 = npix * C // 4 if C % 4 == 0 else 0
    if n4:
        pad = torch.ones(((n4 + 63) // 64 * 64 - n4) * 4)
        x.bits = O.relu_bits(torch.cat([ref.reshape(-1), pad]))
    return x


def _case_inputs(case):
    return bwd_inputs(case.C, case.npix, case.gb, case.ch)


@functools.lru_cache(maxsize=None)
def reduce_want(case):
    x = _case_inputs(case)
    ref = None if case.ref is None else (x.ref if case.ref == "f32" else x.ref > 0)
    return O.bn_bwd_sums(x.g, None if case.cmode == "none" else x.c, x.mean, x.invstd, (x.ms, x.mh) if case.cmode == "mask" else None,
                         ref, bool(case.ob and case.dz))


# ---- helpers ----------------------------------------------------------------------------------------------------------------------------
def _p(t):
    return None if t is None else t.data_ptr()


def _ratio(got, want, M):
    """max |got - want| / M; where M == 0 the two must be equal"""
    err = (got.detach().double().cpu() - want).abs()
    M = M.expand_as(err)
    zero = M == 0
    assert bool((err[zero] == 0).all()), "a value whose terms are all zero is not zero"
    return float((err[~zero] / M[~zero]).max()) if bool((~zero).any()) else 0.0


def _bits_equal(a, b):
    it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def _report(entry, case, err, stock, bound):
    print(f"GLUE {entry} {tuple(case)}: {err:.3e} (stock {stock:.3e}; bound {bound:.3e})")


def _lib():
    from srbh_amd import _lib as m
    return m, m.lib()


def _no_error_pending():
    torch.cuda.synchronize()
    assert float(torch.ones(8, device=DEV).sum()) == 8.0


# ---- backward reduce ----------------------------------------------------------------------------------------------------------------------
def _run_reduce(case, stale=7.0, extra_io=0, g_cpu=None, expect_ok=True):
    """one call of srbh_bn_bwd_reduce (no 16-bit tensor, no ReLU), srbh_bn_bwd_reduce_relu (fp32 ReLU reference) or srbh_bn_bwd_reduce_io
    on a statistics buffer that holds `stale`.  Returns (statistics image, dz, device tensors) -- or the return code with expect_ok = False"""
    m, L = _lib()
    x = _case_inputs(case)
    C, npix = case.C, case.npix
    g_cpu = x.g if g_cpu is None else g_cpu
    bufs = Buffers()
    d = SimpleNamespace(mean=None, invstd=None, ms=None, mh=None, c=None, ref=None, dz=None)
    d.g = bufs.inp(g_cpu, 1 if case.mis else 0, dtype=g_cpu.dtype)
    if case.cmode != "none":
        d.c, d.mean, d.invstd = bufs.inp(x.c, dtype=x.c.dtype), bufs.inp(x.mean), bufs.inp(x.invstd)
    if case.cmode == "mask":
        d.ms, d.mh = bufs.inp(x.ms), bufs.inp(x.mh)
    if case.ref == "f32":
        d.ref = bufs.inp(x.ref)
    elif case.ref == "bits":
        assert x.bits.numel() * 8 == L.srbh_relu_bits_bytes(npix, C)
        d.ref = bufs.inp(x.bits, dtype=torch.int64)
    if case.dz:
        d.dz = bufs.out((npix, C), dtype=torch.bfloat16 if case.ob else torch.float32)
    stats = bufs.out((O.NSLOT, 2, C), dtype=torch.float64, fill=torch.full((O.NSLOT, 2, C), stale, dtype=torch.float64))
    assert C > 64 or stats.numel() * 8 == L.srbh_bn_stats_bytes(C)
    io = (G_B16 if case.gb else 0) | (C_H16 if case.ch else 0) | (OUT_B16 if case.ob else 0) | (REF_BITS if case.ref == "bits" else 0) | extra_io
    if io == 0 and case.ref is None:
        rc = L.srbh_bn_bwd_reduce(_p(d.g), _p(d.c), _p(d.mean), _p(d.invstd), _p(d.ms), _p(d.mh), npix, C, _p(stats), m.stream_ptr())
    elif io == 0:
        rc = L.srbh_bn_bwd_reduce_relu(_p(d.g), _p(d.ref), _p(d.dz), _p(d.c), _p(d.mean), _p(d.invstd), npix, C, _p(stats), m.stream_ptr())
    else:
        rc = L.srbh_bn_bwd_reduce_io(_p(d.g), _p(d.ref), _p(d.dz), _p(d.c), _p(d.mean), _p(d.invstd), _p(d.ms), _p(d.mh), npix, C, _p(stats), io,
                                     m.stream_ptr())
    if not expect_ok:
        return rc, bufs, stats
    m.check(rc, "bn_bwd_reduce")
    bufs.verify()
    return stats.cpu(), None if d.dz is None else d.dz.cpu(), d


def _stock_sums(case, d):
    """the stock fp32 chain on the device: mask, product and torch's own column sums"""
    dy = d.g.float()
    if case.ref is not None:
        x = _case_inputs(case)
        dy = torch.where(x.ref.to(DEV) > 0, dy, torch.zeros_like(dy))
        if case.ob and case.dz:
            dy = dy.bfloat16().float()
    if case.cmode == "mask":
        dy = torch.where(d.c.float() * d.ms + d.mh > 0, dy, torch.zeros_like(dy))
    q = (dy * ((d.c.float() - d.mean) * d.invstd)).sum(0) if d.c is not None else torch.zeros_like(dy[0])
    return dy.sum(0), q


def _check_reduce(case, image, dz, d, entry="bn_bwd_reduce"):
    s_w, q_w, dz_w, s_abs, q_abs = reduce_want(case)
    s, q = O.fold(image)
    es, eq = _ratio(s, s_w, s_abs), _ratio(q, q_w, q_abs)
    ss, sq = _stock_sums(case, d)
    _report(entry + "/" + reduce_form(case)[0], case, max(es, eq), max(_ratio(ss, s_w, s_abs), _ratio(sq, q_w, q_abs)), SUM_BOUND)
    if case.cmode == "none":
        assert bool((image[:, 1] == 0).all()), "bias gradient: a q slot is not exactly 0"
    items, block = reduce_items(case)
    blocks = O.grid(items)
    assert bool((image[blocks:] == 0).all()), "a slot no block adds to is not zero (the zero fill)"
    assert es <= SUM_BOUND and eq <= SUM_BOUND
    if case.dz:
        want = dz_w if case.ob else dz_w.float()
        assert _bits_equal(dz, want), "dz_out is not the masked g bit for bit"


@pytest.mark.parametrize("case", REDUCE_SCALAR, ids=lambda c: "-".join(map(str, c)))
def test_bwd_reduce_scalar_kernel(case):
    """bn_bwd_reduce_kernel: block sizes 256 (C = 1; C = 16 behind the alignment fallback), 255 (C = 3), 252 (C = 7, a partial last wave),
    240 (C = 24, 48); one pixel, one block, several blocks, and a second trip of the 252-thread blocks; c NULL, c, c with mask"""
    assert reduce_form(case)[0] == "scalar"
    image, dz, d = _run_reduce(case)
    _check_reduce(case, image, dz, d)


@pytest.mark.parametrize("case", REDUCE_VECTOR, ids=lambda c: "-".join(map(str, c)))
def test_bwd_reduce_vector_kernel(case):
    """bn_bwd_reduce4_kernel<GB, CH, OB, RB>: every instantiation at C = 16, the plain and the all-16-bit one at every width; with a bf16
    dz_out the sums are those of the ROUNDED dz (g is not bf16-representable, so they differ from the unrounded sums); dz_out NULL with
    either kind of ReLU reference masks all the same"""
    assert reduce_form(case)[0] == "reduce4"
    image, dz, d = _run_reduce(case)
    _check_reduce(case, image, dz, d, "bn_bwd_reduce_io" if (case.gb or case.ch or case.ob or case.ref == "bits") else
                  ("bn_bwd_reduce_relu" if case.ref else "bn_bwd_reduce"))


@pytest.mark.parametrize("case", [R(16, 77, ref="f32", dz=True), R(7, 1000, cmode="mask"), R(16, 77, 1, 1, 1, ref="bits", dz=True)],
                         ids=lambda c: "-".join(map(str, c)))
def test_bwd_reduce_statistics_buffer(case):
    """a buffer that holds 1e300 gives the sums of a zeroed one (the call zeroes it), and SRBH_BN_STATS_CLEAN on a zeroed buffer gives them
    too: each of the three images holds the oracle's sums within the bound, and the same slots are exactly zero (the images are not
    equal bit for bit: the order of a block's fp32 LDS atomics is not fixed)"""
    blocks = O.grid(reduce_items(case)[0])
    assert blocks < O.NSLOT
    s_w, q_w, _, s_abs, q_abs = reduce_want(case)
    for stale, extra_io in ((0.0, 0), (1e300, 0), (0.0, STATS_CLEAN)):          # (the flag goes through srbh_bn_bwd_reduce_io, which takes it)
        image, _, _ = _run_reduce(case, stale=stale, extra_io=extra_io)
        s, q = O.fold(image)
        assert _ratio(s, s_w, s_abs) <= SUM_BOUND and _ratio(q, q_w, q_abs) <= SUM_BOUND, (stale, extra_io)
        assert not bool(image[blocks:].any()) and bool(image[:blocks, 0].all())


def spike_positions(n, stride):
    """about 64 positions of 0 .. n-1: the first and last element, both sides of every multiple of the grid stride, the rest spread evenly"""
    pos = {0, n - 1}
    for k in range(stride, n, stride):
        pos |= {k - 1, k}
    extra = max(64 - len(pos), 0)
    pos |= {(i * 2654435761) % n for i in range(1, extra + 1)}
    return sorted(pos)


@pytest.mark.parametrize("case", [R(7, 73800, cmode="none"), R(4, BIG, cmode="none")], ids=lambda c: "-".join(map(str, c)))
def test_bwd_reduce_spikes(case):
    """g zero except 1.0 at ~64 positions around every seam of the capped grid: a dropped or doubled work item changes an integer sum"""
    items, block = reduce_items(case)
    assert O.trips(items, block=block) == 2
    g = torch.zeros((case.npix, case.C))
    pos = spike_positions(items, O.stride(items, block=block))        # work items: elements (scalar kernel) or 4-channel groups
    g.view(-1)[torch.tensor(pos if reduce_form(case)[0] == "scalar" else [p * 4 + p % 4 for p in pos])] = 1.0
    image, _, _ = _run_reduce(case, g_cpu=g)
    s, q = O.fold(image)
    assert torch.equal(s, g.double().sum(0)) and not bool(q.any())


# ---- backward apply -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def apply_want(case):
    x = _case_inputs(case)
    return O.bn_bwd_apply(x.g, x.c, x.mean, x.invstd, (x.ms, x.mh) if case.mask else None, x.coef, x.k1, x.k2)


def _run_apply(case, g_cpu=None, vectors=None, expect_ok=True, vec_offset=0):
    m, L = _lib()
    x = _case_inputs(case)
    v = x if vectors is None else vectors
    C, npix = case.C, case.npix
    g_cpu = x.g if g_cpu is None else g_cpu
    bufs = Buffers()
    g = bufs.inp(g_cpu, 1 if case.mis else 0, dtype=g_cpu.dtype)
    c = bufs.inp(x.c, dtype=x.c.dtype)
    mean, invstd, coef, k1 = bufs.inp(v.mean), bufs.inp(v.invstd), bufs.inp(v.coef), bufs.inp(v.k1)
    k2 = bufs.inp(v.k2, vec_offset)
    ms, mh = (bufs.inp(x.ms), bufs.inp(x.mh)) if case.mask else (None, None)
    out = bufs.out((npix, C), dtype=torch.bfloat16 if case.ob else torch.float32)
    io = (G_B16 if case.gb else 0) | (C_H16 if case.ch else 0) | (OUT_B16 if case.ob else 0)
    if io == 0 and not vec_offset:
        rc = L.srbh_bn_bwd_apply(_p(g), _p(c), _p(mean), _p(invstd), _p(ms), _p(mh), _p(coef), _p(k1), _p(k2), _p(out), npix, C, m.stream_ptr())
    else:
        rc = L.srbh_bn_bwd_apply_io(_p(g), _p(c), _p(mean), _p(invstd), _p(ms), _p(mh), _p(coef), _p(k1), _p(k2), _p(out), npix, C, io,
                                    m.stream_ptr())
    if not expect_ok:
        return rc, bufs
    m.check(rc, "bn_bwd_apply")
    bufs.verify()
    dy = g.float()
    if case.mask:
        dy = torch.where(c.float() * ms + mh > 0, dy, torch.zeros_like(dy))
    stock = coef * (dy - k1 - (c.float() - mean) * invstd * k2)
    return out, stock


def _check_apply(case):
    out, stock = _run_apply(case)
    want, M = apply_want(case)
    bound = K_APPLY * EPS
    if case.ob:
        M = M + want.abs() * (O.BF16_REL / bound)            # the fp32 bound + 2^-8 |want|, in units of the fp32 bound
        stock = stock.bfloat16()
    e = _ratio(out.float(), want, M)
    _report("bn_bwd_apply" + ("_io" if case.gb or case.ch or case.ob else "") + "/" + apply_form(case)[0], case, e, _ratio(stock.float(), want, M), bound)
    assert e <= bound


@pytest.mark.parametrize("case", APPLY_SCALAR, ids=lambda c: "-".join(map(str, c)))
def test_bwd_apply_scalar_kernel(case):
    """bn_bwd_apply_kernel: channel counts the vector form cannot take, C = 16 behind the alignment fallback, a second grid-stride trip"""
    assert apply_form(case)[0] == "scalar"
    _check_apply(case)


@pytest.mark.parametrize("case", APPLY_VECTOR, ids=lambda c: "-".join(map(str, c)))
def test_bwd_apply_vector_kernel(case):
    """bn_bwd_apply4_kernel<GB, CH, OB>: every instantiation at C = 16, the plain one at every width, a second grid-stride trip"""
    assert apply_form(case)[0] == "apply4"
    _check_apply(case)


def test_bwd_apply_spikes():
    """coef = 1, k1 = k2 = 0: the output is g itself, 1.0 at ~64 positions around the seams of the capped grid and zero elsewhere"""
    case = A(4, BIG)
    items = apply_items(case)
    assert O.trips(items) == 2
    g = torch.zeros((case.npix, case.C))
    g.view(-1)[torch.tensor([p * 4 + p % 4 for p in spike_positions(items, O.stride(items))])] = 1.0
    x = _case_inputs(case)
    one, zero = torch.ones(case.C), torch.zeros(case.C)
    out, _ = _run_apply(case, g_cpu=g, vectors=SimpleNamespace(mean=x.mean, invstd=x.invstd, coef=one, k1=zero, k2=zero))
    assert torch.equal(out.cpu(), g)


# ---- the two finalize kernels (one block; fold_stat_slots) --------------------------------------------------------------------------------
def fold_keep(C):
    """slots that must hold something: the first and the last slot of the fold's last group that owns any (a fold that skips that
    group then loses them)"""
    sl = O.fold_group_slots(C, min(O.fold_groups(C), O.NSLOT) - 1)
    return tuple(sorted({sl[0], sl[-1]}))


@functools.lru_cache(maxsize=None)
def finalize_inputs(C, count):
    """a statistics image with known totals: `count` float64 rows [x, x^2] (channel means up to 100, spreads 0.5-2; with C > 1 the
    last channel is the constant 3.0: its variance is exactly 0) spread over the slots, some slots left empty"""
    gen = torch.Generator().manual_seed(31 * C + count)
    x = torch.randn((count, C), generator=gen, dtype=torch.float64) * (0.5 + 1.5 * torch.rand(C, generator=gen, dtype=torch.float64)) + \
        (torch.rand(C, generator=gen, dtype=torch.float64) * 200 - 100)
    if C > 1:
        x[:, -1] = 3.0
    v = SimpleNamespace(image=O.split_into_slots(torch.stack([x, x * x], 1), gen, fold_keep(C)), x=x)
    v.gamma, v.beta = (0.5 + torch.rand(C, generator=gen)) * _sign((C,), gen), torch.randn(C, generator=gen)
    v.rm, v.rv = torch.randn(C, generator=gen) * 10, torch.rand(C, generator=gen) + 0.5
    v.invstd = 0.4 + 1.2 * torch.rand(C, generator=gen)
    return v


FWD_NULLS = (None, "affine", "running", "save")
BN_EPS = 1e-5


def _run_finalize(C, count, null, momentum, clear):
    m, L = _lib()
    v = finalize_inputs(C, count)
    bufs = Buffers()
    stats = bufs.out((O.NSLOT, 2, C), dtype=torch.float64, fill=v.image) if clear else bufs.inp(v.image, dtype=torch.float64)
    gamma, beta = (None, None) if null == "affine" else (bufs.inp(v.gamma), bufs.inp(v.beta))
    rm, rv = (None, None) if null == "running" else (bufs.out((C,), fill=v.rm), bufs.out((C,), fill=v.rv))
    sm, si = (None, None) if null == "save" else (bufs.out((C,)), bufs.out((C,)))
    scale, shift = bufs.out((C,)), bufs.out((C,))
    fn = L.srbh_bn_finalize_clear if clear else L.srbh_bn_finalize
    m.check(fn(_p(stats), C, float(count), _p(gamma), _p(beta), BN_EPS, momentum, _p(rm), _p(rv), _p(scale), _p(shift), _p(sm), _p(si), m.stream_ptr()),
            "bn_finalize")
    bufs.verify()
    return dict(scale=scale, shift=shift, save_mean=sm, save_invstd=si, running_mean=rm, running_var=rv), stats


@pytest.mark.parametrize("null", FWD_NULLS)
@pytest.mark.parametrize("count", FINALIZE_COUNTS)
@pytest.mark.parametrize("C", FINALIZE_WIDTHS)
def test_bn_finalize_and_clear(C, count, null):
    """srbh_bn_finalize on known sums at every width of the fold (idle threads 0 / 4 / 16 / 64, C = 1: more groups than slots), count 1
    (no unbiased correction), a constant channel (variance 0, invstd = 1 / sqrt(eps)), each optional pointer group NULL in turn; the
    plain call leaves the image as it was; srbh_bn_finalize_clear gives the same bits and leaves the image all zero"""
    v = finalize_inputs(C, count)
    momentum = 0.1 if (C + count) % 2 else 0.01
    got, _ = _run_finalize(C, count, null, momentum, clear=False)
    got_c, stats_c = _run_finalize(C, count, null, momentum, clear=True)
    assert not bool(stats_c.any()), "srbh_bn_finalize_clear left a non-zero slot"
    w = O.bn_finalize(v.image, count, None if null == "affine" else v.gamma, None if null == "affine" else v.beta, BN_EPS, momentum,
                      None if null == "running" else v.rm, None if null == "running" else v.rv)
    if C > 1 or count == 1:
        assert float(w["save_invstd"][-1]) == pytest.approx(1.0 / O._f32(BN_EPS) ** 0.5, rel=1e-12)      # the clamped / zero variance
    s32, q32 = (t.float().to(DEV) for t in O.fold(v.image))
    mean32 = s32 / count
    inv32 = torch.rsqrt((q32 / count - mean32 * mean32).clamp_min(0) + BN_EPS)
    stock = dict(save_mean=mean32, save_invstd=inv32)
    worst = stock_worst = 0.0
    for name, t in got.items():
        if t is None:
            continue
        assert _bits_equal(t, got_c[name]), name
        M = w.get("M_" + name, w[name].abs())
        e = _ratio(t, w[name], M)
        worst = max(worst, e)
        if name in stock:
            stock_worst = max(stock_worst, _ratio(stock[name], w[name], M))
        assert e <= K_FIN * EPS, (name, e)
    _report("bn_finalize", (C, count, null), worst, stock_worst, K_FIN * EPS)


@functools.lru_cache(maxsize=None)
def bwd_finalize_inputs(C, count):
    gen = torch.Generator().manual_seed(77 * C + count)
    dy = torch.randn((count, C), generator=gen, dtype=torch.float64) + (torch.rand(C, generator=gen, dtype=torch.float64) - 0.5)
    xhat = torch.randn((count, C), generator=gen, dtype=torch.float64)
    v = SimpleNamespace(image=O.split_into_slots(torch.stack([dy, dy * xhat], 1), gen, fold_keep(C)))
    v.gamma, v.invstd = (0.5 + torch.rand(C, generator=gen)) * _sign((C,), gen), 0.4 + 1.2 * torch.rand(C, generator=gen)
    return v


def _run_bwd_finalize(C, count, null, clear):
    m, L = _lib()
    v = bwd_finalize_inputs(C, count)
    bufs = Buffers()
    stats = bufs.out((O.NSLOT, 2, C), dtype=torch.float64, fill=v.image) if clear else bufs.inp(v.image, dtype=torch.float64)
    gamma = None if null == "gamma" else bufs.inp(v.gamma)
    invstd = bufs.inp(v.invstd)
    dg, db = (None, None) if null == "dgamma" else (bufs.out((C,)), bufs.out((C,)))
    coef, k1, k2 = (None, None, None) if null == "coef" else (bufs.out((C,)), bufs.out((C,)), bufs.out((C,)))
    fn = L.srbh_bn_bwd_finalize_clear if clear else L.srbh_bn_bwd_finalize
    m.check(fn(_p(stats), C, float(count), _p(gamma), _p(invstd), _p(dg), _p(db), _p(coef), _p(k1), _p(k2), m.stream_ptr()), "bn_bwd_finalize")
    bufs.verify()
    return dict(dgamma=dg, dbeta=db, coef=coef, k1=k1, k2=k2), stats


@pytest.mark.parametrize("null", (None, "gamma", "dgamma", "coef"))
@pytest.mark.parametrize("count", FINALIZE_COUNTS)
@pytest.mark.parametrize("C", FINALIZE_WIDTHS)
def test_bn_bwd_finalize_and_clear(C, count, null):
    """srbh_bn_bwd_finalize on known sums, as test_bn_finalize_and_clear: every width of the fold, gamma NULL (= 1), the gradient pair
    NULL, the constants NULL; the _clear variant gives the same bits and leaves the image all zero"""
    v = bwd_finalize_inputs(C, count)
    got, _ = _run_bwd_finalize(C, count, null, clear=False)
    got_c, stats_c = _run_bwd_finalize(C, count, null, clear=True)
    assert not bool(stats_c.any()), "srbh_bn_bwd_finalize_clear left a non-zero slot"
    s, q = O.fold(v.image)
    w = O.bn_bwd_finalize(s, q, count, None if null == "gamma" else v.gamma, v.invstd)
    worst = 0.0
    for name, t in got.items():
        if t is None:
            continue
        assert _bits_equal(t, got_c[name]), name
        e = _ratio(t, w[name], w[name].abs())
        worst = max(worst, e)
        assert e <= K_FIN * EPS, (name, e)
    stock = _ratio((s.float().to(DEV) / count), w["k1"], w["k1"].abs())
    _report("bn_bwd_finalize", (C, count, null), worst, stock, K_FIN * EPS)


# ---- residual tail --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bar_inputs(C, npix, io):
    gen = torch.Generator().manual_seed(13 * C + npix + 101 * io)
    a, idt = torch.randn((npix, C), generator=gen) * 1.5 + 0.3, torch.randn((npix, C), generator=gen)
    v = SimpleNamespace(a=a.half() if io & 1 else a, idt=idt.half() if io & 2 else idt)
    v.sa, v.ha = (0.5 + torch.rand(C, generator=gen)) * _sign((C,), gen), torch.randn(C, generator=gen) * 0.5
    v.si, v.hi = (0.5 + torch.rand(C, generator=gen)) * _sign((C,), gen), torch.randn(C, generator=gen) * 0.5
    return v


def _run_bar(C, npix, io, with_si, bits, a_cpu=None, vectors=None, offsets=None, expect_ok=True):
    """srbh_bn_add_relu (io = 0, no bits), srbh_bn_add_relu_io or srbh_bn_add_relu_bits.  offsets: elements past alignment, by name"""
    m, L = _lib()
    v = bar_inputs(C, npix, io)
    vec = v if vectors is None else vectors
    off = offsets or {}
    a_cpu = v.a if a_cpu is None else a_cpu
    bufs = Buffers()
    a, idt = bufs.inp(a_cpu, off.get("a", 0), dtype=a_cpu.dtype), bufs.inp(v.idt, off.get("idt", 0), dtype=v.idt.dtype)
    sa, ha = bufs.inp(vec.sa, off.get("sa", 0)), bufs.inp(vec.ha, off.get("ha", 0))
    si, hi = (bufs.inp(vec.si, off.get("si", 0)), bufs.inp(vec.hi, off.get("hi", 0))) if with_si else (None, None)
    out = bufs.out((npix, C), off.get("out", 0))
    words = None
    if bits:
        nbytes = L.srbh_relu_bits_bytes(npix, C)
        assert nbytes == (npix * C // 4 + 63) // 64 * 32
        words = bufs.out((nbytes // 8,), off.get("bits", 0), dtype=torch.int64)
    if bits:
        rc = L.srbh_bn_add_relu_bits(_p(a), _p(sa), _p(ha), _p(idt), _p(si), _p(hi), _p(out), _p(words), npix, C, io, m.stream_ptr())
    elif io == 0:
        rc = L.srbh_bn_add_relu(_p(a), _p(sa), _p(ha), _p(idt), _p(si), _p(hi), _p(out), npix, C, m.stream_ptr())
    else:
        rc = L.srbh_bn_add_relu_io(_p(a), _p(sa), _p(ha), _p(idt), _p(si), _p(hi), _p(out), npix, C, io, m.stream_ptr())
    if not expect_ok:
        return rc, bufs
    m.check(rc, "bn_add_relu")
    bufs.verify()
    d = idt.float() * si + hi if with_si else idt.float()
    return out, words, torch.relu(a.float() * sa + ha + d)


@pytest.mark.parametrize("C,npix,io,with_si,bits", BAR_CASES)
def test_bn_add_relu(C, npix, io, with_si, bits):
    """bn_add_relu_kernel<AH, IH>: the per-channel vector index (4 i) % C at C = 12 (wraps at a non-power-of-two), one pixel, a ragged
    last wave, a second trip of the 4 096-block grid; the bit words that cover groups below n4 are the activity pattern of the fp32
    `out` this very call wrote (the bits of later groups are unspecified)"""
    v = bar_inputs(C, npix, io)
    out, words, stock = _run_bar(C, npix, io, with_si, bits)
    want, M = O.bn_add_relu(v.a, v.sa, v.ha, v.idt, v.si if with_si else None, v.hi if with_si else None)
    e = _ratio(out, want, M)
    entry = "bn_add_relu_bits" if bits else ("bn_add_relu_io" if io else "bn_add_relu")
    _report(entry, (C, npix, io, with_si, bits), e, _ratio(stock, want, M), K_BAR * EPS)
    assert e <= K_BAR * EPS
    if bits:
        n4 = npix * C // 4
        assert torch.equal(O.unpack_relu_bits(words, n4), out.cpu().view(n4, 4) > 0)
        assert torch.equal(O.unpack_relu_bits(O.relu_bits(out), n4), out.cpu().view(n4, 4) > 0)


def test_bn_add_relu_spikes():
    """scale 1, shifts 0, identity 0: the output is `a` itself, 1.0 at ~64 positions around the seams of the 4 096-block grid"""
    C, npix = 16, BAR_BIG
    items = npix * C // 4
    assert O.trips(items, O.GRID_CAP_BAR) == 2
    a = torch.zeros((npix, C))
    a.view(-1)[torch.tensor([p * 4 + p % 4 for p in spike_positions(items, O.stride(items, O.GRID_CAP_BAR))])] = 1.0
    one, zero = torch.ones(C), torch.zeros(C)
    out, words, _ = _run_bar(C, npix, 0, True, True, a_cpu=a, vectors=SimpleNamespace(sa=one, ha=zero, si=zero, hi=zero))
    assert torch.equal(out.cpu(), a)
    assert torch.equal(O.unpack_relu_bits(words, items), a.view(items, 4) > 0)


# ---- ReLU mask, in-place add, nearest-x2, NCHW -> NHWC, aggregate ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", ELTWISE_N)
def test_relu_mask_mul(n):
    """one work item, a ragged last block, a second trip; ref holds +0.0 and -0.0 (both masked); an inf in g at a masked position
    comes out 0: a select, not a product.  Bit-exact"""
    m, L = _lib()
    gen = torch.Generator().manual_seed(n)
    g, ref = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    ref[0], ref[1], ref[2] = 0.0, -0.0, -1.0
    g[0] = g[2] = float("inf")
    g[1] = float("-inf")
    ref[n - 1] = 2.0
    bufs = Buffers()
    gd, rd = bufs.inp(g), bufs.inp(ref)
    out = bufs.out((n,))
    m.check(L.srbh_relu_mask_mul(_p(gd), _p(rd), _p(out), n, m.stream_ptr()), "relu_mask_mul")
    bufs.verify()
    assert _bits_equal(out.cpu(), O.relu_mask(g, ref))
    assert float(out[0]) == 0.0 and float(out[1]) == 0.0 and float(out[2]) == 0.0


@pytest.mark.parametrize("n", ELTWISE_N)
def test_add_inplace(n):
    m, L = _lib()
    gen = torch.Generator().manual_seed(n + 1)
    a, b = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 3
    bufs = Buffers()
    ad, bd = bufs.out((n,), fill=a), bufs.inp(b)
    m.check(L.srbh_add_inplace(_p(ad), _p(bd), n, m.stream_ptr()), "add_inplace")
    bufs.verify()
    assert _bits_equal(ad.cpu(), a + b)


@pytest.mark.parametrize("B,H,W,C", [(1, 2, 2, 4), (3, 6, 10, 12), (2, 4, 4, 64)])
def test_nearest2x(B, H, W, C):
    m, L = _lib()
    src = torch.randn((B, H // 2, W // 2, C), generator=torch.Generator().manual_seed(H * W + C))
    bufs = Buffers()
    sd, out = bufs.inp(src), bufs.out((B, H, W, C))
    m.check(L.srbh_nearest2x_f32(_p(sd), _p(out), B, H, W, C, m.stream_ptr()), "nearest2x")
    bufs.verify()
    assert _bits_equal(out.cpu(), O.nearest2x(src))


@pytest.mark.parametrize("B,C,H,W", [(1, 1, 1, 1), (2, 3, 5, 7), (1, 7, 4, 6), (2, 64, 3, 2)])
def test_nchw_to_nhwc(B, C, H, W):
    m, L = _lib()
    src = torch.randn((B, C, H, W), generator=torch.Generator().manual_seed(C * H + W))
    bufs = Buffers()
    sd, out = bufs.inp(src), bufs.out((B, H, W, C))
    m.check(L.srbh_nchw_to_nhwc_f32(_p(sd), _p(out), B, C, H, W, m.stream_ptr()), "nchw_to_nhwc")
    bufs.verify()
    assert _bits_equal(out.cpu(), O.nchw_to_nhwc(src))


@pytest.mark.parametrize("N,H,W,step", [(3, 8, 8, 4), (2, 10, 7, 3), (1, 5, 5, 1), (2, 8, 8, 8)])
def test_aggregate(N, H, W, step):
    """ragged H / W (the rest is not read), step 1, one block per image; negatives, -0.0 (counts as >= 0), and one block that is all
    negative: its count is 0 and the result is the sum / fp32(1e-10)"""
    m, L = _lib()
    data = torch.randn((N, H, W), generator=torch.Generator().manual_seed(H * 10 + step))
    data[0, :step, :step] = -data[0, :step, :step].abs() - 0.25
    data[-1, -1 - (H % step), -1 - (W % step)] = -0.0
    bufs = Buffers()
    dd, out = bufs.inp(data), bufs.out((N, H // step, W // step))
    m.check(L.srbh_aggregate(_p(dd), _p(out), N, H, W, step, m.stream_ptr()), "aggregate")
    bufs.verify()
    want, M = O.aggregate(data, step)
    assert float(want[0, 0, 0]) < -1e9
    blk = dd[:, :H // step * step, :W // step * step].reshape(N, H // step, step, W // step, step)
    stock = blk.sum((2, 4)) / ((blk >= 0).float().sum((2, 4)) + 1e-10)
    e, bound = _ratio(out, want, M), min((step * step + 2) * EPS, AGG_BOUND)
    _report("aggregate", (N, H, W, step), e, _ratio(stock, want, M), bound)
    assert e <= bound


# ---- refusals: a non-zero return code, no output written, no HIP error left behind ----------------------------------------------------------
def test_refusals_of_the_backward_reduce():
    m, L = _lib()
    # srbh_bn_bwd_reduce_relu at C = 12 (no vector form: 256 % 3 != 0)
    for case in (R(12, 37, ref="f32", dz=True), R(12, 37, ref="f32")):
        rc, bufs, _ = _run_reduce(case, expect_ok=False)
        assert rc != 0 and b"reduce" in L.srbh_last_error()
        bufs.verify(written=False)
    # a 16-bit form with a tensor that is 2 bytes past its alignment
    rc, bufs, _ = _run_reduce(R(16, 37, gb=1, mis=True), expect_ok=False)
    assert rc != 0
    bufs.verify(written=False)
    # C = 65
    rc, bufs, _ = _run_reduce(R(65, 3), expect_ok=False)
    assert rc != 0
    bufs.verify(written=False)
    # SRBH_BN_REF_BITS together with a mask (called directly: no case of the tables has both)
    x = bwd_inputs(16, 37)
    bufs = Buffers()
    g, c, mean, invstd, ms, mh = (bufs.inp(t) for t in (x.g, x.c, x.mean, x.invstd, x.ms, x.mh))
    bits = bufs.inp(x.bits, dtype=torch.int64)
    dz = bufs.out((37, 16))
    stats = bufs.out((O.NSLOT, 2, 16), dtype=torch.float64)
    rc = L.srbh_bn_bwd_reduce_io(_p(g), _p(bits), _p(dz), _p(c), _p(mean), _p(invstd), _p(ms), _p(mh), 37, 16, _p(stats), REF_BITS, m.stream_ptr())
    assert rc != 0
    bufs.verify(written=False)
    _no_error_pending()


def test_refusals_of_the_backward_apply():
    m, L = _lib()
    rc, bufs = _run_apply(A(16, 37, gb=1, mis=True), expect_ok=False)                 # bf16 g, 2 bytes past 8-byte alignment
    assert rc != 0
    bufs.verify(written=False)
    rc, bufs = _run_apply(A(12, 37, ob=1), expect_ok=False)                            # a 16-bit form without a vector kernel
    assert rc != 0
    bufs.verify(written=False)
    rc, bufs = _run_apply(A(16, 37, ch=1), expect_ok=False, vec_offset=1)              # a per-channel vector 4 bytes past 16-byte alignment
    assert rc != 0 and b"apply_io" in L.srbh_last_error()
    bufs.verify(written=False)
    _no_error_pending()


@pytest.mark.parametrize("which", ["a", "idt", "out", "sa", "ha", "si", "hi"])
@pytest.mark.parametrize("io,bits", [(0, False), (3, False), (3, True)])
def test_refusals_of_bn_add_relu_unaligned(which, io, bits):
    """every tensor and per-channel vector is read in 16-byte (fp16 tensors: 8-byte) groups: one element past alignment is refused"""
    m, L = _lib()
    rc, bufs = _run_bar(16, 37, io, True, bits, offsets={which: 1}, expect_ok=False)
    assert rc != 0 and b"bn_add_relu" in L.srbh_last_error()
    bufs.verify(written=False)
    _no_error_pending()


def test_refusals_of_the_other_entry_points():
    m, L = _lib()
    rc, bufs = _run_bar(65, 3, 0, False, False, expect_ok=False)                               # C % 4 != 0
    assert rc != 0
    bufs.verify(written=False)
    # C = 65 at the two finalize kernels
    bufs = Buffers()
    stats = bufs.inp(torch.ones((O.NSLOT, 2, 65), dtype=torch.float64), dtype=torch.float64)
    outs = [bufs.out((65,)) for _ in range(5)]
    invstd = bufs.inp(torch.ones(65))
    assert L.srbh_bn_finalize(_p(stats), 65, 10.0, None, None, BN_EPS, 0.1, None, None, _p(outs[0]), _p(outs[1]), _p(outs[2]), _p(outs[3]),
                              m.stream_ptr()) != 0
    assert L.srbh_bn_bwd_finalize(_p(stats), 65, 10.0, None, _p(invstd), _p(outs[0]), _p(outs[1]), _p(outs[2]), _p(outs[3]), _p(outs[4]),
                                  m.stream_ptr()) != 0
    assert L.srbh_bn_finalize_clear(_p(stats), 65, 10.0, None, None, BN_EPS, 0.1, None, None, _p(outs[0]), _p(outs[1]), _p(outs[2]), _p(outs[3]),
                                    m.stream_ptr()) != 0
    bufs.verify(written=False)
    _no_error_pending()
