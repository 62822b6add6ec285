"""Thin test-side wrappers that drive individual libsrbh entry points through the C ABI."""
import ctypes as C
import math

import torch
import torch.nn.functional as F

from srbh_amd import _lib


def act16_from_nchw(x, chunks_total=None):
    """(B,C,H,W) fp32 cuda -> zero-bordered ACT16 buffer (uint8 tensor)."""
    L = _lib.lib()
    B, Cc, H, W = x.shape
    ch = chunks_total or (Cc + 31) // 32
    buf = torch.zeros(L.srbh_act16_bytes(B, ch * 32, H, W), dtype=torch.uint8, device=x.device)
    _lib.check(L.srbh_nchw32_to_act16(x.contiguous().data_ptr(), buf.data_ptr(), B, Cc, H, W, _lib.stream_ptr()))
    return buf


def act16_alloc(B, chunks, H, W, device):
    return torch.zeros(_lib.lib().srbh_act16_bytes(B, chunks * 32, H, W), dtype=torch.uint8, device=device)


def act16_to_nchw(buf, B, Cc, H, W):
    out = torch.empty(B, Cc, H, W, dtype=torch.float32, device=buf.device)
    _lib.check(_lib.lib().srbh_act16_to_nchw32(buf.data_ptr(), out.data_ptr(), B, Cc, H, W, _lib.stream_ptr()))
    return out


def pack_w(w):
    L = _lib.lib()
    cout, cin = w.shape[:2]
    buf = torch.zeros(L.srbh_wpack16_bytes(cout, cin), dtype=torch.uint8, device=w.device)
    _lib.check(L.srbh_pack_conv3x3_f16(w.contiguous().data_ptr(), cout, cin, buf.data_ptr(), _lib.stream_ptr()))
    return buf


def conv_args(**kw):
    a = _lib.ConvArgs()
    for k, v in kw.items():
        setattr(a, "in_" if k == "in" else k, v)
    return a


def run_conv(a):
    _lib.check(_lib.lib().srbh_conv3x3_f16(C.byref(a), _lib.stream_ptr()), "conv3x3_f16")


def h16(t):
    """round to fp16 and back (what the MFMA operands see)."""
    return t.half().float()


def ref_conv(x, w, b, ups=False, rounded=True):
    """CPU fp32 conv of (optionally fp16-rounded) operands, fp32 accumulate (double for stability)."""
    x = x.double() if not rounded else h16(x).double()
    w = w.double() if not rounded else h16(w).double()
    if ups:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    return F.conv2d(x, w, None if b is None else b.double(), 1, 1).float()


# ---- 16-bit forms of the conv (srbh_conv3x3_x16): bf16 planes, bf16 packs -------------------------------------------------------
def b16(t):
    """round to bf16 (RNE) and back"""
    return t.to(torch.bfloat16).float()


def act16_from_nchw_x16(x, bf16=1, chunks_total=None, chunk0=0, scale=1.0, buf=None):
    """(B,C,H,W) fp32 cuda, C % 32 == 0 -> planes chunk0.. of a zero-bordered ACT16 buffer as bf16 (or fp16) through
    srbh_nhwc32_to_act16: the entry the gradient path and the bf16 trunk's tests feed 16-bit planes with"""
    L = _lib.lib()
    B, Cc, H, W = x.shape
    ch = chunks_total or Cc // 32
    if buf is None:
        buf = act16_alloc(B, ch, H, W, x.device)
    src = x.permute(0, 2, 3, 1).contiguous()
    _lib.check(L.srbh_nhwc32_to_act16(src.data_ptr(), buf.data_ptr(), B, Cc, H, W, ch, chunk0, scale, bf16, _lib.stream_ptr()), "nhwc32_to_act16")
    torch.cuda.current_stream().synchronize()
    return buf


def act16_raw(buf, B, chunks, H, W, dtype=torch.bfloat16):
    """the raw 16-bit elements of an ACT16 buffer, borders included: [B][chunks][H+2][W+2][32] view of `dtype`"""
    return buf.view(dtype)[: B * chunks * (H + 2) * (W + 2) * 32].view(B, chunks, H + 2, W + 2, 32)


def act16_planes(buf, B, chunks, H, W, dtype=torch.bfloat16):
    """the interior of an ACT16 buffer as a (B, 32*chunks, H, W) tensor of `dtype` (the stored bits, no conversion kernel in between)"""
    raw = act16_raw(buf, B, chunks, H, W, dtype)
    return raw[:, :, 1:-1, 1:-1].permute(0, 1, 4, 2, 3).reshape(B, chunks * 32, H, W)


def border_is_zero(buf, B, chunks, H, W):
    raw = act16_raw(buf, B, chunks, H, W, torch.int16)
    return not bool(raw[:, :, 0].any() or raw[:, :, -1].any() or raw[:, :, :, 0].any() or raw[:, :, :, -1].any())


def pack_w_b16(w):
    L = _lib.lib()
    cout, cin = w.shape[:2]
    buf = torch.zeros(L.srbh_wpack16_bytes(cout, cin), dtype=torch.uint8, device=w.device)
    _lib.check(L.srbh_pack_conv3x3_b16(w.contiguous().data_ptr(), cout, cin, buf.data_ptr(), _lib.stream_ptr()), "pack_conv3x3_b16")
    return buf


def run_conv_x16(a, bf16, mask16=None, mask_chunks_total=0, mask_chunk0=0):
    _lib.check(_lib.lib().srbh_conv3x3_x16(C.byref(a), bf16, None if mask16 is None else mask16.data_ptr(), mask_chunks_total, mask_chunk0,
                                           _lib.stream_ptr()), "conv3x3_x16")


def ref_conv64(x, w, b):
    """float64 conv of the operands AS GIVEN (round them first), float64 result"""
    return F.conv2d(x.double(), w.double(), None if b is None else b.double(), 1, 1)


# ---- memory contract of one C-ABI call: writes stay inside the outputs, inputs stay as they were -------------------------------------
SLACK = 64          # floats of NaN on either side of every output (256 bytes of guard for every other element type)
# guard pattern of the integer types, which have no NaN.  uint32 / uint16 data (the mosaics' accumulators, the finalised height) live in
# int32 / int16 storage -- torch lacks most ops on the unsigned types -- and are read back as bit patterns through a numpy view
SENTINEL = {torch.int64: 0x5AA5A55A5AA5A55A, torch.int32: 0x5AA5A55A, torch.int16: 0x5AA5, torch.uint8: 0xA5}


class GuardedBuffers:
    """the device buffers of one call: inputs with a clone to compare with afterwards, outputs carved out of guard-filled storage (NaN for
    the float types, SENTINEL for the integer types).  `offset` counts ELEMENTS of the buffer's dtype past a 16-byte boundary."""

    def __init__(self):
        self.inputs, self.outputs, self.before = [], [], {}

    @staticmethod
    def _guard(dtype):
        return float("nan") if dtype.is_floating_point else SENTINEL[dtype]

    @staticmethod
    def _carve(shape, offset, dtype=torch.float32):
        n = math.prod(shape)
        esz = torch.empty((), dtype=dtype).element_size()
        slack = SLACK * 4 // esz
        buf = torch.full((n + 2 * slack + 16 // esz,), GuardedBuffers._guard(dtype), dtype=dtype, device="cuda:0")
        view = buf[slack + offset: slack + offset + n].view(shape)
        assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == (esz * offset) % 16, (buf.data_ptr(), offset)
        return buf, view

    def inp(self, t, offset=0, dtype=torch.float32):
        """`t` on the device as `dtype`, `offset` elements past a 16-byte boundary"""
        _, v = self._carve(tuple(t.shape), offset, dtype)
        v.copy_(t)
        self.inputs.append((v, v.clone()))
        return v

    def out(self, shape, offset=0, fill=None, dtype=torch.float32):
        buf, v = self._carve(tuple(shape), offset, dtype)
        if fill is not None:
            v.copy_(fill)
        self.outputs.append((buf, v))
        self.before[id(buf)] = None if fill is None else v.clone()
        return v

    @staticmethod
    def _is_guard(t):
        return t.isnan() if t.dtype.is_floating_point else t == SENTINEL[t.dtype]

    def verify(self, written=True):
        """inputs unchanged, guards intact, and every output element written (written = False: NO output element written -- a refused call)"""
        torch.cuda.synchronize()
        for v, c in self.inputs:
            assert torch.equal(v, c), "an input was written"
        for buf, v in self.outputs:
            slack = SLACK * 4 // buf.element_size()
            lo = (v.data_ptr() - buf.data_ptr()) // buf.element_size()
            assert lo >= slack and buf.numel() - lo - v.numel() >= slack
            assert bool(self._is_guard(buf[:lo]).all()) and bool(self._is_guard(buf[lo + v.numel():]).all()), "a write outside the output"
            if not written:
                was = self.before[id(buf)]          # what the output held before the call: its guard pattern, or the `fill`
                assert bool(self._is_guard(v).all()) if was is None else torch.equal(v, was), "a refused call wrote to an output"
            elif v.element_size() > 2:        # (a byte or a 16-bit value may equal its guard by chance)
                assert not bool(self._is_guard(v).any()), "an output element was left unwritten (or is NaN)"
