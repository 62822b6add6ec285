"""Every refusal of the three wide conv entry points (srbh_wconv3x3, srbh_wconv2x2, srbh_wconv3x3_lrelu), which share one argument check
(csrc/srbh_wconv_host.h, wide_validate): the call returns SRBH_ERR_ARG and srbh_last_error() is that entry's own name and text -- not
another entry's name, not a check the form does not have.  No kernel is launched: the pointers are small dummy buffers and every call
returns before a launch (the "too many workgroups" case too: the batch is large, nothing of that size is allocated)."""
import ctypes as C

import pytest
import torch

from srbh_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SRBH_ERR_ARG = -1
W3, W2, WL = "srbh_wconv3x3", "srbh_wconv2x2", "srbh_wconv3x3_lrelu"
PTRS = ("in_", "w", "bias", "mask16", "add16", "out16", "out32")      # fields given as True take the dummy buffer's address

# arguments every entry accepts: 32 -> 64 channels, one 4 x 4 image, fp32 output of all channels
BASE = dict(in_=True, in_chunks_total=1, in_chunk0=0, in_chunks=1, w=True, cout=64, B=1, H=4, W=4, out32=True, out32_c=64)
NO_EPILOGUE = {WL: "no bias / relu / mask16 / add16 in this form", W2: "no bias / relu / mask16 / add16 / out16 in this form"}


def _cases():
    out = []
    for e in (W3, W2, WL):
        def add(name, text, **change):
            out.append(pytest.param(e, change, f"{e}: {text}", id=f"{e[5:]}-{name}"))
        add("null_args", "null args", args=None)
        null = {W3: "null input/weight pointer", WL: "null input / weight pointer", W2: "null input / weight / out32 pointer"}[e]
        add("null_in", null, in_=None)
        add("null_w", null, w=None)
        add("cout_96", ("cout must be a multiple of 64 (got 96)" if e == W2 else "cout must be 32 or a multiple of 64 (got 96)"), cout=96, out32_c=96)
        add("cout_0", ("cout must be a multiple of 64 (got 0)" if e == W2 else "cout must be 32 or a multiple of 64 (got 0)"), cout=0)
        add("geometry_B", "bad geometry B=0 H=4 W=4", B=0)
        add("geometry_W", "bad geometry B=1 H=4 W=-1", W=-1)
        add("in_chunks_0", "input chunk range [0,+0) outside 1 planes", in_chunks=0)
        add("in_chunk0_past", "input chunk range [1,+1) outside 1 planes", in_chunk0=1)
        add("too_many_workgroups", "too many workgroups", B=1 << 30)
        if e == W2:
            add("null_out32", null, out32=None)
            add("cout_32", "cout must be a multiple of 64 (got 32)", cout=32, out32_c=32)
            add("out32_c", "out32_c=32 must equal cout=64", out32_c=32)
            add("takes_no_out16", NO_EPILOGUE[e], out16=True, out16_chunks_total=2)
        else:
            add("no_output", "no output requested", out32=None)
            add("out16_range", "output chunk range outside its buffer", out16=True, out16_chunks_total=1)
            add("out16_chunk0", "output chunk range outside its buffer", out16=True, out16_chunks_total=4, out16_chunk0=-1)
            add("out32_c_0", "out32_c=0 invalid", out32_c=0)
            add("out32_c_65", "out32_c=65 invalid", out32_c=65)
        if e == W3:
            add("mask_range", "mask chunk range outside its buffer", mask16=True, mask_chunks_total=1)
            add("add_range", "addend chunk range outside its buffer", add16=True, add_chunks_total=2, add_chunk0=1)
            add("no_output_before_ranges", "no output requested", out32=None, mask16=True, mask_chunks_total=1)
        else:
            add("takes_no_bias", NO_EPILOGUE[e], bias=True)
            add("takes_no_relu", NO_EPILOGUE[e], relu=1)
            add("takes_no_mask16", NO_EPILOGUE[e], mask16=True, mask_chunks_total=2)
            add("takes_no_add16", NO_EPILOGUE[e], add16=True, add_chunks_total=2)
        if e == WL:
            add("form_before_outputs", NO_EPILOGUE[e], relu=1, out32=None)
    return out


@pytest.fixture(scope="module")
def dummy():
    return torch.zeros(4096, dtype=torch.uint8, device=DEV)


@pytest.mark.parametrize("entry,change,want", _cases())
def test_refusal_names_its_own_entry(dummy, entry, change, want):
    L = _lib.lib()
    fields = {**BASE, **change}
    a = None
    if fields.pop("args", True) is not None:
        a = _lib.WConvArgs()
        for k, v in fields.items():
            setattr(a, k, (dummy.data_ptr() if v else None) if k in PTRS else v)
    rc = getattr(L, entry)(None if a is None else C.byref(a), _lib.stream_ptr())
    got = L.srbh_last_error().decode()
    print(f"{entry}: rc={rc} {got!r}")
    assert rc == SRBH_ERR_ARG
    assert got == want
    assert not dummy.any()
