"""The split-fp16 tail kernel (csrc/srbh_ptail_split.hip) compiled for gfx950: no scratch (its three unrolled passes keep 128 accumulator
registers live across 864 MFMAs; as a runtime loop it spilled; each pass is its own scheduling region) and every product is there.  (The hazard
scan around its LDS-DMA asm and its scratch budget: tests/test_isa_hazards.py, tests/test_isa_registers.py.)"""
import os, re, shutil, subprocess
import pytest

from tests.test_isa_hazards import CSRC, HIPCC, ROOT

SRC = "srbh_ptail_split.hip"


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("isa") / (SRC + ".s"))
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-inline-asm", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
           "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, SRC)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def test_no_scratch_and_every_product_is_there(isa):
    text = open(isa).read()
    kernels = re.findall(r"\.name:\s+(\S*ptail_split_kernel\S*)", text)
    assert len(set(kernels)) == 2, kernels            # plain and nearest-x2 read
    for key in ("private_segment_fixed_size", "vgpr_spill_count"):      # (every kernel of the file: the two forms and the lo' plane kernel)
        vals = [int(v) for v in re.findall(r"\.%s:\s+(\d+)" % key, text)]
        assert len(vals) == 3 and not any(vals), (key, vals)
    assert "scratch_" not in text
    # 3 passes x 288 MFMAs per tile and kernel (the compiler folds two of the 576 of a fp16 pass pair in the nearest-x2 form, as in srbh_ptail.hip)
    assert 2 * 864 - 4 <= len(re.findall(r"\bv_mfma_f32_32x32x16_f16\b", text)) <= 2 * 864
