"""The epilogue forms of the persistent tail conv kernel (csrc/srbh_ptail.hip) compiled for gfx950: what each form's instruction stream holds.

Per kernel symbol ptail_kernel<UPS, LRELU, OUT, FULL> (LRELU 2 = run time, OUT 1 = 16-bit, 2 = fp32, 3 = run time):
  * no scratch and no spilled VGPR, in every form;
  * every product is there: 288 MFMAs per tile pass (UPS = 1: 286 -- with zero accumulators the first MFMAs of output rows 1 and 2 read the same
    input row of the nearest-x2 map through the same weights, and the compiler folds each of the two pairs, as it always has: same sums);
  * the full-tile forms store without predication: no s_and_saveexec_b64 between the first and the last global_store_dwordx4, exactly 32 (fp32)
    or 16 (16-bit) stores -- the count the wait at the top of the tile loop relies on;
  * conv_hr's fp32 form (<0, 0, 2, 1>) has no v_cvt_pk_f16_f32 / v_cvt_f16_f32 and no half-wave swap anywhere, and no v_cndmask_b32 in its
    per-tile code.  (Five selects remain in the set-up in front of the tile loop -- the masked tail units of the input DMA addresses and one
    flag of the bias load -- in this form as in every other and in the general form before the forms existed; they run once per workgroup.)

`python -m tests.test_isa_ptail_forms` prints the census that profiles/ptail_forms_isa_census.txt records."""
import os
import re
import shutil
import subprocess
import sys

import pytest

from tests.test_isa_hazards import CSRC, HIPCC, ROOT

SRC = "srbh_ptail.hip"
OPS = ["v_mfma_f32_32x32x16_f16", "ds_read_b128", "global_load_lds_dwordx4", "v_accvgpr_read_b32", "v_pk_add_f32", "v_add_f32", "v_pk_mul_f32", "v_max_f32",
       "v_cmp_nle_f32", "v_cndmask_b32", "v_cvt_pk_f16_f32", "v_cvt_f16_f32", "v_permlane32_swap", "global_store_dwordx4", "s_and_saveexec_b64",
       "s_cbranch_execz", "s_barrier"]
FORMS = {(u, 2, 3, 0) for u in (0, 1)} | {(u, l, o, 1) for u in (0, 1) for l in (0, 1) for o in (1, 2)}
SETUP_SELECTS = 5


def compile_isa(out):
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-inline-asm", "-Wno-unused-result", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
           "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, SRC)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read()


def census(text):
    """{(UPS, LRELU, OUT, FULL): dict(scratch, vgprs, spills, lines = the kernel's instructions, tile = those from the first MFMA's tile pass to the
    last store, n = {mnemonic: count})}"""
    out = {}
    for m in re.finditer(r"^(_Z\S*ptail_kernelILi(\d)ELi(\d)ELi(\d)ELi(\d)E\S*):[^\n]*\n(.*?)^\.Lfunc_end", text, re.S | re.M):
        sym, form = m.group(1), tuple(int(v) for v in m.group(2, 3, 4, 5))
        lines = [l.strip() for l in m.group(6).splitlines() if l.strip() and not l.strip().startswith((";", ".")) and not l.strip().endswith(":")]
        md = re.search(r"\.name:\s+%s\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)"
                       % re.escape(sym), text)
        at = lambda op: [i for i, l in enumerate(lines) if l.startswith(op)]      # noqa: E731
        # the tile loop is rotated (the epilogue may stand in front of the MFMA pass in the text): its instructions are everything from the
        # first of {first MFMA, first store} to the last of {last MFMA, last store}
        lo = min(at("v_mfma")[0], at("global_store_dwordx4")[0])
        hi = max(at("v_mfma")[-1], at("global_store_dwordx4")[-1])
        out[form] = dict(scratch=int(md.group(1)), vgprs=int(md.group(2)), spills=int(md.group(3)), lines=lines, tile=lines[lo:hi + 1],
                         n={op: len(at(op)) for op in OPS})
    return out


@pytest.fixture(scope="module")
def forms(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("no hipcc")
    return census(compile_isa(str(tmp_path_factory.mktemp("isa") / (SRC + ".s"))))


def test_the_forms_are_the_ones_the_host_selects(forms):
    assert set(forms) == FORMS, sorted(forms)


def test_no_form_spills_or_touches_scratch(forms):
    assert {f: (k["scratch"], k["spills"]) for f, k in forms.items()} == {f: (0, 0) for f in FORMS}
    assert not any(l.startswith("scratch_") for k in forms.values() for l in k["lines"])


def test_every_product_is_in_every_form(forms):
    assert {f: k["n"]["v_mfma_f32_32x32x16_f16"] for f, k in forms.items()} == {f: 286 if f[0] else 288 for f in FORMS}


def test_full_forms_store_unpredicated_and_a_fixed_number_of_times(forms):
    for f, k in forms.items():
        st = [i for i, l in enumerate(k["lines"]) if l.startswith("global_store_dwordx4")]
        between = [l for l in k["lines"][st[0]:st[-1]] if l.startswith(("s_and_saveexec_b64", "s_cbranch_execz"))]
        if f[3]:
            assert not between, (f, between)
            assert len(st) == (32 if f[2] == 2 else 16), (f, len(st))
            assert f"s_waitcnt vmcnt({len(st)})" in k["lines"], f      # the counted wait at the top of the tile loop leaves exactly these in flight
        else:
            assert len(st) == 48 and len(between) >= 47, (f, len(st), len(between))


def test_barriers_per_tile_follow_the_input_request_schedule(forms):
    """general form: top of the tile + behind the last MFMA; full-tile forms, UPS = 1: the top only (tile t + 1 goes to the other pair of input
    areas); UPS = 0: one more behind the chunk-0 MFMAs, where chunk 0 of tile t + 1 is requested"""
    assert {f: k["n"]["s_barrier"] for f, k in forms.items()} == {f: (3 - 2 * f[0]) if f[3] else 2 for f in FORMS}


def test_full_forms_carry_only_their_own_epilogue(forms):
    for f, k in forms.items():
        n = k["n"]
        if not f[3]:
            continue
        assert not n["v_cmp_nle_f32"] and not [l for l in k["tile"] if l.startswith("v_cndmask_b32")], f      # LeakyReLU is max(v, 0.2 v)
        assert n["v_cndmask_b32"] <= SETUP_SELECTS, (f, n["v_cndmask_b32"])
        assert n["v_max_f32"] == (128 if f[1] else 0), (f, n["v_max_f32"])
        if f[2] == 2:      # fp32 only: no 16-bit value is ever made
            assert not (n["v_cvt_pk_f16_f32"] or n["v_cvt_f16_f32"] or n["v_permlane32_swap"]), (f, n)
        else:
            assert n["v_permlane32_swap"] == 32 and 2 * n["v_cvt_pk_f16_f32"] + n["v_cvt_f16_f32"] == 128, (f, n)


def main():
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        fs = census(compile_isa(os.path.join(d, SRC + ".s")))
    print("ptail_kernel<UPS, LRELU, OUT, FULL> for gfx950: instructions per kernel (one tile pass + set-up), hipcc -O3")
    print("(LRELU 2 = run time; OUT 1 = 16-bit records, 2 = fp32 NHWC, 3 = run time; <u, 2, 3, 0> is the general form)")
    for f in sorted(fs, key=lambda f: (f[3], f)):
        k = fs[f]
        print(f"\n<{', '.join(map(str, f))}>  instructions {len(k['lines'])}  vgprs {k['vgprs']}  spilled {k['spills']}  scratch {k['scratch']} B")
        print("   " + "  ".join(f"{op} {c}" for op, c in k["n"].items()))
        print(f"   v_cndmask_b32 in the per-tile code: {sum(l.startswith('v_cndmask_b32') for l in k['tile'])}"
              f"   counted waits: {sorted(set(l for l in k['lines'] if l.startswith('s_waitcnt vmcnt')))}")


if __name__ == "__main__":
    sys.exit(main())
