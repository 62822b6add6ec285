"""CPU: the height-stage evaluation's fixture, its float64 restatement, the C ABI's argument checks and the loud failure of
srbh_amd.evaluate without a device.  No kernel is launched here (the kernel: tests/test_gpu_evaluate.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import evaluate_oracle as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOATS = ("loss", "rmse", "acc_total", "hm_stats", "oa", "iou", "mfwiou", "hm_each", "hm_balance", "hm_all")


@pytest.fixture(scope="module")
def g17(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g17_evaluate.npz")))


def fixture_tensors(g):
    return tuple(torch.from_numpy(g["in_" + k]) for k in ("height", "logits", "ref", "label"))


def test_fixture_is_small_and_complete(g17, golden_dir):
    size = os.path.getsize(os.path.join(golden_dir, "g17_evaluate.npz"))
    assert size < os.path.getsize(os.path.join(golden_dir, "g10_losses.npz")), size
    want = {"in_height", "in_logits", "in_ref", "in_label", "q_height", "cls_map"}
    want |= {f"rb{rb}_{k}" for rb in E.REF_BATCHES for k in FLOATS + ("cm", "hm_count")}
    assert set(g17) == want
    height, logits, ref, label = fixture_tensors(g17)
    assert tuple(logits.shape) == (10, 7, 24, 20) and tuple(height.shape) == tuple(ref.shape) == tuple(label.shape) == (10, 24, 20)
    assert height.dtype == logits.dtype == ref.dtype == torch.float32 and label.dtype == torch.uint8
    for got, want_t in zip(fixture_tensors(g17), E.fixture_inputs()):       # the seeded generator gives the stored inputs bit for bit
        assert torch.equal(got, want_t)
    classes = [set(np.unique(label[b].numpy()).tolist()) for b in range(10)]
    assert any(len(s) <= 5 for s in classes) and any(len(s) == 1 for s in classes)      # an image lacking two classes, a single-class image
    assert 0.015 <= E.tie_fraction(logits) <= 0.03                                        # exact ties in about 2 % of the pixels
    t10 = height * 10                                                                     # exact in fp32 for the half-way heights
    assert float(height.min()) < 0 and int(((t10 % 1) == 0.5).sum()) > 50
    assert {0.25, 0.75, 1.25} <= set(height[(t10 % 1) == 0.5].tolist())
    assert g17["q_height"].dtype == np.uint16 and g17["cls_map"].dtype == np.uint8


def test_oracle_helper_equals_the_reference_fixture(g17):
    """tests/evaluate_oracle.py (float64) against the imported reference's recorded results (fp32 differences and squares): confusion
    matrices exact, every float within 1e-5 relative, for the three loader batch sizes"""
    height, logits, ref, label = fixture_tensors(g17)
    worst = 0.0
    for rb in E.REF_BATCHES:
        got = E.evaluate(height, logits, ref, label, rb)
        got.update(E.derived(got["cm"], got["hm_stats"], got["hm_count"]))
        assert np.array_equal(got["cm"].numpy(), g17[f"rb{rb}_cm"]) and np.array_equal(got["hm_count"].numpy(), g17[f"rb{rb}_hm_count"])
        for k in FLOATS:
            scale = got["hm_stats"][:, 1:2].expand(-1, 3) if k == "hm_stats" else None
            err = E.rel_err(got[k], g17[f"rb{rb}_{k}"], scale=scale)
            worst = max(worst, err)
            assert err <= 1e-5, (rb, k, err)
    qh, cl = E.saved_maps(height, logits)
    assert np.array_equal(qh, g17["q_height"]) and np.array_equal(cl, g17["cls_map"])
    print(f"oracle helper vs reference fixture: worst relative gap = {worst:.2e}")


def test_image_sums_regroup_to_the_loop_results(g17):
    """the per-image sums the kernel returns are enough: regrouped into runs of ref_batch they give the loop's numbers (float64 rounding)"""
    height, logits, ref, label = fixture_tensors(g17)
    sums, cm = E.image_sums(height, logits, ref, label)
    assert torch.equal(sums[:, :, 3].sum(1), torch.full((10,), 480.0, dtype=torch.float64))
    for rb in E.REF_BATCHES:
        want = E.evaluate(height, logits, ref, label, rb)
        stats = torch.zeros(7, 3, dtype=torch.float64)
        rmse = 0.0
        for s in range(0, 10, rb):
            g = sums[s:s + rb].sum(0)
            n = g[:, 3]
            stats[:, 0] += torch.sqrt(g[:, 0] / n.clamp_min(1)) * n
            stats[:, 1] += g[:, 1]
            stats[:, 2] += g[:, 2]
            rmse += float(torch.sqrt(g[:, 0].sum() / n.sum())) * sums[s:s + rb].shape[0]
        assert E.rel_err(stats, want["hm_stats"], scale=want["hm_stats"][:, 1:2].expand(-1, 3)) <= 1e-12
        assert abs(rmse / 10 - float(want["rmse"])) <= 1e-12 * float(want["rmse"])
        assert torch.equal(cm.sum(0).double(), want["cm"])


def test_ref_batch_dependence_is_real(g17):
    a, b = g17["rb1_hm_stats"][:, 0], g17["rb4_hm_stats"][:, 0]
    assert np.all(np.abs(a - b) > 1e-3 * np.abs(a))                # every class's rmse * count moves with the loader's batch size
    assert abs(float(g17["rb1_rmse"]) - float(g17["rb4_rmse"])) > 1e-3
    assert np.allclose(g17["rb1_hm_stats"][:, 1:], g17["rb4_hm_stats"][:, 1:], rtol=1e-5)      # sum |d| and sum d do not
    assert np.array_equal(g17["rb1_cm"], g17["rb4_cm"])


def _header_fields(struct):
    hdr = open(os.path.join(ROOT, "include", "srbh.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        for part in decl.strip().split(","):
            if part.strip():
                names.append(re.findall(r"([A-Za-z_0-9]+)\s*$", part.strip())[0])
    return names


def test_eval_args_struct_matches_its_ctypes_mirror():
    from srbh_amd import _lib
    assert _header_fields("srbh_eval_args") == [n for n, _ in _lib.EvalArgs._fields_]
    kinds = dict(_lib.EvalArgs._fields_)
    assert all(kinds[n] is C.c_long for n in ("height_bs", "logits_bs", "logits_cs", "logits_ps"))
    assert all(kinds[n] is C.c_int for n in ("label_u8", "B", "C", "HW")) and kinds["ws_bytes"] is C.c_size_t
    assert all(kinds[n] is C.c_void_p for n in ("height", "logits", "ref", "label", "sums", "cm", "bad", "q_height", "cls_map", "ws"))
    hdr = open(os.path.join(ROOT, "include", "srbh.h")).read()
    block = hdr[hdr.index("Height-stage validation"):hdr.index("srbh_eval_sums(")]
    assert "train.py:315-344" in block and ":427-486 vtest_epoch2" in block and "metrics.py:186-200" in block      # the reference lines it serves


def _args(L, **over):
    from srbh_amd import _lib
    B, C_, HW = 2, 7, 480
    p = 4096       # never dereferenced
    kw = dict(height=p, height_bs=HW, logits=p, logits_bs=C_ * HW, logits_cs=HW, logits_ps=1, ref=p, label=p, label_u8=0, B=B, C=C_, HW=HW,
              sums=p, cm=p, bad=p, q_height=None, cls_map=None, ws=p, ws_bytes=L.srbh_eval_ws_bytes(B, HW, C_))
    kw.update(over)
    if "ws_bytes" not in over and ("B" in over or "C" in over or "HW" in over):
        kw["ws_bytes"] = 1 << 30
    return _lib.EvalArgs(**kw)


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """nothing reaches a device: every call returns SRBH_ERR_ARG (-1) first"""
    from srbh_amd import _lib
    _lib.build()
    L = _lib.lib()
    ERR_ARG = -1
    assert L.srbh_eval_sums(None, None) == ERR_ARG
    for name in ("height", "logits", "ref", "label", "sums", "cm", "bad", "ws"):
        assert L.srbh_eval_sums(C.byref(_args(L, **{name: None})), None) == ERR_ARG, name
    for bad in (dict(C=1), dict(C=17), dict(C=0), dict(B=0), dict(B=-3), dict(HW=0), dict(HW=-480), dict(B=65536),
                dict(height_bs=-480), dict(logits_ps=-1), dict(logits_cs=-1), dict(logits_bs=-1)):
        assert L.srbh_eval_sums(C.byref(_args(L, **bad)), None) == ERR_ARG, bad
    need = L.srbh_eval_ws_bytes(2, 480, 7)
    assert L.srbh_eval_sums(C.byref(_args(L, ws_bytes=need - 1)), None) == ERR_ARG          # a short workspace
    assert L.srbh_eval_sums(C.byref(_args(L, ws_bytes=0)), None) == ERR_ARG
    assert b"srbh_eval_sums" in L.srbh_last_error()


def test_workspace_query():
    from srbh_amd import _lib
    _lib.build()
    L = _lib.lib()
    # one slot per 4096 pixels and image: C x 3 doubles and C x C counts
    assert L.srbh_eval_ws_bytes(1, 5, 7) == 7 * 3 * 8 + 49 * 4
    assert L.srbh_eval_ws_bytes(3, 2240, 7) == 3 * (7 * 3 * 8 + 49 * 4)
    assert L.srbh_eval_ws_bytes(2, 65536, 16) == 2 * 16 * (16 * 3 * 8 + 256 * 4)
    assert L.srbh_eval_ws_bytes(1, 4096, 2) == 2 * 3 * 8 + 4 * 4 and L.srbh_eval_ws_bytes(1, 4097, 2) == 2 * (2 * 3 * 8 + 4 * 4)
    sizes = [L.srbh_eval_ws_bytes(b, 65536, 7) for b in range(1, 66)]
    assert sizes[0] > 0 and all(y > x for x, y in zip(sizes, sizes[1:]))                     # positive, monotone in B
    assert L.srbh_eval_ws_bytes(0, 65536, 7) == 0 and L.srbh_eval_ws_bytes(-1, 65536, 7) == 0
    assert L.srbh_eval_ws_bytes(1, 0, 7) == 0 and L.srbh_eval_ws_bytes(1, 480, 1) == 0 and L.srbh_eval_ws_bytes(1, 480, 17) == 0


def test_cpu_tensors_raise_and_bad_shapes_raise_value_error(g17):
    from srbh_amd import evaluate, harness
    from srbh_amd.metrics import HeightMetric, SegmentationMetric
    height, logits, ref, label = fixture_tensors(g17)
    ev = evaluate.HeightEvaluation(num_class=7, device="cpu")
    with pytest.raises(RuntimeError, match="GPU only"):
        ev.add(height, logits, ref, label)
    with pytest.raises(RuntimeError, match="GPU only"):
        ev.add(height[:, None], logits, ref, label.long())
    with pytest.raises(ValueError):
        ev.add(height, logits[:, :6], ref, label)                  # not num_class channels
    with pytest.raises(ValueError):
        ev.add(height, logits, ref[:, :20], label)
    with pytest.raises(ValueError):
        ev.add(height[:, None].expand(-1, 2, -1, -1), logits, ref, label)
    with pytest.raises(ValueError):
        evaluate.HeightEvaluation(num_class=17)
    with pytest.raises(ValueError):
        evaluate.HeightEvaluation(ref_batch=0)
    res = ev.result()
    assert res["count"] == 0 and ev.count == 0
    assert isinstance(res["seg"], SegmentationMetric) and isinstance(res["height"], HeightMetric)
    assert callable(harness.evaluate_tiles) and callable(ev.merge_)
