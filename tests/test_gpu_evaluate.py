"""GPU: the height-stage evaluation kernel (csrc/srbh_eval.hip) against the float64 oracle tests/evaluate_oracle.py, its reproducibility,
HeightEvaluation.result() against the reference fixture and the existing metric classes, and harness.evaluate_tiles.

Bounds.  Kernel and oracle both accumulate float64 values of exactly the same terms (the fp32 inputs cast to double; d, d^2 and |d| are then
the same doubles on both sides), only the ORDER of the additions differs.  A sum of n non-negative terms in any order carries a relative
error of at most (n - 1) 2^-53, so two orders differ by at most 2 n 2^-53: 1e-12 up to n = 4 096 (the small shapes), 2e-12 at the 5 184 pixels of
72 x 72 (2 n 2^-53 = 1.2e-12; its last image is one class) and 2e-11 at n = 65 536 (256 x 256).  sum d cancels, so its gap is bounded relative to sum |d|.  Counts, the confusion matrix and the
two maps are integers: exact."""
import os

import numpy as np
import pytest
import torch

from oracle import synth
from tests import evaluate_oracle as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make_case(B, H, W, C, seed):
    """seeded head outputs with the content the kernel can go wrong on: image 0 lacks class C - 1, the last image of a batch (B > 1) is one
    class only, ~2 % exact ties, NaN logits in a handful of pixels (first channel, two channels, all channels), negative and half-way heights"""
    rs = np.random.RandomState(seed)
    bh, bw = max(1, H // 4), max(1, W // 4)
    coarse = rs.randint(0, C, size=(B, bh, bw))
    label = np.kron(coarse, np.ones((4, 4), dtype=np.int64))[:, :H, :W]
    if label.shape[1] < H or label.shape[2] < W:
        label = np.pad(label, ((0, 0), (0, H - label.shape[1]), (0, W - label.shape[2])), mode="edge")
    if H * W > C:
        label[0][label[0] == C - 1] = 0
    if B > 1:
        label[B - 1] = C // 2
    ref = (rs.randint(0, 40, size=(B, H, W)) * (label > 0)).astype(np.float32)
    height = (ref + rs.randn(B, H, W) * 3.0).astype(np.float32)
    halves = np.array([0.25, 0.75, 1.25, 1.75, 2.25, 6.25, 12.75], dtype=np.float32)
    pick = rs.rand(B, H, W) < 0.03
    height[pick] = halves[rs.randint(0, len(halves), size=int(pick.sum()))]
    height.reshape(-1)[:3] = (0.25, -0.75, 1.25)[:min(3, height.size)]
    logits = (rs.randn(B, C, H, W) * 2.0).astype(np.float32)
    tie = rs.rand(B, H, W) < 0.02
    tie.reshape(-1)[min(4, tie.size - 1)] = True
    other = rs.randint(0, C, size=(B, H, W))
    mx = logits.max(1)
    for b, r, c in zip(*np.nonzero(tie)):
        logits[b, other[b, r, c], r, c] = mx[b, r, c]
    flat = logits.reshape(B, C, H * W)
    n = H * W
    flat[0, 0, n // 2] = np.nan                       # the first channel
    flat[B - 1, C - 1, n // 3] = np.nan               # the last channel
    flat[0, 1:3 if C > 2 else 2, n - 1] = np.nan      # two channels: the first NaN wins
    flat[B - 1, :, 0] = np.nan                        # every channel
    flat[0, C - 1, 1 % n] = np.inf
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))      # noqa: E731
    return t(height), t(logits), t(ref), t(label)


CASES = {"b3_40x56_c7": (3, 40, 56, 7, 171), "b1_1x5_c7": (1, 1, 5, 7, 172), "b2_256x256_c7": (2, 256, 256, 7, 173),
         "b2_72x72_c7": (2, 72, 72, 7, 176),      # 5 184 pixels: two workgroups per image, the second with one full round and 64 pixels of the next
         "b3_40x56_c2": (3, 40, 56, 2, 174), "b3_40x56_c16": (3, 40, 56, 16, 175),
         "b3_40x56_c8": (3, 40, 56, 8, 177)}      # (the kernel is instantiated for C <= 7, C == 8 and C <= 16)
_cache = {}


def case(name):
    """(inputs on the CPU, oracle results): computed once per module, never modified"""
    if name not in _cache:
        B, H, W, C, seed = CASES[name]
        inp = make_case(B, H, W, C, seed)
        sums, cm = E.image_sums(*inp, num_class=C)
        qh, cl = E.saved_maps(inp[0], inp[1])
        _cache[name] = (inp, {"sums": sums, "cm": cm, "q_height": qh, "cls_map": cl})
    return _cache[name]


def same_maps(a, b):
    """torch.equal of two (uint16, uint8) pairs (the 16-bit map compared through its int16 view)"""
    return torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and torch.equal(a[1], b[1])


def strided_height(height):
    """the (B,1,H,W) tensor as a NON-contiguous batch slice (every second image of a buffer twice as long)"""
    B, H, W = height.shape
    big = torch.full((2 * B, 1, H, W), float("nan"), device=DEV)
    big[::2, 0] = height.to(DEV)
    v = big[::2]
    assert B == 1 or not v.is_contiguous()
    return v


def run(inp, C, layout="nchw", label_dtype=torch.int64, height4d=True, keep_maps=True):
    from srbh_amd.evaluate import HeightEvaluation
    height, logits, ref, label = inp
    lg = logits.to(DEV)
    if layout == "channels_last":
        lg = lg.contiguous(memory_format=torch.channels_last)
    ev = HeightEvaluation(num_class=C, device=DEV, keep_maps=keep_maps)
    maps = ev.add(strided_height(height) if height4d else height.to(DEV), lg, ref.to(DEV), label.to(DEV).to(label_dtype))
    sums, cm = ev.image_sums()
    return ev, sums, cm, maps


def check_against_oracle(sums, cm, maps, want, tol, tag):
    assert sums.dtype == torch.float64 and cm.dtype == torch.int64
    sums, cm = sums.cpu(), cm.cpu()
    assert torch.equal(cm, want["cm"]), tag
    assert torch.equal(sums[:, :, 3], want["sums"][:, :, 3]), tag                       # counts
    e2 = E.rel_err(sums[:, :, 0], want["sums"][:, :, 0])
    e1 = E.rel_err(sums[:, :, 1], want["sums"][:, :, 1])
    e0 = E.rel_err(sums[:, :, 2], want["sums"][:, :, 2], scale=want["sums"][:, :, 1])
    print(f"{tag}: sum d^2 {e2:.2e}  sum |d| {e1:.2e}  sum d / sum |d| {e0:.2e}  (bound {tol:.0e})")
    assert e2 <= tol and e1 <= tol and e0 <= tol, (tag, e2, e1, e0)
    if maps is not None:
        qh, cl = maps
        assert qh.dtype == torch.uint16 and cl.dtype == torch.uint8
        assert np.array_equal(qh.cpu().numpy(), want["q_height"]), tag
        assert np.array_equal(cl.cpu().numpy(), want["cls_map"]), tag


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_matches_the_float64_oracle_in_every_layout(name):
    inp, want = case(name)
    C = CASES[name][3]
    tol = 2e-11 if "256x256" in name else 2e-12 if "72x72" in name else 1e-12
    assert torch.equal(torch.from_numpy(want["cls_map"]).long(), inp[1].argmax(1))      # the expected argmax IS torch.argmax on the CPU (NaN, ties)
    assert int(torch.isnan(inp[1]).sum()) >= 4 and E.tie_fraction(torch.nan_to_num(inp[1], nan=-1e30)) > 0
    results = []
    for layout, ldt, h4 in (("nchw", torch.int64, True), ("channels_last", torch.uint8, True), ("channels_last", torch.int64, False),
                            ("nchw", torch.uint8, False)):
        _, sums, cm, maps = run(inp, C, layout, ldt, h4)
        check_against_oracle(sums, cm, maps, want, tol, f"{name} {layout} {str(ldt)[6:]} {'B1HW' if h4 else 'BHW'}")
        results.append((sums, cm, maps))
    for sums, cm, maps in results[1:]:          # either logits layout, label type and height view: the same bits
        assert torch.equal(sums, results[0][0]) and torch.equal(cm, results[0][1])
        assert same_maps(maps, results[0][2])


def test_absent_and_single_classes_leave_exact_zeros():
    inp, want = case("b3_40x56_c7")
    _, sums, cm, _ = run(inp, 7)
    assert float(want["sums"][0, 6].abs().sum()) == 0.0 and torch.equal(sums[0, 6].cpu(), torch.zeros(4, dtype=torch.float64))
    assert int((sums[2, :, 3] > 0).sum()) == 1 and float(sums[2, 3, 3]) == 40 * 56
    assert int(cm[0, 6].sum()) == 0


@pytest.mark.parametrize("name", ["b3_40x56_c7", "b2_72x72_c7", "b2_256x256_c7"])
def test_results_are_bit_reproducible_and_independent_of_the_batch(name):
    inp, _ = case(name)
    C = CASES[name][3]
    _, s1, c1, m1 = run(inp, C)
    _, s2, c2, m2 = run(inp, C)
    assert torch.equal(s1, s2) and torch.equal(c1, c2) and same_maps(m1, m2)      # run to run
    for b in range(inp[0].shape[0]):                                                                                  # alone == inside the batch
        one = tuple(t[b:b + 1] for t in inp)
        _, sb, cb, mb = run(one, C, layout="channels_last" if b & 1 else "nchw")
        assert torch.equal(sb[0], s1[b]) and torch.equal(cb[0], c1[b]), (name, b)
        assert same_maps((mb[0][0], mb[1][0]), (m1[0][b], m1[1][b]))
    # a batch in another order / of another size: still the same rows
    perm = list(reversed(range(inp[0].shape[0])))
    _, sp, cp, _ = run(tuple(t[perm] for t in inp), C)
    assert torch.equal(sp, s1[perm]) and torch.equal(cp, c1[perm])


def test_out_of_range_labels_set_the_flag_and_are_counted_nowhere():
    inp, _ = case("b3_40x56_c7")
    height, logits, ref, label = inp
    label = label.clone()
    label[1, 7, 9] = 7            # == C
    label[2, 39, 55] = -1
    want_sums, want_cm = E.image_sums(height, logits, ref, label, num_class=7)      # the oracle leaves the two pixels out
    assert int(want_cm.sum()) == 3 * 40 * 56 - 2
    ev, sums, cm, _ = run((height, logits, ref, label), 7)
    assert torch.equal(cm.cpu(), want_cm) and torch.equal(sums[:, :, 3].cpu(), want_sums[:, :, 3])
    assert E.rel_err(sums[:, :, :2], want_sums[:, :, :2]) <= 1e-12
    assert E.rel_err(sums[:, :, 2], want_sums[:, :, 2], scale=want_sums[:, :, 1]) <= 1e-12
    with pytest.raises(ValueError, match=r"outside \[0, 7\)"):
        ev.result()
    # the flag is sticky over later clean batches, and a clean evaluation does not raise
    clean = case("b3_40x56_c7")[0]
    ev.add(clean[0].to(DEV), clean[1].to(DEV), clean[2].to(DEV), clean[3].to(DEV))
    with pytest.raises(ValueError):
        ev.result()
    ok, *_ = run(clean, 7)
    assert ok.result()["count"] == 3
    # uint8 labels: 7 is out of range as well
    ev8, *_ = run((height, logits, ref, label.clamp_min(0)), 7, label_dtype=torch.uint8)
    with pytest.raises(ValueError):
        ev8.result()


@pytest.fixture(scope="module")
def g17(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g17_evaluate.npz")))


@pytest.mark.parametrize("rb", E.REF_BATCHES)
@pytest.mark.parametrize("add_batch", [10, 4])
def test_result_matches_the_reference_fixture_and_the_existing_metric_classes(g17, rb, add_batch):
    """the g17 inputs on the device, added in batches of `add_batch` (whatever the device loop ran with), regrouped into the reference
    loader's batches of rb: the fixture's numbers (1e-5 on floats: the reference works in fp32; matrix exact) and those of the existing
    SegmentationMetric / HeightMetric fed group by group (confusion exact; height statistics 1e-9: their float atomics have no order)"""
    from srbh_amd.evaluate import HeightEvaluation
    from srbh_amd.metrics import HeightMetric, SegmentationMetric
    height, logits, ref, label = (torch.from_numpy(g17["in_" + k]).to(DEV) for k in ("height", "logits", "ref", "label"))
    ev = HeightEvaluation(num_class=7, device=DEV, ref_batch=rb)
    for s in range(0, 10, add_batch):
        ev.add(height[s:s + add_batch, None], logits[s:s + add_batch], ref[s:s + add_batch], label[s:s + add_batch])
    res = ev.result()
    assert res["count"] == 10
    seg, hm = res["seg"], res["height"]
    got = {"loss": res["loss"], "rmse": res["rmse"], "acc_total": res["acc_total"], "hm_stats": hm.stats, "oa": seg.OverallAccuracy(),
           "iou": seg.IntersectionOverUnion(), "mfwiou": seg.mFWIoU(), "hm_each": hm.getAvgEach(), "hm_balance": hm.getAvgBalance(),
           "hm_all": hm.getAvgAll()}
    assert np.array_equal(seg.getConfusionMatrix().cpu().numpy(), g17[f"rb{rb}_cm"])
    assert np.array_equal(hm.getCount().cpu().numpy(), g17[f"rb{rb}_hm_count"])
    worst = 0.0
    for k, v in got.items():
        assert v.dtype == torch.float64 and v.is_cuda, k
        scale = torch.from_numpy(g17[f"rb{rb}_hm_stats"][:, 1:2]).expand(-1, 3) if k == "hm_stats" else None
        err = E.rel_err(v, g17[f"rb{rb}_{k}"], scale=scale)
        worst = max(worst, err)
        assert err <= 1e-5, (rb, k, err)
    seg2, hm2 = SegmentationMetric(7, device=DEV), HeightMetric(7, device=DEV)
    for s in range(0, 10, rb):
        seg2.addBatch(logits[s:s + rb].argmax(1), label[s:s + rb])
        hm2.addBatch(height[s:s + rb], ref[s:s + rb], label[s:s + rb])
    assert torch.equal(seg.getConfusionMatrix(), seg2.getConfusionMatrix()) and torch.equal(hm.count, hm2.count)
    e_old = E.rel_err(hm.stats, hm2.stats, scale=hm2.stats[:, 1:2].expand(-1, 3))
    print(f"ref_batch {rb}, added by {add_batch}: vs fixture {worst:.2e} (bound 1e-5), vs existing HeightMetric {e_old:.2e} (bound 1e-9)")
    assert e_old <= 1e-9
    # every ref_batch from the same per-image sums
    assert E.rel_err(ev.result(ref_batch=1)["rmse"], g17["rb1_rmse"]) <= 1e-5


def test_merge_appends_in_order_and_keeps_the_flag(g17):
    from srbh_amd.evaluate import HeightEvaluation
    height, logits, ref, label = (torch.from_numpy(g17["in_" + k]).to(DEV) for k in ("height", "logits", "ref", "label"))
    whole = HeightEvaluation(7, DEV, ref_batch=3)
    whole.add(height, logits, ref, label)
    a, b = HeightEvaluation(7, DEV, ref_batch=3), HeightEvaluation(7, DEV, ref_batch=3)
    a.add(height[:5], logits[:5], ref[:5], label[:5])
    b.add(height[5:], logits[5:], ref[5:], label[5:])
    assert a.merge_(b) is a and a.count == 10
    ra, rw = a.result(), whole.result()
    for k in ("loss", "rmse", "acc_total"):
        assert torch.equal(ra[k], rw[k]), k
    assert torch.equal(ra["height"].stats, rw["height"].stats) and torch.equal(ra["seg"].confusionMatrix, rw["seg"].confusionMatrix)
    c = HeightEvaluation(7, DEV)
    c.add(height[:1], logits[:1], ref[:1], label[:1].long() + 7)
    with pytest.raises(ValueError):
        a.merge_(c).result()


# ---- harness.evaluate_tiles ----------------------------------------------------------------------------------------------------------
def _labels(n, seed):
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randint(0, 7, (n, 32, 32), generator=g)
    label = coarse.repeat_interleave(8, 1).repeat_interleave(8, 2)
    ref = (torch.randint(0, 60, (n, 256, 256), generator=g) * (label > 0)).float()
    return ref, label


def test_evaluate_tiles_scores_the_tiles_through_the_predict_graph():
    """10 tiles at batch 4: two replays of predict_tiles' graph and a zero-padded tail of two.  Expected values: the same forward run by hand,
    batch by batch, its outputs copied to the CPU and given to the float64 oracle."""
    from srbh_amd import harness
    from srbh_amd.mosaic import Mosaic
    from srbh_amd.rrdbnet import RRDBNet
    from tests.test_gpu_model import make_model
    net_hr = RRDBNet(3, 3, num_block=2)
    net_hr.load_state_dict(synth.rrdbnet_state_dict(num_block=2, seed=4, mode="stress"))
    net_hr = net_hr.to(DEV).eval()
    model = make_model(seed=12, isaggre=False).to(DEV).eval()
    tiles = synth.tiles(10, 8, 64, seed=23).to(DEV)
    ref, label = _labels(10, 29)
    ref, label = ref.to(DEV), label.to(DEV)
    pos = [[(i % 4) * 48, (i // 4) * 48, 64, 64] for i in range(10)]
    Hh, Ww = 4 * (48 * 2 + 64), 4 * (48 * 3 + 64)

    def mosaic_heights():
        m = Mosaic(Hh, Ww, 7, DEV)
        assert harness.predict_tiles(net_hr, model, tiles, pos, m, batch=4) == 10
        return m.finalize()[0].int()

    before = mosaic_heights()
    pg = model.__dict__["_srbh_predict_graph"]
    assert pg is not None

    hs, ls = [], []
    with torch.no_grad():
        for s in range(0, 10, 4):
            x = tiles[s:s + 4]
            k = x.shape[0]
            if k < 4:
                x = torch.cat([x, x.new_zeros((4 - k,) + tuple(x.shape[1:]))], 0)
            out = model(x, harness.features_for_head(net_hr, x[:, :3], model=model))
            hs.append(out[0][:k].float().cpu())
            ls.append(out[1][:k].float().cpu())
    height, logits = torch.cat(hs), torch.cat(ls).contiguous()
    want_sums, want_cm = E.image_sums(height, logits, ref.cpu(), label.cpu())

    ev = harness.evaluate_tiles(net_hr, model, tiles, ref, label, batch=4, ref_batch=4)
    assert model.__dict__["_srbh_predict_graph"] is pg                     # the graph predict_tiles captured, not a second one
    assert ev.count == 10
    sums, cm = ev.image_sums()
    pix = float((cm.cpu() != want_cm).sum())
    e = [E.rel_err(sums[:, :, j].cpu(), want_sums[:, :, j], scale=want_sums[:, :, 1] if j == 2 else None) for j in range(3)]
    print(f"evaluate_tiles vs hand-run forward + oracle: confusion entries that differ {pix:.0f}, sums {e[0]:.2e} {e[1]:.2e} {e[2]:.2e} (bound 2e-11)")
    assert torch.equal(cm.cpu(), want_cm)
    assert torch.equal(sums[:, :, 3].cpu(), want_sums[:, :, 3]) and max(e) <= 2e-11
    for rb in (1, 4):
        res, want = ev.result(ref_batch=rb), E.evaluate(height, logits, ref.cpu(), label.cpu(), rb)
        assert res["count"] == 10 and torch.equal(res["seg"].getConfusionMatrix().cpu(), want["cm"])
        for k, v in (("loss", res["loss"]), ("rmse", res["rmse"]), ("acc_total", res["acc_total"]), ("hm_stats", res["height"].stats)):
            assert E.rel_err(v, want[k], scale=want["hm_stats"][:, 1:2].expand(-1, 3) if k == "hm_stats" else None) <= 2e-11, (rb, k)
        assert torch.equal(res["height"].count.cpu(), want["hm_count"])

    again = harness.evaluate_tiles(net_hr, model, tiles, ref, label, batch=4, ref_batch=4)
    assert model.__dict__["_srbh_predict_graph"] is pg
    s2, c2 = again.image_sums()
    assert torch.equal(s2, sums) and torch.equal(c2, cm)                   # equal bits

    assert torch.equal(mosaic_heights(), before)                           # predict_tiles on the shared graph is undisturbed
    assert model.__dict__["_srbh_predict_graph"] is pg

    a = harness.evaluate_tiles(net_hr, model, tiles, ref, label, batch=4, ref_batch=4, rank=0, world=2)
    b = harness.evaluate_tiles(net_hr, model, tiles, ref, label, batch=4, ref_batch=4, rank=1, world=2)
    assert a.count == 5 and b.count == 5
    sm, cmm = a.merge_(b).image_sums()
    assert torch.equal(sm, sums) and torch.equal(cmm, cm)                  # sharded + merged == unsharded, exactly

    km = harness.evaluate_tiles(net_hr, model, tiles, ref, label, batch=4, keep_maps=True)
    assert len(km.maps) == 3 and tuple(km.maps[2][0].shape) == (2, 256, 256) and km.maps[0][1].dtype == torch.uint8
