"""GPU: the training augmentation kernels (srbh_aug_image, srbh_aug_label_prep) and their Python entries against the numpy oracle
tests/augment_oracle.py (float64 values, integer indices) and, for the labels, against the parent's own srbh_label_prep.

The image bound: every element within 2^-21 (S + |min_c|) / range_c of the float64 oracle, S the same bilinear combination of |raw|
(2^-21 S without normalisation).  First order, four products, three additions, one subtraction and one division are 6 x 2^-24;
rounded up to 8 x 2^-24 = 2^-21 for fused-multiply-add differences.  All elements are compared."""
import os

import numpy as np
import pytest
import torch

from srbh_amd import _lib
from srbh_amd import loader_math as LM
from tests import augment_oracle as AO
from tests.gpu_util import GuardedBuffers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HIR = (0, 3, 12, 21, 30, 60, 90, 256)
I = (0, 1, 2, 3)
SRBH_ERR_ARG = -1

# (flip code, perm, angle or None = not rotated): the identity, every step alone, three rows with all three at once
TABLE = ([(0, I, None)] + [(f, I, None) for f in (1, 2, 3)] + [(0, p, None) for p in ((1, 0, 3, 2), (1, 2, 0, 3), (3, 2, 1, 0))]
         + [(0, I, a) for a in (90.0, -90.0, 45.0, 1e-3, 30.0, -77.7)]
         + [(1, (1, 2, 0, 3), 30.0), (2, (3, 0, 1, 2), -77.7), (3, (2, 3, 1, 0), 61.25)])
B = 12
BATCHES = (slice(0, 12), slice(4, 16))                 # the sixteen rows in batches of B = 12
# 8 x 48 is beyond the issue's list: a quarter turn of it samples 20 px outside an axis of 8, where one reflection does not fold back
SMALL_GRIDS = ((16, 24), (32, 32), (40, 24), (8, 48))
MINS = np.linspace(-100, 50, 8)
MAXS = MINS + np.linspace(1500, 2600, 8)


def _params(rows):
    return LM.AugmentParams([r[0] for r in rows], [r[1] for r in rows], [0.0 if r[2] is None else r[2] for r in rows],
                            [r[2] is not None for r in rows])


@pytest.fixture(scope="module")
def g9(golden_dir):
    g = np.load(os.path.join(golden_dir, "g9_hierweight.npz"))
    return g["stats"], LM.hierweight(g["stats"], HIR)


def _labels(stats, n, H, W, seed):
    gen = torch.Generator()
    gen.manual_seed(seed)
    p = torch.from_numpy(stats / stats.sum())
    return torch.multinomial(p, n * H * W, replacement=True, generator=gen).reshape(n, H, W).to(torch.uint8)


def _bands(n, C, H, W, seed):
    gen = torch.Generator()
    gen.manual_seed(seed)
    return torch.rand(n, C, H, W, generator=gen) * 3000 - 200


def _label_prep_call(lab_dev, dp, prep, label_out=True):
    n, H, W = lab_dev.shape
    build = torch.empty((n, H, W), dtype=torch.int64, device=DEV)
    hf, wt = torch.empty((n, H, W), device=DEV), torch.empty((n, H, W), device=DEV)
    ha, wa = torch.empty((n, H // 4, W // 4), device=DEV), torch.empty((n, H // 4, W // 4), device=DEV)
    out = torch.empty((n, H, W), dtype=torch.uint8, device=DEV) if label_out else None
    _lib.check(_lib.lib().srbh_aug_label_prep(lab_dev.data_ptr(), n, H, W, dp.flip.data_ptr(), dp.perm.data_ptr(), dp.tables.data_ptr(),
                                              prep.lut.data_ptr(), prep.cw.data_ptr(), build.data_ptr(), hf.data_ptr(), wt.data_ptr(),
                                              ha.data_ptr(), wa.data_ptr(), None if out is None else out.data_ptr(), _lib.stream_ptr()),
               "aug_label_prep")
    return out, (hf, ha, build, wt, wa)


@pytest.mark.parametrize("grid", SMALL_GRIDS + ((256, 256),), ids=lambda g: f"{g[0]}x{g[1]}")
def test_labels_equal_the_oracle_and_the_parents_kernel(g9, grid):
    stats, hw = g9
    H, W = grid
    prep = LM.LabelPrep(HIR, hw, DEV)
    lab_all = _labels(stats, len(TABLE), H, W, seed=H * 1000 + W)
    for rows in (BATCHES if H < 256 else BATCHES[1:]):
        lab = lab_all[rows]
        dp = LM.Augment().to_device(_params(TABLE[rows]), H, W, DEV)
        out, got = _label_prep_call(lab.to(DEV), dp, prep)
        again, _ = _label_prep_call(lab.to(DEV), dp, prep)
        assert torch.equal(out, again)
        # second witness: the parent's kernel on the augmented label, all five outputs bit for bit
        for a, b, name in zip(got, prep(out), ("height", "height_aggre", "build", "weight", "weight_aggre")):
            assert torch.equal(a, b), name
        hf, ha, build, wt, wa = (t.cpu() for t in got)
        for i, (f, p, ang) in enumerate(TABLE[rows]):
            want_lab, (oh, oha, ob, ow, owa) = AO.aug_label_prep(lab[i].numpy(), f, p, ang, HIR, hw)
            assert np.array_equal(out[i].cpu().numpy(), want_lab), (i, f, p, ang)
            assert torch.equal(hf[i], oh) and torch.equal(build[i], ob) and torch.equal(wt[i], ow), (i, f, p, ang)
            assert torch.allclose(ha[i], oha.reshape(ha[i].shape), rtol=1e-6, atol=1e-6)
            # class of the aggregated height may flip only where the mean sits on an integer boundary (sum-order noise)
            assert float((wa[i] != owa.reshape(wa[i].shape)).float().mean()) < 1e-3
        if rows == BATCHES[-1]:           # the optional label_out left out: the other outputs do not change
            _, bare = _label_prep_call(lab.to(DEV), dp, prep, label_out=False)
            assert all(torch.equal(a, b) for a, b in zip(got, bare))


def _aug_image_call(x_dev, up, step, dp, norm, clip):
    return LM._aug_image(x_dev, up, step, dp, dp.consts[0] if norm else None, dp.consts[1] if norm else None, (0, 1) if clip else None,
                         "aug_image")


MODES = ((False, False), (True, False), (True, True))             # (normalise, clip)


def _check_images(H, W, C, batches, cases):
    """cases: (up, step, normalise, clip)"""
    mn, mx = MINS[:C], MAXS[:C]
    mn32, rg32 = mn.astype(np.float32), (mx - mn).astype(np.float32)
    worst = 0.0
    for up, step, norm, clip in cases:
        raw_all = _bands(len(TABLE), C, H // up, W // up, seed=H * 1000 + W + up)
        for rows in batches:
            raw = raw_all[rows]
            dp = LM.Augment().to_device(_params(TABLE[rows]), H, W, DEV, (mn32, rg32))
            got = _aug_image_call(raw.to(DEV), up, step, dp, norm, clip).cpu().numpy()
            assert got.shape == (B, C, H // step, W // step) and got.dtype == np.float32
            for i, (f, p, ang) in enumerate(TABLE[rows]):
                want, scale = AO.aug_image(raw[i].numpy(), up, step, f, p, ang, mn32 if norm else None, rg32 if norm else None,
                                           (0, 1) if clip else None)
                err = np.abs(got[i].astype(np.float64) - want)
                bound = 2.0 ** -21 * scale
                worst = max(worst, float((err / bound).max()))
                assert np.all(err <= bound), (up, step, norm, clip, i, f, p, ang, float((err / bound).max()))
            if clip:
                assert got.min() >= 0.0 and got.max() <= 1.0
    print(f"{H}x{W} C={C}: worst error / bound = {worst:.3f}")


FORMS = ((4, 4), (1, 1), (4, 1))


@pytest.mark.parametrize("C", (1, 3, 8))
@pytest.mark.parametrize("grid", SMALL_GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_images_within_rounding_of_the_float64_oracle(grid, C):
    _check_images(grid[0], grid[1], C, BATCHES, [(up, step, norm, clip) for up, step in FORMS for norm, clip in MODES])


def test_images_at_the_reference_size():
    """256 x 256, 8 bands, the rows of the table from the perms on (every rotation and the three combined rows): each form once, in the
    mode the loader uses it in (the small grids above run every form in every mode)"""
    _check_images(256, 256, 8, BATCHES[1:], ((4, 4, True, True), (1, 1, True, False), (4, 1, False, False)))


def test_identity_parameters_are_todays_prep_bit_for_bit(g9, golden_dir):
    stats, hw = g9
    prep = LM.LabelPrep(HIR, hw, DEV)
    raw = _bands(B, 8, 64, 64, seed=11).to(DEV)
    lab = _labels(stats, B, 256, 256, seed=12).to(DEV)
    for datarange in ((0, 1), None):
        got = LM.train_batch(raw, lab, MINS, MAXS, prep, params=None, datarange=datarange)
        want = (LM.normalize_tiles(raw, MINS, MAXS, datarange),) + tuple(prep(lab))
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    # explicit identity parameters, and a rotation by 0 degrees, are the same batch
    want = LM.train_batch(raw, lab, MINS, MAXS, prep)
    for p in (LM.AugmentParams.identity(B), LM.AugmentParams([0] * B, [I] * B, [0.0] * B, [True] * B)):
        assert all(torch.equal(a, b) for a, b in zip(LM.train_batch(raw, lab, MINS, MAXS, prep, params=p), want))
    # the g13 fixture: the reference dataset's own outputs for its un-augmented samples
    g = np.load(os.path.join(golden_dir, "g13_loader.npz"))
    n = g["s2"].shape[0]
    raw = torch.from_numpy(np.concatenate([g["s2"], g["s1"]], axis=-1)).permute(0, 3, 1, 2).contiguous().to(DEV)
    h8 = torch.from_numpy(g["height_u8"]).to(DEV)
    prep = LM.LabelPrep(HIR, g["heightweight"], DEV)
    got = LM.train_batch(raw, h8, g["mins"], g["maxs"], prep)
    want = (LM.normalize_tiles(raw, g["mins"], g["maxs"], (0, 1)),) + tuple(prep(h8))
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    lr, hf, ha, build, wt, wa = (t.cpu().numpy() for t in got)
    for i in range(n):
        assert np.allclose(lr[i], g[f"img{i}"], rtol=1e-6, atol=1e-7)
        assert np.array_equal(build[i], g[f"build{i}"]) and np.array_equal(wt[i], g[f"weight{i}"])
        assert np.allclose(ha[i], g[f"height_aggre{i}"], rtol=1e-6, atol=1e-6)
        assert float((wa[i] != g[f"weight_aggre{i}"]).mean()) < 1e-2


def test_train_batch_is_what_the_training_step_consumes(g9):
    from srbh_amd import harness
    stats, hw = g9
    prep = LM.LabelPrep(HIR, hw, DEV)
    gen = torch.Generator()
    gen.manual_seed(3)
    params = LM.Augment().draw(B, gen)
    raw = _bands(B, 8, 64, 64, seed=21)
    lab = _labels(stats, B, 256, 256, seed=22)
    got = LM.train_batch(raw.to(DEV), lab.to(DEV), MINS, MAXS, prep, params)
    dgen = torch.Generator(device=DEV)
    dgen.manual_seed(3)
    model = harness.synthetic_batch_device(B, dgen, DEV)
    assert len(got) == len(model) == 6
    for a, b in zip(got, model):
        assert a.shape == b.shape and a.dtype == b.dtype and a.stride() == b.stride() and a.device == b.device and a.is_contiguous()
    again = LM.train_batch(raw.to(DEV), lab.to(DEV), MINS, MAXS, prep, params)         # equal parameters: equal bits
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    # and the drawn batch is the oracle's
    mn32, rg32 = MINS.astype(np.float32), (MAXS - MINS).astype(np.float32)
    lr = got[0].cpu().numpy()
    for i in range(B):
        ang = float(params.angle[i]) if bool(params.rotate[i]) else None
        f, p = int(params.flip[i]), tuple(int(v) for v in params.perm[i])
        want, scale = AO.aug_image(raw[i].numpy(), 4, 4, f, p, ang, mn32, rg32, (0, 1))
        assert np.all(np.abs(lr[i] - want) <= 2.0 ** -21 * scale)
        want_lab, (oh, _, ob, ow, _) = AO.aug_label_prep(lab[i].numpy(), f, p, ang, HIR, hw)
        assert torch.equal(got[1][i].cpu(), oh) and torch.equal(got[3][i].cpu(), ob) and torch.equal(got[4][i].cpu(), ow)


def test_sr_pair_clips_lq_and_not_gt():
    rows = TABLE[4:16]
    params = _params(rows)
    lr, hr = _bands(B, 3, 8, 8, seed=31), _bands(B, 3, 32, 32, seed=32)
    lmn, lmx, hmn, hmx = MINS[:3], MAXS[:3], np.array([0.0, 10.0, -20.0]), np.array([255.0, 900.0, 2000.0])
    lq, gt = LM.sr_pair(lr.to(DEV), hr.to(DEV), lmn, lmx, hmn, hmx, params)
    assert lq.shape == (B, 3, 8, 8) and gt.shape == (B, 3, 32, 32) and lq.is_contiguous() and gt.is_contiguous()
    lq, gt = lq.cpu().numpy(), gt.cpu().numpy()
    f32 = lambda v: np.asarray(v).astype(np.float32)          # noqa: E731
    for i, (f, p, ang) in enumerate(rows):
        want, scale = AO.aug_image(lr[i].numpy(), 4, 4, f, p, ang, f32(lmn), f32(lmx - lmn), (0, 1))
        assert np.all(np.abs(lq[i] - want) <= 2.0 ** -21 * scale)
        want, scale = AO.aug_image(hr[i].numpy(), 1, 1, f, p, ang, f32(hmn), f32(hmx - hmn), None)
        assert np.all(np.abs(gt[i] - want) <= 2.0 ** -21 * scale)
    assert lq.min() == 0.0 and lq.max() == 1.0 and gt.min() < 0.0 and gt.max() > 1.0
    # no parameters: the un-augmented pair
    lq0, gt0 = LM.sr_pair(lr.to(DEV), hr.to(DEV), lmn, lmx, hmn, hmx, None)
    assert torch.equal(lq0, LM.normalize_tiles(lr.to(DEV), lmn, lmx, (0, 1))) and torch.equal(gt0, LM.normalize_tiles(hr.to(DEV), hmn, hmx, None))


def test_writes_stay_inside_the_outputs(g9):
    """both entries at 16 x 24 with every output carved out of guard-filled storage, the byte label at an odd 4-byte offset"""
    stats, hw = g9
    prep = LM.LabelPrep(HIR, hw, DEV)
    rows = TABLE[4:16]
    dp = LM.Augment().to_device(_params(rows), 16, 24, DEV)
    L = _lib.lib()
    gb = GuardedBuffers()
    raw = gb.inp(_bands(B, 3, 4, 6, seed=41))
    for up, step, src in ((4, 4, raw), (4, 1, raw)):
        dst = gb.out((B, 3, 16 // step, 24 // step), offset=1)
        _lib.check(L.srbh_aug_image(src.data_ptr(), B, 3, 4, 6, up, dst.data_ptr(), step, dp.flip.data_ptr(), dp.perm.data_ptr(),
                                    dp.tables.data_ptr(), None, None, 0.0, 0.0, 0, _lib.stream_ptr()), "aug_image")
    lab = gb.inp(_labels(stats, B, 16, 24, seed=42), dtype=torch.uint8)
    build = gb.out((B, 16, 24), dtype=torch.int64)
    hf, wt, ha, wa = gb.out((B, 16, 24), 1), gb.out((B, 16, 24), 3), gb.out((B, 4, 6), 1), gb.out((B, 4, 6), 2)
    out = gb.out((B, 16, 24), offset=4, dtype=torch.uint8)
    _lib.check(L.srbh_aug_label_prep(lab.data_ptr(), B, 16, 24, dp.flip.data_ptr(), dp.perm.data_ptr(), dp.tables.data_ptr(),
                                     prep.lut.data_ptr(), prep.cw.data_ptr(), build.data_ptr(), hf.data_ptr(), wt.data_ptr(), ha.data_ptr(),
                                     wa.data_ptr(), out.data_ptr(), _lib.stream_ptr()), "aug_label_prep")
    gb.verify()


# ---- refusals: SRBH_ERR_ARG and the entry's own name in the text; nothing is launched ------------------------------------------------
IMG, LAB = "srbh_aug_image", "srbh_aug_label_prep"
IMG_BASE = dict(src=True, B=1, C=1, Hs=4, Ws=6, up=4, dst=True, step=4, flip=True, perm=True, tables=True, mins=None, ranges=None,
                lo=0.0, hi=1.0, clamp=0)
LAB_BASE = dict(height=True, B=1, H=16, W=24, flip=True, perm=True, tables=True, lut=True, cw=True, build=True, height_f=True, weight=True,
                height_aggre=True, weight_aggre=True, label_out=None)
INTS = ("B", "C", "Hs", "Ws", "up", "step", "clamp", "H", "W")
FLOATS = ("lo", "hi")


def _refusals():
    out = []

    def add(entry, name, text, **change):
        out.append(pytest.param(entry, change, f"{entry}: {text}", id=f"{entry[5:]}-{name}"))
    for k in ("src", "dst", "flip", "perm", "tables"):
        add(IMG, f"null_{k}", "null pointer", **{k: None})
    add(IMG, "mins_alone", "mins and ranges go together", mins=True)
    add(IMG, "ranges_alone", "mins and ranges go together", ranges=True)
    add(IMG, "B_0", "bad geometry B=0 C=1 Hs=4 Ws=6", B=0)
    add(IMG, "C_0", "bad geometry B=1 C=0 Hs=4 Ws=6", C=0)
    add(IMG, "Ws_neg", "bad geometry B=1 C=1 Hs=4 Ws=-6", Ws=-6)
    add(IMG, "up_0", "up=0 step=4 must be >= 1 and the grid at most 32768 a side", up=0)
    add(IMG, "step_0", "up=4 step=0 must be >= 1 and the grid at most 32768 a side", step=0)
    add(IMG, "grid_too_large", "up=4 step=4 must be >= 1 and the grid at most 32768 a side", Hs=8200)
    add(IMG, "H_not_8", "grid 20 x 24 must be multiples of 8", Hs=5)
    add(IMG, "W_not_8", "grid 16 x 12 must be multiples of 8", Ws=3)
    add(IMG, "step_3", "step=3 does not divide the grid 16 x 24", step=3)
    add(IMG, "step_16", "step=16 does not divide the grid 16 x 24", step=16)
    add(IMG, "perm_unaligned", "perm must be 16-byte aligned", perm=4)
    for k in ("height", "flip", "perm", "tables", "lut", "cw", "build", "height_f", "weight", "height_aggre", "weight_aggre"):
        add(LAB, f"null_{k}", "null pointer", **{k: None})
    add(LAB, "B_0", "bad geometry B=0 H=16 W=24", B=0)
    add(LAB, "H_too_large", "bad geometry B=1 H=32776 W=24", H=32776)
    add(LAB, "H_not_8", "H=20, W=24 must be multiples of 8", H=20)
    add(LAB, "W_not_8", "H=16, W=12 must be multiples of 8", W=12)
    add(LAB, "tables_unaligned", "perm and tables must be 16-byte aligned", tables=8)
    add(LAB, "label_out_unaligned", "label_out must be 4-byte aligned", label_out=2)
    return out


@pytest.fixture(scope="module")
def dummy():
    return torch.zeros(4096, dtype=torch.uint8, device=DEV)


@pytest.mark.parametrize("entry,change,want", _refusals())
def test_refusal_names_its_own_entry(dummy, entry, change, want):
    import ctypes as C
    L = _lib.lib()
    fields = {**(IMG_BASE if entry == IMG else LAB_BASE), **change}
    args = []
    for k, v in fields.items():
        if k in INTS:
            args.append(v)
        elif k in FLOATS:
            args.append(float(v))
        else:                  # a pointer: None, True = the dummy buffer, an int = that many bytes past it
            args.append(None if v is None else C.c_void_p(dummy.data_ptr() + (0 if v is True else v)))
    rc = getattr(L, entry)(*args, _lib.stream_ptr())
    got = L.srbh_last_error().decode()
    print(f"{entry}: rc={rc} {got!r}")
    assert rc == SRBH_ERR_ARG
    assert got == want
    assert not dummy.any()


def test_host_tensors_and_bad_parameters_raise(g9):
    stats, hw = g9
    prep = LM.LabelPrep(HIR, hw, DEV)
    raw, lab = _bands(2, 8, 4, 6, seed=51), _labels(stats, 2, 16, 24, seed=52)
    with pytest.raises(RuntimeError, match="no CPU"):
        LM.train_batch(raw, lab.to(DEV), MINS, MAXS, prep)
    with pytest.raises(RuntimeError, match="no CPU"):
        LM.train_batch(raw.to(DEV), lab, MINS, MAXS, prep)
    with pytest.raises(RuntimeError, match="no CPU"):
        LM.sr_pair(raw.to(DEV), _bands(2, 3, 16, 24, seed=53), MINS, MAXS, MINS[:3], MAXS[:3], None)
    with pytest.raises(ValueError, match="x4 grid"):
        LM.train_batch(raw.to(DEV), lab[:, :8].to(DEV), MINS, MAXS, prep)
    with pytest.raises(ValueError, match="parameters made for"):
        LM.train_batch(raw.to(DEV), lab.to(DEV), MINS, MAXS, prep, LM.AugmentParams.identity(3))
    with pytest.raises(RuntimeError, match="srbh_aug_image: grid 20 x 24"):        # the library's refusal reaches the caller as an error
        dp = LM.Augment().to_device(LM.AugmentParams.identity(2), 16, 24, DEV)
        dp.Hg = 20
        LM._aug_image(torch.zeros(2, 1, 5, 6, device=DEV), 4, 4, dp, None, None, None, "aug_image")
