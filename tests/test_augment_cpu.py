"""CPU: the training augmentation's definition -- the numpy oracle against plain numpy facts, Augment.tables against
the float64 coordinates it rounds, Augment.draw against its distribution.  No kernel is launched here."""
import itertools
import math

import numpy as np
import pytest
import torch

from oracle import loader_oracle as LO
from tests import augment_oracle as AO

HIR = (0, 3, 12, 21, 30, 60, 90, 256)
IDENT = (0, 1, 2, 3)
# 8 x 48 is there for the fold: a quarter turn of it samples 20 px outside an axis of 8, where one reflection is not enough
SHAPES = ((256, 256), (32, 48), (16, 24), (8, 48))
ANGLES = np.concatenate([np.random.default_rng(0).uniform(-90.0, 90.0, 200), [0.0, 90.0, -90.0, 45.0, -45.0, 1e-3]])


def _lm():
    from srbh_amd import loader_math as LM
    return LM


def _ramp(H, W):
    return np.arange(H * W, dtype=np.int64).reshape(H, W)


def test_identity_parameters_are_todays_loader_math():
    LM = _lm()
    rs = np.random.default_rng(1)
    raw = (rs.random((8, 6, 10)) * 3000 - 200).astype(np.float32)
    mins = np.linspace(-100, 50, 8)
    maxs = mins + np.linspace(1500, 2600, 8)
    mn32, rg32 = mins.astype(np.float32), (maxs - mins).astype(np.float32)
    want = LO.normalize(torch.from_numpy(raw), mins, maxs, (0, 1)).numpy()
    for angle in (None, 0.0):
        got32, _ = AO.aug_image(raw, 4, 4, 0, IDENT, angle, mn32, rg32, (0, 1), dtype=np.float32)
        assert got32.dtype == np.float32 and np.array_equal(got32, want)        # the literal chain in fp32: bit for bit
        got64, scale = AO.aug_image(raw, 4, 4, 0, IDENT, angle, mn32, rg32, (0, 1))
        assert got64.dtype == np.float64 and np.all(np.abs(got64 - want) <= 2.0 ** -21 * scale)
        up, _ = AO.aug_image(raw, 4, 1, 0, IDENT, angle)
        assert np.array_equal(up, np.repeat(np.repeat(raw, 4, 1), 4, 2).astype(np.float64))
    lab = rs.integers(0, 256, (24, 40)).astype(np.uint8)
    hw = np.linspace(0.1, 3.0, 7)
    out, prepped = AO.aug_label_prep(lab, 0, IDENT, None, HIR, hw)
    assert np.array_equal(out, lab)
    for a, b in zip(prepped, LO.label_prep(lab, HIR, hw)):
        assert torch.equal(a, b)
    # Augment.tables: the identity tables for an image that is not rotated, and for one rotated by 0 degrees
    p = LM.AugmentParams([0, 0, 0], [IDENT] * 3, [0.0, 33.0, 0.0], [False, False, True])
    t = LM.Augment().tables(p, 24, 40)
    assert t.dtype == np.int32 and t.shape == (3, 2 * 40 + 2 * 24)
    ident = np.concatenate([1024 * np.arange(40), np.zeros(40), np.zeros(24), 1024 * np.arange(24)]).astype(np.int32)
    assert np.array_equal(t, np.stack([ident] * 3))
    assert np.array_equal(LM.Augment().tables(LM.AugmentParams.identity(2), 24, 40), np.stack([ident] * 2))
    assert np.array_equal(np.concatenate(AO.tables(None, 24, 40)), ident)


def test_flips_and_shuffle_are_what_numpy_says():
    img = _ramp(16, 24)
    assert np.array_equal(AO.aug_label(img, 1, IDENT, None), np.flip(img, 1))
    assert np.array_equal(AO.aug_label(img, 2, IDENT, None), np.flip(img, 0))
    assert np.array_equal(AO.aug_label(img, 3, IDENT, None), np.flip(img, (0, 1)))
    assert np.array_equal(AO.aug_label(img, 0, IDENT, None), img)
    tl, tr, bl, br = img[:8, :12], img[:8, 12:], img[8:, :12], img[8:, 12:]
    want = np.block([[tr, bl], [tl, br]])                    # perm (1, 2, 0, 3): dst 0 <- cell 1, dst 1 <- cell 2, dst 2 <- cell 0
    got = AO.aug_label(img, 0, (1, 2, 0, 3), None)
    assert np.array_equal(got, want)
    inverse = AO.aug_label(img, 0, (2, 0, 1, 3), None)
    assert np.array_equal(inverse, np.block([[bl, tl], [tr, br]])) and not np.array_equal(got, inverse)
    assert np.array_equal(AO.aug_label(got, 0, (2, 0, 1, 3), None), img)


def test_flip_comes_before_shuffle():
    img = _ramp(16, 24)
    perm = (1, 2, 0, 3)
    flip_then_shuffle = AO.grid_shuffle(np.flip(img, 1), perm)
    shuffle_then_flip = np.flip(AO.grid_shuffle(img, perm), 1)
    assert not np.array_equal(flip_then_shuffle, shuffle_then_flip)
    assert np.array_equal(AO.aug_label(img, 1, perm, None), flip_then_shuffle)
    fl = np.flip(img, 1)
    assert np.array_equal(flip_then_shuffle, np.block([[fl[:8, 12:], fl[8:, :12]], [fl[:8, :12], fl[8:, 12:]]]))


def test_quarter_turns_are_rot90():
    img = _ramp(32, 32)
    assert np.array_equal(AO.rotate_nearest(img, 90.0), np.rot90(img, 1))
    assert np.array_equal(AO.rotate_nearest(img, -90.0), np.rot90(img, -1))
    assert np.array_equal(AO.rotate_nearest(img, 0.0), img)
    for ang, k in ((90.0, 1), (-90.0, -1), (0.0, 0)):
        v, _ = AO.rotate_bilinear(img, ang)
        assert np.array_equal(v, np.rot90(img, k).astype(np.float64))              # fraction 0 everywhere
    b = _ramp(16, 24)
    r = AO.rotate_nearest(b, 90.0)
    assert r.shape == b.shape and set(r.ravel()) <= set(b.ravel())
    assert np.array_equal(r[:, 4:20], np.rot90(b, 1)[4:20, :])                     # the part of the turned image that stays in the frame


@pytest.fixture(scope="module")
def coordinate_cases():
    """per shape: Augment.tables of every angle, and the float64 source coordinates"""
    LM = _lm()
    out = {}
    p = LM.AugmentParams(np.zeros(len(ANGLES), dtype=np.int32), [IDENT] * len(ANGLES), ANGLES)
    for H, W in SHAPES:
        t = LM.Augment().tables(p, H, W).astype(np.int64)
        out[(H, W)] = (t[:, :W], t[:, W:2 * W], t[:, 2 * W:2 * W + H], t[:, 2 * W + H:])
    return out


def _float_coords(angle, H, W):
    m = AO.matrix(angle, H, W)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    return m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fixed_point_coordinates_follow_the_float64_map(coordinate_cases, shape):
    H, W = shape
    ax, bx, X0, Y0 = coordinate_cases[shape]
    worst_near, worst_lin, overshoot = 0, 0.0, np.zeros(2)
    for k, angle in enumerate(ANGLES):
        o = AO.tables(float(angle), H, W)                       # the oracle's own tables are the same integers
        assert all(np.array_equal(a, b) for a, b in zip(o, (ax[k], bx[k], X0[k], Y0[k]))), angle
        sx, sy = _float_coords(float(angle), H, W)
        for s, t0, t1 in ((sx, X0[k], ax[k]), (sy, Y0[k], bx[k])):
            fixed = t0[:, None] + t1[None, :]
            near = (fixed + 512) >> 10
            clear = np.abs(s + 0.5 - np.rint(s + 0.5)) > 2.0 ** -10      # farther than 2^-10 from a half-integer
            worst_near = max(worst_near, int(np.abs(near - np.floor(s + 0.5))[clear].max(initial=0)))
            worst_lin = max(worst_lin, float(np.abs(((fixed + 16) >> 5) / 32.0 - s).max()))
        overshoot = np.maximum(overshoot, [max(-sx.min(), sx.max() - (W - 1)) / (W - 1), max(-sy.min(), sy.max() - (H - 1)) / (H - 1)])
    print(f"{H}x{W}: nearest off by {worst_near}, bilinear coordinate error {worst_lin:.5f} px, overshoot / (N-1) = {overshoot}")
    assert worst_near == 0
    assert worst_lin <= 1.0 / 64 + 2.0 ** -10
    if shape == (8, 48):
        assert overshoot[1] > 1.0          # beyond one reflection: the general fold is needed and is what these cases sample through


def test_fold_is_the_general_reflect_101():
    i = np.arange(-40, 60)
    want = []
    for v in i:                            # walk the mirror literally
        while v < 0 or v > 7:
            v = -v if v < 0 else 14 - v
        want.append(v)
    assert np.array_equal(AO.reflect101(i, 8), want)
    img = _ramp(8, 48)
    r = AO.rotate_nearest(img, 90.0)       # source rows run from -20 to 27 about the 8 rows there are
    _, Y = AO.coords_nearest(90.0, 8, 48)
    assert Y.min() == -20 and Y.max() == 27 and r.shape == img.shape
    single = np.where(Y < 0, -Y, np.where(Y > 7, 14 - Y, Y))
    assert (single < 0).any() or (single > 7).any()             # one reflection leaves the image


def _within(count, n, p, what):
    sd = math.sqrt(n * p * (1 - p))
    assert abs(count - n * p) <= 5 * sd, f"{what}: {count} of {n}, expected {n * p:.0f} +- {sd:.1f}"


def test_draw_distribution_and_seed():
    LM = _lm()
    N = 24000
    g = torch.Generator()
    g.manual_seed(2024)
    p = LM.Augment().draw(N, g)
    assert p.flip.dtype == torch.int32 and p.perm.shape == (N, 4) and p.angle.dtype == torch.float64 and p.rotate.dtype == torch.bool
    flip, perm, angle, rot = p.flip.numpy(), p.perm.numpy(), p.angle.numpy(), p.rotate.numpy()
    _within(int((flip != 0).sum()), N, 0.5, "flip applied")
    _within(int(rot.sum()), N, 0.5, "rotate applied")
    for code in (1, 2, 3):
        _within(int((flip == code).sum()), N, 0.5 / 3, f"flip code {code}")
    seen = 0
    for q in itertools.permutations(range(4)):
        n = int((perm == np.array(q)).all(axis=1).sum())
        seen += n
        _within(n, N, 0.5 / 24 + (0.5 if q == IDENT else 0.0), f"perm {q}")      # (the identity is also what no shuffle leaves)
    assert seen == N
    assert np.all(angle[~rot] == 0.0) and angle[rot].min() >= -90.0 and angle[rot].max() < 90.0
    bins = np.floor((angle[rot] + 90.0) / 18.0).astype(int)
    for k in range(10):
        _within(int((bins == k).sum()), N, 0.05, f"angle bin {k}")
    # the three steps are drawn independently of each other
    _within(int(((flip != 0) & rot).sum()), N, 0.25, "flip and rotate")
    _within(int(((flip != 0) & (perm != np.array(IDENT)).any(axis=1)).sum()), N, 0.5 * 0.5 * 23 / 24, "flip and shuffle")
    g2 = torch.Generator()
    g2.manual_seed(2024)
    q = LM.Augment().draw(N, g2)
    assert torch.equal(p.flip, q.flip) and torch.equal(p.perm, q.perm) and torch.equal(p.angle, q.angle) and torch.equal(p.rotate, q.rotate)
    g2.manual_seed(2025)
    assert not torch.equal(LM.Augment().draw(N, g2).flip, p.flip)
    none = LM.Augment(p_flip=0.0, p_shuffle=0.0, p_rotate=0.0).draw(64, g2)
    assert not none.flip.any() and not none.rotate.any() and bool((none.perm == torch.tensor(IDENT, dtype=torch.int32)).all())


def test_refusals():
    LM = _lm()
    with pytest.raises(NotImplementedError):
        LM.Augment(grid=(3, 3))
    with pytest.raises(NotImplementedError):
        LM.Augment(grid=(2, 4))
    with pytest.raises(ValueError, match="permutation"):
        LM.AugmentParams([0], [(0, 1, 1, 3)], [0.0])
    with pytest.raises(ValueError, match="permutation"):
        LM.AugmentParams([0, 0], [IDENT, (1, 2, 3, 4)], [0.0, 0.0])
    with pytest.raises(ValueError, match="flip code"):
        LM.AugmentParams([4], [IDENT], [0.0])
    with pytest.raises(ValueError, match="flip code"):
        LM.AugmentParams([-1], [IDENT], [0.0])
    with pytest.raises(ValueError, match="same"):
        LM.AugmentParams([0, 0], [IDENT], [0.0, 0.0])
    p = LM.AugmentParams.identity(1)
    for H, W in ((20, 24), (24, 20), (0, 8)):
        with pytest.raises(ValueError, match="multiples of 8"):
            LM.Augment().tables(p, H, W)
    with pytest.raises(RuntimeError, match="device"):
        LM.Augment().to_device(p, 16, 24, "cpu")
    prep = object()
    with pytest.raises(RuntimeError, match="no CPU"):
        LM.train_batch(torch.zeros(1, 8, 4, 6), torch.zeros(1, 16, 24, dtype=torch.uint8), np.zeros(8), np.ones(8), prep)
    with pytest.raises(RuntimeError, match="no CPU"):
        LM.sr_pair(torch.zeros(1, 3, 4, 6), torch.zeros(1, 3, 16, 24), np.zeros(3), np.ones(3), np.zeros(3), np.ones(3), p)
