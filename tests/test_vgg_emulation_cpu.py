"""The arithmetic contract of PerceptualLoss.libsrbh = "f16" on the CPU (tests/vgg_emulation.py: float64 with every rounding of the kernels at its
place, forward and backward) against fixture g15, the reference's own PerceptualLoss on the seeded VGG19 stack and rand((2, 3, 48, 40), 150 / 151):
planes 48x40 -> 24x20 -> 12x10 -> 6x5 -> 3x2 (ragged tiles, an odd size in front of a pool, a 3x2 plane).

The mode's own distance from the reference -- what one fp16 rounding per conv and one bf16 rounding per gradient plane cost, nothing a kernel
could remove -- from the reference and a CPU computation only:

    list form (cuts 2, 7, 16, 25, 34, L1, ImageNet norm):   e_loss = 1.4424e-4   e_gx = 1.0224e-1
    single cut 7, MSE, range map:                            e_loss = 3.604e-6    e_gx = 3.631e-2

The L1 gradient is a sign function of feature differences and every ReLU a step function of a pre-activation: an element whose fp16 rounding
moves it across zero changes its gradient by 100 %, which is where the 10 % of the list form come from (with the bf16 roundings of the backward
switched off it is 1.018e-1; with every rounding off the emulation meets the fixture at 1.3e-7 / 6.5e-7).

What the contract does NOT pin: it fixes the roundings, not the order of the additions inside a conv, and a kernel accumulates in fp32.  A change
of 1e-7 in a pre-activation flips the fp16 rounding of one element in ~5 000; the flipped elements are a perturbation of the next conv's input
that flips more roundings there (r_out ~ sqrt(r_in * ulp)), and after a few layers two accumulation orders are two independent draws of the
fp16 rounding noise.  e_loss is the small systematic part of a mean over that noise and moves by its own size from draw to draw.  Measured here
(vgg_emulation.conv(real=k): fp32, input channels in a seeded order; the float64 run and 8 realisations), signed (loss - reference) / reference:

    list form     -1.3e-6 .. +2.04e-4, mean +9.3e-5, standard deviation 6.0e-5      (e_gx 8.46e-2 .. 1.022e-1)
    single form   -7.0e-6 .. -1.5e-6,  mean -4.2e-6, standard deviation 1.6e-6      (e_gx 3.595e-2 .. 3.634e-2)

LOSS_SPREAD records mean and standard deviation: tests/test_gpu_perceptual.py holds the kernels' loss to mean +- 4 standard deviations.  The ABI
symbols the mode needs are checked here too, so that this file fails on a tree without the mode."""
import pytest
import torch

from tests import vgg_emulation as E

E_LIST = (1.4424e-4, 1.0224e-1)
E_SINGLE = (3.604e-6, 3.631e-2)
LOSS_SPREAD = {"list": (9.3e-5, 6.0e-5), "single": (-4.2e-6, 1.6e-6)}        # (mean, standard deviation) of the signed relative loss error
REPRODUCED = 0.02        # the float64 computation is deterministic up to the summation order inside a float64 conv: 2 % of a distance is generous


@pytest.fixture(scope="module")
def setup(golden_dir):
    return E.g15(golden_dir), E.seeded_state_dict(), E.fixture_inputs()


def test_the_mode_exists():
    """the attribute with its default, and every entry point of the mode in the ABI mirror"""
    from srbh_amd import _lib, srgan
    assert srgan.PerceptualLoss.libsrbh is None
    for name in ("srbh_wconv3x3", "srbh_vgg_input_f16", "srbh_vgg_relu_pool_f16", "srbh_vgg_relu_pool_bwd_b16", "srbh_vgg_dist_ws_bytes",
                 "srbh_vgg_dist", "srbh_vgg_dx_nchw"):
        assert name in _lib.SIGNATURES, name
        assert name in open(_lib.INCLUDE + "/srbh.h").read(), name


def test_list_form_distance_from_the_reference(setup):
    g, sd, (x, gt) = setup
    loss, gx = E.perceptual(sd, x, gt)
    e_loss = abs(loss - float(g["l1_list_loss"])) / abs(float(g["l1_list_loss"]))
    e_gx = E.rel_l2(gx, torch.from_numpy(g["l1_list_gx"]))
    print(f"[vgg emulation] list form: e_loss = {e_loss:.4e}  e_gx = {e_gx:.4e}")
    assert abs(e_loss - E_LIST[0]) <= REPRODUCED * E_LIST[0] and abs(e_gx - E_LIST[1]) <= REPRODUCED * E_LIST[1], (e_loss, e_gx)


def test_single_cut_mse_form_with_the_range_map(setup):
    g, sd, (x, gt) = setup
    loss, gx = E.perceptual(sd, x * 2 - 1, gt * 2 - 1, cuts=(7,), weights=(1.0,), l2=True, use_input_norm=False, use_range_norm=True)
    gx = gx * 2                                             # d(2 x - 1) / dx
    e_loss = abs(loss - float(g["mse_single_loss"])) / abs(float(g["mse_single_loss"]))
    e_gx = E.rel_l2(gx, torch.from_numpy(g["mse_single_gx"]))
    print(f"[vgg emulation] single cut, MSE, range map: e_loss = {e_loss:.4e}  e_gx = {e_gx:.4e}")
    assert abs(e_loss - E_SINGLE[0]) <= REPRODUCED * E_SINGLE[0] and abs(e_gx - E_SINGLE[1]) <= REPRODUCED * E_SINGLE[1], (e_loss, e_gx)


@pytest.mark.parametrize("form", ["list", "single"])
def test_accumulation_order_moves_the_loss_distance(setup, form):
    """the spread LOSS_SPREAD records: 8 fp32 realisations + the float64 run; sample mean within one recorded standard deviation of the recorded
    mean, sample standard deviation within a factor 2 (9 samples estimate it to ~25 %; the fp32 conv of another CPU may block its sums differently)"""
    g, sd, (x, gt) = setup
    if form == "list":
        ref, run = float(g["l1_list_loss"]), lambda k: E.perceptual(sd, x, gt, want_grad=False, real=k)[0]
    else:
        ref = float(g["mse_single_loss"])
        run = lambda k: E.perceptual(sd, x * 2 - 1, gt * 2 - 1, cuts=(7,), weights=(1.0,), l2=True, use_input_norm=False, use_range_norm=True,      # noqa: E731
                                     want_grad=False, real=k)[0]
    d = torch.tensor([(run(k) - ref) / abs(ref) for k in [None] + list(range(8))], dtype=torch.float64)
    mu, sigma = float(d.mean()), float(d.std())
    print(f"[vgg emulation] {form}: signed loss error over accumulation orders {float(d.min()):+.3e} .. {float(d.max()):+.3e}, mean {mu:+.3e}, std {sigma:.3e}")
    mu_r, sigma_r = LOSS_SPREAD[form]
    assert abs(mu - mu_r) <= sigma_r and 0.5 * sigma_r <= sigma <= 2 * sigma_r, (mu, sigma)
    assert float(d.max() - d.min()) > 0.03 * abs(float(d[0]))          # the 3 % rule of two distances cannot hold for this quantity


def test_the_emulation_without_roundings_is_the_reference(setup, monkeypatch):
    """structure check: with every rounding replaced by the identity the emulation is the reference's loss and gradient"""
    g, sd, (x, gt) = setup
    monkeypatch.setattr(E, "r16", lambda t: t.double())
    monkeypatch.setattr(E, "rb16", lambda t: t.double())

    def exact(x, use_input_norm, use_range_norm):
        x = x.double()
        if use_range_norm:
            x = (x + 1.0) / 2.0
        return (x - E.MEAN.double()) / E.STD.double() if use_input_norm else x
    monkeypatch.setattr(E, "normalise", exact)
    loss, gx = E.perceptual(sd, x, gt)
    assert abs(loss - float(g["l1_list_loss"])) <= 1e-5 * abs(float(g["l1_list_loss"]))
    assert E.rel_l2(gx, torch.from_numpy(g["l1_list_gx"])) <= 1e-5


def test_plan_of_the_mode_and_unsupported_cuts():
    from srbh_amd import srgan
    pl = srgan.PerceptualLoss()
    plan, cuts, weights = srgan._vgg_plan(pl)
    assert cuts == [2, 7, 16, 25, 34] and weights == [0.1, 0.1, 1.0, 1.0, 1.0] and len(plan) == 16
    assert [(c.in_channels, c.out_channels, cut, pool) for c, cut, pool, _ in plan][:5] == [
        (3, 64, False, False), (64, 64, True, True), (64, 128, False, False), (128, 128, True, True), (128, 256, False, False)]
    plan, cuts, weights = srgan._vgg_plan(srgan.PerceptualLoss(feature_layer=7))
    assert cuts == [7] and weights == [1.0] and [i for *_, i in plan] == [0, 2, 5, 7]
    with pytest.raises(NotImplementedError, match="cut 3"):
        srgan._vgg_plan(srgan.PerceptualLoss(feature_layer=(3, 8), weights=(1.0, 1.0)))
    with pytest.raises(NotImplementedError, match="cut 4"):
        srgan._vgg_plan(srgan.PerceptualLoss(feature_layer=4))
