"""srgan.PerceptualLoss.libsrbh = "f16" on the device: the VGG19 feature stack, the loss and its input gradient on libsrbh's 16-bit kernels
(srbh_wconv3x3 + csrc/srbh_vgg.hip), against fixture g15 (the reference's own class on the seeded stack) and against the float64 emulation of the
arithmetic contract (tests/vgg_emulation.py), in both forms of the fixture: cuts [2, 7, 16, 25, 34] / L1 / ImageNet norm, and the single cut 7 /
MSE / range map.  Inputs rand((2, 3, 48, 40), 150 / 151): planes 48x40 -> 24x20 -> 12x10 -> 6x5 -> 3x2.

Bounds.  The mode's own distance from the reference is e_loss / e_gx of tests/test_vgg_emulation_cpu.py (reference + CPU only).  The kernels
differ from the emulation by fp32 instead of float64 accumulation only -- but one fp16 rounding per conv turns that into an independent draw of
the rounding noise within a few layers (measured on an MI355X, fixture inputs: planes of conv 0 differ from the emulation's in 47 of 245 760
elements, of conv 3 in 10 %, of the last cut in 78 %, rel-L2 9.8e-4: the fp16 noise itself).  The project's 3 % rule for "two distances from the
oracle agree" (tests/test_gpu_f16x2_net.py) therefore does not hold for the loss and is not asserted: d_gpu 2.296e-4 against d_emu 1.442e-4 on the
list form (59 %), while on the CPU alone 8 accumulation orders of the emulation give -1.3e-6 .. +2.04e-4 (test_vgg_emulation_cpu.py,
LOSS_SPREAD).  Asserted instead, from that CPU measurement: the signed relative loss error within mean +- 4 standard deviations of the
realisations (list: <= 3.3e-4 = 2.3 e_loss), and kernels against emulation within 4 sqrt(2) standard deviations (two draws).
The gradient is a sign function of feature differences behind step functions, so its margin is MEASURED as the issue asks: |d_gpu - d_emu| / d_emu
over three input seeds on an MI355X, twice the largest value seen is asserted (GX_AGREE below, the measured values next to it)."""
import pytest
import torch

from srbh_amd import srgan
from tests import vgg_emulation as E
from tests.test_vgg_emulation_cpu import E_LIST, E_SINGLE, LOSS_SPREAD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NSIGMA = 4.0
# |d_gpu - d_emu| / d_emu of the input gradient, distances from the float64 stock module, seeds (150, 151), (152, 153), (154, 155), MI355X:
#   list form   1.1034e-1, 4.768e-2, 1.461e-2      (d_gpu 9.096e-2 / 9.148e-2 / 8.925e-2, d_emu 1.0224e-1 / 8.732e-2 / 8.797e-2)
#   single form 9.476e-3, 3.169e-3, 6.5e-5         (d_gpu 3.592e-2 / 3.166e-2 / 3.218e-2, d_emu 3.627e-2 / 3.156e-2 / 3.218e-2)
GX_AGREE = {"list": 2 * 1.1034e-1, "single": 2 * 9.476e-3}
SEEDS = [(150, 151), (152, 153), (154, 155)]
FORMS = {
    "list": dict(ctor=dict(), emu=dict(), pre=lambda t: t, chain=1.0, keys=("l1_list_loss", "l1_list_gx"), e=E_LIST),
    "single": dict(ctor=dict(feature_layer=7, lossfn_type="l2", use_input_norm=False, use_range_norm=True, loss_weight=0.5),
                   emu=dict(cuts=(7,), weights=(1.0,), l2=True, use_input_norm=False, use_range_norm=True), pre=lambda t: t * 2 - 1, chain=2.0,
                   keys=("mse_single_loss", "mse_single_gx"), e=E_SINGLE),
}


@pytest.fixture(scope="module")
def sd():
    return E.seeded_state_dict()


@pytest.fixture(scope="module")
def modules(sd):
    """{form: (module on the device with the mode on, float64 stock module on the CPU)}: built once"""
    out = {}
    for form, f in FORMS.items():
        dev = srgan.PerceptualLoss(state_dict=sd, **f["ctor"]).to(DEV)
        dev.libsrbh = "f16"
        out[form] = (dev, srgan.PerceptualLoss(state_dict=sd, **f["ctor"]).double())
    return out


def run_gpu(pl, f, x, gt, scale=None):
    xd = x.to(DEV).requires_grad_(True)
    loss = pl(f["pre"](xd), f["pre"](gt.to(DEV)))
    (loss if scale is None else loss * scale).backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), xd.grad.cpu()


def run_stock64(pl, f, x, gt):
    xc = x.double().requires_grad_(True)
    loss = pl(f["pre"](xc), f["pre"](gt.double()))
    loss.backward()
    return float(loss.detach()), xc.grad


@pytest.mark.parametrize("form", ["list", "single"])
def test_against_the_reference_fixture_and_the_emulation(form, modules, sd, golden_dir):
    f, g = FORMS[form], E.g15(golden_dir)
    x, gt = E.fixture_inputs()
    loss, gx = run_gpu(modules[form][0], f, x, gt)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    l_emu, gx_emu = E.perceptual(sd, f["pre"](x), f["pre"](gt), **f["emu"])
    gx_emu = gx_emu * f["chain"]
    l_ref, gx_ref = float(g[f["keys"][0]]), torch.from_numpy(g[f["keys"][1]])
    d_loss, d_loss_emu = abs(float(loss) - l_ref) / abs(l_ref), abs(l_emu - l_ref) / abs(l_ref)
    d_gx, d_gx_emu = E.rel_l2(gx, gx_ref), E.rel_l2(gx_emu, gx_ref)
    e_loss, e_gx = f["e"]
    print(f"[perceptual {form}] loss gpu {float(loss)!r} emu {l_emu!r} ref {l_ref!r}: d_gpu {d_loss:.4e} d_emu {d_loss_emu:.4e} "
          f"({100 * abs(d_loss - d_loss_emu) / d_loss_emu:.2f} %), gpu vs emu {abs(float(loss) - l_emu) / abs(l_emu):.3e}")
    print(f"[perceptual {form}] x.grad: d_gpu {d_gx:.4e} d_emu {d_gx_emu:.4e} ({100 * abs(d_gx - d_gx_emu) / d_gx_emu:.3f} %), "
          f"gpu vs emu {E.rel_l2(gx, gx_emu):.3e}")
    mu, sigma = LOSS_SPREAD[form]
    assert abs((float(loss) - l_ref) / abs(l_ref) - mu) <= NSIGMA * sigma, (float(loss), l_ref, mu, sigma)
    assert abs(float(loss) - l_emu) / abs(l_ref) <= NSIGMA * 2 ** 0.5 * sigma, (float(loss), l_emu, sigma)
    assert d_gx <= e_gx * (1 + GX_AGREE[form]), (d_gx, e_gx)
    assert abs(d_gx - d_gx_emu) <= GX_AGREE[form] * d_gx_emu, (d_gx, d_gx_emu)


@pytest.mark.parametrize("form", ["list", "single"])
def test_gradient_agrees_with_the_emulation_over_three_seeds(form, modules, sd):
    """the measurement behind GX_AGREE, asserted: distances of x.grad from the float64 stock module, kernels against emulation"""
    f = FORMS[form]
    seen = []
    for sx, sg in SEEDS:
        x, gt = E.rand((2, 3, 48, 40), sx, 0.0, 1.0), E.rand((2, 3, 48, 40), sg, 0.0, 1.0)
        l_ref, gx_ref = run_stock64(modules[form][1], f, x, gt)
        loss, gx = run_gpu(modules[form][0], f, x, gt)
        l_emu, gx_emu = E.perceptual(sd, f["pre"](x), f["pre"](gt), **f["emu"])
        d_gpu, d_emu = E.rel_l2(gx, gx_ref), E.rel_l2(gx_emu * f["chain"], gx_ref)
        seen.append(abs(d_gpu - d_emu) / d_emu)
        print(f"[perceptual {form}] seeds ({sx},{sg}): x.grad d_gpu {d_gpu:.5e} d_emu {d_emu:.5e} |d_gpu - d_emu| / d_emu = {seen[-1]:.4e}; "
              f"loss gpu vs emu {abs(float(loss) - l_emu) / abs(l_emu):.3e}, gpu vs float64 stock {abs(float(loss) - l_ref) / abs(l_ref):.3e}")
    assert max(seen) <= GX_AGREE[form], seen


def test_grad_output_scaling_and_a_second_call(modules):
    """(3 loss).backward() scales dloss/dx in the last kernel; a second call reuses the packs and the plane buffers and returns the same bits"""
    pl, f = modules["list"][0], FORMS["list"]
    x, gt = E.fixture_inputs()
    l1, g1 = run_gpu(pl, f, x, gt)
    packs, planes = pl._srbh_vgg_packs, pl._srbh_vgg_planes
    ptrs = {k: b.data_ptr() for pool in planes.values() for k, b in pool.bufs.items()}
    l2, g2 = run_gpu(pl, f, x, gt)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    assert pl._srbh_vgg_packs is packs and {k: b.data_ptr() for pool in pl._srbh_vgg_planes.values() for k, b in pool.bufs.items()} == ptrs
    l3, g3 = run_gpu(pl, f, x, gt, scale=3.0)
    assert torch.equal(l3, l1) and torch.equal(g3, g1 * 3.0)
    with torch.no_grad():
        assert torch.equal(pl(x.to(DEV), gt.to(DEV)).cpu(), l1)


def test_unsupported_cut_raises(sd):
    pl = srgan.PerceptualLoss(feature_layer=(3, 8), weights=(1.0, 1.0), state_dict=sd).to(DEV)
    x, gt = E.fixture_inputs()
    with torch.no_grad():
        pl(x.to(DEV), gt.to(DEV))                             # stock path: fine
    pl.libsrbh = "f16"
    with pytest.raises(NotImplementedError, match="cut 3"):
        pl(x.to(DEV), gt.to(DEV))


def test_cpu_input_and_unset_attribute_keep_the_stock_path(sd, golden_dir):
    g = E.g15(golden_dir)
    x, gt = E.fixture_inputs()
    stock = srgan.PerceptualLoss(state_dict=sd)
    mode = srgan.PerceptualLoss(state_dict=sd)
    mode.libsrbh = "f16"
    assert list(mode.state_dict()) == list(stock.state_dict()) and [n for n, _ in mode.named_modules()] == [n for n, _ in stock.named_modules()]
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    la, lb = stock(xa, gt), mode(xb, gt)                      # CPU tensors: the stock ops, whatever the attribute says
    la.backward()
    lb.backward()
    assert torch.equal(la, lb) and torch.equal(xa.grad, xb.grad)
    dev = srgan.PerceptualLoss(state_dict=sd).to(DEV)         # attribute unset on the device: as today, the fixture at 1e-5
    assert dev.libsrbh is None
    xd = x.to(DEV).requires_grad_(True)
    ld = dev(xd, gt.to(DEV))
    ld.backward()
    assert abs(float(ld) - float(g["l1_list_loss"])) <= 1e-5 * abs(float(g["l1_list_loss"]))
    assert E.rel_l2(xd.grad.cpu(), torch.from_numpy(g["l1_list_gx"])) <= 1e-5
    assert not hasattr(dev, "_srbh_vgg_packs")


def test_trainer_runs_the_term_on_libsrbh(sd, monkeypatch):
    """RealESRGAN(is_train=True, vgg19_weights=...) with SRBH_SR_VGG=libsrbh in the `mixed` mode: four iterations on the 128x128 pair of
    tests/test_sr_stage.py; loss_dict keys as upstream, l_g_percep finite, positive and falling; the mode really ran (its packs exist)"""
    from srbh_amd import rrdbnet_autograd as RA
    from srbh_amd.rrdbnet import RealESRGAN
    monkeypatch.setenv("SRBH_SR_VGG", "libsrbh")
    RA.set_train_precision("mixed")
    try:
        torch.manual_seed(3)
        m = RealESRGAN(3, 3, num_block=1, device=DEV, is_train=True, vgg19_weights=sd)
        gt = torch.nn.functional.interpolate(E.rand((2, 3, 16, 16), 9, 0.0, 1.0), scale_factor=8, mode="bilinear")
        lq = torch.nn.functional.avg_pool2d(gt, 4)
        vals = []
        for it in range(4):
            m.feed_data({"lq": lq, "gt": gt})
            ld = m.optimize_parameters()
            assert list(ld) == ["l_g_pix", "l_g_percep", "l_g_gan", "l_d_real", "out_d_real", "l_d_fake", "out_d_fake"]
            vals.append(ld["l_g_percep"])
        print(f"[perceptual trainer] l_g_percep {vals}")
        assert m.cri_perceptual.libsrbh == "f16" and hasattr(m.cri_perceptual, "_srbh_vgg_packs")
        assert all(v == v and v > 0 for v in vals) and vals[-1] < vals[0], vals
    finally:
        RA.set_train_precision("f32")
