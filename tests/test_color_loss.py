"""CPU: the fused Lab colour / RGB / background L1 loss (mg_color_loss_*) through every host layer, on the float64 contract
emulator of its two entry points (oracle/cabi_emulator.py, oracle/contracts.py), against what the REFERENCE's own classes computed
(tests/golden/color_loss_{i,ii}.npz, trainer_C*.npz from tools/make_color_loss_golden.py).

  1  the emulator contract vs the reference's float64 run: pins the contract in include/michigan_hip.h to the reference;
  2  networks.LabColorLoss / RGBBackgroundL1Loss / Pix2PixModel: the loss keys appear exactly under the reference's
     conditions, one forward call per generator step whatever subset is enabled;
  3  the reference's trainer with the README flags as published, through dropin.install(): reproduces trainer_C
     (the reference's own LabColorLoss raises on a current torch; the patched class needs no shim);
  3b this package's trainer against the same record.
The kernels themselves are checked on the GPU (tests/test_gpu_color_loss.py).
"""
import tempfile

import pytest
import torch

import color_loss_fixtures as CE
import parity_utils as PU
from oracle import contracts as K
from oracle import ref_harness as R
from oracle import trainer_parity as TP
from oracle.cabi_emulator import EmulatorBackend

needs_reference = pytest.mark.skipif(not R.reference_available(), reason="reference checkout not present")
# tests/test_dropin.py's emulator leg
TOL = dict(rtol_loss0=2e-4, rtol_later=1e-2, atol_img=2e-4, atol_weight=2 * 4e-4 * 2 + 1e-5)


pair = CE.load_pair


@pytest.fixture
def color_emulator():
    from michigan_amd import _cabi
    be = EmulatorBackend()
    prev = _cabi.set_backend(be)
    yield be
    _cabi.set_backend(prev)


@pytest.mark.parametrize("tag", ["i", "ii"])
def test_contract_matches_the_reference_in_float64(tag):
    fx = pair(tag)
    losses, grad, _ = K.color_terms(fx["fake"], fx["real"], fx["back"].float(), 7, tuple(fx["weights"].tolist()))
    for k in range(3):
        assert abs(float(losses[k]) - float(fx["losses"][k])) <= 1e-9 * abs(float(fx["losses"][k])), (k, losses, fx["losses"])
    # every pixel, the ones near a sign change included: float64 on both sides
    assert float((grad - fx["grad"]).norm() / fx["grad"].norm()) <= 1e-9
    if tag == "ii":
        assert float(grad[:, :, 40:48, 24:32].abs().max()) == 0.0            # sign(0) = 0 where fake == real


@pytest.mark.parametrize("tag", ["i", "ii"])
@pytest.mark.parametrize("channels", [3, 8])
def test_ops_color_losses_on_the_emulator(color_emulator, tag, channels):
    """ops.color_losses through the C ABI: NHWC image with padding channels, strided background plane, device gradient scalars."""
    from michigan_amd import ops
    fx = pair(tag)
    n, _, h, w = fx["fake"].shape
    img = torch.zeros(n, h, w, channels)
    img[..., :3] = fx["fake"].permute(0, 2, 3, 1)
    img[..., 3:] = 7.0                                                       # padding channels are not read
    img.requires_grad_(True)
    sem = torch.stack([fx["back"].float(), 1 - fx["back"].float()], dim=1)
    lab, rgb, back = ops.color_losses(img, fx["real"], sem[:, 0], 7)
    wl, wr, wb = fx["weights"].tolist()
    (wl * lab + wr * rgb + wb * back).backward()
    for got, want in zip((lab, rgb, back), fx["losses"]):
        assert abs(float(got.detach()) - float(want)) <= 2e-7 * float(want)  # one rounding to the fp32 output
    g = img.grad
    assert float(g[..., 3:].abs().max()) == 0.0 if channels > 3 else True
    want = fx["grad"].permute(0, 2, 3, 1)
    assert float((g[..., :3].double() - want).norm() / want.norm()) <= 2e-7
    assert color_emulator.flags("mg_color_loss_fwd") == [7] and color_emulator.flags("mg_color_loss_bwd") == [7]


def test_loss_classes_alone_and_balance_lab(color_emulator):
    from michigan_amd import networks
    from michigan_amd.model import default_options
    fx = pair("ii")
    sem = torch.stack([fx["back"].float(), 1 - fx["back"].float()], dim=1)
    fake = fx["fake"].clone().requires_grad_(True)                           # plain contiguous NCHW, as the reference's trainer hands over
    lab = networks.LabColorLoss(default_options(gpu_ids=[]))(fake, fx["real"], sem[:, 1:2])
    bg = networks.RGBBackgroundL1Loss()(fake, sem, fx["real"])
    assert color_emulator.flags("mg_color_loss_fwd") == [1, 4]                       # one bit each
    assert abs(float(lab.detach()) - float(fx["losses"][0])) <= 2e-7 * float(fx["losses"][0])
    assert abs(float(bg.detach()) - float(fx["losses"][2])) <= 2e-7 * float(fx["losses"][2])
    (lab + bg).backward()
    assert fake.grad.shape == fake.shape and float(fake.grad.abs().max()) > 0
    # the generator's output: an NCHW view of NHWC memory, bf16
    nhwc = torch.zeros(2, 96, 80, 8, dtype=torch.bfloat16)
    nhwc[..., :3] = fx["fake"].permute(0, 2, 3, 1).to(torch.bfloat16)
    view = nhwc.permute(0, 3, 1, 2)[:, :3]
    want = K.color_terms(nhwc[..., :3].permute(0, 3, 1, 2).float(), fx["real"], None, 1)[0][0]
    got = networks.LabColorLoss(default_options(gpu_ids=[]))(view, fx["real"])
    assert abs(float(got) - float(want)) <= 2e-7 * float(want)
    with pytest.raises(NotImplementedError, match="balance_Lab"):
        networks.LabColorLoss(default_options(gpu_ids=[], balance_Lab=True))


def test_entry_points_validate_their_arguments_without_a_gpu():
    """Like tests/test_cabi_host.py: the real library, arguments refused before anything touches a device."""
    from michigan_amd import _cabi, build
    be = _cabi.HipBackend(build.build(verbose=False))
    ok = dict(img=64, real=64, rs=3 * 64, back=None, bs=0, dtype=_cabi.MG_F32, N=1, H=8, W=8, C=8, flags=1, out=64, ws=64)
    def fwd(**over):
        a = dict(ok, **over)
        return be.mg_color_loss_fwd(a["img"], a["real"], a["rs"], a["back"], a["bs"], a["dtype"], a["N"], a["H"], a["W"], a["C"], a["flags"],
                                    a["out"], a["ws"], None)
    with pytest.raises(RuntimeError, match="null pointer"):
        fwd(img=None)
    with pytest.raises(RuntimeError, match="flags"):
        fwd(flags=0)
    with pytest.raises(RuntimeError, match="flags"):
        fwd(flags=8)
    with pytest.raises(RuntimeError, match="label plane"):
        fwd(flags=5)
    with pytest.raises(RuntimeError, match="bad geometry"):
        fwd(C=2)
    with pytest.raises(RuntimeError, match="three dense planes"):
        fwd(rs=64)
    with pytest.raises(RuntimeError, match="bad dtype"):
        fwd(dtype=7)
    with pytest.raises(RuntimeError, match="null pointer"):
        be.mg_color_loss_bwd(64, 64, 3 * 64, None, 0, None, None, None, _cabi.MG_BF16, 1, 8, 8, 8, 1, None, None)


def _generator_step(color_emulator, same_ref=True, **over):
    from michigan_amd.model import Pix2PixModel
    from michigan_amd.synth import synth_loader_batch
    torch.manual_seed(0)
    model = Pix2PixModel(TP.repo_options(dict(TP.CFGS["A"], ngf=8, ndf=8, crop=64), **over))
    data = synth_loader_batch(1, 64, seed=3)
    if not same_ref:
        data["label_ref"] = data["label_ref"].clone()
        data["label_ref"][:, :, :32] = 0                                     # a hair mask of another area: sum(tag - ref) != 0 (pix2pix_model.py:286)
        assert float((data["label_ref"] - data["label_tag"]).sum()) != 0
    color_emulator.calls.clear()
    losses, fake = model(data, mode="generator")
    return losses, fake, data


def test_model_adds_the_keys_under_the_reference_conditions(color_emulator):
    """pix2pix_model.py:317-336: `curr_step == 1 and ref_is_tag`, one switch per term; off by default."""
    base = {"GAN", "GAN_Feat", "VGG", "ORIENT"}
    losses, _, _ = _generator_step(color_emulator)
    assert set(losses) == base and color_emulator.flags("mg_color_loss_fwd") == []             # default_options(): all three off
    subsets = {1: {"lab"}, 2: {"rgb"}, 4: {"background"}, 3: {"lab", "rgb"}, 5: {"lab", "background"}, 6: {"rgb", "background"},
               7: {"lab", "rgb", "background"}}
    for flags, keys in subsets.items():
        losses, _, _ = _generator_step(color_emulator, no_lab_loss=not flags & 1, no_rgb_loss=not flags & 2, no_background_loss=not flags & 4)
        assert set(losses) == base | keys, (flags, set(losses))
        assert color_emulator.flags("mg_color_loss_fwd") == [flags]                            # ONE call per generator step, union of the bits
    on = dict(no_lab_loss=False, no_rgb_loss=False, no_background_loss=False)
    losses, _, _ = _generator_step(color_emulator, same_ref=False, **on)
    assert not {"lab", "rgb", "background"} & set(losses) and color_emulator.flags("mg_color_loss_fwd") == []   # ref_is_tag false
    losses, _, _ = _generator_step(color_emulator, curr_step=2, **on)
    assert not {"lab", "rgb", "background"} & set(losses) and color_emulator.flags("mg_color_loss_fwd") == []   # unpaired step
    from michigan_amd.model import Pix2PixModel
    with pytest.raises(NotImplementedError, match="balance_Lab"):
        Pix2PixModel(TP.repo_options(dict(TP.CFGS["A"], ngf=8, ndf=8, crop=64), no_lab_loss=False, balance_Lab=True))


def test_model_losses_are_the_contract_values_times_lambda(color_emulator):
    losses, fake, data = _generator_step(color_emulator, no_lab_loss=False, no_rgb_loss=False, no_background_loss=False,
                                         lambda_lab=0.5, lambda_rgb=2.0, lambda_background=3.0)
    back = (data["label_tag"][:, 0] == 0).float()                            # channel 0 of the one-hot label
    want = K.color_terms(fake.detach().float(), data["image_tag"], back, 7)[0]
    for key, k, lam in (("lab", 0, 0.5), ("rgb", 1, 2.0), ("background", 2, 3.0)):
        assert abs(float(losses[key].detach()) - lam * float(want[k])) <= 1e-6 * lam * float(want[k]), key


@needs_reference
def test_reference_trainer_with_published_flags_over_dropin(color_emulator):
    """The README training command as published (Lab on; here background and rgb on as well) through dropin.install(): the
    reference's unmodified option parser, trainer and model.  No __rsub__ shim: the patched LabColorLoss makes it unnecessary."""
    R.setup()
    import michigan_amd.dropin as dropin
    from michigan_amd import networks as hip
    dropin.install(compute_dtype="fp32")
    try:
        from trainers.pix2pix_trainer import Pix2PixTrainer
        cfg = dict(TP.CFGS["A"], tag="C")
        with tempfile.TemporaryDirectory() as ck:
            opt = R.reference_options(CE.color_argv(cfg, ck), train=True)
            assert not opt.no_lab_loss and not opt.no_rgb_loss and not opt.no_background_loss
            torch.manual_seed(0)
            trainer = Pix2PixTrainer(opt)
            m = trainer.pix2pix_model_on_one_gpu
            assert isinstance(m.criterionLabL1, hip.LabColorLoss) and isinstance(m.criterionBackground, hip.RGBBackgroundL1Loss)
            TP.load_weights(trainer, cfg)
            rec = CE.drive_with_color_losses(trainer, cfg)
        assert color_emulator.flags("mg_color_loss_fwd") == [4, 1] * cfg["iters"]              # the reference calls the two classes separately
    finally:
        dropin.uninstall()
    import models.networks as N
    assert not issubclass(N.LabColorLoss, hip.LabColorLoss)                            # uninstall() put the reference's back
    TP.compare(rec, PU.load_trainer_golden("C"), **TOL)


def test_repo_trainer_matches_reference_golden_with_color_losses(color_emulator):
    from michigan_amd.model import Pix2PixTrainer
    cfg = dict(TP.CFGS["A"], tag="C")
    torch.manual_seed(0)
    trainer = Pix2PixTrainer(TP.repo_options(cfg, no_lab_loss=False, no_rgb_loss=False, no_background_loss=False))
    TP.load_weights(trainer, cfg)
    rec = CE.drive_with_color_losses(trainer, cfg)
    assert color_emulator.flags("mg_color_loss_fwd") == [7] * cfg["iters"]
    gold = PU.load_trainer_golden("C")
    assert all(("it%d.loss.%s" % (it, k)) in gold for it in range(cfg["iters"]) for k in CE.COLOR_KEYS)
    TP.compare(rec, gold, **TOL)
