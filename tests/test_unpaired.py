"""CPU: the unpaired training stage (unpairTrain, curr_step = 2) through every host layer, on the float64 contract emulator of
mg_hair_lab_fwd / mg_hair_lab_bwd (oracle/cabi_emulator.py, oracle/contracts.py), against what the REFERENCE's own classes and trainer computed
(tests/golden/hair_lab_{i,ii}.npz, trainer_U*.npz from tools/make_unpaired_golden.py).

  1  the emulator contract vs the reference's float64 run: pins the contract in include/michigan_hip.h to the reference;
  2  ops.hair_lab_losses through the C ABI (padding channels, strided planes, flag subsets, call counts);
  3  networks.HairAvgLabLoss; 4 the real library's argument checks and ABI number;
  5  Pix2PixModel / create_optimizers: keys, one fused call, netD2 vs netD;  6 checkpoints;  7 synth(unpaired=True);
  8  this package's trainer vs trainer_U;  9 the reference's trainer with --unpairTrain over dropin.install() vs trainer_U;
  10 two ranks over gloo.
The kernels themselves are checked on the GPU (tests/test_gpu_unpaired.py).
"""
import os
import socket
import tempfile

import pytest
import torch

import hair_lab_fixtures as HE
import parity_utils as PU
from oracle import contracts as K
from oracle import ref_harness as R
from oracle import trainer_parity as TP
from oracle.cabi_emulator import EmulatorBackend

needs_reference = pytest.mark.skipif(not R.reference_available(), reason="reference checkout not present")
# tests/test_color_loss.py::TOL (tests/test_dropin.py's emulator leg)
TOL = dict(rtol_loss0=2e-4, rtol_later=1e-2, atol_img=2e-4, atol_weight=2 * 4e-4 * 2 + 1e-5)
SMALL = dict(TP.CFGS["A"], ngf=8, ndf=8, crop=64)

pair = HE.load_pair


@pytest.fixture
def hair_emulator():
    from michigan_amd import _cabi
    be = EmulatorBackend()
    prev = _cabi.set_backend(be)
    yield be
    _cabi.set_backend(prev)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["i", "ii"])
def test_contract_matches_the_reference_in_float64(tag):
    fx = pair(tag)
    made = HE.make_pairs()[tag]
    assert all(torch.equal(made[k], fx[k]) for k in made), "the committed inputs are the seeded ones"
    losses, grad, (da, db) = K.hair_terms(fx["fake"], fx["ref"], fx["m_f"], fx["m_r"], fx["tgt"], fx["m_b"], 3, tuple(fx["weights"].tolist()))
    for k in range(2):
        assert abs(float(losses[k]) - float(fx["losses"][k])) <= 1e-9 * abs(float(fx["losses"][k])), (k, losses, fx["losses"])
    assert float((grad - fx["grad"]).norm() / fx["grad"].norm()) <= 1e-9                # every element
    assert float((da - fx["da"]).abs().max()) <= 1e-9 * float(fx["da"].abs().max()) and float((db - fx["db"]).abs().max()) <= 1e-9 * float(fx["db"].abs().max())
    assert float(torch.cat([fx["da"], fx["db"]]).abs().min()) >= 1.0                     # what the fixture generator asserted
    hair_only = K.hair_terms(fx["fake"], fx["ref"], fx["m_f"], fx["m_r"], flags=1)[1]
    assert float((hair_only * (fx["m_f"] == 0).unsqueeze(1)).abs().max()) == 0.0
    if tag == "ii":
        # "the mask value multiplies": reading the 0.5 rows as a predicate moves a weighted MEAN only a little (6e-4 here), but that is
        # 10^5 times the 1e-9 the comparison above allows -- the fixture tells the two readings apart
        pred = K.hair_terms(fx["fake"], fx["ref"], (fx["m_f"] != 0).float(), fx["m_r"], flags=1)[0][0]
        assert abs(float(pred) - float(fx["losses"][0])) > 1e-6 * float(fx["losses"][0])


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
def _label(fx):
    """The NCHW one-hot tag label (channel 0 = background, 1 = hair) and the reference label: their channel views are strided planes."""
    return torch.stack([fx["m_b"], fx["m_f"]], dim=1).contiguous(), torch.stack([1 - fx["m_r"], fx["m_r"]], dim=1).contiguous()


@pytest.mark.parametrize("tag", ["i", "ii"])
@pytest.mark.parametrize("channels", [3, 8])
@pytest.mark.parametrize("flags", [1, 2, 3])
def test_ops_hair_lab_losses_on_the_emulator(hair_emulator, tag, channels, flags):
    from michigan_amd import ops
    assert (ops.HAIR_LAB, ops.HAIR_BACKGROUND) == (1, 2)
    fx = pair(tag)
    n, _, h, w = fx["fake"].shape
    img = torch.zeros(n, h, w, channels)
    img[..., :3] = fx["fake"].permute(0, 2, 3, 1)
    img[..., 3:] = float("nan")                                              # padding channels are not read
    img.requires_grad_(True)
    sem_tag, sem_ref = _label(fx)
    assert not sem_tag[:, 1].is_contiguous()
    hair, back = ops.hair_lab_losses(img, fx["ref"], sem_tag[:, 1], sem_ref[:, 1], fx["tgt"], sem_tag[:, 0], flags=flags)
    wh, wb = fx["weights"].tolist()
    (wh * hair + wb * back).backward()
    want_l, want_g, _ = K.hair_terms(fx["fake"], fx["ref"], fx["m_f"], fx["m_r"], fx["tgt"], fx["m_b"], flags, (wh, wb))
    for k, got in enumerate((hair, back)):
        if flags & (1 << k):
            assert abs(float(got.detach()) - float(fx["losses"][k])) <= 2e-7 * float(fx["losses"][k])       # one rounding to the fp32 output
        else:
            assert float(got.detach()) == 0.0
    g = img.grad
    if channels > 3:
        assert float(g[..., 3:].abs().max()) == 0.0
    want = want_g.permute(0, 2, 3, 1)
    assert float((g[..., :3].double() - want).norm() / want.norm()) <= 2e-7
    if flags == 3:
        assert float((g[..., :3].double() - fx["grad"].permute(0, 2, 3, 1)).norm() / fx["grad"].norm()) <= 2e-7
    assert hair_emulator.flags("mg_hair_lab_fwd") == [flags] and hair_emulator.flags("mg_hair_lab_bwd") == [flags]       # one forward and one backward call
    assert hair_emulator.flags("mg_color_loss_fwd") == [] and hair_emulator.flags("mg_color_loss_bwd") == []


def test_ops_hair_lab_losses_checks_and_lazy_backward(hair_emulator):
    from michigan_amd import ops
    fx = pair("i")
    img = fx["fake"].permute(0, 2, 3, 1).contiguous().requires_grad_(True)
    sem_tag, sem_ref = _label(fx)
    with pytest.raises(ValueError, match="flags"):
        ops.hair_lab_losses(img, fx["ref"], sem_tag[:, 1], sem_ref[:, 1], flags=0)
    with pytest.raises(ValueError, match="flags"):
        ops.hair_lab_losses(img, fx["ref"], sem_tag[:, 1], sem_ref[:, 1], flags=4)
    with pytest.raises(ValueError, match="image_tag"):
        ops.hair_lab_losses(img, fx["ref"], sem_tag[:, 1], sem_ref[:, 1], flags=3)
    with pytest.raises(ValueError, match="does not match"):
        ops.hair_lab_losses(img, fx["ref"][:, :, :-1], sem_tag[:, 1], sem_ref[:, 1], flags=1)
    with pytest.raises(ValueError, match="does not match"):
        ops.hair_lab_losses(img, fx["ref"], sem_tag[:, 1, :-1], sem_ref[:, 1], flags=1)
    # terms not selected need no operands; nothing flows back when no gradient arrives
    hair, back = ops.hair_lab_losses(img, None, None, None, fx["tgt"], sem_tag[:, 0], flags=ops.HAIR_BACKGROUND)
    assert float(hair.detach()) == 0.0 and hair_emulator.flags("mg_hair_lab_fwd") == [2]
    hair, back = ops.hair_lab_losses(img, fx["ref"], sem_tag[:, 1], sem_ref[:, 1], fx["tgt"], sem_tag[:, 0], flags=3)
    (img.sum() * 0 + 1.0).backward()
    assert hair_emulator.flags("mg_hair_lab_bwd") == []
    hair.backward()                                                          # only one of the two gradients arrives: the other is a NULL pointer
    assert hair_emulator.flags("mg_hair_lab_bwd") == [3]
    want = K.hair_terms(fx["fake"], fx["ref"], fx["m_f"], fx["m_r"], flags=1)[1].permute(0, 2, 3, 1)
    assert float((img.grad.double() - want).norm() / want.norm()) <= 2e-7


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
def test_loss_class_alone_and_balance_lab(hair_emulator):
    from michigan_amd import networks
    from michigan_amd.model import default_options
    fx = pair("ii")
    fake = fx["fake"].clone().requires_grad_(True)                           # plain contiguous NCHW, as the reference's trainer hands over
    crit = networks.HairAvgLabLoss(default_options(gpu_ids=[]))
    got = crit(fake, fx["ref"], fx["m_f"].unsqueeze(1), fx["m_r"].unsqueeze(1))
    assert hair_emulator.flags("mg_hair_lab_fwd") == [1]
    assert abs(float(got.detach()) - float(fx["losses"][0])) <= 2e-7 * float(fx["losses"][0])
    got.backward()
    want = K.hair_terms(fx["fake"], fx["ref"], fx["m_f"], fx["m_r"], flags=1)[1]
    assert fake.grad.shape == fake.shape and float((fake.grad.double() - want).norm() / want.norm()) <= 2e-7
    # the generator's output: an NCHW view of NHWC memory, bf16
    nhwc = torch.zeros(2, HE.H, HE.W, 8, dtype=torch.bfloat16)
    nhwc[..., :3] = fx["fake"].permute(0, 2, 3, 1).to(torch.bfloat16)
    view = nhwc.permute(0, 3, 1, 2)[:, :3]
    want = K.hair_terms(nhwc[..., :3].permute(0, 3, 1, 2).float(), fx["ref"], fx["m_f"], fx["m_r"], flags=1)[0][0]
    got = crit(view, fx["ref"], fx["m_f"].unsqueeze(1), fx["m_r"].unsqueeze(1))
    assert abs(float(got) - float(want)) <= 2e-7 * float(want)
    with pytest.raises(NotImplementedError, match="balance_Lab"):
        networks.HairAvgLabLoss(default_options(gpu_ids=[], balance_Lab=True))


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
def test_entry_points_validate_their_arguments_without_a_gpu():
    """Like tests/test_cabi_host.py: the real library, arguments refused before anything touches a device."""
    from michigan_amd import _cabi, build
    be = _cabi.HipBackend(build.build(verbose=False))
    assert be.mg_abi_version() == 10 and _cabi.MG_ABI_VERSION == 10
    ok = dict(img=64, ref=64, rs=3 * 64, mf=64, fs=64, mr=64, ms=64, tgt=64, ts=3 * 64, back=64, bs=64, dtype=_cabi.MG_F32, N=1, H=8, W=8, C=8,
              flags=3, out=64, stats=64, ws=64)

    def fwd(**over):
        a = dict(ok, **over)
        return be.mg_hair_lab_fwd(a["img"], a["ref"], a["rs"], a["mf"], a["fs"], a["mr"], a["ms"], a["tgt"], a["ts"], a["back"], a["bs"], a["dtype"],
                                  a["N"], a["H"], a["W"], a["C"], a["flags"], a["out"], a["stats"], a["ws"], None)

    def bwd(**over):
        a = dict(ok, **over)
        return be.mg_hair_lab_bwd(a["img"], a["mf"], a["fs"], a["tgt"], a["ts"], a["back"], a["bs"], a["stats"], None, None, a["dtype"],
                                  a["N"], a["H"], a["W"], a["C"], a["flags"], a.get("dimg"), None)
    for call in (fwd, lambda **o: bwd(dimg=64, **o)):
        with pytest.raises(RuntimeError, match="null pointer"):
            call(img=None)
        with pytest.raises(RuntimeError, match="flags"):
            call(flags=0)
        with pytest.raises(RuntimeError, match="flags"):
            call(flags=4)
        with pytest.raises(RuntimeError, match="bad geometry"):
            call(C=2)
        with pytest.raises(RuntimeError, match="bad geometry"):
            call(N=0)
        with pytest.raises(RuntimeError, match="bad dtype"):
            call(dtype=7)
        with pytest.raises(RuntimeError, match="tag hair plane"):
            call(fs=63)                                                      # a plane stride smaller than H*W
        with pytest.raises(RuntimeError, match="tag hair plane"):
            call(mf=None)
        with pytest.raises(RuntimeError, match="label plane"):
            call(bs=8)
        with pytest.raises(RuntimeError, match="three dense planes"):
            call(ts=2 * 64)                                                  # an image stride smaller than 3*H*W
        with pytest.raises(RuntimeError, match="stats"):
            call(stats=None)
    with pytest.raises(RuntimeError, match="three dense planes"):
        fwd(rs=64)
    with pytest.raises(RuntimeError, match="reference hair plane"):
        fwd(mr=None)
    with pytest.raises(RuntimeError, match="null pointer"):
        fwd(ws=None)
    with pytest.raises(RuntimeError, match="null pointer"):
        bwd(dimg=None)
    # a term whose bit is clear needs no operands: with them NULL the checks get as far as the last one (no call here is valid as a
    # whole -- a valid one would launch on whatever these made-up addresses are)
    with pytest.raises(RuntimeError, match="reference hair plane"):
        fwd(flags=1, tgt=None, ts=0, back=None, bs=0, mr=None)
    with pytest.raises(RuntimeError, match=r"null pointer \(ws\)"):
        fwd(flags=2, ref=None, rs=0, mf=None, fs=0, mr=None, ms=0, stats=None, ws=None)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
def _model(**over):
    from michigan_amd.model import Pix2PixModel
    torch.manual_seed(0)
    return Pix2PixModel(TP.repo_options(SMALL, **over))


def _batch(unpaired=True):
    from michigan_amd.synth import synth_loader_batch
    return synth_loader_batch(1, 64, seed=3, unpaired=unpaired)


def test_model_step_two_objective_and_call_counts(hair_emulator):
    """pix2pix_model.py:352-363: hairAvgLab + background exactly at `unpairTrain and curr_step == 2`, from ONE fused call."""
    model = _model(unpairTrain=True, curr_step=2, lambda_hairavglab=0.5, lambda_background=3.0)
    assert model.netD2 is not None and hasattr(model, "criterionHairAvgLab")
    data = _batch()
    losses, fake = model(data, mode="generator")
    assert set(losses) == {"GAN", "ORIENT", "hairAvgLab", "background"}
    assert hair_emulator.flags("mg_hair_lab_fwd") == [3] and hair_emulator.flags("mg_color_loss_fwd") == []
    hair_tag, hair_ref = (data["label_tag"][:, 0] != 0).float(), (data["label_ref"][:, 0] != 0).float()
    want = K.hair_terms(fake.detach().float(), data["image_ref"], hair_tag, hair_ref, data["image_tag"], 1 - hair_tag, 3)[0]
    for key, k, lam in (("hairAvgLab", 0, 0.5), ("background", 1, 3.0)):
        assert abs(float(losses[key].detach()) - lam * float(want[k])) <= 1e-6 * lam * float(want[k]), key
    sum(losses.values()).backward()
    assert hair_emulator.flags("mg_hair_lab_fwd") == [3] and hair_emulator.flags("mg_hair_lab_bwd") == [3]               # 2 + 1 launches for the two image-space terms
    # the paired half of the same model: no fused call, the usual keys
    model.opt.curr_step = 1
    losses, _ = model(_batch(unpaired=False), mode="generator")
    assert set(losses) == {"GAN", "GAN_Feat", "VGG", "ORIENT"} and hair_emulator.flags("mg_hair_lab_fwd") == [3]
    # curr_step = 2 WITHOUT unpairTrain: GAN + ORIENT only (the reference's condition), no netD2
    plain = _model(curr_step=2)
    assert plain.netD2 is None and not hasattr(plain, "criterionHairAvgLab")
    losses, _ = plain(_batch(), mode="generator")
    assert set(losses) == {"GAN", "ORIENT"} and hair_emulator.flags("mg_hair_lab_fwd") == [3]
    # background is added at step 2 whatever no_background_loss says, and not twice
    assert TP.repo_options(SMALL).no_background_loss and not TP.repo_options(SMALL).unpairTrain
    from michigan_amd.model import default_options
    o = default_options()
    assert (o.unpairTrain, o.lambda_hairavglab, o.same_netD_model) == (False, 1.0, False)


def test_discriminator_steps_train_the_discriminator_in_use(hair_emulator):
    model = _model(unpairTrain=True, curr_step=2)
    params = lambda net: {k: v.detach().clone() for k, v in net.state_dict().items()}
    for step, used, idle in ((2, "netD2", "netD"), (1, "netD", "netD2")):
        model.opt.curr_step = step
        model.zero_grad(set_to_none=True)
        before = params(getattr(model, idle))
        losses = model(_batch(unpaired=step == 2), mode="discriminator")
        assert set(losses) == {"D_Fake", "D_real"}
        sum(losses.values()).backward()
        assert all(p.grad is None for p in getattr(model, idle).parameters()), "step %d: the idle discriminator got gradients" % step
        assert any(p.grad is not None and float(p.grad.abs().max()) > 0 for p in getattr(model, used).parameters())
        assert all(torch.equal(v, before[k]) for k, v in getattr(model, idle).state_dict().items()), "spectral-norm vectors of the idle net moved"
    # the generator step's GAN term is scored by the discriminator in use as well (split form: fake with a graph, real under no_grad)
    model.opt.curr_step = 2
    before = params(model.netD)
    u_before = {k: v.clone() for k, v in model.netD2.state_dict().items() if k.endswith("weight_u")}
    model(_batch(), mode="generator")
    assert all(torch.equal(v, before[k]) for k, v in model.netD.state_dict().items())
    assert any(not torch.equal(v, model.netD2.state_dict()[k]) for k, v in u_before.items()), "netD2's power iteration did not run"


def test_create_optimizers_arity_and_trainer_wiring(hair_emulator):
    from michigan_amd.model import Pix2PixTrainer
    opt = TP.repo_options(SMALL)
    torch.manual_seed(0)
    plain = Pix2PixTrainer(opt)
    assert len(plain.pix2pix_model.create_optimizers(opt)) == 2 and plain.optimizer_D2 is None
    opt = TP.repo_options(SMALL, unpairTrain=True)
    torch.manual_seed(0)
    tr = Pix2PixTrainer(opt)
    optimizers = tr.pix2pix_model.create_optimizers(opt)
    assert len(optimizers) == 3
    assert optimizers[2].param_groups[0]["lr"] == optimizers[1].param_groups[0]["lr"] == opt.lr * 2
    assert {id(p) for p in tr.optimizer_D2.params} == {id(p) for p in tr.pix2pix_model.netD2.parameters()}
    tr.g_losses, tr.d_losses = {"x": 1}, {"y": 2}
    tr.init_losses()
    assert tr.get_latest_losses() == {}
    # update_learning_rate leaves optimizer_D2 alone, as the reference does (pix2pix_trainer.py:99-119)
    tr.opt.niter, tr.opt.niter_decay = 1, 2
    tr.update_learning_rate(2)
    assert tr.optimizer_D.param_groups[0]["lr"] == pytest.approx(opt.lr) and tr.optimizer_D2.param_groups[0]["lr"] == opt.lr * 2


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip_of_netD2(hair_emulator):
    from michigan_amd.model import Pix2PixTrainer
    with tempfile.TemporaryDirectory() as ck:
        os.makedirs(os.path.join(ck, "u"))
        mk = lambda seed, **over: (torch.manual_seed(seed), Pix2PixTrainer(TP.repo_options(SMALL, unpairTrain=True, checkpoints_dir=ck, name="u", **over)))[1]
        a = mk(1, curr_step=2)
        data = _batch()
        a.run_generator_one_step(data)
        a.run_discriminator_one_step(data)                                   # optimizer_D2 has state now
        a.save("7")
        assert sorted(os.listdir(os.path.join(ck, "u"))) == ["7_net_D.pth", "7_net_D2.pth", "7_net_G.pth", "7_optim.pth"]
        assert set(torch.load(os.path.join(ck, "u", "7_optim.pth"))) == {"G", "D", "D2", "old_lr"}
        b = mk(2)
        ma, mb = a.pix2pix_model, b.pix2pix_model
        assert not all(torch.equal(v, mb.netD2.state_dict()[k]) for k, v in ma.netD2.state_dict().items())
        b.load("7")
        for net in ("netG", "netD", "netD2"):
            assert all(torch.equal(v, getattr(mb, net).state_dict()[k]) for k, v in getattr(ma, net).state_dict().items()), net
        sa, sb = a.optimizer_D2.state_dict(), b.optimizer_D2.state_dict()
        assert sa["state"].keys() == sb["state"].keys() and len(sa["state"]) > 0
        for i in sa["state"]:
            for k, v in sa["state"][i].items():
                assert torch.equal(torch.as_tensor(v), torch.as_tensor(sb["state"][i][k])), (i, k)
        # same_netD_model: netD2 starts from the D file
        c = mk(3, same_netD_model=True)
        c.load("7")
        mc = c.pix2pix_model
        assert all(torch.equal(v, mc.netD2.state_dict()[k]) for k, v in ma.netD.state_dict().items())
        # a checkpoint of a paired-only run has no D2 file: fall back to the D file
        os.remove(os.path.join(ck, "u", "7_net_D2.pth"))
        d = mk(4)
        d.load("7")
        assert all(torch.equal(v, d.pix2pix_model.netD2.state_dict()[k]) for k, v in ma.netD.state_dict().items())
        # without unpairTrain nothing about D2 is written
        torch.manual_seed(5)
        p = Pix2PixTrainer(TP.repo_options(SMALL, checkpoints_dir=ck, name="p"))
        os.makedirs(os.path.join(ck, "p"))
        p.save("1")
        assert sorted(os.listdir(os.path.join(ck, "p"))) == ["1_net_D.pth", "1_net_G.pth", "1_optim.pth"]
        assert set(torch.load(os.path.join(ck, "p", "1_optim.pth"))) == {"G", "D", "old_lr"}


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------
def test_synth_unpaired_batches():
    from michigan_amd.synth import synth_batch, synth_loader_batch
    for fn, ref_keys in ((synth_batch, ("input_ref", "image_ref")), (synth_loader_batch, ("label_ref", "image_ref"))):
        a, b = fn(2, 64, seed=5), fn(2, 64, seed=5, unpaired=True)
        for k, v in a.items():
            if torch.is_tensor(v) and k not in ref_keys:
                assert torch.equal(v, b[k]), k                               # every tag tensor bit-identical to the default call
        for k in ref_keys:
            assert not torch.equal(a[k], b[k]), k
    b = synth_batch(2, 64, seed=5, unpaired=True)
    assert float((b["input_tag"][:, 1] - b["input_ref"][:, 1]).sum()) != 0
    b = synth_loader_batch(2, 64, seed=5, unpaired=True)
    assert float((b["label_tag"] - b["label_ref"]).sum()) != 0 and float((b["image_tag"] - b["image_ref"]).abs().sum()) != 0
    assert set(b["label_ref"].unique().tolist()) == {0.0, 1.0}


# ---- 8, 9 ------------------------------------------------------------------------------------------------------------------------
def _check_record(rec, gold, cfg):
    assert all(("it%d.loss.%s" % (it, k)) in gold for it in range(cfg["iters"]) for k in HE.STEP2_KEYS)
    assert all(("it%dp.loss.%s" % (it, k)) in gold for it in range(cfg["iters"]) for k in TP.LOSS_KEYS)
    assert all(("D.2." + k) in gold for k in TP.D_WEIGHTS + TP.D_BUFFERS)
    assert {k for k in rec if ".loss." in k} == {k for k in gold if ".loss." in k}, "the trainer reports other losses than the reference"
    TP.compare(rec, gold, **TOL)


def test_repo_trainer_matches_reference_golden_unpaired(hair_emulator):
    from michigan_amd.model import Pix2PixTrainer
    cfg = dict(TP.CFGS["A"], tag="U")
    torch.manual_seed(0)
    trainer = Pix2PixTrainer(TP.repo_options(cfg, unpairTrain=True))
    HE.load_weights(trainer, cfg)
    rec = HE.drive_unpaired(trainer, cfg)
    assert hair_emulator.flags("mg_hair_lab_fwd") == [3] * cfg["iters"] and hair_emulator.flags("mg_hair_lab_bwd") == [3] * cfg["iters"]     # one fused call per step-2 generator step
    assert hair_emulator.flags("mg_color_loss_fwd") == []
    _check_record(rec, PU.load_trainer_golden("U"), cfg)


@needs_reference
def test_reference_trainer_with_unpair_train_over_dropin(hair_emulator):
    """`train.py --unpairTrain` in miniature through dropin.install(): the reference's unmodified option parser, trainer and model.
    No __rsub__ shim: the reference's own HairAvgLabLoss raises on this torch, the patched one makes the stage run."""
    R.setup()
    import michigan_amd.dropin as dropin
    from michigan_amd import networks as hip
    import models.networks.loss as RL
    ref_cls = RL.HairAvgLabLoss
    import types
    fx = pair("i")
    with pytest.raises((RuntimeError, TypeError)):                                       # `1 - mask` on a bool mask (loss.py:546)
        ref_cls(types.SimpleNamespace(balance_Lab=False))(fx["fake"], fx["ref"], fx["m_f"].unsqueeze(1), fx["m_r"].unsqueeze(1))
    dropin.install(compute_dtype="fp32")
    try:
        from trainers.pix2pix_trainer import Pix2PixTrainer
        cfg = dict(TP.CFGS["A"], tag="U")
        with tempfile.TemporaryDirectory() as ck:
            opt = R.reference_options(HE.unpaired_argv(cfg, ck), train=True)
            assert opt.unpairTrain
            torch.manual_seed(0)
            trainer = Pix2PixTrainer(opt)
            m = trainer.pix2pix_model_on_one_gpu
            assert isinstance(m.criterionHairAvgLab, hip.HairAvgLabLoss) and isinstance(m.netD2, hip.MultiscaleDiscriminator)
            HE.load_weights(trainer, cfg)
            rec = HE.drive_unpaired(trainer, cfg)
        # the reference calls its two classes separately
        assert hair_emulator.flags("mg_hair_lab_fwd") == [1] * cfg["iters"] and hair_emulator.flags("mg_color_loss_fwd") == [4] * cfg["iters"]
    finally:
        dropin.uninstall()
    import models.networks as N
    assert N.HairAvgLabLoss is ref_cls and RL.HairAvgLabLoss is ref_cls                  # uninstall() put the reference's back
    _check_record(rec, PU.load_trainer_golden("U"), cfg)


# ---- 10 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
def test_two_ranks_over_gloo_keep_netG_and_netD2_identical():
    import torch.multiprocessing as mp
    import unpaired_dp_worker as worker
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=worker.run, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=600) for _ in range(2))
    for p in procs:
        p.join()
        assert p.exitcode == 0
    for rank in (0, 1):
        ok = got[rank]
        assert ok["keys"] == sorted(HE.STEP2_KEYS), ok
        assert ok["hair_fwd"] == [3] and ok["hair_bwd"] == [3], ok
        assert ok["replicas_identical"] and ok["netD_untouched"] and ok["netD2_moved"] and ok["netG_moved"], ok
