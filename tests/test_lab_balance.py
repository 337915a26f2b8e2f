"""CPU: the --balance_Lab weighting of the Lab colour loss and the hair-average Lab loss (include/michigan_hip/losses/lab_balance.h)
through every host layer, on the float64 contract of tests/lab_balance_fixtures.py, against what the REFERENCE's own classes computed
(tests/golden/lab_balance_{i,ii,hair}.npz, ab_count.npz, trainer_L*.npz from tools/make_lab_balance_golden.py).

  1  the contract vs the reference's float64 run; the table: ops.lab_weight_table bit for bit against the reference's cal_weight over
     all 65536 bin pairs and against the literal grid_sample expression;
  2  ops.color_losses / ops.hair_lab_losses on the emulator (C = 3 and C = 8), the loss classes alone and through the model;
  3  this package's trainer, and the reference's trainer over dropin.install(), against the reference trainer's record; the train driver;
  4  refusals: ops before any launch, the library before the device is touched; the header outside the ledger, the other tables unchanged.
The kernels themselves are checked on the GPU (tests/test_gpu_lab_balance.py).
"""
import ctypes
import os
import re
import tempfile

import numpy as np
import pytest
import torch

import lab_balance_fixtures as LB
import parity_utils as PU
from oracle import contracts as K
from oracle import ref_harness as R
from oracle import trainer_parity as TP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_reference = pytest.mark.skipif(not R.reference_available(), reason="reference checkout not present")
TOL = dict(rtol_loss0=2e-4, rtol_later=1e-2, atol_img=2e-4, atol_weight=2 * 4e-4 * 2 + 1e-5)      # tests/test_color_loss.py's emulator leg


@pytest.fixture
def emulator():
    from michigan_amd import _cabi
    be = LB.LabBalanceEmulator()
    prev = _cabi.set_backend(be)
    yield be
    _cabi.set_backend(prev)


def _sem(fx):
    return torch.stack([fx["back"].float(), fx["hair"].float()], dim=1)         # the one-hot label: channel 0 background, 1 hair


# ---- 1. the contract and the table -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["i", "ii"])
def test_colour_contract_matches_the_reference_in_float64(tag):
    fx = LB.load_pair(tag)
    losses, grad, _, w = LB.color_terms(fx["fake"], fx["real"], fx["back"].float(), fx["hair"].float(), fx["S"], 7, tuple(fx["weights"].tolist()))
    assert torch.equal(w.float(), fx["w"]), "a pixel's weight differs from the reference's cal_weight"
    for k in range(3):
        assert abs(float(losses[k]) - float(fx["losses"][k])) <= 1e-9 * abs(float(fx["losses"][k])), (k, losses, fx["losses"])
    assert float((grad - fx["grad"]).norm() / fx["grad"].norm()) <= 1e-9      # every pixel, the ones near a sign change included
    if tag == "ii":
        assert float(grad[:, :, 40:48, 24:32].abs().max()) == 0.0            # sign(0) = 0 where fake == real, whatever the weight
    # the fixture is what the issue asks of it
    on = fx["hair"] > 0
    assert float((fx["w"][on] < fx["th"]).double().mean()) >= 0.10 and int(torch.unique(fx["w"][on]).numel()) >= 30
    assert bool((fx["w"][~on] == 1).all()) and float(fx["excluded"].double().mean()) <= 5e-3
    assert fx["edge_margin"] >= 4 * fx["ref32_ab_err"]
    # without the weight the value is another one: the fixture notices a pass that ignores the table
    plain = K.color_terms(fx["fake"], fx["real"], fx["back"].float(), 7)[0][0]
    assert abs(float(plain) - float(fx["losses"][0])) > 0.1 * float(fx["losses"][0])


def test_hair_contract_matches_the_reference_in_float64():
    fx = LB.load_pair("hair")
    losses, grad, (da, db), w = LB.hair_terms(fx["fake"], fx["ref"], fx["m_f"], fx["m_r"], fx["S"], flags=1)
    assert torch.equal(w.float(), fx["w"]) and int(torch.unique(w).numel()) == 3
    assert abs(float(losses[0]) - float(fx["loss"])) <= 1e-9 * float(fx["loss"])
    assert float((grad - fx["grad"]).norm() / fx["grad"].norm()) <= 1e-9
    assert float((da - fx["da"]).abs().max()) <= 1e-9 and float((db - fx["db"]).abs().max()) <= 1e-9
    assert float(fx["m_r"][2].sum()) == 0 and float(fx["w"][2]) == float(fx["S"][128, 128])        # an empty reference mask: the mean is 0
    plain = K.hair_terms(fx["fake"], fx["ref"], fx["m_f"], fx["m_r"], flags=1)[0][0]
    assert abs(float(plain) - float(fx["loss"])) > 0.1 * float(fx["loss"])


@pytest.mark.parametrize("th", [10.0, 1e4, 2.5])
def test_weight_table_is_the_references_bit_for_bit(th):
    from michigan_amd import ops
    counts = LB.ab_count()
    assert counts.shape == (256, 256) and counts.dtype == np.float64
    seen = np.argwhere(counts > 0)                                            # the shipped histogram: where hair colours were counted at all
    assert (seen[:, 0].min(), seen[:, 0].max(), seen[:, 1].min(), seen[:, 1].max()) == (55, 226, 22, 222)
    S = ops.lab_weight_table(counts, th)
    assert S.dtype == torch.float32 and tuple(S.shape) == (256, 256) and S.is_contiguous()
    assert torch.equal(S, LB.grid_sample_table(counts, th)), "the definition differs from the literal grid_sample expression"
    assert torch.equal(S, LB.weight_table(counts, th))
    for tag in ("i", "ii", "hair"):
        fx = LB.load_pair(tag)
        if fx["th"] == th:
            assert torch.equal(S, fx["S"]), "the table differs from what the reference's cal_weight returned (%s)" % tag
    assert float(S[255].abs().max()) == 0.0 and float(S[:, 255].abs().max()) == 0.0                # bin 255 falls outside the table
    inner = S[:255, :255]
    assert float(inner.min()) == 1.0 and float(inner.max()) == min(th, float(inner.max())) <= th
    if th == 10.0:
        below = (inner < th).nonzero()
        assert len(below) == 74                                                                    # the shipped file: 74 bins below the cap,
        assert 0 < int(below.min()) and int(below.max()) < 255                                     # all of them inside the table
    assert torch.equal(ops.lab_weight_table(torch.from_numpy(counts), th), S)                      # a tensor is taken as well


def test_weight_table_refuses_bad_operands():
    from michigan_amd import ops
    counts = LB.ab_count()
    with pytest.raises(ValueError, match="256 x 256"):
        ops.lab_weight_table(counts[:255], 10.0)
    with pytest.raises(ValueError, match="256 x 256"):
        ops.lab_weight_table(counts.reshape(-1), 10.0)
    for bad in (np.nan, np.inf, -1.0):
        c = counts.copy()
        c[3, 4] = bad
        with pytest.raises(ValueError, match="finite and not negative"):
            ops.lab_weight_table(c, 10.0)
    for th in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="Lab_weight_th"):
            ops.lab_weight_table(counts, th)


# ---- 2. the operator, class and model layers ---------------------------------------------------------------------------------------------
def _image(fake, channels):
    n, _, h, w = fake.shape
    img = torch.zeros(n, h, w, channels)
    img[..., :3] = fake.permute(0, 2, 3, 1)
    img[..., 3:] = 7.0                                                       # padding channels are not read
    return img.requires_grad_(True)


@pytest.mark.parametrize("tag", ["i", "ii"])
@pytest.mark.parametrize("channels", [3, 8])
def test_ops_color_losses_balanced_on_the_emulator(emulator, tag, channels):
    from michigan_amd import ops
    fx = LB.load_pair(tag)
    img, sem = _image(fx["fake"], channels), _sem(fx)
    lab, rgb, back = ops.color_losses(img, fx["real"], sem[:, 0], 7, hair=sem[:, 1], table=fx["S"])         # strided planes of one label
    wl, wr, wb = fx["weights"].tolist()
    (wl * lab + wr * rgb + wb * back).backward()
    for got, want in zip((lab, rgb, back), fx["losses"]):
        assert abs(float(got.detach()) - float(want)) <= 2e-7 * float(want)  # one rounding to the fp32 output
    g = img.grad
    assert channels == 3 or float(g[..., 3:].abs().max()) == 0.0
    want = fx["grad"].permute(0, 2, 3, 1)
    assert float((g[..., :3].double() - want).norm() / want.norm()) <= 2e-7
    assert emulator.flags("mgc_color_loss_balanced_fwd") == [7] and emulator.flags("mgc_color_loss_balanced_bwd") == [7]
    assert emulator.count("mg_color_loss_fwd") == 0 and emulator.count("mg_color_loss_bwd") == 0
    # without a table: the unbalanced entry points, as before
    ops.color_losses(img, fx["real"], sem[:, 0], 7)[0].backward()
    assert emulator.flags("mg_color_loss_fwd") == [7] and emulator.flags("mg_color_loss_bwd") == [7]
    assert emulator.count("mgc_color_loss_balanced_fwd") == 1


@pytest.mark.parametrize("channels", [3, 8])
def test_ops_hair_lab_losses_balanced_on_the_emulator(emulator, channels):
    from michigan_amd import ops
    fx = LB.load_pair("hair")
    img = _image(fx["fake"], channels)
    tgt = fx["ref"].flip(0).contiguous()
    m_b = 1 - fx["m_f"]
    hair, back = ops.hair_lab_losses(img, fx["ref"], fx["m_f"], fx["m_r"], tgt, m_b, 3, table=fx["S"])
    (0.5 * hair + 2.0 * back).backward()
    want_l, want_g, _, _ = LB.hair_terms(fx["fake"], fx["ref"], fx["m_f"], fx["m_r"], fx["S"], tgt, m_b, 3, (0.5, 2.0))
    assert abs(float(hair.detach()) - float(fx["loss"])) <= 2e-7 * float(fx["loss"])
    assert abs(float(back.detach()) - float(want_l[1])) <= 2e-7 * float(want_l[1])
    g = img.grad
    assert channels == 3 or float(g[..., 3:].abs().max()) == 0.0
    want = want_g.permute(0, 2, 3, 1)
    assert float((g[..., :3].double() - want).norm() / want.norm()) <= 3e-7       # stats pass through fp32 once more
    assert emulator.flags("mgc_hair_lab_balanced_fwd") == [3] and emulator.flags("mgc_hair_lab_balanced_bwd") == [3]
    assert emulator.count("mg_hair_lab_fwd") == 0 and emulator.count("mg_hair_lab_bwd") == 0
    # the hair term alone against the reference's own gradient
    img2 = _image(fx["fake"], channels)
    ops.hair_lab_losses(img2, fx["ref"], fx["m_f"], fx["m_r"], flags=1, table=fx["S"])[0].backward()
    want = fx["grad"].permute(0, 2, 3, 1)
    assert float((img2.grad[..., :3].double() - want).norm() / want.norm()) <= 3e-7


def _opt(**over):
    from michigan_amd.model import default_options
    return default_options(gpu_ids=[], balance_Lab=True, weight_dir=LB.ab_count_path(), **over)


def test_loss_classes_alone(emulator):
    from michigan_amd import networks
    fx = LB.load_pair("i")
    sem = _sem(fx)
    fake = fx["fake"].clone().requires_grad_(True)                           # plain contiguous NCHW, as the reference's trainer hands over
    crit = networks.LabColorLoss(_opt())
    lab = crit(fake, fx["real"], sem[:, 1:2])
    assert abs(float(lab.detach()) - float(fx["losses"][0])) <= 2e-7 * float(fx["losses"][0])
    assert emulator.flags("mgc_color_loss_balanced_fwd") == [1]
    lab.backward()
    assert fake.grad.shape == fake.shape and float(fake.grad.abs().max()) > 0
    assert crit.balance.table("cpu") is crit.balance.table("cpu")            # built once
    with pytest.raises(ValueError, match="hair mask"):
        crit(fake, fx["real"])
    hx = LB.load_pair("hair")
    hcrit = networks.HairAvgLabLoss(_opt(Lab_weight_th=hx["th"]), balance=None)
    got = hcrit(hx["fake"], hx["ref"], hx["m_f"].unsqueeze(1), hx["m_r"].unsqueeze(1))
    assert abs(float(got) - float(hx["loss"])) <= 2e-7 * float(hx["loss"])
    assert emulator.flags("mgc_hair_lab_balanced_fwd") == [1]
    shared = networks.HairAvgLabLoss(_opt(), balance=crit.balance)
    assert shared.balance is crit.balance
    # an .npy file, the reference's own format
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "ab_count.npy")
        np.save(path, LB.ab_count())
        from michigan_amd.model import default_options
        again = networks.LabColorLoss(default_options(gpu_ids=[], balance_Lab=True, weight_dir=path))
        assert torch.equal(again.balance.host, crit.balance.host)
    # the one refusal left: no histogram is shipped
    for cls in (networks.LabColorLoss, networks.HairAvgLabLoss):
        with pytest.raises(NotImplementedError, match=r"balance_Lab.*ships no histogram.*--weight_dir"):
            cls(default_options(gpu_ids=[], balance_Lab=True))
    assert networks.LabColorLoss(default_options(gpu_ids=[])).balance is None


def _generator_step(emulator, unpaired=False, **over):
    from michigan_amd.model import Pix2PixModel
    from michigan_amd.synth import synth_loader_batch
    torch.manual_seed(0)
    model = Pix2PixModel(TP.repo_options(dict(TP.CFGS["A"], ngf=8, ndf=8, crop=64), **over))
    data = synth_loader_batch(1, 64, seed=3, unpaired=unpaired)
    emulator.calls.clear()
    losses, fake = model(data, mode="generator")
    return model, losses, fake, model.preprocess_input(data)


def test_model_losses_are_the_contract_values_times_lambda(emulator):
    from michigan_amd import ops
    on = dict(balance_Lab=True, weight_dir=LB.ab_count_path())
    model, losses, fake, d = _generator_step(emulator, no_lab_loss=False, no_rgb_loss=False, no_background_loss=False, lambda_lab=0.5, **on)
    S = ops.lab_weight_table(LB.ab_count(), 10.0)
    assert torch.equal(model.lab_balance.table("cpu"), S)
    want = LB.color_terms(fake.detach().float(), d["image_tag"], d["input_tag"][:, 0], d["input_tag"][:, 1], S, 7)[0]
    assert abs(float(losses["lab"].detach()) - 0.5 * float(want[0])) <= 1e-6 * 0.5 * float(want[0])
    assert abs(float(losses["rgb"].detach()) - float(want[1])) <= 1e-6 * float(want[1])
    assert emulator.flags("mgc_color_loss_balanced_fwd") == [7] and emulator.count("mg_color_loss_fwd") == 0       # ONE fused call
    plain = K.color_terms(fake.detach().float(), d["image_tag"], d["input_tag"][:, 0], 7)[0][0]
    assert abs(float(plain) - float(want[0])) > 0.1 * float(want[0])
    # rgb alone under balance_Lab: no Lab term, so the unbalanced entry point
    _, losses, _, _ = _generator_step(emulator, no_rgb_loss=False, **on)
    assert "lab" not in losses and emulator.flags("mg_color_loss_fwd") == [2] and emulator.count("mgc_color_loss_balanced_fwd") == 0
    # the unpaired step: the same table into the hair pass
    model, losses, fake, d = _generator_step(emulator, unpaired=True, unpairTrain=True, curr_step=2, lambda_hairavglab=2.0, **on)
    assert model.criterionHairAvgLab.balance is model.lab_balance
    want = LB.hair_terms(fake.detach().float(), d["image_ref"], d["input_tag"][:, 1], d["input_ref"][:, 1], S, d["image_tag"], d["input_tag"][:, 0], 3)[0]
    assert abs(float(losses["hairAvgLab"].detach()) - 2.0 * float(want[0])) <= 1e-6 * max(2.0 * float(want[0]), 1e-3)
    assert emulator.flags("mgc_hair_lab_balanced_fwd") == [3] and emulator.count("mg_hair_lab_fwd") == 0
    # off: nothing of the group is called
    _, _, _, _ = _generator_step(emulator, no_lab_loss=False)
    assert emulator.flags("mg_color_loss_fwd") == [1] and not any(name.startswith("mgc_") for name, _ in emulator.calls)


def test_the_one_refusal_left():
    from michigan_amd.model import Pix2PixModel, default_options
    cfg = dict(TP.CFGS["A"], ngf=8, ndf=8, crop=64)
    with pytest.raises(NotImplementedError, match=r"balance_Lab.*--weight_dir"):
        Pix2PixModel(TP.repo_options(cfg, no_lab_loss=False, balance_Lab=True))
    with pytest.raises(NotImplementedError, match=r"balance_Lab.*--weight_dir"):
        Pix2PixModel(TP.repo_options(cfg, unpairTrain=True, balance_Lab=True))
    Pix2PixModel(TP.repo_options(cfg, balance_Lab=True))                      # neither Lab term in the objective: nothing to weight
    opt = default_options()
    assert opt.weight_dir is None and opt.Lab_weight_th == 10.0 and opt.balance_Lab is False


# ---- 3. trainers and the driver ------------------------------------------------------------------------------------------------------------
def test_repo_trainer_matches_the_reference_trainers_record(emulator):
    from michigan_amd.model import Pix2PixTrainer
    cfg = dict(TP.CFGS["A"], tag="L")
    torch.manual_seed(0)
    trainer = Pix2PixTrainer(TP.repo_options(cfg, no_lab_loss=False, balance_Lab=True, weight_dir=LB.ab_count_path()))
    TP.load_weights(trainer, cfg)
    rec = LB.drive_with_lab(trainer, cfg)
    assert emulator.flags("mgc_color_loss_balanced_fwd") == [1] * cfg["iters"]
    gold = PU.load_trainer_golden("L")
    assert all(("it%d.loss.lab" % it) in gold for it in range(cfg["iters"]))
    TP.compare(rec, gold, **TOL)
    # the record is of the balanced objective: trainer_C's Lab value is another one
    assert abs(float(gold["it0.loss.lab"]) - float(PU.load_trainer_golden("C")["it0.loss.lab"])) > 0.1 * float(gold["it0.loss.lab"])


@needs_reference
def test_reference_trainer_with_balance_lab_over_dropin(emulator, tmp_path):
    """The reference's unmodified option parser, trainer and model with --balance_Lab --weight_dir <file> through dropin.install(); the
    reference's own cal_weight needs a CUDA tensor type, the patched class does not."""
    R.setup()
    import michigan_amd.dropin as dropin
    from michigan_amd import networks as hip
    npy = str(tmp_path / "ab_count.npy")
    np.save(npy, LB.ab_count())
    dropin.install(compute_dtype="fp32")
    try:
        from trainers.pix2pix_trainer import Pix2PixTrainer
        cfg = dict(TP.CFGS["A"], tag="L")
        opt = R.reference_options(LB.balance_argv(cfg, str(tmp_path), npy), train=True)
        assert opt.balance_Lab and opt.weight_dir == npy and opt.Lab_weight_th == 10.0 and not opt.no_lab_loss
        default = R.reference_options([a for a in LB.balance_argv(cfg, str(tmp_path), npy) if a not in ("--weight_dir", npy)], train=True)
        assert default.weight_dir == "./data/ab_count.npy"                   # the reference's default reaches the class as it is
        torch.manual_seed(0)
        trainer = Pix2PixTrainer(opt)
        m = trainer.pix2pix_model_on_one_gpu
        assert isinstance(m.criterionLabL1, hip.LabColorLoss) and m.criterionLabL1.balance is not None
        TP.load_weights(trainer, cfg)
        rec = LB.drive_with_lab(trainer, cfg)
        assert emulator.flags("mgc_color_loss_balanced_fwd") == [1] * cfg["iters"]
    finally:
        dropin.uninstall()
    TP.compare(rec, PU.load_trainer_golden("L"), **TOL)


def test_train_driver_runs_with_the_two_flags(emulator, tmp_path):
    import dataset_fixtures as DF
    from michigan_amd import train
    opt = train.parse(["--balance_Lab", "--weight_dir", "some/file.npy", "--Lab_weight_th", "7.5"])
    assert opt.balance_Lab is True and opt.weight_dir == "some/file.npy" and opt.Lab_weight_th == 7.5
    bare = train.parse([])
    assert bare.balance_Lab is False and bare.weight_dir is None and bare.Lab_weight_th == 10.0
    root, ck = str(tmp_path / "data"), str(tmp_path / "ck")
    DF.write_dataset(root, ("a0", "a1", "a2"), seed=3)
    argv = DF.small_argv(root, ck, "b", "--compute_dtype", "fp32", "--gpu_ids", "-1", "--batchSize", 2, "--seed", 5, "--print_freq", 2, "--niter", 1,
                         "--no_lab_loss", "false", "--balance_Lab", "--weight_dir", LB.ab_count_path())
    out = train.train(train.parse(argv))
    assert out["iterations"] == 1 and "lab" in out["losses"] and np.isfinite(out["losses"]["lab"])
    assert emulator.count("mgc_color_loss_balanced_fwd") == 1 and emulator.count("mgc_color_loss_balanced_bwd") == 1
    with pytest.raises(NotImplementedError, match="balance_Lab"):
        train.train(train.parse([a for a in argv if a not in ("--weight_dir", LB.ab_count_path())]))


# ---- 4. refusals and the group's place -----------------------------------------------------------------------------------------------------
def test_ops_refuse_bad_operands_before_any_launch(emulator):
    from michigan_amd import ops
    fx = LB.load_pair("i")
    img, sem, S = _image(fx["fake"], 8), _sem(fx), fx["S"]
    ok = lambda **kw: ops.color_losses(img, fx["real"], sem[:, 0], kw.pop("flags", 7), **dict(dict(hair=sem[:, 1], table=S), **kw))
    with pytest.raises(ValueError, match="needs COLOR_LAB"):
        ok(flags=6)
    with pytest.raises(ValueError, match="hair plane"):
        ok(hair=None)
    with pytest.raises(ValueError, match="does not match"):
        ok(hair=sem[:, 1, :, :-1])
    with pytest.raises(ValueError, match="fp32 \\[256, 256\\]"):
        ok(table=S.double())
    with pytest.raises(ValueError, match="fp32 \\[256, 256\\]"):
        ok(table=S[:255])
    with pytest.raises(ValueError, match="fp32 \\[256, 256\\]"):
        ok(table=S.numpy())
    with pytest.raises(ValueError, match="without a weight table"):
        ok(table=None)
    hx = LB.load_pair("hair")
    himg = _image(hx["fake"], 8)
    with pytest.raises(ValueError, match="needs HAIR_LAB"):
        ops.hair_lab_losses(himg, hx["ref"], hx["m_f"], hx["m_r"], hx["ref"], 1 - hx["m_f"], 2, table=hx["S"])
    with pytest.raises(ValueError, match="fp32 \\[256, 256\\]"):
        ops.hair_lab_losses(himg, hx["ref"], hx["m_f"], hx["m_r"], flags=1, table=hx["S"].t()[:, :128])
    assert emulator.calls == []                                               # nothing reached the backend
    # the emulator's own checks, as the header states them: a refused call is in the log
    p = ctypes.c_void_p(S.data_ptr())
    with pytest.raises(RuntimeError, match="mgc_color_loss_balanced_fwd: flags"):
        emulator.mgc_color_loss_balanced_fwd(p, p, 3 * 64, None, 0, p, 64, p, 0, 1, 8, 8, 8, 2, p, p)
    with pytest.raises(RuntimeError, match="mgc_hair_lab_balanced_bwd: null pointer"):
        emulator.mgc_hair_lab_balanced_bwd(p, p, 64, None, 0, None, 0, None, None, None, 0, 1, 8, 8, 8, 1, p)
    assert emulator.count("mgc_color_loss_balanced_fwd") == 1


def test_the_library_exports_the_group_and_checks_its_arguments():
    """validated before the device is touched, so this runs without one: status, message, and nothing launched"""
    from michigan_amd import _cabi, build
    be = _cabi.HipBackend(build.build(verbose=False))
    F32 = _cabi.MG_F32
    ok = dict(img=64, real=64, rs=3 * 64, back=None, bs=0, hair=64, hs=64, table=64, dtype=F32, N=1, H=8, W=8, C=8, flags=1, out=64, ws=64)

    def fwd(**over):
        a = dict(ok, **over)
        return be.mgc_color_loss_balanced_fwd(a["img"], a["real"], a["rs"], a["back"], a["bs"], a["hair"], a["hs"], a["table"], a["dtype"], a["N"], a["H"],
                                              a["W"], a["C"], a["flags"], a["out"], a["ws"], None)

    def bwd(**over):
        a = dict(ok, **over)
        return be.mgc_color_loss_balanced_bwd(a["img"], a["real"], a["rs"], a["back"], a["bs"], a["hair"], a["hs"], a["table"], None, None, None,
                                              a["dtype"], a["N"], a["H"], a["W"], a["C"], a["flags"], a["out"], None)
    for call, name in ((fwd, "mgc_color_loss_balanced_fwd"), (bwd, "mgc_color_loss_balanced_bwd")):
        for over, msg in ((dict(img=None), "null pointer"), (dict(flags=0), "flags"), (dict(flags=8), "flags"), (dict(flags=6), "must contain lab"),
                          (dict(flags=5), "label plane"), (dict(C=2), "bad geometry"), (dict(rs=64), "three dense planes"), (dict(dtype=7), "bad dtype"),
                          (dict(hair=None), "hair plane"), (dict(hs=63), "hair plane"), (dict(table=None), r"null pointer \(table\)"),
                          (dict(out=None), "null pointer")):
            with pytest.raises(RuntimeError, match=name + ": .*" + msg):
                call(**over)
    hok = dict(img=64, ref=64, rs=3 * 64, ft=64, fs=64, fr=64, frs=64, tgt=None, ts=0, back=None, bs=0, table=64, dtype=F32, N=1, H=8, W=8, C=8,
               flags=1, out=64, stats=64, ws=64)

    def hfwd(**over):
        a = dict(hok, **over)
        return be.mgc_hair_lab_balanced_fwd(a["img"], a["ref"], a["rs"], a["ft"], a["fs"], a["fr"], a["frs"], a["tgt"], a["ts"], a["back"], a["bs"],
                                            a["table"], a["dtype"], a["N"], a["H"], a["W"], a["C"], a["flags"], a["out"], a["stats"], a["ws"], None)

    def hbwd(**over):
        a = dict(hok, **over)
        return be.mgc_hair_lab_balanced_bwd(a["img"], a["ft"], a["fs"], a["tgt"], a["ts"], a["back"], a["bs"], a["stats"], None, None,
                                            a["dtype"], a["N"], a["H"], a["W"], a["C"], a["flags"], a["out"], None)
    for over, msg in ((dict(img=None), "null pointer"), (dict(table=None), "null pointer"), (dict(flags=0), "flags"), (dict(flags=2), "must contain hairAvgLab"),
                      (dict(flags=3), "three dense planes per sample of the target"), (dict(stats=None), "stats"), (dict(ref=None), "reference image"),
                      (dict(fr=None), "reference hair plane"), (dict(ft=None), "tag hair plane"), (dict(N=0), "bad geometry"), (dict(dtype=3), "bad dtype")):
        with pytest.raises(RuntimeError, match="mgc_hair_lab_balanced_fwd: .*" + msg):
            hfwd(**over)
    for over, msg in ((dict(img=None), "null pointer"), (dict(flags=2), "must contain hairAvgLab"), (dict(stats=None), "stats"),
                      (dict(ft=None), "tag hair plane"), (dict(C=2), "bad geometry")):
        with pytest.raises(RuntimeError, match="mgc_hair_lab_balanced_bwd: .*" + msg):
            hbwd(**over)
    with pytest.raises(AttributeError):
        be.mgc_not_an_entry_point


def test_the_header_is_outside_the_ledger_and_the_other_tables_are_unchanged():
    from michigan_amd import _cabi, build, ops
    src = open(os.path.join(ROOT, "include", "michigan_hip", "losses", "lab_balance.h")).read()
    assert re.findall(r"\bmg_[a-z0-9_]+\(", src) == []                        # not even in a comment
    stripped = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = {"mgc_color_loss_balanced_fwd", "mgc_color_loss_balanced_bwd", "mgc_hair_lab_balanced_fwd", "mgc_hair_lab_balanced_bwd"}
    assert set(re.findall(r"\b(mgc_[a-z0-9_]+)\s*\(", stripped)) == set(_cabi._COLOR_PROTOS) == names
    assert not names & set(_cabi._PROTOS) and not names & set(_cabi.EXPORTED_SYMBOLS) and not names & set(_cabi._EXTENSION_PROTOS)
    assert set(_cabi._LOSS_PROTOS) == {"mgl_orient_dog_fwd", "mgl_orient_dog_bwd"}
    assert set(_cabi._EXTENSION_PROTOS) == set(_cabi._EDIT_PROTOS) | set(_cabi._QUALITY_PROTOS) | set(_cabi._LOSS_PROTOS)
    assert _cabi.MG_ABI_VERSION == 10
    # the balanced argument lists are the unbalanced ones plus the new operands
    P, Q = _cabi._PROTOS, _cabi._COLOR_PROTOS
    vp, i64 = _cabi._vp, _cabi._i64
    for plain, balanced, at, extra in (("mg_color_loss_fwd", "mgc_color_loss_balanced_fwd", 5, [vp, i64, vp]),
                                       ("mg_color_loss_bwd", "mgc_color_loss_balanced_bwd", 5, [vp, i64, vp]),
                                       ("mg_hair_lab_fwd", "mgc_hair_lab_balanced_fwd", 11, [vp]), ("mg_hair_lab_bwd", "mgc_hair_lab_balanced_bwd", 0, [])):
        a = P[plain][0]
        assert Q[balanced][0] == a[:at] + extra + a[at:] and Q[balanced][1] == P[plain][1], balanced
    d = {k: int(v) for k, v in re.findall(r"#define\s+(MGC_[A-Z0-9_]+)\s+(\d+)\b", src)}
    assert (d["MGC_TABLE_BINS"], d["MGC_HAIR_STATS"]) == (LB.BINS, LB.HAIR_STATS) == (ops.LAB_TABLE_BINS, ops.HAIR_LAB_BALANCED_STATS)
    assert {"mg_color_loss.hip", "mg_hair_lab.hip"} <= set(build.SOURCES)
    from oracle.cabi_emulator import EmulatorBackend
    assert not any(n.startswith("mgc_") for n in dir(EmulatorBackend))
    # product code does not call grid_sample: the one mention is the docstring of ops.lab_weight_table
    for fn in ("ops.py", os.path.join("networks", "loss.py"), "model.py"):
        code = open(os.path.join(ROOT, "michigan_amd", fn)).read()
        assert "F.grid_sample" not in code and "import grid_sample" not in code and code.count("grid_sample(") == (1 if fn == "ops.py" else 0)
