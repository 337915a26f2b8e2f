"""Generate the fixtures of the unpaired training stage by running the REFERENCE's own classes:

    python tools/make_unpaired_golden.py            (where the reference checkout is; CPU, ~1 min)

  tests/golden/hair_lab_i.npz, hair_lab_ii.npz   two seeded input sets at N=2, 3x96x80 (tests/hair_lab_fixtures.make_pairs): the inputs
        (fp32), the reference's HairAvgLabLoss(fake, ref, m_f, m_r) and RGBBackgroundL1Loss(fake, label, tgt) in FLOAT64 on the
        fp32-rounded inputs, d(w_h hair + w_b background) / d fake, the per-sample da, db, and the error of the same classes run in
        FLOAT32 on the CPU against their float64 run -- the yardstick the fp32 kernel's bound is derived from
        (tests/test_gpu_unpaired.py).
  tests/golden/trainer_U.npz, trainer_U_weights.npz, trainer_unpaired_config.json   tests/hair_lab_fixtures.drive_unpaired's record of
        the reference's own Pix2PixTrainer on configuration A with the README flags + --unpairTrain: per iteration curr_step = 2 on
        an unpaired batch, then curr_step = 1 on the paired batch (train.py:41-90 in miniature), netD2 seeded as well.

The reference's HairAvgLabLoss spells the logical complement of a boolean mask `1 - mask` (loss.py:546,565) like its LabColorLoss;
the shim of tools/make_color_loss_golden.py (Tensor.__rsub__ returns the complement of a bool operand, in THIS process only) lets the
unmodified class run.  Conditions a test would otherwise need an exclusion list for are asserted here: every per-sample |da|, |db| >= 1
in float64 and on the bf16-rounded image (sign() is nowhere near its discontinuity), the gradient of the hair term alone exactly 0
outside the tag mask.
"""
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden")

from make_color_loss_golden import _shim_rsub  # noqa: E402  (same directory)


def reference_run(p, dtype, weights):
    """The reference classes in `dtype`: (losses[2], d(weighted sum)/d fake, d hair / d fake, (da, db), share of the image's XYZ below the knee)."""
    import models.networks.loss as RL
    hair_cls, bg_cls = RL.HairAvgLabLoss(types.SimpleNamespace(balance_Lab=False)), RL.RGBBackgroundL1Loss()
    hair_cls.M = hair_cls.M.to(dtype)
    f = p["fake"].to(dtype).clone().requires_grad_(True)
    ref, tgt = p["ref"].to(dtype), p["tgt"].to(dtype)
    sem = torch.stack([p["m_b"], 1 - p["m_b"]], dim=1).to(dtype)          # the one-hot label: channel 0 = background
    hair = hair_cls(f, ref, p["m_f"].to(dtype).unsqueeze(1), p["m_r"].to(dtype).unsqueeze(1))
    bg = bg_cls(f, sem, tgt)
    g_hair, = torch.autograd.grad(hair, f, retain_graph=True)
    (weights[0] * hair + weights[1] * bg).backward()
    with torch.no_grad():
        xyz = hair_cls.rgb2xyz((f + 1) / 2)
        avg = lambda x, m: hair_cls.cal_hair_avg(hair_cls.xyz2lab(hair_cls.rgb2xyz((x + 1) / 2)), m.to(dtype).unsqueeze(1).clone())[:, 1:, 0, 0]
        d = avg(f, p["m_f"]) - avg(ref, p["m_r"])                         # [N, 2]
        knee = float((xyz < 0.008856).double().mean())
    return torch.stack([hair, bg]).detach(), f.grad.detach(), g_hair.detach(), (d[:, 0], d[:, 1]), knee


def make_hair_lab():
    import hair_lab_fixtures as HE
    from oracle import ref_harness as R
    R.setup()
    for tag, p in HE.make_pairs().items():
        # unequal weights that bring the two gradients to one magnitude (the hair term spreads 1 / S_f over the mask, the
        # background term 1 / (3 N H W) over its complement; the Lab chain's factor is ~ 10^2)
        _, _, gh, _, _ = reference_run(p, torch.float64, (1.0, 0.0))
        _, gb, _, _, _ = reference_run(p, torch.float64, (0.0, 1.0))
        weights = (0.5, round(0.5 * float(gh.abs().mean() / gb.abs().mean()) * 1.3, 3))
        l64, g64, gh64, (da, db), knee = reference_run(p, torch.float64, weights)
        l32, g32, _, _, _ = reference_run(p, torch.float32, weights)
        rounded = dict(p, fake=p["fake"].to(torch.bfloat16).float())
        _, _, _, (da16, db16), _ = reference_run(rounded, torch.float64, weights)
        err_loss = ((l32.double() - l64).abs() / l64.abs()).numpy()
        err_grad = float((g32.double() - g64).norm() / g64.norm())
        err_grad_max = float((g32.double() - g64).abs().max() / g64.abs().max())
        outside = float((gh64 * (p["m_f"] == 0).unsqueeze(1)).abs().max())
        print("set %s: weights %s | losses %s | da %s db %s | on the bf16-rounded image da %s db %s | below knee %.3f | grad magnitudes hair %.3e "
              "background %.3e | fp32 reference: loss rel %s, grad rel L2 %.2e, max/largest %.2e | hair grad outside the tag mask %s"
              % (tag, weights, l64.numpy(), da.numpy(), db.numpy(), da16.numpy(), db16.numpy(), knee, weights[0] * float(gh.abs().mean()),
                 weights[1] * float(gb.abs().mean()), err_loss, err_grad, err_grad_max, outside))
        for t in (da, db, da16, db16):
            assert float(t.abs().min()) >= 1.0, "a per-sample mean difference is too close to the discontinuity of sign()"
        assert torch.equal(torch.sign(da), torch.sign(da16)) and torch.equal(torch.sign(db), torch.sign(db16))
        assert outside == 0.0, "the hair term's gradient must be exactly 0 outside the tag mask"
        assert bool(torch.isfinite(l64).all()) and bool(torch.isfinite(g64).all())
        if tag == "i":
            assert knee >= 0.05, "the linear branch of f is not exercised"
        if tag == "ii":
            assert float(p["m_r"][0].sum()) == 0 and float(p["m_f"][1].sum()) == 0 and bool(((p["m_f"] > 0) & (p["m_f"] < 1)).any())
        np.savez_compressed(os.path.join(OUT, "hair_lab_%s.npz" % tag), weights=np.array(weights), losses=l64.numpy(), grad=g64.numpy(),
                            da=da.numpy(), db=db.numpy(), ref32_loss_rel=err_loss, ref32_grad_rel_l2=np.array(err_grad),
                            ref32_grad_max_over_largest=np.array(err_grad_max), below_knee=np.array(knee),
                            **{k: v.numpy() for k, v in p.items()})


def make_trainer():
    import hair_lab_fixtures as HE
    from oracle import ref_harness as R
    from oracle import trainer_parity as TP
    R.setup()
    from trainers.pix2pix_trainer import Pix2PixTrainer
    cfg = dict(TP.CFGS["A"], tag="U")
    with tempfile.TemporaryDirectory() as ck:
        opt = R.reference_options(HE.unpaired_argv(cfg, ck), train=True)
        assert opt.unpairTrain and opt.lambda_hairavglab == 1 and not opt.same_netD_model
        torch.manual_seed(0)
        trainer = Pix2PixTrainer(opt)
        HE.load_weights(trainer, cfg)
        rec = HE.drive_unpaired(trainer, cfg)
    assert all("it%d.loss.%s" % (it, k) in rec for it in range(cfg["iters"]) for k in HE.STEP2_KEYS)
    weights = {k: v for k, v in rec.items() if k.startswith(("G.", "D."))}
    np.savez_compressed(os.path.join(OUT, "trainer_U.npz"), **{k: v for k, v in rec.items() if k not in weights})
    np.savez_compressed(os.path.join(OUT, "trainer_U_weights.npz"), **weights)
    with open(os.path.join(OUT, "trainer_unpaired_config.json"), "w") as fh:
        json.dump({"U": dict(cfg, lambda_hairavglab=opt.lambda_hairavglab, lambda_background=opt.lambda_background, seed_d2=cfg["seed_d"] + 1000,
                             flags_added=["--unpairTrain"])}, fh)
    print("trainer golden U", {k: float(v) for k, v in rec.items() if ".loss." in k})


if __name__ == "__main__":
    _shim_rsub()
    make_hair_lab()
    make_trainer()
    for fn in sorted(os.listdir(OUT)):
        if fn.startswith(("hair_lab", "trainer_U", "trainer_unpaired")):
            size = os.path.getsize(os.path.join(OUT, fn))
            assert size <= 1 << 20, (fn, size)
            print("%8d  %s" % (size, fn))
