"""Generate the fixtures of the fused Lab / RGB / background loss by running the REFERENCE's own classes:

    python tools/make_color_loss_golden.py            (where the reference checkout is; CPU, ~10 s)

  tests/golden/color_loss_i.npz, color_loss_ii.npz   two seeded input pairs at N=2, 3x96x80 and a random 0/1 background plane: the
        inputs (fp32), the three reference losses, the reference's d(w_l lab + w_r rgb + w_b background) / d fake, all from
        LabColorLoss / RGBBackgroundL1Loss / nn.L1Loss in FLOAT64 on the fp32-rounded inputs; the pixels left out of gradient
        comparisons (see EXCLUDE_BELOW); and the error of the same classes run in FLOAT32 on the CPU against their float64 run --
        the yardstick the fp32 kernel's bound is derived from (tests/test_gpu_color_loss.py).
        One file per pair: a pair with its float64 gradient is ~0.8 MB, and no committed file may exceed 1 MiB.
  tests/golden/trainer_C.npz, trainer_C_weights.npz, trainer_color_config.json   oracle.trainer_parity.drive's record of the
        reference's own Pix2PixTrainer on configuration A with the README flags AS PUBLISHED (Lab on) plus background and rgb
        on, extended by the three new loss values per iteration (weights in the second file, for the same size limit).

The reference's LabColorLoss spells the logical complement of a boolean mask `1 - mask` (loss.py:443,472), which meant that on
the torch it was written for and raises today.  In THIS process only, Tensor.__rsub__ is wrapped so that a bool operand returns
its complement; the unmodified class then runs, and its two independent Lab implementations (rgb2xyz + xyz2lab, RGB2Lab) agree
to 1e-8, which is what shows the shim restores the intended semantics.
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

N, H, W = 2, 96, 80
WEIGHTS = (0.05, 3.0, 2.0)            # (lab, rgb, background): unequal, and chosen so that the three gradients are of one magnitude
EXCLUDE_BELOW = 1e-3                  # sign() is discontinuous at 0: pixels with 0 < |delta| < this in da or db are left out (see excluded())
EXCLUDE_CAP = 0.005                   # ... and at most this share of the pixels may be


def _shim_rsub():
    orig = torch.Tensor.__rsub__

    def rsub(self, other):
        return ~self if self.dtype == torch.bool else orig(self, other)
    torch.Tensor.__rsub__ = rsub


def make_pairs():
    g = torch.Generator().manual_seed(2024)
    dark = H // 8

    def uniform():
        x = torch.rand(N, 3, H, W, generator=g) * 2 - 1
        x[:, :, :dark] = -1 + 0.01 * torch.rand(N, 3, dark, W, generator=g)
        return x
    fake_i, real_i = uniform(), uniform()
    real_ii = torch.rand(N, 3, H, W, generator=g) * 2 - 1
    fake_ii = (real_ii + 0.3 * torch.randn(N, 3, H, W, generator=g)).clamp(-1, 1)
    fake_ii[:, :, 40:48, 24:32] = real_ii[:, :, 40:48, 24:32]          # an exactly equal patch: sign(0) = 0
    back = (torch.rand(N, H, W, generator=g) > 0.4).float()
    return {"i": (fake_i, real_i, back), "ii": (fake_ii, real_ii, back.flip(2).contiguous())}


def reference_run(fake, real, back, dtype):
    """The reference classes in `dtype`: (losses[3], d(weighted sum)/d fake, (da, db, drgb), share of XYZ values below the knee)."""
    import models.networks.loss as RL
    lab_cls, bg_cls = RL.LabColorLoss(types.SimpleNamespace(balance_Lab=False)), RL.RGBBackgroundL1Loss()
    lab_cls.M = lab_cls.M.to(dtype)
    f = fake.to(dtype).clone().requires_grad_(True)
    r = real.to(dtype)
    sem = torch.stack([back, 1 - back], dim=1).to(dtype)                 # the one-hot label: channel 0 = background
    lab = lab_cls(f, r.detach(), sem[:, 1:2])
    rgb = torch.nn.L1Loss()(f, r.detach())
    bg = bg_cls(f, sem, r)
    (WEIGHTS[0] * lab + WEIGHTS[1] * rgb + WEIGHTS[2] * bg).backward()
    with torch.no_grad():
        xyz_f, xyz_r = lab_cls.rgb2xyz((f + 1) / 2), lab_cls.rgb2xyz((r + 1) / 2)
        lf, lr = lab_cls.xyz2lab(xyz_f), lab_cls.xyz2lab(xyz_r)
        deltas = (lf[:, 1] - lr[:, 1], lf[:, 2] - lr[:, 2], f - r)
        knee = float((torch.cat([xyz_f, xyz_r]) < 0.008856).double().mean())
        # the class's second, independent implementation
        other = (lab_cls.RGB2Lab((f + 1) / 2)[:, 1:] - lab_cls.RGB2Lab((r + 1) / 2)[:, 1:]).abs().mean()
    return torch.stack([lab, rgb, bg]).detach(), f.grad.detach(), deltas, knee, float(other)


def excluded(deltas):
    """Pixels left out of gradient comparisons: 0 < |da| or |db| < EXCLUDE_BELOW, where an implementation in another precision may
    land on the other side of sign().  The RGB differences are NOT a reason to leave a pixel out: x_f - x_r of two given fp32 (or
    bf16) values has the right sign in every IEEE precision, and m is 0 or 1, so sign(drgb) cannot flip.  (Leaving out pixels with a
    small drgb as well would drop 6 % of pair (i) -- its dark rows differ by < 0.01 -- and 1 % of pair (ii), beyond EXCLUDE_CAP.)"""
    da, db, _ = deltas
    near = lambda t: (t.abs() > 0) & (t.abs() < EXCLUDE_BELOW)
    return near(da) | near(db)                                           # [N, H, W]


def make_color_loss():
    from oracle import ref_harness as R
    R.setup()
    for tag, (fake, real, back) in make_pairs().items():
        l64, g64, deltas, knee, other = reference_run(fake, real, back, torch.float64)
        l32, g32, _, _, _ = reference_run(fake, real, back, torch.float32)
        ex = excluded(deltas)
        keep = (~ex).unsqueeze(1).double()
        share = float(ex.double().mean())
        err_loss = ((l32.double() - l64).abs() / l64.abs()).numpy()
        err_grad = float(((g32.double() - g64) * keep).norm() / (g64 * keep).norm())
        err_grad_max = float(((g32.double() - g64) * keep).abs().max() / g64.abs().max())
        zero_patch = float(g64[:, :, 40:48, 24:32].abs().max()) if tag == "ii" else float("nan")
        print("pair %s: losses %s | second Lab implementation %.8f (rel %.1e) | below knee %.3f | excluded %.2e | fp32 reference: loss rel %s, "
              "grad rel L2 %.2e, max/largest %.2e | saturated %.3f | grad in the equal patch (lab+rgb part) %s"
              % (tag, l64.numpy(), other, abs(other - float(l64[0])) / float(l64[0]), knee, share, err_loss, err_grad, err_grad_max,
                 float((fake.abs() == 1).double().mean()), zero_patch))
        assert abs(other - float(l64[0])) < 1e-6 * float(l64[0]), "the two Lab implementations of the reference disagree: the shim is wrong"
        assert share <= EXCLUDE_CAP, "too many pixels near a sign change"
        if tag == "i":
            assert knee >= 0.05, "the linear branch of f is not exercised"
        if tag == "ii":
            # in the patch da = db = drgb = 0 exactly: only the background term's sign(0 * m) = 0 remains, so the gradient is 0 there
            assert zero_patch == 0.0 and not bool(ex[:, 40:48, 24:32].any())
        np.savez_compressed(os.path.join(OUT, "color_loss_%s.npz" % tag), fake=fake.numpy(), real=real.numpy(), back=back.numpy().astype(np.uint8),
                            weights=np.array(WEIGHTS), losses=l64.numpy(), grad=g64.numpy(), excluded=ex.numpy(),
                            ref32_loss_rel=err_loss, ref32_grad_rel_l2=np.array(err_grad), ref32_grad_max_over_largest=np.array(err_grad_max),
                            below_knee=np.array(knee), exclude_below=np.array(EXCLUDE_BELOW))


def make_trainer():
    import color_loss_fixtures as CE
    from oracle import ref_harness as R
    from oracle import trainer_parity as TP
    R.setup()
    from trainers.pix2pix_trainer import Pix2PixTrainer
    cfg = dict(TP.CFGS["A"], tag="C")
    with tempfile.TemporaryDirectory() as ck:
        opt = R.reference_options(CE.color_argv(cfg, ck), train=True)
        assert not (opt.no_lab_loss or opt.no_rgb_loss or opt.no_background_loss) and opt.lambda_lab == 1
        torch.manual_seed(0)
        trainer = Pix2PixTrainer(opt)
        TP.load_weights(trainer, cfg)
        rec = CE.drive_with_color_losses(trainer, cfg)
    weights = {k: v for k, v in rec.items() if k.startswith(("G.", "D."))}
    np.savez_compressed(os.path.join(OUT, "trainer_C.npz"), **{k: v for k, v in rec.items() if k not in weights})
    np.savez_compressed(os.path.join(OUT, "trainer_C_weights.npz"), **weights)
    with open(os.path.join(OUT, "trainer_color_config.json"), "w") as fh:
        json.dump({"C": dict(cfg, lambda_lab=opt.lambda_lab, lambda_rgb=opt.lambda_rgb, lambda_background=opt.lambda_background,
                             flags_removed=["--no_lab_loss", "--no_background_loss", "--no_rgb_loss"])}, fh)
    print("trainer golden C", {k: float(v) for k, v in rec.items() if ".loss." in k})


if __name__ == "__main__":
    _shim_rsub()
    make_color_loss()
    make_trainer()
    for fn in sorted(os.listdir(OUT)):
        if fn.startswith(("color_loss", "trainer_C", "trainer_color")):
            size = os.path.getsize(os.path.join(OUT, fn))
            assert size <= 1 << 20, (fn, size)
            print("%8d  %s" % (size, fn))
