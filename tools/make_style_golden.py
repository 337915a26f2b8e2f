"""Generate the fixtures of the style / content terms by running the REFERENCE's own classes:

    python tools/make_style_golden.py [--no-trainer]        (where the reference checkout is; CPU, ~1 min)

  tests/golden/style_loss_i.npz, style_loss_ii.npz   for the two seeded feature sets of tests/style_loss_fixtures.make_sets (the
        fixtures hold RESULTS only, the sets are regenerated from their seed): the reference's StyleContentLoss.calc_style_loss /
        calc_content_loss in FLOAT64 on the fp32 features with remove_background off (`plain`) and on (`masked`), the gradient
        d(w_s style + w_c content) / dx, and the error of the same methods run in FLOAT32 on the CPU against their float64 run -- the
        yardstick the fp32 kernel's bound is derived from (tests/test_gpu_style_loss.py).
  tests/golden/trainer_S.npz, trainer_S_weights.npz, trainer_style_config.json   the reference's own Pix2PixTrainer on configuration A
        with the README flags minus --no_style_loss / --no_content_loss, the style tower's weights copied from the VGG tower's (the
        reference loads the same pretrained file into both); two iterations, the second on a batch whose reference mask differs from
        the tag mask (style / content are computed there, GAN_Feat / VGG are not).

Asserted here on the CPU so that no test needs an exclusion list: every result is finite; on set ii a mutant that forms
E[x^2] - mu^2 from unshifted fp32 sums exceeds the fp32 gradient bound of the GPU test.
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
ULP32 = 2.0 ** -23


def _reference_class(remove_background):
    """StyleContentLoss without its constructor (which builds a pretrained tower): the two methods need mse_loss and opt only."""
    import models.networks.loss as RL
    crit = RL.StyleContentLoss.__new__(RL.StyleContentLoss)
    torch.nn.Module.__init__(crit)
    crit.mse_loss = torch.nn.MSELoss()
    crit.opt = types.SimpleNamespace(remove_background=remove_background)
    return crit


def reference_run(p, dtype, masked, weights):
    """(losses[2] = (style, content), d(w_s style + w_c content) / dx) of the reference's methods in `dtype`.  calc_style_loss(input,
    target, style_label, content_label) takes input under style_label and target under content_label (loss.py:692-693): mask_x and
    mask_s of the set in that order."""
    crit = _reference_class(masked)
    x = p["x"].to(dtype).clone().requires_grad_(True)
    s, t = p["s"].to(dtype), p["t"].to(dtype)
    lab = lambda k: p[k].to(dtype).unsqueeze(1) if masked else None
    style = crit.calc_style_loss(x, s, lab("mask_x"), lab("mask_s"))
    content = crit.calc_content_loss(x, t, lab("mask_t"))
    (weights[0] * style + weights[1] * content).backward()
    return torch.stack([style, content]).detach(), x.grad.detach()


def mutant_gradient(p, weights):
    """The unmasked gradient with sigma_x from E[x^2] - mu^2 of UNSHIFTED fp32 sums: what the pivot is there to prevent."""
    from oracle import contracts as K
    x = p["x"]
    n, c, h, w = x.shape
    P = h * w
    x3 = x.float().reshape(n, c, P)
    s1, s2 = x3.sum(dim=2), (x3 * x3).sum(dim=2)                               # fp32
    mu = (s1 / P).double()
    sg_x = (((s2 - s1 * s1 / P) / (P - 1)).double().clamp_min(0) + K.FEAT_EPS).sqrt()
    mu_s, sg_s, _, _ = K.moments(p["s"].double().reshape(n, c, P))
    gm, gs = 2 * (mu - mu_s) / (n * c), 2 * (sg_x - sg_s) / (n * c)
    x64, t64 = x.double().reshape(n, c, P), p["t"].double().reshape(n, c, P)
    g = K.gradient(x64, t64, None, None, gm / P, gs / (sg_x * (P - 1)), mu, float(n * P * c), weights[0], weights[1])
    return g.reshape(n, c, h, w)


def make_sets():
    import style_loss_fixtures as SE
    from oracle import ref_harness as R
    R.setup()
    for tag, p in SE.make_sets().items():
        rec = {"weights": np.array(SE.WEIGHTS)}
        for mode, masked in (("plain", False), ("masked", True)):
            l64, g64 = reference_run(p, torch.float64, masked, SE.WEIGHTS)
            l32, g32 = reference_run(p, torch.float32, masked, SE.WEIGHTS)
            assert bool(torch.isfinite(l64).all()) and bool(torch.isfinite(g64).all()) and bool(torch.isfinite(l32).all()) and bool(torch.isfinite(g32).all())
            err_loss = ((l32.double() - l64).abs() / l64.abs()).numpy()
            err_grad = float((g32.double() - g64).norm() / g64.norm())
            rec.update({"losses_" + mode: l64.numpy(), "grad_" + mode: g64.numpy(), "ref32_loss_rel_" + mode: err_loss,
                        "ref32_grad_rel_l2_" + mode: np.array(err_grad)})
            print("set %s %s: losses %s | fp32 reference: loss rel %s, grad rel L2 %.2e" % (tag, mode, l64.numpy(), err_loss, err_grad))
        if tag == "i":
            assert all(bool(((p[k] == 0) | (p[k] == 1)).all()) for k in ("mask_x", "mask_s", "mask_t"))
        if tag == "ii":
            assert float(p["mask_x"][1].sum()) == 0 and float(p["mask_s"][2].sum()) == 0
            assert all(bool(((p[k] > 0) & (p[k] < 1)).any()) for k in ("mask_x", "mask_s", "mask_t"))
            g64 = torch.from_numpy(rec["grad_plain"])
            mut = float((mutant_gradient(p, SE.WEIGHTS) - g64).norm() / g64.norm())
            bound = max(4 * float(rec["ref32_grad_rel_l2_plain"]), 8 * ULP32)
            print("set ii: E[x^2] - mu^2 mutant grad rel L2 %.2e against the fp32 bound %.2e" % (mut, bound))
            assert mut > bound, "the set does not tell shifted from unshifted sums apart"
            rec["mutant_grad_rel_l2"] = np.array(mut)
        np.savez_compressed(os.path.join(OUT, "style_loss_%s.npz" % tag), **rec)


# ---- the trainer protocol with the two terms on ------------------------------------------------------------------------------------
def make_trainer():
    import style_loss_fixtures as SP
    from oracle import ref_harness as R
    from oracle import trainer_parity as TP
    R.setup()
    from trainers.pix2pix_trainer import Pix2PixTrainer
    cfg = dict(TP.CFGS["A"], tag="S")
    with tempfile.TemporaryDirectory() as ck:
        opt = R.reference_options(SP.style_argv(cfg, ck), train=True)
        assert not opt.no_style_loss and not opt.no_content_loss and opt.lambda_style == 1 and opt.lambda_content == 1
        torch.manual_seed(0)
        trainer = Pix2PixTrainer(opt)
        SP.load_weights(trainer, cfg)
        rec = SP.drive_style(trainer, cfg)
    assert all("it%d.loss.%s" % (it, k) in rec for it in range(cfg["iters"]) for k in ("content", "style"))
    assert "it0.loss.VGG" in rec and "it1.loss.VGG" not in rec, "iteration 1 must run on a batch whose reference mask differs"
    assert all(np.isfinite(v).all() for v in rec.values())
    weights = {k: v for k, v in rec.items() if k.startswith(("G.", "D."))}
    np.savez_compressed(os.path.join(OUT, "trainer_S.npz"), **{k: v for k, v in rec.items() if k not in weights})
    np.savez_compressed(os.path.join(OUT, "trainer_S_weights.npz"), **weights)
    with open(os.path.join(OUT, "trainer_style_config.json"), "w") as fh:
        json.dump({"S": dict(cfg, lambda_style=opt.lambda_style, lambda_content=opt.lambda_content,
                             flags_removed=["--no_style_loss", "--no_content_loss"])}, fh)
    print("trainer golden S", {k: float(v) for k, v in rec.items() if ".loss." in k})


if __name__ == "__main__":
    make_sets()
    if "--no-trainer" not in sys.argv:
        make_trainer()
    largest = max(os.path.getsize(os.path.join(OUT, fn)) for fn in os.listdir(OUT) if not fn.startswith(("style_loss", "trainer_S", "trainer_style")))
    for fn in sorted(os.listdir(OUT)):
        if fn.startswith(("style_loss", "trainer_S", "trainer_style")):
            size = os.path.getsize(os.path.join(OUT, fn))
            assert size <= largest, (fn, size, largest)
            print("%8d  %s" % (size, fn))
