"""MI355X: the fused Lab colour / RGB / background L1 kernels (mg_color_loss.hip) against what the reference's own classes
computed in float64 (tests/golden/color_loss_{i,ii}.npz, tools/make_color_loss_golden.py), and this package's trainer
with the three terms on against the reference trainer's record (trainer_C*.npz).

Bounds, and where they come from:
  losses    the project's fused-loss tolerance (tests/test_gpu_kernels.py::test_gabor_argmax_and_orientation_loss): 1e-4 (fp32 image)
            / 2e-2 (bf16 image) relative to max(1, |want|).
  gradient  relative L2 over the pixels that are not within 1e-3 of a sign change of da or db in the float64 reference (sign() is
            discontinuous there; the fixtures leave out 1.3e-4 and 2.0e-4 of the pixels of pairs (i) and (ii), the cap is 5e-3;
            the exactly-equal patch of pair (ii) is NOT left out, sign(0) = 0 must hold there).  RGB differences are no reason
            to leave a pixel out: the sign of x_f - x_r of two given values is exact in every precision.
            fp32 image: the reference's own classes run in fp32 on the CPU are 1.01e-7 (i) / 1.24e-7 (ii) relative L2 from their
            float64 run (stored in the fixtures, largest element error 2.1e-7 of the largest element); the kernel gets the larger
            of 4x that and 8 fp32 ulp = 9.5e-7 -- its cbrtf and division are each allowed a couple of ulp by HIP's device-math
            accuracy table and its sums are ordered differently.
            bf16 image: the fixture image is rounded to bf16 first and the reference is the float64 contract
            (oracle/contracts.py, pinned to the reference at 1e-9 by tests/test_color_loss.py) on the rounded image, so the
            bound measures the kernel and not the input rounding; dimg is written in bf16: one bf16 ulp, 2^-8 relative L2.
  measured  on MI355X (printed by the tests before they assert): see MEASURED below.
"""
import pytest
import torch

import color_loss_fixtures as CE
import parity_utils as PU
from color_loss_fixtures import load_pair as pair
from oracle import contracts as K
from oracle import trainer_parity as TP

pytestmark = pytest.mark.gpu

LOSS_RTOL = {torch.float32: 1e-4, torch.bfloat16: 2e-2}
EXCLUDE_BELOW, EXCLUDE_CAP = 1e-3, 5e-3
# MEASURED (MI355X, this file's own output; bound in brackets)
#   fp32 image: losses <= 3.1e-8 relative [1e-4]; gradient 9.9e-8 (i), 1.15e-7 (ii) relative L2 [9.5e-7], worst element 2.5e-7 of the largest
#   bf16 image: losses <= 3.7e-8 relative [2e-2]; gradient 1.53e-3 (i), 1.66e-3 (ii) relative L2 [3.9e-3]; left out <= 2.0e-4 of the pixels [5e-3]


def _image(fake, dtype, channels, device="cuda"):
    """NHWC image with `channels` >= 3 (padding filled with a value that must never be read)."""
    n, _, h, w = fake.shape
    img = torch.full((n, h, w, channels), 3.0, dtype=dtype)
    img[..., :3] = fake.permute(0, 2, 3, 1).to(dtype)
    return img.to(device).requires_grad_(True)


def _run(fx, dtype, channels, flags=7, real=None):
    from michigan_amd import ops
    img = _image(fx["fake"], dtype, channels)
    real = (fx["real"] if real is None else real).cuda()
    sem = torch.stack([fx["back"].float(), 1 - fx["back"].float()], dim=1).cuda()            # channel 0 of an NCHW label: strided planes
    out = ops.color_losses(img, real, sem[:, 0], flags)
    wl, wr, wb = fx["weights"].tolist()
    (wl * out[0] + wr * out[1] + wb * out[2]).backward()
    torch.cuda.synchronize()
    return torch.stack([o.detach() for o in out]).cpu(), img.grad.detach().cpu()


@pytest.mark.parametrize("tag", ["i", "ii"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_kernels_match_the_reference(hip_backend, tag, dtype):
    fx = pair(tag)
    weights = tuple(fx["weights"].tolist())
    real = fx["real"]
    if dtype == torch.float32:
        want_l, want_g, ex = fx["losses"], fx["grad"], fx["excluded"]
        bound = max(4 * float(fx["ref32_grad_rel_l2"]), 8 * 2.0 ** -23)
    else:
        rounded = fx["fake"].to(torch.bfloat16).float()
        if tag == "ii":                                            # keep the exactly-equal patch exactly equal after the rounding
            real = real.clone()
            real[:, :, 40:48, 24:32] = rounded[:, :, 40:48, 24:32]
        want_l, want_g, (da, db, _) = K.color_terms(rounded, real, fx["back"].float(), 7, weights)
        near = lambda t: (t.abs() > 0) & (t.abs() < EXCLUDE_BELOW)
        ex = near(da) | near(db)
        bound = 2.0 ** -8
    share = float(ex.double().mean())
    keep = (~ex).unsqueeze(1).double()
    got_l, got_g = _run(fx, dtype, 8, real=real)
    got_g3 = got_g[..., :3].permute(0, 3, 1, 2).double()
    rel_l = [abs(float(got_l[k]) - float(want_l[k])) / max(1.0, abs(float(want_l[k]))) for k in range(3)]
    rel_g = float(((got_g3 - want_g) * keep).norm() / (want_g * keep).norm())
    worst = float(((got_g3 - want_g) * keep).abs().max() / want_g.abs().max())
    print("color loss %s %s: losses %s want %s rel %s | grad rel L2 %.3e (bound %.3e), worst element / largest %.3e | left out %.2e of the pixels"
          % (tag, dtype, got_l.tolist(), [float(v) for v in want_l], ["%.2e" % v for v in rel_l], rel_g, bound, worst, share))
    assert share <= EXCLUDE_CAP
    assert max(rel_l) <= LOSS_RTOL[dtype], rel_l
    assert rel_g <= bound, (rel_g, bound)
    assert float(got_g[..., 3:].abs().max()) == 0.0                # padding channels of dimg
    if tag == "ii":
        assert float(want_g[:, :, 40:48, 24:32].abs().max()) == 0.0
        assert float(got_g3[:, :, 40:48, 24:32].abs().max()) == 0.0, "sign(0) must be 0"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_flag_subsets_layouts_and_reproducibility(hip_backend, dtype):
    fx = pair("i")
    all_l, all_g = _run(fx, dtype, 8)
    again_l, again_g = _run(fx, dtype, 8)
    assert torch.equal(all_l, again_l) and torch.equal(all_g, again_g), "ordered sums: two runs must be bit-identical"
    assert float(all_g[..., 3:].abs().max()) == 0.0
    l3, g3 = _run(fx, dtype, 3)
    assert torch.equal(l3, all_l) and torch.equal(g3, all_g[..., :3]), "C = 3 and C = 8 layouts must agree"
    for flags in range(1, 8):
        l, g = _run(fx, dtype, 8, flags=flags)
        for k in range(3):
            if flags & (1 << k):
                assert float(l[k]) == float(all_l[k]), (flags, k)  # bit for bit the value of the all-on call
            else:
                assert float(l[k]) == 0.0, (flags, k)
        assert float(g[..., 3:].abs().max()) == 0.0
    # the three one-bit gradients add up to the all-on one (one rounding per term and element)
    parts = sum(_run(fx, dtype, 8, flags=f)[1].double() for f in (1, 2, 4))
    tol = 2.0 ** -7 if dtype == torch.bfloat16 else 1e-6
    assert float((parts - all_g.double()).norm() / all_g.double().norm()) <= tol


def test_trainer_fp32_with_color_losses_matches_reference_trainer_golden(hip_backend):
    """tests/test_gpu_trainer.py's fp32 protocol and tolerances, with the README objective as published (+ rgb, background)."""
    from michigan_amd.model import Pix2PixTrainer
    cfg = dict(TP.CFGS["A"], tag="C")
    torch.manual_seed(0)
    trainer = Pix2PixTrainer(TP.repo_options(cfg, gpu_ids=[0], compute_dtype="fp32", no_lab_loss=False, no_rgb_loss=False, no_background_loss=False))
    TP.load_weights(trainer, cfg)
    rec = CE.drive_with_color_losses(trainer, cfg, device="cuda")
    print("trainer C losses", {k: float(v) for k, v in rec.items() if ".loss." in k})
    TP.compare(rec, PU.load_trainer_golden("C"), rtol_loss0=5e-4, rtol_later=TP.RTOL_LATER_HIP, atol_img=1e-3, atol_weight=2 * 4e-4 * 2 + 1e-5)
