"""MI355X: the fused hair-average Lab / background kernels (mg_hair_lab.hip) against what the reference's own classes computed in
float64 (tests/golden/hair_lab_{i,ii}.npz, tools/make_unpaired_golden.py), and this package's trainer through the unpaired stage
against the reference trainer's record (trainer_U*.npz).  Reads only tests/golden/.

Bounds, and where they come from (the rule of tests/test_gpu_color_loss.py, whose docstring has the reasoning):
  losses    the project's fused-loss tolerance: 1e-4 (fp32 image) / 2e-2 (bf16 image) relative to max(1, |want|).
  gradient  relative L2 over ALL elements -- no exclusion list: the fixture generator asserts every per-sample |da|, |db| >= 1 in
            float64 and on the bf16-rounded image, so sign() is nowhere near its discontinuity.
            fp32 image: the larger of 4 x the reference classes' own fp32-vs-float64 error stored in the fixture (1.24e-7 (i),
            8.7e-8 (ii)) and 8 fp32 ulp = 9.5e-7.
            bf16 image: want = the float64 contract (oracle/contracts.py, pinned to the reference at 1e-9 by
            tests/test_unpaired.py) on the bf16-rounded image, so the bound measures the kernel and not the input rounding; dimg is
            written in bf16: one bf16 ulp, 2^-8.  The signs of da, db on the rounded image are asserted equal to the fixture's first.
  measured  on MI355X (printed by the tests before they assert): see MEASURED below.
"""
import pytest
import torch

import hair_lab_fixtures as HE
import parity_utils as PU
from hair_lab_fixtures import load_pair as pair
from oracle import contracts as K
from oracle import trainer_parity as TP

pytestmark = pytest.mark.gpu

LOSS_RTOL = {torch.float32: 1e-4, torch.bfloat16: 2e-2}            # tests/test_gpu_color_loss.py::LOSS_RTOL
# MEASURED (MI355X, this file's own output; bound in brackets)
#   not measured yet


def _image(fake, dtype, channels, device="cuda"):
    """NHWC image with `channels` >= 3 (padding filled with a value that must never be read)."""
    n, _, h, w = fake.shape
    img = torch.full((n, h, w, channels), 3.0, dtype=dtype)
    img[..., :3] = fake.permute(0, 2, 3, 1).to(dtype)
    return img.to(device).requires_grad_(True)


def _run(fx, dtype, channels, flags=3, weights=None):
    """ops.hair_lab_losses on the GPU with the masks as channel views of NCHW labels (strided planes); (losses[2], dimg) on the host."""
    from michigan_amd import ops
    img = _image(fx["fake"], dtype, channels)
    sem_tag = torch.stack([fx["m_b"], fx["m_f"]], dim=1).cuda()
    sem_ref = torch.stack([1 - fx["m_r"], fx["m_r"]], dim=1).cuda()
    out = ops.hair_lab_losses(img, fx["ref"].cuda(), sem_tag[:, 1], sem_ref[:, 1], fx["tgt"].cuda(), sem_tag[:, 0], flags=flags)
    wh, wb = weights if weights is not None else fx["weights"].tolist()
    (wh * out[0] + wb * out[1]).backward()
    torch.cuda.synchronize()
    return torch.stack([o.detach() for o in out]).cpu(), img.grad.detach().cpu()


@pytest.mark.parametrize("tag", ["i", "ii"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_kernels_match_the_reference(hip_backend, tag, dtype):
    fx = pair(tag)
    weights = tuple(fx["weights"].tolist())
    if dtype == torch.float32:
        want_l, want_g = fx["losses"], fx["grad"]
        bound = max(4 * float(fx["ref32_grad_rel_l2"]), 8 * 2.0 ** -23)
    else:
        rounded = fx["fake"].to(torch.bfloat16).float()
        want_l, want_g, (da, db) = K.hair_terms(rounded, fx["ref"], fx["m_f"], fx["m_r"], fx["tgt"], fx["m_b"], 3, weights)
        assert torch.equal(torch.sign(da), torch.sign(fx["da"])) and torch.equal(torch.sign(db), torch.sign(fx["db"]))
        bound = 2.0 ** -8
    got_l, got_g = _run(fx, dtype, 8)
    got_g3 = got_g[..., :3].permute(0, 3, 1, 2).double()
    rel_l = [abs(float(got_l[k]) - float(want_l[k])) / max(1.0, abs(float(want_l[k]))) for k in range(2)]
    rel_g = float((got_g3 - want_g).norm() / want_g.norm())
    worst = float((got_g3 - want_g).abs().max() / want_g.abs().max())
    print("hair lab %s %s: losses %s want %s rel %s | grad rel L2 %.3e (bound %.3e), worst element / largest %.3e"
          % (tag, dtype, got_l.tolist(), [float(v) for v in want_l], ["%.2e" % v for v in rel_l], rel_g, bound, worst))
    assert max(rel_l) <= LOSS_RTOL[dtype], rel_l
    assert rel_g <= bound, (rel_g, bound)
    assert float(got_g[..., 3:].abs().max()) == 0.0                # padding channels of dimg


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_flag_subsets_layouts_and_reproducibility(hip_backend, dtype):
    from michigan_amd import ops
    fx = pair("i")
    all_l, all_g = _run(fx, dtype, 8)
    again_l, again_g = _run(fx, dtype, 8)
    assert torch.equal(all_l, again_l) and torch.equal(all_g, again_g), "ordered sums: two runs must be bit-identical"
    assert float(all_g[..., 3:].abs().max()) == 0.0
    l3, g3 = _run(fx, dtype, 3)
    assert torch.equal(l3, all_l) and torch.equal(g3, all_g[..., :3]), "C = 3 and C = 8 layouts must agree"
    parts = 0
    for flags in (1, 2):
        l, g = _run(fx, dtype, 8, flags=flags)
        for k in range(2):
            if flags & (1 << k):
                assert float(l[k]) == float(all_l[k]), (flags, k)  # bit for bit the value of the both-bits call
            else:
                assert float(l[k]) == 0.0, (flags, k)
        assert float(g[..., 3:].abs().max()) == 0.0
        if flags == 1:                                             # the hair term alone: exactly 0 where m_f == 0
            assert float((g[..., :3] * (fx["m_f"] == 0).unsqueeze(-1)).abs().max()) == 0.0
            assert float((g[..., :3] * (fx["m_f"] != 0).unsqueeze(-1)).abs().max()) > 0.0
        parts = parts + g.double()
    # the two one-bit gradients add up to the fused one (one rounding per term and element)
    tol = 2.0 ** -7 if dtype == torch.bfloat16 else 1e-6
    assert float((parts - all_g.double()).norm() / all_g.double().norm()) <= tol
    # the background value is the colour pass's (another partition of the same sum)
    img = _image(fx["fake"], dtype, 8)
    sem_tag = torch.stack([fx["m_b"], fx["m_f"]], dim=1).cuda()
    want = float(ops.color_losses(img, fx["tgt"].cuda(), sem_tag[:, 0], ops.COLOR_BACKGROUND)[2].detach())
    print("background %s: hair pass %.9g colour pass %.9g" % (dtype, float(all_l[1]), want))
    assert abs(float(all_l[1]) - want) <= LOSS_RTOL[dtype] * max(1.0, abs(want))


@pytest.mark.parametrize("shape", [(1, 96, 80), (1, 67, 35), (3, 33, 130)], ids=["n1", "odd", "n3"])
@pytest.mark.parametrize("channels", [3, 8])
def test_other_geometries_against_the_contract(hip_backend, shape, channels):
    """N = 1 and geometries that are no multiple of a workgroup: every sample's sums stay its own."""
    n, h, w = shape
    g = torch.Generator().manual_seed(h * w)
    rnd = lambda *s: torch.rand(*s, generator=g)
    shift = lambda: (rnd(n, 3, 1, 1) - 0.5)
    fx = {"fake": (0.5 * (rnd(n, 3, h, w) * 2 - 1) + shift()).clamp(-1, 1), "ref": (0.5 * (rnd(n, 3, h, w) * 2 - 1) - shift()).clamp(-1, 1),
          "tgt": rnd(n, 3, h, w) * 2 - 1, "m_f": (rnd(n, h, w) > 0.6).float(), "m_r": (rnd(n, h, w) > 0.5).float()}
    fx["m_b"] = 1 - fx["m_f"]
    weights = (0.5, 40.0)
    want_l, want_g, (da, db) = K.hair_terms(fx["fake"], fx["ref"], fx["m_f"], fx["m_r"], fx["tgt"], fx["m_b"], 3, weights)
    assert float(torch.cat([da, db]).abs().min()) >= 1.0, "a mean difference too close to the discontinuity of sign(): pick another seed"
    got_l, got_g = _run(fx, torch.float32, channels, weights=weights)
    got_g3 = got_g[..., :3].permute(0, 3, 1, 2).double()
    rel_l = [abs(float(got_l[k]) - float(want_l[k])) / max(1.0, abs(float(want_l[k]))) for k in range(2)]
    rel_g = float((got_g3 - want_g).norm() / want_g.norm())
    print("hair lab %s C=%d: losses rel %s | grad rel L2 %.3e | min |d| %.3f" % (shape, channels, ["%.2e" % v for v in rel_l], rel_g, float(torch.cat([da, db]).abs().min())))
    assert max(rel_l) <= LOSS_RTOL[torch.float32], rel_l
    assert rel_g <= 8 * 2.0 ** -23, rel_g                          # the fp32 bound of test_kernels_match_the_reference without a stored reference error


def test_trainer_fp32_unpaired_matches_reference_trainer_golden(hip_backend):
    """tests/test_gpu_color_loss.py's fp32 trainer protocol and tolerances, through the unpaired stage."""
    from michigan_amd.model import Pix2PixTrainer
    cfg = dict(TP.CFGS["A"], tag="U")
    torch.manual_seed(0)
    trainer = Pix2PixTrainer(TP.repo_options(cfg, gpu_ids=[0], compute_dtype="fp32", unpairTrain=True))
    HE.load_weights(trainer, cfg)
    rec = HE.drive_unpaired(trainer, cfg, device="cuda")
    print("trainer U losses", {k: float(v) for k, v in rec.items() if ".loss." in k})
    gold = PU.load_trainer_golden("U")
    assert {k for k in rec if ".loss." in k} == {k for k in gold if ".loss." in k}
    TP.compare(rec, gold, rtol_loss0=5e-4, rtol_later=TP.RTOL_LATER_HIP, atol_img=1e-3, atol_weight=2 * 4e-4 * 2 + 1e-5)


def test_bf16_unpaired_step_at_full_width(hip_backend):
    """One generator + discriminator step of the unpaired stage at ngf 64 / 512x512 / batch 2 in bf16."""
    from michigan_amd.model import Pix2PixTrainer, default_options
    from michigan_amd.synth import synth_batch
    torch.manual_seed(0)
    trainer = Pix2PixTrainer(default_options(gpu_ids=[0], unpairTrain=True, curr_step=2))
    m = trainer.pix2pix_model
    before = {k: v.detach().clone() for k, v in m.netD.state_dict().items()}
    d2 = {k: v.detach().clone() for k, v in m.netD2.named_parameters()}
    data = {k: v.cuda() for k, v in synth_batch(2, 512, seed=1234, unpaired=True).items()}
    trainer.run_generator_one_step(data)
    trainer.run_discriminator_one_step(data)
    torch.cuda.synchronize()
    losses = {k: float(v.detach().float().mean()) for k, v in trainer.get_latest_losses().items()}
    print("bf16 unpaired step", losses)
    assert set(losses) == {"GAN", "ORIENT", "hairAvgLab", "background", "D_Fake", "D_real"}
    assert all(torch.isfinite(torch.tensor(v)) for v in losses.values()), losses
    assert losses["hairAvgLab"] > 0 and losses["background"] > 0
    assert all(torch.equal(v, before[k]) for k, v in m.netD.state_dict().items()), "netD must be untouched at curr_step 2"
    assert any(not torch.equal(v.detach(), d2[k]) for k, v in m.netD2.named_parameters()), "netD2 did not train"
