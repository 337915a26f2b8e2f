"""TEST INFRASTRUCTURE ONLY -- fixtures of the unpaired-stage tests: the seeded inputs of tests/golden/hair_lab_{i,ii}.npz (`make_pairs`),
their loader, and the protocol that drives a trainer through the unpaired stage (`drive_unpaired`: what tests/golden/trainer_U*.npz
holds).  The float64 contract itself is oracle/contracts.hair_terms.
"""
import numpy as np
import torch

import parity_utils as PU

N, H, W = 2, 96, 80


# ---- the seeded inputs of tests/golden/hair_lab_{i,ii}.npz (shared with tools/make_unpaired_golden.py) ------------------------------
def _ellipse(cy, cx, ry, rx):
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    return ((((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2) <= 1.0).float()


def make_pairs():
    """{tag: dict(fake, ref, tgt [N,3,H,W]; m_f, m_r, m_b [N,H,W])}.
    i : different ellipses for tag and reference, a colour cast per image, the top H/8 rows of fake within 0.01 of -1 (linear branch of f);
    ii: sample 0 with an empty reference mask and a tag mask of 0.5 on a few rows, sample 1 with an empty tag mask."""
    g = torch.Generator().manual_seed(2025)

    def image(shift):
        """U(-1, 1) noise of half amplitude around a colour: the means over a mask are then far apart between images"""
        x = 0.5 * (torch.rand(N, 3, H, W, generator=g) * 2 - 1) + torch.stack([torch.tensor(s) for s in shift]).view(N, 3, 1, 1)
        return x.clamp(-1, 1)
    out = {}
    fake = image([(0.4, -0.3, -0.2), (-0.3, 0.35, -0.1)])
    fake[:, :, :H // 8] = -1 + 0.01 * torch.rand(N, 3, H // 8, W, generator=g)
    ref = image([(-0.35, 0.3, 0.3), (0.3, -0.35, 0.4)])
    tgt = image([(0.0, 0.1, -0.1), (0.1, 0.0, 0.2)])
    m_f = torch.stack([_ellipse(30, 40, 40, 28), _ellipse(36, 36, 42, 22)])     # both reach the dark rows at the top
    m_r = torch.stack([_ellipse(52, 44, 24, 30), _ellipse(40, 40, 30, 30)])
    out["i"] = dict(fake=fake, ref=ref, tgt=tgt, m_f=m_f, m_r=m_r, m_b=1 - m_f)
    fake = image([(0.35, -0.3, 0.2), (0.2, 0.3, -0.3)])
    ref = image([(-0.3, 0.35, -0.3), (-0.3, -0.2, 0.35)])
    tgt = image([(0.1, -0.1, 0.0), (-0.1, 0.1, 0.1)])
    m_f = torch.stack([_ellipse(48, 40, 30, 26), torch.zeros(H, W)])
    m_b = 1 - m_f                                                   # the one-hot label's channel 0, before the non-binary rows
    m_f[0, 40:44] *= 0.5                                            # "the mask value multiplies"
    m_r = torch.stack([torch.zeros(H, W), _ellipse(50, 38, 28, 24)])
    out["ii"] = dict(fake=fake, ref=ref, tgt=tgt, m_f=m_f, m_r=m_r, m_b=m_b)
    return out


def load_pair(tag):
    """tests/golden/hair_lab_<tag>.npz as tensors (scalars as Python numbers)."""
    return PU.load_tensors("hair_lab_%s.npz" % tag)


# ---- the unpaired trainer protocol -------------------------------------------------------------------------------------------------
def unpaired_argv(cfg, checkpoints_dir):
    from oracle import trainer_parity as TP
    return TP.reference_argv(cfg, checkpoints_dir) + ["--unpairTrain"]


def load_weights(trainer, cfg):
    """oracle.trainer_parity.load_weights + a seeded netD2 (left at its xavier / 0.02 init the GAN term would be ~1e-5)."""
    from michigan_amd.synth import synth_state_dict
    from oracle import trainer_parity as TP
    TP.load_weights(trainer, cfg)
    net = trainer.pix2pix_model_on_one_gpu.netD2
    dev = next(net.parameters()).device
    sd = synth_state_dict({k: v.cpu() for k, v in net.state_dict().items()}, seed=cfg["seed_d"] + 1000, gain=cfg["gain"])
    net.load_state_dict({k: v.to(dev) for k, v in sd.items()})


def _set_step(trainer, step):
    trainer.opt.curr_step = step
    trainer.pix2pix_model_on_one_gpu.opt.curr_step = step


def drive_unpaired(trainer, cfg, device="cpu"):
    """cfg['iters'] x (curr_step 2: generator + discriminator step on the unpaired batch; curr_step 1: both steps on the paired batch of
    the same seed), the shared Python RNG seeded before each of the four steps.  Keys: it<i>.* the unpaired half, it<i>p.* the paired
    half (so that oracle.trainer_parity.compare treats only what precedes the first optimiser step as iteration 0), G.* / D.* the
    weights of oracle.trainer_parity, D.2.* the same names of netD2."""
    from michigan_amd import parallel
    from michigan_amd.synth import synth_loader_batch
    from oracle import trainer_parity as TP
    rec = {}
    to = lambda d: {k: (v.to(device).clone() if torch.is_tensor(v) else v) for k, v in d.items()}
    try:
        for it in range(cfg["iters"]):
            for half, (step, unpaired) in enumerate(((2, True), (1, False))):
                data = synth_loader_batch(cfg["n"], cfg["crop"], seed=cfg["seed_x"] + it, unpaired=unpaired)
                _set_step(trainer, step)
                parallel.seed_shared_rng(cfg["seed_py"] + 4 * it + 2 * half)
                trainer.run_generator_one_step(to(data))
                parallel.seed_shared_rng(cfg["seed_py"] + 4 * it + 2 * half + 1)
                trainer.run_discriminator_one_step(to(data))
                pre = "it%d%s." % (it, "" if unpaired else "p")
                for k, v in trainer.get_latest_losses().items():
                    rec[pre + "loss." + k] = np.array(float(v.detach().float().mean()))
                gen = trainer.get_latest_generated().detach().float().cpu()
                rec[pre + "generated_stat"] = TP._stats(gen)
                if it == 0:
                    rec[pre + "generated"] = gen.numpy().astype(np.float32)
    finally:
        _set_step(trainer, 1)
    m = trainer.pix2pix_model_on_one_gpu
    for pre, sd, names in (("G.", m.netG.state_dict(), TP.G_WEIGHTS + TP.G_BUFFERS), ("D.", m.netD.state_dict(), TP.D_WEIGHTS + TP.D_BUFFERS),
                           ("D.2.", m.netD2.state_dict(), TP.D_WEIGHTS + TP.D_BUFFERS)):
        for k in names:
            rec[pre + k] = sd[k].detach().float().cpu().numpy()
    return rec


STEP2_KEYS = ("GAN", "ORIENT", "hairAvgLab", "background", "D_Fake", "D_real")
