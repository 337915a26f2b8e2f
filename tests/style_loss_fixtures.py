"""TEST INFRASTRUCTURE ONLY -- fixtures of the style / content tests: the seeded feature sets of tests/golden/style_loss_{i,ii}.npz
(`make_sets`: the fixtures hold only what the reference computed on them), their loader, the mirror of the kernels' chunking
(`kernel_geometry`, `workspace_layout_bytes`) and the trainer protocol with the two terms on (`drive_style`: what
tests/golden/trainer_S*.npz holds).  The float64 contract itself is oracle/contracts.style_terms.
"""
import numpy as np
import torch

import parity_utils as PU

WEIGHTS = (0.7, 1.3)                                   # (w_s, w_c) of the stored gradient d(w_s style + w_c content) / dx


# ---- the seeded feature sets of tests/golden/style_loss_{i,ii}.npz (shared with tools/make_style_golden.py) ---------------------------
def make_sets():
    """{tag: dict(x, s, t [N, C, h, w] fp32; mask_x, mask_s, mask_t [N, h, w] fp32)} -- mask_x multiplies the fake features x, mask_s the
    style features s, mask_t the content term.
    i : N=2, C=24, 5x7, unit-scale features, binary masks;
    ii: N=3, C=136, 9x11, features 8 + 0.25 noise (a mean 32 standard deviations from 0: sums of squares that are not taken about a
        pivot cancel), sample 1 with an empty mask_x, sample 2 with an empty mask_s, fractional values in all three masks."""
    g = torch.Generator().manual_seed(4711)
    out = {}
    n, c, h, w = 2, 24, 5, 7
    feats = lambda scale, shift: shift + scale * torch.randn(n, c, h, w, generator=g)
    binary = lambda p: (torch.rand(n, h, w, generator=g) < p).float()
    out["i"] = dict(x=feats(1.0, 0.3).relu(), s=feats(1.2, 0.1).relu(), t=feats(1.0, 0.2).relu(),
                    mask_x=binary(0.6), mask_s=binary(0.5), mask_t=binary(0.7))
    n, c, h, w = 3, 136, 9, 11
    mx, ms, mt = binary(0.6), binary(0.55), binary(0.65)
    mx[1], ms[2] = 0.0, 0.0
    mx[0, 2:4] *= 0.5
    mx[2, :, 3] *= 0.25
    ms[0, 4:6] *= 0.75
    ms[1, 1] *= 0.5
    mt[:, 5:7] *= 0.5
    mt[1, :, 0] *= 0.3
    out["ii"] = dict(x=feats(0.25, 8.0), s=feats(0.3, 8.1), t=feats(0.25, 7.9), mask_x=mx, mask_s=ms, mask_t=mt)
    return out


def load_set(tag):
    """tests/golden/style_loss_<tag>.npz as tensors (scalars as Python numbers)."""
    return PU.load_tensors("style_loss_%s.npz" % tag)


# ---- the kernels' chunking (michigan_amd/csrc/mg_feat_moments.hip fm_geom / fm_layout), for the tests that sit on its edges -----------
def kernel_geometry(bf16, n, p, c):
    """dict(vec, cv, tile_cv, ctiles, rows, chunk, nchunks): a workgroup owns `chunk` pixels of one sample and min(cv, 256) 16-byte
    channel vectors, `rows` pixels at a time (a chunk is at least max(4 rows, 128) pixels).  The tests assert the library's workspace size against `workspace_layout_bytes`, so a
    change of the kernel's geometry that this mirror misses fails loudly instead of moving the edge cases off the edges."""
    vec = 8 if bf16 else 4
    cv = c // vec
    tile_cv, ctiles = min(cv, 256), -(-cv // 256)
    rows = 256 // tile_cv
    want = min(max(2048 // (n * ctiles), 1), 256)
    cps = min(want, -(-p // max(rows * 4, 128)))
    chunk = -(-(-(-p // cps)) // rows) * rows
    return dict(vec=vec, cv=cv, tile_cv=tile_cv, ctiles=ctiles, rows=rows, chunk=chunk, nchunks=-(-p // chunk))


def workspace_layout_bytes(n, p, c):
    def one(bf16):
        g = kernel_geometry(bf16, n, p, c)
        cnt = -(-(n * g["nchunks"] * 9 * 8 + n * (-(-c // 16)) * 8) // 16) * 16
        return -(-(cnt + 16 + n * g["nchunks"] * 10 * c * 4 + n * g["nchunks"] * g["ctiles"] * 4) // 16) * 16
    return max(one(False), one(True) if c % 8 == 0 else 0)


# ---- the trainer protocol with the two terms on (what tests/golden/trainer_S*.npz holds) ------------------------------------------------
STYLE_LOSS_KEYS = {0: ("GAN", "GAN_Feat", "VGG", "content", "style", "ORIENT", "D_Fake", "D_real"),
                   1: ("GAN", "content", "style", "ORIENT", "D_Fake", "D_real")}        # iteration 1: the reference is not the target


def style_argv(cfg, checkpoints_dir):
    """The README flags minus --no_style_loss / --no_content_loss."""
    from oracle import trainer_parity as TP
    return [a for a in TP.reference_argv(cfg, checkpoints_dir) if a not in ("--no_style_loss", "--no_content_loss")]


def load_weights(trainer, cfg):
    """oracle.trainer_parity.load_weights; a style tower of its own (the reference's) gets the VGG tower's weights: the reference loads
    one pretrained file into both."""
    from oracle import trainer_parity as TP
    TP.load_weights(trainer, cfg)
    m = trainer.pix2pix_model_on_one_gpu
    if m.criterionStyleContent.vgg is not m.criterionVGG.vgg:
        m.criterionStyleContent.vgg.load_state_dict(m.criterionVGG.vgg.state_dict())


def drive_style(trainer, cfg, device="cpu"):
    """cfg['iters'] x (generator step, discriminator step): iteration 0 on the paired batch, every later one on an unpaired batch (the
    reference mask differs from the tag mask: style / content are computed, GAN_Feat / VGG are not).  Keys as
    oracle.trainer_parity.drive, every loss the trainer reports."""
    from michigan_amd import parallel
    from michigan_amd.synth import synth_loader_batch
    from oracle import trainer_parity as TP
    rec = {}
    to = lambda d: {k: (v.to(device).clone() if torch.is_tensor(v) else v) for k, v in d.items()}
    for it in range(cfg["iters"]):
        data = synth_loader_batch(cfg["n"], cfg["crop"], seed=cfg["seed_x"] + it, unpaired=it > 0)
        trainer.init_losses()
        parallel.seed_shared_rng(cfg["seed_py"] + 2 * it)
        trainer.run_generator_one_step(to(data))
        parallel.seed_shared_rng(cfg["seed_py"] + 2 * it + 1)
        trainer.run_discriminator_one_step(to(data))
        for k, v in trainer.get_latest_losses().items():
            rec["it%d.loss.%s" % (it, k)] = np.array(float(v.detach().float().mean()))
        gen = trainer.get_latest_generated().detach().float().cpu()
        rec["it%d.generated_stat" % it] = TP._stats(gen)
        if it == 0:
            rec["it0.generated"] = gen.numpy().astype(np.float32)
    m = trainer.pix2pix_model_on_one_gpu
    for pre, sd, names in (("G.", m.netG.state_dict(), TP.G_WEIGHTS + TP.G_BUFFERS), ("D.", m.netD.state_dict(), TP.D_WEIGHTS + TP.D_BUFFERS)):
        for k in names:
            rec[pre + k] = sd[k].detach().float().cpu().numpy()
    return rec
