"""TEST INFRASTRUCTURE ONLY -- the float64 contract of mg_feat_moment_loss_fwd / mg_feat_moment_loss_bwd
(include/michigan_hip/feature_losses.h) on plain tensors (`style_terms`) and on top of the C-ABI contract emulator
(`StyleLossEmulator`, which also carries the colour and hair-Lab passes of tests/hair_lab_emulator.py), the seeded feature sets of
tests/golden/style_loss_{i,ii}.npz (`make_sets`: the fixtures hold only what the reference computed on them) and the loaders.

Works on host memory through the raw pointers the kernels get, computes in float64 and rounds once to the storage dtype.
The product never imports it.
"""
import os

import numpy as np
import torch

from hair_lab_emulator import GOLDEN, HairLabEmulator
from oracle.cabi_emulator import _TD, _addr, _view

STYLE, CONTENT = 1, 2
EPS = 1e-5
WEIGHTS = (0.7, 1.3)                                   # (w_s, w_c) of the stored gradient d(w_s style + w_c content) / dx


def _kept(f, m):
    """f where the mask is non-zero, 0 elsewhere: what is masked out is not read (a NaN there reaches nothing)"""
    return torch.where((m != 0).unsqueeze(1), f, torch.zeros_like(f))


def moments(f, m=None):
    """(mu, sigma, S, T) per (n, c) of f [N, C, P] (float64) under m [N, P] or unmasked (calc_mean_std / calc_mean_std_mask)."""
    if m is None:
        p = f.shape[2]
        mu = f.mean(dim=2)
        return mu, (((f - mu.unsqueeze(2)) ** 2).sum(dim=2) / (p - 1) + EPS).sqrt(), None, None
    f = _kept(f, m)
    mm = m.unsqueeze(1)
    s = (m.sum(dim=1) + EPS).unsqueeze(1)                                     # [N, 1]
    mu = (f * mm).sum(dim=2) / s
    r = (f * mm - mu.unsqueeze(2)) * mm
    return mu, ((r ** 2).sum(dim=2) / s + EPS).sqrt(), s, (r * mm).sum(dim=2)


def coefficients(x, s, mask_x=None, mask_s=None):
    """(style, a, b, mu_x) of one tap: the style term and the table the backward reads; x, s [N, C, P] float64."""
    n, c, p = x.shape
    mu_x, sg_x, S, T = moments(x, mask_x)
    mu_s, sg_s, _, _ = moments(s, mask_s)
    style = (((mu_x - mu_s) ** 2) + ((sg_x - sg_s) ** 2)).sum() / (n * c)
    gm, gs = 2 * (mu_x - mu_s) / (n * c), 2 * (sg_x - sg_s) / (n * c)
    if mask_x is None:
        return style, gm / p, gs / (sg_x * (p - 1)), mu_x
    return style, gm / S - gs * T / (sg_x * S * S), gs / (sg_x * S), mu_x


def content_den(n, c, p, mask_t):
    return float(n * p * c) if mask_t is None else float(c * mask_t.sum() + EPS)


def gradient(x, t, mask_x, mask_t, a, b, mu_x, den, g_style, g_content):
    """dx = g_style (m a + m^3 b (m x - mu_x)) + g_content 2 l^2 (x - t) / den; x, t [N, C, P], a / b / mu_x [N, C]."""
    d = torch.zeros_like(x)
    if g_style:
        if mask_x is None:
            d = d + g_style * (a.unsqueeze(2) + b.unsqueeze(2) * (x - mu_x.unsqueeze(2)))
        else:
            m = mask_x.unsqueeze(1)
            d = d + g_style * (m * a.unsqueeze(2) + m ** 3 * b.unsqueeze(2) * (m * _kept(x, mask_x) - mu_x.unsqueeze(2)))
    if g_content:
        if mask_t is None:
            d = d + g_content * 2 * (x - t) / den
        else:
            l = mask_t.unsqueeze(1)
            d = d + g_content * 2 * l * l * (_kept(x, mask_t) - _kept(t, mask_t)) / den
    return d


def style_terms(x, s, t=None, mask_x=None, mask_s=None, mask_t=None, flags=3, weights=(1.0, 1.0)):
    """float64 contract on plain tensors: x / s / t NCHW [N, C, h, w], masks [N, h, w] or None; operands of a term that is not
    selected may be None.  Returns (losses[2], d(weights[0] style + weights[1] content) / dx [N, C, h, w])."""
    n, c, h, w = x.shape
    flat = lambda f: None if f is None else f.double().reshape(n, c, h * w)
    fm = lambda m: None if m is None else m.double().reshape(n, h * w)
    x3, s3, t3, mx, ms, ml = flat(x), flat(s), flat(t), fm(mask_x), fm(mask_s), fm(mask_t)
    out = torch.zeros(2, dtype=torch.float64)
    a = b = mu_x = None
    den = 1.0
    if flags & STYLE:
        out[0], a, b, mu_x = coefficients(x3, s3, mx, ms)
    if flags & CONTENT:
        den = content_den(n, c, h * w, ml)
        diff = x3 - t3 if ml is None else ml.unsqueeze(1) * (_kept(x3, ml) - _kept(t3, ml))
        out[1] = (diff ** 2).sum() / den
    grad = gradient(x3, t3, mx, ml, a, b, mu_x, den, weights[0] if flags & STYLE else 0.0, weights[1] if flags & CONTENT else 0.0)
    return out, grad.reshape(n, c, h, w)


def workspace_bytes(n, p, c):
    """Any positive size will do for the emulator; the real library's layout is its own business."""
    return 64 if n > 0 and p > 0 and c > 0 and c % 4 == 0 else 0


class StyleLossEmulator(HairLabEmulator):
    """HairLabEmulator + the extension group of michigan_hip/feature_losses.h; counts its calls (tests check launches per step)."""

    def __init__(self):
        super().__init__()
        self.feat_calls = {"fwd": [], "bwd": []}

    def mg_ext_version(self):
        return 1

    def mg_feat_moment_workspace(self, n, p, c):
        return workspace_bytes(n, p, c)

    @staticmethod
    def _feat(ptr, d):
        v = _view(ptr, (d.N, d.P, d.C), _TD[d.dtype])
        return None if v is None else v.double().permute(0, 2, 1)

    @staticmethod
    def _mask(ptr, nstride, d):
        if not _addr(ptr):
            return None
        base = _view(ptr, ((d.N - 1) * nstride + d.P,), torch.float32)
        return torch.as_strided(base, (d.N, d.P), (nstride, 1)).double()

    def _operands(self, d):
        assert 1 <= d.flags <= 3 and d.C % (8 if d.dtype == 1 else 4) == 0
        st, co = d.flags & STYLE, d.flags & CONTENT
        x = self._feat(d.x, d)
        s = self._feat(d.s, d) if st else None
        t = self._feat(d.t, d) if co else None
        mx = self._mask(d.mask_x, d.mask_x_nstride, d) if st else None
        ms = self._mask(d.mask_s, d.mask_s_nstride, d) if st else None
        ml = self._mask(d.mask_t, d.mask_t_nstride, d) if co else None
        assert (mx is None) == (ms is None)
        return x, s, t, mx, ms, ml

    def mg_feat_moment_loss_fwd(self, d, stream=None):
        self.feat_calls["fwd"].append(d.flags)
        x, s, t, mx, ms, ml = self._operands(d)
        out = _view(d.out, (2,), torch.float32)
        coef = _view(d.coef, (d.N, d.C, 4), torch.float32)
        out.zero_()
        coef.zero_()
        if d.flags & STYLE:
            style, a, b, mu_x = coefficients(x, s, mx, ms)
            out[0] = float(style)
            coef[..., 0], coef[..., 1], coef[..., 2] = a.float(), b.float(), mu_x.float()
        if d.flags & CONTENT:
            den = content_den(d.N, d.C, d.P, ml)
            diff = x - t if ml is None else ml.unsqueeze(1) * (_kept(x, ml) - _kept(t, ml))
            out[1] = float((diff ** 2).sum() / den)
            coef[..., 3] = 2.0 / den
        return 0

    def mg_feat_moment_loss_bwd(self, d, g_style, g_content, dx, stream=None):
        """Uses what the kernel uses: the fp32 table of the forward, no second reduction."""
        self.feat_calls["bwd"].append(d.flags)
        x = self._feat(d.x, d)
        gs, gc = [float(_view(p, (1,), torch.float32)[0]) if _addr(p) else 0.0 for p in (g_style, g_content)]
        gs, gc = (gs if d.flags & STYLE else 0.0), (gc if d.flags & CONTENT else 0.0)
        coef = _view(d.coef, (d.N, d.C, 4), torch.float32).double()
        mx = self._mask(d.mask_x, d.mask_x_nstride, d) if gs else None
        ml = self._mask(d.mask_t, d.mask_t_nstride, d) if gc else None
        t = self._feat(d.t, d) if gc else None
        den = 2.0 / float(coef[0, 0, 3]) if gc else 1.0
        grad = gradient(x, t, mx, ml, coef[..., 0], coef[..., 1], coef[..., 2], den, gs, gc)
        _view(dx, (d.N, d.P, d.C), _TD[d.dtype])[:] = grad.permute(0, 2, 1).to(_TD[d.dtype])
        return 0


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
    z = np.load(os.path.join(GOLDEN, "style_loss_%s.npz" % tag))
    return {k: (torch.from_numpy(z[k]) if z[k].ndim else z[k].item()) for k in z.files}


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


def load_trainer_golden():
    """trainer_S.npz + trainer_S_weights.npz (one record, split in two files like trainer_U)."""
    from color_loss_emulator import _Record
    rec = {}
    for fn in ("trainer_S.npz", "trainer_S_weights.npz"):
        with np.load(os.path.join(GOLDEN, fn)) as z:
            rec.update({k: z[k] for k in z.files})
    return _Record(rec)
