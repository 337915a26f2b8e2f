"""TEST INFRASTRUCTURE ONLY -- the float64 contract of mg_hair_lab_fwd / mg_hair_lab_bwd (include/michigan_hip.h) on plain
tensors (`hair_terms`) and on top of the C-ABI contract emulator (`HairLabEmulator`, which also carries the colour pass of
tests/color_loss_emulator.py), the protocol that drives a trainer through the unpaired stage (`drive_unpaired`: what
tests/golden/trainer_U*.npz holds), the seeded inputs of tests/golden/hair_lab_{i,ii}.npz and the fixture loaders.

Works on host memory through the raw pointers the kernels get, computes in float64 and rounds once to the storage dtype.
The product never imports it.
"""
import os

import numpy as np
import torch

import color_loss_emulator as CE
from color_loss_emulator import _Record
from oracle.cabi_emulator import _TD, _addr, _view

HAIR, BACKGROUND = 1, 2
N, H, W = 2, 96, 80
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def hair_terms(fake, ref, m_f, m_r, tgt=None, m_b=None, flags=3, weights=(1.0, 1.0)):
    """float64 contract on plain tensors: fake / ref / tgt [N, 3, H, W], m_f / m_r / m_b [N, H, W]; operands of a term that is
    not selected may be None.  Returns (losses[2], d(sum_k weights[k] * losses[k]) / d fake [N, 3, H, W], (da[N], db[N]))."""
    fake = fake.double()
    n, _, h, w = fake.shape
    out = torch.zeros(2, dtype=torch.float64)
    grad = torch.zeros_like(fake)
    da = db = None
    if flags & HAIR:
        mf, mr = m_f.double(), m_r.double()
        xyz_f = CE._xyz(fake)
        af, bf = CE._ab(xyz_f)
        ar, br = CE._ab(CE._xyz(ref.double()))
        sf, sr = mf.sum(dim=(1, 2)), mr.sum(dim=(1, 2))
        sf, sr = torch.where(sf == 0, torch.ones_like(sf), sf), torch.where(sr == 0, torch.ones_like(sr), sr)
        da = (mf * af).sum(dim=(1, 2)) / sf - (mr * ar).sum(dim=(1, 2)) / sr
        db = (mf * bf).sum(dim=(1, 2)) / sf - (mr * br).sum(dim=(1, 2)) / sr
        out[0] = (da.abs().sum() + db.abs().sum()) / (2 * n)
        sa, sb = 500 * torch.sign(da)[:, None, None], 200 * torch.sign(db)[:, None, None]
        dfx = CE._df(xyz_f)
        dxyz = torch.stack([sa * dfx[:, 0], (sb - sa) * dfx[:, 1], -sb * dfx[:, 2]], dim=1)
        scale = (mf / sf[:, None, None]).unsqueeze(1)
        grad += weights[0] / (2 * n) * 0.5 * scale * torch.einsum("rc,nrhw->nchw", CE.MN, dxyz)
    if flags & BACKGROUND:
        m = m_b.double().unsqueeze(1)
        dm = fake * m - tgt.double() * m
        out[1] = dm.abs().sum() / (n * 3 * h * w)
        grad += weights[1] / (n * 3 * h * w) * torch.sign(dm) * m
    return out, grad, (da, db)


class HairLabEmulator(CE.ColorLossEmulator):
    """ColorLossEmulator + the two entry points of mg_hair_lab.hip; counts its calls (tests check launches per step)."""

    def __init__(self):
        super().__init__()
        self.hair_calls = {"fwd": [], "bwd": []}

    @staticmethod
    def _image(ptr, nstride, N, H, W):
        base = _view(ptr, ((N - 1) * nstride + 3 * H * W,), torch.float32)
        return torch.as_strided(base, (N, 3, H, W), (nstride, H * W, W, 1)).double()

    def _hair_inputs(self, img, ref, ref_nstride, hair_tag, hair_tag_nstride, hair_ref, hair_ref_nstride, tgt, tgt_nstride, back, back_nstride,
                     dtype, N, H, W, C, flags):
        assert 1 <= flags <= 3 and C >= 3
        x = _view(img, (N, H, W, C), _TD[dtype]).double()[..., :3].permute(0, 3, 1, 2)
        r = mf = mr = t = mb = None
        if flags & HAIR:
            mf = self._plane(hair_tag, N, hair_tag_nstride, H, W).double()
            if _addr(ref):                                               # the backward does not get ref / hair_ref
                r, mr = self._image(ref, ref_nstride, N, H, W), self._plane(hair_ref, N, hair_ref_nstride, H, W).double()
        if flags & BACKGROUND:
            t, mb = self._image(tgt, tgt_nstride, N, H, W), self._plane(back, N, back_nstride, H, W).double()
        return x, r, mf, mr, t, mb

    def mg_hair_lab_fwd(self, img, ref, ref_nstride, hair_tag, hair_tag_nstride, hair_ref, hair_ref_nstride, tgt, tgt_nstride, back, back_nstride,
                        dtype, N, H, W, C, flags, out, stats, ws, stream=None):
        self.hair_calls["fwd"].append(flags)
        x, r, mf, mr, t, mb = self._hair_inputs(img, ref, ref_nstride, hair_tag, hair_tag_nstride, hair_ref, hair_ref_nstride, tgt, tgt_nstride,
                                                back, back_nstride, dtype, N, H, W, C, flags)
        losses, _, (da, db) = hair_terms(x, r, mf, mr, t, mb, flags)
        _view(out, (2,), torch.float32)[:] = losses.float()
        if flags & HAIR:
            sf, sr = mf.sum(dim=(1, 2)), mr.sum(dim=(1, 2))
            inv = lambda s: 1.0 / torch.where(s == 0, torch.ones_like(s), s)
            _view(stats, (N, 4), torch.float32)[:] = torch.stack([da, db, inv(sf), inv(sr)], dim=1).float()
        return 0

    def mg_hair_lab_bwd(self, img, hair_tag, hair_tag_nstride, tgt, tgt_nstride, back, back_nstride, stats, g_hair, g_back,
                        dtype, N, H, W, C, flags, dimg, stream=None):
        """Uses what the kernel uses: the per-sample signs and 1 / S_f of `stats`, no second reduction."""
        self.hair_calls["bwd"].append(flags)
        x, _, mf, _, t, mb = self._hair_inputs(img, None, 0, hair_tag, hair_tag_nstride, None, 0, tgt, tgt_nstride, back, back_nstride,
                                               dtype, N, H, W, C, flags)
        g = [float(_view(p, (1,), torch.float32)[0]) if _addr(p) else 0.0 for p in (g_hair, g_back)]
        grad = torch.zeros_like(x)
        if flags & HAIR:
            st = _view(stats, (N, 4), torch.float32).double()
            xyz_f = CE._xyz(x)
            sa, sb = 500 * torch.sign(st[:, 0])[:, None, None], 200 * torch.sign(st[:, 1])[:, None, None]
            dfx = CE._df(xyz_f)
            dxyz = torch.stack([sa * dfx[:, 0], (sb - sa) * dfx[:, 1], -sb * dfx[:, 2]], dim=1)
            grad += g[0] / (2 * N) * 0.5 * (mf * st[:, 2][:, None, None]).unsqueeze(1) * torch.einsum("rc,nrhw->nchw", CE.MN, dxyz)
        if flags & BACKGROUND:
            grad += hair_terms(x, None, None, None, t, mb, BACKGROUND, (0.0, g[1]))[1]
        d = _view(dimg, (N, H, W, C), _TD[dtype])
        d.zero_()
        d[..., :3] = grad.permute(0, 2, 3, 1).to(_TD[dtype])
        return 0


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
    z = np.load(os.path.join(GOLDEN, "hair_lab_%s.npz" % tag))
    return {k: (torch.from_numpy(z[k]) if z[k].ndim else z[k].item()) for k in z.files}


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


def load_trainer_golden():
    """trainer_U.npz + trainer_U_weights.npz (one record, split in two files to keep each under the size limit of a committed file)."""
    rec = {}
    for fn in ("trainer_U.npz", "trainer_U_weights.npz"):
        with np.load(os.path.join(GOLDEN, fn)) as z:
            rec.update({k: z[k] for k in z.files})
    return _Record(rec)
