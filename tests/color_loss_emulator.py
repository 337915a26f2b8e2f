"""TEST INFRASTRUCTURE ONLY -- the float64 contract of mg_color_loss_fwd / mg_color_loss_bwd (include/michigan_hip.h)
on top of the C-ABI contract emulator (oracle/cabi_emulator.py), plus the same mathematics on plain tensors
(`color_terms`) for the tests that need a reference value on inputs of their own (e.g. a bf16-rounded image).

Like the emulator it extends, this works on host memory through the raw pointers the kernels get, computes in float64
and rounds once to the storage dtype.  The product never imports it.
"""
import torch

from oracle.cabi_emulator import EmulatorBackend, _TD, _addr, _view

LAB, RGB, BACKGROUND = 1, 2, 4
KNEE = 0.008856
# loss.py:409 is an fp32 tensor: the contract's matrix entries are those fp32 values, each row divided by its row sum
M = torch.tensor([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]], dtype=torch.float32).double()
MN = M / M.sum(dim=1, keepdim=True)


def _f(t):
    return torch.where(t > KNEE, t.clamp_min(KNEE).pow(1.0 / 3.0), 7.787 * t + 0.137931)


def _df(t):
    return torch.where(t > KNEE, t.clamp_min(KNEE).pow(-2.0 / 3.0) / 3.0, torch.full_like(t, 7.787))


def _xyz(x):
    """x [N, 3, H, W] in [-1, 1] -> XYZ [N, 3, H, W].  Spelled element-wise on purpose: the result must not depend on the memory
    layout of x (a library contraction may sum in another order for a strided operand), or an image equal to its target would
    not give da = db = 0 exactly."""
    c = (x + 1) / 2
    return torch.stack([float(MN[r, 0]) * c[:, 0] + float(MN[r, 1]) * c[:, 1] + float(MN[r, 2]) * c[:, 2] for r in range(3)], dim=1)


def _ab(xyz):
    f = _f(xyz)
    return 500 * (f[:, 0] - f[:, 1]), 200 * (f[:, 1] - f[:, 2])


def color_terms(fake, real, back, flags=7, weights=(1.0, 1.0, 1.0)):
    """float64 contract on plain tensors: fake / real [N, 3, H, W], back [N, H, W] or None.
    Returns (losses[3], d(sum_k weights[k] * losses[k]) / d fake [N, 3, H, W], deltas) where deltas = (da, db, drgb) are the
    differences the sign() of the gradient is taken of."""
    fake, real = fake.double(), real.double()
    n, _, h, w = fake.shape
    out = torch.zeros(3, dtype=torch.float64)
    grad = torch.zeros_like(fake)
    xyz_f = _xyz(fake)
    af, bf = _ab(xyz_f)
    ar, br = _ab(_xyz(real))
    da, db, drgb = af - ar, bf - br, fake - real
    if flags & LAB:
        out[0] = (da.abs().sum() + db.abs().sum()) / (n * 2 * h * w)
        sa, sb = 500 * torch.sign(da), 200 * torch.sign(db)
        dfx = _df(xyz_f)
        dxyz = torch.stack([sa * dfx[:, 0], (sb - sa) * dfx[:, 1], -sb * dfx[:, 2]], dim=1)
        grad += weights[0] / (n * 2 * h * w) * 0.5 * torch.einsum("rc,nrhw->nchw", MN, dxyz)
    if flags & RGB:
        out[1] = drgb.abs().sum() / (n * 3 * h * w)
        grad += weights[1] / (n * 3 * h * w) * torch.sign(drgb)
    if flags & BACKGROUND:
        m = back.double().unsqueeze(1)
        dm = fake * m - real * m
        out[2] = dm.abs().sum() / (n * 3 * h * w)
        grad += weights[2] / (n * 3 * h * w) * torch.sign(dm) * m
    return out, grad, (da, db, drgb)


class ColorLossEmulator(EmulatorBackend):
    """EmulatorBackend + the two entry points of mg_color_loss.hip; counts its calls (tests check launches per step)."""

    def __init__(self):
        self.color_calls = {"fwd": [], "bwd": []}

    def _color_inputs(self, img, real, real_nstride, back, back_nstride, dtype, N, H, W, C, flags):
        assert 1 <= flags <= 7 and C >= 3
        x = _view(img, (N, H, W, C), _TD[dtype]).double()[..., :3].permute(0, 3, 1, 2)
        base = _view(real, ((N - 1) * real_nstride + 3 * H * W,), torch.float32)
        r = torch.as_strided(base, (N, 3, H, W), (real_nstride, H * W, W, 1)).double()
        m = self._plane(back, N, back_nstride, H, W).double() if flags & BACKGROUND else None
        return x, r, m

    def mg_color_loss_fwd(self, img, real, real_nstride, back, back_nstride, dtype, N, H, W, C, flags, out, ws, stream=None):
        self.color_calls["fwd"].append(flags)
        x, r, m = self._color_inputs(img, real, real_nstride, back, back_nstride, dtype, N, H, W, C, flags)
        _view(out, (3,), torch.float32)[:] = color_terms(x, r, m, flags)[0].float()
        return 0

    def mg_color_loss_bwd(self, img, real, real_nstride, back, back_nstride, g_lab, g_rgb, g_back, dtype, N, H, W, C, flags, dimg, stream=None):
        self.color_calls["bwd"].append(flags)
        x, r, m = self._color_inputs(img, real, real_nstride, back, back_nstride, dtype, N, H, W, C, flags)
        g = [float(_view(p, (1,), torch.float32)[0]) if _addr(p) else 0.0 for p in (g_lab, g_rgb, g_back)]
        grad = color_terms(x, r, m, flags, g)[1]
        d = _view(dimg, (N, H, W, C), _TD[dtype])
        d.zero_()
        d[..., :3] = grad.permute(0, 2, 3, 1).to(_TD[dtype])
        return 0


COLOR_KEYS = ("background", "rgb", "lab")


class _ColorRecorder:
    """A trainer proxy that notes the three image-space losses after every generator step (oracle.trainer_parity.drive keeps
    its own fixed list of loss keys)."""

    def __init__(self, trainer):
        self.__dict__["_tr"], self.__dict__["seen"] = trainer, []

    def __getattr__(self, name):
        return getattr(self._tr, name)

    def run_generator_one_step(self, data):
        self._tr.run_generator_one_step(data)
        self.seen.append({k: float(self._tr.g_losses[k].detach().float().mean()) for k in COLOR_KEYS})


def drive_with_color_losses(trainer, cfg, device="cpu"):
    """oracle.trainer_parity.drive's record + it<i>.loss.{background,rgb,lab}: what tests/golden/trainer_C.npz holds."""
    import numpy as np
    from oracle import trainer_parity as TP
    rec_tr = _ColorRecorder(trainer)
    rec = TP.drive(rec_tr, cfg, device=device)
    for it, vals in enumerate(rec_tr.seen):
        for k, v in vals.items():
            rec["it%d.loss.%s" % (it, k)] = np.array(v)
    return rec


def color_argv(cfg, checkpoints_dir):
    """The README training flags AS PUBLISHED (Lab on) plus background and rgb on: oracle.trainer_parity.reference_argv
    without the three switches that turn the terms off."""
    from oracle import trainer_parity as TP
    return [a for a in TP.reference_argv(cfg, checkpoints_dir) if a not in ("--no_lab_loss", "--no_background_loss", "--no_rgb_loss")]


def load_trainer_golden():
    """trainer_C.npz + trainer_C_weights.npz (one record, split in two files to keep each under the size limit of a committed file)."""
    import os
    import numpy as np
    g = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    rec = {}
    for fn in ("trainer_C.npz", "trainer_C_weights.npz"):
        with np.load(os.path.join(g, fn)) as z:
            rec.update({k: z[k] for k in z.files})
    return _Record(rec)


class _Record(dict):
    """dict with the `.files` of an NpzFile (what oracle.trainer_parity.compare iterates)."""
    @property
    def files(self):
        return list(self)


def load_pair(tag):
    """tests/golden/color_loss_<tag>.npz as tensors (scalars as Python numbers)."""
    import os
    import numpy as np
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "color_loss_%s.npz" % tag))
    return {k: (torch.from_numpy(z[k]) if z[k].ndim else z[k].item()) for k in z.files}
