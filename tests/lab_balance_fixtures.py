"""TEST INFRASTRUCTURE ONLY -- fixtures of the --balance_Lab tests: the float64 contract of the colour-balance extension group
(include/michigan_hip/losses/lab_balance.h) on plain tensors, an EmulatorBackend subclass with its four entry points (the emulator under
oracle/ does not know the group), the reference's flags for the trainer record and the loaders of tests/golden/lab_balance_*.npz,
ab_count.npz and trainer_L*.npz (tools/make_lab_balance_golden.py).  The unbalanced contracts are oracle/contracts.color_terms and
hair_terms; what is added here is the weight.
"""
import os

import numpy as np
import torch

import parity_utils as PU
from oracle import contracts as K
from oracle.cabi_emulator import _TD, EmulatorBackend, _addr, _view

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BINS, HAIR_STATS = 256, 8                       # MGC_TABLE_BINS, MGC_HAIR_STATS
COLOR_KEYS = ("background", "rgb", "lab")


# ---- the table ---------------------------------------------------------------------------------------------------------------------------
def weight_table(counts, th):
    """S, fp32 [256, 256], as the header defines it: counts -> fp32 first, zeros -> 1, max / w, min(w, th), all in fp32; row 255 and
    column 255 are 0 (bin 255 falls outside the table under grid_sample's align_corners=False)."""
    w = torch.from_numpy(np.ascontiguousarray(counts)).to(torch.float32)
    w = torch.where(w == 0, torch.ones_like(w), w)
    w = torch.minimum(w.max() / w, torch.tensor(th, dtype=torch.float32))
    w[BINS - 1, :] = 0
    w[:, BINS - 1] = 0
    return w


def grid_sample_table(counts, th):
    """The reference's literal expression (loss.py:486-503 without the mask) over all 65536 bin pairs: entry [i][j] is what a pixel with
    a + 128 = i, b + 128 = j samples."""
    import torch.nn.functional as F
    weight = torch.FloatTensor(np.asarray(counts))[None, None]
    weight[weight == 0] = 1
    weight = weight.max() / weight
    weight[weight > th] = th
    a = torch.arange(BINS, dtype=torch.float32).view(1, 1, BINS, 1).expand(1, 1, BINS, BINS)
    b = torch.arange(BINS, dtype=torch.float32).view(1, 1, 1, BINS).expand(1, 1, BINS, BINS)
    m = torch.cat([b, a], 1)
    m = m.int().float()
    m = (m - 127.5) / 127.5
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)                          # "default behaviour has changed to align_corners=False": the point
        return F.grid_sample(weight, m.permute([0, 2, 3, 1]), mode="nearest")[0, 0]


def bins(v):
    """k(v) = trunc(clamp(v + 128, 0, 255)) of a Lab coordinate, as long"""
    return (v + 128).clamp(0, 255).long()


# ---- the float64 contracts -----------------------------------------------------------------------------------------------------------------
def color_weights(real, hair, S):
    """w [N, H, W] of the balanced colour pass: S[k(a_r)][k(b_r)] * hair, 1 where that is 0"""
    ar, br = K._ab(K._xyz(real.double()))
    w = S.double()[bins(ar), bins(br)] * hair.double()
    return torch.where(w == 0, torch.ones_like(w), w)


def color_terms(fake, real, back, hair, S, flags=7, weights=(1.0, 1.0, 1.0)):
    """oracle.contracts.color_terms with the Lab term weighted per pixel: (losses[3], d(sum_k weights[k] losses[k]) / d fake, deltas, w)"""
    assert flags & K.COLOR_LAB
    fake, real = fake.double(), real.double()
    n, _, h, w_ = fake.shape
    out, grad, deltas = K.color_terms(fake, real, back, flags & 6, weights) if flags & 6 else \
        (torch.zeros(3, dtype=torch.float64), torch.zeros_like(fake), K.color_terms(fake, real, None, 1)[2])
    da, db, _ = deltas
    w = color_weights(real, hair, S)
    out[0] = (w * (da.abs() + db.abs())).sum() / (n * 2 * h * w_)
    xyz_f = K._xyz(fake)
    sa, sb = 500 * torch.sign(da), 200 * torch.sign(db)
    dfx = K._df(xyz_f)
    dxyz = torch.stack([sa * dfx[:, 0], (sb - sa) * dfx[:, 1], -sb * dfx[:, 2]], dim=1)
    grad = grad + weights[0] / (n * 2 * h * w_) * 0.5 * w.unsqueeze(1) * torch.einsum("rc,nrhw->nchw", K.MN, dxyz)
    return out, grad, deltas, w


def ref_means(ref, m_r):
    """(mean a, mean b) [N] of the reference image's hair, an empty mask dividing by 1"""
    mr = m_r.double()
    ar, br = K._ab(K._xyz(ref.double()))
    sr = mr.sum(dim=(1, 2))
    sr = torch.where(sr == 0, torch.ones_like(sr), sr)
    return (mr * ar).sum(dim=(1, 2)) / sr, (mr * br).sum(dim=(1, 2)) / sr


def hair_weights(ref, m_r, S):
    """w_n [N] of the balanced hair pass: the means rounded to fp32 once, binned in fp32; no zero-to-one replacement"""
    ma, mb = ref_means(ref, m_r)
    return S.double()[bins(ma.float()), bins(mb.float())]


def hair_terms(fake, ref, m_f, m_r, S, tgt=None, m_b=None, flags=3, weights=(1.0, 1.0)):
    """oracle.contracts.hair_terms with sample n's hair term weighted by w_n: (losses[2], gradient, (da, db), w)"""
    assert flags & K.HAIR_LAB
    w = hair_weights(ref, m_r, S)
    _, g_h, (da, db) = K.hair_terms(fake, ref, m_f, m_r, None, None, K.HAIR_LAB, (weights[0], 0.0))
    out = torch.zeros(2, dtype=torch.float64)
    out[0] = (w * (da.abs() + db.abs())).sum() / (2 * fake.shape[0])
    grad = g_h * w[:, None, None, None]
    if flags & K.HAIR_BACKGROUND:
        o_b, g_b, _ = K.hair_terms(fake, None, None, None, tgt, m_b, K.HAIR_BACKGROUND, (0.0, weights[1]))
        out[1] = o_b[1]
        grad = grad + g_b
    return out, grad, (da, db), w


# ---- the emulator --------------------------------------------------------------------------------------------------------------------------
class LabBalanceEmulator(EmulatorBackend):
    """EmulatorBackend + the colour-balance extension group from the contracts above, results rounded to fp32 once.  Argument checks as the
    header states them; a refused call is in the log too, as the base class keeps it."""

    def _balance_operands(self, fn, hair, hair_nstride, table, N, H, W, flags):
        if not flags & 1:
            self._fail(fn, "flags must contain bit 1")
        if not _addr(table):
            self._fail(fn, "null pointer (table)")
        if not _addr(hair) or hair_nstride < H * W:
            self._fail(fn, "the balanced Lab term needs the hair plane")
        return self._plane(hair, N, hair_nstride, H, W).double(), _view(table, (BINS, BINS), torch.float32)

    def mgc_color_loss_balanced_fwd(self, img, real, real_nstride, back, back_nstride, hair, hair_nstride, table, dtype, N, H, W, C, flags, out, ws,
                                    stream=None):
        self._note("mgc_color_loss_balanced_fwd", flags)
        m, S = self._balance_operands("mgc_color_loss_balanced_fwd", hair, hair_nstride, table, N, H, W, flags)
        x, r, mb = self._color_inputs(img, real, real_nstride, back, back_nstride, dtype, N, H, W, C, flags)
        _view(out, (3,), torch.float32)[:] = color_terms(x, r, mb, m, S, flags)[0].float()
        return 0

    def mgc_color_loss_balanced_bwd(self, img, real, real_nstride, back, back_nstride, hair, hair_nstride, table, g_lab, g_rgb, g_back,
                                    dtype, N, H, W, C, flags, dimg, stream=None):
        self._note("mgc_color_loss_balanced_bwd", flags)
        m, S = self._balance_operands("mgc_color_loss_balanced_bwd", hair, hair_nstride, table, N, H, W, flags)
        x, r, mb = self._color_inputs(img, real, real_nstride, back, back_nstride, dtype, N, H, W, C, flags)
        g = [float(_view(p, (1,), torch.float32)[0]) if _addr(p) else 0.0 for p in (g_lab, g_rgb, g_back)]
        grad = color_terms(x, r, mb, m, S, flags, g)[1]
        d = _view(dimg, (N, H, W, C), _TD[dtype])
        d.zero_()
        d[..., :3] = grad.permute(0, 2, 3, 1).to(_TD[dtype])
        return 0

    def mgc_hair_lab_balanced_fwd(self, img, ref, ref_nstride, hair_tag, hair_tag_nstride, hair_ref, hair_ref_nstride, tgt, tgt_nstride, back,
                                  back_nstride, table, dtype, N, H, W, C, flags, out, stats, ws, stream=None):
        fn = "mgc_hair_lab_balanced_fwd"
        self._note(fn, flags)
        if not flags & 1:
            self._fail(fn, "flags must contain bit 1")
        if not _addr(table) or not _addr(stats):
            self._fail(fn, "null pointer")
        S = _view(table, (BINS, BINS), torch.float32)
        x, r, mf, mr, t, mb = self._hair_inputs(img, ref, ref_nstride, hair_tag, hair_tag_nstride, hair_ref, hair_ref_nstride, tgt, tgt_nstride,
                                                back, back_nstride, dtype, N, H, W, C, flags)
        losses, _, (da, db), w = hair_terms(x, r, mf, mr, S, t, mb, flags)
        _view(out, (2,), torch.float32)[:] = losses.float()
        sf, sr = mf.sum(dim=(1, 2)), mr.sum(dim=(1, 2))
        inv = lambda s: 1.0 / torch.where(s == 0, torch.ones_like(s), s)
        z = torch.zeros_like(da)
        _view(stats, (N, HAIR_STATS), torch.float32)[:] = torch.stack([da, db, inv(sf), inv(sr), w, z, z, z], dim=1).float()
        return 0

    def mgc_hair_lab_balanced_bwd(self, img, hair_tag, hair_tag_nstride, tgt, tgt_nstride, back, back_nstride, stats, g_hair, g_back,
                                  dtype, N, H, W, C, flags, dimg, stream=None):
        """Uses what the kernel uses: the per-sample signs, 1 / S_f and w_n of `stats`, no second reduction."""
        fn = "mgc_hair_lab_balanced_bwd"
        self._note(fn, flags)
        if not flags & 1:
            self._fail(fn, "flags must contain bit 1")
        if not _addr(stats):
            self._fail(fn, "null pointer (stats)")
        x, _, mf, _, t, mb = self._hair_inputs(img, None, 0, hair_tag, hair_tag_nstride, None, 0, tgt, tgt_nstride, back, back_nstride,
                                               dtype, N, H, W, C, flags)
        g = [float(_view(p, (1,), torch.float32)[0]) if _addr(p) else 0.0 for p in (g_hair, g_back)]
        st = _view(stats, (N, HAIR_STATS), torch.float32).double()
        sa, sb = 500 * torch.sign(st[:, 0])[:, None, None], 200 * torch.sign(st[:, 1])[:, None, None]
        dfx = K._df(K._xyz(x))
        dxyz = torch.stack([sa * dfx[:, 0], (sb - sa) * dfx[:, 1], -sb * dfx[:, 2]], dim=1)
        grad = g[0] / (2 * N) * 0.5 * (mf * (st[:, 2] * st[:, 4])[:, None, None]).unsqueeze(1) * torch.einsum("rc,nrhw->nchw", K.MN, dxyz)
        if flags & K.HAIR_BACKGROUND:
            grad = grad + K.hair_terms(x, None, None, None, t, mb, K.HAIR_BACKGROUND, (0.0, g[1]))[1]
        d = _view(dimg, (N, H, W, C), _TD[dtype])
        d.zero_()
        d[..., :3] = grad.permute(0, 2, 3, 1).to(_TD[dtype])
        return 0


# ---- seeded operands for other geometries ------------------------------------------------------------------------------------------------
EDGE_MARGIN = 1e-3                               # tools/make_lab_balance_golden.py: 20 x the float32 route's largest error in a and b (5e-5)


def operands(n, h, w, seed, sd=0.08):
    """dict(fake, real [n,3,h,w]; hair, back [n,h,w]) like the golden pairs: a grey base plus chroma noise (the bins below the cap lie around
    grey), every target pixel at least EDGE_MARGIN from an integer value of a + 128 and b + 128 in float64 -- the weight jumps there, and
    a kernel that lands a pixel in the neighbouring bin for a rounding error would differ by the table's step, not by a rounding error."""
    g = torch.Generator().manual_seed(seed)

    def draw():
        grey = torch.rand(n, 1, h, w, generator=g) * 1.4 - 0.7
        return (grey + sd * torch.randn(n, 3, h, w, generator=g)).clamp(-1, 1)
    real = draw()
    for _ in range(100):
        a, b = K._ab(K._xyz(real.double()))
        near = ((a + 128 - (a + 128).round()).abs() < EDGE_MARGIN) | ((b + 128 - (b + 128).round()).abs() < EDGE_MARGIN)
        if not bool(near.any()):
            break
        real = torch.where(near.unsqueeze(1), draw(), real)
    assert not bool(near.any())
    fake = (real + 0.15 * torch.randn(n, 3, h, w, generator=g)).clamp(-1, 1)
    hair = (torch.rand(n, h, w, generator=g) > 0.4).float()
    return dict(fake=fake, real=real, hair=hair, back=1 - hair)


# ---- the fixtures --------------------------------------------------------------------------------------------------------------------------
def ab_count():
    """The reference's histogram of hair colours over the a/b plane (data/ab_count.npy), float64 [256, 256] counts"""
    return np.load(os.path.join(GOLDEN, "ab_count.npz"))["ab_count"]


def ab_count_path():
    return os.path.join(GOLDEN, "ab_count.npz")


def load_pair(tag):
    """tests/golden/lab_balance_<tag>.npz (tag i, ii or hair) as tensors (scalars as Python numbers)."""
    return PU.load_tensors("lab_balance_%s.npz" % tag)


def balance_argv(cfg, checkpoints_dir, weight_file):
    """The README training flags AS PUBLISHED (Lab on) plus --balance_Lab --weight_dir <file>"""
    from oracle import trainer_parity as TP
    return [a for a in TP.reference_argv(cfg, checkpoints_dir) if a != "--no_lab_loss"] + ["--balance_Lab", "--weight_dir", weight_file]


class _LabRecorder:
    """A trainer proxy that notes the Lab loss after every generator step (oracle.trainer_parity.drive keeps its own list of keys)."""

    def __init__(self, trainer):
        self.__dict__["_tr"], self.__dict__["seen"] = trainer, []

    def __getattr__(self, name):
        return getattr(self._tr, name)

    def run_generator_one_step(self, data):
        self._tr.run_generator_one_step(data)
        self.seen.append(float(self._tr.g_losses["lab"].detach().float().mean()))


def drive_with_lab(trainer, cfg, device="cpu"):
    """oracle.trainer_parity.drive's record + it<i>.loss.lab: what tests/golden/trainer_L.npz holds."""
    from oracle import trainer_parity as TP
    rec_tr = _LabRecorder(trainer)
    rec = TP.drive(rec_tr, cfg, device=device)
    for it, v in enumerate(rec_tr.seen):
        rec["it%d.loss.lab" % it] = np.array(v)
    return rec
