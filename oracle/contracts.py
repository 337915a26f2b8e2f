"""TEST INFRASTRUCTURE ONLY -- the float64 contracts of the loss, preprocessing and editing entry points of libmichigan_hip on plain
tensors and arrays, one function per formula of the headers under include/.  The C-ABI contract emulator (oracle/cabi_emulator.py)
calls them on views of the raw buffers; the tests call them on inputs of their own (a bf16-rounded image, a fixture of the
reference) and flip their mutant switches to show that a fixture notices a broken contract.  The product never imports this module.

  colour      mg_color_loss_fwd / _bwd (include/michigan_hip.h)                  color_terms, _f, _df, _xyz, _ab, M, MN
  hair-Lab    mg_hair_lab_fwd / _bwd (include/michigan_hip.h)                    hair_terms
  style       mg_feat_moment_loss_fwd / _bwd (michigan_hip/feature_losses.h)     moments, coefficients, content_den, gradient, style_terms
  dense orientation   mg_gabor_argmax_fwd, mg_orient_smooth (michigan_hip/preprocess/dense_orient.h)   argmax_contract, smooth_contract
  stroke      mg_stroke_orient, mg_stroke_compose, mg_inpaint_finish (michigan_hip/editing/stroke_orient.h)
              responses, stroke_contract, compose_contract, finish_contract
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

# ---- colour (mg_color_loss.hip) ----------------------------------------------------------------------------------------------------------
COLOR_LAB, COLOR_RGB, COLOR_BACKGROUND = 1, 2, 4
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
    if flags & COLOR_LAB:
        out[0] = (da.abs().sum() + db.abs().sum()) / (n * 2 * h * w)
        sa, sb = 500 * torch.sign(da), 200 * torch.sign(db)
        dfx = _df(xyz_f)
        dxyz = torch.stack([sa * dfx[:, 0], (sb - sa) * dfx[:, 1], -sb * dfx[:, 2]], dim=1)
        grad += weights[0] / (n * 2 * h * w) * 0.5 * torch.einsum("rc,nrhw->nchw", MN, dxyz)
    if flags & COLOR_RGB:
        out[1] = drgb.abs().sum() / (n * 3 * h * w)
        grad += weights[1] / (n * 3 * h * w) * torch.sign(drgb)
    if flags & COLOR_BACKGROUND:
        m = back.double().unsqueeze(1)
        dm = fake * m - real * m
        out[2] = dm.abs().sum() / (n * 3 * h * w)
        grad += weights[2] / (n * 3 * h * w) * torch.sign(dm) * m
    return out, grad, (da, db, drgb)


# ---- hair-Lab (mg_hair_lab.hip) ----------------------------------------------------------------------------------------------------------
HAIR_LAB, HAIR_BACKGROUND = 1, 2


def hair_terms(fake, ref, m_f, m_r, tgt=None, m_b=None, flags=3, weights=(1.0, 1.0)):
    """float64 contract on plain tensors: fake / ref / tgt [N, 3, H, W], m_f / m_r / m_b [N, H, W]; operands of a term that is
    not selected may be None.  Returns (losses[2], d(sum_k weights[k] * losses[k]) / d fake [N, 3, H, W], (da[N], db[N]))."""
    fake = fake.double()
    n, _, h, w = fake.shape
    out = torch.zeros(2, dtype=torch.float64)
    grad = torch.zeros_like(fake)
    da = db = None
    if flags & HAIR_LAB:
        mf, mr = m_f.double(), m_r.double()
        xyz_f = _xyz(fake)
        af, bf = _ab(xyz_f)
        ar, br = _ab(_xyz(ref.double()))
        sf, sr = mf.sum(dim=(1, 2)), mr.sum(dim=(1, 2))
        sf, sr = torch.where(sf == 0, torch.ones_like(sf), sf), torch.where(sr == 0, torch.ones_like(sr), sr)
        da = (mf * af).sum(dim=(1, 2)) / sf - (mr * ar).sum(dim=(1, 2)) / sr
        db = (mf * bf).sum(dim=(1, 2)) / sf - (mr * br).sum(dim=(1, 2)) / sr
        out[0] = (da.abs().sum() + db.abs().sum()) / (2 * n)
        sa, sb = 500 * torch.sign(da)[:, None, None], 200 * torch.sign(db)[:, None, None]
        dfx = _df(xyz_f)
        dxyz = torch.stack([sa * dfx[:, 0], (sb - sa) * dfx[:, 1], -sb * dfx[:, 2]], dim=1)
        scale = (mf / sf[:, None, None]).unsqueeze(1)
        grad += weights[0] / (2 * n) * 0.5 * scale * torch.einsum("rc,nrhw->nchw", MN, dxyz)
    if flags & HAIR_BACKGROUND:
        m = m_b.double().unsqueeze(1)
        dm = fake * m - tgt.double() * m
        out[1] = dm.abs().sum() / (n * 3 * h * w)
        grad += weights[1] / (n * 3 * h * w) * torch.sign(dm) * m
    return out, grad, (da, db)


# ---- style and content (mg_feat_moments.hip) -----------------------------------------------------------------------------------------------
FEAT_STYLE, FEAT_CONTENT = 1, 2
FEAT_EPS = 1e-5


def _kept(f, m):
    """f where the mask is non-zero, 0 elsewhere: what is masked out is not read (a NaN there reaches nothing)"""
    return torch.where((m != 0).unsqueeze(1), f, torch.zeros_like(f))


def moments(f, m=None):
    """(mu, sigma, S, T) per (n, c) of f [N, C, P] (float64) under m [N, P] or unmasked (calc_mean_std / calc_mean_std_mask)."""
    if m is None:
        p = f.shape[2]
        mu = f.mean(dim=2)
        return mu, (((f - mu.unsqueeze(2)) ** 2).sum(dim=2) / (p - 1) + FEAT_EPS).sqrt(), None, None
    f = _kept(f, m)
    mm = m.unsqueeze(1)
    s = (m.sum(dim=1) + FEAT_EPS).unsqueeze(1)                                     # [N, 1]
    mu = (f * mm).sum(dim=2) / s
    r = (f * mm - mu.unsqueeze(2)) * mm
    return mu, ((r ** 2).sum(dim=2) / s + FEAT_EPS).sqrt(), s, (r * mm).sum(dim=2)


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
    return float(n * p * c) if mask_t is None else float(c * mask_t.sum() + FEAT_EPS)


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
    if flags & FEAT_STYLE:
        out[0], a, b, mu_x = coefficients(x3, s3, mx, ms)
    if flags & FEAT_CONTENT:
        den = content_den(n, c, h * w, ml)
        diff = x3 - t3 if ml is None else ml.unsqueeze(1) * (_kept(x3, ml) - _kept(t3, ml))
        out[1] = (diff ** 2).sum() / den
    grad = gradient(x3, t3, mx, ml, a, b, mu_x, den, weights[0] if flags & FEAT_STYLE else 0.0, weights[1] if flags & FEAT_CONTENT else 0.0)
    return out, grad.reshape(n, c, h, w)


# ---- dense orientation (mg_gabor.hip, mg_orient_smooth.hip) ----------------------------------------------------------------------------------
ORIENT_RADIUS = 16


def smooth_contract(conf, idx, mask, trig, taps, reflect101=True, mask_multiply=True, truncate=True):
    """conf / idx / mask [N,H,W] arrays, trig [32,2], taps [2r+1] -> dict(theta, level (float64 [N,H,W]), u8, bx, by).  The three
    switches are the contract as written; a mutant turns one off."""
    conf, trig, taps = np.asarray(conf, np.float64), np.asarray(trig, np.float64), np.asarray(taps, np.float64)
    idx, m = np.asarray(idx).astype(np.int64), np.asarray(mask) != 0
    r = (len(taps) - 1) // 2
    n, h, w = conf.shape
    assert h > r and w > r
    c = np.where(m, conf, 0.0)                                            # conf is not read as a number where the mask is 0
    out = []
    for f in (trig[idx, 0] * c, trig[idx, 1] * c):
        p = np.pad(f, ((0, 0), (r, r), (r, r)), mode="reflect" if reflect101 else "symmetric")
        rows = sum(taps[k] * p[:, :, k:k + w] for k in range(2 * r + 1))
        out.append(sum(taps[k] * rows[:, k:k + h, :] for k in range(2 * r + 1)))
    bx, by = out
    theta = 0.5 * np.arctan2(by, bx)
    theta = np.where(theta < 0, theta + math.pi, theta)
    level = theta * 255.0 / math.pi * (m if mask_multiply else 1.0)
    level = np.minimum(level, 255.0)
    u8 = (np.trunc(level) if truncate else np.minimum(np.round(level), 255.0)).astype(np.uint8)
    return dict(theta=theta, level=level, u8=u8, bx=bx, by=by)


def argmax_contract(image, bank):
    """float64 contract of mg_gabor_argmax_fwd on plain tensors: image fp32 [N,H,W,3] in [-1, 1], bank [32,17,17] -> (conf, idx) arrays"""
    x = (image[..., :3].double() + 1) / 2 * 255
    g = (0.299 * x[..., 0] + 0.587 * x[..., 1] + 0.144 * x[..., 2])[:, None]
    r = F.conv2d(g, bank.double().view(32, 1, 17, 17), padding=8).clamp_min(0)
    return r.max(1)[0].numpy(), r.argmax(1).numpy()


# ---- stroke editing (mg_stroke.hip) --------------------------------------------------------------------------------------------------------
STROKE_RADIUS = 8
STROKE_MUTANTS = ("convolution", "bank_transposed", "argmax_before_clamp", "last_argmax", "rg_swapped", "outside_not_black", "reflected_border")


def responses(stroke, bank, border="zero"):
    """float64 [N,32,H,W]: resp_k[y,x] = sum_ij bank[k][i][j] s[y+i-8, x+j-8] with s = stroke != 0 (correlation)"""
    s = torch.from_numpy((np.asarray(stroke) != 0).astype(np.float64))[:, None]
    b = torch.as_tensor(np.asarray(bank), dtype=torch.float64).view(32, 1, 17, 17)
    if border == "reflect":
        n, _, h, w = s.shape
        iy = np.pad(np.arange(h), STROKE_RADIUS, mode="symmetric" if h <= STROKE_RADIUS else "reflect")
        ix = np.pad(np.arange(w), STROKE_RADIUS, mode="symmetric" if w <= STROKE_RADIUS else "reflect")
        return F.conv2d(s[:, :, iy][:, :, :, ix], b).numpy()
    return F.conv2d(s, b, padding=STROKE_RADIUS).numpy()


def stroke_contract(stroke, bank, rgb_table, mutant=None):
    """stroke u8 [N,H,W], bank [32,17,17], rgb_table u8 [32,3] -> dict(rgb u8 [N,H,W,3], idx u8, conf float64, resp float64
    [N,32,H,W]).  `mutant` (one of STROKE_MUTANTS) breaks one thing the fixtures must notice."""
    assert mutant is None or mutant in STROKE_MUTANTS
    bank, table = np.asarray(bank), np.asarray(rgb_table)
    if mutant == "convolution":
        bank = bank[:, ::-1, ::-1].copy()
    if mutant == "bank_transposed":
        bank = bank.transpose(0, 2, 1).copy()
    if mutant == "rg_swapped":
        table = table[:, [1, 0, 2]]
    s = np.asarray(stroke) != 0
    resp = responses(stroke, bank, border="reflect" if mutant == "reflected_border" else "zero")
    clamped = np.maximum(resp, 0.0)
    conf = clamped.max(axis=1)
    if mutant == "argmax_before_clamp":
        idx = resp.argmax(axis=1)
    elif mutant == "last_argmax":
        idx = 31 - clamped[:, ::-1].argmax(axis=1)
    else:
        idx = clamped.argmax(axis=1)                                       # numpy: the first maximum
    rgb = table[idx]
    if mutant != "outside_not_black":
        rgb = np.where(s[..., None], rgb, 0)
    return dict(rgb=rgb.astype(np.uint8), idx=np.where(s, idx, 0).astype(np.uint8), conf=np.where(s, conf, 0.0), resp=resp)


# the two glue entry points of the stroke route: fp32, one operation at a time
def _gather(t, ytab, xtab):
    t = t if ytab is None else t[:, :, ytab.long()]
    return t if xtab is None else t[:, :, :, xtab.long()]


def compose_contract(orient_rgb, noise, hole, stroke, stroke_mask, ytab, xtab, dtype):
    """fp32 torch tensors (NCHW) -> NHWC8 `dtype`; every product and sum is one fp32 torch operation, in the reference's order"""
    o, nz, hl = (_gather(t, ytab, xtab) for t in (orient_rgb, noise, hole))
    if stroke is not None:
        st, sm = _gather(stroke, ytab, xtab), _gather(stroke_mask, ytab, xtab)
        rgb = o * (1 - hl) + nz * (hl - sm) + st * sm
    else:
        sm = torch.zeros_like(hl)
        rgb = o * (1 - hl) + nz * hl
    z = torch.zeros_like(hl)
    return torch.cat([rgb, hl, sm, z, z, z], dim=1).permute(0, 2, 3, 1).contiguous().to(dtype)


def finish_contract(net_out, ytab, xtab, hole, orient_rgb, mask):
    out = _gather(net_out, ytab, xtab) * hole + orient_rgb * (1 - hole)
    o2 = (out[:, :-1] - 0.5) * 2
    return out, torch.stack([o2[:, 1], o2[:, 0]], dim=1) * mask
