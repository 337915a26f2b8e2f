"""Helpers of tests/test_orient_dog.py (CPU) and tests/test_gpu_orient_dog.py (-m gpu): the float64 contract of the loss extension
group (include/michigan_hip/losses/orient_dog.h) -- the tail of the orientation loss behind the arg-max under the difference-of-
Gaussians bank -- its one-line mutants, the seeded operand builders, the case table, the comparison rules with their derivation, and
`OrientDogEmulator`: oracle/cabi_emulator.py's EmulatorBackend plus mgl_* from the contract (the group is outside the versioned table,
so the emulator under oracle/ does not carry it).

THE CONTRACT (R >= 0 the clamped maximum response, idx its arg-max, m the hair plane, (l0, l1) the label planes, a = idx pi / 32):
    c1 = R m,  M = max c1 over the whole batch,  q = c1 / M,  c = q where not (q <= 0), else q * 0        (NaN stays NaN)
    orient = mean over N 2 H W of |sin 2a c m - l0 m|, |cos 2a c m - l1 m|;   confidence = sum |c m - m| / (sum m + 1e-5)
`forward` is those lines as differentiable torch ops; `gradient` is the closed form of the header, evaluated in the header's order:
    g_o = g_orient / (2 N HW),  g_c = g_conf / (sum m + 1e-5),  A = sum (sg0 sin 2a + sg1 cos 2a) m c1,  B = sum sign(c m - m) m c1
    dL/dc = g_o (sg0 sin 2a + sg1 cos 2a) m + g_c sign(c m - m) m
    dR    = (c > 0 ? dL/dc m / M : 0) + (c1 == M ? -((g_o A + g_c B) / M^2) / count m : 0)
tests/test_orient_dog.py holds the closed form to autograd of `forward`.

THE COMPARISON RULES (kernel in fp32 against the contract in float64 on the same fp32 operands; u = 2^-24):
  scalars   |got - want| <= 1e-4 max(1, |want|) (2e-2 behind a bf16 image): the rule of the Gabor end-to-end test.  The summation scheme
            is the Gabor tail's, and the batch-max division adds nothing: M is a maximum of products R m that are exact for m in {0, 1}
            (no rounding at all), and q = c1 / M is one correctly rounded division, relative error u = 6e-8 per pixel.
  dconf     per element.  Everything behind the fp32 per-pixel terms is evaluated in double and rounded once, so what differs is
            (i) sin 2a, cos 2a: the kernel takes a = fl(idx fl(pi) / 32) and sinf / cosf; pi's rounding (8.7e-8 relative) and the
                product's (6e-8) move 2a <= 6.1 by <= 9e-7, the functions add a few u: absolute error E_F = 2e-6 per factor;
           (ii) q, one rounding, which only matters through the signs (the builders keep every |d0|, |d1| of a hair pixel above
                MARGIN = 2e-5 > 4 E_F unless the factor beside the sign is itself below E_F, which costs 2 E_F
                more; and c < 1 strictly off the maximum, see below), and the last rounding to fp32 (u |want|);
          (iii) at the pixels that attain M, the two sums A and B: fp32 per-thread sums of at most n_seq terms, six levels of the wave
                tree and three joins, each term itself three roundings: |dA| <= (n_seq + 12) u sum|a_j| + 2 E_F sum(m c1), with
                |a_j| <= sqrt(2) m c1; B likewise without the E_F part (its factors are signs).  sum m is exact (an integer < 2^24).
            bound_i = 4 u |want_i| + 4 E_F |g_o| m_i / M [c_i > 0]
                      + [c1_i == M] ((|g_o| (1.42 (n_seq + 12) u + 4 E_F) + |g_c| (n_seq + 12) u) sum(m c1) / M^2 / count)
  c == 1 only at the maximum: c1 < M for two fp32 numbers means c1 <= M (1 - 2u), and the correctly rounded quotient of that is at most
  1 - u, which fp32 holds.  So sign(c m - m) is -1 at every other hair pixel in fp32 as in float64."""
import ctypes
import math

import numpy as np
import torch

from oracle.cabi_emulator import EmulatorBackend, _addr, _view

BLOCKS, WS_ROWS, OUT = 1024, 7, 8               # MGL_ORIENT_DOG_BLOCKS, _WS_ROWS, _OUT
U = 2.0 ** -24
E_F = 2e-6
MARGIN = 2e-5
SCALAR_TOL = {"f32": 1e-4, "bf16": 2e-2}
MUTANTS = ("per_sample_max", "no_max_path", "no_eps", "mean_nhw", "sign_at_one")


def _label_planes(label):
    """label float64 [N, 1 or 2, H, W] -> (l0, l1) [N, H, W]"""
    if label.shape[1] == 2:
        return label[:, 0], label[:, 1]
    t = label[:, 0] / 255 * math.pi
    return torch.sin(2 * t), torch.cos(2 * t)


def _trig(idx):
    a = idx.double() * (math.pi / 32)
    return torch.sin(2 * a), torch.cos(2 * a)


def forward(R, idx, label, m, mutant=None):
    """(orient, confidence) as differentiable float64 torch ops on R [N,H,W]; idx integer [N,H,W]; label [N,1|2,H,W]; m [N,H,W]"""
    R, label, m = R.double(), label.double(), m.double()
    l0, l1 = _label_planes(label)
    f0, f1 = _trig(idx)
    c1 = R * m
    M = c1.amax(dim=(1, 2), keepdim=True) if mutant == "per_sample_max" else torch.max(c1)
    q = c1 / M
    c = q * (~(q <= 0)).double()
    n, h, w = R.shape
    count = n * h * w if mutant == "mean_nhw" else 2 * n * h * w
    orient = ((f0 * c * m - l0 * m).abs().sum() + (f1 * c * m - l1 * m).abs().sum()) / count
    confidence = (c * m - m).abs().sum() / (m.sum() + (0.0 if mutant == "no_eps" else 1e-5))
    return orient, confidence


def terms(R, idx, label, m):
    """every intermediate of the contract as float64 tensors / python floats"""
    R, label, m = R.detach().double(), label.double(), m.double()
    l0, l1 = _label_planes(label)
    f0, f1 = _trig(idx)
    c1 = R * m
    M = torch.max(c1)
    q = c1 / M
    c = q * (~(q <= 0)).double()
    d0, d1, e = f0 * c * m - l0 * m, f1 * c * m - l1 * m, c * m - m
    a = (torch.sign(d0) * f0 + torch.sign(d1) * f1)
    return dict(c1=c1, M=float(M), c=c, m=m, f0=f0, f1=f1, d0=d0, d1=d1, e=e, a=a, summ=float(m.sum()),
                count=float((c1 == M).sum()), A=float((a * m * c1).sum()), B=float((torch.sign(e) * m * c1).sum()))


def contract(R, idx, label, m):
    """the eight floats of `out` in float64 (out[7] = 0)"""
    t = terms(R, idx, label, m)
    n, h, w = R.shape
    orient = float((t["d0"].abs().sum() + t["d1"].abs().sum()) / (2 * n * h * w))
    confidence = float(t["e"].abs().sum() / (t["summ"] + 1e-5))
    return [orient, confidence, t["summ"], t["M"], t["count"], t["A"], t["B"], 0.0]


def gradient(R, idx, label, m, g_orient, g_conf, mutant=None, fwd_out=None):
    """d(g_orient orient + g_conf confidence) / dR, float64 [N,H,W], in the header's order of operations.  g_* python floats or None.
    `fwd_out`: take sum m, M, count, A, B from a forward's out (what the entry point does) instead of from the operands"""
    t = terms(R, idx, label, m)
    n, h, w = R.shape
    summ, M, count, A, B = [float(v) for v in fwd_out[2:7]] if fwd_out is not None else (t["summ"], t["M"], t["count"], t["A"], t["B"])
    g_o = torch.tensor(0.0 if g_orient is None else float(g_orient), dtype=torch.float64) / (2.0 * (n * h * w))
    g_c = torch.tensor(0.0 if g_conf is None else float(g_conf), dtype=torch.float64) / torch.tensor(summ + (0.0 if mutant == "no_eps" else 1e-5), dtype=torch.float64)
    md, Md = t["m"], torch.tensor(M, dtype=torch.float64)
    sgn = torch.sign(t["e"])
    if mutant == "sign_at_one":
        sgn = torch.where((t["e"] == 0) & (md > 0), -torch.ones_like(sgn), sgn)
    dc = g_o * t["a"] * md + g_c * sgn * md
    d = torch.where(t["c"] > 0, dc * md / Md, torch.zeros_like(dc))
    if mutant != "no_max_path":
        tie = -((g_o * A + g_c * B) / (Md * Md)) / count
        d = d + torch.where(t["c1"] == Md, tie * md, torch.zeros_like(md))
    return d


# ---- comparison rules --------------------------------------------------------------------------------------------------------------------
def scalar_close(got, want, tol):
    got, want = (float(v.detach()) if torch.is_tensor(v) else float(v) for v in (got, want))
    return abs(got - want) <= tol * max(1.0, abs(want))


def n_seq(total):
    """terms one thread adds in the partial pass: the grid is min(ceil(total / 256), 1024) workgroups of 256"""
    grid = min(-(-total // 256), BLOCKS)
    return -(-total // (grid * 256))


def dconf_bound(R, idx, label, m, g_orient, g_conf):
    """float64 [N,H,W]: the per-element bound of the module docstring"""
    t = terms(R, idx, label, m)
    want = gradient(R, idx, label, m, g_orient, g_conf)
    total = R.numel()
    g_o = abs(0.0 if g_orient is None else float(g_orient)) / (2.0 * total)
    g_c = abs(0.0 if g_conf is None else float(g_conf)) / (t["summ"] + 1e-5)
    k = (n_seq(total) + 12) * U
    at_max = (g_o * (1.42 * k + 4 * E_F) + g_c * k) * float((t["m"] * t["c1"]).sum()) / t["M"] ** 2 / t["count"]
    return 4 * U * want.abs() + 4 * E_F * g_o * t["m"] / t["M"] * (t["c"] > 0).double() + at_max * (t["c1"] == t["M"]).double()


def margin_violations(R, idx, label, m):
    """bool [N,H,W]: hair pixels with a positive confidence at which a difference within MARGIN of a sign change belongs to a factor above
    E_F.  (Where the factor is at most E_F -- sin 0, sin pi, ... against a label at the same place -- the sign moves dL/dc by at most
    2 E_F, the second 2 E_F of the bound; where c == 0 no sign reaches dconf, A or B.)"""
    t = terms(R, idx, label, m)
    live = (t["m"] > 0) & (t["c"] > 0)
    ok = ((t["d0"].abs() >= MARGIN) | (t["f0"].abs() <= E_F)) & ((t["d1"].abs() >= MARGIN) | (t["f1"].abs() <= E_F))
    return live & ~ok


def margins_ok(R, idx, label, m):
    return not bool(margin_violations(R, idx, label, m).any())


# ---- operand builders ----------------------------------------------------------------------------------------------------------------------
def flat_index(n, h, w, where):
    return {"first": 0, "last": n * h * w - 1, "tail": n * h * w - 1 - ((n * h * w - 1) % 256) // 2 if (n * h * w) % 256 else n * h * w - 3,
            "sample1": h * w + (h * w) // 2}[where]


def one_hot(m):
    """[N, 2, H, W] one-hot label whose plane 1 is m: the hair plane is then a strided view"""
    return torch.stack([1 - m, m], dim=1).contiguous()


def operands(n, h, w, label_ch, seed, max_at="first", ties=1, hair="strided", sparse=False):
    """fp32 operands with the maximum M = 6.5 of R m at flat index `max_at` (and at ties - 1 more pixels), every other response below 6.
    max_at 'sample1': sample 0 has no hair at all.  sparse: the hair is the maximum and one more pixel, so that sum m = 2 and the 1e-5
    beside it is 5e-6 of the denominator.  Keeps the margin condition."""
    g = torch.Generator().manual_seed(seed)
    R = torch.rand(n, h, w, generator=g) * 6
    R[torch.rand(n, h, w, generator=g) < 0.1] = 0                     # the clamp's zeros
    idx = torch.randint(0, 32, (n, h, w), generator=g, dtype=torch.uint8)
    m = (torch.rand(n, h, w, generator=g) < 0.6).float()
    if max_at == "sample1":
        m[0] = 0
    if label_ch == 2:
        t = torch.rand(n, h, w, generator=g) * math.pi
        r = 0.5 + 0.5 * torch.rand(n, h, w, generator=g)
        label = torch.stack([torch.sin(2 * t) * r, torch.cos(2 * t) * r], dim=1)
    else:
        label = torch.randint(0, 256, (n, 1, h, w), generator=g).float()
    at = flat_index(n, h, w, max_at)
    spots = [at] + [(at + 37 * (j + 1)) % (n * h * w) for j in range(ties - 1)]
    if max_at == "sample1":
        spots = [at] + [h * w + (at - h * w + 37 * (j + 1)) % (h * w) for j in range(ties - 1)]
    if sparse:
        m.zero_()
        other = (at + 11) % (n * h * w)
        R.view(-1)[other], m.view(-1)[other] = 3.25, 1.0
    for s in spots:
        R.view(-1)[s], m.view(-1)[s] = 6.5, 1.0
    # among 3e5 random pixels a few differences always fall within MARGIN of 0: those pixels get no response (the clamp's zero)
    R[margin_violations(R, idx, label, m)] = 0
    assert margins_ok(R, idx, label, m) and all(float(R.view(-1)[s]) == 6.5 for s in spots), "a difference at the maximum sits within MARGIN of a sign change: choose another seed"
    sem = one_hot(m)
    return dict(R=R, idx=idx, label=label.contiguous(), m=sem[:, 1] if hair == "strided" else m.contiguous(), sem=sem, spots=spots)


def exact_operands(n, h, w, seed, max_at="first", ties=1, empty=False):
    """idx == 0 (sin 0 = 0, cos 0 = 1 exactly), R in {0, 1/8 .. 63/8} with M = 8 at `max_at`, 2-plane labels in multiples of 1/16, m in
    {0, 1}: every product and every fp32 partial sum is exact.  empty: no hair pixel has a positive response (M == 0)"""
    g = torch.Generator().manual_seed(seed)
    R = torch.randint(0, 64, (n, h, w), generator=g).float() / 8
    idx = torch.zeros((n, h, w), dtype=torch.uint8)
    m = (torch.rand(n, h, w, generator=g) < 0.6).float()
    label = torch.randint(-16, 17, (n, 2, h, w), generator=g).float() / 16
    if max_at == "sample1":
        m[0] = 0
    at = flat_index(n, h, w, max_at)
    spots = [at] + [(at + 37 * (j + 1)) % (n * h * w) for j in range(ties - 1)]
    if max_at == "sample1":
        spots = [at] + [h * w + (at - h * w + 37 * (j + 1)) % (h * w) for j in range(ties - 1)]
    for s in spots:
        R.view(-1)[s], m.view(-1)[s] = 8.0, 1.0
    if empty:
        R = R * (1 - m)
        spots = []
    sem = one_hot(m)
    return dict(R=R, idx=idx, label=label.contiguous(), m=sem[:, 1], sem=sem, spots=spots)


SHAPES = ((2, 5, 7), (2, 16, 16), (2, 1, 257), (2, 384, 384))          # below one block, exactly one... (N = 2: 2 blocks), 257, the stride trips twice
SMALL_SHAPES = SHAPES[:3]
WHERE = ("first", "last", "tail", "sample1")


def small_cases():
    """{id: operands}: the CPU case table -- the small shapes, the four positions of the maximum, both label layouts, one two-way tie"""
    out = {}
    for si, (n, h, w) in enumerate(SMALL_SHAPES):
        for wi, where in enumerate(WHERE):
            ch = 1 + (si + wi) % 2
            out["%dx%dx%d-%s-%dch" % (n, h, w, where, ch)] = operands(n, h, w, ch, 100 + 10 * si + wi, where)
    out["2x16x16-tie-2ch"] = operands(2, 16, 16, 2, 150, "first", ties=2)
    out["2x5x7-sparse-2ch"] = operands(2, 5, 7, 2, 151, "last", sparse=True)
    return out


def rejects(mutant, ops, g_orient=0.7, g_conf=1.3):
    """does this case tell the mutant from the contract, by the comparison rules above?"""
    R, idx, label, m = ops["R"], ops["idx"], ops["label"], ops["m"]
    if mutant in ("per_sample_max", "no_eps", "mean_nhw"):
        want = contract(R, idx, label, m)[:2]
        got = [float(v) for v in forward(R, idx, label, m, mutant)]
        if not all(scalar_close(a, b, SCALAR_TOL["f32"]) for a, b in zip(got, want)):
            return True
        if mutant == "per_sample_max":
            return False
    want = gradient(R, idx, label, m, g_orient, g_conf)
    got = gradient(R, idx, label, m, g_orient, g_conf, mutant)
    return bool(((got - want).abs() > dconf_bound(R, idx, label, m, g_orient, g_conf)).any())


# ---- the emulator ----------------------------------------------------------------------------------------------------------------------------
class OrientDogEmulator(EmulatorBackend):
    """EmulatorBackend + the loss extension group from the contract above, results rounded to fp32 once.  Argument checks as the header
    states them; a refused call is in the log too, as the base class keeps it."""

    def _dog_operands(self, fn, conf_raw, idx, label, label_ch, label_nstride, hair, hair_nstride, N, HW, extra):
        self._note(fn)
        if not all(_addr(p) for p in (conf_raw, idx, label, hair) + tuple(extra)):
            self._fail(fn, "null pointer")
        if label_ch not in (1, 2) or N < 1 or not 1 <= HW < 1 << 31 or (N > 1 and (label_nstride < label_ch * HW or hair_nstride < HW)):
            self._fail(fn, "bad geometry")
        R = _view(conf_raw, (N, 1, HW), torch.float32)
        ix = _view(idx, (N, 1, HW), torch.uint8)
        m = self._plane(hair, N, hair_nstride, 1, HW)
        base = _view(label, ((N - 1) * label_nstride + label_ch * HW,), torch.float32)
        lab = torch.as_strided(base, (N, label_ch, 1, HW), (label_nstride, HW, HW, 1))
        return R, ix, lab, m

    def mgl_orient_dog_fwd(self, conf_raw, idx, label, label_ch, label_nstride, hair, hair_nstride, N, HW, out, ws, stream=None):
        R, ix, lab, m = self._dog_operands("mgl_orient_dog_fwd", conf_raw, idx, label, label_ch, label_nstride, hair, hair_nstride, N, HW, (out, ws))
        _view(out, (OUT,), torch.float32)[:] = torch.tensor(contract(R, ix, lab, m), dtype=torch.float64).float()
        return 0

    def mgl_orient_dog_bwd(self, conf_raw, idx, label, label_ch, label_nstride, hair, hair_nstride, g_orient, g_conf, fwd_out, N, HW, dconf,
                           stream=None):
        R, ix, lab, m = self._dog_operands("mgl_orient_dog_bwd", conf_raw, idx, label, label_ch, label_nstride, hair, hair_nstride, N, HW,
                                           (fwd_out, dconf))
        g0 = float(_view(g_orient, (1,), torch.float32)[0]) if _addr(g_orient) else None
        g1 = float(_view(g_conf, (1,), torch.float32)[0]) if _addr(g_conf) else None
        fo = _view(fwd_out, (OUT,), torch.float32).double().tolist()
        _view(dconf, (N, 1, HW), torch.float32)[:] = gradient(R, ix, lab, m, g0, g1, fwd_out=fo).float()
        return 0


def header_defines():
    """{name: int} of the integer MGL_ #defines of include/michigan_hip/losses/orient_dog.h"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "michigan_hip", "losses", "orient_dog.h")) as fh:
        return {k: int(v) for k, v in re.findall(r"#define\s+(MGL_[A-Z0-9_]+)\s+(\d+)\b", fh.read())}


def pointer(t):
    return ctypes.c_void_p(t.data_ptr())


# ---- the whole loss in float64 ---------------------------------------------------------------------------------------------------------------
def responses(img, bank):
    """img [N,3,H,W] in [-1, 1], bank fp32 [32,17,17] -> the 32 clamped responses [N,32,H,W] in the dtype of img (loss.py:356-358, 323-335)"""
    import torch.nn.functional as F
    x = (img + 1) / 2.0 * 255
    gray = 0.299 * x[:, 0] + 0.587 * x[:, 1] + 0.144 * x[:, 2]
    return F.conv2d(gray[:, None], bank.to(img.dtype)[:, None], padding=8).clamp_min(0)


def l1o_contract(img, label, sem, bank):
    """(orient, confidence) of the whole L1OLoss in DoG mode, float64, differentiable w.r.t. img"""
    r = responses(img.double(), bank)
    R, idx = r.max(1)
    return forward(R, idx, label, sem[:, 1])


# ---- the reference fixture -----------------------------------------------------------------------------------------------------------------
def golden():
    """tests/golden/orient_dog.npz (tools/make_orient_dog_golden.py): the reference's own L1OLoss in DoG mode at crop 64"""
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "orient_dog.npz"))
