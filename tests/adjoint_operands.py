"""Operands, float64 references and comparison rules for the NHWC streaming kernels, the loss gradients and Adam.

tests/exact_operands.py pins the convolutions, tests/census_operands.py the reductions; this file does the same for what streams:
csrc/mg_pointwise.hip and csrc/mg_loss.hip.  A reference here is torch's OWN operator on float64 CPU tensors (F.interpolate(nearest),
nn.ReflectionPad2d, F.avg_pool2d(3, 2, 1, count_include_pad=False), F.max_pool2d(2), F.relu, F.leaky_relu, F.l1_loss, the hinge
expression of test_hinge_loss_and_wide_edge_weight_fused, torch.optim.Adam(foreach=False)) with torch autograd for the adjoints --
never the contract emulator and never a kernel's formula written out again.  (The background blend has no torch operator: its
reference is the expression the header names, act(bg (1 - hair) + x (1 - back)), in float64 with autograd.)

The five rules, each stated once (``check_one``):

  1 raw        copies and selections (mg_upsample2x_fwd, mg_reflect_pad_fwd, mg_maxpool2_fwd, mg_assemble_nhwc8, and the routed
               gradient of mg_maxpool2_bwd): operands are arbitrary finite values of the tensor's dtype with +-0 and subnormals among
               them (``raw_values``); the INTEGER VIEWS of result and reference must be equal, so that -0 and +0 differ.
               mg_assemble_nhwc8's planar fp32 input meets one round-to-nearest-even store: it is compared with planar.to(dtype).
  2 bits       short sums of exact operands (mg_upsample2x_bwd 4 terms, mg_reflect_pad_bwd up to 9, mg_grad_sum_act, mg_act_bwd,
               mg_blend_fwd / mg_blend_bwd): integers of magnitude 128 .. 255 (8 bits: exact in bf16), masks from {0, 1/4, 1/2, 1},
               slope 1/4.  Every sum is exact in fp32 in any order: exact_operands.assert_bits, no tolerance.  Preconditions on the
               reference (``check_sum_output``): sum over |terms| below 2^24 quanta; distinct values (exact_operands.check_distinct on
               the flattened output); from 256 elements on at most half zero and, in bf16 where the op adds, at least 5 % of the outputs
               in need of rounding.  Activation outputs hold exact zeros, so the factor at y == 0 is fixed: 0 (ReLU), the slope (Leaky).
  3 max-pool   mg_maxpool2_bwd: small-integer operands, a tie for the maximum in at least 20 % of the windows; rule 1's comparison.
  4 quotient   a count that is no power of two (mg_avgpool3s2_fwd / _bwd, mg_l1_mean_bwd, mg_hinge_bwd).  ONE fp32 quotient: within 1
               fp32 ulp of fp32(exact) (census_operands.assert_ulp1), and rule 2's assert_bits where the count is a power of two.  A sum
               of quotients, and every bf16 store: ``assert_interval`` -- got must lie in [rne(exact - d), rne(exact + d)] of the output
               dtype, d = k 2^-24 sum|terms| with k the number of fp32 roundings of a straightforward evaluation (K below), and the
               smallest term at least 2^10 d (``check_term_floor``), so that a dropped or doubled term cannot fit.
  5 Adam       mg_adam_step, one teacher-forced step from a given nonzero (p, m, v, g); reference torch.optim.Adam on float64 with the
               fp32-rounded hyper-parameters the C ABI receives.  exp_avg at beta1 = 0 and a power-of-two grad_scale: bits.  Everything
               else: the interval rule with the bounds of ``adam_reference``.

Every reference takes ``mut``: None for the true value (preconditions asserted, a dict name -> Want returned), or the name of a MUTANT --
an edit of the reference that states what a subtly wrong kernel would store (a dict name -> tensor in the storage dtype).
tests/test_adjoint_operands.py asserts that the rule rejects every mutant on the committed case lists.
"""
import collections
import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from census_operands import ROUNDING_MIN_NUMEL, assert_ulp1, hinge_operands, nonzero_ints
from exact_operands import DT, SLOPE, _gen, assert_bits, check_distinct, check_exact, ints, nchw, nhwc, rounding_share

U24 = 2.0 ** -24
FLOOR = 2.0 ** 10
TIE_SHARE = 0.20
WRAP = 8192 * 256                                  # mg_ew_grid caps a launch at 8192 x 256 threads: one more and the grid-stride loop wraps

# fp32 roundings of a straightforward evaluation, per kernel (rule 4's k)
K = {"avgpool_fwd": 10,       # 8 additions of the 9 window terms, the reciprocal of the count, the product
     "avgpool_bwd": 11,       # per term a reciprocal and a product (4 x 2), 3 additions
     "l1_bwd": 2,             # 1 / numel, times gscale
     "hinge_bwd": 2}          # g / n, times the weight

# ---------------------------------------------------------------------------------------------------------------------
# shapes: the smallest at which these kernels can go wrong
# ---------------------------------------------------------------------------------------------------------------------
NS = (1, 3)
CS = (4, 8, 12, 136)           # a lone quad, an 8-byte and a 16-byte bf16 row, a row that is no multiple of 16 bytes, many quads per pixel
HWS = ((2, 2), (2, 3), (3, 2), (7, 9), (8, 8), (16, 17))
HWS_THIN = ((1, 1), (1, 5), (5, 1))                # upsample and avg-pool also take an axis of 1
REFLECT = tuple((h, w, p) for h, w in ((2, 2), (4, 7), (9, 5), (8, 8)) for p in sorted({1, 3, min(h, w) - 1}) if 1 <= p < min(h, w))
FLAT_QUADS = (1, 255, 256, 257)
WRAP_QUADS = WRAP + 3                              # one bf16 case per flat kernel
ADAM_BETAS = ((0.0, 0.9), (0.5, 0.999), (0.9, 0.999))     # the exact-copy branch, w >= 0.5 with memory, w < 0.5
ADAM_SCALES = (1.0, 0.125, 1.0 / 3.0)
ADAM_STEPS = (1, 2, 10, 1000)
ADAM_NUMELS = (1, 3, 255, 256, 257, 4099, WRAP + 3)
HINGE_N = (1, 3, 255, 256, 257, 4099, 67 * 67)
ASSEMBLE = ((4, 4, 3), (3, 0, 0), (8, 0, 0), (1, 8, 5), (0, 8, 8))     # (planar channels, image pitch, image channels taken)


def geoms(thin=False, ns=NS, cs=CS):
    return [(n, h, w, c) for n in ns for c in cs for h, w in HWS + (HWS_THIN if thin else ())]


Want = collections.namedtuple("Want", "ref dtype rule delta pow2", defaults=(None, None))


# ---------------------------------------------------------------------------------------------------------------------
# comparison rules
# ---------------------------------------------------------------------------------------------------------------------
def _int_view(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _first(bad, got, want):
    idx = bad.nonzero()[:6].tolist()
    return ", ".join(f"{tuple(i)}: got {got[tuple(i)].item()!r} want {want[tuple(i)].item()!r}" for i in idx)


def assert_raw(name, got, want):
    """Same dtype, same shape, same BITS: -0 is not +0 here."""
    got = got.detach().cpu()
    assert got.dtype == want.dtype, f"{name}: returned as {got.dtype}, expected {want.dtype}"
    assert got.shape == want.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    bad = _int_view(got) != _int_view(want)
    if bool(bad.any()):
        raise AssertionError(f"{name}: {int(bad.sum())} of {got.numel()} elements differ in their bits; first: {_first(bad, got, want)}")


def assert_interval(name, got, exact, delta, dtype):
    """rne(exact - delta) <= got <= rne(exact + delta) in `dtype` (by value)."""
    got = got.detach().cpu()
    assert got.dtype == dtype, f"{name}: returned as {got.dtype}, expected {dtype}"
    exact = exact.reshape(got.shape)
    delta = torch.as_tensor(delta, dtype=torch.float64).reshape(exact.shape)
    lo, hi = (exact - delta).to(dtype).double(), (exact + delta).to(dtype).double()
    g = got.double()
    bad = ~((g >= lo) & (g <= hi))
    if bool(bad.any()):
        idx = bad.nonzero()[:6].tolist()
        first = ", ".join(f"{tuple(i)}: got {g[tuple(i)].item()!r} outside [{lo[tuple(i)].item()!r}, {hi[tuple(i)].item()!r}]" for i in idx)
        raise AssertionError(f"{name}: {int(bad.sum())} of {got.numel()} values leave the interval of the rounding count; first: {first}")


def assert_quotient(name, got, exact, pow2):
    """One fp32 quotient: 1 ulp; bit for bit where the count is a power of two (`pow2`: a mask, or True / False for all)."""
    assert_ulp1(name, got, exact)
    want = exact.to(torch.float32).reshape(got.shape)
    mask = torch.as_tensor(pow2).expand(want.shape)
    bad = mask & (got.detach().cpu() != want)
    if bool(bad.any()):
        raise AssertionError(f"{name}: {int(bad.sum())} quotients by a power of two are not the once-rounded exact value; first: {_first(bad, got.detach().cpu(), want)}")


def check_one(name, got, w):
    if w.rule == "raw":
        assert_raw(name, got, w.ref.reshape(got.shape))
    elif w.rule == "bits":
        assert_bits(name, got, w.ref.reshape(got.shape), w.dtype)
    elif w.rule == "ulp":
        assert_quotient(name, got, w.ref, w.pow2)
    else:
        assert w.rule == "interval", w.rule
        assert_interval(name, got, w.ref, w.delta, w.dtype)


def rejects(got, want):
    """True when the rules reject `got` (a mutant's {name: stored tensor}) against `want` somewhere."""
    assert set(got) == set(want), (sorted(got), sorted(want))
    for n, w in want.items():
        try:
            check_one(n, got[n], w)
        except AssertionError:
            return True
    return False


def stored(want):
    """What a kernel that computes the reference exactly would store: the comparison must ACCEPT it."""
    return {n: (w.ref if w.rule == "raw" else w.ref.to(w.dtype)) for n, w in want.items()}


def truncate_bf16(exact):
    """fp32 -> bf16 by dropping the low 16 bits instead of rounding to nearest even."""
    bits = exact.float().contiguous().view(torch.int32) & -65536
    return bits.view(torch.float32).to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------------------
# preconditions
# ---------------------------------------------------------------------------------------------------------------------
def check_sum_output(name, ref, bound, dt, unit=1.0, adds=True):
    check_exact(name, bound / unit)
    check_distinct(name, ref.reshape(-1))
    if ref.numel() >= ROUNDING_MIN_NUMEL:
        zeros = float((ref == 0).double().mean())
        assert zeros <= 0.5, f"{name}: {zeros:.0%} of the outputs are zero"
        if dt == "bf16" and adds:
            share = rounding_share(ref)
            assert share >= 0.05, f"{name}: only {share:.1%} of the outputs need rounding in bf16 (need 5 %)"


def check_term_floor(name, min_term, delta):
    m, d = float(torch.as_tensor(min_term).min()), float(torch.as_tensor(delta).max())
    assert m >= FLOOR * d, f"{name}: the smallest term {m:.4g} is below 2^10 delta = {FLOOR * d:.4g}: a dropped term could hide"


# ---------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------
def raw_values(g, shape, dt):
    """Finite random values over 60 binades in `dt`; 5 % each of +0, -0 and subnormals of either sign."""
    td = DT[dt] if isinstance(dt, str) else dt
    t = (torch.randn(tuple(shape), generator=g) * 2.0 ** ints(g, shape, -30, 30)).to(td)
    it, mant, sign = (torch.int16, 7, -2 ** 15) if td == torch.bfloat16 else (torch.int32, 23, -2 ** 31)
    r = torch.rand(tuple(shape), generator=g)
    neg = torch.randint(0, 2, tuple(shape), generator=g) * sign
    sub = torch.randint(1, 2 ** mant, tuple(shape), generator=g) + neg
    bits = t.view(it).long()
    bits = torch.where(r < 0.15, sub, bits)
    bits = torch.where(r < 0.10, torch.full_like(bits, sign), bits)
    bits = torch.where(r < 0.05, torch.zeros_like(bits), bits)
    out = bits.to(it).view(td)
    assert bool(torch.isfinite(out.float()).all())
    return out


def has_edge_values(t):
    i = _int_view(t).long()
    mant = 7 if t.dtype == torch.bfloat16 else 23
    mag = i & (2 ** (8 * t.element_size() - 1) - 1)
    return bool((i == 0).any()) and bool(((mag == 0) & (i != 0)).any()) and bool(((mag > 0) & (mag < 2 ** mant)).any())


def big_ints(g, shape):
    """Integers of magnitude 128 .. 255 with a random sign: 8 significant bits, so that a sum of two already leaves bf16."""
    return ints(g, shape, 128, 255) * (ints(g, shape, 0, 1) * 2 - 1)


def _adjoint(fn, shape_nchw, gy_nchw):
    x = torch.zeros(shape_nchw, dtype=torch.float64, requires_grad=True)
    (dx,) = torch.autograd.grad(fn(x), x, gy_nchw)
    return dx


def _up(x):
    return F.interpolate(x, scale_factor=2, mode="nearest")


def _avg(x, include_pad=False):
    return F.avg_pool2d(x, 3, 2, 1, count_include_pad=include_pad)


# ---------------------------------------------------------------------------------------------------------------------
# rule 1: copies and selections
# ---------------------------------------------------------------------------------------------------------------------
def copy_operands(dt, geom, seed=0):
    return raw_values(_gen(seed + sum(geom) + 13 * geom[3]), geom, dt)


def copy_reference(kind, x, P=None):
    """kind: "up" | "reflect" | "maxpool".  float64 holds every bf16 / fp32 value, -0 and the subnormals included."""
    if x.numel() >= ROUNDING_MIN_NUMEL:
        assert has_edge_values(x), f"{kind}: the operands lack +0, -0 or a subnormal"
    fn = {"up": _up, "reflect": lambda t: nn.ReflectionPad2d(P)(t), "maxpool": lambda t: F.max_pool2d(t, 2)}[kind]
    return {"y": Want(nhwc(fn(nchw(x))).to(x.dtype), x.dtype, "raw")}


def assemble_operands(dt, N, H, W, cp, cs, cf, seed=0):
    g = _gen(seed + N + H * W + cp + 10 * cf)
    return dict(planar=raw_values(g, (N, cp, H, W), torch.float32) if cp else None,
                image=raw_values(g, (N, H, W, cs), dt) if cf else None, cf=cf, cp=cp, N=N, H=H, W=W, dt=dt)


def assemble_reference(o, mut=None):
    """[planar.to(dtype) | image[..., :cf] | +0] per pixel."""
    td = DT[o["dt"]]
    parts = []
    if o["cp"]:
        pl = o["planar"].permute(0, 2, 3, 1)
        parts.append(truncate_bf16(pl) if (mut == "truncating-store" and td == torch.bfloat16) else pl.to(td))
    if o["cf"]:
        parts.append(o["image"][..., :o["cf"]])
    parts.append(torch.zeros(o["N"], o["H"], o["W"], 8 - o["cp"] - o["cf"], dtype=td))
    out = torch.cat(parts, 3).contiguous()
    return {"out": out} if mut else {"out": Want(out, td, "raw")}


# ---------------------------------------------------------------------------------------------------------------------
# rule 2: short sums with exact operands
# ---------------------------------------------------------------------------------------------------------------------
def _store(exact, dt, mut):
    return truncate_bf16(exact) if (mut == "truncating-store" and dt == "bf16") else exact.to(DT[dt])


def up_bwd_operands(dt, geom, seed=0):
    n, h, w, c = geom
    return big_ints(_gen(seed + 3 * sum(geom) + c), (n, 2 * h, 2 * w, c)).to(DT[dt])


def up_bwd_reference(dy, dt, mut=None):
    n, h2, w2, c = dy.shape
    shape = (n, c, h2 // 2, w2 // 2)
    if mut == "bf16-accumulate":                    # the four children added one after the other into a bf16 accumulator
        d = dy.view(n, h2 // 2, 2, w2 // 2, 2, c).to(torch.bfloat16)
        acc = d[:, :, 0, :, 0]
        for a, b in ((0, 1), (1, 0), (1, 1)):
            acc = (acc.float() + d[:, :, a, :, b].float()).to(torch.bfloat16)
        return {"dx": acc.to(DT[dt])}
    exact = nhwc(_adjoint(_up, shape, nchw(dy)))
    if mut:
        return {"dx": _store(exact, dt, mut)}
    check_sum_output(f"upsample2x_bwd {tuple(dy.shape)}", exact, nhwc(_adjoint(_up, shape, nchw(dy).abs())), dt)
    return {"dx": Want(exact, DT[dt], "bits")}


def reflect_bwd_operands(dt, n, h, w, c, p, seed=0):
    return big_ints(_gen(seed + 7 * h + w + c + p), (n, h + 2 * p, w + 2 * p, c)).to(DT[dt])


def reflect_bwd_reference(dy, p, dt, mut=None):
    n, hp, wp, c = dy.shape
    shape = (n, c, hp - 2 * p, wp - 2 * p)
    pad = nn.ReflectionPad2d(p)
    d = nchw(dy)
    if mut == "no-corner-mirror":                   # the terms mirrored in BOTH axes left out: the four p x p corners of the padded image
        d = d.clone()
        for ys in (slice(0, p), slice(hp - p, hp)):
            for xs in (slice(0, p), slice(wp - p, wp)):
                d[:, :, ys, xs] = 0
    exact = nhwc(_adjoint(pad, shape, d))
    if mut:
        return {"dx": _store(exact, dt, mut)}
    check_sum_output(f"reflect_pad_bwd {tuple(dy.shape)} P={p}", exact, nhwc(_adjoint(pad, shape, d.abs())), dt)
    return {"dx": Want(exact, DT[dt], "bits")}


ACTS = {"none": 0, "relu": 1, "lrelu": 2}


def _act64(pre, act):
    return {"none": lambda t: t * 1, "relu": F.relu, "lrelu": lambda t: F.leaky_relu(t, SLOPE)}[act](pre)


def act_operands(dt, nq, seed=0):
    """pre: integers in [-2, 4] (0 included: the activation output holds exact zeros on either side's border); g1, g2 big integers."""
    g = _gen(seed + nq % 100003)
    n = 4 * nq
    return dict(pre=ints(g, (n,), -2, 4), g1=big_ints(g, (n,)).to(DT[dt]), g2=big_ints(g, (n,)).to(DT[dt]), dt=dt)


def act_output(o, act):
    """The activation output the kernel is handed, in the operand dtype (representable: multiples of 1/4 below 8)."""
    y = _act64(o["pre"].double(), act)
    assert torch.equal(y, y.to(DT[o["dt"]]).double())
    return y.to(DT[o["dt"]])


def act_bwd_reference(o, act, two, mut=None):
    """(g1 [+ g2]) * act'(pre) by torch's own backward of F.relu / F.leaky_relu: 0 / the slope at pre == 0."""
    dt = o["dt"]
    pre = o["pre"].double().requires_grad_()
    y = _act64(pre, act)
    gsum = o["g1"].double() + (o["g2"].double() if two else 0)
    (exact,) = torch.autograd.grad(y, pre, gsum)
    if mut == "lrelu-one-at-zero":
        exact = torch.where(pre.detach() == 0, gsum, exact)
    if mut:
        return {"out": _store(exact, dt, mut)}
    name = f"act gradient {act} two={two} n={pre.numel()}"
    if act != "none" and pre.numel() >= ROUNDING_MIN_NUMEL:
        assert bool((y == 0).any()), f"{name}: no exact zero in the activation output"
    check_sum_output(name, exact, 4 * (o["g1"].double().abs() + o["g2"].double().abs() * two), dt, adds=two)
    return {"out": Want(exact, DT[dt], "bits")}


def blend_operands(dt, P, C, seed=0):
    g = _gen(seed + P % 100003 + C)
    lv = torch.tensor([0.0, 0.25, 0.5, 1.0])
    hair, back = lv[torch.randint(0, 4, (P,), generator=g)], lv[torch.randint(0, 4, (P,), generator=g)]
    if P >= 3:                                      # the first pixel blends to an exact zero, the last one by 3/4 and 3/4 (products that need rounding)
        hair[0] = back[0] = 1.0
        hair[-1] = back[-1] = 0.25
    return dict(bg=big_ints(g, (P, C)).to(DT[dt]), x=big_ints(g, (P, C)).to(DT[dt]), dy=big_ints(g, (P, C)).to(DT[dt]), hair=hair, back=back, dt=dt)


def blend_reference(o, act, mut=None):
    """y = act(bg (1 - hair) + x (1 - back)) and both gradients by autograd; every product a multiple of 1/16 below 2^24 of them."""
    dt = o["dt"]
    bg, x = o["bg"].double().requires_grad_(), o["x"].double().requires_grad_()
    wb, wx = (1 - o["hair"].double()).view(-1, 1), (1 - o["back"].double()).view(-1, 1)
    if mut == "weights-swapped":
        wb, wx = wx, wb
    y = _act64(bg * wb + x * wx, act)
    dbg, dx = torch.autograd.grad(y, [bg, x], o["dy"].double())
    out = {"y": y.detach(), "dbg": dbg, "dx": dx}
    if mut:
        return {n: _store(v, dt, mut) for n, v in out.items()}
    name = f"blend {act} {tuple(bg.shape)}"
    if act != "none" and y.numel() >= ROUNDING_MIN_NUMEL:
        assert bool((y == 0).any()), f"{name}: no exact zero in the activation output"
    bound = 16 * (o["bg"].double().abs() + o["x"].double().abs())
    check_sum_output(name + " y", out["y"], bound, dt)
    for n in ("dbg", "dx"):
        check_sum_output(f"{name} {n}", out[n], 16 * o["dy"].double().abs(), dt)
    return {n: Want(v, DT[dt], "bits") for n, v in out.items()}


# ---------------------------------------------------------------------------------------------------------------------
# rule 3: max-pool adjoint
# ---------------------------------------------------------------------------------------------------------------------
def maxpool_operands(dt, geom, seed=0):
    """pre: integers in [-2, 2] with a planted tie in every other window (x = pre, or x = relu(pre) when the kernel is told that x is a
    ReLU's output); dy big integers."""
    n, h, w, c = geom
    g = _gen(seed + 5 * sum(geom) + c)
    pre = ints(g, geom, -2, 2)
    he, we = h // 2 * 2, w // 2 * 2
    win = pre[:, :he, :we].view(n, he // 2, 2, we // 2, 2, c)                  # (a view: the planting below lands in pre)
    oy, ox, ch = torch.meshgrid(torch.arange(he // 2), torch.arange(we // 2), torch.arange(c), indexing="ij")
    plant = ((oy + ox + ch) % 2 == 0).expand(n, -1, -1, -1)
    for a, b in ((0, 1), (1, 0)):                                               # every other window: its second and third element tie at the top value
        win[:, :, a, :, b] = torch.where(plant, torch.full_like(win[:, :, a, :, b], 2.0), win[:, :, a, :, b])
    return dict(pre=pre, dy=big_ints(g, (n, h // 2, w // 2, c)).to(DT[dt]), dt=dt)


def maxpool_input(o, relu_input):
    return (F.relu(o["pre"]) if relu_input else o["pre"]).to(DT[o["dt"]])


def tie_share(x):
    n, h, w, c = x.shape
    win = x[:, :h // 2 * 2, :w // 2 * 2].reshape(n, h // 2, 2, w // 2, 2, c).permute(0, 1, 3, 5, 2, 4).reshape(-1, 4).double()
    return float(((win == win.amax(1, keepdim=True)).sum(1) >= 2).double().mean())


def _flip_windows(t):
    """NCHW: every 2 x 2 window turned by 180 degrees (the odd last row / column stays)."""
    n, c, h, w = t.shape
    out = t.clone()
    he, we = h // 2 * 2, w // 2 * 2
    out[:, :, :he, :we] = t[:, :, :he, :we].reshape(n, c, he // 2, 2, we // 2, 2).flip(3, 5).reshape(n, c, he, we)
    return out


def maxpool_bwd_reference(o, relu_input, mut=None):
    """The gradient of F.max_pool2d(x, 2) (of F.max_pool2d(F.relu(pre), 2) with respect to pre when relu_input): ATen's first maximum
    in scan order, +0 everywhere else, the odd last row and column included."""
    dt = o["dt"]
    pre = nchw(o["pre"])
    if mut == "last-maximum":
        pre = _flip_windows(pre)
    leaf = pre.clone().requires_grad_()
    x = F.relu(leaf) if relu_input else leaf
    if mut == "relu-input-ignored":
        x = x.detach().requires_grad_()
        leaf = x
    (dx,) = torch.autograd.grad(F.max_pool2d(x, 2), leaf, nchw(o["dy"]))
    if mut == "last-maximum":
        dx = _flip_windows(dx)
    ref = nhwc(dx).to(DT[dt])
    if mut:
        return {"dx": ref}
    share = tie_share(maxpool_input(o, relu_input))
    assert share >= TIE_SHARE, f"maxpool {tuple(o['pre'].shape)}: only {share:.0%} of the windows hold a tie"
    return {"dx": Want(ref, DT[dt], "raw")}


# ---------------------------------------------------------------------------------------------------------------------
# rule 4: quotients by a count that is no power of two
# ---------------------------------------------------------------------------------------------------------------------
def _pool_counts(n, c, h, w):
    """Elements inside the image per window: the operator itself, padding counted, on a tensor of ones."""
    return (_avg(torch.ones(n, c, h, w, dtype=torch.float64), True) * 9).round()


def _is_pow2(cnt):
    c = cnt.long()
    return (c & (c - 1)) == 0


def avgpool_operands(dt, geom, seed=0):
    n, h, w, c = geom
    g = _gen(seed + 11 * sum(geom) + c)
    return dict(x=big_ints(g, geom).to(DT[dt]), dy=big_ints(g, (n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c)).to(DT[dt]), dt=dt)


def avgpool_fwd_reference(o, mut=None):
    """f32: the window sum is exact, so one quotient (counts 4, 6, 9; 1, 2, 3 when an axis is 1).  bf16: the interval with k = 10."""
    dt = o["dt"]
    x = nchw(o["x"])
    cnt = _pool_counts(*x.shape)                    # window element counts, from the operator itself on a tensor of ones
    exact = _avg(x, include_pad=(mut == "count-include-pad"))
    if mut == "bf16-reciprocal":
        exact = (_avg(x) * cnt) * (1 / cnt).to(torch.bfloat16).double()
    if mut:
        return {"y": _store(nhwc(exact), dt, mut)}
    name = f"avgpool3s2_fwd {tuple(o['x'].shape)}"
    terms = _avg(x.abs())
    check_exact(name, terms * cnt)
    check_distinct(name, exact.reshape(-1))
    delta = K["avgpool_fwd"] * U24 * terms
    check_term_floor(name, -F.max_pool2d(-x.abs(), 3, 2, 1) / cnt, delta)
    if dt == "f32":
        return {"y": Want(nhwc(exact), torch.float32, "ulp", None, nhwc(_is_pow2(cnt)))}
    return {"y": Want(nhwc(exact), DT[dt], "interval", nhwc(delta))}


def avgpool_bwd_reference(o, mut=None):
    """Up to 4 quotients added: the interval with k = 11 in either dtype."""
    dt = o["dt"]
    n, h, w, c = o["x"].shape
    dy = nchw(o["dy"])
    fn = lambda t: _avg(t, include_pad=(mut == "count-include-pad"))
    exact = nhwc(_adjoint(fn, (n, c, h, w), dy))
    if mut:
        return {"dx": _store(exact, dt, mut)}
    name = f"avgpool3s2_bwd {tuple(o['x'].shape)}"
    terms = nhwc(_adjoint(_avg, (n, c, h, w), dy.abs()))
    delta = K["avgpool_bwd"] * U24 * terms
    if exact.numel() >= ROUNDING_MIN_NUMEL * 4:        # (one window's four pixels share a value: a small image repeats by construction)
        check_distinct(name, exact.reshape(-1))
    check_term_floor(name, (dy.abs() / _pool_counts(n, c, h, w)), delta)
    return {"dx": Want(exact, DT[dt], "interval", delta)}


L1_GSCALE = 3.0


def l1_operands(dt, nq, seed=0):
    """a: nonzero integers in [-2, 2]; b = a + d, d in [-2, 2] (zero at a fifth of the elements: sign 0)."""
    g = _gen(seed + nq % 100003 + 1)
    a = nonzero_ints(g, (4 * nq,), 2)
    return dict(a=a.to(DT[dt]), b=(a + ints(g, (4 * nq,), -2, 2)).to(DT[dt]), dt=dt)


def l1_bwd_reference(o, mut=None):
    """d/da of F.l1_loss(a, b) * 3: sign(a - b) * 3 / numel."""
    dt = o["dt"]
    a = o["a"].double().requires_grad_()
    (exact,) = torch.autograd.grad(F.l1_loss(a, o["b"].double()) * L1_GSCALE, a)
    n = a.numel()
    if mut == "no-inverse-numel":
        exact = exact * n
    if mut:
        return {"da": _store(exact, dt, mut)}
    if n >= ROUNDING_MIN_NUMEL:
        assert {-1.0, 0.0, 1.0} <= set(torch.sign(exact).unique().tolist())
    if dt == "f32":
        return {"da": Want(exact, torch.float32, "ulp", None, n & (n - 1) == 0)}
    return {"da": Want(exact, DT[dt], "interval", K["l1_bwd"] * U24 * exact.abs())}


HINGE_GSCALE = 3.0


def hinge_bwd_reference(o, mode, use_w, dt, mut=None):
    """d/dx of -(f(x) * w).mean() * 3, f as in test_hinge_loss_and_wide_edge_weight_fused; census_operands.hinge_operands puts logits on
    both sides of the kinks and none on them."""
    x = o["x"].double().requires_grad_()
    assert bool((x.abs() != 1).all())
    f = x if mode == 0 else torch.clamp_max((x if mode == 1 else -x) - 1, 0)
    wgt = o["w"].double() if (use_w and mut != "no-weight") else 1.0
    (exact,) = torch.autograd.grad(-(f * wgt).mean() * HINGE_GSCALE, x)
    if mut:
        return {"dx": _store(exact, dt, mut)}
    n = x.numel()
    if n >= ROUNDING_MIN_NUMEL and mode:
        assert bool((exact == 0).any()) and bool((exact != 0).any()), "logits on one side of the hinge only"
    if dt == "f32" and not use_w:
        return {"dx": Want(exact, torch.float32, "ulp", None, n & (n - 1) == 0)}
    return {"dx": Want(exact, DT[dt], "interval", K["hinge_bwd"] * U24 * exact.abs())}


# ---------------------------------------------------------------------------------------------------------------------
# rule 5: Adam, one teacher-forced step
# ---------------------------------------------------------------------------------------------------------------------
ADAM_LR, ADAM_EPS = 0.01, 1e-8


def f32r(v):
    """The value a `float` argument of the C ABI receives, widened back to double."""
    return ctypes.c_float(v).value


def adam_operands(numel, betas, scale, step, seed=0):
    """Distinct values per element: |g| in [0.5, 1.5), |p| in [0.03, 0.05), one per cell of a grid of numel cells in a random order (and at
    a random place inside its cell: full mantissas), random signs.
    m has g's sign and 0.5 .. 1.5 times |g scale| (at beta1 = 0: 4096 times more, the state a one-branch lerp would round g away
    against); v is 0.25 .. 1 times (g scale)^2, as a running mean of squared gradients is."""
    g_ = _gen(seed + numel % 100003 + step + int(1000 * betas[0]) + int(64 * scale))
    grid = lambda: (torch.randperm(numel, generator=g_).double() + 0.25 + 0.5 * torch.rand(numel, generator=g_, dtype=torch.float64)) / numel
    sign = lambda: (torch.randint(0, 2, (numel,), generator=g_) * 2 - 1).double()
    g = (sign() * (0.5 + grid())).float()
    p = (sign() * (0.03 + 0.02 * grid())).float()
    gg = g.double() * f32r(scale)
    m = (gg * (0.5 + grid()) * (4096.0 if betas[0] == 0 else 1.0)).float()
    v = (gg * gg * (0.25 + 0.75 * grid())).float()
    assert torch.unique(g).numel() == numel and torch.unique(p).numel() == numel
    return dict(p=p, g=g, m=m, v=v, betas=betas, scale=scale, step=step, lr=ADAM_LR, eps=ADAM_EPS)


def _adam_formula(o, mut):
    """MUTANTS only: Adam's update written out in float64 with one edit (the true value comes from torch.optim.Adam)."""
    b1, b2, lr, eps, gs, step = f32r(o["betas"][0]), f32r(o["betas"][1]), f32r(o["lr"]), f32r(o["eps"]), f32r(o["scale"]), o["step"]
    p, m, v = o["p"].double(), o["m"].double(), o["v"].double()
    g = o["g"].double() * (1.0 if mut == "grad-scale-ignored" else gs)
    if mut == "one-branch-lerp":                    # fp32 m + (g - m) * w: at w = 1 it rounds g away against a large m
        gf = g.float()
        m1 = (o["m"] + (gf - o["m"]) * torch.tensor(1 - b1, dtype=torch.float32)).double()
    else:
        m1 = m + (g - m) * (1 - b1)
    v1 = ((1 - b2) * v + b2 * g * g) if mut == "beta2-swapped" else (b2 * v + (1 - b2) * g * g)
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    denom = v1.sqrt() / (bc2 if mut == "bc2-without-sqrt" else bc2 ** 0.5) + eps
    p1 = p - lr / bc1 * m1 / denom
    if mut == "skip-at-wrap":                       # the first element of the grid-stride loop's second trip left as it was
        assert p.numel() > WRAP
        p1[WRAP], m1[WRAP], v1[WRAP] = p[WRAP], m[WRAP], v[WRAP]
    return {"p": p1.float(), "m": m1.float(), "v": v1.float()}


def adam_reference(o, mut=None):
    """torch.optim.Adam(foreach=False) on float64, its state preloaded with (m, v) and step - 1, its gradient g * grad_scale, its
    hyper-parameters the fp32-rounded values widened to double.

    Bounds (u = 2^-24, gg = g * grad_scale; roundings counted on torch's update as written, then DOUBLED for slack):
      m   lerp: sub, mul, add, and the scalings gg and 1 - beta1                       5 -> d_m = 10 u (|(1 - b1) gg| + |b1 m|)
      v   mul; addcmul: square, value, add; the scalar 1 - beta2; gg twice (squared)    7 -> d_v = 14 u (b2 v + (1 - b2) gg^2)
      p   denom = sqrt(v') / sqrt(bc2) + eps: sqrt, div, the scalar sqrt(bc2) (3 on the quotient), add (1 on denom), and d_v through
          the square root:      d_den = d_v / (2 sqrt(v') sqrt(bc2)) + 2 u (3 sqrt(v') / sqrt(bc2) + denom)
          p' = p - step_size m' / denom: d_m and d_den to first order, then div, the scalars lr / bc1 (2), mul (4 on the update U),
          add (1 on |p| + |U|):  d_p = step_size (d_m / denom + |m'| d_den / denom^2) + 2 u (4 |U| + |p| + |U|)"""
    if mut:
        return _adam_formula(o, mut)
    b1, b2, lr, eps, gs, step = f32r(o["betas"][0]), f32r(o["betas"][1]), f32r(o["lr"]), f32r(o["eps"]), f32r(o["scale"]), o["step"]
    p0, m0, v0 = o["p"].double(), o["m"].double(), o["v"].double()
    gg = o["g"].double() * gs
    p = p0.clone().requires_grad_()
    p.grad = gg.clone()
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps, foreach=False)
    opt.state[p] = {"step": torch.tensor(float(step - 1)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
    opt.step()
    st = opt.state[p]
    assert float(st["step"]) == step
    p1, m1, v1 = p.detach(), st["exp_avg"], st["exp_avg_sq"]
    name = f"adam n={p0.numel()} betas={o['betas']} scale={o['scale']:.3g} step={step}"
    tm = [((1 - b1) * gg).abs()] + ([(b1 * m0).abs()] if b1 else [])
    d_m = 10 * U24 * sum(tm)
    tv = [b2 * v0, (1 - b2) * gg * gg]
    d_v = 14 * U24 * sum(tv)
    bc1, bc2s = 1 - b1 ** step, (1 - b2 ** step) ** 0.5
    sq = v1.sqrt()
    denom, ss = sq / bc2s + eps, lr / bc1
    upd = ss * m1 / denom
    d_den = d_v / (2 * sq * bc2s) + 2 * U24 * (3 * sq / bc2s + denom)
    d_p = ss * (d_m / denom + m1.abs() * d_den / denom ** 2) + 2 * U24 * (5 * upd.abs() + p0.abs())
    check_term_floor(name + " m", torch.stack(tm).amin(0) / d_m, 1.0)
    check_term_floor(name + " v", torch.stack(tv).amin(0) / d_v, 1.0)
    check_term_floor(name + " p", torch.minimum(p0.abs(), upd.abs()) / d_p, 1.0)
    pow2_scale = gs > 0 and (gs * 2.0 ** 40) == float(int(gs * 2.0 ** 40)) and bin(int(gs * 2.0 ** 40)).count("1") == 1
    if b1 == 0 and pow2_scale:
        assert torch.equal(m1, gg)
        wm = Want(gg, torch.float32, "bits")        # exp_avg = g * grad_scale, bit for bit
    else:
        wm = Want(m1, torch.float32, "interval", d_m)
    return {"p": Want(p1, torch.float32, "interval", d_p), "m": wm, "v": Want(v1, torch.float32, "interval", d_v)}
