"""Operands for which a convolution's float64 value is EXACT in fp32, whatever the summation order.

Every operand is a small integer (or an integer times a power of two), every product and every partial sum an integer (a multiple
of 1/8 once a 0.25 slope is involved) whose magnitude stays below 2^24.  fp32 accumulation of such terms is exact in any order --
MFMA chunk order, two-level sums, split-K partials, fp32 atomics, slab order -- so the only rounding a kernel may make is the one
store conversion, and its result must equal ``reference.to(dtype)`` bit for bit.  No tolerance is involved.

Recipe (plain torch, no GPU):
  activations, output gradients   integers in [-2, 2]; the channels that meet a planted weight are 2
  weights                         +-1 at density ``density / K`` (K = cin * taps, default density 64), 0 elsewhere, and a CANCELLING
                                  PAIR: w[:, 0, first tap] = +512, w[:, cin - 1, last tap] = -512.  Intermediate sums sit near
                                  +-1024 while the results are small; at an image border one half of the pair falls into the zero
                                  padding, the exact result is +-1024 + k and needs rounding in bf16.
  the same pair, transposed       w[0, :, first tap] = +512, w[cout - 1, :, last tap of the first tap's stride class] = -512, and
                                  the output gradient's channels 0 and cout - 1 are 2: the data-gradient sum cancels too
  ``holes``                       share of pixels at which the last channel (activation and output gradient) is 0 instead of 2:
                                  the pair does not cancel there, as at a border.  For images so large that their border is less
                                  than 5 % of the pixels (the chip-filling shapes): the rounding condition below, not a looser one.
  bias                            integers in [-8, 8];  residual: integers in [-4, 4];  slopes: 0.25
  weight gradient on its own      x and dy integers in [-2, 2]; at two pixels far apart (first and last image row, which any split
                                  of the pixel sum separates) dy = +64 / -64 against x = 64: every dW entry passes through +-4096
  SPADE                           mean: integers in [-2, 2]; rstd in {1/2, 1, 2}; gamma / beta weights and biases as above

Preconditions (``check_*``) are asserted on the reference alone, before a kernel's result is looked at:
  exactness        the same sum over |operands| stays below 2^24 everywhere (ConvReference: a closed-form upper bound of it)
  rounding         at least 5 % of the bf16 forward outputs have an exact value that bf16 cannot hold
  non-degeneracy   at least 100 distinct reference values (a bias gradient: a quarter of its channel count, see check_distinct),
                   at most half of the outputs zero
Gradients have the exactness and the distinct-values conditions only (dw / db are fp32).
"""
import torch
import torch.nn.functional as F

DT = {"f32": torch.float32, "bf16": torch.bfloat16}
LIMIT = float(2 ** 24)
SLOPE = 0.25
BIG, WG_BIG = 512.0, 64.0


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).float()


def sparse_signs(g, shape, density, tilt=0.0):
    """+-1 with probability `density`, 0 elsewhere; +1 with probability 1/2 + tilt among them."""
    keep = torch.rand(tuple(shape), generator=g) < density
    sign = (torch.rand(tuple(shape), generator=g) < 0.5 + tilt).float() * 2 - 1
    return sign * keep


def conv_weight(g, cin, cout, k, s=1, density=64.0, transposed_pair=True, tilt=0.0):
    """[cout, cin, k, k] fp32 of the recipe.  The transposed pair's negative half sits on the last tap of the first tap's stride
    class ((k - 1) // s * s): the data gradient of a strided conv sums each output-parity class over its own taps only."""
    w = sparse_signs(g, (cout, cin, k, k), min(1.0, density / (cin * k * k)), tilt)
    w[:, 0, 0, 0] = BIG
    w[:, cin - 1, k - 1, k - 1] = -BIG
    if transposed_pair and cout >= 8:
        kt = (k - 1) // s * s
        w[0, :, 0, 0] = BIG
        w[cout - 1, :, kt, kt] = -BIG
    return w


def _image(g, shape, holes, lo=-2):
    """NHWC integers in [lo, 2], first and last channel 2 (last channel 0 at a `holes` share of the pixels)."""
    t = ints(g, shape, lo, 2)
    t[..., 0] = 2
    t[..., -1] = 2
    if holes:
        t[..., -1] *= (torch.rand(tuple(shape[:3]), generator=g) >= holes).float()
    return t


def conv_operands(dt, cin, cout, k, s, p, H, W, N, bias=True, resid=False, density=64.0, holes=0.0, seed=0, bias_lo=-8, tilt=0.0, **_):
    """dict(x, w, b, r, gy): x / r / gy in `dt` (NHWC), w / b fp32; b and r None when not asked for.
    bias_lo = 0 (a ReLU case): the bias from [0, 8], so that fewer than half of the outputs are clamped to zero.
    tilt > 0 (ReLU with ONE output channel, where a bias cannot do that against a dense kernel): +1 weights outnumber -1 by 2 tilt
    and the activations come from [-1, 2], so that the sums have a positive mean."""
    g = _gen(seed + 1000 * cin + cout + 7 * k)
    ho, wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    x = _image(g, (N, H, W, cin), holes, -1 if tilt else -2)
    w = conv_weight(g, cin, cout, k, s, density, tilt=tilt)
    b = ints(g, (cout,), bias_lo, 8) if bias else None
    r = ints(g, (N, ho, wo, cout), -4, 4).to(DT[dt]) if resid else None
    gy = _image(g, (N, ho, wo, cout), holes) if cout >= 8 else ints(g, (N, ho, wo, cout), -2, 2)
    return dict(x=x.to(DT[dt]), w=w, b=b, r=r, gy=gy.to(DT[dt]))


def wgrad_operands(dt, N, H, W, cin, cg, k, s, p, seed=0, **_):
    """x [N, H, W, cin], dy [N, ho, wo, cg] for ops.conv_wgrad on its own.  dy = +64 at the first output pixel of the first image and
    -64 at the last output pixel of the last image, x = 64 on the k x k window either of them meets: every dW entry whose tap lies
    inside the image at those corners gains +4096 early and loses it late in pixel order, on both sides of any split of the sum."""
    g = _gen(seed + 100 * cin + cg + H)
    ho, wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    x, dy = ints(g, (N, H, W, cin), -2, 2), ints(g, (N, ho, wo, cg), -2, 2)
    dy[0, 0, 0], dy[N - 1, ho - 1, wo - 1] = WG_BIG, -WG_BIG
    y1, x1 = (ho - 1) * s - p, (wo - 1) * s - p                    # top-left input pixel of the last output pixel's window
    x[0, :max(k - p, 1), :max(k - p, 1)] = WG_BIG
    x[N - 1, max(y1, 0):y1 + k, max(x1, 0):x1 + k] = WG_BIG
    return dict(x=x.to(DT[dt]), dy=dy.to(DT[dt]))


def spade_operands(dt, C, H, W, N=2, ca=128, up=False, density=64.0, holes=0.0, seed=0):
    """x (half resolution when `up`), actv, gamma / beta weights and biases, mean, rstd, gh for ops.spade_modulate.
    (x - mean) * rstd is a multiple of 1/2 of magnitude <= 8, 1 + gamma and beta integers: h is a multiple of 1/2 (1/8 under the 0.25
    slope) below 2^24.  The gradient of the gamma|beta conv's output, gh * act' * (x - mean) * rstd, is a multiple of 1/8 below 16 and
    so exact in bf16, the dtype the operator layer stores it in between its two launches."""
    g = _gen(seed + C + H)
    hs, ws = (H // 2, W // 2) if up else (H, W)
    x = ints(g, (N, hs, ws, C), -2, 2)
    actv = _image(g, (N, H, W, ca), holes)
    wg, wb = conv_weight(g, ca, C, 3, 1, density), conv_weight(g, ca, C, 3, 1, density)
    bg, bb = ints(g, (C,), -8, 8), ints(g, (C,), -8, 8)
    mean = ints(g, (C,), -2, 2)
    rstd = 2.0 ** ints(g, (C,), -1, 1)
    gh = _image(g, (N, H, W, C), 0.0)
    return dict(x=x.to(DT[dt]), actv=actv.to(DT[dt]), wg=wg, bg=bg, wb=wb, bb=bb, mean=mean, rstd=rstd, gh=gh.to(DT[dt]))


# ---------------------------------------------------------------------------------------------------------------------
# references: torch on the CPU, float64 (fp32 where asked: the same bits once the exactness precondition holds)
# ---------------------------------------------------------------------------------------------------------------------
def nchw(t, dtype=torch.float64):
    return t.detach().to(dtype).permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def act_fn(v, act, slope=SLOPE):
    if act == "relu":
        return torch.clamp_min(v, 0)
    if act == "lrelu":
        return torch.where(v > 0, v, v * slope)
    assert act == "none", act
    return v


def act_grad(v, act, slope=SLOPE):
    """d act / d pre from the pre-activation (or the output: same sign, same zeros)."""
    if act == "relu":
        return (v > 0).to(v.dtype)
    if act == "lrelu":
        return torch.where(v > 0, torch.ones_like(v), torch.full_like(v, slope))
    return torch.ones_like(v)


def check_exact(name, bound):
    m = float(bound.detach().abs().max())
    assert m < LIMIT, f"{name}: the sum over |operands| reaches {m:.4g} >= 2^24 -- the recipe is not exact here"
    return m


def check_distinct(name, ref):
    """>= 100 distinct values.  The one exception is a bias gradient (1-d, one entry per channel), which cannot hold 100 values
    below 100 channels and, being a column sum of npix terms from [-2, 2], repeats values where the pixels are few (32 distinct of
    128 channels at 32 pixels, the smallest weight-gradient shape): a quarter of its channel count, rounded up, at 100 the most."""
    need = min(100, -(-ref.numel() // 4)) if ref.dim() == 1 else 100
    n = int(torch.unique(ref).numel())
    assert n >= need, f"{name}: only {n} distinct reference values (need {need})"
    return n


def rounding_share(ref):
    """Share of the exact values bf16 cannot hold."""
    return float((ref.double() != ref.to(torch.bfloat16).double()).double().mean())


def check_forward(name, ref, dt):
    check_distinct(name, ref)
    zeros = float((ref == 0).double().mean())
    assert zeros <= 0.5, f"{name}: {zeros:.0%} of the outputs are zero"
    share = rounding_share(ref)
    if dt == "bf16":
        assert share >= 0.05, f"{name}: only {share:.1%} of the outputs need rounding in bf16 (need 5 %)"
    return share


class ConvReference:
    """The exact linear convolution of one operand set, computed ONCE, and from it every epilogue's output and gradients
    (bias: False, True = the operand set's, or a tensor to use in its place):
    y = act(conv(x, w) + b + r) and (dx, dw, db, dres), differentiated with act'(pre) taken from the exact pre-activation.
    The exactness precondition is asserted on closed-form bounds of the sums over |operands| (|x|, |gy| <= 2, |b| <= 8, |r| <= 4)."""

    def __init__(self, ops_, k, s, p, ref_dtype=torch.float64, name="conv"):
        self.o, self.name, self.rd = ops_, name, ref_dtype
        x, w, gy = ops_["x"], ops_["w"], ops_["gy"]
        assert float(x.float().abs().max()) <= 2 and float(gy.float().abs().max()) <= 2
        npix = gy.numel() // gy.shape[3]
        check_exact(name + " y", 2 * w.abs().sum((1, 2, 3)) + 8 + 4)
        check_exact(name + " dx", 4 * 2 * w.abs().sum((0, 2, 3)))            # x 4: under a 0.25 slope the gradient terms are multiples of 1/4,
        check_exact(name + " dw", torch.tensor(4 * 4.0 * npix))              # so it is 4 |sum| that has to fit the 24-bit significand
        self.xr, self.wr = nchw(x, ref_dtype).requires_grad_(), w.to(ref_dtype).requires_grad_()
        self.lin = F.conv2d(self.xr, self.wr, None, stride=s, padding=p)

    def _pre(self, bias, resid):
        pre = self.lin.detach()
        if bias is not False:
            pre = pre + (self.o["b"] if bias is True else bias).to(self.rd).view(1, -1, 1, 1)
        if resid:
            pre = pre + nchw(self.o["r"], self.rd)
        return pre

    def forward(self, act="none", bias=True, resid=False, dt="bf16"):
        """(exact y NHWC float64, share of it that needs rounding in bf16); forward preconditions asserted."""
        y = nhwc(act_fn(self._pre(bias, resid), act)).double()
        return y, check_forward(f"{self.name} {act} y", y, dt)

    def grads(self, act="none", bias=True, resid=False):
        dpre = nchw(self.o["gy"], self.rd) * act_grad(self._pre(bias, resid), act)
        dx, dw = torch.autograd.grad(self.lin, [self.xr, self.wr], dpre, retain_graph=True)
        out = {"dx": nhwc(dx).double(), "dw": dw.double()}
        if bias is not False:
            out["db"] = dpre.double().sum((0, 2, 3))
        if resid:
            out["dres"] = nhwc(dpre).double()
        for n in ("dx", "dw", "db"):
            if n in out:
                check_distinct(f"{self.name} {act} {n}", out[n])
        return out


def conv_reference(ops_, k, s, p, act="none", with_grads=True, ref_dtype=torch.float64, dt="bf16", name="conv"):
    """One epilogue of ConvReference (bias / residual: whichever the operand set carries): (dict of exact tensors, rounding share)."""
    ref = ConvReference(ops_, k, s, p, ref_dtype, name)
    bias, resid = ops_["b"] is not None, ops_["r"] is not None
    y, share = ref.forward(act, bias, resid, dt)
    out = {"y": y}
    if with_grads:
        out.update(ref.grads(act, bias, resid))
    return out, share


def wgrad_reference(ops_, k, s, p, name="wgrad"):
    """dW in GEMM order [taps, cg, cin] and the bias gradient [cg] of ops.conv_wgrad, float64; preconditions asserted."""
    x, dy = ops_["x"], ops_["dy"]
    cin, cg = x.shape[3], dy.shape[3]
    xr = nchw(x)
    wz = torch.zeros(cg, cin, k, k, dtype=torch.float64, requires_grad=True)
    (dw,) = torch.autograd.grad(F.conv2d(xr, wz, None, stride=s, padding=p), wz, nchw(dy))
    wa = torch.zeros(cg, cin, k, k, requires_grad=True)
    (bound,) = torch.autograd.grad(F.conv2d(nchw(x, torch.float32).abs(), wa, None, stride=s, padding=p), wa, nchw(dy, torch.float32).abs())
    check_exact(name + " dw", bound)
    check_exact(name + " db", dy.float().abs().sum((0, 1, 2)))
    assert float(bound.max()) >= WG_BIG * WG_BIG, f"{name}: the planted +-4096 pair is missing"
    out = {"dw": dw.permute(2, 3, 0, 1).reshape(k * k, cg, cin).contiguous(), "db": dy.double().sum((0, 1, 2))}
    check_distinct(name + " dw", out["dw"])
    check_distinct(name + " db", out["db"])
    return out


def spade_reference(ops_, act="lrelu", up=False, dt="bf16", name="spade"):
    """h = act((x - mean) * rstd * (1 + gamma) + beta) and its gradients with respect to actv, both weights and both biases (mean and
    rstd constants), float64; preconditions asserted, the intermediate gradient's bf16 representability included."""
    o = ops_
    x = o["x"].double()
    if up:
        x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    xhat = (nchw(x) - o["mean"].double().view(1, -1, 1, 1)) * o["rstd"].double().view(1, -1, 1, 1)
    ar = nchw(o["actv"]).requires_grad_()
    leaves = [ar] + [o[n].double().requires_grad_() for n in ("wg", "bg", "wb", "bb")]
    gam = F.conv2d(ar, leaves[1], leaves[2], padding=1)
    bet = F.conv2d(ar, leaves[3], leaves[4], padding=1)
    pre = xhat * (1 + gam) + bet
    h = act_fn(pre.detach(), act)
    aa = nchw(o["actv"], torch.float32).abs()
    ga = F.conv2d(aa, o["wg"].abs(), o["bg"].abs(), padding=1)
    ba = F.conv2d(aa, o["wb"].abs(), o["bb"].abs(), padding=1)
    check_exact(name + " h", 2 * (xhat.abs().float() * (1 + ga) + ba))      # x 2: multiples of 1/2
    share = check_forward(name + " h", h, dt)
    dpre = nchw(o["gh"]) * act_grad(pre.detach(), act)
    dgam = dpre * xhat
    for nm, t in (("dgamma", dgam), ("dbeta", dpre)):
        assert torch.equal(t, t.to(DT[dt]).double()), f"{name}: {nm}, which the operator layer stores in {dt}, is not representable"
    grads = torch.autograd.grad(pre, leaves, dpre)
    aq = aa.clone().requires_grad_()
    wq = [o[n].abs().requires_grad_() for n in ("wg", "wb")]
    bound = torch.autograd.grad(F.conv2d(aq, wq[0], None, padding=1) + F.conv2d(aq, wq[1], None, padding=1), [aq] + wq,
                                torch.maximum(dgam.abs(), dpre.abs()).float())
    out = {"h": nhwc(h), "dactv": nhwc(grads[0])}
    out.update(zip(("dwg", "dbg", "dwb", "dbb"), grads[1:]))
    for nm, t in zip(("dactv", "dwg", "dwb"), bound):
        check_exact(f"{name} {nm}", 8 * t)                                     # x 8: multiples of 1/8
    for nm in ("dactv", "dwg", "dbg", "dwb", "dbb"):
        check_distinct(f"{name} {nm}", out[nm])
    return out, share


def out_dtype(name, dt):
    """Weight and bias gradients are fp32; outputs, data gradients and residual gradients have the operand dtype."""
    return torch.float32 if name in ("dw", "db", "dwg", "dbg", "dwb", "dbb") else DT[dt]


def assert_bits(name, got, want_exact, dtype):
    """got has `dtype` and torch.equal(got, once-rounded reference) (every value identical; +0 and -0 compare equal); a failure
    reports how many elements differ and the first few of them."""
    got = got.detach().cpu()
    assert got.dtype == dtype, f"{name}: returned as {got.dtype}, expected {dtype}"
    want = want_exact.to(got.dtype)
    assert got.shape == want.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    if torch.equal(got, want):
        return
    bad = (got != want) | (got != got)
    idx = bad.nonzero()[:6].tolist()
    first = ", ".join(f"{tuple(i)}: got {got[tuple(i)].item()!r} want {want[tuple(i)].item()!r}" for i in idx)
    raise AssertionError(f"{name}: {int(bad.sum())} of {got.numel()} elements differ from the once-rounded exact value; first: {first}")


# ---------------------------------------------------------------------------------------------------------------------
# the operator-layer calls both test files make (on whichever backend is installed)
# ---------------------------------------------------------------------------------------------------------------------
def run_conv(ops_, k, s, p, act="none", dev="cpu", with_grads=True, bias=True, resid=True):
    """ops.conv2d(+ bias, + residual, + act at slope 0.25) and its autograd gradients: dict like conv_reference's.
    bias / resid = False: leave out what the operand set carries; bias = a tensor: use it in place of the operand set's."""
    from michigan_amd import ops
    code = {"none": ops.ACT_NONE, "relu": ops.ACT_RELU, "lrelu": ops.ACT_LRELU}[act]
    ops_ = dict(ops_, b=ops_["b"] if bias is True else (None if bias is False else bias), r=ops_["r"] if resid else None)
    t = {n: (v.detach().to(dev) if v is not None else None) for n, v in ops_.items()}
    leaves = {n: t[n].requires_grad_(with_grads) for n in ("x", "w", "b", "r") if t[n] is not None}
    y = ops.conv2d(t["x"], t["w"], t["b"], stride=s, padding=p, act=code, slope=SLOPE, resid=t["r"])
    out = {"y": y.detach()}
    if with_grads:
        grads = torch.autograd.grad(y, list(leaves.values()), t["gy"])
        out.update(zip(({"x": "dx", "w": "dw", "b": "db", "r": "dres"}[n] for n in leaves), grads))
    return {n: v.cpu() for n, v in out.items()}


def run_wgrad(ops_, k, s, p, want_bias, dev="cpu"):
    from michigan_amd import ops
    res = ops.conv_wgrad(ops_["x"].to(dev), ops_["dy"].to(dev), k, k, s, p, want_bias=want_bias)
    return {"dw": res[0].cpu(), "db": res[1].cpu()} if want_bias else {"dw": res.cpu()}


def run_spade(ops_, act="lrelu", up=False, dev="cpu"):
    """ops.spade_modulate with the caller's mean / rstd (`up`: through spade_modulate_pair's folded upsample, both branches given
    the same operands, the first with the activation): h and the gradients with respect to actv, weights and biases."""
    from michigan_amd import ops
    code = {"none": ops.ACT_NONE, "lrelu": ops.ACT_LRELU}[act]
    t = {n: v.detach().to(dev) for n, v in ops_.items()}
    names = ("actv", "wg", "bg", "wb", "bb")
    leaves = [t[n].requires_grad_() for n in names]
    x = t["x"].requires_grad_()
    count = float(t["actv"].numel() // t["actv"].shape[3])
    if up:
        assert ops.spade_pair_supported(x)
        twin = [v.detach().clone().requires_grad_() for v in leaves]
        h, h1 = ops.spade_modulate_pair(x, (tuple(leaves), tuple(twin)), t["mean"], t["rstd"], count, acts=(code, ops.ACT_NONE), slope=SLOPE, up=True)
        grads = torch.autograd.grad([h, h1], leaves, [t["gh"], torch.zeros_like(t["gh"])])
    else:
        h = ops.spade_modulate(x, *leaves, t["mean"], t["rstd"], count, act=code, slope=SLOPE)
        grads = torch.autograd.grad(h, leaves, t["gh"])
    out = {"h": h.detach()}
    out.update(zip(("dactv", "dwg", "dbg", "dwb", "dbb"), grads))
    return {n: v.cpu() for n, v in out.items()}
