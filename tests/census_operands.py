"""Operands for which every REDUCTION outside the convolutions has an exact, order-independent value: a census of the summed elements.

tests/exact_operands.py pins the convolution family; this file does the same for what reduces elsewhere -- the channel statistics, the
norm backward (reduce and apply), the scalar losses and the optimiser's gradient drain.  Every summed term is a small NONZERO integer
(or an integer times a power of two), every partial sum stays below 2^24 in units of its quantum, so fp32 accumulation is exact in any
order and a dropped, doubled or misplaced element moves the result by at least one unit: it cannot hide under a max-norm bound.

Recipe (plain torch, no GPU):
  values             nonzero integers; a ReLU / hair mask legitimately zeroes terms: at least half of the summed terms are nonzero and the
                     STRUCTURAL pixels (first, last, last of the first half, both sides of every P of P_LIST) are nonzero in every channel
  cancelling pair    +64 at the first and -64 at the last pixel of each group along the reduced axis (exact_operands.WG_BIG)
  scales             rstd in {1/2, 1, 2}; mean, 1 + gamma, dh integers in [-2, 2]; slope 0.25; every scale handed to a kernel a power of two
  exactness          sum over |terms| of the WHOLE reduced axis below 2^24 quanta (check_exact): independent of the kernel's chunking
  means              a quotient by a count that is no power of two is compared with fp32(float64 quotient) to 1 fp32 ulp (the kernels
                     multiply by a reciprocal or take a double sqrt); the exact numerator stays at or below 2^20 units (check_numerator), so
                     one element moves the result by at least 8 ulp and the ulp cannot hide a miscount

A reference returns {name: (exact float64 tensor, dtype the kernel stores, "bits" | "ulp")}.  Every reference takes `pw` (a weight per
reduced element) and `cw` (a weight per channel): None for the true value; MUTATIONS builds the weights of a kernel that drops the last
pixel, the last pixel of the first half or the last channel quad, or counts the first pixel twice -- tests/test_census_operands.py checks
that the comparison rejects each of them.
"""
import math

import torch

from exact_operands import DT, LIMIT, SLOPE, WG_BIG, _gen, act_grad, assert_bits, check_distinct, check_exact, ints, rounding_share

P_LIST = (1, 2, 15, 16, 17, 255, 256, 257, 511, 513, 4099)
C_LIST = (4, 24, 48, 64, 136, 1024, 2048, 4096)
S_MAX = float(2 ** 20)
EPS = 2.0 ** -17                     # exact in fp32
MOMENTUM = 0.5
ROUNDING_MIN_NUMEL = 256             # the 5 % rounding share is asked of outputs with at least this many elements (a 4-element case cannot promise it)
PAIR_MIN_P = 4                       # below it the pair would be all there is: it is planted where other elements remain on both sides


def p_list(C):
    """Cases with C >= 1024 use P <= 513."""
    return tuple(p for p in P_LIST if C < 1024 or p <= 513)


def nonzero_ints(g, shape, hi):
    """Integers in [-hi, hi] without 0."""
    t = ints(g, shape, 1, hi)
    return t * (ints(g, shape, 0, 1) * 2 - 1)


def structural_pixels(P):
    """First and last pixel, the last pixel of the first half, and both pixels on either side of every listed P."""
    s = {0, P - 1, max(P // 2 - 1, 0)}
    for q in P_LIST:
        s.update(i for i in (q - 1, q) if 0 <= i < P)
    return sorted(s)


def check_terms(name, terms, axis=1):
    """terms [G, P, C] (reduced over `axis`): at least half nonzero, every structural position nonzero."""
    nz = terms != 0
    share = float(nz.double().mean())
    assert share >= 0.5, f"{name}: only {share:.0%} of the summed terms are nonzero"
    idx = torch.tensor(structural_pixels(terms.shape[axis]))
    assert bool(nz.index_select(axis, idx).all()), f"{name}: a structural position holds a zero term"
    if axis == 1 and terms.dim() == 3:
        assert bool(nz[:, :, 0].any(1).all() and nz[:, :, -1].any(1).all())


def check_numerator(name, s, unit=1.0):
    m = float(s.abs().max()) / unit
    assert m <= S_MAX, f"{name}: the numerator reaches {m:.4g} units > 2^20 -- one fp32 ulp could hide an element"


def distinct(name, ref):
    """exact_operands.check_distinct on the flattened vector (its 1-d rule: a quarter of the entries, 100 at the most)."""
    return check_distinct(name, ref.reshape(-1)[:1 << 20])          # (the rule asks for 100 values at the most: a million entries show them)


def _ordered(t):
    i = t.contiguous().view(torch.int32).long()
    return torch.where(i < 0, -(i & 0x7FFFFFFF), i)


def assert_ulp1(name, got, want_exact):
    """got is fp32 and within ONE fp32 ulp of fp32(float64 reference): the rule for quotients by a count that is no power of two."""
    got = got.detach().cpu()
    assert got.dtype == torch.float32, f"{name}: returned as {got.dtype}, expected fp32"
    want = want_exact.to(torch.float32).reshape(got.shape)
    bad = ((_ordered(got) - _ordered(want)).abs() > 1) | (got != got)
    if bool(bad.any()):
        idx = bad.nonzero()[:6].tolist()
        first = ", ".join(f"{tuple(i)}: got {got[tuple(i)].item()!r} want {want[tuple(i)].item()!r}" for i in idx)
        raise AssertionError(f"{name}: {int(bad.sum())} of {got.numel()} values are more than 1 ulp from the fp32 of the exact quotient; first: {first}")


def check_one(name, got, entry):
    ref, dtype, rule = entry
    if rule == "bits":
        assert_bits(name, got, ref.reshape(got.shape), dtype)
    else:
        assert rule == "ulp", rule
        assert_ulp1(name, got, ref)


# ---------------------------------------------------------------------------------------------------------------------
# mutations: what a kernel that miscounts would return, stated on the reference
# ---------------------------------------------------------------------------------------------------------------------
def _pw(G, P, edit):
    w = torch.ones(G, P, 1, dtype=torch.float64)
    edit(w)
    return w


def mutations(G, P, C):
    """{name: (pw, cw)} for a reduction over P elements per group with C channels (C = 0: no channel axis)."""
    m = {"drop-last-pixel": (_pw(G, P, lambda w: w[:, P - 1].zero_()), None),
         "first-pixel-twice": (_pw(G, P, lambda w: w[:, 0].mul_(2)), None)}
    if P >= 4:
        m["drop-last-of-first-half"] = (_pw(G, P, lambda w: w[:, P // 2 - 1].zero_()), None)
    if C >= 8:
        cw = torch.ones(C, dtype=torch.float64)
        cw[C - 4:] = 0
        m["drop-last-quad"] = (None, cw)
    return m


def _w(pw, cw, G, P, C):
    w = torch.ones(G, P, C, dtype=torch.float64)
    if pw is not None:
        w = w * pw
    if cw is not None:
        w = w * cw
    return w


# ---------------------------------------------------------------------------------------------------------------------
# group 1: channel statistics
# ---------------------------------------------------------------------------------------------------------------------
def pair_weight(P, pivot):
    """64, as in wgrad_operands -- but with the first pixel as the pivot every shifted term carries the pair's +W, and 4099 * 64^2 alone
    exceeds 2^24: the whole-axis exactness bound then leaves room for 32 only (the largest power of two that fits)."""
    return 32.0 if (pivot and P > 3000) else WG_BIG


def stats_operands(dt, G, P, C, pivot):
    """x [G, P, C]: nonzero integers in [-60, 60] (around 192 in the pivot case, exact in bf16: spacing 1 in [128, 256]) with the pair."""
    g = _gen(31 * C + P + 7 * G + int(pivot))
    x = nonzero_ints(g, (G, P, C), 60)
    if P >= PAIR_MIN_P:
        w = pair_weight(P, pivot)
        x[:, 0], x[:, P - 1] = w, -w
    if pivot:
        x = x + 192
    return dict(x=x.to(DT[dt]), pivot=bool(pivot))


def stats_check(o, name):
    x = o["x"].double()
    G, P, C = x.shape
    assert torch.equal(x, x.round()) and bool((x != 0).all())
    check_terms(name, x)
    k = x[:, :1] if o["pivot"] else torch.zeros_like(x[:, :1])        # the kernel sums x - pivot in fp32 and un-shifts in fp64
    check_exact(name + " sum", (x - k).abs().sum(1))
    check_exact(name + " sum of squares", ((x - k) ** 2).sum(1))
    if o["pivot"] and P >= 511:
        assert float((x * x).sum(1).min()) >= LIMIT, f"{name}: the pivot does not matter here"


def stats_reference(o, sum_scale=1.0, count=None, running=None, pw=None, cw=None, name="stats"):
    """sums [G, 2, C] (fp64, bitwise); with `count`: mean, rstd (and the running statistics, G == 1) of a finalize by the quotient rule."""
    x = o["x"].double()
    G, P, C = x.shape
    w = _w(pw, cw, G, P, C)
    sums = torch.stack([(x * w).sum(1), (x * x * w).sum(1)], 1) * sum_scale
    out = {"sums": (sums, torch.float64, "bits")}
    if pw is None and cw is None:
        distinct(name + " sums", sums)
    if count is not None:
        m = sums[:, 0] / count
        var = (sums[:, 1] / count - m * m).clamp_min(0)
        if pw is None and cw is None:
            check_numerator(name + " mean", sums[:, 0], sum_scale)
            distinct(name + " mean", m)
            if P > 1:
                distinct(name + " rstd", var)          # P == 1: the variance is 0 in every channel by construction
        out["mean"] = (m, torch.float32, "ulp")
        out["rstd"] = ((var + EPS) ** -0.5, torch.float32, "ulp")
        if running is not None:
            rm0, rv0 = running
            unb = var[0] * (count / max(count - 1.0, 1.0))
            out["running_mean"] = ((1 - MOMENTUM) * rm0.double() + MOMENTUM * m[0].float().double(), torch.float32, "ulp")
            out["running_var"] = ((1 - MOMENTUM) * rv0.double() + MOMENTUM * unb.float().double(), torch.float32, "ulp")
    return out


def running_init(C):
    g = _gen(C)
    return ints(g, (C,), -3, 3), ints(g, (C,), 1, 4)


# ---------------------------------------------------------------------------------------------------------------------
# groups 2 and 3: norm backward (reduce, apply, apply2) and norm forward
# ---------------------------------------------------------------------------------------------------------------------
def upsample(xs):
    return xs.repeat_interleave(2, 1).repeat_interleave(2, 2)


def bwd_operands(dt, G, P, C, up=None, seed=0):
    """dh, h, g1, x [G, P, C], mean, rstd [G, C].  up = (N, H, W): G = 1, P = N H W and x is also given as its half-resolution source xs.
    dh, g1: nonzero integers in [-2, 2]; h: +-1, +-2, positive at 70 % of the elements and at every structural pixel; x = mean + d with d a
    nonzero integer in [-40, 40], so that xhat = d * rstd never vanishes; the pair: dh = +64 / -64 at the first / last pixel, where g1 = 1 and
    x agrees, so that both sums cancel it."""
    g = _gen(17 * C + P + 5 * G + seed)
    mean, rstd = ints(g, (G, C), -2, 2), 2.0 ** ints(g, (G, C), -1, 1)
    dh, g1 = nonzero_ints(g, (G, P, C), 2), nonzero_ints(g, (G, P, C), 2)
    h = ints(g, (G, P, C), 1, 2) * ((torch.rand((G, P, C), generator=g) < 0.7).float() * 2 - 1)
    h[:, structural_pixels(P)] = h[:, structural_pixels(P)].abs()
    o = {}
    if up is not None:
        n, hh, ww = up
        assert G == 1 and P == n * hh * ww and hh % 2 == 0 and ww % 2 == 0
        xs = nonzero_ints(g, (n, hh // 2, ww // 2, C), 40)
        xs[n - 1, -1, -1] = xs[0, 0, 0]
        xs = xs + mean.view(1, 1, 1, C)
        d = upsample(xs).reshape(1, P, C) - mean.view(1, 1, C)
        o["xs"] = xs.to(DT[dt])
    else:
        d = nonzero_ints(g, (G, P, C), 40)
        d[:, P - 1] = d[:, 0]
    x = d + mean.view(G, 1, C)
    if P >= PAIR_MIN_P:
        dh[:, 0], dh[:, P - 1] = WG_BIG, -WG_BIG
        g1[:, 0], g1[:, P - 1] = 1, 1
    o.update(dh=dh.to(DT[dt]), h=h.to(DT[dt]), g1=g1.to(DT[dt]), x=x.to(DT[dt]), mean=mean, rstd=rstd, up=up)
    for n_ in ("dh", "h", "g1", "x"):
        assert torch.equal(o[n_].double(), {"dh": dh, "h": h, "g1": g1, "x": x}[n_].double()), n_     # representable in dt
    return o


def _bwd_terms(o, act, use_g1, pw, cw):
    G, P, C = o["dh"].shape
    w = _w(pw, cw, G, P, C)
    dpre = o["dh"].double() * act_grad(o["h"].double(), act, SLOPE) * w
    xh = (o["x"].double() - o["mean"].double().view(G, 1, C)) * o["rstd"].double().view(G, 1, C)
    dxh = dpre * o["g1"].double() if use_g1 else dpre
    return dpre, xh, dxh


def gemm_rows(C):
    ch = torch.arange(C)
    return 64 * (ch // 32) + ch % 32


def bwd_reduce_reference(o, act, use_g1, want_dgb, dt, pw=None, cw=None, name="bwd"):
    """sums [G, 2, C] fp32 (sum dxhat, sum dxhat * xhat) and, G == 1, dgb [P, 2 roundup(C, 32)] in the operand dtype: bitwise."""
    G, P, C = o["dh"].shape
    dpre, xh, dxh = _bwd_terms(o, act, use_g1, pw, cw)
    sums = torch.stack([dxh.sum(1), (dxh * xh).sum(1)], 1)
    if pw is None and cw is None:
        check_terms(name + " dxhat", dxh)
        check_terms(name + " dxhat * xhat", dxh * xh)
        check_exact(name + " sum dxhat", 4 * dxh.abs().sum(1))                  # multiples of 1/4 under the slope
        check_exact(name + " sum dxhat * xhat", 8 * (dxh * xh).abs().sum(1))    # multiples of 1/8
        distinct(name + " sums", sums)
    out = {"sums": (sums, torch.float32, "bits")}
    if want_dgb:
        assert G == 1
        dgb = torch.zeros(P, 2 * ((C + 31) // 32) * 32, dtype=torch.float64)
        rg = gemm_rows(C)
        dgb[:, rg], dgb[:, rg + 32] = (dpre * xh)[0], dpre[0]
        if pw is None and cw is None:
            assert torch.equal(dgb, dgb.to(DT[dt]).double()), f"{name}: dgb, stored in {dt}, is not representable"
            distinct(name + " dgb", dgb[:, torch.cat([rg, rg + 32])])
        out["dgb"] = (dgb, DT[dt], "bits")
    return out


def apply_operands(dt, G, P, C, gstride_pad=8, k=3, seed=0):
    """bwd_operands plus GIVEN sums: s1, s2 nonzero integers in [-64, 64] at a group stride of 2 C + gstride_pad, scale 2^-k."""
    o = bwd_operands(dt, G, P, C, seed=seed + 1)
    g = _gen(C + P + seed)
    gs = 2 * C + gstride_pad
    o["s"] = torch.zeros(G, gs)
    o["s"][:, :2 * C] = nonzero_ints(g, (G, 2 * C), 64)
    o.update(gstride=gs, scale=2.0 ** -k, k=k)
    return o


def apply_reference(o, act, use_g1, dt, pw=None, cw=None, name="apply"):
    """dx = rstd * (dxhat - s1 * scale - xhat * s2 * scale), once rounded.  Every term is a multiple of 2^-(k + 5) (rstd^2 >= 1/4, xhat and the
    slope's 1/4 included) whose magnitudes sum to less than 2^24 of them: each fp32 operation of either kernel is exact."""
    G, P, C = o["dh"].shape
    _, xh, dxh = _bwd_terms(o, act, use_g1, pw, cw)
    r = o["rstd"].double().view(G, 1, C)
    s1 = o["s"][:, :C].double().view(G, 1, C) * o["scale"]
    s2 = o["s"][:, C:2 * C].double().view(G, 1, C) * o["scale"]
    dx = r * (dxh - s1 - xh * s2)
    if pw is None and cw is None:
        check_exact(name + " dx", (r * (dxh.abs() + s1.abs() + (xh * s2).abs())) * 2.0 ** (o["k"] + 5))
        distinct(name + " dx", dx)
        if dt == "bf16" and dx.numel() >= ROUNDING_MIN_NUMEL:
            assert rounding_share(dx) >= 0.05, f"{name}: only {rounding_share(dx):.1%} of dx need rounding in bf16"
    return {"dx": (dx, DT[dt], "bits")}


def apply2_operands(dt, P, C, two, up=None, k=4):
    """One or two branches (dh, h, g1, raw sums [2, C] each) over the same x; up = (N, H, W): x and dx at half resolution."""
    a = bwd_operands(dt, 1, P, C, up=up, seed=3)
    g = _gen(C + P + 11)
    a["sums"] = [nonzero_ints(g, (2, C), 64)]
    if two:
        b = bwd_operands(dt, 1, P, C, up=up, seed=4)
        a["b"] = b
        a["sums"].append(nonzero_ints(g, (2, C), 64))
    a.update(k=k, inv_count=2.0 ** -k)
    return a


def apply2_reference(o, acts, dt, pw=None, cw=None, name="apply2"):
    _, P, C = o["dh"].shape
    r, mean = o["rstd"].double().view(1, 1, C), o["mean"].double().view(1, 1, C)
    xh = (o["x"].double() - mean) * r
    total, bound = torch.zeros(1, P, C, dtype=torch.float64), torch.zeros(1, P, C, dtype=torch.float64)
    for b, br in enumerate([o] + ([o["b"]] if "b" in o else [])):
        _, _, dxh = _bwd_terms(dict(br, x=o["x"], mean=o["mean"], rstd=o["rstd"]), acts[b], True, pw, cw)
        s = o["sums"][b].double() * o["inv_count"]
        total += r * (dxh - s[0] - xh * s[1])
        bound += r * (dxh.abs() + s[0].abs() + (xh * s[1]).abs())
    if o["up"] is not None:
        n, hh, ww = o["up"]
        total = total.view(n, hh // 2, 2, ww // 2, 2, C).sum((2, 4))
        bound = bound.view(n, hh // 2, 2, ww // 2, 2, C).sum((2, 4))
    if pw is None and cw is None:
        check_exact(name + " dx", bound * 2.0 ** (o["k"] + 5))
        distinct(name + " dx", total)
        if dt == "bf16" and total.numel() >= ROUNDING_MIN_NUMEL:
            assert rounding_share(total) >= 0.05, f"{name}: only {rounding_share(total):.1%} of dx need rounding in bf16"
    return {"dx": (total, DT[dt], "bits")}


def fwd_operands(dt, G, P, C):
    """x = mean + d, d a nonzero integer in [-250, 250] (x exact in bf16); resid multiples of 1/8 in [-4, 4]."""
    g = _gen(3 * C + P + G)
    mean, rstd = ints(g, (G, C), -2, 2), 2.0 ** ints(g, (G, C), -1, 1)
    x = nonzero_ints(g, (G, P, C), 250) + mean.view(G, 1, C)
    return dict(x=x.to(DT[dt]), resid=(ints(g, (G, P, C), -32, 32) / 8).to(DT[dt]), mean=mean, rstd=rstd)


def fwd_reference(o, act, use_resid, dt, pw=None, cw=None, name="fwd"):
    x = o["x"].double()
    G, P, C = x.shape
    v = (x * _w(pw, cw, G, P, C) - o["mean"].double().view(G, 1, C)) * o["rstd"].double().view(G, 1, C)
    y = torch.where(v > 0, v, v * {"none": 1.0, "relu": 0.0, "lrelu": SLOPE}[act])
    if use_resid:
        y = y + o["resid"].double()
    if pw is None and cw is None:
        assert torch.equal(x, o["x"].to(DT[dt]).double())
        check_exact(name + " y", 8 * (v.abs() + 4))
        distinct(name + " y", y)
        if dt == "bf16" and y.numel() >= ROUNDING_MIN_NUMEL and use_resid:      # an 8-bit integer times powers of two is representable: only the residual sum is not
            assert rounding_share(y) >= 0.05, f"{name}: only {rounding_share(y):.1%} of y need rounding in bf16"
    return {"y": (y, DT[dt], "bits")}


# ---------------------------------------------------------------------------------------------------------------------
# group 4: scalar losses.  Every loss is sum(terms) / count; terms are multiples of `unit`
# ---------------------------------------------------------------------------------------------------------------------
def _mean_entry(name, terms, count, unit, pw, extra_exact=None):
    """terms [G, P]: the summed values; the mean by the quotient rule (bitwise when the count is a power of two)."""
    t = terms.double()
    if pw is not None:
        t = t * pw.reshape(t.shape[0], -1)
    else:
        check_terms(name, t.unsqueeze(2))
        check_exact(name, t.abs().sum() / unit)
        check_numerator(name, t.abs().sum(), unit)
    s = t.sum()
    pow2 = math.log2(count) == int(math.log2(count))
    return (s / count).reshape(1), torch.float32, ("bits" if pow2 else "ulp")


def l1_operands(dt, q):
    g = _gen(q)
    a = nonzero_ints(g, (1, 4 * q), 2)
    b = a + nonzero_ints(g, (1, 4 * q), 2)
    return dict(a=a.to(DT[dt]), b=b.to(DT[dt]))


def l1_reference(o, pw=None):
    t = (o["a"].double() - o["b"].double()).abs()
    return {"loss": _mean_entry("l1_mean", t, t.numel(), 1.0, pw)}


def hinge_operands(dt, n):
    """Logits: half-integers in [-3.5, 3.5] and integers other than +-1: on both sides of the kinks at +-1, never on them.  weight in {1, 2, 3}."""
    g = _gen(n + 1)
    x = nonzero_ints(g, (1, n), 7) / 2
    x = torch.where(x.abs() == 1, x * 3, x)
    sp = structural_pixels(n)
    x[:, sp] = (ints(g, (1, len(sp)), 0, 1) - 0.5)           # +-1/2: inside both kinks, so that no mode zeroes a structural term
    return dict(x=x.to(DT[dt]), w=ints(g, (1, n), 1, 3))


def hinge_reference(o, mode, use_w, pw=None):
    x = o["x"].double()
    f = x if mode == 0 else torch.clamp_max((x if mode == 1 else -x) - 1, 0)
    if use_w:
        f = f * o["w"].double()
    if pw is None:
        assert bool((x.abs() != 1).all())
    name = f"hinge mode {mode}"
    t = f.double() if pw is None else f * pw.reshape(1, -1)
    if pw is None:
        check_terms(name, f.unsqueeze(2))                    # min(. - 1, 0) legitimately zeroes one side of the kink: still half nonzero
        check_exact(name, f.abs().sum() * 2)
        check_numerator(name, f.abs().sum(), 0.5)
    n = x.numel()
    pow2 = n & (n - 1) == 0
    return {"loss": ((-t.sum() / n).reshape(1), torch.float32, "bits" if pow2 else "ulp")}


def image_operands(dt, N, H, W, C=4, pad=5):
    """fake NHWC in dt and real fp32 planes, multiples of 1/64 in [-1, 1] that differ at every element; back / hair masks in {0, 1}
    (0 at 30 %, 1 at the structural pixels); the planes sit at sample strides larger than H W."""
    g = _gen(N + 10 * H + W)
    fake = ints(g, (N, H, W, C), -64, 64)
    d = nonzero_ints(g, (N, H, W, 3), 32)
    real = fake[..., :3] + d
    real = torch.where(real.abs() > 64, fake[..., :3] - d, real)              # stays inside [-1, 1] and still differs
    mask = (torch.rand((N, H * W), generator=g) >= 0.3).float()
    mask[:, structural_pixels(H * W)] = 1
    hw = H * W
    real_buf = torch.zeros(N, 3 * hw + pad)
    real_buf[:, :3 * hw] = (real / 64).permute(0, 3, 1, 2).reshape(N, 3 * hw)
    mask_buf = torch.zeros(N, hw + pad)
    mask_buf[:, :hw] = mask
    o = dict(fake=(fake / 64).to(DT[dt]), real_buf=real_buf, mask_buf=mask_buf, N=N, H=H, W=W)
    assert torch.equal(o["fake"].double(), (fake / 64).double())
    return o


def image_real(o):
    N, H, W = o["N"], o["H"], o["W"]
    return o["real_buf"][:, :3 * H * W].view(N, 3, H, W)


def image_mask(o):
    N, H, W = o["N"], o["H"], o["W"]
    return o["mask_buf"][:, :H * W].view(N, H, W)


def image_reference(o, masked, pw=None):
    """mean |fake - real| (rgb) or mean |fake m - real m| (background) over N 3 H W: one term per pixel, the three channels added."""
    N, H, W = o["N"], o["H"], o["W"]
    diff = (o["fake"][..., :3].double() - image_real(o).permute(0, 2, 3, 1).double()).abs().sum(3).reshape(N, H * W)
    if masked:
        diff = diff * image_mask(o).reshape(N, H * W).double()
    name = "background" if masked else "rgb"
    return {name: _mean_entry(name, diff, 3 * N * H * W, 1.0 / 64, pw)}


def orient_operands(N, H, W, pad=3):
    """conf_raw = 0 and idx = 0: confidence = 1/2 and fake = (0, 1/2) exactly; label planes multiples of 1/64 other than 0 and 1/2; hair in {0, 1}."""
    g = _gen(H + W + N)
    hw = H * W
    lab = nonzero_ints(g, (N, 2, hw), 64)
    lab = torch.where(lab == 32, lab + 1, lab) / 64
    hair = (torch.rand((N, hw), generator=g) >= 0.3).float()
    hair[:, structural_pixels(hw)] = 1
    buf = torch.zeros(N, hw + pad)
    buf[:, :hw] = hair
    return dict(conf=torch.zeros(N, H, W), idx=torch.zeros(N, H, W, dtype=torch.uint8), label=lab.view(N, 2, H, W), hair_buf=buf, N=N, H=H, W=W)


def orient_hair(o):
    return o["hair_buf"][:, :o["H"] * o["W"]].view(o["N"], o["H"], o["W"])


def orient_reference(o, pw=None):
    N, hw = o["N"], o["H"] * o["W"]
    hv = orient_hair(o).reshape(N, hw).double()
    lab = o["label"].reshape(N, 2, hw).double()
    t = (0.0 * hv - lab[:, 0] * hv).abs() + (0.5 * hv - lab[:, 1] * hv).abs()
    hs = hv if pw is None else hv * pw.reshape(N, hw)
    if pw is None:
        check_exact("orient hair", hv.sum())
    return {"orient": _mean_entry("orient", t, 2 * N * hw, 1.0 / 64, pw), "hair_sum": (hs.sum().reshape(1), torch.float32, "bits")}


def fill_operands(dt, N, P, C, empty=False):
    """x nonzero integers in [-8, 8] with the pair; lref / ltag masks in {0, 1} (1 at the structural pixels; lref all 0 when `empty`)."""
    g = _gen(P + C)
    x = nonzero_ints(g, (N, P, C), 8)
    lref = (torch.rand((N, P), generator=g) >= 0.3).float()
    ltag = (torch.rand((N, P), generator=g) >= 0.3).float()
    lref[:, structural_pixels(P)], ltag[:, structural_pixels(P)] = 1, 1
    if P >= PAIR_MIN_P:
        x[:, 0], x[:, P - 1] = WG_BIG, -WG_BIG
    if empty:
        lref.zero_()
    return dict(x=x.to(DT[dt]), lref=lref, ltag=ltag, empty=empty)


def fill_reference(o, adjoint, pw=None, cw=None, name="masked_mean_fill"):
    """out[n, q, c] = w_out[n, q] * sum_p(x w_in) / max(sum_p w_norm, 1).  forward: w_in = w_norm = lref, w_out = ltag; adjoint: w_in = ltag,
    w_out = w_norm = lref."""
    x = o["x"].double()
    N, P, C = x.shape
    w_in, w_out, w_norm = ((o["ltag"], o["lref"], o["lref"]) if adjoint else (o["lref"], o["ltag"], o["lref"]))
    terms = x * w_in.double().view(N, P, 1)
    s = (terms * _w(pw, cw, N, P, C)).sum(1)
    area = w_norm.double().sum(1).clamp_min(1.0)
    if pw is None and cw is None and not o["empty"]:
        check_terms(name, terms)
        check_exact(name, terms.abs().sum(1))
        check_numerator(name, terms.abs().sum(1))
    out = (s / area.view(N, 1)).float().double().view(N, 1, C) * w_out.double().view(N, P, 1)      # the quotient is rounded to fp32, then masked
    return {"out": (out, torch.float32, "ulp")}


# ---------------------------------------------------------------------------------------------------------------------
# group 5: gradient sink drain
# ---------------------------------------------------------------------------------------------------------------------
# (cin, cout, kernel, bias, spectral norm)
DRAIN_LAYERS = [(3, 1, 7, True, False), (64, 3, 3, True, False), (65, 5, 4, False, False), (200, 130, 1, True, False), (64, 130, 3, False, False),
                (200, 3, 7, True, False), (3, 5, 4, True, True), (65, 130, 3, True, True), (200, 1, 1, False, True), (64, 5, 7, True, True)]
DRAIN_SPADE = (48, 136)           # fused gamma|beta pairs: 128 -> C, 3 x 3


def drain_plain(cout, cin, taps, rows, cols, two=False, seed=0):
    """A GEMM image [taps, rows, cols] whose live elements carry distinct ids 1 .. (below 2^22), the rest 0, and the reference-layout
    tensors [cout, cin, taps] it drains into (two: gamma and beta through the [32 | 32] row blocks)."""
    n = (2 if two else 1) * cout * cin * taps
    assert n < 2 ** 22
    ids = (torch.randperm(n, generator=_gen(seed + n)) + 1).float().view(-1, cout, cin, taps)       # distinct, in no order the layout knows
    gemm = torch.zeros(taps, rows, cols)
    co = torch.arange(cout)
    for which in range(ids.shape[0]):
        r = (gemm_rows(cout) + 32 * which) if two else co
        gemm[:, r, :cin] = ids[which].permute(2, 0, 1)
    return gemm, [ids[w].double() for w in range(ids.shape[0])]


def drain_bias(cout, rows, two=False, seed=0):
    g = _gen(seed + cout)
    vals = nonzero_ints(g, (2 if two else 1, cout), 100)
    db = torch.zeros(rows)
    for which in range(vals.shape[0]):
        db[(gemm_rows(cout) + 32 * which) if two else torch.arange(cout)] = vals[which]
    return db, [v.double() for v in vals]


def drain_sn(cout, cin, taps, rows, cols, seed=0):
    """Spectral-normed slot: g integers in [-4, 4] (nonzero), W_sn, u, v in {0, +-1, +-2}, sigma = 2^k; the exact drained value
    (g - s u[co] v[ci, t]) / sigma with s = sum(g W_sn) != 0."""
    gen = _gen(seed + cout * cin + taps)
    g = nonzero_ints(gen, (cout, cin, taps), 4)
    w_sn, u, v = ints(gen, (cout, cin, taps), -2, 2), ints(gen, (cout,), -2, 2), ints(gen, (cin * taps,), -2, 2)
    u[0], u[-1], v[0], v[-1] = 1, 2, 2, 1
    sigma = 2.0 ** float(ints(gen, (1,), -1, 2))
    s = float((g.double() * w_sn.double()).sum())
    if s == 0:
        w_sn[0, 0, 0] += 1 if g[0, 0, 0] > 0 else -1
        s = float((g.double() * w_sn.double()).sum())
    check_exact("drain s", (g * w_sn).abs().sum() * 4 + 16)             # s u v with |u v| <= 4, plus g
    gemm = torch.zeros(taps, rows, cols)
    gemm[:, :cout, :cin] = g.permute(2, 0, 1)
    val = (g.double() - s * u.double().view(-1, 1, 1) * v.double().view(1, cin, taps)) / sigma
    return gemm, dict(w_sn=w_sn, u=u, v=v, sigma=torch.tensor([sigma])), val


def swap_permutation(ref):
    """The drain with two elements of its permutation exchanged (the first and the last of the tensor)."""
    m = ref.clone().reshape(-1)
    m[0], m[-1] = ref.reshape(-1)[-1], ref.reshape(-1)[0]
    return m.reshape(ref.shape)
