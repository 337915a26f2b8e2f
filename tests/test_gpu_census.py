"""-m gpu: every reduction outside the convolutions counts each element exactly once.

tests/test_gpu_exact_sums.py holds the convolution family to one rounding; what reduces elsewhere was judged by |hip - ref| <= tol * max|ref|,
which a lost or doubled element of a sum over a few thousand pixels passes.  Here the operands (tests/census_operands.py) are small nonzero
integers times powers of two: every sum is exact in fp32 in any order, so sums, the elementwise outputs built from them and the drained
gradients must satisfy ``torch.equal(hip, float64_reference.to(dtype))``.  The ONE tolerance of this file is 1 fp32 ulp on quotients by a
count that is no power of two (mean / rstd / running statistics of a finalize, the loss means, masked_mean_fill), whose exact numerator is
held at or below 2^20 units so that one element moves them by 8 ulp or more.

  1  channel statistics       mg_channel_stats (shift off / on), mg_channel_stats_finalize (sum_scale 1 and 4, running statistics at G = 1)
  2  norm backward reduce     mg_norm_bwd_reduce, mg_norm_bwd_reduce_up: act none / relu / lrelu x h x g1 x dgb, OPT_NORM_BWD_VEC on and off
  3  norm apply and forward   mg_norm_bwd_apply, mg_norm_bwd_apply2 (one / two branches, with and without `up`), mg_norm_act_fwd, and
                              ops.spade_modulate end to end with x.requires_grad (the gradient test_gpu_exact_sums.py leaves out)
  4  scalar losses            mg_l1_mean_fwd, mg_hinge_fwd, mg_color_loss_fwd (rgb, background), mg_hair_lab_fwd (background),
                              mg_orient_loss_fwd, mg_masked_mean_fill
  5  gradient sink drain      mg_grad_drain through FlatAdam(grad_sink=True).sync_grads(): plain, fused gamma|beta and spectral-normed slots

C in {4, 24, 48, 64, 136, 1024, 2048, 4096} and P in {1, 2, 15, 16, 17, 255, 256, 257, 511, 513, 4099} straddle every tail of stat_geom,
pix_grid, PIX and rows; the kernel a case reaches is derived from the dispatch predicates (``norm_path``) and the coverage asserted when
this module is imported.  Preconditions are asserted on the reference before a kernel's result is looked at.  MG_TEST_DRYRUN=1 runs the
contract emulator in place of the GPU; tests/test_census_operands.py runs the ``*_case`` functions below that way on a thinned list.
"""
import os

import pytest
import torch

import census_operands as Z
import exact_operands as X

pytestmark = pytest.mark.gpu

DRY = os.environ.get("MG_TEST_DRYRUN") == "1"
DEV = "cpu" if DRY else "cuda"
ACT = {"none": 0, "relu": 1, "lrelu": 2}


def install_emulator():
    """The contract emulator (oracle/cabi_emulator.py); returns the backend it replaced."""
    from michigan_amd import _cabi
    from oracle.cabi_emulator import EmulatorBackend
    return _cabi.set_backend(EmulatorBackend())


@pytest.fixture
def backend(request):
    if not DRY:
        yield request.getfixturevalue("hip_backend")
        return
    request.getfixturevalue("emulator_backend")
    from michigan_amd import _cabi
    prev = install_emulator()
    yield
    _cabi.set_backend(prev)


class _Report:
    """Collects every mismatch of a case, so that one run names them all."""

    def __init__(self):
        self.failures, self.compared = [], 0

    def check(self, tag, got, want):
        assert set(got) == set(want), (tag, sorted(got), sorted(want))
        for n, entry in want.items():
            self.compared += 1
            try:
                Z.check_one(f"{tag} {n}", got[n], entry)
            except AssertionError as e:
                self.failures.append(str(e))

    def done(self):
        assert not self.failures, "\n".join(self.failures[:40]) + f"\n({len(self.failures)} mismatches)"


def rejects(got_exact, want):
    """True when the comparison of this file rejects `got_exact` (a mutated reference, rounded as a kernel would store it)."""
    rep = _Report()
    rep.check("mutant", {n: e[0].to(e[1]) for n, e in got_exact.items()}, want)
    return bool(rep.failures)


# =====================================================================================================================
# which kernel a geometry reaches (mg_norm.hip: vec_geom_ok, stat_geom)
# =====================================================================================================================
def norm_path(dt, C, vec_opt=True):
    vec = 8 if dt == "bf16" else 4
    if vec_opt and C % vec == 0 and C // vec <= 256 and 256 % (C // vec) == 0:
        return f"vec-rows{256 // (C // vec)}"
    c4 = C // 4
    tpr = min(c4, 256)
    return f"quad-tpr{tpr}-trips{-(-c4 // tpr)}"


PATHS = {dt: {C: norm_path(dt, C) for C in Z.C_LIST} for dt in ("f32", "bf16")}
for _dt in ("f32", "bf16"):
    _p = set(PATHS[_dt].values())
    assert {"vec-rows1", "vec-rows2" if _dt == "bf16" else "vec-rows16"} <= _p, _p
    assert any(q.startswith("quad-tpr") and not q.startswith("quad-tpr256") for q in _p) and "quad-tpr256-trips4" in _p, _p
assert PATHS["bf16"][64] == "vec-rows32" and PATHS["f32"][4] == "vec-rows256" and PATHS["f32"][2048] == "quad-tpr256-trips2"
VEC_C = {dt: [C for C in Z.C_LIST if PATHS[dt][C].startswith("vec")] for dt in ("f32", "bf16")}


def _dev(o, dev, names):
    return {n: (o[n].to(dev) if o.get(n) is not None else None) for n in names}


def _be():
    from michigan_amd import _cabi
    return _cabi.backend()


def _ws(G, P, C, dev):
    return torch.empty(max(int(_be().mg_stats_workspace(G, P, C)), 4), dtype=torch.uint8, device=dev)


# =====================================================================================================================
# 1  channel statistics
# =====================================================================================================================
def stats_case(rep, dt, G, P, C, dev):
    from michigan_amd import ops
    tag = f"stats {dt} G={G} P={P} C={C} [{PATHS[dt][C]}]"
    for pivot in (False, True):
        o = Z.stats_operands(dt, G, P, C, pivot)
        Z.stats_check(o, tag)
        x = o["x"].to(dev)
        rep.check(f"{tag} shift={int(pivot)}", {"sums": ops.channel_sums(x, groups=G, shift=pivot).cpu()}, Z.stats_reference(o, name=tag))
        if not pivot:
            continue                                       # mg_channel_stats_finalize always shifts: the pivot operands
        for scale in (1.0, 4.0):
            count = float(P) * scale
            run0 = Z.running_init(C) if G == 1 else None
            rm, rv = (run0[0].clone().to(dev), run0[1].clone().to(dev)) if G == 1 else (None, None)
            mean, rstd, sums = ops.stats_finalize(x, G, count, Z.EPS, Z.MOMENTUM if G == 1 else 0.0, rm, rv, scale)
            got = {"sums": sums.cpu(), "mean": mean.cpu(), "rstd": rstd.cpu()}
            if G == 1:
                got.update(running_mean=rm.cpu(), running_var=rv.cpu())
            rep.check(f"{tag} finalize x{scale:g}", got, Z.stats_reference(o, scale, count, run0, name=tag))


@pytest.mark.parametrize("C", Z.C_LIST)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_channel_statistics_count_every_element(backend, dt, C):
    rep = _Report()
    for P in Z.p_list(C):
        for G in (1, 3):
            stats_case(rep, dt, G, P, C, DEV)
    print(f"[census] group 1 {dt} C={C} {PATHS[dt][C]}: {rep.compared} results compared")
    rep.done()


# =====================================================================================================================
# 2  norm backward reduce
# =====================================================================================================================
# (act, h given, g1 given, dgb asked): h = None is legal with act none only
REDUCE_VARIANTS = [(a, h, g1, dgb) for a, h in (("none", False), ("none", True), ("relu", True), ("lrelu", True)) for g1 in (False, True) for dgb in (False, True)]
UP_SHAPES = [(1, 2, 2), (2, 6, 10), (1, 18, 30)]      # even H, W; 10 and 30 are no multiple of any rows > 2


def run_reduce(o, act, use_h, use_g1, want_dgb, dt, dev):
    from michigan_amd import ops
    G, P, C = o["dh"].shape
    t = _dev(o, dev, ("dh", "h", "g1", "x", "xs", "mean", "rstd"))
    sums = torch.full((G, 2, C), float("nan"), dtype=torch.float32, device=dev)
    dgb = torch.zeros((P, 2 * ops._roundup(C, 32)), dtype=X.DT[dt], device=dev) if want_dgb else None     # the padded rows must stay zero
    hp, gp = (ops._p(t["h"]) if use_h else None), (ops._p(t["g1"]) if use_g1 else None)
    if o["up"] is not None:
        n, hh, ww = o["up"]
        _be().mg_norm_bwd_reduce_up(ops._p(t["dh"]), hp, ops._p(t["xs"]), gp, ops._dt(t["dh"]), n, hh, ww, C, ops._p(t["mean"]), ops._p(t["rstd"]),
                                    ACT[act], X.SLOPE, ops._p(dgb), ops._p(sums), ops._p(_ws(1, P, C, dev)), ops._stream(t["dh"]))
    else:
        _be().mg_norm_bwd_reduce(ops._p(t["dh"]), hp, ops._p(t["x"]), gp, ops._dt(t["dh"]), G, P, C, ops._p(t["mean"]), ops._p(t["rstd"]),
                                 ACT[act], X.SLOPE, ops._p(dgb), ops._p(sums), ops._p(_ws(G, P, C, dev)), ops._stream(t["dh"]))
    out = {"sums": sums.cpu()}
    if want_dgb:
        out["dgb"] = dgb.cpu()
    return out


def reduce_case(rep, dt, G, P, C, variants, dev, up=None):
    from michigan_amd import _cabi
    o = Z.bwd_operands(dt, G, P, C, up=up)
    for act, use_h, use_g1, want_dgb in variants:
        if want_dgb and G != 1:
            continue
        tag = f"reduce {dt} G={G} P={P} C={C} up={up} act={act} h={int(use_h)} g1={int(use_g1)} dgb={int(want_dgb)}"
        ref = Z.bwd_reduce_reference(o, act, use_g1, want_dgb, dt, name=tag)
        for vec in ((1, 0) if PATHS[dt][C].startswith("vec") else (1,)):          # a vec-capable C: both kernels must equal the reference
            with _cabi.options({_cabi.OPT_NORM_BWD_VEC: vec}):
                rep.check(f"{tag} [{norm_path(dt, C, bool(vec))}]", run_reduce(o, act, use_h, use_g1, want_dgb, dt, dev), ref)


def reduce_variants(C, P):
    """The full cross where it is cheap and at one P on either side of 256 for the wide C; elsewhere the two variants that differ in everything."""
    if C < 1024 or P in (17, 257):
        return REDUCE_VARIANTS
    return [("lrelu", True, True, True), ("none", False, False, False)]


@pytest.mark.parametrize("C", Z.C_LIST)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_norm_backward_reduce_counts_every_element(backend, dt, C):
    rep = _Report()
    for P in Z.p_list(C):
        reduce_case(rep, dt, 1, P, C, reduce_variants(C, P), DEV)
        reduce_case(rep, dt, 3, P, C, [v for v in reduce_variants(C, P) if not v[3]], DEV)
    print(f"[census] group 2 {dt} C={C} {PATHS[dt][C]} / {norm_path(dt, C, False)}: {rep.compared} results compared")
    rep.done()


@pytest.mark.parametrize("C", (24, 48, 64, 136, 1024))
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_norm_backward_reduce_through_the_folded_upsample(backend, dt, C):
    rep = _Report()
    for n, hh, ww in UP_SHAPES:
        reduce_case(rep, dt, 1, n * hh * ww, C, [("lrelu", True, True, True), ("none", False, False, False), ("relu", True, True, False), ("none", True, False, True)],
                    DEV, up=(n, hh, ww))
    print(f"[census] group 2 up {dt} C={C}: {rep.compared} results compared")
    rep.done()


# =====================================================================================================================
# 3  norm apply and forward
# =====================================================================================================================
APPLY_VARIANTS = [("none", False, False), ("none", True, True), ("relu", True, True), ("lrelu", True, False), ("lrelu", True, True)]


def run_apply(o, act, use_h, use_g1, dev):
    from michigan_amd import ops
    G, P, C = o["dh"].shape
    t = _dev(o, dev, ("dh", "h", "g1", "x", "mean", "rstd", "s"))
    dx = torch.empty_like(t["x"])
    _be().mg_norm_bwd_apply(ops._p(t["dh"]), ops._p(t["h"]) if use_h else None, ops._p(t["x"]), ops._p(t["g1"]) if use_g1 else None, ops._dt(t["x"]), G, P, C,
                            ops._p(t["mean"]), ops._p(t["rstd"]), ops._p(t["s"][0, :C]), ops._p(t["s"][0, C:]), o["gstride"], o["scale"], ACT[act], X.SLOPE,
                            ops._p(dx), ops._stream(dx))
    return {"dx": dx.cpu()}


def run_fwd(o, act, use_resid, dev):
    from michigan_amd import ops
    G, P, C = o["x"].shape
    t = _dev(o, dev, ("x", "resid", "mean", "rstd"))
    y = torch.empty_like(t["x"])
    _be().mg_norm_act_fwd(ops._p(t["x"]), ops._p(y), ops._dt(y), G, P, C, ops._p(t["mean"]), ops._p(t["rstd"]), ACT[act], X.SLOPE,
                          ops._p(t["resid"]) if use_resid else None, ops._stream(y))
    return {"y": y.cpu()}


def _thin(variants, C, P):
    """Every variant where it is cheap and at one P on either side of 256 for the wide C; elsewhere the first and the last, which differ in everything."""
    return variants if (C < 1024 or P in (17, 257)) else [variants[0], variants[-1]]


FWD_VARIANTS = [("none", False), ("relu", True), ("lrelu", False), ("lrelu", True)]


def apply_case(rep, dt, G, P, C, dev):
    o = Z.apply_operands(dt, G, P, C)
    for act, use_h, use_g1 in _thin(APPLY_VARIANTS, C, P):
        tag = f"apply {dt} G={G} P={P} C={C} act={act} h={int(use_h)} g1={int(use_g1)} [{PATHS[dt][C]}]"
        rep.check(tag, run_apply(o, act, use_h, use_g1, dev), Z.apply_reference(o, act, use_g1, dt, name=tag))


def fwd_case(rep, dt, G, P, C, dev):
    o = Z.fwd_operands(dt, G, P, C)
    for act, use_resid in _thin(FWD_VARIANTS, C, P):
        tag = f"fwd {dt} G={G} P={P} C={C} act={act} resid={int(use_resid)} [{PATHS[dt][C]}]"
        rep.check(tag, run_fwd(o, act, use_resid, dev), Z.fwd_reference(o, act, use_resid, dt, name=tag))


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("C", Z.C_LIST)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_norm_apply_and_forward_round_once(backend, dt, C, G):
    rep = _Report()
    for P in Z.p_list(C):
        apply_case(rep, dt, G, P, C, DEV)
        fwd_case(rep, dt, G, P, C, DEV)
    print(f"[census] group 3 {dt} C={C} G={G} {PATHS[dt][C]}: {rep.compared} results compared")
    rep.done()


def run_apply2(o, acts, dev):
    from michigan_amd import _cabi, ops
    _, P, C = o["dh"].shape
    keep = []
    d = _cabi.NormApply2Desc()
    for b, br in enumerate([o] + ([o["b"]] if "b" in o else [])):
        t = _dev(br, dev, ("dh", "h", "g1"))
        s = o["sums"][b].to(dev)
        keep += [t, s]
        d.dh[b], d.g1[b], d.sums[b] = t["dh"].data_ptr(), t["g1"].data_ptr(), s.data_ptr()
        d.h[b] = t["h"].data_ptr() if acts[b] != "none" else None
        d.act[b], d.slope[b] = ACT[acts[b]], X.SLOPE
    x = (o["xs"] if o["up"] is not None else o["x"][0]).to(dev)
    mean, rstd = o["mean"][0].to(dev), o["rstd"][0].to(dev)
    dx = torch.empty_like(x)
    d.x, d.mean, d.rstd, d.dx = x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx.data_ptr()
    d.P, d.dtype, d.C, d.inv_count = P, ops._dt(x), C, o["inv_count"]
    d.up, d.H, d.W = (1, o["up"][1], o["up"][2]) if o["up"] is not None else (0, 0, 0)
    _be().mg_norm_bwd_apply2(d, ops._stream(x))
    return {"dx": dx.cpu()}


def apply2_case(rep, dt, C, dev, shapes=None):
    for two in (False, True):
        for up in (shapes or ([None] + UP_SHAPES)):
            for P in ((1, 17, 257, 513) if up is None else (up[0] * up[1] * up[2],)):
                o = Z.apply2_operands(dt, P, C, two, up=up)
                for acts in (("lrelu", "none"), ("none", "relu")):
                    tag = f"apply2 {dt} P={P} C={C} two={int(two)} up={up} acts={acts}"
                    rep.check(tag, run_apply2(o, acts, dev), Z.apply2_reference(o, acts, dt, name=tag))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_norm_apply2_rounds_once(backend, dt):
    rep = _Report()
    for C in VEC_C[dt]:                                  # mg_norm_apply2_supported: the vec geometries
        assert _be().mg_norm_apply2_supported(0 if dt == "f32" else 1, C)
        apply2_case(rep, dt, C, DEV)
    print(f"[census] group 3 apply2 {dt} C={VEC_C[dt]}: {rep.compared} results compared")
    rep.done()


def spade_dx_case(rep, dt, dev, C=64, H=20, W=24, N=2, k=10):
    """ops.spade_modulate with x.requires_grad and count = 2^k: dx against a reference that uses (1 + gamma).to(dt), the stored form."""
    import torch.nn.functional as F
    from michigan_amd import ops
    o = X.spade_operands(dt, C, H, W, N=N)
    g = X._gen(77)
    o["wg"] = X.sparse_signs(g, o["wg"].shape, 64.0 / (o["wg"].shape[1] * 9))           # no +-512 pair: 1 + gamma stays representable
    count = float(2 ** k)
    a = X.nchw(o["actv"])
    gam = F.conv2d(a, o["wg"].double(), o["bg"].double(), padding=1)
    bet = F.conv2d(a, o["wb"].double(), o["bb"].double(), padding=1)
    g1 = 1 + gam
    assert torch.equal(g1, g1.to(X.DT[dt]).double()), "1 + gamma is not representable in the operand dtype"
    r, mu = o["rstd"].double().view(1, -1, 1, 1), o["mean"].double().view(1, -1, 1, 1)
    xh = (X.nchw(o["x"]) - mu) * r
    pre = xh * g1 + bet
    dxh = X.nchw(o["gh"]) * X.act_grad(pre, "lrelu") * g1
    s1, s2 = dxh.sum((0, 2, 3), keepdim=True), (dxh * xh).sum((0, 2, 3), keepdim=True)
    X.check_exact("spade dx sums", 8 * torch.maximum(dxh.abs().sum((0, 2, 3)), (dxh * xh).abs().sum((0, 2, 3))))
    dx = r * (dxh - s1 / count - xh * s2 / count)
    X.check_exact("spade dx", r * (dxh.abs() + s1.abs() / count + (xh * s2).abs() / count) * 2.0 ** (k + 5))
    Z.distinct("spade dx", dx)
    t = {n: v.detach().to(dev) for n, v in o.items()}
    x = t["x"].requires_grad_()
    h = ops.spade_modulate(x, t["actv"], t["wg"], t["bg"], t["wb"], t["bb"], t["mean"], t["rstd"], count, act=ops.ACT_LRELU, slope=X.SLOPE)
    (got,) = torch.autograd.grad(h, x, t["gh"])
    rep.check(f"spade dx {dt} C={C} {H}x{W}", {"dx": got.cpu()}, {"dx": (X.nhwc(dx), X.DT[dt], "bits")})


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_spade_input_gradient_rounds_once(backend, dt):
    rep = _Report()
    spade_dx_case(rep, dt, DEV)
    rep.done()


# =====================================================================================================================
# 4  scalar losses
# =====================================================================================================================
def l1_case(rep, dt, q, dev):
    from michigan_amd import ops
    o = Z.l1_operands(dt, q)
    a, b = o["a"].to(dev), o["b"].to(dev)
    out, ws = torch.empty(1, dtype=torch.float32, device=dev), torch.empty(1024, dtype=torch.float32, device=dev)
    _be().mg_l1_mean_fwd(ops._p(a), ops._p(b), ops._dt(a), a.numel(), ops._p(out), ops._p(ws), ops._stream(a))
    rep.check(f"l1_mean {dt} numel={4 * q}", {"loss": out.cpu()}, Z.l1_reference(o))


def hinge_case(rep, dt, n, dev):
    from michigan_amd import ops
    o = Z.hinge_operands(dt, n)
    x, w = o["x"].to(dev), o["w"].to(dev)
    for mode in (0, 1, 2):
        for use_w in (False, True):
            out = torch.empty(1, dtype=torch.float32, device=dev)
            _be().mg_hinge_fwd(ops._p(x), ops._p(w) if use_w else None, ops._dt(x), n, mode, ops._p(out), ops._stream(x))
            rep.check(f"hinge {dt} n={n} mode={mode} weight={int(use_w)}", {"loss": out.cpu()}, Z.hinge_reference(o, mode, use_w))


def image_case(rep, dt, N, H, W, dev):
    from michigan_amd import ops
    o = Z.image_operands(dt, N, H, W)
    fake, real_buf, mask_buf = o["fake"].to(dev), o["real_buf"].to(dev), o["mask_buf"].to(dev)
    tag = f"{dt} N={N} {H}x{W}"
    for flags, name in ((2, "rgb"), (4, "background")):
        out, ws = torch.empty(3, dtype=torch.float32, device=dev), torch.empty(3 * 1024, dtype=torch.float32, device=dev)
        _be().mg_color_loss_fwd(ops._p(fake), ops._p(real_buf), real_buf.stride(0), ops._p(mask_buf) if flags & 4 else None, mask_buf.stride(0) if flags & 4 else 0,
                                ops._dt(fake), N, H, W, fake.shape[3], flags, ops._p(out), ops._p(ws), ops._stream(fake))
        rep.check(f"color_loss {tag}", {name: out[1 if flags == 2 else 2:][:1].cpu()}, Z.image_reference(o, flags == 4))
    out, ws = torch.empty(2, dtype=torch.float32, device=dev), torch.empty(7 * max(1024, N), dtype=torch.float32, device=dev)
    _be().mg_hair_lab_fwd(ops._p(fake), None, 0, None, 0, None, 0, ops._p(real_buf), real_buf.stride(0), ops._p(mask_buf), mask_buf.stride(0),
                          ops._dt(fake), N, H, W, fake.shape[3], 2, ops._p(out), None, ops._p(ws), ops._stream(fake))
    rep.check(f"hair_lab {tag}", {"background": out[1:].cpu()}, Z.image_reference(o, True))


def orient_case(rep, N, H, W, dev):
    from michigan_amd import ops
    o = Z.orient_operands(N, H, W)
    conf, idx, label, hair = o["conf"].to(dev), o["idx"].to(dev), o["label"].to(dev), o["hair_buf"].to(dev)
    out, ws = torch.empty(3, dtype=torch.float32, device=dev), torch.empty(3 * 1024, dtype=torch.float32, device=dev)
    _be().mg_orient_loss_fwd(ops._p(conf), ops._p(idx), ops._p(label), 2, label.stride(0), ops._p(hair), hair.stride(0), N, H * W, ops._p(out), ops._p(ws),
                             ops._stream(conf))
    rep.check(f"orient_loss N={N} {H}x{W}", {"orient": out[:1].cpu(), "hair_sum": out[2:].cpu()}, Z.orient_reference(o))


def run_fill(o, adjoint, dev):
    from michigan_amd import ops
    x, lref, ltag = o["x"].to(dev), o["lref"].to(dev), o["ltag"].to(dev)
    N, P, C = x.shape
    w_in, w_out, w_norm = (ltag, lref, lref) if adjoint else (lref, ltag, lref)
    out = torch.empty((N, P, C), dtype=torch.float32, device=dev)
    _be().mg_masked_mean_fill(ops._p(x), ops._p(w_in), ops._p(w_out), ops._p(w_norm), ops._dt(x), N, P, C, ops._p(out), ops._stream(x))
    return {"out": out.cpu()}


def fill_case(rep, dt, P, C, dev):
    for empty in (False, True):
        o = Z.fill_operands(dt, 3, P, C, empty)
        for adjoint in (False, True):
            rep.check(f"masked_mean_fill {dt} P={P} C={C} adjoint={int(adjoint)} empty={int(empty)}", run_fill(o, adjoint, dev), Z.fill_reference(o, adjoint))


L1_Q, HINGE_N, IMAGE_HW, FILL_P, FILL_C = (1, 255, 256, 257, 65537), (1, 1023, 1024, 1025, 4489), ((1, 1), (3, 5), (17, 16), (67, 35)), (1, 15, 16, 17, 256), (4, 60, 64, 68)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_scalar_losses_count_every_element(backend, dt):
    rep = _Report()
    for q in L1_Q:
        l1_case(rep, dt, q, DEV)
    for n in HINGE_N:
        hinge_case(rep, dt, n, DEV)
    for H, W in IMAGE_HW:
        for N in (1, 3):
            image_case(rep, dt, N, H, W, DEV)
            if dt == "f32":
                orient_case(rep, N, H, W, DEV)            # fp32 operands only
    for P in FILL_P:
        for C in FILL_C:
            fill_case(rep, dt, P, C, DEV)
    print(f"[census] group 4 {dt}: {rep.compared} results compared")
    rep.done()


# =====================================================================================================================
# 5  gradient sink drain
# =====================================================================================================================
def drain_case(rep, dev):
    """One FlatAdam(grad_sink=True) over bare layers; the GEMM arena and its bias rows written directly, flat_grad pre-filled with integers,
    ONE sync_grads().  No `swapped` slot: ops._Conv2dFn keeps the launches whose operand roles are exchanged on the autograd path."""
    import torch.nn as nn
    from michigan_amd import ops
    from michigan_amd.networks.layers import HipConv2d
    from michigan_amd.networks.normalization import SPADE
    from michigan_amd.networks.spectral import spectral_norm
    from michigan_amd.optim import FlatAdam
    torch.manual_seed(3)
    convs = [HipConv2d(cin, cout, k, bias=bias) for cin, cout, k, bias, _ in Z.DRAIN_LAYERS]
    layers = nn.ModuleList([spectral_norm(c) if sn else c for c, (*_g, sn) in zip(convs, Z.DRAIN_LAYERS)]
                           + [SPADE("spadesyncbatch3x3", C, 4) for C in Z.DRAIN_SPADE]).to(dev)
    opt = FlatAdam(layers.parameters(), lr=1e-3, grad_sink=True)
    prefill = X.ints(X._gen(4), (opt.flat_grad.numel(),), -8, 8)
    opt.flat_grad.copy_(prefill)
    want = prefill.double().clone()

    def expect(p, val):
        a, b = opt._span_of[id(p)]
        want[a:b] += val.reshape(-1)
        Z.distinct("drained gradient", want[a:b])           # (a spectral-normed slot's own alphabet is small: the integer pre-fill widens it)

    keep = []
    for i, (lay, (cin, cout, k, bias, sn)) in enumerate(zip(layers, Z.DRAIN_LAYERS)):
        taps, rows, cols = k * k, ops._roundup(cout, 8), ops._roundup(cin, 8)
        w = lay.weight_orig if sn else lay.weight
        if sn:
            gemm, st, val = Z.drain_sn(cout, cin, taps, rows, cols, seed=i)
            st = {n: v.to(dev) for n, v in st.items()}
            keep.append(st)
            slot = opt.grad_slot(w, None, lay.bias, None, taps, rows, cols, (st["w_sn"], st["u"], st["v"], st["sigma"]))
            expect(w, val)
        else:
            gemm, vals = Z.drain_plain(cout, cin, taps, rows, cols, seed=i)
            slot = opt.grad_slot(w, None, lay.bias, None, taps, rows, cols, None)
            expect(w, vals[0])
        assert slot is not None, (cin, cout, k)
        slot[1].copy_(gemm)
        if bias:
            db, bv = Z.drain_bias(cout, rows, seed=i)
            slot[2].copy_(db)
            expect(lay.bias, bv[0])
        opt.slot_written(slot[0])
    for j, C in enumerate(Z.DRAIN_SPADE):
        sp = layers[len(Z.DRAIN_LAYERS) + j]
        rows, cols = 2 * ops._roundup(C, 32), 128
        gemm, vals = Z.drain_plain(C, 128, 9, rows, cols, two=True, seed=50 + j)
        db, bv = Z.drain_bias(C, rows, two=True, seed=50 + j)
        slot = opt.grad_slot(sp.mlp_gamma.weight, sp.mlp_beta.weight, sp.mlp_gamma.bias, sp.mlp_beta.bias, 9, rows, cols, None)
        assert slot is not None, C
        slot[1].copy_(gemm)
        slot[2].copy_(db)
        for p, v in zip((sp.mlp_gamma.weight, sp.mlp_beta.weight, sp.mlp_gamma.bias, sp.mlp_beta.bias), vals + bv):
            expect(p, v)
        opt.slot_written(slot[0])
    X.check_exact("drain", want)
    opt.sync_grads()
    rep.check("drain", {"flat_grad": opt.flat_grad.cpu(), "arena": opt.gemm.cpu()},
              {"flat_grad": (want, torch.float32, "bits"), "arena": (torch.zeros(opt.gemm.numel(), dtype=torch.float64), torch.float32, "bits")})
    return opt, want


def test_gradient_sink_drain_places_every_element(backend):
    rep = _Report()
    drain_case(rep, DEV)
    print(f"[census] group 5: {len(Z.DRAIN_LAYERS)} conv slots ({sum(1 for l in Z.DRAIN_LAYERS if l[4])} spectral-normed), {len(Z.DRAIN_SPADE)} gamma|beta pairs in one drain")
    rep.done()
