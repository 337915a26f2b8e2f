"""-m gpu: the NHWC streaming kernels, the loss gradients and Adam, held to their arithmetic (tests/adjoint_operands.py).

The value tests of these kernels (test_resampling, test_blend_and_adam, test_reflect_pad_fwd_bwd, test_relu_tap_and_masked_maxpool_backward,
test_l1_mean_fused, test_hinge_loss_and_wide_edge_weight_fused and the guard-band cases of their form) compare a few shapes with the contract
emulator under |hip - ref| <= 2^-7 max|ref|: one bf16 ulp at the top of the range.  Here every reference is torch's own operator on float64
CPU tensors with torch autograd for the adjoints, and the comparison says yes or no to the bit.  Per entry point, the rule and the count
of fp32 roundings behind any delta (d = k 2^-24 sum|terms|; got in [rne(exact - d), rne(exact + d)] of the output dtype):

  mg_upsample2x_fwd, mg_reflect_pad_fwd,      rule 1: arbitrary finite operands with +-0 and subnormals; integer views equal
  mg_maxpool2_fwd
  mg_assemble_nhwc8                           rule 1 against planar.to(dtype) (one round-to-nearest-even store), the image channels copied,
                                              the pad channels +0
  mg_upsample2x_bwd (4 terms),                rule 2: integer operands of 8 significant bits, masks in {0, 1/4, 1/2, 1}, slope 1/4: the sums
  mg_reflect_pad_bwd (up to 9),               are exact in fp32 in any order, assert_bits; the factor at y == 0 is 0 (ReLU) / the slope (Leaky)
  mg_act_bwd, mg_grad_sum_act (g2 NULL and
  given; none / relu / lrelu), mg_blend_fwd,
  mg_blend_bwd (dbg only, dx only, both)
  mg_maxpool2_bwd (relu_input 0 and 1)        rule 3: ties in >= 20 % of the windows, first maximum in ATen's scan order, +0 elsewhere (odd
                                              last row / column included): integer views equal; and conv(relu) -> act_tap -> maxpool2 ->
                                              l1_mean beside a second l1_mean through ops with FUSE_RELU_MASK on and off: bit-identical
                                              dx and dw, in fp32 equal to the float64 autograd of the unfused expression
  mg_avgpool3s2_fwd                           rule 4: fp32 one quotient (window sum exact) -> 1 ulp, bits at the counts 1, 2, 4;
                                              bf16 interval, k = 10 (8 additions, reciprocal, product)
  mg_avgpool3s2_bwd                           rule 4: interval in both dtypes, k = 11 (4 x (reciprocal, product), 3 additions)
  mg_l1_mean_bwd                              rule 4: fp32 1 ulp (bits at a power-of-two numel); bf16 interval, k = 2 (1 / numel, x gscale)
  mg_hinge_bwd (3 modes, weight or none)      rule 4: fp32 without weight 1 ulp (bits at a power-of-two n); else interval, k = 2 (g / n, x weight);
                                              logits on both sides of the hinge, none on it (the kernel declares the tie unreproduced)
  mg_adam_step                                rule 5: one teacher-forced step against torch.optim.Adam(foreach=False) on float64; exp_avg at
                                              beta1 = 0 and a power-of-two grad_scale bit for bit; otherwise the interval with torch's rounding
                                              counts doubled: m 2 x 5, v 2 x 7, p from both through the denominator plus 2 x (4 on the update,
                                              1 on the final add) -- adjoint_operands.adam_reference states the three bounds

Shapes: N in {1, 3} x C in {4, 8, 12, 136} x (H, W) in {(2, 2), (2, 3), (3, 2), (7, 9), (8, 8), (16, 17)} (+ (1, 1), (1, 5), (5, 1) for
upsample and avg-pool); reflect pad P in {1, 3, min(H, W) - 1} on (2, 2), (4, 7), (9, 5), (8, 8); the flat kernels at 1, 255, 256, 257 quads
and one bf16 launch above 8192 x 256 quads; Adam at numel in {1, 3, 255, 256, 257, 4099, 8192 x 256 + 3}.  Preconditions (exactness, rounding
share, tie share, term floor against delta) are asserted on the reference before a kernel's result is read; a counting backend confirms
that every claimed entry point was reached.  MG_TEST_DRYRUN=1 runs the contract emulator in place of the GPU;
tests/test_adjoint_operands.py runs the ``*_case`` functions below that way on a thinned list and checks that the rules reject the mutants.
"""
import os

import pytest
import torch
import torch.nn.functional as F

import adjoint_operands as A
import exact_operands as X
import guard_alloc as GA
from census_operands import hinge_operands

pytestmark = pytest.mark.gpu

DRY = os.environ.get("MG_TEST_DRYRUN") == "1"
DEV = "cpu" if DRY else "cuda"
NAN = float("nan")


def install_emulator():
    """The contract emulator (oracle/cabi_emulator.py); returns the backend it replaced."""
    from michigan_amd import _cabi
    from oracle.cabi_emulator import EmulatorBackend
    return _cabi.set_backend(EmulatorBackend())


def install_counter():
    """Wrap the active backend in guard_alloc's call counter: (counter, the backend it replaced)."""
    from michigan_amd import _cabi
    cb = GA.CountingBackend(_cabi.backend())
    return cb, _cabi.set_backend(cb)


@pytest.fixture
def be(request):
    from michigan_amd import _cabi
    if DRY:
        request.getfixturevalue("emulator_backend")
        outer = install_emulator()
    else:
        request.getfixturevalue("hip_backend")
    cb, prev = install_counter()
    yield cb
    _cabi.set_backend(prev)
    if DRY:
        _cabi.set_backend(outer)


def reached(cb, entry_points):
    """An eager fallback is not coverage: every entry point a test claims was really called."""
    missing = [ep for ep in entry_points if cb.count(ep) == 0]
    assert not missing, f"entry points never called: {missing}; called: {sorted(set(cb.calls))}"


class _Report:
    """Collects every mismatch of a test, so that one run names them all."""

    def __init__(self):
        self.failures, self.compared = [], 0

    def check(self, tag, got, want):
        assert set(got) == set(want), (tag, sorted(got), sorted(want))
        for n, w in want.items():
            self.compared += 1
            try:
                A.check_one(f"{tag} {n}", got[n], w)
            except AssertionError as e:
                self.failures.append(str(e))

    def done(self):
        assert self.compared
        assert not self.failures, "\n".join(self.failures[:40]) + f"\n({len(self.failures)} of {self.compared} comparisons failed)"


def _to(t, dev):
    """A fresh copy on `dev` (on the CPU too: a test must never hand the reference's own tensor to a kernel)."""
    return t.detach().clone().to(dev)


def _backend():
    from michigan_amd import _cabi
    return _cabi.backend()


def _gtag(geom):
    return "x".join(map(str, geom))


# =====================================================================================================================
# geometry kernels
# =====================================================================================================================
def upsample_case(rep, dt, geom, dev):
    from michigan_amd import ops
    x = A.copy_operands(dt, geom)
    xd = _to(x, dev).requires_grad_()
    y = ops.upsample2x(xd)
    rep.check(f"upsample2x_fwd {dt} {_gtag(geom)}", {"y": y.detach().cpu()}, A.copy_reference("up", x))
    dy = A.up_bwd_operands(dt, geom)
    want = A.up_bwd_reference(dy, dt)
    (dx,) = torch.autograd.grad(y, xd, _to(dy, dev))
    rep.check(f"upsample2x_bwd {dt} {_gtag(geom)}", {"dx": dx.cpu()}, want)


def reflect_case(rep, dt, n, h, w, c, p, dev):
    from michigan_amd import ops
    x = A.copy_operands(dt, (n, h, w, c), seed=p)
    xd = _to(x, dev).requires_grad_()
    y = ops.reflect_pad(xd, p)
    tag = f"{dt} {_gtag((n, h, w, c))} P={p}"
    rep.check(f"reflect_pad_fwd {tag}", {"y": y.detach().cpu()}, A.copy_reference("reflect", x, p))
    dy = A.reflect_bwd_operands(dt, n, h, w, c, p)
    want = A.reflect_bwd_reference(dy, p, dt)
    (dx,) = torch.autograd.grad(y, xd, _to(dy, dev))
    rep.check(f"reflect_pad_bwd {tag}", {"dx": dx.cpu()}, want)


def avgpool_case(rep, dt, geom, dev):
    from michigan_amd import ops
    o = A.avgpool_operands(dt, geom)
    want_y, want_dx = A.avgpool_fwd_reference(o), A.avgpool_bwd_reference(o)
    xd = _to(o["x"], dev).requires_grad_()
    y = ops.avgpool3s2(xd)
    (dx,) = torch.autograd.grad(y, xd, _to(o["dy"], dev))
    rep.check(f"avgpool3s2_fwd {dt} {_gtag(geom)}", {"y": y.detach().cpu()}, want_y)
    rep.check(f"avgpool3s2_bwd {dt} {_gtag(geom)}", {"dx": dx.cpu()}, want_dx)


def maxpool_case(rep, dt, geom, dev):
    """Forward through ops on raw values; the adjoint on hand-built buffers, where `relu_input` is an argument."""
    from michigan_amd import ops
    n, h, w, c = geom
    x = A.copy_operands(dt, geom, seed=1)
    with torch.no_grad():
        y = ops.maxpool2(_to(x, dev))
    rep.check(f"maxpool2_fwd {dt} {_gtag(geom)}", {"y": y.cpu()}, A.copy_reference("maxpool", x))
    o = A.maxpool_operands(dt, geom)
    for relu in (0, 1):
        want = A.maxpool_bwd_reference(o, relu)
        xin, dy = _to(A.maxpool_input(o, relu), dev), _to(o["dy"], dev)
        dx = torch.full_like(xin, NAN)
        _backend().mg_maxpool2_bwd(ops._p(dy), ops._p(xin), ops._p(dx), ops._dt(xin), n, h, w, c, relu, ops._stream(xin))
        rep.check(f"maxpool2_bwd {dt} {_gtag(geom)} relu_input={relu}", {"dx": dx.cpu()}, want)


ASSEMBLE_NHW = ((1, 1, 1), (3, 7, 9), (2, 16, 17))


def assemble_case(rep, dt, nhw, cp, cs, cf, dev):
    from michigan_amd import ops
    n, h, w = nhw
    o = A.assemble_operands(dt, n, h, w, cp, cs, cf)
    dst = torch.full((n + 1, h, w, 8), NAN, dtype=A.DT[dt], device=dev)          # the batch lands at an offset of one sample
    planar = _to(o["planar"], dev) if cp else None
    image = _to(o["image"], dev) if cf else None
    if cp:
        ops.assemble_nhwc8(dst, 1, planar, image, cf)
    else:                                                                           # the operator layer always has planar maps
        _backend().mg_assemble_nhwc8(None, 0, ops._p(image), cs, cf, ops._p(dst[1:]), ops._dt(dst), n, h * w, ops._stream(dst))
    rep.check(f"assemble_nhwc8 {dt} {_gtag(nhw)} cp={cp} cs={cs} cf={cf}", {"out": dst[1:].cpu()}, A.assemble_reference(o))
    assert bool(torch.isnan(dst[0].float()).all()), "mg_assemble_nhwc8 wrote outside its batch slice"


# =====================================================================================================================
# flat kernels
# =====================================================================================================================
ACT_CODE = {"none": 0, "relu": 1, "lrelu": 2}


def act_case(rep, dt, nq, dev, acts=("none", "relu", "lrelu")):
    from michigan_amd import ops
    o = A.act_operands(dt, nq)
    g1, g2 = _to(o["g1"], dev), _to(o["g2"], dev)
    n = 4 * nq
    for act in acts:
        y = _to(A.act_output(o, act), dev)
        if act != "none":
            got = ops.act_backward(g1, y, ACT_CODE[act], A.SLOPE)
            rep.check(f"act_bwd {dt} {act} n={n}", {"out": got.cpu()}, A.act_bwd_reference(o, act, False))
        for two in (False, True):
            want = A.act_bwd_reference(o, act, two)
            out = torch.full_like(g1, NAN)
            _backend().mg_grad_sum_act(ops._p(g1), ops._p(g2) if two else None, ops._p(y), ops._p(out), ops._dt(g1), n, ACT_CODE[act], A.SLOPE, ops._stream(g1))
            rep.check(f"grad_sum_act {dt} {act} g2={'given' if two else 'NULL'} n={n}", {"out": out.cpu()}, want)


def blend_case(rep, dt, P, C, dev, acts=("none", "lrelu"), needs_list=(("bg",), ("x",), ("bg", "x"))):
    from michigan_amd import ops
    o = A.blend_operands(dt, P, C)
    for act in acts:
        want = A.blend_reference(o, act)
        for needs in needs_list:
            bg = _to(o["bg"], dev).view(1, 1, P, C).requires_grad_("bg" in needs)
            x = _to(o["x"], dev).view(1, 1, P, C).requires_grad_("x" in needs)
            y = ops.blend(bg, x, _to(o["hair"], dev), _to(o["back"], dev), act=ACT_CODE[act], slope=A.SLOPE)
            grads = torch.autograd.grad(y, [t for t in (bg, x) if t.requires_grad], _to(o["dy"], dev).view(1, 1, P, C))
            got = {"y": y.detach().cpu().view(P, C)}
            got.update({{"bg": "dbg", "x": "dx"}[nm]: g.cpu().view(P, C) for nm, g in zip(needs, grads)})
            rep.check(f"blend {dt} {act} P={P} C={C} grads={'+'.join(needs)}", got, {k: want[k] for k in got})


def l1_case(rep, dt, nq, dev):
    from michigan_amd import ops
    o = A.l1_operands(dt, nq)
    want = A.l1_bwd_reference(o)
    a = _to(o["a"], dev).requires_grad_()
    (da,) = torch.autograd.grad(ops.l1_mean(a, _to(o["b"], dev)) * A.L1_GSCALE, a)
    rep.check(f"l1_mean_bwd {dt} numel={4 * nq}", {"da": da.cpu()}, want)


def hinge_case(rep, dt, n, dev):
    from michigan_amd import ops
    o = hinge_operands(dt, n)
    for mode in (0, 1, 2):
        for use_w in (False, True):
            want = A.hinge_bwd_reference(o, mode, use_w, dt)
            x = _to(o["x"], dev).requires_grad_()
            (dx,) = torch.autograd.grad(ops.hinge_loss(x, _to(o["w"], dev) if use_w else None, mode) * A.HINGE_GSCALE, x)
            rep.check(f"hinge_bwd {dt} n={n} mode={mode} weight={use_w}", {"dx": dx.cpu()}, want)


def adam_case(rep, numel, betas, scale, step, dev):
    from michigan_amd import ops
    o = A.adam_operands(numel, betas, scale, step)
    want = A.adam_reference(o)
    p, g, m, v = (o[k].clone().to(dev) for k in ("p", "g", "m", "v"))
    ops.adam_step(p, g, m, v, lr=o["lr"], beta1=betas[0], beta2=betas[1], eps=o["eps"], step=step, grad_scale=scale)
    assert torch.equal(g.cpu(), o["g"]), "mg_adam_step changed the gradient"
    rep.check(f"adam n={numel} betas={betas} scale={scale:.3g} step={step}", {"p": p.cpu(), "m": m.cpu(), "v": v.cpu()}, want)


# =====================================================================================================================
# conv(relu) -> act_tap -> maxpool2 -> l1_mean, the other tap into a second l1_mean
# =====================================================================================================================
CHAIN = dict(cin=8, cout=16, k=3, s=1, p=1, H=8, W=8, N=2)        # both L1 counts powers of two: every gradient is an integer


def chain_operands(dt):
    o = X.conv_operands(dt, bias=True, bias_lo=0, **CHAIN)
    g = X._gen(77)
    n, h, w, c = CHAIN["N"], CHAIN["H"], CHAIN["W"], CHAIN["cout"]
    o["t_tap"], o["t_pool"] = X.ints(g, (n, h, w, c), -2, 6).to(X.DT[dt]), X.ints(g, (n, h // 2, w // 2, c), -2, 6).to(X.DT[dt])
    return o


def chain_reference(o):
    """float64 autograd of the unfused expression; the convolution's exactness preconditions are ConvReference's."""
    X.ConvReference(o, 3, 1, 1, name="chain")
    xr, wr = X.nchw(o["x"]).requires_grad_(), o["w"].double().requires_grad_()
    a = F.relu(F.conv2d(xr, wr, o["b"].double(), padding=1))
    tt, tp = X.nchw(o["t_tap"]), X.nchw(o["t_pool"])
    loss = F.l1_loss(F.max_pool2d(a, 2), tp) * tp.numel() + F.l1_loss(a, tt) * tt.numel()
    dx, dw = torch.autograd.grad(loss, [xr, wr])
    assert float((a == 0).double().mean()) > 0.05 and A.tie_share(X.nhwc(a.detach())) >= 0.05
    X.check_distinct("chain dx", X.nhwc(dx))
    return {"dx": X.nhwc(dx), "dw": dw}


def chain_run(o, dev, fuse):
    from michigan_amd import ops
    saved, det = ops.FUSE_RELU_MASK, ops.set_deterministic(True)
    ops.FUSE_RELU_MASK = fuse
    try:
        ops.reset_mask_protocol()
        x, w = _to(o["x"], dev).requires_grad_(), _to(o["w"], dev).requires_grad_()
        a = ops.conv2d(x, w, _to(o["b"], dev), stride=1, padding=1, act=ops.ACT_RELU)
        a1, a2 = ops.act_tap(a)
        tp, tt = _to(o["t_pool"], dev), _to(o["t_tap"], dev)
        loss = ops.l1_mean(ops.maxpool2(a1), tp) * float(tp.numel()) + ops.l1_mean(a2, tt) * float(tt.numel())
        dx, dw = torch.autograd.grad(loss, [x, w])
        ops.wgrad_join()
        return {"dx": dx.cpu(), "dw": dw.cpu()}
    finally:
        ops.FUSE_RELU_MASK = saved
        ops.set_deterministic(det)


def chain_case(rep, dt, dev):
    o = chain_operands(dt)
    on, off = chain_run(o, dev, True), chain_run(o, dev, False)
    for n in ("dx", "dw"):
        rep.compared += 1
        if not torch.equal(on[n], off[n]):
            rep.failures.append(f"chain {dt} {n}: FUSE_RELU_MASK on and off differ in {int((on[n] != off[n]).sum())} elements")
    if dt == "f32":
        ref = chain_reference(o)
        rep.check("chain f32", on, {n: A.Want(ref[n], torch.float32, "bits") for n in ("dx", "dw")})


# =====================================================================================================================
# the tests
# =====================================================================================================================
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_upsample_copies_and_its_adjoint_sums_exactly(be, dt):
    rep = _Report()
    for geom in A.geoms(thin=True):
        upsample_case(rep, dt, geom, DEV)
    reached(be, ["mg_upsample2x_fwd", "mg_upsample2x_bwd"])
    rep.done()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_reflect_pad_copies_and_its_adjoint_sums_every_mirror(be, dt):
    rep = _Report()
    for h, w, p in A.REFLECT:
        for n in A.NS:
            for c in A.CS:
                reflect_case(rep, dt, n, h, w, c, p, DEV)
    reached(be, ["mg_reflect_pad_fwd", "mg_reflect_pad_bwd"])
    rep.done()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_avgpool_quotients_by_the_window_count(be, dt):
    rep = _Report()
    for geom in A.geoms(thin=True):
        avgpool_case(rep, dt, geom, DEV)
    reached(be, ["mg_avgpool3s2_fwd", "mg_avgpool3s2_bwd"])
    rep.done()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_maxpool_selects_and_routes_to_the_first_maximum(be, dt):
    rep = _Report()
    for geom in A.geoms():
        maxpool_case(rep, dt, geom, DEV)
    reached(be, ["mg_maxpool2_fwd", "mg_maxpool2_bwd"])
    rep.done()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_relu_tap_maxpool_l1_chain_is_the_unfused_gradient(be, dt):
    rep = _Report()
    chain_case(rep, dt, DEV)
    reached(be, ["mg_grad_sum_act", "mg_maxpool2_bwd", "mg_l1_mean_bwd", "mg_act_bwd"])
    rep.done()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_assemble_rounds_planar_once_and_pads_with_zero(be, dt):
    rep = _Report()
    for nhw in ASSEMBLE_NHW:
        for cp, cs, cf in A.ASSEMBLE:
            assemble_case(rep, dt, nhw, cp, cs, cf, DEV)
    reached(be, ["mg_assemble_nhwc8"])
    rep.done()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_activation_gradients_are_exact_and_fix_the_factor_at_zero(be, dt):
    rep = _Report()
    for nq in A.FLAT_QUADS:
        act_case(rep, dt, nq, DEV)
    reached(be, ["mg_act_bwd", "mg_grad_sum_act"])
    rep.done()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_blend_and_its_gradients_are_exact(be, dt):
    rep = _Report()
    for nq in A.FLAT_QUADS:
        blend_case(rep, dt, nq, 4, DEV)
    blend_case(rep, dt, 85, 12, DEV)
    blend_case(rep, dt, 3, 136, DEV)
    reached(be, ["mg_blend_fwd", "mg_blend_bwd"])
    rep.done()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_l1_gradient_divides_by_numel(be, dt):
    rep = _Report()
    for nq in A.FLAT_QUADS:
        l1_case(rep, dt, nq, DEV)
    reached(be, ["mg_l1_mean_bwd"])
    rep.done()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_hinge_gradient_in_three_modes_with_and_without_weight(be, dt):
    rep = _Report()
    for n in A.HINGE_N:
        hinge_case(rep, dt, n, DEV)
    reached(be, ["mg_hinge_bwd"])
    rep.done()


def test_flat_kernels_past_the_grid_stride_wrap_bf16(be):
    """One bf16 launch above 8192 x 256 quads per flat kernel: the second trip of the grid-stride loop."""
    rep = _Report()
    act_case(rep, "bf16", A.WRAP_QUADS, DEV, acts=("lrelu",))
    blend_case(rep, "bf16", A.WRAP_QUADS, 4, DEV, acts=("lrelu",), needs_list=(("bg", "x"),))
    l1_case(rep, "bf16", A.WRAP_QUADS, DEV)
    reached(be, ["mg_act_bwd", "mg_grad_sum_act", "mg_blend_fwd", "mg_blend_bwd", "mg_l1_mean_bwd"])
    rep.done()


@pytest.mark.parametrize("betas", A.ADAM_BETAS, ids=lambda b: f"beta1-{b[0]}")
def test_adam_single_step_against_torch(be, betas):
    rep = _Report()
    for numel in A.ADAM_NUMELS[:-1]:
        for scale in A.ADAM_SCALES:
            for step in A.ADAM_STEPS:
                adam_case(rep, numel, betas, scale, step, DEV)
    reached(be, ["mg_adam_step"])
    rep.done()


def test_adam_past_the_grid_stride_wrap(be):
    rep = _Report()
    for i, betas in enumerate(A.ADAM_BETAS):
        adam_case(rep, A.ADAM_NUMELS[-1], betas, A.ADAM_SCALES[i], A.ADAM_STEPS[i + 1], DEV)
    reached(be, ["mg_adam_step"])
    rep.done()
