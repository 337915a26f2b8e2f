"""-m gpu: every device-writing entry point of libmichigan_hip.so inside guard bands (tests/guard_alloc.py), at the geometries
where kernels go wrong: one below / exactly at / one above each tile multiple, the smallest size the argument check accepts, and
launches large enough that the grid-stride loops of the streaming kernels wrap (ew_grid caps the grid at 8192 x 256 threads).

Each case
  * runs an op (or a C-ABI call on hand-built buffers) under ``guard_alloc.guard()`` on the HIP backend, with the tensors the test
    supplies placed in guarded buffers too,
  * runs the same function on CPU copies with the float64 contract emulator and compares with ``_close`` and the tolerances of
    tests/test_gpu_kernels.py (no new tolerance: the per-output factors are the ones the value test of the same op uses),
  * calls ``check()``: every guard byte still 0xFF,
  * asserts through the call-counting backend that the ``mg_*`` entry points it claims (``covers``) were really called -- several
    ops fall back to eager torch on geometry they do not take, and a case that took the fallback is not coverage.
0xFF is NaN in every float format: a read outside a tensor that reaches a result, and an output element a kernel never wrote,
show as a non-finite value in ``_close``.

``CASES`` is also part of the ledger tests/test_guard_alloc.py checks against ``_cabi.EXPORTED_SYMBOLS`` (with the cases of
tests/test_gpu_style_guard_bands.py, test_gpu_dense_orient.py and test_gpu_stroke.py).
MG_TEST_DRYRUN=1 runs the emulator on both sides (plumbing check on a machine without a GPU).

What the guards cannot see: the split-K scratch of mg_conv_taps and the slab workspace of the thin weight gradient are allocated
inside the library (hipMalloc), not by the operator layer; one arena slot overrunning into the next (the value tests of the
gradient sink and the batched spectral norm own that); reads outside an allocation whose value is discarded.
"""
import collections
import contextlib
import math
import os
import time

import pytest
import torch

import guard_alloc as GA
from test_gpu_kernels import DT, TOL, _close

pytestmark = pytest.mark.gpu

DRY = os.environ.get("MG_TEST_DRYRUN") == "1"
WRAP_QUADS = 8192 * 256                      # ew_grid: more quads (threads' worth of work) than this and the grid-stride loop wraps
STATS = {"cases": 0, "allocations": 0, "seconds": 0.0}

Case = collections.namedtuple("Case", "id covers build")
CASES = []


def case(id_, covers):
    def deco(build):
        CASES.append(Case(id_, tuple(covers), build))
        return build
    return deco


def _emulator():
    from oracle.cabi_emulator import EmulatorBackend
    return EmulatorBackend()


class _Ctx:
    """What a case function may ask of the side it runs on: buffers (guarded on the device side) and the backend."""

    def __init__(self, guard, dev):
        self.guard, self.dev = guard, dev

    def buf(self, shape, dtype, zero=False):
        if self.guard is not None:
            return self.guard.guarded(shape, dtype, self.dev, zero=zero)
        return (torch.zeros if zero else torch.empty)(shape, dtype=dtype)

    def put(self, t):
        return self.guard.place(t, self.dev) if self.guard is not None else t.clone()


@contextlib.contextmanager
def _settings(opts, flags):
    """Kernel tuning switches (``_cabi.OPT_*`` names) and module flags of michigan_amd.ops for the duration."""
    from michigan_amd import _cabi, ops
    saved = {k: getattr(ops, k) for k in flags}
    try:
        for k, v in flags.items():
            setattr(ops, k, v)
        with _cabi.options({getattr(_cabi, k): v for k, v in opts.items()}):
            yield
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)


def _run(spec, covers):
    """spec: dict(fn=callable(ctx, *tensors) -> outputs, tensors=[...], checks=[(name, tol | "equal" | callable)], opts={}, flags={})."""
    from michigan_amd import _cabi, ops
    fn, tensors, checks = spec["fn"], spec["tensors"], spec["checks"]
    opts, flags = spec.get("opts", {}), spec.get("flags", {})
    dev = "cpu" if DRY else "cuda"
    t0 = time.time()
    prev = _cabi.set_backend(_emulator() if DRY else None)
    try:
        if not DRY:
            assert _cabi.backend().name == "hip"
        ops.reset_mask_protocol()
        with GA.guard() as g:
            with _settings(opts, flags):
                args = [g.place(t, dev) for t in tensors]
                res = fn(_Ctx(g, dev), *args)
                nalloc = g.check()
            missing = [ep for ep in covers if g.backend.count(ep) == 0]
            assert not missing, "entry points this case claims but never called (an eager fallback?): %s; called: %s" % (missing, sorted(set(g.backend.calls)))
            got = [r.detach().to("cpu", copy=True) for r in res]
    finally:
        _cabi.set_backend(prev)
    prev = _cabi.set_backend(_emulator())
    try:
        ops.reset_mask_protocol()
        with _settings({}, flags):
            ref = fn(_Ctx(None, "cpu"), *[t.detach().clone().requires_grad_(t.requires_grad) if torch.is_tensor(t) else t for t in tensors])
            ref = [r.detach() for r in ref]
    finally:
        _cabi.set_backend(prev)
    assert len(got) == len(ref) == len(checks), (len(got), len(ref), len(checks))
    for (name, tol), a, r in zip(checks, got, ref):
        if tol == "equal":
            assert a.shape == r.shape and torch.equal(a, r), "%s: not bit-identical to the contract" % name
        elif callable(tol):
            tol(name, a, r)
        else:
            _close(name, a, r, tol)
    STATS["cases"] += 1
    STATS["allocations"] += nalloc
    STATS["seconds"] += time.time() - t0
    return nalloc


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape, dt="f32", grad=False):
    t = torch.randn(*shape, generator=g).to(DT[dt])
    return t.requires_grad_() if grad else t


def _gy(y, seed=1):
    return torch.randn(y.shape, generator=_gen(seed)).to(y.dtype).to(y.device)


# =====================================================================================================================
# streaming kernels (mg_pointwise.hip)
# =====================================================================================================================
# C = 4: one quad per pixel; 12; 20: C % 8 == 4.  H = 1 / W = 1; and one geometry per kernel beyond WRAP_QUADS quads.
RESAMPLE_GEOMS = [(1, 1, 1, 4), (2, 1, 5, 12), (2, 5, 1, 20), (2, 17, 21, 20), (1, 3, 3, 4), (3, 16, 16, 12)]
MAXPOOL_GEOMS = [(2, 2, 2, 4), (2, 3, 3, 12), (1, 2, 3, 20), (1, 3, 2, 4), (2, 17, 21, 20)]       # odd last row / column: zero gradient there
RESAMPLE_WRAP = {"upsample2x": (8, 512, 512, 8), "avgpool3s2": (8, 512, 512, 20), "maxpool2": (8, 512, 512, 20)}


def _resample_spec(op, geom, dt):
    from michigan_amd import ops
    x = _randn(_gen(sum(geom)), *geom, dt=dt, grad=True)

    def fn(ctx, x):
        y = getattr(ops, op)(x)
        (gx,) = torch.autograd.grad(y, x, ctx.put(_gy(y)))
        return y, gx
    return dict(fn=fn, tensors=[x], checks=[(f"{op} {geom} {dt} y", TOL[dt]), (f"{op} {geom} {dt} dx", TOL[dt])])


for _op, _eps in (("upsample2x", ("mg_upsample2x_fwd", "mg_upsample2x_bwd")), ("avgpool3s2", ("mg_avgpool3s2_fwd", "mg_avgpool3s2_bwd")),
                  ("maxpool2", ("mg_maxpool2_fwd", "mg_maxpool2_bwd"))):
    for _geom in (MAXPOOL_GEOMS if _op == "maxpool2" else RESAMPLE_GEOMS):
        for _dt in ("f32", "bf16"):
            case(f"{_op}-{'x'.join(map(str, _geom))}-{_dt}", _eps)(lambda op=_op, geom=_geom, dt=_dt: _resample_spec(op, geom, dt))
    _g = RESAMPLE_WRAP[_op]
    _n, _h, _w, _q = _g[0], _g[1], _g[2], _g[3] // 4
    # what each launch passes to ew_grid (mg_pointwise.hip): forward / backward quads
    _launched = {"upsample2x": (_n * 4 * _h * _w * _q, _n * _h * _w * _q), "avgpool3s2": (_n * ((_h - 1) // 2 + 1) * ((_w - 1) // 2 + 1) * _q, _n * _h * _w * _q),
                 "maxpool2": (_n * (_h // 2) * (_w // 2) * _q, _n * _h * _w * _q)}[_op]
    assert min(_launched) > WRAP_QUADS, (_op, _launched)
    case(f"{_op}-wrap-{'x'.join(map(str, _g))}-bf16", _eps)(lambda op=_op, geom=_g: _resample_spec(op, geom, "bf16"))


def _reflect_spec(geom, dt):
    from michigan_amd import ops
    n, h, w, c, p = geom
    x = _randn(_gen(h * 100 + w), n, h, w, c, dt=dt, grad=True)

    def fn(ctx, x):
        y = ops.reflect_pad(x, p)
        (gx,) = torch.autograd.grad(y, x, ctx.put(_gy(y, 5)))
        return y, gx
    return dict(fn=fn, tensors=[x], checks=[(f"reflect pad {geom} {dt} y", 0.0 if dt == "f32" else TOL[dt]), (f"reflect pad {geom} {dt} dx", TOL[dt])])


# P = min(H, W) - 1 (the largest the argument check takes), the smallest image (2 x 2, P = 1), and a wrapping launch
for _geom in [(2, 5, 7, 12, 4), (1, 2, 2, 4, 1), (1, 4, 4, 8, 3), (2, 9, 11, 20, 3), (1, 2, 9, 4, 1)]:
    for _dt in ("f32", "bf16"):
        case(f"reflect_pad-{'x'.join(map(str, _geom))}-{_dt}", ("mg_reflect_pad_fwd", "mg_reflect_pad_bwd"))(lambda geom=_geom, dt=_dt: _reflect_spec(geom, dt))
case("reflect_pad-wrap-8x512x512x8x3-bf16", ("mg_reflect_pad_fwd", "mg_reflect_pad_bwd"))(lambda: _reflect_spec((8, 512, 512, 8, 3), "bf16"))

# flat element-wise kernels: numel = 4 (one quad), around one 256-thread block of quads, and just above 4 * 8192 * 256
FLAT_NUMELS = [4, 1020, 1024, 1028, 4 * WRAP_QUADS + 4 * 37]


def _act_bwd_spec(numel, dt):
    from michigan_amd import ops
    g = _gen(numel % 1000)
    dy, y = _randn(g, numel, dt=dt), _randn(g, numel, dt=dt)

    def fn(ctx, dy, y):
        return (ops.act_backward(dy, y, ops.ACT_LRELU, 0.2), ops.act_backward(dy, y, ops.ACT_TANH, 0.2))
    return dict(fn=fn, tensors=[dy, y], checks=[(f"act_bwd lrelu {numel} {dt}", TOL[dt]), (f"act_bwd tanh {numel} {dt}", TOL[dt])])


def _grad_sum_act_spec(numel, dt):
    from michigan_amd import ops
    g = _gen(numel % 1000 + 1)
    a = _randn(g, numel, dt=dt, grad=True)
    g1, g2 = _randn(g, numel, dt=dt), _randn(g, numel, dt=dt)

    def fn(ctx, a, g1, g2):
        a1, a2 = ops.act_tap(a)                                    # two consumers of a ReLU output: the backward is mg_grad_sum_act
        assert a1 is not a
        return torch.autograd.grad([a1, a2], a, [g1, g2])
    return dict(fn=fn, tensors=[a, g1, g2], checks=[(f"grad_sum_act {numel} {dt}", TOL[dt])])


def _l1_spec(numel, dt):
    from michigan_amd import ops
    g = _gen(numel % 1000 + 2)
    a, b = _randn(g, numel, dt=dt, grad=True), _randn(g, numel, dt=dt)

    def fn(ctx, a, b):
        loss = ops.l1_mean(a, b) * 3.0
        (ga,) = torch.autograd.grad(loss, a)
        return loss.reshape(1), ga
    return dict(fn=fn, tensors=[a, b], checks=[(f"l1 {numel} {dt} loss", 1e-5), (f"l1 {numel} {dt} grad", TOL[dt])])


def _blend_spec(shape, dt):
    from michigan_amd import ops
    g = _gen(sum(shape))
    bgf, x = _randn(g, *shape, dt=dt, grad=True), _randn(g, *shape, dt=dt, grad=True)
    hair = (torch.rand(shape[:3] + (1,), generator=g) > 0.5).float()
    back = (torch.rand(shape[:3] + (1,), generator=g) > 0.5).float()

    def fn(ctx, bgf, x, hair, back):
        y = ops.blend(bgf, x, hair, back, act=ops.ACT_LRELU)
        return (y,) + torch.autograd.grad(y, (bgf, x), ctx.put(_gy(y)))
    return dict(fn=fn, tensors=[bgf, x, hair, back], checks=[(f"blend {shape} {dt} {nm}", TOL[dt]) for nm in ("y", "dbg", "dx")])


for _n in FLAT_NUMELS:
    for _dt in (("bf16",) if _n > 4 * WRAP_QUADS else ("f32", "bf16")):
        case(f"act_bwd-{_n}-{_dt}", ("mg_act_bwd",))(lambda n=_n, dt=_dt: _act_bwd_spec(n, dt))
        case(f"grad_sum_act-{_n}-{_dt}", ("mg_grad_sum_act",))(lambda n=_n, dt=_dt: _grad_sum_act_spec(n, dt))
        case(f"l1_mean-{_n}-{_dt}", ("mg_l1_mean_fwd", "mg_l1_mean_bwd"))(lambda n=_n, dt=_dt: _l1_spec(n, dt))
for _shape in [(1, 1, 1, 4), (2, 9, 9, 64), (1, 3, 85, 12), (1, 1, 257, 20), (1, 1, WRAP_QUADS + 37, 4)]:
    for _dt in (("bf16",) if _shape[2] > WRAP_QUADS else ("f32", "bf16")):
        case(f"blend-{'x'.join(map(str, _shape))}-{_dt}", ("mg_blend_fwd", "mg_blend_bwd"))(lambda s=_shape, dt=_dt: _blend_spec(s, dt))


def _adam_spec(n):
    from michigan_amd import ops
    g = _gen(n % 997)
    p, gr = torch.randn(n, generator=g), torch.randn(n, generator=g)

    def fn(ctx, p, gr):
        m, v = ctx.buf(n, torch.float32, zero=True), ctx.buf(n, torch.float32, zero=True)        # parameter, gradient and both moments guarded
        for step in (1, 2, 3):
            ops.adam_step(p, gr, m, v, lr=1e-3, beta1=0.0, beta2=0.9, eps=1e-8, step=step)
        return p, m, v
    return dict(fn=fn, tensors=[p, gr], checks=[(f"adam n={n} {nm}", 1e-6) for nm in ("param", "exp_avg", "exp_avg_sq")])


for _n in (1, 255, 257, 10007, WRAP_QUADS + 77):               # one thread per element: the grid wraps above 8192 x 256 elements
    case(f"adam_step-{_n}", ("mg_adam_step",))(lambda n=_n: _adam_spec(n))


# =====================================================================================================================
# norm and statistics (mg_norm.hip)
# =====================================================================================================================
# C on both sides of vec_geom_ok (C % VEC == 0, C / VEC <= 256 and a divisor of 256; VEC = 8 bf16 / 4 f32); P = 1, one less / one
# more than rows = 256 / (C / VEC), P not a multiple of rows * PIX; G = 1 and G > 1.
NORM_GEOMS = {"bf16": [(8, (1, 255, 257, 1031)), (2048, (1, 2, 7)), (24, (1, 5, 37)), (4096, (1, 3))],
              "f32": [(4, (1, 255, 257, 1031)), (1024, (1, 2, 7)), (12, (1, 5, 37)), (2048, (1, 3))]}


def _stats_spec(dt, c, p, groups, fused):
    """ops.channel_sums / stats_finalize (fused) or channel_sums + mg_norm_finalize (instance norm's three-launch path)."""
    from michigan_amd import ops
    x = (torch.randn(groups, 1, p, c, generator=_gen(c + p)) * 2 + 0.5).to(DT[dt])
    rm0, rv0 = torch.randn(c, generator=_gen(3)), torch.rand(c, generator=_gen(4)) + 0.5

    def fn(ctx, x, rm, rv):
        outs = [ops.channel_sums(x, groups, False), ops.channel_sums(x, groups, True)]
        if fused:
            mean, rstd, sums = ops.stats_finalize(x, groups, float(max(p, 2)), 1e-5, 0.1, rm if groups == 1 else None, rv if groups == 1 else None, 1.0)
        else:
            sums = ops.channel_sums(x, groups, True)
            mean, rstd = ctx.buf((groups, c), torch.float32), ctx.buf((groups, c), torch.float32)
            from michigan_amd import _cabi
            _cabi.backend().mg_norm_finalize(ops._p(sums), groups, c, float(max(p, 2)), 1e-5, 0.1, ops._p(rm) if groups == 1 else None,
                                             ops._p(rv) if groups == 1 else None, ops._p(mean), ops._p(rstd), ops._stream(x))
        return outs + [sums, mean, rstd, rm, rv]
    nm = f"stats {dt} C={c} P={p} G={groups} fused={fused}"
    return dict(fn=fn, tensors=[x, rm0, rv0], checks=[(nm + " sums", 1e-5), (nm + " shifted sums", 1e-5), (nm + " finalize sums", 1e-5),
                                                       (nm + " mean", 1e-5), (nm + " rstd", 1e-5), (nm + " running mean", 1e-5), (nm + " running var", 1e-5)])


def _norm_direct_spec(dt, c, p, groups, act_name):
    """mg_norm_act_fwd (+ residual), mg_norm_bwd_reduce (with and without the gamma|beta gradient image) and mg_norm_bwd_apply on
    hand-built buffers.  mean / rstd / the sums are GIVEN (random), not derived from the P samples, so that small P stays well
    conditioned: instance-norm's own dx cancels to rounding noise at P <= 2, which no relative tolerance can judge."""
    from michigan_amd import ops
    td = DT[dt]
    act = {"none": ops.ACT_NONE, "lrelu": ops.ACT_LRELU, "tanh": ops.ACT_TANH}[act_name]        # tanh: always the quad kernels
    g = _gen(c * 7 + p)
    x = (torch.randn(groups, p, c, generator=g) * 1.5 + 0.3).to(td)
    dh, resid, g1 = _randn(g, groups, p, c, dt=dt), _randn(g, groups, p, c, dt=dt), (1 + 0.3 * torch.randn(groups, p, c, generator=g)).to(td)
    mean, rstd = torch.randn(groups, c, generator=g) * 0.2, torch.rand(groups, c, generator=g) + 0.5
    rows = 2 * ops._roundup(c, 32)

    def fn(ctx, x, dh, resid, g1, mean, rstd):
        from michigan_amd import _cabi
        be, P, st = _cabi.backend(), ops._p, ops._stream(x)
        code = ops._dt(x)
        ws = lambda: ctx.buf(max(int(be.mg_stats_workspace(groups, p, c)), 4), torch.uint8)
        y, yr = ctx.buf((groups, p, c), td), ctx.buf((groups, p, c), td)
        be.mg_norm_act_fwd(P(x), P(y), code, groups, p, c, P(mean), P(rstd), act, 0.2, None, st)
        be.mg_norm_act_fwd(P(x), P(yr), code, groups, p, c, P(mean), P(rstd), act, 0.2, P(resid), st)
        hp = P(y) if act != ops.ACT_NONE else None
        sums = ctx.buf((groups, 2, c), torch.float32)
        be.mg_norm_bwd_reduce(P(dh), hp, P(x), None, code, groups, p, c, P(mean), P(rstd), act, 0.2, None, P(sums), P(ws()), st)
        outs = [y, yr, sums]
        if groups == 1:                                            # SPADE's form: (1 + gamma) and the [P, 2 * roundup(C, 32)] image
            sums_g = ctx.buf((1, 2, c), torch.float32)
            dgb = ctx.buf((p, rows), td, zero=True)
            be.mg_norm_bwd_reduce(P(dh), hp, P(x), P(g1), code, 1, p, c, P(mean), P(rstd), act, 0.2, P(dgb), P(sums_g), P(ws()), st)
            dxg = ctx.buf((1, p, c), td)
            be.mg_norm_bwd_apply(P(dh), hp, P(x), P(g1), code, 1, p, c, P(mean), P(rstd), P(sums_g[0, 0]), P(sums_g[0, 1]), 2 * c, 1.0 / p,
                                 act, 0.2, P(dxg), st)
            outs += [sums_g, dgb, dxg]
        dx = ctx.buf((groups, p, c), td)
        be.mg_norm_bwd_apply(P(dh), hp, P(x), None, code, groups, p, c, P(mean), P(rstd), P(sums[0, 0]), P(sums[0, 1]), 2 * c, 1.0 / p,
                             act, 0.2, P(dx), st)
        return outs + [dx]
    nm = f"norm {dt} C={c} P={p} G={groups} {act_name}"
    # tolerances: test_instance_norm_act (y: TOL, dx: 2 TOL), test_spade_modulate_fwd_bwd (bf16 gradients: 6 TOL); the fp32 sums are
    # two-stage fp32 reductions of P terms against float64: the statistics tolerance 1e-5 of test_channel_stats_wide_and_grouped
    loose = TOL[dt] * (6 if dt == "bf16" else 2)
    checks = [(nm + " y", TOL[dt]), (nm + " y + resid", TOL[dt]), (nm + " sums", 1e-5 if dt == "f32" else TOL[dt])]
    if groups == 1:
        checks += [(nm + " sums (g1)", 1e-5 if dt == "f32" else TOL[dt]), (nm + " dgb", TOL[dt]), (nm + " dx (g1)", loose)]
    return dict(fn=fn, tensors=[x, dh, resid, g1, mean, rstd], checks=checks + [(nm + " dx", loose)])


def _apply2_spec(dt, c, n, h, w, up):
    """mg_norm_bwd_reduce_up (when up) + mg_norm_bwd_apply2 on hand-built buffers, both branches, given mean / rstd."""
    from michigan_amd import ops
    td = DT[dt]
    g = _gen(c + h * w + up)
    p = n * h * w
    xs = (torch.randn(n, h // 2, w // 2, c, generator=g) if up else torch.randn(n, h, w, c, generator=g)).to(td)
    dh0, dh1, h0 = _randn(g, n, h, w, c, dt=dt), _randn(g, n, h, w, c, dt=dt), _randn(g, n, h, w, c, dt=dt)
    g10, g11 = (1 + 0.3 * torch.randn(n, h, w, c, generator=g)).to(td), (1 + 0.3 * torch.randn(n, h, w, c, generator=g)).to(td)
    mean, rstd = torch.randn(c, generator=g) * 0.2, torch.rand(c, generator=g) + 0.5
    rows = 2 * ops._roundup(c, 32)

    def fn(ctx, xs, dh0, dh1, h0, g10, g11, mean, rstd):
        from michigan_amd import _cabi
        be, P, st = _cabi.backend(), ops._p, ops._stream(xs)
        assert be.mg_norm_apply2_supported(ops._dt(xs), c)
        sums = ctx.buf((2, 2, c), torch.float32)
        dgbs = []
        for b, (dh, hh, g1, act) in enumerate(((dh0, h0, g10, ops.ACT_LRELU), (dh1, None, g11, ops.ACT_NONE))):
            dgb = ctx.buf((n, h, w, rows), td, zero=True)
            ws = ctx.buf(max(int(be.mg_stats_workspace(1, p, c)), 4), torch.uint8)
            if up:
                be.mg_norm_bwd_reduce_up(P(dh), P(hh), P(xs), P(g1), ops._dt(xs), n, h, w, c, P(mean), P(rstd), act, 0.2, P(dgb), P(sums[b]), P(ws), st)
            else:
                be.mg_norm_bwd_reduce(P(dh), P(hh), P(xs), P(g1), ops._dt(xs), 1, p, c, P(mean), P(rstd), act, 0.2, P(dgb), P(sums[b]), P(ws), st)
            dgbs.append(dgb)
        d = _cabi.NormApply2Desc()
        for b, (dh, hh, g1, act) in enumerate(((dh0, h0, g10, ops.ACT_LRELU), (dh1, None, g11, ops.ACT_NONE))):
            d.dh[b], d.g1[b], d.sums[b] = dh.data_ptr(), g1.data_ptr(), sums[b].data_ptr()
            d.h[b] = hh.data_ptr() if hh is not None else None
            d.act[b], d.slope[b] = act, 0.2
        dx = ctx.buf(tuple(xs.shape), td)
        d.x, d.mean, d.rstd, d.dx = xs.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx.data_ptr()
        d.P, d.dtype, d.C, d.up, d.H, d.W, d.inv_count = p, ops._dt(xs), c, int(up), h, w, 1.0 / p
        be.mg_norm_bwd_apply2(d, st)
        return [sums, dgbs[0], dgbs[1], dx]
    nm = f"apply2 {dt} C={c} {n}x{h}x{w} up={up}"
    # the pair test's tolerances (test_spade_pair_with_folded_upsample): 5e-5 / 2^-6; dx of the up form sums four bf16-rounded terms there too
    tol = {"f32": 5e-5, "bf16": 2.0 ** -6}[dt]
    return dict(fn=fn, tensors=[xs, dh0, dh1, h0, g10, g11, mean, rstd],
                checks=[(nm + " sums", tol), (nm + " dgb0", tol), (nm + " dgb1", tol), (nm + " dx", tol)])


def _inorm_spec(dt, shape, fused):
    from michigan_amd import ops
    x = (torch.randn(*shape, generator=_gen(sum(shape))) * 2 + 1).to(DT[dt]).requires_grad_()

    def fn(ctx, x):
        y = ops.instance_norm_act(x, act=ops.ACT_LRELU)
        (gx,) = torch.autograd.grad(y, x, ctx.put(_gy(y, 6)))
        yi = ops.instance_norm_act_infer(x, act=ops.ACT_LRELU, resid=x.detach())
        return y, gx, yi
    nm = f"inorm {dt} {shape} fused={fused}"
    return dict(fn=fn, tensors=[x], flags={"FUSED_STATS_FINALIZE": fused},
                checks=[(nm + " y", TOL[dt]), (nm + " dx", TOL[dt] * 2), (nm + " y + resid", TOL[dt])])


_NORM_EPS = ("mg_norm_act_fwd", "mg_norm_bwd_reduce", "mg_norm_bwd_apply")
for _dt, _geoms in NORM_GEOMS.items():
    for _c, _ps in _geoms:
        for _p in _ps:
            for _G in (1, 3):
                case(f"stats-{_dt}-C{_c}-P{_p}-G{_G}", ("mg_channel_stats", "mg_channel_stats_finalize"))(
                    lambda dt=_dt, c=_c, p=_p, G=_G: _stats_spec(dt, c, p, G, True))
                for _vec in (1, 0):                                 # both values of MG_OPT_NORM_BWD_VEC
                    case(f"norm-{_dt}-C{_c}-P{_p}-G{_G}-bwdvec{_vec}", _NORM_EPS)(
                        lambda dt=_dt, c=_c, p=_p, G=_G, v=_vec: dict(_norm_direct_spec(dt, c, p, G, "lrelu"), opts={"OPT_NORM_BWD_VEC": v}))
        case(f"stats-unfused-{_dt}-C{_c}", ("mg_channel_stats", "mg_norm_finalize"))(lambda dt=_dt, c=_c, p=_ps[-1]: _stats_spec(dt, c, p, 1, False))
        case(f"stats-unfused-{_dt}-C{_c}-G3", ("mg_channel_stats", "mg_norm_finalize"))(lambda dt=_dt, c=_c, p=_ps[-1]: _stats_spec(dt, c, p, 3, False))
        case(f"norm-{_dt}-C{_c}-none", _NORM_EPS)(lambda dt=_dt, c=_c, p=_ps[-1]: _norm_direct_spec(dt, c, p, 1, "none"))
        case(f"norm-{_dt}-C{_c}-tanh", _NORM_EPS)(lambda dt=_dt, c=_c, p=_ps[-1]: _norm_direct_spec(dt, c, p, 3, "tanh"))
    # the pair backward only exists on the vector geometry (mg_norm_apply2_supported); rows = 256 / (C / VEC) pixels per workgroup pass:
    # P = 1, rows - 1, rows + 1, a multiple of rows, not a multiple (the up form needs even H and W, so its smallest P is 4)
    _cs, _cl = (8, 2048) if _dt == "bf16" else (4, 1024)           # rows = 256 and rows = 1
    for _c, _nhw in ((_cs, (1, 1, 1)), (_cs, (1, 1, 255)), (_cs, (1, 1, 257)), (_cs, (1, 2, 2)), (_cs, (2, 16, 16)), (_cs, (2, 18, 14)), (_cs, (1, 2, 128)), (_cs, (1, 2, 130)),
                     (64, (2, 6, 10)), (_cl, (1, 1, 1)), (_cl, (1, 1, 2)), (_cl, (1, 2, 2)), (_cl, (1, 2, 6))):
        for _up in ((0, 1) if _nhw[1] % 2 == 0 and _nhw[2] % 2 == 0 else (0,)):
            for _vec in (1, 0):
                case(f"apply2-{_dt}-C{_c}-{'x'.join(map(str, _nhw))}-up{_up}-bwdvec{_vec}", ("mg_norm_bwd_apply2",) + (("mg_norm_bwd_reduce_up",) if _up else ("mg_norm_bwd_reduce",)))(
                    lambda dt=_dt, c=_c, nhw=_nhw, up=_up, v=_vec: dict(_apply2_spec(dt, c, nhw[0], nhw[1], nhw[2], up), opts={"OPT_NORM_BWD_VEC": v}))
    for _shape in [(4, 33, 35, 128), (1, 7, 9, 24 if _dt == "bf16" else 12), (3, 5, 13, 8 if _dt == "bf16" else 4)]:
        for _fused in (True, False):
            case(f"instance_norm-{_dt}-{'x'.join(map(str, _shape))}-fused{int(_fused)}",
                 _NORM_EPS + (("mg_channel_stats_finalize",) if _fused else ("mg_channel_stats", "mg_norm_finalize")))(
                lambda dt=_dt, s=_shape, f=_fused: _inorm_spec(dt, s, f))


# =====================================================================================================================
# convolution and weight gradient
# =====================================================================================================================
def _conv_spec(dt, cin, cout, k, s, p, H, W, N, act="lrelu", bias=True, resid=False, opts=None, flags=None, seed=1234, fwd_act=None):
    """conv2d forward and all gradients through autograd (test_conv2d_fwd_bwd's form and tolerances).
    fwd_act: the chip-filling cases differentiate the LINEAR convolution (act "none") and run the fused activation forward-only.
    With 10^7 outputs some pre-activations lie within rounding of 0, the kernel and the float64 contract then take different
    branches of (Leaky)ReLU', and dx differs by a whole weight x gradient term there -- the reference's discontinuity, not a kernel
    error (test_halo_conv_ragged_geometry avoids it by differentiating through the output the kernel stored)."""
    from michigan_amd import ops
    g = _gen(seed)
    x = _randn(g, N, H, W, cin, dt=dt, grad=True)
    w = (torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5).requires_grad_()
    b = torch.randn(cout, generator=g).requires_grad_() if bias else None
    ho, wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    r = _randn(g, N, ho, wo, cout, dt=dt, grad=True) if resid else None
    acts = {"lrelu": ops.ACT_LRELU, "relu": ops.ACT_RELU, "none": ops.ACT_NONE, "tanh": ops.ACT_TANH}
    assert fwd_act is None or act == "none"
    code = acts[act]

    def fn(ctx, x, w, b, r):
        y = ops.conv2d(x, w, b, stride=s, padding=p, act=code, resid=r)
        wanted = [t for t in (x, w, b, r) if t is not None]
        outs = (y,) + torch.autograd.grad(y, wanted, ctx.put(_gy(y, 7)))
        if fwd_act is not None:
            with torch.no_grad():
                outs += (ops.conv2d(x, w, b, stride=s, padding=p, act=acts[fwd_act], resid=r),)
        return outs
    names = ["y", "dx", "dw"] + (["db"] if bias else []) + (["dres"] if resid else []) + ([f"y ({fwd_act})"] if fwd_act else [])
    nm = f"conv {dt} {(cin, cout, k, s, p, H, W, N)} {act}"
    checks = [(f"{nm} {n}", TOL[dt] * (4 if n in ("dw", "db") and dt == "bf16" else 1)) for n in names]
    return dict(fn=fn, tensors=[x, w, b, r], checks=checks, opts=opts or {}, flags=flags or {})


_CONV = ("mg_conv_taps", "mg_conv_wgrad", "mg_pack_weight", "mg_unpack_wgrad")
_OPT_DEFAULTS = dict(OPT_CONV_BIGTILES=1, OPT_CONV_HALO=1, OPT_CONV_HALO_BIG=1, OPT_CONV_SPLITK=1, OPT_CONV_THIN=2, OPT_CONV_WIDE=1, OPT_CONV_DOT=2,
                     OPT_CONV_HALO64=1)                            # csrc/mg_options.h


def _conv_path(dt, cin, cout, k, s, p, H, W, N, act="lrelu", resid=False, mask=False, opts=None, **_):
    """Which kernel dispatch_conv (csrc/mg_conv.hip) gives a plain-epilogue launch: the geometry conditions of the *_applies functions
    and of dispatch_tiles restated, thresholds included.  The C ABI does not say which kernel ran, so every case of CONV_PATHS
    carries the path it is there for and this arithmetic is asserted when the table is built: a case that a threshold moves off
    its kernel fails at import instead of silently guarding another one.  (Kept next to the sources it restates: a dispatch change
    has to be made here too, which is the point.)"""
    o = dict(_OPT_DEFAULTS, **(opts or {}))
    cdiv = lambda a, b: (a + b - 1) // b
    bf, esz = dt == "bf16", 2 if dt == "bf16" else 4
    cin = cdiv(cin, 8) * 8                                         # conv2d pads the input channels to a multiple of 8
    hj, wj, ntaps = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1, k * k
    ngemm, same3 = N * hj * wj, (k, s, p) == (3, 1, 1)
    aux = resid or mask
    if bf and cin == 8 and not aux and act != "tanh" and cout % 8 == 0 and 32 <= cout <= 128:          # mg_conv_thin.hip
        if o["OPT_CONV_THIN"] and same3 and W % 32 == 0 and N * cdiv(H, 8) * (W // 32) >= 64:
            return "thin"
        cs, st = (1 if cout <= 64 else 2), s
        lds = cdiv(ntaps, 2) * 2 * cs * 64 * 16 + (7 * st + k) * (31 * st + k) * 16 + 64 * 4 + cs * 64 * 4 + 4 * 32 * 128
        if o["OPT_CONV_THIN"] >= 2 and st in (1, 2) and k <= 7 and lds <= 80 * 1024 and N * cdiv(hj, 8) * cdiv(wj, 32) >= 64:
            return "thin-taps"
    if o["OPT_CONV_DOT"] and 1 <= cout <= 4 and cin >= 128 and (cin * esz) % 16 == 0 and not mask and ntaps * cout * cin * esz <= 60 * 1024:
        return "dot"                                               # mg_conv_dot.hip: weights resident in LDS
    if o["OPT_CONV_DOT"] >= 2 and bf and cin == 64 and cout <= 16 and k <= 3 and s == 1 and not aux and N * cdiv(hj, 8) * cdiv(wj, 32) >= 64:
        return "few-output"
    wide = o["OPT_CONV_WIDE"] and bf and cout % 8 == 0
    if (o["OPT_CONV_HALO"] and o["OPT_CONV_HALO64"] and bf and cin == 64 and cout % 64 == 0 and cout <= 128 and same3 and H % 16 == 0 and W % 16 == 0
            and H >= 32 and W >= 32 and wide and ((not aux and act != "tanh") or act == "none") and N * (H // 16) * (W // 16) * (cout // 64) >= 1024):
        return "halo64"                                            # mg_conv_halo64.hip: every CU's workgroup walks >= 4 tiles
    ch = 64 // esz
    if o["OPT_CONV_HALO"] and same3 and cin % ch == 0 and cout > 32 and H >= 8 and W >= 16 and not (cout <= 64 and H < 16):
        th, tmh = (16, 64) if cout <= 64 else (8, 128)
        if N * cdiv(H, th) * cdiv(W, 16) * cdiv(cout, tmh) >= 384:                                    # halo_applies
            if cout <= 64:
                return "halo-64rows"                               # launch_halo: <1, 2>, 16 x 16 pixels x 64 rows
            if bf and o["OPT_CONV_HALO_BIG"] and H >= 16 and N * cdiv(H, 16) * cdiv(W, 16) * cdiv(cout, 128) >= 1024:
                return "halo-16x16"
            return "halo-8x16"
    kchunks = ntaps * cdiv(cin * esz, 64)
    if o["OPT_CONV_BIGTILES"] and kchunks >= 64 and cout >= 256 and (cdiv(cout, 128) * 128) % 256 == 0 and cdiv(cout, 256) * cdiv(ngemm, 256) >= 384:
        return "tile256"
    packed = "-packed-taps" if cin < ch and ch % cin == 0 else ""
    if cout > 64:
        nblk = cdiv(cout, 128) * cdiv(ngemm, 128)
        if not packed and o["OPT_CONV_SPLITK"] and nblk <= 160 and kchunks >= 64 and cout % 4 == 0 and min(16, kchunks // 16, cdiv(384, nblk)) >= 2:
            return "tile128-splitk"
        return "tile128" + packed
    return ("tile64" if cout > 32 else "tile32") + packed


# one ragged geometry per path dispatch_conv can take (the path is the FORWARD launch's; the data and weight gradients of the same case
# go where their own geometry sends them); the shapes are the value tests' where those reach the path
CONV_PATHS = [
    # id, dtypes, expected path, kwargs
    ("thin-8ch-3x3", ("bf16",), "thin", dict(cin=8, cout=64, k=3, s=1, p=1, H=45, W=96, N=4, act="none", fwd_act="lrelu", bias=False)),      # 4 * 6 * 3 = 72 tiles of 8 x 32 >= 64
    ("thin-8ch-3x3-bias-relu", ("bf16",), "thin", dict(cin=8, cout=128, k=3, s=1, p=1, H=61, W=128, N=4, act="none", fwd_act="relu")),      # 4 * 8 * 4 = 128
    ("thin-taps-4x4s2", ("bf16",), "thin-taps", dict(cin=8, cout=64, k=4, s=2, p=2, H=128, W=96, N=4, act="none", fwd_act="lrelu")),         # 65 x 49 outputs: 4 * 9 * 2 = 72 tiles
    ("thin-taps-5x5", ("bf16",), "thin-taps", dict(cin=8, cout=64, k=5, s=1, p=2, H=67, W=100, N=2, act="none")),                            # 2 * 9 * 4 = 72
    ("thin-taps-7x7-valid", ("bf16",), "thin-taps", dict(cin=8, cout=64, k=7, s=1, p=0, H=70, W=70, N=4, act="none", fwd_act="relu")),       # 64 x 64 outputs: 4 * 8 * 2 = 64
    ("few-output-img", ("bf16",), "few-output", dict(cin=64, cout=3, k=3, s=1, p=1, H=72, W=100, N=3, act="tanh")),                          # conv_img: 3 * 9 * 4 = 108 tiles >= 64
    # data gradients that end in an 8-channel input: 64 -> 8 launches of the few-output kernel, stride 1 and the four parity classes of stride 2
    ("few-output-dgrad-3x3", ("bf16",), "thin", dict(cin=8, cout=64, k=3, s=1, p=1, H=70, W=96, N=3, act="none", bias=False)),
    ("few-output-dgrad-3x3s2", ("bf16",), "thin-taps", dict(cin=8, cout=64, k=3, s=2, p=1, H=140, W=192, N=3, act="none", bias=False)),      # 70 x 96 outputs and pixels per class: 3 * 9 * 3 = 81 tiles
    ("dot-head", ("f32", "bf16"), "dot", dict(cin=512, cout=1, k=4, s=1, p=2, H=9, W=9, N=2)),                                               # D head: Cin >= 128, one output channel, 16 * 512 * 4 B of weights
    ("halo64", ("bf16",), "halo64", dict(cin=64, cout=64, k=3, s=1, p=1, H=512, W=512, N=1, act="none", fwd_act="relu")),                    # 1 * 32 * 32 * 1 = 1024 tiles >= 1024
    ("halo64-resid-128", ("bf16",), "halo64", dict(cin=64, cout=128, k=3, s=1, p=1, H=512, W=512, N=2, act="none", resid=True)),             # 2 * 32 * 32 * 2 = 4096
    ("halo64-off", ("bf16",), "halo-64rows", dict(cin=64, cout=64, k=3, s=1, p=1, H=512, W=512, N=1, act="none", fwd_act="relu", opts={"OPT_CONV_HALO64": 0})),
    ("halo-64rows-ragged", ("f32", "bf16"), "halo-64rows", dict(cin=64, cout=64, k=3, s=1, p=1, H=203, W=181, N=3, act="none", fwd_act="lrelu")),     # 3 * 13 * 12 = 468 >= 384; 203 % 16 != 0: not halo64
    ("halo-16x16-ragged", ("bf16",), "halo-16x16", dict(cin=32, cout=200, k=3, s=1, p=1, H=150, W=210, N=4, act="none", fwd_act="lrelu", opts={"OPT_CONV_HALO_BIG": 1})),   # 4 * 10 * 14 * 2 = 1120 >= 1024
    ("halo-8x16-ragged", ("f32", "bf16"), "halo-8x16", dict(cin=256, cout=136, k=3, s=1, p=1, H=97, W=131, N=2, act="none", fwd_act="lrelu", opts={"OPT_CONV_HALO_BIG": 0})),   # 2 * 13 * 9 * 2 = 468 >= 384
    ("tile128", ("f32", "bf16"), {"bf16": "tile128", "f32": "tile128-splitk"}, dict(cin=128, cout=128, k=3, s=1, p=1, H=24, W=20, N=2)),                       # CONV_CASES; 2 * 3 * 2 = 12 halo workgroups < 384, 36 / 72 K chunks
    ("tile128-ktail-ragged-cout", ("f32", "bf16"), "tile128", dict(cin=48, cout=200, k=3, s=1, p=1, H=9, W=13, N=2)),
    ("tile64", ("f32", "bf16"), "tile64", dict(cin=64, cout=64, k=3, s=1, p=1, H=33, W=17, N=1)),
    ("tile32-cout3", ("f32",), "tile32", dict(cin=64, cout=3, k=3, s=1, p=1, H=20, W=20, N=2)),
    ("packed-taps", ("f32", "bf16"), {"bf16": "tile32-packed-taps", "f32": "tile32"}, dict(cin=16, cout=32, k=3, s=1, p=1, H=12, W=12, N=2)),
    ("packed-taps-49", ("f32",), "tile128-packed-taps", dict(cin=8, cout=128, k=7, s=1, p=3, H=14, W=14, N=1)),
    ("packed-taps-49-cout136", ("bf16",), "tile128-packed-taps", dict(cin=8, cout=136, k=7, s=1, p=3, H=14, W=14, N=1)),    # (Cout 136: not a thin-taps channel count)
    ("stride2-odd", ("f32",), "tile64-packed-taps", dict(cin=8, cout=64, k=4, s=2, p=2, H=21, W=19, N=2)),
    ("stride2-odd-cout72", ("bf16",), "tile128-packed-taps", dict(cin=8, cout=72, k=4, s=2, p=2, H=21, W=19, N=2)),
    ("splitk", ("f32", "bf16"), "tile128-splitk", dict(cin=2048, cout=128, k=3, s=1, p=1, H=8, W=8, N=2)),                  # 1 workgroup, 576 / 1152 K chunks
    ("splitk-ragged", ("f32", "bf16"), "tile128-splitk", dict(cin=512, cout=200, k=3, s=1, p=1, H=7, W=5, N=1)),
    ("splitk-off", ("bf16",), "tile128", dict(cin=512, cout=200, k=3, s=1, p=1, H=7, W=5, N=1, opts={"OPT_CONV_SPLITK": 0})),
    # 256 x 256 tiles: 16 taps x 4 chunks = 64 K chunks, Cout 512, 2 * 195 = 390 workgroups >= 384 (4x4 / stride 1 / pad 2: not a halo shape)
    ("tile256", ("bf16",), "tile256", dict(cin=128, cout=512, k=4, s=1, p=2, H=127, W=129, N=3, act="none", fwd_act="lrelu", opts={"OPT_CONV_BIGTILES": 1})),
    ("tile256-off", ("bf16",), "tile128", dict(cin=128, cout=512, k=4, s=1, p=2, H=127, W=129, N=3, act="none", fwd_act="lrelu", opts={"OPT_CONV_BIGTILES": 0})),
    # epilogue: 16-byte stores (MG_OPT_CONV_WIDE) with Cout % 8 == 0 and Cout % 8 == 4, on a halo shape and a generic shape; residual
    ("wide-cout72", ("bf16",), "tile128", dict(cin=64, cout=72, k=4, s=2, p=1, H=33, W=29, N=2, opts={"OPT_CONV_WIDE": 1})),
    ("wide-cout76", ("bf16",), "tile128", dict(cin=64, cout=76, k=4, s=2, p=1, H=33, W=29, N=2, opts={"OPT_CONV_WIDE": 1})),
    ("wide-halo-cout132", ("bf16",), "halo-8x16", dict(cin=64, cout=132, k=3, s=1, p=1, H=48, W=67, N=8, act="none", fwd_act="lrelu", opts={"OPT_CONV_WIDE": 1})),   # 8 * 6 * 5 * 2 = 480
    ("wide-off-cout72", ("bf16",), "tile128", dict(cin=64, cout=72, k=4, s=2, p=1, H=33, W=29, N=2, opts={"OPT_CONV_WIDE": 0})),
    ("resid", ("f32", "bf16"), "tile128", dict(cin=64, cout=96, k=3, s=1, p=1, H=12, W=12, N=2, act="none", bias=False, resid=True)),
    ("wide-resid-halo", ("bf16",), "halo-8x16", dict(cin=64, cout=128, k=3, s=1, p=1, H=96, W=64, N=8, act="none", fwd_act="lrelu", resid=True, opts={"OPT_CONV_WIDE": 1})),   # 8 * 12 * 4 = 384; 384 halo64 tiles < 1024
    # deterministic weight gradients: the caller's slab workspace + the library's ordered finishing pass
    ("deterministic-thin-taps", ("bf16",), "thin-taps", dict(cin=8, cout=64, k=4, s=2, p=2, H=128, W=96, N=4, act="none", fwd_act="lrelu", flags={"WGRAD_DETERMINISTIC": True})),
    ("deterministic-generic", ("f32", "bf16"), "tile128", dict(cin=48, cout=200, k=3, s=1, p=1, H=9, W=13, N=2, flags={"WGRAD_DETERMINISTIC": True})),
    ("deterministic-3x3", ("bf16",), "tile128", dict(cin=136, cout=200, k=3, s=1, p=1, H=32, W=32, N=1, flags={"WGRAD_DETERMINISTIC": True})),
]
for _id, _dts, _path, _kw in CONV_PATHS:
    for _dt in _dts:
        _want = _path[_dt] if isinstance(_path, dict) else _path
        assert _conv_path(_dt, **_kw) == _want, (_id, _dt, _conv_path(_dt, **_kw), _want)
        case(f"conv-{_id}-{_dt}", _CONV)(lambda dt=_dt, kw=_kw: _conv_spec(dt, **kw))
assert _conv_path("bf16", 64, 8, 3, 1, 1, 70, 96, 3, act="none") == "few-output"          # the dx launches of the two few-output-dgrad cases (per parity class: 70 x 96 pixels)
assert {"thin", "thin-taps", "dot", "few-output", "halo64", "halo-64rows", "halo-16x16", "halo-8x16", "tile256", "tile128", "tile128-splitk", "tile64", "tile32",
        "tile32-packed-taps", "tile128-packed-taps"} <= {q for _, _, pth, _ in CONV_PATHS for q in (pth.values() if isinstance(pth, dict) else (pth,))}


def _dgrad_mask_spec(dt, n, h, w, cin, cout, slope):
    """test_data_gradient_with_folded_activation_mask's call: the data gradient with the consumed (Leaky)ReLU's mask in its epilogue.
    The mask tensor is GIVEN, so the contract's branch is the kernel's."""
    from michigan_amd import ops
    g = _gen(int(slope * 10) + 3 + cin)
    x, dy = _randn(g, n, h, w, cin, dt=dt), _randn(g, n, h, w, cout, dt=dt)
    wgt = torch.randn(cout, cin, 3, 3, generator=g) / 24

    def fn(ctx, x, dy, wgt):
        wt = ops.pack_weight(wgt, None, DT[dt], ops._roundup(cin, 128), cout, 1)
        plain = ops.conv_dgrad(dy, wt, 3, 3, 1, 1, (h, w), cin)
        masked = ops.conv_dgrad(dy, wt, 3, 3, 1, 1, (h, w), cin, relu_mask=x, mask_slope=slope)
        ops._RELU_MASKED.pop(masked.data_ptr(), None)
        return plain, masked
    nm = f"dgrad {dt} {(n, h, w, cin, cout)} mask slope {slope}"
    return dict(fn=fn, tensors=[x, dy, wgt], checks=[(nm + " plain", TOL[dt]), (nm + " masked", TOL[dt])])


for _dt, _geom in (("f32", (2, 40, 48, 128, 128)), ("bf16", (2, 40, 48, 128, 128)), ("bf16", (1, 512, 512, 64, 64)), ("bf16", (2, 97, 131, 136, 256))):
    # the launch: dy [cout channels] -> dx [cin channels]; 1 x 512 x 512, 64 -> 64 is a halo64 shape (1024 tiles), 136 <- 256 at 97 x 131 the ragged 8 x 16 halo kernel
    assert _conv_path(_dt, _geom[4], _geom[3], 3, 1, 1, _geom[1], _geom[2], _geom[0], act="none", mask=True) == {40: "tile128" if _dt == "bf16" else "tile128-splitk", 512: "halo64", 97: "halo-8x16"}[_geom[1]]
    for _slope in (0.0, 0.2):
        case(f"dgrad-mask-{_dt}-{'x'.join(map(str, _geom))}-slope{_slope}", ("mg_conv_taps", "mg_pack_weight"))(lambda dt=_dt, gm=_geom, sl=_slope: _dgrad_mask_spec(dt, *gm, sl))


def _wgrad_spec(dt, N, H, W, cin, cg, k, s, p, want_bias, tol, opts=None, flags=None):
    """ops.conv_wgrad on its own (test_wgrad3x3_kernel_row_tiles' form): dW in GEMM order and the fused bias gradient."""
    from michigan_amd import ops
    g = _gen(N * 1000 + H * 10 + cin)
    ho, wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    x, dy = _randn(g, N, H, W, cin, dt=dt), _randn(g, N, ho, wo, cg, dt=dt)

    def fn(ctx, x, dy):
        r = ops.conv_wgrad(x, dy, k, k, s, p, want_bias=want_bias)
        return r if want_bias else (r,)
    nm = f"wgrad {dt} {(N, H, W, cin, cg, k, s, p)}"
    return dict(fn=fn, tensors=[x, dy], checks=[(nm + " dw", tol)] + ([(nm + " dbias", tol)] if want_bias else []), opts=opts or {}, flags=flags or {})


WGRAD_PATHS = [
    # generic kernel, both bf16 fragment paths (test_wgrad_bf16_both_fragment_paths: 2e-3)
    ("generic-tr16", "bf16", dict(N=2, H=19, W=23, cin=136, cg=200, k=3, s=1, p=1, want_bias=False, tol=2e-3, opts={"OPT_WGRAD3X3": 0}, flags={"WGRAD_USE_TR": True})),
    ("generic-gather", "bf16", dict(N=2, H=19, W=23, cin=136, cg=200, k=3, s=1, p=1, want_bias=True, tol=2e-3, opts={"OPT_WGRAD3X3": 0}, flags={"WGRAD_USE_TR": False})),
    ("generic-f32-4x4s2", "f32", dict(N=2, H=21, W=19, cin=8, cg=64, k=4, s=2, p=2, want_bias=True, tol=2e-3)),
    # thin weight gradient (8-channel input; test_thin_wgrad_8_channel_input: 1e-4), height not a multiple of its 4-row tile
    ("thin", "bf16", dict(N=4, H=45, W=96, cin=8, cg=64, k=3, s=1, p=1, want_bias=True, tol=1e-4)),
    ("thin-nobias-128", "bf16", dict(N=4, H=61, W=128, cin=8, cg=128, k=3, s=1, p=1, want_bias=False, tol=1e-4)),
    ("thin-taps-5x5", "bf16", dict(N=2, H=67, W=100, cin=8, cg=64, k=5, s=1, p=2, want_bias=True, tol=1e-4)),
]
# kernel-row 3x3 kernel (test_wgrad3x3_kernel_row_tiles: 2e-3) with the stripe switch at 0 and 64
for _stripe in (0, 64):
    for _geom in [(1, 32, 32, 136, 200), (3, 16, 32, 72, 72), (2, 4, 16, 64, 64), (1, 6, 64, 128, 64), (1, 2, 16, 256, 128)]:
        WGRAD_PATHS.append((f"3x3-stripe{_stripe}-{'x'.join(map(str, _geom))}", "bf16",
                            dict(N=_geom[0], H=_geom[1], W=_geom[2], cin=_geom[3], cg=_geom[4], k=3, s=1, p=1, want_bias=_geom[1] != 16, tol=2e-3,
                                 opts={"OPT_WGRAD3X3_STRIPE": _stripe})))
for _id, _dt, _kw in WGRAD_PATHS:
    case(f"wgrad-{_id}", ("mg_conv_wgrad",))(lambda dt=_dt, kw=_kw: _wgrad_spec(dt, **kw))


def _spade_spec(dt, C, H, W, N=2, act="lrelu"):
    """test_spade_modulate_fwd_bwd's form and tolerances: the SPADE epilogue with gamma_out, its reduce / apply backward."""
    from michigan_amd import ops
    g = _gen(C)
    x = (torch.randn(N, H, W, C, generator=g) * 1.5 + 0.3).to(DT[dt]).requires_grad_()
    actv = torch.randn(N, H, W, 128, generator=g).clamp_min(0).to(DT[dt]).requires_grad_()
    wg, wb = [(torch.randn(C, 128, 3, 3, generator=g) / 34).requires_grad_() for _ in range(2)]
    bg, bb = [(torch.randn(C, generator=g) * 0.1).requires_grad_() for _ in range(2)]

    def fn(ctx, x, actv, wg, bg, wb, bb):
        mean, rstd, cnt, _ = ops.batch_stats(x)
        h = ops.spade_modulate(x, actv, wg, bg, wb, bb, mean, rstd, cnt, act=ops.ACT_LRELU if act == "lrelu" else ops.ACT_NONE)
        return (h, mean, rstd) + torch.autograd.grad(h, (x, actv, wg, bg, wb, bb), ctx.put(_gy(h, 9)))
    names = ("h", "mean", "rstd", "dx", "dactv", "dwg", "dbg", "dwb", "dbb")
    checks = [(f"spade C={C} {H}x{W} {dt} {n}", 1e-5 if n in ("mean", "rstd") else TOL[dt] * (6 if dt == "bf16" and n != "h" else 1)) for n in names]
    return dict(fn=fn, tensors=[x, actv, wg, bg, wb, bb], checks=checks)


for _dt in ("f32", "bf16"):
    for _C, _H, _W in [(48, 9, 11), (16, 12, 12), (64, 20, 24), (8 if _dt == "bf16" else 4, 3, 5), (24 if _dt == "bf16" else 12, 5, 7)]:
        case(f"spade-{_dt}-C{_C}-{_H}x{_W}", ("mg_conv_taps", "mg_channel_stats_finalize", "mg_norm_bwd_reduce", "mg_norm_bwd_apply", "mg_conv_wgrad", "mg_unpack_wgrad"))(
            lambda dt=_dt, C=_C, H=_H, W=_W: _spade_spec(dt, C, H, W))
case("spade-halo-ragged-bf16", ("mg_conv_taps", "mg_norm_bwd_reduce", "mg_norm_bwd_apply"))(lambda: _spade_spec("bf16", 136, 97, 131, N=4, act="none"))   # test_spade_halo_ragged_geometry (no activation there either)


def _spade_pair_spec(dt, up):
    """test_spade_pair_with_folded_upsample's fused form and tolerance (hip vs emulator): x_up epilogue, reduce_up, apply2."""
    from michigan_amd import ops
    g = _gen(41)
    n, hs, ws, c, ca = 2, 18, 22, 64, 128
    h, w = (2 * hs, 2 * ws) if up else (hs, ws)
    x = _randn(g, n, hs, ws, c, dt=dt, grad=True)
    a0 = torch.randn(n, h, w, ca, generator=g).clamp_min(0).to(DT[dt]).requires_grad_()
    a1 = torch.randn(n, h, w, ca, generator=g).clamp_min(0).to(DT[dt]).requires_grad_()
    ws_ = [torch.randn(c, ca, 3, 3, generator=g).mul_(0.03).requires_grad_() for _ in range(4)]
    bs_ = [torch.randn(c, generator=g).mul_(0.1).requires_grad_() for _ in range(4)]
    gy0, gy1 = _randn(g, n, h, w, c, dt=dt), _randn(g, n, h, w, c, dt=dt)

    def fn(ctx, x, a0, a1, w0, w1, w2, w3, b0, b1, b2, b3, gy0, gy1):
        assert ops.spade_pair_supported(x)
        mean, rstd, count, _ = ops.batch_stats_finish(ops.batch_stats_begin(x.detach(), up=up))
        h0, h1 = ops.spade_modulate_pair(x, ((a0, w0, b0, w1, b1), (a1, w2, b2, w3, b3)), mean, rstd, count, acts=(ops.ACT_LRELU, ops.ACT_NONE), up=up)
        loss = (h0.float() * gy0.float()).sum() + (h1.float() * gy1.float()).sum()
        return [h0, h1] + list(torch.autograd.grad(loss, [x, a0, a1, w0, w1, w2, w3, b0, b1, b2, b3]))
    names = ["h0", "h1", "dx", "dactv0", "dactv1", "dwg0", "dwb0", "dwg1", "dwb1", "dbg0", "dbb0", "dbg1", "dbb1"]
    tol = {"f32": 5e-5, "bf16": 2.0 ** -6}[dt]
    return dict(fn=fn, tensors=[x, a0, a1, *ws_, *bs_, gy0, gy1], checks=[(f"pair {dt} up={up} {n_}", tol) for n_ in names])


for _dt in ("f32", "bf16"):
    for _up in (False, True):
        case(f"spade-pair-{_dt}-up{int(_up)}", ("mg_conv_taps", "mg_norm_bwd_apply2", "mg_norm_bwd_reduce_up" if _up else "mg_norm_bwd_reduce"))(
            lambda dt=_dt, up=_up: _spade_pair_spec(dt, up))


# =====================================================================================================================
# Gabor arg-max (mg_gabor.hip: 16 x 32 pixel tiles)
# =====================================================================================================================
GABOR_SIZES = [(5, 7), (16, 31), (16, 32), (64, 64), (17, 33), (75, 83)]       # below one tile, exactly one, exact multiples, one over, the value test's


def _gabor_spec(dt, n, h, w, c):
    from michigan_amd import ops
    img = torch.tanh(torch.randn(n, h, w, c, generator=_gen(h * w + c))).to(DT[dt]).requires_grad_()

    def fn(ctx, img):
        bank = ctx.put(ops.gabor_bank())
        conf, idx = ops.gabor_argmax(img, bank)
        gc = ctx.put(torch.rand(conf.shape, generator=_gen(2)))
        (gi,) = torch.autograd.grad(conf, img, gc)
        return conf, idx.float(), gi

    def agree(name, a, r):
        share = (a == r).float().mean().item()
        assert share > 0.999, f"{name}: arg-max agreement {share}"
    nm = f"gabor {dt} {(n, h, w, c)}"
    # test_gabor_argmax_and_orientation_loss's bounds; arg-max ties may fall either way, which is why dimg is loose there
    return dict(fn=fn, tensors=[img], checks=[(nm + " conf", 1e-4), (nm + " idx", agree), (nm + " dimg", 5e-3 if dt == "f32" else 2e-2)])


def _gabor_bwd_exact_spec(dt, n, h, w, c):
    """The backward alone with the CONTRACT's arg-max on both sides (ties cannot differ): dimg to TOL instead of 5e-3, channels 3.. zero."""
    from michigan_amd import ops
    from oracle.cabi_emulator import EmulatorBackend
    img = torch.tanh(torch.randn(n, h, w, c, generator=_gen(h * w + c))).to(DT[dt])
    bank = ops.gabor_bank()
    conf, idx = torch.empty(n, h, w), torch.empty(n, h, w, dtype=torch.uint8)
    EmulatorBackend().mg_gabor_argmax_fwd(img.data_ptr(), bank.data_ptr(), conf.data_ptr(), idx.data_ptr(), ops._dt(img), n, h, w, c)
    dconf = (torch.rand(n, h, w, generator=_gen(2)) * (conf > 0)).contiguous()

    def fn(ctx, dconf, idx, bank):
        from michigan_amd import _cabi
        dimg = ctx.buf((n, h, w, c), DT[dt])
        _cabi.backend().mg_gabor_argmax_bwd(ops._p(dconf), ops._p(idx), ops._p(bank), ops._p(dimg), ops._dtype_code(DT[dt]), n, h, w, c, ops._stream(dconf))
        return dimg, dimg[..., 3:].float().abs().sum().reshape(1)
    nm = f"gabor bwd (contract arg-max) {dt} {(n, h, w, c)}"
    return dict(fn=fn, tensors=[dconf, idx, bank], checks=[(nm + " dimg", TOL[dt]), (nm + " channels 3..", "equal")])


for _h, _w in GABOR_SIZES:
    for _n, _c in ((1, 3), (3, 8)):
        for _dt in ("f32", "bf16"):
            case(f"gabor-{_dt}-{_n}x{_h}x{_w}x{_c}", ("mg_gabor_argmax_fwd", "mg_gabor_argmax_bwd"))(lambda dt=_dt, n=_n, h=_h, w=_w, c=_c: _gabor_spec(dt, n, h, w, c))
            case(f"gabor-bwd-exact-{_dt}-{_n}x{_h}x{_w}x{_c}", ("mg_gabor_argmax_bwd",))(lambda dt=_dt, n=_n, h=_h, w=_w, c=_c: _gabor_bwd_exact_spec(dt, n, h, w, c))


# =====================================================================================================================
# glue, losses, attention, spectral norm, pack, drain, inputs
# =====================================================================================================================
def _bits(name, a, r):
    v = (lambda t: t.view(torch.int16)) if a.dtype == torch.bfloat16 else (lambda t: t)
    assert a.shape == r.shape and torch.equal(v(a), v(r)), "%s: not bit-identical to the contract" % name


def _pyramid_spec(dt, n, H, W, sizes, nplanes, cout):
    from michigan_amd import ops
    g = _gen(H + W)
    seg = torch.cat([(torch.rand(n, 2, H, W, generator=g) > 0.5).float(), torch.randn(n, 2, H, W, generator=g)], dim=1)

    def fn(ctx, seg):
        return ops.nearest_pyramid(ops.planes_of(seg)[:nplanes], sizes, cout, DT[dt])
    return dict(fn=fn, tensors=[seg], checks=[(f"pyramid {dt} {s}", _bits) for s in sizes])


for _dt in ("f32", "bf16"):
    case(f"nearest_pyramid-{_dt}-ragged", ("mg_nearest_pyramid",))(lambda dt=_dt: _pyramid_spec(dt, 3, 72, 60, [(9, 8), (18, 15), (36, 30), (72, 60), (50, 41)], 4, 8))
    case(f"nearest_pyramid-{_dt}-1x1-level", ("mg_nearest_pyramid",))(lambda dt=_dt: _pyramid_spec(dt, 2, 8, 8, [(1, 1), (2, 2), (8, 8), (3, 1)], 4, 8))
case("nearest_pyramid-f32-one-plane", ("mg_nearest_pyramid",))(lambda: _pyramid_spec("f32", 3, 72, 60, [(9, 7), (18, 15), (1, 1)], 1, 1))


def _pconv_affine_spec(dt, n, H, W, c, cr):
    """test_glue_kernels_match_contract's partial-conv chain: mask half, per-pixel affine forward and both gradients."""
    from michigan_amd import ops
    g = _gen(H * W + c)
    mask = (torch.rand(n, H, W, 1, generator=g) > 0.6).float()
    x = _randn(g, n, H, W, c, dt=dt, grad=True)
    ho, wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    raw = _randn(g, n, ho, wo, cr, dt=dt, grad=True)
    bias = torch.randn(cr, generator=g).requires_grad_()

    def fn(ctx, mask, x, raw, bias):
        sc, up = ops.pconv_mask(mask, 3, 2, 1)
        y0 = ops.pixel_affine(x, mask)
        y1 = ops.pixel_affine(raw, sc, bias, up)
        gx, = torch.autograd.grad(y0.float().square().sum(), x)
        graw, gb = torch.autograd.grad((y1.float() * 0.5).square().sum(), (raw, bias))
        return sc, up, y0, y1, gx, graw, gb
    nm = f"pconv/affine {dt} {(n, H, W, c, cr)}"
    return dict(fn=fn, tensors=[mask, x, raw, bias],
                checks=[(nm + " scale", "equal"), (nm + " update", "equal"), (nm + " x*m", TOL[dt]), (nm + " raw*scale+b*m'", TOL[dt]), (nm + " d x", TOL[dt]),
                        (nm + " d raw", TOL[dt]), (nm + " d bias", 2e-2 if dt == "bf16" else 1e-4)])


def _bg_compose_spec(dt, k, mode):
    from michigan_amd import ops
    g = _gen(k)
    image, noise = torch.rand(2, 3, 70, 90, generator=g) * 2 - 1, torch.rand(2, 3, 70, 90, generator=g)
    m2 = torch.zeros(2, 2, 70, 90)
    m2[:, 1, 20:45, 30:70] = 1.0
    m2[:, 0] = 1 - m2[:, 1]

    def fn(ctx, image, noise, m2):
        return ops.bg_compose(image, noise, m2[:, 1] if mode == 0 else m2[:, 0], k, mode, DT[dt])
    return dict(fn=fn, tensors=[image, noise, m2], checks=[(f"bg_compose {dt} k={k} inp", TOL[dt]), (f"bg_compose {dt} k={k} back", "equal")])


def _mmf_spec(dt, n, h, w, c):
    from michigan_amd import ops
    g = _gen(h * w + c)
    feat = _randn(g, n, h, w, c, dt=dt, grad=True)
    lref, ltag = (torch.rand(n, h, w, 1, generator=g) > 0.6).float(), (torch.rand(n, h, w, 1, generator=g) > 0.4).float()
    lref[-1] = 0                                                    # an empty reference region: the area clamps to 1
    if n > 1:
        lref[0, 0, 0], ltag[0] = 1.0, 1.0

    def fn(ctx, feat, lref, ltag):
        out = ops.masked_mean_fill(feat, lref, ltag)
        gx, = torch.autograd.grad((out * out).sum(), feat)
        return out, gx
    return dict(fn=fn, tensors=[feat, lref, ltag], checks=[(f"masked_mean_fill {dt} {(n, h, w, c)}", 1e-5), (f"masked_mean_fill {dt} {(n, h, w, c)} adjoint", TOL[dt])])


def _orient_spec(n, h, w, label_ch):
    from michigan_amd import ops
    g = _gen(h * w + label_ch)
    conf_raw = (torch.randn(n, h, w, generator=g) * 1.5).requires_grad_()
    idx = torch.randint(0, 32, (n, h, w), generator=g, dtype=torch.uint8)
    sem = torch.zeros(n, 2, h, w)
    sem[:, 1, h // 5:h - h // 6, w // 5:w - w // 4] = 1.0
    label = torch.randn(n, 2, h, w, generator=g).clamp(-1, 1) if label_ch == 2 else torch.randint(0, 255, (n, 1, h, w), generator=g).float()

    def fn(ctx, conf_raw, idx, label, sem):
        lo, lc = ops.orient_loss(conf_raw, idx, label, sem[:, 1])
        g0, = torch.autograd.grad(lo * 3.0, conf_raw, retain_graph=True)
        g1, = torch.autograd.grad(lo + lc * 0.25, conf_raw)
        return lo.reshape(1), lc.reshape(1), g0, g1
    return dict(fn=fn, tensors=[conf_raw, idx, label, sem], checks=[(f"orient_loss {(n, h, w)} {label_ch}ch out {i}", 2e-5) for i in range(4)])


def _hinge_spec(dt, shape):
    """test_hinge_loss_and_wide_edge_weight_fused's form: the edge weight map bit-exact, the three hinge modes."""
    from michigan_amd import ops
    g = _gen(sum(shape))
    n, _, h, w = shape
    label = (torch.rand(n, 1, 96, 80, generator=g) > 0.55).float()
    x = (torch.randn(*shape, generator=g) * 1.5).to(DT[dt]).requires_grad_()

    def fn(ctx, x, label):
        wm = ops.wide_edge_weight(label, h, w, 2.0)
        outs = [wm]
        for mode in (ops.HINGE_G, ops.HINGE_D_REAL, ops.HINGE_D_FAKE):
            loss = ops.hinge_loss(x, None if mode == ops.HINGE_G else wm, mode)
            (gx,) = torch.autograd.grad(loss * 2.0, x)
            outs += [loss.reshape(1), gx]
        return outs
    checks = [(f"wide_edge {shape}", "equal")]
    for mode in range(3):
        checks += [(f"hinge {dt} {shape} loss mode {mode}", 1e-5), (f"hinge {dt} {shape} grad mode {mode}", TOL[dt])]
    return dict(fn=fn, tensors=[x, label], checks=checks)


def _assemble_spec(dt):
    from michigan_amd import ops
    g = _gen(13)
    planar = torch.randn(2, 3, 9, 11, generator=g)
    image = _randn(g, 2, 9, 11, 8, dt=dt, grad=True)

    def fn(ctx, planar, image):
        dst = ctx.buf((5, 9, 11, 8), DT[dt], zero=True)            # the destination is a batch-stacked buffer: rows 1..2 and 3..4 are written
        ops.assemble_nhwc8(dst, 3, planar)
        out = ops.assemble_nhwc8(dst, 1, planar, image, 4)
        (gi,) = torch.autograd.grad((out.float() ** 2).sum(), image)
        return out, gi
    return dict(fn=fn, tensors=[planar, image], checks=[(f"assemble {dt}", TOL[dt]), (f"assemble {dt} d image", TOL[dt])])


for _dt in ("f32", "bf16"):
    case(f"pconv-affine-{_dt}-ragged", ("mg_pconv_mask", "mg_pixel_affine", "mg_channel_stats"))(lambda dt=_dt: _pconv_affine_spec(dt, 2, 40, 36, 16, 24))
    case(f"pconv-affine-{_dt}-C4-P1", ("mg_pconv_mask", "mg_pixel_affine"))(lambda dt=_dt: _pconv_affine_spec(dt, 1, 1, 1, 4, 4))
    for _k, _mode in ((5, 0), (33, 0), (1, 1)):
        case(f"bg_compose-{_dt}-k{_k}", ("mg_bg_compose",))(lambda dt=_dt, k=_k, mode=_mode: _bg_compose_spec(dt, k, mode))
    case(f"masked_mean_fill-{_dt}-ragged", ("mg_masked_mean_fill",))(lambda dt=_dt: _mmf_spec(dt, 3, 16, 12, 72))
    case(f"masked_mean_fill-{_dt}-C4-P1", ("mg_masked_mean_fill",))(lambda dt=_dt: _mmf_spec(dt, 2, 1, 1, 4))
    for _shape in [(3, 1, 67, 67), (3, 1, 17, 19), (1, 1, 1, 1), (3, 1, 1, 1), (3, 1, 66, 52)]:        # n = 1 and n = 3 logits: no multiple-of-4 rule here
        case(f"hinge-{_dt}-{'x'.join(map(str, _shape))}", ("mg_hinge_fwd", "mg_hinge_bwd", "mg_wide_edge_weight"))(lambda dt=_dt, s=_shape: _hinge_spec(dt, s))
    case(f"assemble_nhwc8-{_dt}", ("mg_assemble_nhwc8",))(lambda dt=_dt: _assemble_spec(dt))
for _geom in [(2, 48, 40), (1, 1, 1), (3, 1, 1), (2, 7, 3)]:
    for _ch in (1, 2):
        case(f"orient_loss-{'x'.join(map(str, _geom))}-{_ch}ch", ("mg_orient_loss_fwd", "mg_orient_loss_bwd"))(lambda gm=_geom, ch=_ch: _orient_spec(*gm, ch))


def _loss_fx(n, h, w, seed):
    g = _gen(seed)
    rnd = lambda *s: torch.rand(*s, generator=g)
    shift = lambda: (rnd(n, 3, 1, 1) - 0.5)
    fx = {"fake": (0.5 * (rnd(n, 3, h, w) * 2 - 1) + shift()).clamp(-1, 1), "ref": (0.5 * (rnd(n, 3, h, w) * 2 - 1) - shift()).clamp(-1, 1),
          "tgt": rnd(n, 3, h, w) * 2 - 1, "m_f": (rnd(n, h, w) > 0.6).float(), "m_r": (rnd(n, h, w) > 0.5).float()}
    fx["m_b"] = 1 - fx["m_f"]
    return fx


def _image(fake, channels):
    n, _, h, w = fake.shape
    img = torch.full((n, h, w, channels), 3.0)                     # padding channels: a value that must never be read
    img[..., :3] = fake.permute(0, 2, 3, 1)
    return img.requires_grad_(True)


def _rel_l2(bound):
    def check(name, a, r):
        rel = float((a.double() - r.double()).norm() / r.double().norm())
        assert math.isfinite(rel) and rel <= bound, f"{name}: relative L2 {rel:.3e} > {bound:.3e}"
    return check


def _scalar(rtol):
    def check(name, a, r):
        for k in range(r.numel()):
            assert abs(float(a[k]) - float(r[k])) <= rtol * max(1.0, abs(float(r[k]))), f"{name}[{k}]: {float(a[k])} vs {float(r[k])}"
    return check


def _color_spec(shape, channels):
    """ops.color_losses in fp32 against the float64 contract with the bounds of tests/test_gpu_color_loss.py: losses 1e-4 relative to
    max(1, |want|); gradient 8 fp32 ulp relative L2 over the pixels that are not within 1e-3 of a sign change of da or db (sign() is
    discontinuous there), at most 5e-3 of the pixels left out."""
    from oracle import contracts as K
    from michigan_amd import ops
    n, h, w = shape
    fx = _loss_fx(n, h, w, h * w)
    img = _image(fx["fake"], channels)
    sem = torch.stack([fx["m_b"], fx["m_f"]], dim=1)
    weights = (1.0, 10.0, 40.0)
    _, _, (da, db, _) = K.color_terms(fx["fake"], fx["tgt"], fx["m_b"], 7, weights)
    near = lambda t: (t.abs() > 0) & (t.abs() < 1e-3)
    ex = near(da) | near(db)
    assert float(ex.double().mean()) <= 5e-3
    keep = (~ex).reshape(n, h, w, 1).double()

    def fn(ctx, img, real, sem):
        out = ops.color_losses(img, real, sem[:, 0], 7)
        (gi,) = torch.autograd.grad(weights[0] * out[0] + weights[1] * out[1] + weights[2] * out[2], img)
        return torch.stack([o.detach() for o in out]), gi

    def grad_check(name, a, r):
        rel = float(((a.double() - r.double()) * keep).norm() / (r.double() * keep).norm())
        assert math.isfinite(float(a.double().abs().sum())) and rel <= 8 * 2.0 ** -23, f"{name}: relative L2 {rel:.3e}"
        assert float(a[..., 3:].abs().sum()) == 0.0, f"{name}: padding channels of dimg"
    nm = f"color {shape} C={channels}"
    return dict(fn=fn, tensors=[img, fx["tgt"], sem], checks=[(nm + " losses", _scalar(1e-4)), (nm + " dimg", grad_check)])


def _hair_spec(shape, channels):
    """tests/test_gpu_unpaired.py::test_other_geometries_against_the_contract's form and bounds."""
    from michigan_amd import ops
    n, h, w = shape
    fx = _loss_fx(n, h, w, h * w)
    img = _image(fx["fake"], channels)
    sem_tag, sem_ref = torch.stack([fx["m_b"], fx["m_f"]], dim=1), torch.stack([1 - fx["m_r"], fx["m_r"]], dim=1)
    from oracle import contracts as K
    _, _, (da, db) = K.hair_terms(fx["fake"], fx["ref"], fx["m_f"], fx["m_r"], fx["tgt"], fx["m_b"], 3, (0.5, 40.0))
    assert float(torch.cat([da, db]).abs().min()) >= 1.0, "a mean difference too close to the discontinuity of sign(): pick another seed"

    def fn(ctx, img, ref, tgt, sem_tag, sem_ref):
        out = ops.hair_lab_losses(img, ref, sem_tag[:, 1], sem_ref[:, 1], tgt, sem_tag[:, 0], flags=3)
        (gi,) = torch.autograd.grad(0.5 * out[0] + 40.0 * out[1], img)
        return torch.stack([o.detach() for o in out]), gi
    nm = f"hair lab {shape} C={channels}"
    return dict(fn=fn, tensors=[img, fx["ref"], fx["tgt"], sem_tag, sem_ref], checks=[(nm + " losses", _scalar(1e-4)), (nm + " dimg", _rel_l2(8 * 2.0 ** -23))])


for _shape in [(1, 96, 80), (1, 67, 35), (3, 33, 130)]:
    for _c in (3, 8):
        case(f"color_loss-{'x'.join(map(str, _shape))}-C{_c}", ("mg_color_loss_fwd", "mg_color_loss_bwd"))(lambda s=_shape, c=_c: _color_spec(s, c))
        case(f"hair_lab-{'x'.join(map(str, _shape))}-C{_c}", ("mg_hair_lab_fwd", "mg_hair_lab_bwd"))(lambda s=_shape, c=_c: _hair_spec(s, c))


def _attention_spec(dt, n, L, scale, fused):
    """test_self_attention_matches_contract's form: slices of a fused projection, the output in the second half of a wider buffer."""
    from michigan_amd import ops
    g = _gen(L)
    q, k = (torch.randn(n, L, 64, generator=g) * scale).to(DT[dt]), (torch.randn(n, L, 64, generator=g) * scale).to(DT[dt])
    v = _randn(g, n, L, 256, dt=dt)
    if L > 8:
        k[:, L - 5] = (4.0 * q[:, 7].float()).to(DT[dt])
    qkv = torch.cat([q, k, v], dim=2).contiguous()

    def fn(ctx, q, k, v, qkv):
        if fused:
            q, k, v = qkv[:, :, :64], qkv[:, :, 64:128], qkv[:, :, 128:]
        buf = ctx.buf((n, L, 512), DT[dt], zero=True)
        ops.self_attention(q, k, v, out=buf[:, :, 256:])
        return buf[:, :, 256:], buf[:, :, :256].float().abs().sum().reshape(1), ops.self_attention(q, k, v)
    tol = 2e-5 if dt == "f32" else 2.0 ** -8
    nm = f"self_attention {dt} n={n} L={L}"
    return dict(fn=fn, tensors=[q, k, v, qkv], checks=[(nm, tol), (nm + ": the other half of the rows", "equal"), (nm + " (own output)", tol)])


for _dt in ("f32", "bf16"):
    for _n, _L, _scale, _fused in [(2, 1, 1.0, False), (2, 63, 0.5, True), (1, 64, 0.2, True), (3, 65, 0.5, False), (3, 200, 0.5, True), (1, 333, 1.5, False)]:
        case(f"self_attention-{_dt}-n{_n}-L{_L}", ("mg_self_attention",))(lambda dt=_dt, n=_n, L=_L, s=_scale, f=_fused: _attention_spec(dt, n, L, s, f))


def _spectral_spec(shape, train):
    """ops.spectral_weight: mg_sn_normalize (training) / mg_sn_scale / mg_sn_bwd; u, v are the module's buffers, updated in place."""
    from michigan_amd import ops
    g = _gen(shape[0] + shape[1])
    weight = (torch.randn(*shape, generator=g) * 0.1).requires_grad_()
    u = torch.nn.functional.normalize(torch.randn(shape[0], generator=g), dim=0)
    v = torch.nn.functional.normalize(torch.randn(shape[1] * shape[2] * shape[3], generator=g), dim=0)

    def fn(ctx, weight, u, v):
        w = ops.spectral_weight(weight, u, v, train, 1e-12)
        (gw,) = torch.autograd.grad(w, weight, ctx.put(_gy(w, 4)))
        with torch.no_grad():
            w_eval = ops.spectral_weight(weight, u, v, False, 1e-12)
        return w, u, v, gw, w_eval
    return dict(fn=fn, tensors=[weight, u, v], checks=[(f"spectral {shape} train={train} {n}", 2e-5) for n in ("weight", "u", "v", "grad", "weight (no grad)")])


for _shape in [(64, 7, 4, 4), (128, 4, 3, 3), (24, 3, 3, 3)]:       # cols = 27: rows of W are not 16-byte aligned
    case(f"spectral_weight-{'x'.join(map(str, _shape))}-train", ("mg_sn_normalize", "mg_sn_scale", "mg_sn_bwd"))(lambda s=_shape: _spectral_spec(s, True))
    case(f"spectral_weight-{'x'.join(map(str, _shape))}-eval", ("mg_sn_scale", "mg_sn_bwd"))(lambda s=_shape: _spectral_spec(s, False))


def _batched_net_spec(dt, sink):
    """test_batched_spectral_norm_and_pack_match_contract's net, protocol and tolerances: mg_sn_power_iteration, mg_pack_weights,
    the gradient sink's mg_grad_drain and the arena Adam step, three optimiser iterations (the batched paths are live from the second)."""
    import torch.nn as nn
    from michigan_amd import ops
    from michigan_amd.networks import spectral
    from michigan_amd.networks.layers import HipConv2d
    from michigan_amd.networks.normalization import SPADE
    from michigan_amd.optim import FlatAdam

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.c7 = HipConv2d(8, 24, 7, padding=3)
            self.c3 = spectral.spectral_norm(HipConv2d(24, 40, 3, padding=1))
            self.c1 = spectral.spectral_norm(HipConv2d(40, 72, 1, bias=False))
            self.sp = SPADE("spadesyncbatch3x3", 72, 4)
            self.c4 = HipConv2d(72, 16, 4, stride=2, padding=2)

        def forward(self, x, seg):
            spectral.prepare(self)
            h = self.c7(x, act=ops.ACT_LRELU)
            h = self.c3(h, act=ops.ACT_RELU)
            h = self.c1(h)
            h = self.sp(h, seg, act=ops.ACT_LRELU)
            return self.c4(h)

    torch.manual_seed(6)
    sd = {k: v.clone() for k, v in Net().state_dict().items()}
    g = _gen(9)
    x = _randn(g, 2, 20, 28, 8, dt=dt)
    seg = (torch.rand(2, 4, 20, 28, generator=g) > 0.5).float()
    gy = _randn(g, 2, 11, 15, 16, dt=dt)

    def fn(ctx, x, seg, gy):
        net = Net().to(x.device)
        net.load_state_dict(sd)
        opt = FlatAdam(net.parameters(), lr=1e-3, grad_sink=sink)
        outs = []
        for it in range(3):
            opt.zero_grad()
            out = net(x, seg)
            (out.float() * gy.float()).sum().backward()
            opt.step()
            outs.append(out.detach().float().clone())
        return outs + [net.c3.weight_u.clone(), net.c1.weight_v.clone()]
    nm = f"batched net {dt} sink={sink}"
    checks = [(f"{nm}: output of pass {i}", (5e-4 if i == 0 else 3e-3) if dt == "f32" else 2.0 ** -5) for i in range(3)]
    checks += [(nm + ": u", 1e-4 if dt == "f32" else 5e-3), (nm + ": v", 1e-4 if dt == "f32" else 5e-3)]
    return dict(fn=fn, tensors=[x, seg, gy], checks=checks, flags={"WGRAD_DETERMINISTIC": True})


for _dt in ("f32", "bf16"):
    case(f"batched-net-{_dt}-sink", ("mg_sn_power_iteration", "mg_pack_weights", "mg_grad_drain", "mg_adam_step", "mg_conv_taps", "mg_conv_wgrad"))(
        lambda dt=_dt: _batched_net_spec(dt, True))
case("batched-net-f32-autograd", ("mg_sn_power_iteration", "mg_pack_weights", "mg_adam_step", "mg_unpack_wgrad", "mg_sn_bwd"))(lambda: _batched_net_spec("f32", False))


# ---- the device input pipeline (mg_inputs.hip): bit-exact, the geometries of tests/test_gpu_inputs.py ---------------------------------
def _ellipses(n, h, w, seed):
    g = _gen(seed)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    out = []
    for _ in range(n):
        cy, cx = (torch.rand(2, generator=g) * 0.2 + 0.4).tolist()
        ry, rx = (torch.rand(2, generator=g) * 0.15 + 0.2).tolist()
        out.append(((((yy - cy * h) / (ry * h)) ** 2 + ((xx - cx * w) / (rx * w)) ** 2) <= 1).to(torch.uint8))
    return torch.stack(out)


def _crop_spec(geom, mode):
    from michigan_amd import inputs
    n, hs, ws, load, c, cs = geom
    g = _gen(hs * 7 + mode)
    src = torch.randint(0, 256, (n, hs, ws, c), generator=g, dtype=torch.uint8)
    crop = torch.stack([torch.randint(0, load - cs + 1, (n,), generator=g), torch.randint(0, load - cs + 1, (n,), generator=g),
                        torch.randint(0, 2, (n,), generator=g)], dim=1).to(torch.int32)
    mul = torch.randint(0, 3, (n, 1, cs, cs), generator=g).float() if mode == 2 else None

    def fn(ctx, src, crop, mul):
        yt, xt = inputs.nearest_table(hs, load, src.device), inputs.nearest_table(ws, load, src.device)
        return (inputs.crop_u8(src, crop, cs, mode=mode, unknown_label=2 if mode == 1 else -1, ytab=yt, xtab=xt, mul=mul),)
    return dict(fn=fn, tensors=[src, crop, mul], checks=[(f"crop {geom} mode {mode}", "equal")])


def _inputs_spec(which):
    from michigan_amd import inputs
    from oracle import inputs_oracle as IO
    if which == "bicubic":
        src = torch.randint(0, 256, (1, 50, 40, 1), generator=_gen(5), dtype=torch.uint8)
        return dict(fn=lambda ctx, s: (inputs.resize_bicubic_u8(s, (37, 64)),), tensors=[src], checks=[("bicubic 50x40 -> 37x64", "equal")])
    if which == "bicubic-rgb":
        src = torch.randint(0, 256, (2, 64, 64, 3), generator=_gen(6), dtype=torch.uint8)
        return dict(fn=lambda ctx, s: (inputs.resize_bicubic_u8(s, (71, 71)),), tensors=[src], checks=[("bicubic 64x64 -> 71x71", "equal")])
    if which == "onehot":
        lab = _ellipses(3, 37, 53, 1)[:, None].float()
        lab[1, 0, :2] = 2.0
        return dict(fn=lambda ctx, l: (inputs.onehot_labels(l, 2),), tensors=[lab], checks=[("onehot 3x37x53", "equal")])
    if which == "orient_rgb":
        lab = _ellipses(2, 47, 41, 2)
        orient = (torch.arange(2 * 47 * 41) % 256).view(2, 47, 41).to(torch.uint8)
        return dict(fn=lambda ctx, o, l: (inputs.orient_to_rgb_u8(o, l, inputs.orient_rgb_table(o.device)),), tensors=[orient, lab], checks=[("orient rgb 2x47x41", "equal")])
    if which == "hole":
        mask = _ellipses(2, 31, 45, 3)
        omask = mask.clone()
        omask[-1] = _ellipses(1, 31, 45, 9)[0]
        th, u = torch.tensor([0.5, 1.2], dtype=torch.float64), torch.tensor([0.0, 0.999999], dtype=torch.float64)
        return dict(fn=lambda ctx, m, o, t, uu: inputs.generate_hole_u8(m, o, t, uu, want_info=True), tensors=[mask, omask, th, u],
                    checks=[("hole 2x31x45", "equal"), ("hole info", "equal")])
    assert which.startswith("noise")
    size = int(which[5:])
    per = sum(s * s * 3 for s in IO.noise_octave_sizes(size))
    fields = torch.randn(1, per, dtype=torch.float64, generator=_gen(size)) * 0.25 + 0.5

    def close_abs(name, a, r):
        err = (a - r).abs().max().item()
        assert math.isfinite(err) and err <= 1e-6, f"{name}: max abs err {err:.3e}"      # tests/test_gpu_inputs.py::test_noise_octaves_match_oracle
    return dict(fn=lambda ctx, f: (inputs.noise_from_fields(f, size),), tensors=[fields], checks=[(f"noise {size}", close_abs)])


for _geom, _mode in [((3, 33, 37, 45, 1, 32), 1), ((3, 33, 37, 45, 1, 32), 2), ((2, 40, 40, 40, 3, 24), 0)]:
    case(f"input_crop-{'x'.join(map(str, _geom))}-mode{_mode}", ("mg_input_crop_u8",))(lambda gm=_geom, m=_mode: _crop_spec(gm, m))
for _which, _ep in (("bicubic", "mg_resize_bicubic_u8"), ("bicubic-rgb", "mg_resize_bicubic_u8"), ("onehot", "mg_onehot_labels"), ("orient_rgb", "mg_orient_to_rgb_u8"),
                    ("hole", "mg_generate_hole_u8"), ("noise40", "mg_noise_octaves"), ("noise100", "mg_noise_octaves")):
    case(f"inputs-{_which}", (_ep,))(lambda w=_which: _inputs_spec(w))


# =====================================================================================================================
@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_guarded(c):
    _run(c.build(), c.covers)


def test_zz_report():
    """Last in the file: what the run covered (printed with -s; recorded in DESIGN.md)."""
    print("guard bands: %d cases, %d guarded allocations checked, %.1f s in the guarded runs and their references"
          % (STATS["cases"], STATS["allocations"], STATS["seconds"]))
    assert len({c.id for c in CASES}) == len(CASES), "duplicate case ids"
