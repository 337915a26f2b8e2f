"""-m gpu: every route of the convolution family held to ONE rounding, bit for bit.

The value tests (tests/test_gpu_kernels.py and the guard-band cases that reuse its form) bound |hip - ref| by a multiple of
max|ref|: for the bf16-only kernels that is one bf16 ulp at the top of the range, several binades above a typical element's own
rounding, and an accumulator narrowed on the way, a bias added after the store conversion or a truncating conversion all pass it.
Here the operands (tests/exact_operands.py) make every product and partial sum an integer below 2^24, so fp32 accumulation is
exact in ANY order and the only rounding left is the store conversion: every output and every gradient must satisfy
``torch.equal(hip, float64_reference.to(dtype))``.  There is no tolerance in this file.

  * forward and autograd gradients through ``ops.conv2d`` on each of the 15 routes of dispatch_conv (the route arithmetic is
    tests/test_gpu_guard_bands.py's ``_conv_path``, asserted per case and epilogue when this module is imported), in the dtypes a
    route exists in, the option-off twins and the wide-store cases included; epilogues bias + LeakyReLU(0.25), bias + ReLU and
    residual wherever the route takes them.  The gradients are those of the FUSED activation: with exact arithmetic the sign of the
    pre-activation is exact, so the reference's branch is the kernel's.
  * the data gradient with a given mask (``ops.conv_dgrad(relu_mask=, mask_slope=)``) at slopes 0 and 0.25, and stride-2 data
    gradients (4x4 s2 p2, 3x3 s2 p1: every output-parity class) that end in 8 and in 64 channels.
  * ``ops.conv_wgrad`` on its own over the guard-band table's WGRAD_PATHS, with fp32 atomics and with ops.set_deterministic(True),
    with and without the fused bias gradient: both orders must equal the reference, and so each other.
  * the SPADE epilogue (``ops.spade_modulate`` with a GIVEN mean / rstd; one x_up case through spade_modulate_pair): h and the
    gradients with respect to actv, both weights and both biases.  The gradient with respect to x is not compared HERE: it is
    held bit for bit in tests/test_gpu_census.py, whose caller's count is a power of two and whose reference reads (1 + gamma)
    in its stored form, together with the norm backward's reductions and applies on their own.

The reference is torch on the CPU in float64; the chip-filling cases use the fp32 CPU convolution, which returns the same bits once
the exactness precondition holds (tests/test_exact_operands.py asserts that equality).  Preconditions (exactness, >= 5 % of bf16
outputs need rounding, >= 100 distinct values, <= half zeros) are asserted on the reference before a kernel's result is looked at.
MG_TEST_DRYRUN=1 runs the contract emulator in place of the GPU (plumbing and precondition check on a machine without one).
"""
import functools
import os

import pytest
import torch

import exact_operands as X
from test_gpu_guard_bands import CONV_PATHS, WGRAD_PATHS, _conv_path, _settings

pytestmark = pytest.mark.gpu

DRY = os.environ.get("MG_TEST_DRYRUN") == "1"
DEV = "cpu" if DRY else "cuda"


@pytest.fixture
def backend(request):
    return request.getfixturevalue("emulator_backend" if DRY else "hip_backend")


class _Report:
    """Collects every mismatch of a case, so that one run names them all."""

    def __init__(self):
        self.failures = []

    def bits(self, name, got, want, dtype):
        try:
            X.assert_bits(name, got, want, dtype)
        except AssertionError as e:
            self.failures.append(str(e))

    def done(self):
        assert not self.failures, "\n".join(self.failures)


# =====================================================================================================================
# forward + autograd gradients, one case per route
# =====================================================================================================================
EPI = {"lrelu": dict(act="lrelu", bias=True, resid=False), "relu": dict(act="relu", bias=True, resid=False), "resid": dict(act="none", bias=False, resid=True)}
ALL3, NO_AUX = ("lrelu", "relu", "resid"), ("lrelu", "relu")      # thin, thin-taps and few-output take no residual; halo64 one only without activation
_G = lambda cin, cout, k, s, p, H, W, N: dict(cin=cin, cout=cout, k=k, s=s, p=p, H=H, W=W, N=N)
# holes: images whose border is under 5 % of the pixels (exact_operands: the pair fails to cancel there as it does at a border)
# id, dtypes, route (per dtype where they differ), geometry, epilogues, operand / option extras
ROUTES = [
    ("thin", ("bf16",), "thin", _G(8, 64, 3, 1, 1, 45, 96, 4), NO_AUX, dict(holes=0.15)),
    ("thin-cout128", ("bf16",), "thin", _G(8, 128, 3, 1, 1, 61, 128, 4), NO_AUX, dict(holes=0.15)),
    ("thin-taps-4x4s2", ("bf16",), "thin-taps", _G(8, 64, 4, 2, 2, 128, 96, 4), NO_AUX, dict(holes=0.15)),       # dx: four parity classes, few-output launches
    ("thin-taps-3x3s2", ("bf16",), "thin-taps", _G(8, 64, 3, 2, 1, 140, 192, 3), NO_AUX, dict(holes=0.15)),      # dx: few-output launches, 3 x 70 x 96 pixels per class
    ("thin-taps-5x5", ("bf16",), "thin-taps", _G(8, 64, 5, 1, 2, 67, 100, 2), NO_AUX, dict(holes=0.15)),
    ("few-output", ("bf16",), "few-output", _G(64, 3, 3, 1, 1, 72, 100, 3), NO_AUX, dict(holes=0.15)),
    ("dot-head", ("f32", "bf16"), "dot", _G(512, 1, 4, 1, 2, 9, 9, 4), ALL3, dict(density=8192.0, tilt=0.02)),      # one output channel: a dense, tilted kernel (exact_operands.conv_operands)
    ("halo64", ("bf16",), "halo64", _G(64, 64, 3, 1, 1, 512, 512, 1), ALL3, dict(holes=0.15)),
    ("halo64-off", ("bf16",), "halo-64rows", _G(64, 64, 3, 1, 1, 512, 512, 1), ("lrelu",), dict(holes=0.15, opts={"OPT_CONV_HALO64": 0})),
    ("halo-64rows-ragged", ("f32", "bf16"), "halo-64rows", _G(64, 64, 3, 1, 1, 203, 181, 3), ALL3, dict(holes=0.15)),
    ("halo-16x16-ragged", ("bf16",), "halo-16x16", _G(32, 200, 3, 1, 1, 150, 210, 4), ALL3, dict(holes=0.15, opts={"OPT_CONV_HALO_BIG": 1})),
    ("halo-8x16-ragged", ("f32", "bf16"), "halo-8x16", _G(256, 136, 3, 1, 1, 97, 131, 2), ALL3, dict(holes=0.15, opts={"OPT_CONV_HALO_BIG": 0})),
    ("tile256", ("bf16",), "tile256", _G(128, 512, 4, 1, 2, 127, 129, 3), ALL3, dict(holes=0.15, opts={"OPT_CONV_BIGTILES": 1})),
    ("tile256-off", ("bf16",), "tile128", _G(128, 512, 4, 1, 2, 127, 129, 3), ("lrelu",), dict(holes=0.15, opts={"OPT_CONV_BIGTILES": 0})),
    ("tile128", ("f32", "bf16"), {"bf16": "tile128", "f32": "tile128-splitk"}, _G(128, 128, 3, 1, 1, 24, 20, 2), ALL3, {}),
    ("tile128-ktail-ragged-cout", ("f32", "bf16"), "tile128", _G(48, 200, 3, 1, 1, 9, 13, 2), ALL3, {}),
    ("tile64", ("f32", "bf16"), "tile64", _G(64, 64, 3, 1, 1, 33, 17, 1), ALL3, {}),
    ("tile32-cout3", ("f32",), "tile32", _G(64, 3, 3, 1, 1, 20, 20, 2), ALL3, dict(density=256.0)),
    ("packed-taps", ("f32", "bf16"), {"bf16": "tile32-packed-taps", "f32": "tile32"}, _G(16, 32, 3, 1, 1, 12, 12, 2), ALL3, {}),
    ("packed-taps-49", ("f32",), "tile128-packed-taps", _G(8, 128, 7, 1, 3, 14, 14, 1), ALL3, {}),
    ("packed-taps-49-cout136", ("bf16",), "tile128-packed-taps", _G(8, 136, 7, 1, 3, 14, 14, 1), ALL3, {}),
    ("stride2-odd", ("f32",), "tile64-packed-taps", _G(8, 64, 4, 2, 2, 21, 19, 2), ALL3, {}),
    ("stride2-odd-cout72", ("bf16",), "tile128-packed-taps", _G(8, 72, 4, 2, 2, 21, 19, 2), ALL3, {}),
    ("splitk", ("f32", "bf16"), "tile128-splitk", _G(2048, 128, 3, 1, 1, 8, 8, 2), ALL3, {}),
    ("splitk-ragged", ("f32", "bf16"), "tile128-splitk", _G(512, 200, 3, 1, 1, 7, 5, 5), ALL3, {}),
    ("splitk-off", ("bf16",), "tile128", _G(512, 200, 3, 1, 1, 7, 5, 5), ALL3, dict(opts={"OPT_CONV_SPLITK": 0})),
    # 16-byte stores with Cout % 8 == 0 and == 4, their quad-store twin, on a generic and on a halo shape
    ("wide-cout72", ("bf16",), "tile128", _G(64, 72, 4, 2, 1, 33, 29, 2), ALL3, dict(holes=0.15, opts={"OPT_CONV_WIDE": 1})),
    ("wide-cout76", ("bf16",), "tile128", _G(64, 76, 4, 2, 1, 33, 29, 2), ALL3, dict(holes=0.15, opts={"OPT_CONV_WIDE": 1})),
    ("wide-off-cout72", ("bf16",), "tile128", _G(64, 72, 4, 2, 1, 33, 29, 2), ALL3, dict(holes=0.15, opts={"OPT_CONV_WIDE": 0})),
    ("wide-halo-cout132", ("bf16",), "halo-8x16", _G(64, 132, 3, 1, 1, 48, 67, 8), ALL3, dict(holes=0.15, opts={"OPT_CONV_WIDE": 1})),
    # stride-2 data gradients that end in a 64-channel input, odd sizes: every parity class has its own extent
    ("stride2-4x4-cin64", ("f32", "bf16"), {"bf16": "tile128", "f32": "tile128-splitk"}, _G(64, 128, 4, 2, 2, 17, 17, 2), ALL3, {}),
    ("stride2-3x3-cin64", ("f32", "bf16"), "tile128", _G(64, 72, 3, 2, 1, 17, 19, 2), ALL3, {}),
]
ROUTE_PARAMS = []
for _id, _dts, _path, _geom, _epis, _extra in ROUTES:
    for _dt in _dts:
        _w = _path[_dt] if isinstance(_path, dict) else _path
        for _e in _epis:
            _got = _conv_path(_dt, act={"lrelu": "lrelu", "relu": "relu", "resid": "none"}[_e], resid=EPI[_e]["resid"], opts=_extra.get("opts"), **_geom)
            assert _got == _w, (_id, _dt, _e, _got, _w)
        ROUTE_PARAMS.append(pytest.param(_id, _dt, _geom, _epis, _extra, id=f"{_id}-{_dt}"))
# the dx launches of the two thin-taps stride-2 cases: per parity class a stride-1 gather over 64 channels into 8.  4x4 s2: 2 x 2 taps
# onto 64 x 48 pixels (a 2 x 2 window without padding over a 65 x 49 grid has that extent); 3x3 s2: at most 2 x 2 of the 3 x 3 window's
# taps onto 70 x 96 pixels.  Either tap set lies inside a 3 x 3 window, which is all the few-output kernel asks of it (k <= 3).
assert _conv_path("bf16", 64, 8, 2, 1, 0, 65, 49, 4, act="none") == "few-output" and _conv_path("bf16", 64, 8, 3, 1, 1, 70, 96, 3, act="none") == "few-output"
assert ({"thin", "thin-taps", "dot", "few-output", "halo64", "halo-64rows", "halo-16x16", "halo-8x16", "tile256", "tile128", "tile128-splitk", "tile64", "tile32",
         "tile32-packed-taps", "tile128-packed-taps"}
        <= {q for _, _, pth, *_r in ROUTES for q in (pth.values() if isinstance(pth, dict) else (pth,))}), "a route of dispatch_conv has no case"
# the option-off twins and the wide-store cases of the guard-band table are here at the table's own geometry (N = 5 for the ragged split-K
# shape: 35 pixels give a ReLU'd weight gradient fewer than 100 distinct values, 105 a 200-channel bias gradient fewer than 50)
_TABLE = {i: kw for i, _, _, kw in CONV_PATHS}
for _id in ("halo64-off", "tile256-off", "splitk-off", "wide-cout72", "wide-cout76", "wide-off-cout72", "wide-halo-cout132"):
    _mine = {i: (g, x) for i, _, _, g, _, x in ROUTES}[_id]
    assert all(_TABLE[_id][n] == v for n, v in _mine[0].items() if n != "N") and _TABLE[_id]["opts"] == _mine[1]["opts"], _id


def _ref_dtype(geom):
    """float64, or the fp32 CPU convolution for the chip-filling cases (same bits under the exactness precondition)."""
    ho, wo = (geom["H"] + 2 * geom["p"] - geom["k"]) // geom["s"] + 1, (geom["W"] + 2 * geom["p"] - geom["k"]) // geom["s"] + 1
    macs = geom["N"] * ho * wo * geom["cout"] * geom["cin"] * geom["k"] ** 2
    return torch.float64 if macs < 2e9 else torch.float32


@pytest.mark.parametrize("cid,dt,geom,epis,extra", ROUTE_PARAMS)
def test_conv_route_rounds_once(backend, cid, dt, geom, epis, extra):
    k, s, p = geom["k"], geom["s"], geom["p"]
    o = X.conv_operands(dt, **geom, bias=True, resid=True, holes=extra.get("holes", 0.0), density=extra.get("density", 64.0), tilt=extra.get("tilt", 0.0))
    b_relu = X.ints(X._gen(11), o["b"].shape, 0, 8)                 # ReLU alone takes its bias from [0, 8] (at most half of the outputs zero); LeakyReLU from [-8, 8]
    ref = X.ConvReference(o, k, s, p, _ref_dtype(geom), name=f"{cid} {dt}")
    rep = _Report()
    with _settings(extra.get("opts", {}), {}):
        for e in epis:
            epi = dict(EPI[e], bias=b_relu) if e == "relu" else EPI[e]
            want_y, share = ref.forward(dt=dt, **epi)
            want = dict(ref.grads(**epi), y=want_y)
            got = X.run_conv(o, k, s, p, act=epi["act"], dev=DEV, bias=epi["bias"], resid=epi["resid"])
            assert set(got) == set(want), (sorted(got), sorted(want))
            for n in ("y", "dx", "dw", "db", "dres"):
                if n in want:
                    rep.bits(f"{cid} {dt} {e} {n}", got[n], want[n], X.out_dtype(n, dt))
            print(f"[exact-sum] {cid}-{dt}-{e}: {share:.1%} of the outputs need rounding in bf16")
    rep.done()


# =====================================================================================================================
# the data gradient with a GIVEN mask in its epilogue
# =====================================================================================================================
MASK_GEOMS = [("f32", (2, 40, 48, 128, 128)), ("bf16", (2, 40, 48, 128, 128)), ("bf16", (1, 512, 512, 64, 64)), ("bf16", (2, 97, 131, 136, 256))]
for _dt, _gm in MASK_GEOMS:          # the launch: dy [cout channels] -> dx [cin channels]
    assert _conv_path(_dt, _gm[4], _gm[3], 3, 1, 1, _gm[1], _gm[2], _gm[0], act="none", mask=True) == {40: "tile128" if _dt == "bf16" else "tile128-splitk", 512: "halo64", 97: "halo-8x16"}[_gm[1]]


@pytest.mark.parametrize("dt,gm", MASK_GEOMS, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_masked_data_gradient_rounds_once(backend, dt, gm):
    """test_data_gradient_with_folded_activation_mask's call at slopes 0 and 0.25: the tile128 shape, a halo64 shape and the ragged
    8 x 16 halo shape.  acc -> x mask -> one conversion; the plain data gradient of the same launch alongside."""
    from michigan_amd import ops
    n, h, w, cin, cout = gm
    o = X.conv_operands(dt, cin, cout, 3, 1, 1, h, w, n, bias=False, holes=0.15 if h > 90 else 0.0)
    ref = X.ConvReference(o, 3, 1, 1, _ref_dtype(dict(cin=cin, cout=cout, k=3, s=1, p=1, H=h, W=w, N=n)), name=f"dgrad {gm} {dt}")
    dx = ref.grads("none", bias=False)["dx"]
    sign = X.ints(X._gen(5), (n, h, w, cin), -2, 2)                  # the activation output the conv consumed: only its sign matters
    rep = _Report()
    dy, mask = o["gy"].to(DEV), sign.to(X.DT[dt]).to(DEV)
    wt = ops.pack_weight(o["w"].to(DEV), None, X.DT[dt], ops._roundup(cin, 128), cout, 1)
    rep.bits(f"dgrad {gm} {dt} plain", ops.conv_dgrad(dy, wt, 3, 3, 1, 1, (h, w), cin), dx, X.DT[dt])
    for slope in (0.0, X.SLOPE):
        masked = ops.conv_dgrad(dy, wt, 3, 3, 1, 1, (h, w), cin, relu_mask=mask, mask_slope=slope)
        ops._RELU_MASKED.pop(masked.data_ptr(), None)
        want = torch.where(sign.double() > 0, dx, dx * slope)
        X.check_distinct(f"dgrad {gm} slope {slope}", want)
        rep.bits(f"dgrad {gm} {dt} mask slope {slope}", masked, want, X.DT[dt])
    rep.done()


# =====================================================================================================================
# weight gradients on their own
# =====================================================================================================================
@functools.lru_cache(maxsize=None)
def _wgrad_case(dt, geom):
    g = dict(geom)
    o = X.wgrad_operands(dt, **g)
    return o, X.wgrad_reference(o, g["k"], g["s"], g["p"], name=f"wgrad {dt} {geom}")


WGRAD_PARAMS = [pytest.param(dt, tuple(sorted((k, v) for k, v in kw.items() if k in ("N", "H", "W", "cin", "cg", "k", "s", "p"))), kw.get("opts") or {}, kw.get("flags") or {},
                             id=id_) for id_, dt, kw in WGRAD_PATHS]
assert len(WGRAD_PARAMS) == 16, len(WGRAD_PARAMS)       # generic x 2 fragment paths, fp32 4x4 s2, thin x 2, thin-taps, 3x3 kernel: 5 shapes x 2 stripe settings


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("dt,geom,opts,flags", WGRAD_PARAMS)
def test_weight_gradient_sums_exactly(backend, dt, geom, opts, flags, det):
    """ops.conv_wgrad with and without the fused bias gradient: fp32 atomics and the slab order both give the exact sum."""
    from michigan_amd import ops
    o, ref = _wgrad_case(dt, geom)
    g = dict(geom)
    rep = _Report()
    prev = ops.set_deterministic(det)
    try:
        with _settings(opts, flags):
            for want_bias in (True, False):
                got = X.run_wgrad(o, g["k"], g["s"], g["p"], want_bias, dev=DEV)
                for n in got:
                    rep.bits(f"wgrad {dt} {geom} det={det} bias={want_bias} {n}", got[n], ref[n], torch.float32)
    finally:
        ops.set_deterministic(prev)
    rep.done()


# =====================================================================================================================
# SPADE epilogue
# =====================================================================================================================
SPADE_SHAPES = [(48, 9, 11, False), (64, 20, 24, False), (136, 97, 131, False), (64, 36, 44, True)]
SPADE_N, SPADE_CA = 2, 128
for _dt in ("f32", "bf16"):         # the SPADE launch is a 3x3 conv of the 128-channel actv into 2 * roundup(C, 32) interleaved gamma | beta rows
    for _C, _H, _W, _up in SPADE_SHAPES:
        _route = _conv_path(_dt, SPADE_CA, 2 * ((_C + 31) // 32 * 32), 3, 1, 1, _H, _W, SPADE_N, act="lrelu")
        assert _route.startswith("halo-") == (_C == 136), (_dt, _C, _H, _W, _route)       # (136, 97, 131) at N = 2: the halo kernel; the others: generic tiles


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("C,H,W,up", SPADE_SHAPES, ids=str)
def test_spade_epilogue_rounds_once(backend, C, H, W, up, dt):
    """(136, 97, 131): the ragged halo SPADE shape.  up: x enters through the fused nearest-2x index map (spade_modulate_pair)."""
    o = X.spade_operands(dt, C, H, W, N=SPADE_N, ca=SPADE_CA, up=up, holes=0.15 if H * W > 5000 else 0.0)
    ref, share = X.spade_reference(o, act="lrelu", up=up, dt=dt, name=f"spade C={C} {H}x{W} {dt}")
    got = X.run_spade(o, act="lrelu", up=up, dev=DEV)
    rep = _Report()
    for n in ("h", "dactv", "dwg", "dbg", "dwb", "dbb"):
        rep.bits(f"spade C={C} {H}x{W} up={up} {dt} {n}", got[n], ref[n], X.out_dtype(n, dt))
    print(f"[exact-sum] spade-C{C}-{H}x{W}-up{int(up)}-{dt}: {share:.1%} of the outputs need rounding in bf16")
    rep.done()
