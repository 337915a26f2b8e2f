"""-m gpu: the two bodies of the few-output "dot" convolution route (csrc/mg_conv_dot.hip), bit for bit.

Stride-1 tap sets inside a 4 x 4 window -- the 4x4 s1 p2 heads of the patch discriminators -- run on 8 x 8 output tiles with the input
patch staged through LDS in channel slices; everything else the route admits keeps the wave-per-pixel body.  The operands are those of
tests/test_gpu_exact_sums.py's ``dot-head`` case (tests/exact_operands.py: every product and partial sum an integer below 2^24), so
fp32 accumulation is exact in any order and every output must be ``torch.equal`` to the float64 reference rounded once.  No tolerance.

  * 512 channels -> 1 at 33 x 35 (34 x 36 outputs: ragged against the 8 x 8 tile both ways, and against the 4-output strips) and at
    8 x 70 with N = 3 (one tile row with a partial second one, nine tile columns, the image index in the block decode);
  * 128 channels -> 3 (one channel slice in bf16, two in fp32; three outputs per pixel);
  * fp32 and bf16; bias + LeakyReLU and residual;
  * a stride-2 3x3 case, which has to stay on the wave-per-pixel body.
MG_TEST_DRYRUN=1 runs the contract emulator in place of the GPU (plumbing and precondition check on a machine without one).
"""
import os

import pytest
import torch

import exact_operands as X
from test_gpu_guard_bands import _conv_path

pytestmark = pytest.mark.gpu

DRY = os.environ.get("MG_TEST_DRYRUN") == "1"
DEV = "cpu" if DRY else "cuda"

_G = lambda cin, cout, k, s, p, H, W, N: dict(cin=cin, cout=cout, k=k, s=s, p=p, H=H, W=W, N=N)
CASES = [
    ("head-33x35", _G(512, 1, 4, 1, 2, 33, 35, 1)),
    ("head-8x70-n3", _G(512, 1, 4, 1, 2, 8, 70, 3)),
    ("cin128-cout3", _G(128, 3, 4, 1, 2, 13, 18, 2)),
    ("stride2-3x3", _G(128, 1, 3, 2, 1, 31, 37, 2)),          # wave-per-pixel body
]
EPI = {"lrelu": dict(act="lrelu", bias=True, resid=False), "resid": dict(act="none", bias=False, resid=True)}
for _id, _g in CASES:
    for _dt in ("f32", "bf16"):
        for _e in EPI.values():
            assert _conv_path(_dt, act=_e["act"], resid=_e["resid"], **_g) == "dot", (_id, _dt)


@pytest.fixture
def backend(request):
    return request.getfixturevalue("emulator_backend" if DRY else "hip_backend")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("cid,geom", CASES, ids=[c[0] for c in CASES])
def test_dot_route_rounds_once_on_both_bodies(backend, cid, geom, dt):
    k, s, p = geom["k"], geom["s"], geom["p"]
    o = X.conv_operands(dt, **geom, bias=True, resid=True, density=8192.0, tilt=0.02)
    ref = X.ConvReference(o, k, s, p, torch.float64, name=f"{cid} {dt}")
    failures = []
    for e, epi in EPI.items():
        want, share = ref.forward(dt=dt, **epi)
        got = X.run_conv(o, k, s, p, act=epi["act"], dev=DEV, with_grads=False, bias=epi["bias"], resid=epi["resid"])
        print(f"[dot tiles] {cid}-{dt}-{e}: {share:.1%} of the outputs need rounding in bf16")
        try:
            X.assert_bits(f"{cid} {dt} {e} y", got["y"], want, X.DT[dt])
        except AssertionError as err:
            failures.append(str(err))
    assert not failures, "\n".join(failures)
