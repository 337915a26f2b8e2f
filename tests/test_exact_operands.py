"""CPU: the exact-sum operand recipe (tests/exact_operands.py) checked on both of its sides.

1. Reference cross-check: ``ops.*`` on the float64 contract emulator equals the once-rounded float64 torch reference bit for bit,
   with the recipe's preconditions asserted -- this pins the reference side of tests/test_gpu_exact_sums.py without a GPU.
2. The test of the test: a plain-torch tap-loop convolution carrying each of four precision faults the max-norm value tests let
   through must NOT equal the reference on the recipe's operands.  An edit to the recipe that lets a mutant pass fails here.
"""
import pytest
import torch

import exact_operands as X

# cin, cout, k, stride, pad, H, W, N
SHAPES = [(64, 64, 3, 1, 1, 33, 17, 1), (48, 200, 3, 1, 1, 9, 13, 2), (8, 64, 4, 2, 2, 21, 19, 2), (16, 32, 3, 1, 1, 12, 12, 2)]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda c: "x".join(map(str, c)))
def test_emulator_equals_the_once_rounded_float64_reference(emulator_backend, shape, dt):
    """Forward with bias + LeakyReLU(0.25) and every autograd gradient; (8, 64, 4, 2, 2, ...) is the stride-2 data gradient."""
    cin, cout, k, s, p, H, W, N = shape
    o = X.conv_operands(dt, cin, cout, k, s, p, H, W, N)
    ref, share = X.conv_reference(o, k, s, p, act="lrelu", dt=dt, name=f"conv {shape} {dt}")
    got = X.run_conv(o, k, s, p, act="lrelu")
    assert set(got) == set(ref) == {"y", "dx", "dw", "db"}
    for n in got:
        X.assert_bits(f"conv {shape} {dt} {n}", got[n], ref[n], X.out_dtype(n, dt))
    # the fp32 CPU convolution returns the same bits once the exactness precondition holds (the chip-filling GPU cases use it)
    ref32, _ = X.conv_reference(o, k, s, p, act="lrelu", dt=dt, ref_dtype=torch.float32)
    for n in ref:
        assert torch.equal(ref32[n].double(), ref[n]), n


@pytest.mark.parametrize("act,bias,resid", [("relu", True, False), ("none", False, True)], ids=["bias-relu", "resid"])
def test_emulator_epilogues(emulator_backend, act, bias, resid):
    o = X.conv_operands("bf16", 64, 96, 3, 1, 1, 12, 12, 2, bias=bias, resid=resid, bias_lo=0 if act == "relu" else -8)
    ref, _ = X.conv_reference(o, 3, 1, 1, act=act, name=f"conv {act}")
    got = X.run_conv(o, 3, 1, 1, act=act)
    assert set(got) == set(ref)
    for n in got:
        X.assert_bits(f"conv {act} bias={bias} resid={resid} {n}", got[n], ref[n], X.out_dtype(n, "bf16"))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_emulator_weight_gradient_on_its_own(emulator_backend, dt):
    geom = dict(N=2, H=19, W=23, cin=136, cg=200, k=3, s=1, p=1)
    o = X.wgrad_operands(dt, **geom)
    ref = X.wgrad_reference(o, 3, 1, 1)
    got = X.run_wgrad(o, 3, 1, 1, want_bias=True)
    for n in ("dw", "db"):
        X.assert_bits(f"wgrad {dt} {n}", got[n], ref[n], torch.float32)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("up", [False, True], ids=["plain", "x_up"])
def test_emulator_spade(emulator_backend, dt, up):
    C, H, W = (64, 12, 16) if up else (48, 9, 11)
    o = X.spade_operands(dt, C, H, W, up=up)
    ref, _ = X.spade_reference(o, act="lrelu", up=up, dt=dt)
    got = X.run_spade(o, act="lrelu", up=up)
    for n in ref:
        X.assert_bits(f"spade {dt} up={up} {n}", got[n], ref[n], X.out_dtype(n, dt))


# ---------------------------------------------------------------------------------------------------------------------
# mutants
# ---------------------------------------------------------------------------------------------------------------------
def _truncate_bf16(v):
    return (v.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def _tap_loop_conv(x, w, b, mutant=None):
    """3x3 / stride 1 / pad 1 convolution + bias of bf16 operands, one tap after another into an fp32 accumulator, ONE
    round-to-nearest-even at the store -- and the four ways of getting that wrong."""
    n, h, wd, cin = x.shape
    xp = torch.nn.functional.pad(x.float(), (0, 0, 1, 1, 1, 1))
    wq = w.to(torch.bfloat16).float()
    acc = torch.zeros(n, h, wd, w.shape[0])
    for t in range(9):
        ky, kx = divmod(t, 3)
        acc = acc + xp[:, ky:ky + h, kx:kx + wd] @ wq[:, :, ky, kx].t()
        if mutant == "per-tap bf16 accumulator":
            acc = acc.to(torch.bfloat16).float()
        if mutant == "split partial stored as bf16" and t == 4:               # two K splits: taps 0-4 | taps 5-8
            part, acc = acc.to(torch.bfloat16).float(), torch.zeros_like(acc)
    if mutant == "split partial stored as bf16":
        acc = acc + part
    if mutant == "bias after the rounding":
        return (acc.to(torch.bfloat16).float() + b).to(torch.bfloat16)
    if mutant == "truncating conversion":
        return _truncate_bf16(acc + b)
    return (acc + b).to(torch.bfloat16)


MUTANTS = ["per-tap bf16 accumulator", "split partial stored as bf16", "bias after the rounding", "truncating conversion"]
MUTANT_SHAPES = [(64, 64, 33, 17, 1), (8, 64, 45, 96, 1), (512, 200, 7, 5, 1)]


@pytest.mark.parametrize("shape", MUTANT_SHAPES, ids=lambda c: "x".join(map(str, c)))
def test_every_mutant_is_rejected(shape):
    cin, cout, H, W, N = shape
    o = X.conv_operands("bf16", cin, cout, 3, 1, 1, H, W, N)
    ref, share = X.conv_reference(o, 3, 1, 1, with_grads=False, name=f"conv {shape}")
    want = ref["y"].to(torch.bfloat16)
    assert torch.equal(_tap_loop_conv(o["x"], o["w"], o["b"]), want), "the unmutated tap loop must equal the reference"
    for m in MUTANTS:
        got = _tap_loop_conv(o["x"], o["w"], o["b"], m)
        differ = float((got != want).float().mean())
        print(f"{shape} {m}: {differ:.1%} of the outputs differ ({share:.1%} need rounding)")
        assert not torch.equal(got, want), f"{shape}: the mutant '{m}' equals the reference -- the recipe no longer rejects it"
