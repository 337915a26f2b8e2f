"""GPU (-m gpu): mgl_orient_dog_fwd / mgl_orient_dog_bwd (michigan_amd/csrc/mg_orient_dog.hip) against the float64 contract of
tests/orient_dog_fixtures.py, whose module docstring derives the comparison rules used here.

(a) exact operands: every product and sum is exact, so both losses, M, the other scalars, dconf and a second run are torch.equal to the
    once-rounded float64 value; (b) at N = 2 with 5 x 7, 16 x 16, 1 x 257 and 384 x 384 pixels, the maximum at the first pixel, the last,
    inside the last (partial) block and in sample 1 under an empty sample 0, the hair a strided plane of a one-hot and a contiguous map,
    1- and 2-plane labels; (c) realistic operands, scalars by the 1e-4 rule and dconf per element; (d) a two-way tie of M, and M == 0
    (finite operands whose results are NaN); (e) out, ws and dconf inside guard bands; (f) L1OLoss(dog) on the reference's fixture, fp32
    and bf16 image, values and the image gradient."""
import argparse
import math

import pytest
import torch

import orient_dog_fixtures as DF
from guard_alloc import guard

pytestmark = pytest.mark.gpu

G_O, G_C = 0.75, 1.5                    # dyadic upstream gradients


def _run(o, g_o=G_O, g_c=G_C, alloc=None):
    """the two entry points through the operator layer on the device -> (out[8] as saved for the backward, dconf), on the host"""
    from michigan_amd import ops
    R = o["R"].cuda().requires_grad_(True)
    sem = o["sem"].cuda()
    hair = sem[:, 1] if o["m"].data_ptr() == o["sem"][:, 1].data_ptr() else o["m"].cuda()
    lo, lc = ops.orient_loss_dog(R, o["idx"].cuda(), o["label"].cuda(), hair)
    out = lo.grad_fn.saved_tensors[4] if hasattr(lo.grad_fn, "saved_tensors") else None
    loss = (lo * g_o if g_o is not None else 0) + (lc * g_c if g_c is not None else 0)
    loss.backward()
    torch.cuda.synchronize()
    return torch.stack([lo.detach(), lc.detach()]).cpu(), (out.cpu() if out is not None else None), R.grad.cpu()


def _once_rounded(o, g_o=G_O, g_c=G_C):
    want = torch.tensor(DF.contract(o["R"], o["idx"], o["label"], o["m"]), dtype=torch.float64).float()
    return want, DF.gradient(o["R"], o["idx"], o["label"], o["m"], g_o, g_c).float()


# ---- (a) + (b) exact operands at every shape and position of the maximum ---------------------------------------------------------------------
@pytest.mark.parametrize("where", DF.WHERE)
@pytest.mark.parametrize("shape", DF.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exact_operands_are_bit_exact(hip_backend, shape, where):
    o = DF.exact_operands(*shape, seed=sum(shape) + len(where), max_at=where)
    want_out, want_d = _once_rounded(o)
    assert float(want_out[3]) == 8.0 and float(want_out[4]) == 1.0
    losses, out, d = _run(o)
    print("out", out.tolist(), "want", want_out.tolist())
    assert torch.equal(out, want_out) and torch.equal(losses, want_out[:2])
    assert torch.equal(d, want_d)
    if where == "sample1":
        assert not bool(d[0].any())                                    # no hair in sample 0: no gradient there
    losses2, out2, d2 = _run(o)
    assert torch.equal(out2, out) and torch.equal(d2, d)               # a second run: the same bits
    for g_o, g_c in ((2.0, None), (None, 0.5)):
        _, _, d1 = _run(o, g_o, g_c)
        assert torch.equal(d1, _once_rounded(o, g_o, g_c)[1]), (g_o, g_c)


# ---- (b) + (c) realistic operands ------------------------------------------------------------------------------------------------------------
def _check_realistic(o, g_o=0.7, g_c=1.3):
    want = DF.contract(o["R"], o["idx"], o["label"], o["m"])
    losses, out, d = _run(o, g_o, g_c)
    print("out", out.tolist(), "want", want)
    assert float(out[3]) == want[3] == 6.5 and float(out[4]) == want[4] and float(out[2]) == want[2]      # M, the count and sum m are exact
    for i in (0, 1):
        assert DF.scalar_close(out[i], want[i], DF.SCALAR_TOL["f32"]), (i, float(out[i]), want[i])
    hair_c1 = float((o["R"].double() * o["m"].double()).sum())
    for i in (5, 6):                                                   # A and B: the sums behind the path through the maximum
        assert abs(float(out[i]) - want[i]) <= ((DF.n_seq(o["R"].numel()) + 12) * DF.U * 1.42 + 4 * DF.E_F) * hair_c1 + DF.U * abs(want[i]), i
    wd = DF.gradient(o["R"], o["idx"], o["label"], o["m"], g_o, g_c)
    err, bound = (d.double() - wd).abs(), DF.dconf_bound(o["R"], o["idx"], o["label"], o["m"], g_o, g_c)
    print("dconf: max err %.3e, largest %.3e, worst err / bound %.3f" % (float(err.max()), float(wd.abs().max()), float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all())
    return out, d


@pytest.mark.parametrize("hair", ["strided", "contig"])
@pytest.mark.parametrize("label_ch", [1, 2])
@pytest.mark.parametrize("shape", DF.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_realistic_operands_against_the_contract(hip_backend, shape, label_ch, hair):
    where = DF.WHERE[(DF.SHAPES.index(shape) + label_ch + (hair == "contig")) % 4]
    o = DF.operands(*shape, label_ch, seed=7 * sum(shape) + label_ch, max_at=where, hair=hair)
    _check_realistic(o)


@pytest.mark.parametrize("where", DF.WHERE)
def test_positions_of_the_maximum(hip_backend, where):
    for shape in ((2, 1, 257), (2, 16, 16)):
        _check_realistic(DF.operands(*shape, 2, seed=31 + len(where), max_at=where))


# ---- (d) a tie of M, and M == 0 ----------------------------------------------------------------------------------------------------------------
def test_two_way_tie_of_the_maximum(hip_backend):
    o = DF.exact_operands(2, 16, 16, seed=5, max_at="tail", ties=2)
    want_out, want_d = _once_rounded(o)
    assert float(want_out[4]) == 2.0
    _, out, d = _run(o)
    assert torch.equal(out, want_out) and torch.equal(d, want_d)
    a, b = [float(d.view(-1)[s]) for s in o["spots"]]
    assert a == b != 0.0                                               # the direct term is 0 at c == 1: each gets half of the path through M
    out, d = _check_realistic(DF.operands(2, 16, 16, 2, seed=150, max_at="first", ties=2))
    assert float(out[4]) == 2.0


def test_no_positive_response_under_the_hair_is_nan(hip_backend):
    """finite operands; the reference divides 0 by 0 here and so does the kernel"""
    o = DF.exact_operands(2, 5, 7, seed=3, empty=True)
    losses, out, d = _run(o)
    assert math.isnan(float(losses[0])) and math.isnan(float(losses[1]))
    assert float(out[3]) == 0.0 and float(out[2]) == float(o["m"].sum())
    assert not bool(torch.isfinite(d)[o["m"] > 0].any())               # nothing finite reaches the hair pixels' gradient


# ---- (e) guard bands ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label_ch", [1, 2])
@pytest.mark.parametrize("shape", DF.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_writes_stay_inside_out_ws_and_dconf(hip_backend, shape, label_ch):
    from michigan_amd import ops
    o = DF.operands(*shape, label_ch, seed=11 * sum(shape) + label_ch, max_at="last")
    with guard(count_backend=False) as g:
        R = g.place(o["R"], "cuda").requires_grad_(True)
        sem = g.place(o["sem"], "cuda")
        lo, lc = ops.orient_loss_dog(R, g.place(o["idx"], "cuda"), g.place(o["label"], "cuda"), sem[:, 1])
        (lo * 0.7 + lc * 1.3).backward()
        sites = " ".join(a.site for a in g.allocations)
        assert sites.count("torch.empty in ops.py") >= 2 and "torch.empty_like in ops.py" in sites      # out, ws and dconf are guarded
        assert g.check() >= 7
        want = DF.contract(o["R"], o["idx"], o["label"], o["m"])
        assert DF.scalar_close(lo, want[0], DF.SCALAR_TOL["f32"]) and DF.scalar_close(lc, want[1], DF.SCALAR_TOL["f32"])
        assert bool(torch.isfinite(R.grad).all())                      # no 0xFF (NaN) of an unwritten or foreign element reached a result


# ---- (f) end to end ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["ig", "map"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_l1oloss_dog_against_the_reference_fixture(hip_backend, dt, tag):
    from michigan_amd import networks
    fx = DF.golden()
    img = torch.from_numpy(fx["img"])
    label = torch.from_numpy(fx["label_ig"]) if tag == "ig" else torch.from_numpy(fx["label_map"]).float()
    sem = DF.one_hot(torch.from_numpy(fx["hair"]).float())
    crit = networks.L1OLoss(argparse.Namespace(use_ig=tag == "ig", orient_filter="dog")).cuda()
    x = img.permute(0, 2, 3, 1).contiguous().to({"f32": torch.float32, "bf16": torch.bfloat16}[dt]).cuda().requires_grad_(True)
    lo, lc = crit(x.permute(0, 3, 1, 2), label.cuda(), sem.cuda())
    (float(fx["weights"][0]) * lo + float(fx["weights"][1]) * lc).backward()
    torch.cuda.synchronize()
    want_o, want_c = fx["losses_" + tag]
    print("orient %.8f (reference %.8f)  confidence %.8f (reference %.8f)" % (float(lo.detach()), want_o, float(lc.detach()), want_c))
    assert DF.scalar_close(lo, want_o, DF.SCALAR_TOL[dt]) and DF.scalar_close(lc, want_c, DF.SCALAR_TOL[dt])
    ref = torch.from_numpy(fx["grad_" + tag])
    got = x.grad.float().cpu().permute(0, 3, 1, 2)
    err, scale = float((got - ref).abs().max()), float(ref.abs().max())
    print("image gradient: max err %.3e, largest %.3e" % (err, scale))
    assert math.isfinite(err) and err <= (5e-3 if dt == "f32" else 2e-2) * scale       # the dimg rule of test_gabor_argmax_and_orientation_loss
