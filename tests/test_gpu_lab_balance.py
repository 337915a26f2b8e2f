"""MI355X: the balanced colour and hair-Lab passes (mgc_*_balanced_* in mg_color_loss.hip / mg_hair_lab.hip) against what the reference's
own classes computed under --balance_Lab in float64 (tests/golden/lab_balance_{i,ii,hair}.npz, tools/make_lab_balance_golden.py), exact
identities on hand-made tables, other geometries against the float64 contract (tests/lab_balance_fixtures.py), guard bands around every
buffer the four entry points write, and this package's trainer against the reference trainer's record (trainer_L*.npz).

Bounds, and where they come from (those of tests/test_gpu_color_loss.py and tests/test_gpu_unpaired.py):
  losses    the project's fused-loss tolerance: 1e-4 (fp32 image) / 2e-2 (bf16 image) relative to max(1, |want|).
  gradient  relative L2 over the pixels that are not within 1e-3 of a sign change of da or db in the float64 reference (at most 5e-3 of
            the pixels; the exactly-equal patch of pair (ii) is NOT left out).  NO pixel is left out for its bin: the fixtures' target
            pixels are >= 1e-3 from a bin edge, 20 x the float32 route's error in a and b (stored in the fixture).
            fp32 image: max(4 x the error of the reference's own classes run in fp32 against their float64 run, 8 fp32 ulp = 9.5e-7).
            bf16 image: the fixture image is rounded to bf16 first and the reference is the float64 contract on the rounded image (pinned
            to the reference at 1e-9 by tests/test_lab_balance.py); dimg is written in bf16: one bf16 ulp, 2^-8.
            other geometries (no stored reference error): 8 fp32 ulp, as tests/test_gpu_guard_bands.py's colour spec.
  exact     all-ones table, power-of-two table, empty hair plane: torch.equal with the unbalanced entry points -- multiplying by 1 or by
            4 commutes with every rounding of the pass.
  measured  on MI355X (printed by the tests before they assert): see MEASURED below.
"""
import pytest
import torch

import lab_balance_fixtures as LB
import parity_utils as PU
from oracle import contracts as K
from oracle import trainer_parity as TP

pytestmark = pytest.mark.gpu

LOSS_RTOL = {torch.float32: 1e-4, torch.bfloat16: 2e-2}
EXCLUDE_BELOW, EXCLUDE_CAP = 1e-3, 5e-3
# MEASURED (MI355X, this file's own output; bound in brackets)
#   colour, fp32 image: losses <= 4.1e-8 relative [1e-4]; gradient 1.55e-7 (i), 2.11e-7 (ii) relative L2 [9.5e-7], worst element 3.6e-7 of the largest
#   colour, bf16 image: losses <= 6.7e-8 relative [2e-2]; gradient 1.66e-3 (i), 1.57e-3 (ii) relative L2 [3.9e-3]; left out <= 2.6e-4 of the pixels [5e-3]
#   hair:               loss 1.6e-9 (fp32), 2.2e-8 (bf16) relative; gradient 1.46e-7 [9.5e-7] and 1.64e-3 [3.9e-3] relative L2
#   other geometries, fp32: losses <= 2.1e-6 relative (the one-pixel case; <= 4.6e-7 otherwise) [1e-4]; gradient <= 2.7e-7 relative L2 [9.5e-7]


def _image(fake, dtype, channels, device="cuda"):
    """NHWC image with `channels` >= 3 (padding filled with a value that must never be read)."""
    n, _, h, w = fake.shape
    img = torch.full((n, h, w, channels), 3.0, dtype=dtype)
    img[..., :3] = fake.permute(0, 2, 3, 1).to(dtype)
    return img.to(device).requires_grad_(True)


def _sem(fx):
    return torch.stack([fx["back"].float(), fx["hair"].float()], dim=1).cuda()       # planes of one NCHW label: strided


def _run(fx, dtype, channels, table, flags=7, real=None, hair=None, weights=None):
    """ops.color_losses forward + backward; table None = the unbalanced entry points"""
    from michigan_amd import ops
    img = _image(fx["fake"], dtype, channels)
    real = (fx["real"] if real is None else real).cuda()
    sem = _sem(fx)
    hair = sem[:, 1] if hair is None else hair
    if table is None:
        out = ops.color_losses(img, real, sem[:, 0], flags)
    else:
        out = ops.color_losses(img, real, sem[:, 0], flags, hair=hair, table=table.cuda())
    wl, wr, wb = weights if weights is not None else fx["weights"].tolist()
    (wl * out[0] + wr * out[1] + wb * out[2]).backward()
    torch.cuda.synchronize()
    return torch.stack([o.detach() for o in out]).cpu(), img.grad.detach().cpu()


# ---- goldens ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["i", "ii"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_colour_kernels_match_the_reference(hip_backend, tag, dtype):
    fx = LB.load_pair(tag)
    weights = tuple(fx["weights"].tolist())
    real = fx["real"]
    if dtype == torch.float32:
        want_l, want_g, ex = fx["losses"], fx["grad"], fx["excluded"]
        bound = max(4 * float(fx["ref32_grad_rel_l2"]), 8 * 2.0 ** -23)
    else:
        rounded = fx["fake"].to(torch.bfloat16).float()
        if tag == "ii":                                            # keep the exactly-equal patch exactly equal after the rounding
            real = real.clone()
            real[:, :, 40:48, 24:32] = rounded[:, :, 40:48, 24:32]    # (da = db = 0 there: whatever bin the new target falls in, its term is 0)
        want_l, want_g, (da, db, _), _ = LB.color_terms(rounded, real, fx["back"].float(), fx["hair"].float(), fx["S"], 7, weights)
        near = lambda t: (t.abs() > 0) & (t.abs() < EXCLUDE_BELOW)
        ex = near(da) | near(db)
        bound = 2.0 ** -8
    share = float(ex.double().mean())
    keep = (~ex).unsqueeze(1).double()
    got_l, got_g = _run(fx, dtype, 8, fx["S"], real=real)
    got_g3 = got_g[..., :3].permute(0, 3, 1, 2).double()
    rel_l = [abs(float(got_l[k]) - float(want_l[k])) / max(1.0, abs(float(want_l[k]))) for k in range(3)]
    rel_g = float(((got_g3 - want_g) * keep).norm() / (want_g * keep).norm())
    worst = float(((got_g3 - want_g) * keep).abs().max() / want_g.abs().max())
    print("balanced colour loss %s %s: losses %s want %s rel %s | grad rel L2 %.3e (bound %.3e), worst element / largest %.3e | left out %.2e of the pixels"
          % (tag, dtype, got_l.tolist(), [float(v) for v in want_l], ["%.2e" % v for v in rel_l], rel_g, bound, worst, share))
    assert share <= EXCLUDE_CAP
    assert max(rel_l) <= LOSS_RTOL[dtype], rel_l
    assert rel_g <= bound, (rel_g, bound)
    assert float(got_g[..., 3:].abs().max()) == 0.0                # padding channels of dimg
    if tag == "ii":
        assert float(want_g[:, :, 40:48, 24:32].abs().max()) == 0.0
        assert float(got_g3[:, :, 40:48, 24:32].abs().max()) == 0.0, "sign(0) must be 0"


def _run_hair(fx, dtype, channels, table, flags=1):
    from michigan_amd import ops
    img = _image(fx["fake"], dtype, channels)
    sem_tag = torch.stack([1 - fx["m_f"], fx["m_f"]], dim=1).cuda()
    sem_ref = torch.stack([1 - fx["m_r"], fx["m_r"]], dim=1).cuda()
    tgt = fx["ref"].flip(0).contiguous().cuda()
    out = ops.hair_lab_losses(img, fx["ref"].cuda(), sem_tag[:, 1], sem_ref[:, 1], tgt, sem_tag[:, 0], flags,
                              table=None if table is None else table.cuda())
    (0.5 * out[0] + 2.0 * out[1]).backward()
    torch.cuda.synchronize()
    return torch.stack([o.detach() for o in out]).cpu(), img.grad.detach().cpu()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_hair_kernels_match_the_reference(hip_backend, dtype):
    fx = LB.load_pair("hair")
    if dtype == torch.float32:
        want_l, want_g = float(fx["loss"]), 0.5 * fx["grad"]
        bound = max(4 * float(fx["ref32_grad_rel_l2"]), 8 * 2.0 ** -23)
    else:
        rounded = fx["fake"].to(torch.bfloat16).float()
        l, want_g, _, _ = LB.hair_terms(rounded, fx["ref"], fx["m_f"], fx["m_r"], fx["S"], flags=1, weights=(0.5, 0.0))
        want_l, bound = float(l[0]), 2.0 ** -8
    got_l, got_g = _run_hair(fx, dtype, 8, fx["S"], flags=1)
    got_g3 = got_g[..., :3].permute(0, 3, 1, 2).double()
    rel_l = abs(float(got_l[0]) - want_l) / max(1.0, abs(want_l))
    rel_g = float((got_g3 - want_g).norm() / want_g.norm())
    print("balanced hair lab %s: loss %.8f want %.8f rel %.2e | grad rel L2 %.3e (bound %.3e)" % (dtype, float(got_l[0]), want_l, rel_l, rel_g, bound))
    assert rel_l <= LOSS_RTOL[dtype] and rel_g <= bound, (rel_l, rel_g, bound)
    assert float(got_g[..., 3:].abs().max()) == 0.0 and float(got_l[1]) == 0.0
    # sample 2 (an empty reference mask): weight S[128][128]; the gradient of every sample is the unbalanced one times its weight
    plain_l, plain_g = _run_hair(fx, dtype, 8, None, flags=1)
    ratio = got_g.double().flatten(1).norm(dim=1) / plain_g.double().flatten(1).norm(dim=1)
    assert torch.allclose(ratio, fx["w"].double(), rtol=2.0 ** -7 if dtype == torch.bfloat16 else 1e-6), (ratio, fx["w"])


# ---- exact identities on hand-made tables ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_exact_identities_of_the_colour_pass(hip_backend, dtype):
    fx = LB.load_pair("i")
    ones, four = torch.ones(256, 256), torch.full((256, 256), 4.0)
    everywhere, nowhere = torch.ones(2, 96, 80).cuda(), torch.zeros(2, 96, 80).cuda()
    plain_l, plain_g = _run(fx, dtype, 8, None)
    l, g = _run(fx, dtype, 8, ones)
    assert torch.equal(l, plain_l) and torch.equal(g, plain_g), "an all-ones table must reproduce the unbalanced pass bit for bit"
    l, g = _run(fx, dtype, 8, fx["S"], hair=nowhere)
    assert torch.equal(l, plain_l) and torch.equal(g, plain_g), "no hair anywhere: every weight is 1"
    # a constant 4 with hair everywhere: 4 x the Lab loss and the Lab gradient, exactly
    lab_l, lab_g = _run(fx, dtype, 8, None, flags=1, weights=(1.0, 0.0, 0.0))
    l, g = _run(fx, dtype, 8, four, flags=1, hair=everywhere, weights=(1.0, 0.0, 0.0))
    assert torch.equal(l, 4 * lab_l) and torch.equal(g, 4 * lab_g), "a power-of-two weight commutes with every rounding"
    # ... and with the fixture's own 0/1 hair plane: 4 on the hair, 1 off it
    l, g = _run(fx, dtype, 8, four, flags=1, weights=(1.0, 0.0, 0.0))
    on = (fx["hair"] > 0).unsqueeze(-1)
    assert torch.equal(g, torch.where(on, 4 * lab_g, lab_g))
    # a hair VALUE multiplies: 0.5 everywhere under the table of 4 is a weight of 2
    l, g = _run(fx, dtype, 8, four, flags=1, hair=0.5 * everywhere, weights=(1.0, 0.0, 0.0))
    assert torch.equal(l, 2 * lab_l) and torch.equal(g, 2 * lab_g)
    # rgb and background ride along unchanged
    l, g = _run(fx, dtype, 8, four, hair=everywhere)
    assert torch.equal(l[1:], plain_l[1:]) and torch.equal(l[0], 4 * plain_l[0])


def test_bin_255_is_read_as_the_table_says(hip_backend):
    """No RGB colour reaches bin 255 of a or b (tools/make_lab_balance_golden.py scans the cube: a + 128 <= 226.3, b + 128 <= 222.5), so the
    bins of a target are moved there by hand: a table that is `marker` at the bin pair the target's colour falls in.  The table is what
    says which bins are 0; the kernel reads any entry as it stands."""
    from michigan_amd import ops
    n, h, w = 1, 8, 32
    real = torch.zeros(n, 3, h, w)
    real[:, 0], real[:, 1], real[:, 2] = 1.0, -1.0, 1.0                      # magenta: the largest a
    a, b = K._ab(K._xyz(real.double()))
    ka, kb = int(LB.bins(a)[0, 0, 0]), int(LB.bins(b)[0, 0, 0])
    fx = dict(fake=torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(1)) * 2 - 1, real=real, hair=torch.ones(n, h, w),
              back=torch.zeros(n, h, w))
    lab_l, lab_g = _run(fx, torch.float32, 4, None, flags=1, weights=(1.0, 0.0, 0.0))
    marked = torch.ones(256, 256)
    marked[ka, kb] = 8.0
    l, g = _run(fx, torch.float32, 4, marked, flags=1, weights=(1.0, 0.0, 0.0))
    assert torch.equal(l, 8 * lab_l) and torch.equal(g, 8 * lab_g), "row = bin of a, column = bin of b"
    transposed = torch.ones(256, 256)
    transposed[kb, ka] = 8.0
    l, g = _run(fx, torch.float32, 4, transposed, flags=1, weights=(1.0, 0.0, 0.0))
    assert torch.equal(l, lab_l) and ka != kb, "the table is not transposed"
    # row 255 and column 255 nonzero in a caller's table and zero in ops.lab_weight_table's: the latter means weight 1 in the colour pass
    S = ops.lab_weight_table(LB.ab_count(), 10.0)
    assert float(S[255].abs().max()) == 0.0 and float(S[:, 255].abs().max()) == 0.0
    zeroed = torch.full((256, 256), 8.0)
    zeroed[ka, kb] = 0.0                                                      # what a bin-255 pixel finds in the product's table
    l, g = _run(fx, torch.float32, 4, zeroed, flags=1, weights=(1.0, 0.0, 0.0))
    assert torch.equal(l, lab_l) and torch.equal(g, lab_g), "a zero of the table is a weight of 1 in the colour pass"


def test_clamped_bins_of_the_hair_pass_and_its_zero_weight(hip_backend):
    """The hair pass bins a MEAN, which an empty mask makes exactly 0 (bin 128, 128): a table that is 0 there gives weight 0 -- no
    zero-to-one replacement -- and the all-ones and power-of-two identities hold as in the colour pass."""
    fx = LB.load_pair("hair")
    plain_l, plain_g = _run_hair(fx, torch.float32, 8, None, flags=3)
    l, g = _run_hair(fx, torch.float32, 8, torch.ones(256, 256), flags=3)
    assert torch.equal(l, plain_l) and torch.equal(g, plain_g)
    hair_l, hair_g = _run_hair(fx, torch.float32, 8, None, flags=1)
    l, g = _run_hair(fx, torch.float32, 8, torch.full((256, 256), 4.0), flags=1)
    assert torch.equal(l, 4 * hair_l) and torch.equal(g, 4 * hair_g)
    hole = torch.ones(256, 256)
    hole[128, 128] = 0.0
    l, g = _run_hair(fx, torch.float32, 8, hole, flags=1)
    assert torch.equal(g[:2], hair_g[:2]) and float(g[2].abs().max()) == 0.0 and float(hair_g[2].abs().max()) > 0, "weight 0: no gradient for sample 2"
    want = LB.hair_terms(fx["fake"], fx["ref"], fx["m_f"], fx["m_r"], hole, flags=1)[0][0]
    assert abs(float(l[0]) - float(want)) <= 1e-4 * float(want) and float(l[0]) < float(hair_l[0])


# ---- geometry ----------------------------------------------------------------------------------------------------------------------------------
_S10 = {}


def _table():
    from michigan_amd import ops
    if "S" not in _S10:
        _S10["S"] = ops.lab_weight_table(LB.ab_count(), 1e4)                  # the whole range of weights
    return _S10["S"]


@pytest.mark.parametrize("shape,channels", [((1, 1, 1), 3), ((1, 15, 17), 4), ((1, 16, 16), 8), ((1, 257, 1), 3), ((3, 33, 130), 8), ((2, 67, 35), 4),
                                            ((1, 520, 512), 8)],
                         ids=["1px", "255px", "256px", "257px", "3x33x130", "2x67x35", "1x520x512-stride-loop-wraps"])
def test_other_geometries_against_the_contract(hip_backend, shape, channels):
    from michigan_amd import ops
    n, h, w = shape
    fx = LB.operands(n, h, w, seed=7 + h)
    S = _table()
    weights = (0.05, 3.0, 2.0)
    want_l, want_g, (da, db, _), wpix = LB.color_terms(fx["fake"], fx["real"], fx["back"], fx["hair"], S, 7, weights)
    near = lambda t: (t.abs() > 0) & (t.abs() < EXCLUDE_BELOW)
    ex = near(da) | near(db)
    keep = (~ex).unsqueeze(1).double()
    # strided hair and real planes: the label's channel 1, and the target inside a wider NCHW tensor (sample stride 4 HW)
    wide = torch.full((n, 4, h, w), 9.0)
    wide[:, :3] = fx["real"]
    real = wide.cuda()[:, :3]
    assert not real.is_contiguous() or n == 1
    runs = []
    for _ in range(2):
        img = _image(fx["fake"], torch.float32, channels)
        sem = _sem(fx)
        out = ops.color_losses(img, real, sem[:, 0], 7, hair=sem[:, 1], table=S.cuda())
        (weights[0] * out[0] + weights[1] * out[1] + weights[2] * out[2]).backward()
        torch.cuda.synchronize()
        runs.append((torch.stack([o.detach() for o in out]).cpu(), img.grad.detach().cpu()))
    (got_l, got_g), (again_l, again_g) = runs
    assert torch.equal(got_l, again_l) and torch.equal(got_g, again_g), "ordered sums: two runs must be bit-identical"
    got_g3 = got_g[..., :3].permute(0, 3, 1, 2).double()
    rel_l = [abs(float(got_l[k]) - float(want_l[k])) / max(1.0, abs(float(want_l[k]))) for k in range(3)]
    den = float((want_g * keep).norm())
    rel_g = float(((got_g3 - want_g) * keep).norm()) / den if den > 0 else float(((got_g3 - want_g) * keep).abs().max())
    print("balanced colour %s C=%d: losses rel %s | grad rel L2 %.3e | weights %.3g..%.3g | left out %.2e"
          % (shape, channels, ["%.2e" % v for v in rel_l], rel_g, float(wpix.min()), float(wpix.max()), float(ex.double().mean())))
    assert max(rel_l) <= LOSS_RTOL[torch.float32], rel_l
    assert rel_g <= 8 * 2.0 ** -23, rel_g
    assert channels == 3 or float(got_g[..., 3:].abs().max()) == 0.0, "padding channels written zero"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_flag_subsets_layouts_and_reproducibility(hip_backend, dtype):
    fx = LB.load_pair("i")
    S = fx["S"]
    all_l, all_g = _run(fx, dtype, 8, S)
    again_l, again_g = _run(fx, dtype, 8, S)
    assert torch.equal(all_l, again_l) and torch.equal(all_g, again_g), "ordered sums: two runs must be bit-identical"
    for c in (3, 4):
        lc, gc = _run(fx, dtype, c, S)
        assert torch.equal(lc, all_l) and torch.equal(gc[..., :3], all_g[..., :3]), "C = 3, 4 and 8 layouts must agree"
        assert c == 3 or float(gc[..., 3:].abs().max()) == 0.0
    plain_l, _ = _run(fx, dtype, 8, None)
    for flags in (1, 3, 5, 7):                                      # every subset that contains lab
        l, g = _run(fx, dtype, 8, S, flags=flags)
        for k in range(3):
            if flags & (1 << k):
                assert float(l[k]) == float(all_l[k]), (flags, k)   # bit for bit the value of the all-on call
            else:
                assert float(l[k]) == 0.0, (flags, k)
        assert float(l[1]) == (float(plain_l[1]) if flags & 2 else 0.0) and float(l[2]) == (float(plain_l[2]) if flags & 4 else 0.0)
        assert float(g[..., 3:].abs().max()) == 0.0


def test_strided_target_and_hair_planes_at_the_c_abi(hip_backend):
    """The operator layer hands the target over dense; the entry points take any sample stride >= 3 HW (and >= HW for the planes)."""
    from michigan_amd import _cabi as C
    from michigan_amd import ops
    n, h, w = 2, 33, 35
    fx = LB.operands(n, h, w, seed=3)
    S = _table().cuda()
    img = _image(fx["fake"], torch.float32, 4).detach()
    wide = torch.full((n, 5, h, w), float("nan"), device="cuda")
    wide[:, 1:4] = fx["real"].cuda()
    planes = torch.full((n, 3, h, w), float("nan"), device="cuda")
    planes[:, 0], planes[:, 2] = fx["back"].cuda(), fx["hair"].cuda()
    want = ops.color_losses(img, fx["real"].cuda(), planes[:, 0], 7, hair=planes[:, 2], table=S)
    out, ws = torch.empty(3, device="cuda"), torch.empty(3 * 1024, device="cuda")
    p = lambda t: C.ctypes.c_void_p(t.data_ptr())
    C.backend().mgc_color_loss_balanced_fwd(p(img), p(wide[:, 1:4]), 5 * h * w, p(planes[:, 0]), 3 * h * w, p(planes[:, 2]), 3 * h * w, p(S), C.MG_F32,
                                            n, h, w, 4, 7, p(out), p(ws), None)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.stack([o.detach() for o in want]).cpu())


# ---- guard bands ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,channels", [((1, 67, 35), 3), ((3, 33, 130), 8)])
def test_guard_bands_around_everything_the_entry_points_write(hip_backend, shape, channels):
    """out, ws and dimg of the colour pass; out, stats, ws and dimg of the hair pass: all come from the operator layer's allocators, which
    tests/guard_alloc.py carves out of 0xFF-filled buffers; the inputs, the table included, are placed in guarded buffers too, so a read
    past the table's last entry would fetch NaN."""
    import guard_alloc
    from michigan_amd import ops
    n, h, w = shape
    fx = LB.operands(n, h, w, seed=11)
    S = _table()
    g64 = torch.Generator().manual_seed(5)
    ref = (torch.rand(n, 3, h, w, generator=g64) * 2 - 1) * 0.3
    m_r = (torch.rand(n, h, w, generator=g64) > 0.5).float()
    want_l = LB.color_terms(fx["fake"], fx["real"], fx["back"], fx["hair"], S, 7)[0]
    want_h = LB.hair_terms(fx["fake"], ref, fx["hair"], m_r, S, fx["real"], fx["back"], 3)[0]
    means = torch.stack(LB.ref_means(ref, m_r)) + 128
    assert float((means - means.round()).abs().min()) >= 0.01, "a reference mean too close to a bin edge: pick another seed"
    with guard_alloc.guard() as g:
        img = g.place(_image(fx["fake"], torch.float32, channels, device="cpu").detach(), "cuda").requires_grad_(True)
        real, refd, table = g.place(fx["real"], "cuda"), g.place(ref, "cuda"), g.place(S, "cuda")
        sem = g.place(torch.stack([fx["back"], fx["hair"]], dim=1), "cuda")
        mr = g.place(m_r, "cuda")
        out = ops.color_losses(img, real, sem[:, 0], 7, hair=sem[:, 1], table=table)
        (gi,) = torch.autograd.grad(out[0] + out[1] + out[2], img)
        hout = ops.hair_lab_losses(img, refd, sem[:, 1], mr, real, sem[:, 0], 3, table=table)
        (hi,) = torch.autograd.grad(hout[0] + hout[1], img)
        checked = g.check()
        got_l, got_h = torch.stack([o.detach() for o in out]).cpu(), torch.stack([o.detach() for o in hout]).cpu()
        finite = bool(torch.isfinite(gi).all()) and bool(torch.isfinite(hi).all())
    assert checked >= 12, checked
    assert finite
    for got, want in ((got_l, want_l), (got_h, want_h)):
        for a, b in zip(got.tolist(), want.tolist()):
            assert abs(a - b) <= 1e-4 * max(1.0, abs(b)), (got, want)


# ---- the trainer ---------------------------------------------------------------------------------------------------------------------------------
def test_trainer_fp32_with_balance_lab_matches_reference_trainer_golden(hip_backend):
    """tests/test_gpu_color_loss.py's trainer_C protocol and tolerances, with --balance_Lab --weight_dir on top of the published flags."""
    from michigan_amd.model import Pix2PixTrainer
    cfg = dict(TP.CFGS["A"], tag="L")
    torch.manual_seed(0)
    trainer = Pix2PixTrainer(TP.repo_options(cfg, gpu_ids=[0], compute_dtype="fp32", no_lab_loss=False, balance_Lab=True, weight_dir=LB.ab_count_path()))
    TP.load_weights(trainer, cfg)
    rec = LB.drive_with_lab(trainer, cfg, device="cuda")
    print("trainer L losses", {k: float(v) for k, v in rec.items() if ".loss." in k})
    TP.compare(rec, PU.load_trainer_golden("L"), rtol_loss0=5e-4, rtol_later=TP.RTOL_LATER_HIP, atol_img=1e-3, atol_weight=2 * 4e-4 * 2 + 1e-5)
