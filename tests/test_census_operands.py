"""CPU side of the census tests (tests/test_gpu_census.py): the recipes of tests/census_operands.py hold their preconditions for every
operand set, the contract emulator returns exactly what the GPU file will demand (its own ``*_case`` functions on a thinned shape list),
and the tests BITE: a reference that drops the last pixel, the last pixel of the first half or the last channel quad, counts the first
pixel twice, or exchanges two elements of the drain's permutation is rejected by the GPU file's comparison in every group."""
import pytest
import torch

import census_operands as Z
import exact_operands as X
import test_gpu_census as G

THIN_C = (4, 24, 64, 136, 1024)
THIN_P = (1, 2, 17, 257)


@pytest.fixture
def emulator(emulator_backend):
    from michigan_amd import _cabi
    prev = G.install_emulator()
    yield
    _cabi.set_backend(prev)


def _assert_bites(tag, want, mutant_of, G_, P, C):
    muts = Z.mutations(G_, P, C)
    assert muts
    for name, (pw, cw) in muts.items():
        assert G.rejects(mutant_of(pw, cw), want), f"{tag}: the comparison accepts a kernel that would {name}"


# ---------------------------------------------------------------------------------------------------------------------
# preconditions of every operand set (the references assert them when called without a mutation)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_statistics_operands_hold_their_preconditions_and_bite(dt):
    for C in Z.C_LIST:
        for P in Z.p_list(C):
            for G_ in (1, 3):
                for pivot in (False, True):
                    o = Z.stats_operands(dt, G_, P, C, pivot)
                    Z.stats_check(o, f"stats {dt} {G_} {P} {C} {pivot}")
                    run0 = Z.running_init(C) if G_ == 1 else None
                    kw = dict(sum_scale=4.0, count=4.0 * P, running=run0) if pivot else {}
                    want = Z.stats_reference(o, **kw)
                    if C in THIN_C and (P in THIN_P or P == 4099):
                        _assert_bites(f"stats {dt} G={G_} P={P} C={C} pivot={pivot}", want, lambda pw, cw: Z.stats_reference(o, pw=pw, cw=cw, **kw), G_, P, C)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_norm_backward_operands_hold_their_preconditions_and_bite(dt):
    for C in Z.C_LIST:
        for P in Z.p_list(C):
            if C >= 1024 and P not in THIN_P:
                continue                                       # the same generator at the same C: P only moves the tails
            for G_ in (1, 3):
                o = Z.bwd_operands(dt, G_, P, C)
                for act, _h, use_g1, want_dgb in G.REDUCE_VARIANTS:
                    if want_dgb and G_ != 1:
                        continue
                    want = Z.bwd_reduce_reference(o, act, use_g1, want_dgb, dt)
                    if C in THIN_C and P in THIN_P and _h:
                        _assert_bites(f"reduce {dt} G={G_} P={P} C={C} {act}", want,
                                      lambda pw, cw: Z.bwd_reduce_reference(o, act, use_g1, want_dgb, dt, pw=pw, cw=cw), G_, P, C)
    for C in (24, 64):
        for up in G.UP_SHAPES:
            P = up[0] * up[1] * up[2]
            o = Z.bwd_operands(dt, 1, P, C, up=up)
            assert torch.equal(Z.upsample(o["xs"]).reshape(1, P, C), o["x"])
            want = Z.bwd_reduce_reference(o, "lrelu", True, True, dt)
            _assert_bites(f"reduce up {dt} {up} C={C}", want, lambda pw, cw: Z.bwd_reduce_reference(o, "lrelu", True, True, dt, pw=pw, cw=cw), 1, P, C)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_apply_and_forward_operands_hold_their_preconditions_and_bite(dt):
    for C in Z.C_LIST:
        for P in Z.p_list(C):
            if C >= 1024 and P not in THIN_P:
                continue                                       # (the GPU file asserts the same preconditions on every case it runs)
            for G_ in (1, 3):
                o, f = Z.apply_operands(dt, G_, P, C), Z.fwd_operands(dt, G_, P, C)
                assert o["gstride"] > 2 * C - 1 and o["gstride"] > C
                for act, _h, use_g1 in G._thin(G.APPLY_VARIANTS, C, P):
                    want = Z.apply_reference(o, act, use_g1, dt)
                    if C in THIN_C and P in THIN_P:
                        _assert_bites(f"apply {dt} G={G_} P={P} C={C} {act}", want, lambda pw, cw: Z.apply_reference(o, act, use_g1, dt, pw=pw, cw=cw), G_, P, C)
                for act, resid in G._thin(G.FWD_VARIANTS, C, P):
                    want = Z.fwd_reference(f, act, resid, dt)
                    if C in THIN_C and P in THIN_P and act != "relu":          # under ReLU a doubled negative x stays clamped: the other acts carry it
                        _assert_bites(f"fwd {dt} G={G_} P={P} C={C} {act}", want, lambda pw, cw: Z.fwd_reference(f, act, resid, dt, pw=pw, cw=cw), G_, P, C)
    for C in G.VEC_C[dt]:
        for two in (False, True):
            for up in [None] + G.UP_SHAPES:
                for P in ((1, 17, 257, 513) if up is None else (up[0] * up[1] * up[2],)):
                    o = Z.apply2_operands(dt, P, C, two, up=up)
                    for acts in (("lrelu", "none"), ("none", "relu")):
                        want = Z.apply2_reference(o, acts, dt)
                        if C <= 1024:
                            _assert_bites(f"apply2 {dt} P={P} C={C} two={two} up={up}", want, lambda pw, cw: Z.apply2_reference(o, acts, dt, pw=pw, cw=cw), 1, P, C)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_loss_operands_hold_their_preconditions_and_bite(dt):
    for q in G.L1_Q:
        o = Z.l1_operands(dt, q)
        _assert_bites(f"l1 {q}", Z.l1_reference(o), lambda pw, cw: Z.l1_reference(o, pw), 1, 4 * q, 0)
    for n in G.HINGE_N:
        o = Z.hinge_operands(dt, n)
        for mode in (0, 1, 2):
            for use_w in (False, True):
                _assert_bites(f"hinge {n} {mode}", Z.hinge_reference(o, mode, use_w), lambda pw, cw: Z.hinge_reference(o, mode, use_w, pw), 1, n, 0)
    for H, W in G.IMAGE_HW:
        for N in (1, 3):
            o = Z.image_operands(dt, N, H, W)
            assert o["real_buf"].stride(0) > 3 * H * W and o["mask_buf"].stride(0) > H * W
            for masked in (False, True):
                _assert_bites(f"image {N} {H}x{W} {masked}", Z.image_reference(o, masked), lambda pw, cw: Z.image_reference(o, masked, pw), N, H * W, 0)
            oo = Z.orient_operands(N, H, W)
            _assert_bites(f"orient {N} {H}x{W}", Z.orient_reference(oo), lambda pw, cw: Z.orient_reference(oo, pw), N, H * W, 0)
    for P in G.FILL_P:
        for C in G.FILL_C:
            for adjoint in (False, True):
                o = Z.fill_operands(dt, 3, P, C)
                _assert_bites(f"fill {P} {C} {adjoint}", Z.fill_reference(o, adjoint), lambda pw, cw: Z.fill_reference(o, adjoint, pw, cw), 3, P, C)
                Z.fill_reference(Z.fill_operands(dt, 3, P, C, empty=True), adjoint)


def test_kernel_variants_of_the_shape_lists():
    """What the summary reports: the variants the C list reaches in either dtype, derived from the dispatch predicates."""
    assert sorted(set(G.PATHS["bf16"].values())) == ["quad-tpr1-trips1", "quad-tpr12-trips1", "quad-tpr256-trips4", "quad-tpr34-trips1", "quad-tpr6-trips1",
                                                     "vec-rows1", "vec-rows2", "vec-rows32"]
    assert sorted(set(G.PATHS["f32"].values())) == ["quad-tpr12-trips1", "quad-tpr256-trips2", "quad-tpr256-trips4", "quad-tpr34-trips1", "quad-tpr6-trips1",
                                                    "vec-rows1", "vec-rows16", "vec-rows256"]
    for P in Z.P_LIST:
        assert {0, P - 1} <= set(Z.structural_pixels(P))


# ---------------------------------------------------------------------------------------------------------------------
# the GPU file's own cases on the contract emulator, thinned
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_emulator_returns_what_the_gpu_file_demands(emulator, dt):
    rep = G._Report()
    for C in THIN_C:
        for P in THIN_P:
            for G_ in (1, 3):
                G.stats_case(rep, dt, G_, P, C, "cpu")
                G.reduce_case(rep, dt, G_, P, C, G.REDUCE_VARIANTS[3::4], "cpu")
                G.apply_case(rep, dt, G_, P, C, "cpu")
                G.fwd_case(rep, dt, G_, P, C, "cpu")
    G.reduce_case(rep, dt, 1, 120, 24, G.REDUCE_VARIANTS[-1:], "cpu", up=(2, 6, 10))
    G.apply2_case(rep, dt, 64, "cpu", shapes=[None, (2, 6, 10)])
    G.spade_dx_case(rep, dt, "cpu")
    G.l1_case(rep, dt, 257, "cpu")
    G.hinge_case(rep, dt, 1025, "cpu")
    G.image_case(rep, dt, 3, 17, 16, "cpu")
    G.orient_case(rep, 3, 3, 5, "cpu")
    G.fill_case(rep, dt, 17, 68, "cpu")
    assert rep.compared > 500
    rep.done()


def test_drain_on_the_emulator_and_a_swapped_permutation_is_rejected(emulator):
    rep = G._Report()
    opt, want = G.drain_case(rep, "cpu")
    rep.done()
    ok = {"flat_grad": (want, torch.float32, "bits")}
    assert not G.rejects(ok, ok)
    checked = 0
    for p in opt.params:
        a, b = opt._span_of[id(p)]
        if p.dim() == 4 and want[a] != want[b - 1]:
            checked += 1
            mutant = want.clone()
            mutant[a:b] = Z.swap_permutation(want[a:b])
            assert G.rejects({"flat_grad": (mutant, torch.float32, "bits")}, ok), f"a swap inside the weight at [{a}, {b}) goes unnoticed"
    assert checked >= len(Z.DRAIN_LAYERS) + 2 * len(Z.DRAIN_SPADE)
