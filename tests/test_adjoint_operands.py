"""CPU side of the adjoint tests (tests/test_gpu_adjoint_bits.py): every operand set of the committed case lists holds its preconditions
(exactness, rounding share, tie share, term floor against delta -- the references assert them when called without a mutant), a kernel that
computes the reference exactly is ACCEPTED, the contract emulator returns what the GPU file will demand (its own ``*_case`` functions on a
thinned list: the MG_TEST_DRYRUN path), and the rules BITE: every mutant of tests/adjoint_operands.py is rejected."""
import pytest
import torch

import adjoint_operands as A
import test_gpu_adjoint_bits as G
from census_operands import hinge_operands

DTS = ["f32", "bf16"]
BIG = A.ROUNDING_MIN_NUMEL


@pytest.fixture
def emulator(emulator_backend):
    from michigan_amd import _cabi
    outer = G.install_emulator()
    cb, prev = G.install_counter()
    yield cb
    _cabi.set_backend(prev)
    _cabi.set_backend(outer)


def _accepts(tag, want):
    assert not A.rejects(A.stored(want), want), f"{tag}: the rule rejects the exact reference"


def _bites(tag, want, mutant):
    assert A.rejects(mutant, want), f"{tag}: the rule accepts this mutant"


# ---------------------------------------------------------------------------------------------------------------------
# rules 1 and 2: copies, short sums
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_copy_operands_carry_signed_zeros_and_subnormals(dt):
    x = A.copy_operands(dt, (3, 16, 17, 136))
    assert A.has_edge_values(x) and bool(torch.isfinite(x.float()).all())
    for kind, p in (("up", None), ("reflect", 3), ("maxpool", None)):
        want = A.copy_reference(kind, x, p)
        _accepts(kind, want)
        flipped = want["y"].ref.clone()
        zero = (flipped == 0).nonzero()[0]
        flipped[tuple(zero)] = -flipped[tuple(zero)]                            # the other zero: equal by value, not by bits
        assert torch.equal(flipped, want["y"].ref) and A.rejects({"y": flipped}, want), f"{kind}: a zero of the wrong sign passes"


@pytest.mark.parametrize("dt", DTS)
def test_assemble_reference_and_a_truncating_store(dt):
    for nhw in G.ASSEMBLE_NHW:
        for cp, cs, cf in A.ASSEMBLE:
            o = A.assemble_operands(dt, *nhw, cp, cs, cf)
            want = A.assemble_reference(o)
            _accepts(f"assemble {nhw} {cp} {cs} {cf}", want)
            pad = want["out"].ref[..., cp + cf:]
            assert pad.numel() == 0 or not bool(A._int_view(pad).any()), "the pad channels are not +0"
            if dt == "bf16" and cp and nhw[0] * nhw[1] * nhw[2] * cp >= BIG:
                _bites(f"assemble {nhw} cp={cp}: truncating store", want, A.assemble_reference(o, "truncating-store"))


@pytest.mark.parametrize("dt", DTS)
def test_upsample_and_reflect_adjoints_hold_their_preconditions_and_bite(dt):
    for geom in A.geoms(thin=True):
        dy = A.up_bwd_operands(dt, geom)
        want = A.up_bwd_reference(dy, dt)
        _accepts(f"up_bwd {geom}", want)
        if dt == "bf16" and want["dx"].ref.numel() >= BIG:
            for mut in ("bf16-accumulate", "truncating-store"):
                _bites(f"up_bwd {geom}: {mut}", want, A.up_bwd_reference(dy, dt, mut))
    both = 0
    for h, w, p in A.REFLECT:
        both += 2 * p >= h                                                      # a row that the top AND the bottom mirror reach
        for n in A.NS:
            for c in A.CS:
                dy = A.reflect_bwd_operands(dt, n, h, w, c, p)
                want = A.reflect_bwd_reference(dy, p, dt)
                _accepts(f"reflect_bwd {(n, h, w, c, p)}", want)
                _bites(f"reflect_bwd {(n, h, w, c, p)}: no corner mirror", want, A.reflect_bwd_reference(dy, p, dt, "no-corner-mirror"))
                if dt == "bf16" and want["dx"].ref.numel() >= BIG:
                    _bites(f"reflect_bwd {(n, h, w, c, p)}: truncating store", want, A.reflect_bwd_reference(dy, p, dt, "truncating-store"))
    assert both >= 2


@pytest.mark.parametrize("dt", DTS)
def test_activation_and_blend_operands_hold_their_preconditions_and_bite(dt):
    for nq in A.FLAT_QUADS:
        o = A.act_operands(dt, nq)
        for act in ("none", "relu", "lrelu"):
            for two in (False, True):
                want = A.act_bwd_reference(o, act, two)
                _accepts(f"act {act} {two} {nq}", want)
                if act == "lrelu" and nq >= 255:
                    _bites(f"act lrelu two={two} nq={nq}: factor 1 at y == 0", want, A.act_bwd_reference(o, act, two, "lrelu-one-at-zero"))
                if dt == "bf16" and two and nq >= 255:
                    _bites(f"act {act} nq={nq}: truncating store", want, A.act_bwd_reference(o, act, two, "truncating-store"))
    for P, C in [(nq, 4) for nq in A.FLAT_QUADS] + [(85, 12), (3, 136)]:
        o = A.blend_operands(dt, P, C)
        for act in ("none", "lrelu"):
            want = A.blend_reference(o, act)
            _accepts(f"blend {act} {P} {C}", want)
            if P >= 3:
                _bites(f"blend {act} P={P} C={C}: weights swapped", want, A.blend_reference(o, act, "weights-swapped"))
                if dt == "bf16":
                    _bites(f"blend {act} P={P} C={C}: truncating store", want, A.blend_reference(o, act, "truncating-store"))


# ---------------------------------------------------------------------------------------------------------------------
# rule 3: max-pool adjoint
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_maxpool_operands_tie_and_the_rule_sees_the_order(dt):
    for geom in A.geoms():
        o = A.maxpool_operands(dt, geom)
        n, h, w, c = geom
        for relu in (0, 1):
            want = A.maxpool_bwd_reference(o, relu)
            _accepts(f"maxpool {geom} {relu}", want)
            assert not bool(A._int_view(want["dx"].ref[:, h // 2 * 2:]).any()) and not bool(A._int_view(want["dx"].ref[:, :, w // 2 * 2:]).any())
            _bites(f"maxpool {geom} relu_input={relu}: last maximum wins", want, A.maxpool_bwd_reference(o, relu, "last-maximum"))
            if relu and n * (h // 2) * (w // 2) * c >= 64:
                _bites(f"maxpool {geom}: relu_input ignored", want, A.maxpool_bwd_reference(o, relu, "relu-input-ignored"))


def test_chain_operands_are_exact():
    for dt in DTS:
        ref = G.chain_reference(G.chain_operands(dt))
        assert torch.equal(ref["dx"], ref["dx"].round()) and torch.equal(ref["dw"], ref["dw"].round())     # both L1 counts cancel: integers


# ---------------------------------------------------------------------------------------------------------------------
# rule 4: quotients
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_avgpool_operands_hold_the_term_floor_and_bite(dt):
    counts, reciprocal = set(), 0
    for geom in A.geoms(thin=True):
        o = A.avgpool_operands(dt, geom)
        fwd, bwd = A.avgpool_fwd_reference(o), A.avgpool_bwd_reference(o)
        _accepts(f"avgpool {geom}", fwd)
        _accepts(f"avgpool {geom}", bwd)
        n, h, w, c = geom
        cnt = A._pool_counts(1, 1, h, w)
        counts |= set(cnt.unique().tolist())
        _bites(f"avgpool_fwd {geom}: count_include_pad", fwd, A.avgpool_fwd_reference(o, "count-include-pad"))
        _bites(f"avgpool_bwd {geom}: count_include_pad", bwd, A.avgpool_bwd_reference(o, "count-include-pad"))
        if not bool(A._is_pow2(cnt).all()) and (dt == "f32" or fwd["y"].ref.numel() >= BIG):
            reciprocal += 1
            _bites(f"avgpool_fwd {geom}: bf16 reciprocal", fwd, A.avgpool_fwd_reference(o, "bf16-reciprocal"))
        if dt == "bf16" and fwd["y"].ref.numel() >= BIG and float(cnt.max()) > 1:     # (a 1 x 1 image is copied)
            _bites(f"avgpool_fwd {geom}: truncating store", fwd, A.avgpool_fwd_reference(o, "truncating-store"))
            if not bool(A._is_pow2(cnt).all()):                                     # (a lone quotient by 4 of an 8-bit integer needs no rounding)
                _bites(f"avgpool_bwd {geom}: truncating store", bwd, A.avgpool_bwd_reference(o, "truncating-store"))
    assert counts == {1.0, 2.0, 3.0, 4.0, 6.0, 9.0} and reciprocal >= 8


@pytest.mark.parametrize("dt", DTS)
def test_loss_gradient_operands_bite(dt):
    for nq in A.FLAT_QUADS:
        o = A.l1_operands(dt, nq)
        want = A.l1_bwd_reference(o)
        _accepts(f"l1 {nq}", want)
        _bites(f"l1 nq={nq}: no 1 / numel", want, A.l1_bwd_reference(o, "no-inverse-numel"))
    for n in A.HINGE_N:
        o = hinge_operands(dt, n)
        for mode in (0, 1, 2):
            for use_w in (False, True):
                want = A.hinge_bwd_reference(o, mode, use_w, dt)
                _accepts(f"hinge {n} {mode} {use_w}", want)
                if use_w and n >= 255:
                    _bites(f"hinge n={n} mode={mode}: weight dropped", want, A.hinge_bwd_reference(o, mode, use_w, dt, "no-weight"))


def test_wrap_operands_hold_their_preconditions():
    """The float64 references of the launches past the grid-stride wrap (vectorised torch: seconds, not minutes)."""
    o = A.act_operands("bf16", A.WRAP_QUADS)
    for two in (False, True):
        A.act_bwd_reference(o, "lrelu", two)
    A.blend_reference(A.blend_operands("bf16", A.WRAP_QUADS, 4), "lrelu")
    A.l1_bwd_reference(A.l1_operands("bf16", A.WRAP_QUADS))


# ---------------------------------------------------------------------------------------------------------------------
# rule 5: Adam
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("betas", A.ADAM_BETAS, ids=lambda b: f"beta1-{b[0]}")
def test_adam_operands_hold_the_term_floor_and_bite(betas):
    for numel in A.ADAM_NUMELS[:-1]:
        for scale in A.ADAM_SCALES:
            for step in A.ADAM_STEPS:
                o = A.adam_operands(numel, betas, scale, step)
                want = A.adam_reference(o)
                tag = f"adam n={numel} betas={betas} scale={scale:.3g} step={step}"
                _accepts(tag, want)
                assert not A.rejects(A._adam_formula(o, "none"), want), f"{tag}: the mutants' own formula, unedited, is rejected"
                muts = ["beta2-swapped"]
                if 1 - A.f32r(betas[1]) ** step < 0.999:
                    muts.append("bc2-without-sqrt")                             # (at beta2 = 0.9 and step 1000 the correction is 1 and so is its root)
                if scale != 1.0:
                    muts.append("grad-scale-ignored")
                if betas[0] == 0:
                    muts.append("one-branch-lerp")
                    assert (want["m"].rule == "bits") == (scale != A.ADAM_SCALES[2])
                for mut in muts:
                    _bites(f"{tag}: {mut}", want, A.adam_reference(o, mut))


def test_adam_wrap_operands_and_an_element_left_out_at_the_wrap():
    for i, betas in enumerate(A.ADAM_BETAS):
        o = A.adam_operands(A.ADAM_NUMELS[-1], betas, A.ADAM_SCALES[i], A.ADAM_STEPS[i + 1])
        want = A.adam_reference(o)
        _accepts(f"adam wrap {betas}", want)
        _bites(f"adam wrap {betas}: one element left un-updated at the wrap", want, A.adam_reference(o, "skip-at-wrap"))


# ---------------------------------------------------------------------------------------------------------------------
# the GPU file's own cases on the contract emulator, thinned
# ---------------------------------------------------------------------------------------------------------------------
THIN_GEOMS = [(3, h, w, c) for c in (4, 136) for h, w in ((2, 3), (7, 9), (16, 17))]
THIN_AXIS1 = [(3, 1, 5, 12), (1, 5, 1, 4), (1, 1, 1, 8)]


@pytest.mark.parametrize("dt", DTS)
def test_emulator_returns_what_the_gpu_file_demands(emulator, dt):
    rep = G._Report()
    for geom in THIN_GEOMS + THIN_AXIS1:
        G.upsample_case(rep, dt, geom, "cpu")
        G.avgpool_case(rep, dt, geom, "cpu")
    for geom in THIN_GEOMS:
        G.maxpool_case(rep, dt, geom, "cpu")
    for h, w, p in ((2, 2, 1), (4, 7, 3), (9, 5, 4)):
        G.reflect_case(rep, dt, 3, h, w, 12, p, "cpu")
    for cp, cs, cf in A.ASSEMBLE:
        G.assemble_case(rep, dt, (3, 7, 9), cp, cs, cf, "cpu")
    for nq in (1, 257):
        G.act_case(rep, dt, nq, "cpu")
        G.blend_case(rep, dt, nq, 4, "cpu")
        G.l1_case(rep, dt, nq, "cpu")
    for n in (3, 257):
        G.hinge_case(rep, dt, n, "cpu")
    G.chain_case(rep, dt, "cpu")
    G.reached(emulator, ["mg_upsample2x_fwd", "mg_upsample2x_bwd", "mg_avgpool3s2_fwd", "mg_avgpool3s2_bwd", "mg_maxpool2_fwd", "mg_maxpool2_bwd",
                         "mg_reflect_pad_fwd", "mg_reflect_pad_bwd", "mg_assemble_nhwc8", "mg_act_bwd", "mg_grad_sum_act", "mg_blend_fwd", "mg_blend_bwd",
                         "mg_l1_mean_bwd", "mg_hinge_bwd"])
    assert rep.compared > 100
    rep.done()


def test_emulator_adam_lies_inside_the_intervals(emulator):
    rep = G._Report()
    for betas in A.ADAM_BETAS:
        for scale in A.ADAM_SCALES:
            for step in (1, 1000):
                for numel in (3, 257):
                    G.adam_case(rep, numel, betas, scale, step, "cpu")
    G.reached(emulator, ["mg_adam_step"])
    rep.done()
