"""CPU: the table-level spectral-norm helper (tests/sn_tables.py) on the contract emulator, and the preconditions of the exact operand
groups of tests/test_gpu_sn_power_iteration.py, checked in integer arithmetic without any backend.

What "exact" rests on: an fp32 sum of integers whose absolute values add up to less than 2^24 is the same in any order, and a division by a
power of two changes no significand.  So the figures of sn_tables.eval_figures / chain_figures have to stay below 2^24 for every layer an
exact group uses; group B leaves out the 1029 x 2052 layer, whose sum (W t1)^2 does not (shown here), and nothing else.
"""
import pytest
import torch

import sn_tables as S

A_LAYERS = S.layer_set(S.eval_exact_layer)
B_LAYERS = S.layer_set(S.chain_exact_layer, skip=(S.BOTH_LARGE,))
C_LAYERS = S.layer_set(S.dense_int_layer)
D_LAYERS = S.layer_set(S.realistic_layer)


def test_layer_set_and_order():
    shapes = [(L.rows, L.cols) for L in A_LAYERS]
    assert set(shapes) == {(1029, 36), (130, 2052), (128, 1024), (257, 1026), (129, 27), (130, 1028), (5, 27), (1, 8), (1029, 2052)}
    assert [(L.rows, L.cols) for L in B_LAYERS] == [s for s in shapes if s != (1029, 2052)]            # B's one permitted omission
    for layers in (A_LAYERS, B_LAYERS, C_LAYERS, D_LAYERS):
        assert [L.copies for L in layers].count(False) == 1                                            # one layer per group without copies
        assert [L.misalign for L in layers].count(True) == 1 and [L for L in layers if L.misalign][0].cols % 4 == 0
        k1 = [-(-L.cols // 1024) * -(-L.rows // 128) for L in layers]                                  # K1 workgroups
        size = [L.rows * L.cols for L in layers]
        assert k1[0] >= 6 and k1[-1] >= 6 and size.index(min(size)) in (len(size) // 2 - 1, len(size) // 2)   # large, ..., smallest, ..., large


def test_group_a_preconditions():
    for L in A_LAYERS:
        f = S.eval_figures(L)
        assert S.exact(f), (L, f)
        assert int(L.w.abs().max()) == 2 and set(L.u.tolist()) <= {-1.0, 0.0, 1.0} and set(L.v.tolist()) <= {-1.0, 0.0, 1.0}
        ref = S.contract(L.w, L.u, L.v, False, 1e-12)
        assert S.held_by_fp32(ref["t2"]) and S.held_by_fp32(ref["sigma"])
        assert bool(ref["t2"].abs().sum() > 0), L                          # nothing degenerate: a t2 of zeros would pass with W unread
    assert sum(1 for L in A_LAYERS if float(S.contract(L.w, L.u, L.v, False, 1e-12)["sigma"]) != 0) >= len(A_LAYERS) - 1


def test_group_b_preconditions():
    eps = S.EPS_EXACT
    assert eps == 2.0 ** 12
    for L in B_LAYERS:
        f = S.chain_figures(L)
        assert S.exact(f), (L, f)
        assert set(L.w.unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0} and set(L.u.tolist()) <= {-1.0, 0.0, 1.0}
        if L.rows * L.cols >= 4096:
            assert 0.07 < float((L.w != 0).float().mean()) < 0.09
        # eps is above both norms: ||t1|| = sqrt(sum t1^2) < 2^12, and ||t2|| = sqrt(sum (W t1)^2) / eps < 1
        assert f["sum t1^2"] < eps * eps and f["sum (W t1)^2"] < eps ** 4
        ref = S.contract(L.w, L.u, L.v, True, eps)
        # the reference alone stays within the cap: every float64 value of the chain is an fp32 value, so casting it once loses nothing
        for k in ("t1", "t2", "sigma"):
            assert S.held_by_fp32(ref[k]), (L, k)
        w, u = L.w.double(), L.u.double()
        t1 = w.t() @ u
        assert torch.equal(ref["v"].double(), t1 / eps) and torch.equal(ref["t2"], (w @ t1) / eps)
        assert torch.equal(ref["u"].double(), (w @ t1) / eps ** 2) and float(ref["sigma"]) == f["sum (W t1)^2"] / eps ** 3
        assert float(ref["sigma"]) > 0, L                                   # the chain reaches sigma with something in it
        assert float(ref["sigma"]) >= 2.0 ** -100 and float(ref["u"].abs()[ref["u"] != 0].min()) >= 2.0 ** -100      # far from subnormal


def test_group_b_needs_the_sparse_operands():
    both = S.chain_figures(S.chain_exact_layer(*S.BOTH_LARGE))
    assert not S.exact(both), both                                          # why group B leaves the 1029 x 2052 layer out
    dense = [S.chain_figures(L) for L in S.layer_set(lambda r, c, m: S.chain_exact_layer(r, c, m, density=0.25), skip=(S.BOTH_LARGE,))]
    assert not all(S.exact(f) for f in dense), dense                        # at 25 % density the bounds do not hold


def test_group_c_preconditions():
    for L in C_LAYERS:
        f = S.chain_figures(L)
        assert S.exact(f, S.T1_KEYS), (L, f)                                # t1, every partial and sum t1^2 are exact
        assert f["sum t1^2"] > 0, L
        t1 = S.contract(L.w, L.u, L.v, True, 1e-12)["t1"]
        v = S.f32_normalise(t1.float(), f["sum t1^2"], 1e-12)
        assert bool(torch.isfinite(v).all()) and abs(float(v.double().norm()) - 1) < 1e-5


def test_group_d_bounds_catch_one_element():
    """One dropped or doubled product of typical size exceeds each a-priori bound: the median |a_i b_i| of every column (t1), row (t2) and of
    u . t2 (sigma) is above that sum's bound, and dropping one median square from ||t||^2 moves the quotient by more than its bound."""
    for L in D_LAYERS:
        w, u0, v0 = L.w.double(), L.u.double(), L.v.double()
        for power in (True, False):
            ref = S.contract(L.w, L.u, L.v, power, 1e-12)
            u, v = ref["u"].double(), ref["v"].double()
            if power:
                assert bool(((w * u0[:, None]).abs().median(dim=0).values > S.bound_t1(L.w, L.u)).all()), L
                for t in (ref["t1"], ref["t2"]):
                    assert float((t * t).median() / (2 * (t * t).sum())) > S.rel_bound_normalise(t.numel()), L
            assert bool(((w * v[None, :]).abs().median(dim=1).values > S.bound_t2(L.w, ref["v"])).all()), L
            assert float((u * ref["t2"]).abs().median()) > S.bound_sigma(ref["u"], ref["t2"]), L


@pytest.mark.parametrize("power", [True, False], ids=["train", "eval"])
def test_helper_on_the_emulator(emulator_backend, power):
    """Plumbing: table layout, block maps that sum to the launch sizes, one call, intact guards, and the emulator's answer is the contract."""
    layers, eps = (D_LAYERS, 1e-12)
    res = S.run(layers, power, eps, "cpu")
    assert res["guards"] is None, res["guards"]
    assert res["calls"].count("mg_sn_power_iteration") == 1
    n = len(layers)
    for counts, first, bmap, total in ((res["k1"], res["first_k1"], res["map1"], res["nblocks"][0]),
                                       (res["k3"], res["first_k3"], res["map3"], res["nblocks"][1])):
        assert all(c > 0 for c in counts) and sum(counts) == total == bmap.numel()
        assert first == [sum(counts[:i]) for i in range(n)]
        for i in range(n):
            assert bool((bmap[first[i]:first[i] + counts[i]] == i).all())
    for L, o in zip(layers, res["layers"]):
        ref = S.contract(L.w, L.u, L.v, power, eps)
        assert torch.equal(o["w"], L.w)
        assert o["partial"].shape == (o["chunks"], L.cols)
        assert S.same_bits(o["u"], ref["u"]) and S.same_bits(o["v"], ref["v"]) and S.same_bits(o["sigma"], ref["sigma"].float()), L
        assert (o["u_copy"] is None) == (not L.copies) and (o["v_copy"] is None) == (not L.copies)
        if L.copies:
            if power:
                assert S.same_bits(o["u_copy"], o["u"]) and S.same_bits(o["v_copy"], o["v"])
            else:
                assert S.untouched(o["u_copy"]) and S.untouched(o["v_copy"])
        for k in ("t1", "t2", "partial"):                                   # the emulator has no scratch: the sentinel survives
            assert S.untouched(o[k]), (L, k)


def test_helper_exact_groups_on_the_emulator(emulator_backend):
    """The exact groups through the same plumbing: the emulator (float64, cast once) gives the exact values bit for bit."""
    for layers, power, eps in ((A_LAYERS, False, 1e-12), (B_LAYERS, True, S.EPS_EXACT)):
        res = S.run(layers, power, eps, "cpu")
        assert res["guards"] is None, res["guards"]
        for L, o in zip(layers, res["layers"]):
            ref = S.contract(L.w, L.u, L.v, power, eps)
            assert S.same_bits(o["u"], ref["u"]) and S.same_bits(o["v"], ref["v"]) and S.same_bits(o["sigma"], ref["sigma"].float()), L
