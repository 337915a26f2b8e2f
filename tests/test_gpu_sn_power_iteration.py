"""-m gpu: mg_sn_power_iteration (sn_wtu_kernel, sn_finish_v_kernel, sn_wv_kernel, sn_finish_u_kernel of michigan_amd/csrc/mg_weights.hip)
driven from a hand-built mg_sn_layer table (tests/sn_tables.py), at the smallest shapes that cross every boundary of the four kernels'
decode arithmetic: more than one 128-row chunk (full chunks before a ragged one), more than one 1024-column block (the last one 4 or 2
columns wide), second and third trips of the 1024-thread strides of the finishes, nine trips of the 256-column stride, the 4-byte
fallbacks entered through cols & 3 AND through a misaligned W, each with several chunks and column blocks, a single row, and all of that
in ONE table per call, ordered large / small / both-large / smallest / ... / large so that first_block_k1 / _k3 are non-trivial offsets.
One layer of every group runs without u_copy / v_copy.  Every buffer lies between guard regions and starts as NaN.

A  eval mode, exact.  W dense in -2..2, u and v in {-1, 0, 1}: every partial sum of W v and of u . t2 is an integer below 2^24 in any
   order (tests/test_sn_tables.py), so t2 and sigma are torch.equal to the float64 result cast once.  u, v bitwise the inputs; t1, partial
   and the copies still hold the sentinel.
B  training mode, the whole chain exact.  eps = 2^12 is above both norms, so max(sqrt(ss), eps) = eps and both divisions scale by a power
   of two.  W in -2..2 at 8 % density, u in {-1, 0, 1}: t1 = W^T u, v = t1 / eps, t2 = W t1 / eps, u = W t1 / eps^2 and
   sigma = sum (W t1)^2 / eps^3 are integers over powers of two with every partial sum below 2^24 (checked per layer on the CPU; the
   1029 x 2052 layer does not satisfy it and is left out of this group only).  All seven outputs bit for bit against float64.
C  training mode, eps = 1e-12, dense integer W.  t1 and every row of partial[chunks][cols] are exact integers: bit for bit, no sentinel left
   in partial and nothing written behind it.  sum t1^2 is an exact integer below 2^24, so v = fp32(t1) / sqrt(fp32(ss)) evaluated in numpy
   float32 bit for bit (correctly rounded square root and quotient; build.py sets no fast-math flag).  t2, u, sigma as in D.
D  realistic operands (W normals x 0.05, u a normalised normal vector, eps = 1e-12), both modes.  Each kernel is held to its own operation
   on the device's own intermediate, by a bound that is derived here and not fitted:

     fp32 sum of n products along a path of d additions:  |fl(sum) - sum| <= (d + 1) U sum |a_i b_i|,  U = 2^-24     (first order in U;
     the second-order terms are below 1e-5 of the bound and the float64 reference's own error is 2^-29 of it)

   d counts the additions on the longest path of the order the code documents, the +1 is the product's rounding (absent when the product
   is contracted into an fma):
     t1[c]   sn_wtu_kernel adds a chunk's rows one after the other into one accumulator: min(rows, 128); sn_finish_v_kernel adds the
             chunks in ascending order: one per chunk.  d = min(rows, 128) + ceil(rows / 128).             vs float64 W^T u
     t2[r]   sn_wv_kernel: a lane adds its columns c, c + 256, ... into four accumulators: ceil(cols / 256); (a0 + a1) + (a2 + a3): 2; the
             wave tree o = 32 .. 1 of mg_reduce.h: 6.  d = ceil(cols / 256) + 8.                           vs float64 W v_dev
             (the 4-byte fallback walks c, c + 64, ... into one accumulator, ceil(cols / 64) + 6: shorter for 27 columns, 23 instead of
             13 for 1026 / 1028 columns.  The figure above is kept for every layer, so on those two it is the tighter, not the longer.)
     ss, dot (both finishes, mg_block_sum_all<LeftToRight>): a thread's trips over the 1024-thread stride: ceil(n / 1024); the wave tree:
             6; the 16 wave sums joined left to right: 15.  d = ceil(n / 1024) + 21.
     sigma   |sigma - u_dev . t2_dev| <= (d + 1) U sum |u_i t2_i|, n = rows.
     v, u    q = t / max(sqrt(ss), eps): ss is a sum of squares, so its relative error is (d + 1) U; the square root halves it and rounds
             once, the quotient rounds once: |q - t_dev / ||t_dev||| <= ((d + 1) / 2 + 2) U |q| per element.
   Every bound is far below one element: (d + 1) U is at most 138 * 2^-24 = 8.2e-6 of sum |a_i b_i|, the sum has at most 2052 terms, so a
   typical term is > 50 bounds; one dropped square changes a quotient by t^2 / (2 ss) ~ 1 / (2 n) >= 2e-4 relative against 14 U = 8e-7.
   Asserted per layer on the reference side: the median |a_i b_i| of every row / column exceeds its bound (here for the device's
   operands, in tests/test_sn_tables.py for the contract's).  End to end u and v are also held to the contract at 1e-4 of the largest value.

Two routes: under B's operands the per-layer route (ops.spectral_weight: rocBLAS mv + mg_sn_normalize + mg_sn_scale) is exact too; where
numel % 4 == 0 its u and v are bitwise the batched route's and its W / sigma is W / sigma_batched rounded once.

MG_TEST_DRYRUN=1 runs the contract emulator in place of the GPU.  The emulator writes no t1, t2 or partial: the assertions ON those are
skipped there (and only there), and where a check takes a device intermediate as input the float64 one stands in.  Its v is a float64
quotient cast once, not fp32 arithmetic, so C's bitwise v is held to D's bound there.  u, v, sigma and the copies are checked in all groups.
"""
import os

import numpy as np
import pytest
import torch

import sn_tables as S

pytestmark = pytest.mark.gpu

DRY = os.environ.get("MG_TEST_DRYRUN") == "1"
DEV = "cpu" if DRY else "cuda"
EPS = 1e-12

GROUPS = {           # name -> (generator, layers left out, training mode, eps)
    "A": (S.eval_exact_layer, (), False, EPS),
    "B": (S.chain_exact_layer, (S.BOTH_LARGE,), True, S.EPS_EXACT),
    "C": (S.dense_int_layer, (), True, EPS),
    "D-train": (S.realistic_layer, (), True, EPS),
    "D-eval": (S.realistic_layer, (), False, EPS),
}
_RUNS = {}


@pytest.fixture
def backend(request):
    return request.getfixturevalue("emulator_backend" if DRY else "hip_backend")


def _run(group):
    """(layers, result of the one call that takes the whole group's table), computed once per session."""
    if group not in _RUNS:
        make, skip, power, eps = GROUPS[group]
        layers = S.layer_set(make, skip)
        _RUNS[group] = (layers, S.run(layers, power, eps, DEV))
    return _RUNS[group]


def _common(group, fails):
    """What holds for every group: one call, guards intact, W unchanged, copies = the vectors (training) or untouched (eval)."""
    layers, res = _run(group)
    power = GROUPS[group][2]
    if res["guards"] is not None:
        fails.append(res["guards"])
    assert res["calls"].count("mg_sn_power_iteration") == 1
    assert sum(res["k1"]) == res["nblocks"][0] == res["map1"].numel() and sum(res["k3"]) == res["nblocks"][1] == res["map3"].numel()
    for L, o in zip(layers, res["layers"]):
        if not torch.equal(o["w"], L.w):
            fails.append(f"{L}: W changed")
        for k in ("u", "v"):
            c = o[k + "_copy"]
            assert (c is None) == (not L.copies)
            if c is not None and not (S.same_bits(c, o[k]) if power else S.untouched(c)):
                fails.append(f"{L}: {k}_copy " + ("is not bitwise " + k if power else "was written in eval mode"))
        if not power:
            for k in ("t1", "partial"):
                if not S.untouched(o[k]):
                    fails.append(f"{L}: {k} was written in eval mode")
            if not (S.same_bits(o["u"], L.u) and S.same_bits(o["v"], L.v)):
                fails.append(f"{L}: u / v changed in eval mode")
    return layers, res["layers"]


def _bitwise(fails, L, name, got, want64):
    want = want64.float() + 0.0          # a float64 zero may carry either sign; a device sum starts at +0 and is never -0 (mg_reduce.h)
    if not S.same_bits(got, want):
        bad = (S.bits(got) != S.bits(want)).nonzero().flatten()
        fails.append(f"{L}: {name} differs from the float64 result in {bad.numel()} of {want.numel()} elements, first at {int(bad[0])}: "
                     f"{float(got.flatten()[bad[0]])!r} vs {float(want.flatten()[bad[0]])!r}")


def _within(fails, L, name, got, ref, bound):
    """|got - ref| <= bound elementwise (float64; a NaN fails).  Prints the worst ratio."""
    err = (got.double() - ref.double()).abs().reshape(-1)
    bound = torch.as_tensor(bound, dtype=torch.float64).reshape(-1).expand_as(err)
    ok = err <= bound
    worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"{L}: {name}: worst |error| / bound = {worst:.4f}")
    if not bool(ok.all()):
        i = int((~ok).nonzero()[0])
        fails.append(f"{L}: {name}: {int((~ok).sum())} of {err.numel()} elements outside the bound, first at {i}: error {float(err[i]):.3e} > {float(bound[i]):.3e}")


def _judge_second_half(fails, L, o, power, eps):
    """K3 and K4, each on the device's own input: t2 vs W v_dev, u vs t2_dev / ||t2_dev||, sigma vs u_dev . t2_dev."""
    w = L.w.double()
    t2_ref = w @ o["v"].double()
    if DRY:
        t2 = t2_ref
    else:
        t2 = o["t2"]
        _within(fails, L, "t2", t2, t2_ref, S.bound_t2(L.w, o["v"]))
    if power:
        q = S.normalise64(t2, eps)
        _within(fails, L, "u", o["u"], q, S.rel_bound_normalise(L.rows) * q.abs())
    _within(fails, L, "sigma", o["sigma"], (o["u"].double() * t2.double()).sum().reshape(1), S.bound_sigma(o["u"], t2))


def test_eval_mode_exact(backend):
    fails = []
    for L, o in zip(*_common("A", fails)):
        ref = S.contract(L.w, L.u, L.v, False, EPS)
        if not DRY:
            _bitwise(fails, L, "t2", o["t2"], ref["t2"])
        _bitwise(fails, L, "sigma", o["sigma"], ref["sigma"])
    assert not fails, "\n".join(fails)


def test_training_chain_exact(backend):
    fails = []
    for L, o in zip(*_common("B", fails)):
        ref = S.contract(L.w, L.u, L.v, True, S.EPS_EXACT)
        for k in ("t1", "t2") if not DRY else ():
            _bitwise(fails, L, k, o[k], ref[k])
        for k in ("v", "u", "sigma"):
            _bitwise(fails, L, k, o[k], ref[k].double())
    assert not fails, "\n".join(fails)


def test_dense_integer_t1_partial_and_v(backend):
    fails = []
    for L, o in zip(*_common("C", fails)):
        w, u = L.w.double(), L.u.double()
        t1 = w.t() @ u
        ss = S.chain_figures(L)["sum t1^2"]
        assert ss < S.EXACT
        if not DRY:
            _bitwise(fails, L, "t1", o["t1"], t1)
            chunks = -(-L.rows // S.K1_ROWS)
            assert o["partial"].shape == (chunks, L.cols), "partial is sized for another chunk geometry than the kernels'"
            want = torch.stack([w[k * S.K1_ROWS:(k + 1) * S.K1_ROWS].t() @ u[k * S.K1_ROWS:(k + 1) * S.K1_ROWS] for k in range(chunks)])
            if bool((S.bits(o["partial"]) == S.NAN_BITS).any()):
                fails.append(f"{L}: {int((S.bits(o['partial']) == S.NAN_BITS).sum())} elements of partial were never written")
            _bitwise(fails, L, "partial", o["partial"], want)
            _bitwise(fails, L, "v", o["v"], S.f32_normalise(t1.float(), ss, EPS).double())
        else:
            q = S.normalise64(t1, EPS)
            _within(fails, L, "v", o["v"], q, S.rel_bound_normalise(L.cols) * q.abs())
        _judge_second_half(fails, L, o, True, EPS)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_realistic_operands_per_kernel_bounds(backend, mode):
    power = mode == "train"
    fails = []
    for L, o in zip(*_common("D-" + mode, fails)):
        w = L.w.double()
        ref = S.contract(L.w, L.u, L.v, power, EPS)
        if power:
            t1_ref = w.t() @ L.u.double()
            assert bool(((w * L.u.double()[:, None]).abs().median(dim=0).values > S.bound_t1(L.w, L.u)).all()), L
            if DRY:
                t1 = t1_ref
            else:
                t1 = o["t1"]
                _within(fails, L, "t1", t1, t1_ref, S.bound_t1(L.w, L.u))
            q = S.normalise64(t1, EPS)
            _within(fails, L, "v", o["v"], q, S.rel_bound_normalise(L.cols) * q.abs())
            for t in (t1_ref, ref["t2"]):                                    # one dropped square moves a quotient past its bound
                assert float((t * t).median() / (2 * (t * t).sum())) > S.rel_bound_normalise(t.numel()), L
        if bool(torch.isfinite(o["v"]).all()) and bool(torch.isfinite(o["u"]).all()):
            # one dropped or doubled product of typical size fails the bound (the device's own operands)
            assert bool(((w * o["v"].double()[None, :]).abs().median(dim=1).values > S.bound_t2(L.w, o["v"])).all()), L
            assert float((o["u"].double() * ref["t2"]).abs().median()) > S.bound_sigma(o["u"], ref["t2"]), L
        _judge_second_half(fails, L, o, power, EPS)
        for k in ("u", "v"):                                                 # end to end, the rule of test_gpu_kernels._close(.., 1e-4)
            err, scale = float((o[k].double() - ref[k].double()).abs().max()), max(float(ref[k].abs().max()), 1e-6)
            if not (np.isfinite(err) and err <= 1e-4 * scale):
                fails.append(f"{L}: {k} against the contract: max err {err:.3e} > 1e-4 * {scale:.3e}")
    assert not fails, "\n".join(fails)


def test_two_routes_one_answer(backend):
    """ops.spectral_weight (per layer: rocBLAS mv + mg_sn_normalize + mg_sn_scale) on B's operands against the batched table."""
    from michigan_amd import ops

    fails = []
    layers, res = _run("B")
    seen = 0
    for L, o in zip(layers, res["layers"]):
        if (L.rows * L.cols) % 4:
            continue
        seen += 1
        w, u, v = L.w.to(DEV).view(L.rows, L.cols, 1, 1), L.u.to(DEV), L.v.to(DEV)
        with torch.no_grad():
            w_sn = ops.spectral_weight(w, u, v, True, S.EPS_EXACT)
        _bitwise(fails, L, "u of the per-layer route (against the batched route's)", u.cpu(), o["u"].double())
        _bitwise(fails, L, "v of the per-layer route (against the batched route's)", v.cpu(), o["v"].double())
        sigma = np.float32(float(o["sigma"]))
        if not sigma > 0:
            fails.append(f"{L}: sigma of the batched route is {sigma!r}")
            continue
        want = torch.from_numpy(L.w.numpy() / sigma)                        # one fp32 division per element
        _bitwise(fails, L, "W / sigma", w_sn.cpu().view(L.rows, L.cols), want.double())
    assert seen == 5
    assert not fails, "\n".join(fails)
