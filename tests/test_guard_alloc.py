"""The guard-band harness (tests/guard_alloc.py) checked on the CPU, with the contract emulator as the backend:
  * a representative op chain runs under the guard with no damaged guard (the emulator's ``_view`` extents ARE the contract, so
    this also pins that the operator layer never allocates less than the contract says);
  * a stand-in backend that writes one element past / before an output's contract extent is caught and the report names the tensor;
  * a stand-in that reads one element past a guarded input yields a non-finite result;
  * the coverage ledger: every exported entry point is either excluded for one of three stated reasons or has a guarded case in
    one of the four GPU case files (tests/test_gpu_guard_bands.py, test_gpu_style_guard_bands.py, test_gpu_dense_orient.py,
    test_gpu_stroke.py).
Everything here is host memory inside buffers the test owns: no GPU, nothing faults."""
import re

import pytest
import torch

import guard_alloc as GA
import test_gpu_dense_orient as GDO
import test_gpu_guard_bands as GB
import test_gpu_stroke as GS
import test_gpu_style_guard_bands as GSB

ALL_CASES = GB.CASES + GSB.CASES + GDO.CASES + GS.CASES          # the guarded cases of the four GPU case files


@pytest.fixture
def full_emulator():
    """A contract emulator of this test's own as the backend."""
    from michigan_amd import _cabi
    prev = _cabi.set_backend(GB._emulator())
    yield
    _cabi.set_backend(prev)


def test_layout_of_a_guarded_tensor(emulator_backend):
    from michigan_amd import ops
    assert GA.GUARD_BYTES == 256 * 1024                            # a 256 x 256 fp32 tile: the largest footprint one workgroup owns
    with GA.guard() as g:
        assert ops.torch is not torch
        for shape, dtype in (((3, 5, 7), torch.bfloat16), ((1,), torch.float32), ((2, 3), torch.float64), ((13,), torch.uint8)):
            for t in (ops.torch.empty(shape, dtype=dtype), ops.torch.zeros(*shape, dtype=dtype), ops.torch.empty_like(torch.ones(shape, dtype=dtype)),
                      ops.torch.zeros_like(torch.ones(shape, dtype=dtype)), g.guarded(shape, dtype)):
                a = g.allocations[-1]
                assert t.shape == shape and t.dtype == dtype and t.is_contiguous() and t._base is None
                assert t.data_ptr() % GA.ALIGN == 0                                        # the alignment the kernels assume
                assert a.off >= GA.GUARD_BYTES and a.base.numel() - (a.off + a.nbytes) >= GA.GUARD_BYTES
                assert a.nbytes == t.numel() * t.element_size()                            # the upper guard starts at the exact last byte
                assert bool((a.base[:a.off] == 0xFF).all()) and bool((a.base[a.off + a.nbytes:] == 0xFF).all())
        assert float(ops.torch.zeros(4, 4).abs().sum()) == 0.0
        assert not torch.isfinite(ops.torch.empty(4, dtype=torch.float32)).any()          # what a kernel leaves unwritten reads as NaN
        assert ops.torch.empty(3, requires_grad=True).requires_grad
        assert ops.torch.float32 is torch.float32 and ops.torch.autograd is torch.autograd
        assert g.check() == len(g.allocations) > 0
    assert ops.torch is torch


def test_proxy_is_removed_when_the_body_raises(emulator_backend):
    import importlib
    from michigan_amd import _cabi
    mods = [importlib.import_module(m) for m in GA.PATCHED_MODULES]
    be = _cabi.backend()
    with pytest.raises(ZeroDivisionError):
        with GA.guard() as g:
            assert all(m.torch is not torch for m in mods) and _cabi.backend() is g.backend
            1 / 0
    assert all(m.torch is torch for m in mods) and _cabi.backend() is be and g.allocations == []


# the chain of the issue: conv forward and backward, the SPADE pair, instance norm, the three resamplers and reflect pad, blend, l1,
# hinge, gabor, the glue ops, colour and hair-Lab losses, Adam -- the very case functions the GPU file runs, here on the emulator
CHAIN = ["conv-tile128-ktail-ragged-cout-bf16", "conv-stride2-odd-f32", "conv-resid-bf16", "conv-deterministic-generic-f32", "wgrad-3x3-stripe0-2x4x16x64x64",
         "spade-bf16-C48-9x11", "spade-pair-f32-up0", "spade-pair-bf16-up1", "instance_norm-bf16-1x7x9x24-fused1", "instance_norm-f32-3x5x13x4-fused0",
         "norm-bf16-C8-P257-G3-bwdvec1", "apply2-f32-C4-2x18x14-up1-bwdvec1", "stats-f32-C12-P37-G3",
         "upsample2x-2x17x21x20-bf16", "avgpool3s2-2x5x1x20-f32", "maxpool2-2x3x3x12-bf16", "reflect_pad-2x5x7x12x4-f32",
         "blend-1x3x85x12-bf16", "l1_mean-1028-f32", "act_bwd-1020-bf16", "grad_sum_act-1024-f32", "hinge-f32-3x1x17x19", "hinge-bf16-3x1x1x1",
         "gabor-f32-3x17x33x8", "gabor-bwd-exact-bf16-1x5x7x3", "nearest_pyramid-bf16-1x1-level", "pconv-affine-f32-ragged", "bg_compose-bf16-k5",
         "masked_mean_fill-f32-C4-P1", "orient_loss-1x1x1-2ch", "assemble_nhwc8-bf16", "self_attention-f32-n3-L65", "spectral_weight-24x3x3x3-train",
         "batched-net-f32-sink", "color_loss-1x67x35-C8", "hair_lab-3x33x130-C3", "adam_step-257", "input_crop-3x33x37x45x1x32-mode2", "inputs-hole", "inputs-noise40"]


@pytest.mark.parametrize("cid", CHAIN)
def test_clean_run_on_the_emulator(full_emulator, cid):
    from michigan_amd import _cabi, ops
    (c,) = [c for c in GB.CASES if c.id == cid]
    spec = c.build()
    ops.reset_mask_protocol()
    with GA.guard() as g:
        with GB._settings({}, spec.get("flags", {})):
            res = spec["fn"](GB._Ctx(g, "cpu"), *[g.place(t, "cpu") for t in spec["tensors"]])
        n = g.check()                                               # raises GuardDamaged if the op layer under-allocated anything
        assert n >= len([t for t in spec["tensors"] if torch.is_tensor(t)])
        assert all(g.backend.count(ep) for ep in c.covers), sorted(set(g.backend.calls))
        for r in res:
            assert torch.isfinite(r.detach().double()).all(), cid
    assert _cabi.backend().name == "emulator"


def _overrun_backend(where):
    from oracle.cabi_emulator import EmulatorBackend, _TD, _addr, _view

    class Overrun(EmulatorBackend):
        """Writes one element outside the output of mg_upsample2x_fwd: past its contract extent, or before its first element."""

        def mg_upsample2x_fwd(self, x, y, dtype, N, H, W, C, stream=None):
            rc = super().mg_upsample2x_fwd(x, y, dtype, N, H, W, C, stream)
            item = torch.empty((), dtype=_TD[dtype]).element_size()
            at = _addr(y) + (N * 2 * H * 2 * W * C * item if where == "past" else -item)
            _view(at, (1,), _TD[dtype])[0] = 1.0
            return rc
    return Overrun()


@pytest.mark.parametrize("where", ["past", "before"])
def test_a_store_outside_the_contract_extent_is_caught_and_named(where):
    from michigan_amd import _cabi, ops
    prev = _cabi.set_backend(_overrun_backend(where))
    try:
        with GA.guard() as g:
            x = g.place(torch.randn(2, 3, 5, 8).bfloat16())
            y = ops.upsample2x(x)
            ops.avgpool3s2(y)                                       # a later, innocent call: the report must still point at the upsample
            with pytest.raises(GA.GuardDamaged) as e:
                g.check()
    finally:
        _cabi.set_backend(prev)
    msg = str(e.value)
    assert "1 of 3 guarded allocations" in msg, msg
    assert "(2, 6, 10, 8) bfloat16" in msg and "ops.py" in msg and "forward" in msg, msg                     # the tensor and where it was allocated
    assert "first entry point called after it: mg_upsample2x_fwd" in msg and "called last: mg_avgpool3s2_fwd" in msg, msg
    nbytes = 2 * 6 * 10 * 8 * 2
    offset = int(re.search(r"offset ([+-]\d+) relative", msg).group(1))
    assert offset == (nbytes if where == "past" else -2), msg


def test_a_shrunk_workspace_is_caught(emulator_backend):
    """An allocation smaller than what the entry point writes (the silent Python-constant / grid-cap agreements): here the
    emulator writes mean and rstd of C channels into buffers the caller sized for C - 1."""
    from michigan_amd import _cabi, ops
    with GA.guard() as g:
        x = g.place(torch.randn(1, 4, 4, 8))
        sums = ops.channel_sums(x, 1, True)
        mean, rstd = g.guarded((1, 7), torch.float32), g.guarded((1, 7), torch.float32)
        _cabi.backend().mg_norm_finalize(ops._p(sums), 1, 8, 16.0, 1e-5, 0.0, None, None, ops._p(mean), ops._p(rstd), None)
        with pytest.raises(GA.GuardDamaged, match=r"(?s)\(1, 7\) float32 from the test.*offset \+28 relative.*\(1, 7\) float32 from the test"):
            g.check()


def test_a_read_past_a_guarded_input_poisons_the_result():
    from michigan_amd import _cabi, ops
    from oracle.cabi_emulator import EmulatorBackend

    class Overread(EmulatorBackend):
        def mg_l1_mean_fwd(self, a, b, dtype, numel, out, partial, stream=None):
            return super().mg_l1_mean_fwd(a, b, dtype, numel + 1, out, partial, stream)      # one element too far on both inputs

    for dt in (torch.float32, torch.bfloat16):
        outs = []
        for be in (EmulatorBackend(), Overread()):
            prev = _cabi.set_backend(be)
            try:
                with GA.guard() as g:
                    a, b = g.place(torch.randn(64).to(dt)), g.place(torch.randn(64).to(dt))
                    outs.append(float(ops.l1_mean(a, b)))
                    g.check()                                       # a read damages nothing: the value is what shows it
            finally:
                _cabi.set_backend(prev)
        assert outs[0] == outs[0] and outs[0] > 0 and outs[1] != outs[1], outs


def test_u8_poison_reads_255():
    with_guard = GA.Guard()
    t = with_guard.guarded((4,), torch.uint8)
    assert t.tolist() == [255] * 4


# ---- the coverage ledger ------------------------------------------------------------------------------------------------------
NO_DEVICE_WRITE = "writes no device memory: it returns a size, a count, a table on the host, an option, a version or an error text"
NEEDS_SEVERAL_GPUS = "needs more than one GPU or RCCL (tests/test_gpu_multirank.py owns these)"
PROBE = "a hardware-layout probe of the -m gpu suite, not a product kernel"
EXCLUDED = {
    "mg_wgrad_det_workspace": NO_DEVICE_WRITE, "mg_stats_workspace": NO_DEVICE_WRITE, "mg_feat_moment_workspace": NO_DEVICE_WRITE,
    "mg_pack_job_blocks": NO_DEVICE_WRITE, "mg_sn_layer_blocks": NO_DEVICE_WRITE, "mg_grad_slot_blocks": NO_DEVICE_WRITE,
    "mg_bicubic_table": NO_DEVICE_WRITE, "mg_nearest_table": NO_DEVICE_WRITE, "mg_orient_rgb_table": NO_DEVICE_WRITE,
    "mg_bicubic_ksize": NO_DEVICE_WRITE, "mg_noise_field_len": NO_DEVICE_WRITE,
    "mg_set_option": NO_DEVICE_WRITE, "mg_get_option": NO_DEVICE_WRITE, "mg_inputs_set_option": NO_DEVICE_WRITE,
    "mg_abi_version": NO_DEVICE_WRITE, "mg_last_error": NO_DEVICE_WRITE, "mg_sizeof_desc": NO_DEVICE_WRITE, "mg_norm_apply2_supported": NO_DEVICE_WRITE,
    "mg_comm_unique_id": NEEDS_SEVERAL_GPUS, "mg_comm_init": NEEDS_SEVERAL_GPUS, "mg_comm_destroy": NEEDS_SEVERAL_GPUS, "mg_comm_world": NEEDS_SEVERAL_GPUS,
    "mg_allreduce_stats": NEEDS_SEVERAL_GPUS, "mg_allreduce_grads": NEEDS_SEVERAL_GPUS,
    "mg_probe_mfma_layout": PROBE, "mg_probe_tr16": PROBE,
}


def test_every_device_writing_entry_point_has_a_guarded_case():
    from michigan_amd import _cabi
    exported = set(_cabi.EXPORTED_SYMBOLS)
    assert set(EXCLUDED) <= exported, sorted(set(EXCLUDED) - exported)
    for fn, why in EXCLUDED.items():                                # the three admissible reasons, and only where the name says so
        if why == NEEDS_SEVERAL_GPUS:
            assert fn.startswith(("mg_comm_", "mg_allreduce_")), fn
        elif why == PROBE:
            assert fn.startswith("mg_probe_"), fn
        else:
            assert why == NO_DEVICE_WRITE and (fn.endswith(("_workspace", "_blocks", "_table", "_option", "_supported")) or fn in (
                "mg_bicubic_ksize", "mg_noise_field_len", "mg_abi_version", "mg_last_error", "mg_sizeof_desc")), fn
    covered = {ep for c in ALL_CASES for ep in c.covers}
    assert covered <= exported, sorted(covered - exported)
    assert not covered & set(EXCLUDED)
    missing = sorted(exported - set(EXCLUDED) - covered)
    assert not missing, "entry points without a guarded case in the four GPU case files (add one, at its tile-edge geometries): %s" % missing
    assert len(EXCLUDED) == 26 and len(exported) - len(EXCLUDED) == len(covered) == 63
    assert len({c.id for c in ALL_CASES}) == len(ALL_CASES)
