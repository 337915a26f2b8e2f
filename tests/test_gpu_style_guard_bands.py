"""-m gpu: the device-writing entry points of michigan_hip/feature_losses.h inside guard bands
(tests/guard_alloc.py), with the machinery of tests/test_gpu_guard_bands.py: each case runs ops.feat_moment_loss forward and backward
under the guard on the HIP backend, runs the same function on CPU copies with the float64 contract emulator
(oracle/cabi_emulator.py), compares, checks every guard byte and asserts through the call-counting backend that
mg_feat_moment_loss_fwd / _bwd were each called exactly once.  Geometries: one below, exactly at and one above
  * the pixel-chunk multiple (bf16, C = 16: a workgroup row is 128 pixels, the smallest chunk 512 pixels: P = 511, 512, 513), and
  * the channel-tile multiple (fp32: a workgroup owns 256 four-channel vectors: C = 1020, 1024, 1028),
each unmasked and under masks.  ``CASES`` is part of the ledger tests/test_guard_alloc.py checks against ``_cabi.EXPORTED_SYMBOLS``.
Bounds: those of tests/test_gpu_style_loss.py.

Also here: this package's trainer on the kernels, with the style and content terms on, against the reference trainer's record
(tests/golden/trainer_S*.npz) -- the fp32 protocol and tolerances of tests/test_gpu_unpaired.py.
"""
import collections

import pytest
import torch

import parity_utils as PU
import style_loss_fixtures as SE
import test_gpu_guard_bands as GB
from oracle import trainer_parity as TP

pytestmark = pytest.mark.gpu

Case = collections.namedtuple("Case", "id covers build")
CASES = []
COVERS = ("mg_feat_moment_loss_fwd", "mg_feat_moment_loss_bwd")


def _spec(n, h, w, c, dt, masked):
    from michigan_amd import ops
    g = GB._gen(h * w + c)
    dtype = GB.DT[dt]
    feats = lambda shift: (shift + torch.randn(n, h, w, c, generator=g)).relu().to(dtype)
    x, s, t = feats(0.3).requires_grad_(True), feats(0.1), feats(0.2)
    lab = torch.stack([(torch.rand(n, h, w, generator=g) < 0.6).float() * (0.5 + 0.5 * (torch.rand(n, h, w, generator=g) < 0.8).float())
                       for _ in range(3)], dim=1)
    lab[:, :, -1, -1] = 1.0                                        # the last pixel of every plane is read

    def fn(ctx, x, s, t, lab):
        view = lambda f: f.permute(0, 3, 1, 2)
        masks = [lab[:, i] for i in range(3)] if masked else [None] * 3
        out = ops.feat_moment_loss(view(x), view(s), view(t), *masks, flags=3)
        (gx,) = torch.autograd.grad(SE.WEIGHTS[0] * out[0] + SE.WEIGHTS[1] * out[1], x)
        return torch.stack([o.detach() for o in out]), gx
    nm = "feat moments %s %s C=%d %s" % ((n, h, w), dt, c, "masked" if masked else "plain")
    bounds = (1e-4, 8 * 2.0 ** -23) if dt == "f32" else (2e-2, 2.0 ** -8)
    return dict(fn=fn, tensors=[x, s, t, lab], checks=[(nm + " losses", GB._scalar(bounds[0])), (nm + " dx", GB._rel_l2(bounds[1]))],
                geometry=(dt == "bf16", n, h * w, c))


for _p in (511, 512, 513):
    for _masked in (False, True):
        CASES.append(Case("feat_moments-chunk-bf16-2x1x%dx16-%s" % (_p, "masked" if _masked else "plain"), COVERS,
                          lambda p=_p, m=_masked: _spec(2, 1, p, 16, "bf16", m)))
for _c in (1020, 1024, 1028):
    for _masked in (False, True):
        CASES.append(Case("feat_moments-ctile-f32-2x3x5x%d-%s" % (_c, "masked" if _masked else "plain"), COVERS,
                          lambda c=_c, m=_masked: _spec(2, 3, 5, c, "f32", m)))


def test_the_cases_sit_on_the_kernels_edges(hip_backend):
    """The geometry the ids claim, from the mirror of the kernels' chunking -- itself held to the library's workspace size."""
    geo = lambda cid: SE.kernel_geometry(*[c for c in CASES if c.id.startswith(cid)][0].build()["geometry"])
    for c in CASES:
        _, n, p, ch = c.build()["geometry"]
        assert hip_backend.mg_feat_moment_workspace(n, p, ch) == SE.workspace_layout_bytes(n, p, ch), "tests/style_loss_fixtures.kernel_geometry is stale"
    below, at, above = (geo("feat_moments-chunk-bf16-2x1x%d" % p) for p in (511, 512, 513))
    assert below["rows"] == 128 and (below["nchunks"], at["nchunks"], above["nchunks"]) == (1, 1, 2) and at["chunk"] == 512
    below, at, above = (geo("feat_moments-ctile-f32-2x3x5x%d" % c) for c in (1020, 1024, 1028))
    assert (below["cv"], at["cv"], above["cv"]) == (255, 256, 257) and (below["ctiles"], at["ctiles"], above["ctiles"]) == (1, 1, 2)


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_guarded(monkeypatch, c):
    import guard_alloc as GA
    counted = []
    orig = GA.Guard.check

    def check(self):                                                # _run checks inside the guard: read the call counts there
        counted.append({ep: self.backend.count(ep) for ep in c.covers})
        return orig(self)
    monkeypatch.setattr(GA.Guard, "check", check)
    assert GB._run(c.build(), c.covers) >= 4
    assert counted == [{ep: 1 for ep in c.covers}], counted         # one forward call (two launches), one backward call


def test_trainer_fp32_with_style_and_content_matches_reference_trainer_golden(hip_backend):
    from michigan_amd.model import Pix2PixTrainer
    cfg = dict(TP.CFGS["A"], tag="S")
    torch.manual_seed(0)
    trainer = Pix2PixTrainer(TP.repo_options(cfg, gpu_ids=[0], compute_dtype="fp32", no_style_loss=False, no_content_loss=False))
    SE.load_weights(trainer, cfg)
    rec = SE.drive_style(trainer, cfg, device="cuda")
    print("trainer S losses", {k: float(v) for k, v in rec.items() if ".loss." in k})
    gold = PU.load_trainer_golden("S")
    assert {k for k in rec if ".loss." in k} == {k for k in gold if ".loss." in k}
    TP.compare(rec, gold, rtol_loss0=5e-4, rtol_later=TP.RTOL_LATER_HIP, atol_img=1e-3, atol_weight=2 * 4e-4 * 2 + 1e-5)
