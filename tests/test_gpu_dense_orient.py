"""-m gpu: dense hair-orientation extraction on the kernels.

1. mg_orient_smooth alone inside guard bands (tests/guard_alloc.py, the machinery of tests/test_gpu_guard_bands.py): each case runs
   ops.orient_smooth under the guard on the HIP backend and on CPU copies with the float64 contract emulator
   (oracle/cabi_emulator.py), with idx and conf from the contract of mg_gabor_argmax_fwd on BOTH sides, so ties cannot
   differ; every guard byte is checked, a second run must be bit-identical, and the call-counting backend asserts one call per run.
   Geometries: 2x17x17 (radius 16 reflects onto the far edge; the batch stride 289 is odd), 2x33x47, 2x70x95, and one below / exactly
   at / one above the kernel's tile in each axis (dense_orient_fixtures.kernel_geometry, held to the header the kernel is compiled
   from); `angle` null and non-null.  ``CASES`` is part of the ledger tests/test_guard_alloc.py checks against ``_cabi.EXPORTED_SYMBOLS``.
   Bounds: rule 2 of tests/test_dense_orient.py (bytes equal on >= 99.5 % of the compared pixels, within one level on all, the angle
   within 8 x the reference's own fp32-vs-float64 gap of the synthetic fixture, every byte outside the mask equal).
2. The kernel on the reference's own idx and conf, and inputs.dense_orientation end to end, against both fixtures
   (tests/golden/dense_orient_{i,ii}.npz).  End to end an arg-max flip moves one of 33^2 weighted contributions, so the bounds are
   arg-max agreement > 0.999 (the bound of the Gabor cases of tests/test_gpu_kernels.py), bytes equal on >= 99 % of the compared
   pixels and within one level on >= 99.9 %: this one catches wiring errors, test 1 is the strict one.
3. The argument checks: h < 17 and a null table come back through mg_last_error, nothing is launched.
"""
import collections
import math

import numpy as np
import pytest
import torch

import dense_orient_fixtures as DE
import parity_utils as PU
import test_gpu_guard_bands as GB
from oracle import contracts as K
from oracle.cabi_emulator import EmulatorBackend

pytestmark = pytest.mark.gpu

Case = collections.namedtuple("Case", "id covers build")
CASES = []
COVERS = ("mg_orient_smooth",)
EDGE = 40                                                                  # the other axis of a tile-edge case: more than one tile
TILE_CASES = [(DE.TILE_H + d, EDGE) for d in (-1, 0, 1)] + [(EDGE, DE.TILE_W + d) for d in (-1, 0, 1)]
_FIXTURES = {}


def _fixture(tag):
    if tag not in _FIXTURES:
        _FIXTURES[tag] = DE.load_set(tag)
    return _FIXTURES[tag]


def _check(pseudo, want_angle):
    """rule 2 of the kernel's (u8, angle) against the contract's, both stacked into one float64 tensor by the case function"""
    def check(name, a, r):
        assert torch.isfinite(a).all(), name + ": non-finite angle"
        rec = pseudo["geometries"]["case"]
        assert np.array_equal(r[0].numpy().astype(np.uint8), rec["u8"]), name + ": the two contract runs differ"
        got = {"case": dict(u8=a[0].numpy().astype(np.uint8), theta=a[1].numpy() if want_angle else rec["level"] * math.pi / 255.0)}
        ok, fig = DE.rule2(got, pseudo)
        print(name, fig)
        assert ok, "%s: %s" % (name, fig)
    return check


def _spec(n, h, w, want_angle):
    from michigan_amd import ops
    image, mask = DE.strand_image(n, h, w, 7000 + 100 * h + w)
    mask[:, -1, -1] = 1                                                    # the last pixel of every plane is in the mask
    conf, idx = K.argmax_contract(DE.image_fp32(image), ops.dog_bank())
    conf, idx = torch.from_numpy(conf).float(), torch.from_numpy(idx).to(torch.uint8)
    want = K.smooth_contract(conf.numpy(), idx.numpy(), mask.numpy(), ops.orient_trig_table().numpy(), ops.gaussian_taps(4.0).numpy())
    magnitude = np.hypot(want["bx"], want["by"])
    pseudo = dict(geometries={"case": dict(mask=mask.numpy(), magnitude=magnitude, u8=want["u8"], level=want["level"])},
                  magnitude_max=float(magnitude[mask.numpy() != 0].max()), ref32_level_gap=_fixture("i")["ref32_level_gap"])

    def fn(ctx, conf, idx, mask):
        res = ops.orient_smooth(conf, idx, mask, want_angle=want_angle)
        u8, angle = res if want_angle else (res, None)
        again = ops.orient_smooth(conf, idx, mask, want_angle=want_angle)
        u8_2, angle_2 = again if want_angle else (again, None)
        assert torch.equal(u8, u8_2) and (angle is None or torch.equal(angle, angle_2)), "two runs are not bit-identical"
        return (torch.stack([u8.double(), angle.double() if want_angle else torch.zeros_like(u8, dtype=torch.float64)]),)
    nm = "orient smooth %s %s" % ((n, h, w), "angle" if want_angle else "no angle")
    return dict(fn=fn, tensors=[conf, idx, mask], checks=[(nm, _check(pseudo, want_angle))], geometry=(n, h, w))


for _h, _w in DE.SYNTHETIC_SHAPES + tuple(TILE_CASES):
    CASES.append(Case("orient_smooth-2x%dx%d-angle" % (_h, _w), COVERS, lambda h=_h, w=_w: _spec(2, h, w, True)))
for _h, _w in ((17, 17), (DE.TILE_H + 1, DE.TILE_W + 1)):
    CASES.append(Case("orient_smooth-2x%dx%d-noangle" % (_h, _w), COVERS, lambda h=_h, w=_w: _spec(2, h, w, False)))


def test_the_cases_sit_on_the_kernels_edges():
    """The mirror is the tile the kernel is compiled with (the header's defines), and the ids' geometry is what the cases build."""
    d = PU.header_defines("michigan_hip/preprocess/dense_orient.h")
    assert (d["MG_ORIENT_TILE_H"], d["MG_ORIENT_TILE_W"], d["MG_ORIENT_RADIUS"]) == (DE.TILE_H, DE.TILE_W, DE.RADIUS)
    tiles = lambda h, w: (DE.kernel_geometry(2, h, w)["tiles_y"], DE.kernel_geometry(2, h, w)["tiles_x"])
    assert [tiles(h, w) for h, w in TILE_CASES] == [(1, 2), (1, 2), (2, 2), (2, 1), (2, 1), (2, 2)]
    assert tiles(17, 17) == (1, 1) and tiles(70, 95) == (3, 3)
    for c in CASES:
        n, h, w = c.build()["geometry"]
        assert c.id.startswith("orient_smooth-%dx%dx%d-" % (n, h, w))


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_guarded(monkeypatch, c):
    import guard_alloc as GA
    counted = []
    orig = GA.Guard.check

    def check(self):                                                # _run checks inside the guard: read the call counts there
        counted.append({ep: self.backend.count(ep) for ep in c.covers})
        return orig(self)
    monkeypatch.setattr(GA.Guard, "check", check)
    assert GB._run(c.build(), c.covers) >= 5                        # three inputs and at least two outputs under guard
    assert counted == [{ep: 2 for ep in c.covers}], counted         # the run and its repetition, one launch each


def _on_device(fn):
    """fn() on the HIP backend (or, with MG_TEST_DRYRUN=1, on the emulator: plumbing check without a GPU)"""
    from michigan_amd import _cabi
    prev = _cabi.set_backend(EmulatorBackend() if GB.DRY else None)
    try:
        if not GB.DRY:
            assert _cabi.backend().name == "hip"
        return fn("cpu" if GB.DRY else "cuda")
    finally:
        _cabi.set_backend(prev)


@pytest.mark.parametrize("tag", ["i", "ii"])
def test_kernel_on_the_references_idx_and_conf(tag):
    """rule 2 against the reference's float64 run itself, the kernel fed with what the reference computed before the smoothing"""
    from michigan_amd import ops
    fx = _fixture(tag)

    def run(dev):
        got = {}
        for geo, rec in fx["geometries"].items():
            t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
            u8, angle = ops.orient_smooth(t(rec["conf"], torch.float32), t(rec["idx"], torch.uint8), t(rec["mask"], torch.uint8), want_angle=True)
            got[geo] = dict(u8=u8.cpu().numpy(), theta=angle.cpu().numpy())
        return got
    ok, fig = DE.rule2(_on_device(run), fx)
    print("set %s: %s" % (tag, fig))
    assert ok, fig


@pytest.mark.parametrize("tag", ["i", "ii"])
def test_dense_orientation_end_to_end(tag):
    from michigan_amd import inputs
    fx = _fixture(tag)

    def run(dev):
        from michigan_amd import ops
        got = {}
        for geo, rec in fx["geometries"].items():
            image, mask = torch.from_numpy(rec["image"]).to(dev), torch.from_numpy(rec["mask"]).to(dev)
            u8 = inputs.dense_orientation(image, mask)
            conf, idx = ops.gabor_argmax(DE.image_fp32(image), ops.dog_bank(dev))
            rgb = inputs.orient_to_rgb_u8(u8, mask, inputs.orient_rgb_table(dev))              # no conversion in between
            assert rgb.shape == u8.shape + (3,) and rgb.dtype == torch.uint8
            got[geo] = dict(u8=u8.cpu().numpy(), idx=idx.cpu().numpy())
        return got
    got = _on_device(run)
    d, agree, pixels, excluded, inmask = [], 0, 0, 0, 0
    for geo, rec in fx["geometries"].items():
        keep, ex, im = DE.compared(rec["mask"], rec["magnitude"], fx["magnitude_max"])
        excluded, inmask = excluded + ex, inmask + im
        d.append(DE.circular(got[geo]["u8"][keep], rec["u8"][keep]))
        agree += int((got[geo]["idx"] == rec["idx"]).sum())
        pixels += rec["idx"].size
        assert not got[geo]["u8"][rec["mask"] == 0].any()
    d = np.concatenate(d)
    print("set %s: arg-max agreement %.5f, bytes equal %.5f, within one level %.5f, excluded %.5f" % (tag, agree / pixels, (d == 0).mean(), (d <= 1).mean(), excluded / inmask))
    assert excluded / inmask <= DE.MAX_EXCLUDED
    assert agree / pixels > 0.999
    assert (d == 0).mean() >= 0.99 and (d <= 1).mean() >= 0.999


def test_argument_checks_return_errors(hip_backend):
    from michigan_amd import ops
    p = lambda t: None if t is None else t.data_ptr()
    conf = torch.zeros(1, 16, 40, device="cuda")
    idx = torch.zeros(1, 16, 40, dtype=torch.uint8, device="cuda")
    out = torch.full((1, 16, 40), 7, dtype=torch.uint8, device="cuda")
    trig, taps = ops.orient_trig_table().cuda(), ops.gaussian_taps(4.0).cuda()
    with pytest.raises(RuntimeError, match="mg_orient_smooth: bad geometry"):
        hip_backend.mg_orient_smooth(p(conf), p(idx), p(idx), p(trig), p(taps), p(out), None, 1, 16, 40, None)
    with pytest.raises(RuntimeError, match="mg_orient_smooth: bad geometry"):
        hip_backend.mg_orient_smooth(p(conf), p(idx), p(idx), p(trig), p(taps), p(out), None, 1, 40, 16, None)
    with pytest.raises(RuntimeError, match="mg_orient_smooth: null pointer"):
        hip_backend.mg_orient_smooth(p(conf), p(idx), p(idx), None, p(taps), p(out), None, 1, 20, 32, None)
    torch.cuda.synchronize()
    assert bool((out == 7).all())                                    # nothing was launched
