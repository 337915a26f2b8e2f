"""-m gpu: the stroke route on the kernels of mg_stroke.hip.

1. Each entry point alone inside guard bands (tests/guard_alloc.py, the machinery of tests/test_gpu_guard_bands.py): a case runs the
   op under the guard on the HIP backend and on CPU copies with the contract emulator (oracle/cabi_emulator.py); every guard byte is
   checked, a second run must be bit-identical, and the call-counting backend asserts one call per run.  ``CASES`` is part of the
   ledger tests/test_guard_alloc.py checks against ``_cabi.EXPORTED_SYMBOLS``.
   mg_stroke_orient: 2x1x1, 2x5x40 (smaller than the filter radius), 2x17x17, 2x33x47, one below / exactly at / one above the kernel's
   tile in each axis (stroke_fixtures.kernel_geometry, held to the header the kernel is compiled from), an all-zero mask (zeros
   everywhere), a single stroke pixel in the last position, and a seeded bank without point symmetry (a correlation, not a
   convolution); idx / conf null and non-null.  Bound: the rule of tests/test_stroke.py against the float64 contract on the case's
   mask, tau from tests/golden/stroke_i.npz (4 x the reference's own fp32-against-float64 figures).
   mg_stroke_compose / mg_inpaint_finish: fp32 and bf16 at 2x32x32 -> 256^2 and 2x33x47 with identity tables, with and without
   strokes; bit-identical to the torch expressions on the CPU (rounded once for bf16).
2. Both fixtures end to end: inputs.stroke_to_orient on the masks of stroke_i.npz under the rule; SInpaintGenerator in fp32 against
   the reference's output (< 1e-3) and Pix2PixModel.inpainting_stroke_orient on both branches (rgb < 1e-3, orient < 2e-3) -- the
   bounds tests/test_inpaint.py uses for the sister net.  In bf16 only finiteness is asserted and mean / median / max are printed
   (recorded in profiles/stroke_edit.txt: a bound comes later from that record, not from this code).
"""
import collections

import numpy as np
import pytest
import torch

import parity_utils as PU
import stroke_fixtures as SE
import test_gpu_guard_bands as GB
from oracle import contracts as K
from oracle.cabi_emulator import EmulatorBackend

pytestmark = pytest.mark.gpu

Case = collections.namedtuple("Case", "id covers build")
CASES = []
EDGE = 20                                                                  # the other axis of a tile-edge case: more than one tile
TILE_CASES = [(SE.TILE_H + d, EDGE) for d in (-1, 0, 1)] + [(EDGE, SE.TILE_W + d) for d in (-1, 0, 1)]
_FIXTURES = {}


def _fixture():
    if "i" not in _FIXTURES:
        _FIXTURES["i"] = SE.load_set("i")
    return _FIXTURES["i"]


def _mask(kind, n, h, w):
    if kind == "zero":
        return np.zeros((n, h, w), np.uint8)
    if kind == "last":
        m = np.zeros((n, h, w), np.uint8)
        m[-1, -1, -1] = 1                                                  # the very last byte of the map
        return m
    m = SE.polyline_mask(n, h, w, 8000 + 100 * h + w)
    m[:, -1, -1] = 1                                                       # the last pixel of every plane is a stroke pixel
    if (h, w) == (1, 1):
        m[1] = 0                                                           # 2x1x1: one stroke pixel, one empty canvas
    return m


def _orient_spec(n, h, w, extras, kind="lines", asymmetric=False):
    from michigan_amd import ops
    mask = _mask(kind, n, h, w)
    bank = SE.asymmetric_bank() if asymmetric else ops.dog_bank().numpy()
    pseudo = SE.pseudo_fixture(mask, bank, _fixture())

    def fn(ctx, stroke, bank):
        kw = dict(want_idx=extras, want_conf=extras, bank=bank if asymmetric else None)
        res, again = ops.stroke_orient(stroke, **kw), ops.stroke_orient(stroke, **kw)
        res, again = (res, again) if extras else ((res,), (again,))
        assert all(torch.equal(a, b) for a, b in zip(res, again)), "two runs are not bit-identical"
        planes = [res[0].permute(0, 3, 1, 2).double()] + [t.double().unsqueeze(1) for t in res[1:]]
        return (torch.cat(planes, dim=1),)                                 # [N, 3 (+ idx + conf), H, W]

    def check(name, a, r):
        assert torch.isfinite(a).all(), name + ": non-finite"
        want = K.stroke_contract(mask, bank, _fixture()["rgb_table"])
        rgb = a[:, :3].permute(0, 2, 3, 1).numpy().astype(np.uint8)
        assert np.array_equal(r[:, :3].permute(0, 2, 3, 1).numpy().astype(np.uint8), want["rgb"]), name + ": the two contract runs differ"
        s = mask != 0
        if extras:
            got = dict(rgb=rgb, idx=a[:, 3].numpy().astype(np.uint8), conf=a[:, 4].numpy())
        else:                                                              # without idx the picture must name an index that passes: invert the table
            table = _fixture()["rgb_table"].astype(np.int64)
            code = {tuple(c): k for k, c in reversed(list(enumerate(table.tolist())))}
            idx = np.array([code.get(tuple(c), 255) for c in rgb[s].tolist()], np.int64)
            assert (idx < 32).all(), name + ": a colour outside the table"
            full = np.zeros(mask.shape, np.uint8)
            full[s] = idx
            got = dict(rgb=rgb, idx=full, conf=np.where(s, np.maximum(pseudo["geometries"]["case"]["resp"], 0).max(axis=1), 0.0))
        ok, fig = SE.rule({"case": got}, pseudo, max_undecided=None)
        print(name, fig)
        assert ok, "%s: %s" % (name, fig)
        if kind == "zero":
            assert not a.any(), name + ": an empty canvas must come back as zeros"
        if kind == "last":                                                 # one term per sum: all 32 responses are bank[k][8][8] exactly, the first wins
            assert int(s.sum()) == 1 and got["idx"][s][0] == 0 and (not extras or got["conf"][s][0] == np.float32(bank[0, 8, 8]))
    nm = "stroke orient %s %s%s%s" % ((n, h, w), kind, " idx+conf" if extras else "", " asymmetric bank" if asymmetric else "")
    return dict(fn=fn, tensors=[torch.from_numpy(mask), torch.from_numpy(np.ascontiguousarray(bank))], checks=[(nm, check)], geometry=(n, h, w))


def _case(id_, covers, build):
    CASES.append(Case(id_, covers, build))


ORIENT = ("mg_stroke_orient",)
for _h, _w in [(1, 1), (5, 40), (17, 17), (33, 47)] + TILE_CASES:
    _case("stroke_orient-2x%dx%d-extras" % (_h, _w), ORIENT, lambda h=_h, w=_w: _orient_spec(2, h, w, True))
for _h, _w in ((1, 1), (SE.TILE_H + 1, SE.TILE_W + 1), (33, 47)):
    _case("stroke_orient-2x%dx%d-rgbonly" % (_h, _w), ORIENT, lambda h=_h, w=_w: _orient_spec(2, h, w, False))
_case("stroke_orient-2x33x47-zero", ORIENT, lambda: _orient_spec(2, 33, 47, True, kind="zero"))
_case("stroke_orient-2x33x47-zero-rgbonly", ORIENT, lambda: _orient_spec(2, 33, 47, False, kind="zero"))
_case("stroke_orient-2x33x47-last", ORIENT, lambda: _orient_spec(2, 33, 47, True, kind="last"))
_case("stroke_orient-2x33x47-asymmetric", ORIENT, lambda: _orient_spec(2, 33, 47, True, asymmetric=True))


def _glue_spec(n, h, w, size, dtype, strokes):
    from michigan_amd import ops
    from test_stroke import _glue_tensors
    t = _glue_tensors(n, h, w, 300 + h)
    net_out = torch.rand(n, 3, size or h, size or w, generator=torch.Generator().manual_seed(12))
    names = ["orient_rgb", "noise", "hole", "stroke", "stroke_mask", "mask"]

    def fn(ctx, orient_rgb, noise, hole, stroke, stroke_mask, mask, net_out):
        st, sm = (stroke, stroke_mask) if strokes else (None, None)
        inp = ops.stroke_compose(orient_rgb, noise, hole, st, sm, size=size, dtype=dtype)
        out, o2 = ops.inpaint_finish(net_out, hole, orient_rgb, mask)
        again = (ops.stroke_compose(orient_rgb, noise, hole, st, sm, size=size, dtype=dtype),) + ops.inpaint_finish(net_out, hole, orient_rgb, mask)
        assert all(torch.equal(a, b) for a, b in zip((inp, out, o2), again)), "two runs are not bit-identical"
        return inp, out, o2
    nm = "glue %s -> %s %s %s" % ((n, h, w), size, str(dtype).replace("torch.", ""), "strokes" if strokes else "no strokes")
    return dict(fn=fn, tensors=[t[k] for k in names] + [net_out], checks=[(nm + " inp", "equal"), (nm + " out_rgb", "equal"), (nm + " orient2", "equal")],
                geometry=(n, h, w))


GLUE = ("mg_stroke_compose", "mg_inpaint_finish")
for _geom in ((2, 32, 32, 256), (2, 33, 47, None)):
    for _dt in (torch.float32, torch.bfloat16):
        for _st in (True, False):
            _case("glue-%dx%dx%d-%s-%s-%s" % (_geom[:3] + ("to%d" % _geom[3] if _geom[3] else "identity", "bf16" if _dt == torch.bfloat16 else "f32", "strokes" if _st else "nostrokes")),
                  GLUE, lambda g=_geom, dt=_dt, st=_st: _glue_spec(g[0], g[1], g[2], g[3], dt, st))


def test_the_cases_sit_on_the_kernels_edges():
    """The mirror is the tile the kernel is compiled with (the header's defines), and the ids' geometry is what the cases build."""
    d = PU.header_defines("michigan_hip/editing/stroke_orient.h")
    assert (d["MG_STROKE_TILE_H"], d["MG_STROKE_TILE_W"], d["MG_STROKE_RADIUS"]) == (SE.TILE_H, SE.TILE_W, K.STROKE_RADIUS)
    tiles = lambda h, w: (SE.kernel_geometry(2, h, w)["tiles_y"], SE.kernel_geometry(2, h, w)["tiles_x"])
    assert [tiles(h, w) for h, w in TILE_CASES] == [(1, 2), (1, 2), (2, 2), (2, 1), (2, 1), (2, 2)]
    assert tiles(1, 1) == (1, 1) and tiles(5, 40) == (1, 3) and tiles(33, 47) == (3, 3)
    for c in CASES:
        n, h, w = c.build()["geometry"]
        assert c.id.split("-")[1] == "%dx%dx%d" % (n, h, w)


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_guarded(monkeypatch, c):
    import guard_alloc as GA
    counted = []
    orig = GA.Guard.check

    def check(self):                                                # _run checks inside the guard: read the call counts there
        counted.append({ep: self.backend.count(ep) for ep in c.covers})
        return orig(self)
    monkeypatch.setattr(GA.Guard, "check", check)
    assert GB._run(c.build(), c.covers) >= 4                        # the inputs and at least two outputs under guard
    assert counted == [{ep: 2 for ep in c.covers}], counted         # the run and its repetition, one launch each


def _on_device(fn):
    """fn(device) on the HIP backend (or, with MG_TEST_DRYRUN=1, on the emulator: plumbing check without a GPU)"""
    from michigan_amd import _cabi
    prev = _cabi.set_backend(EmulatorBackend() if GB.DRY else None)
    try:
        if not GB.DRY:
            assert _cabi.backend().name == "hip"
        return fn("cpu" if GB.DRY else "cuda")
    finally:
        _cabi.set_backend(prev)


def test_stroke_to_orient_end_to_end():
    from michigan_amd import inputs, ops
    fx = _fixture()

    def run(dev):
        got = {}
        for geo, rec in fx["geometries"].items():
            m = torch.from_numpy(rec["mask"]).to(dev)
            rgb, idx, conf = ops.stroke_orient(m, want_idx=True, want_conf=True)
            assert torch.equal(inputs.stroke_to_orient(m.float()), rgb)
            got[geo] = dict(rgb=rgb.cpu().numpy(), idx=idx.cpu().numpy(), conf=conf.cpu().numpy())
        return got
    got = _on_device(run)
    ok, fig = SE.rule(got, fx)
    agree = np.mean(np.concatenate([(got[g]["rgb"] == rec["rgb"]).all(axis=-1)[rec["mask"] != 0] for g, rec in fx["geometries"].items()]))
    print(fig, "| stroke pixels whose bytes are the reference's fp32 picture's: %.5f" % agree)
    assert ok, fig


def _glue_fixture():
    import os
    z = np.load(os.path.join(PU.GOLDEN, "stroke_glue.npz"))
    return {k: z[k] for k in z.files}


def _err(name, got, want):
    e = (got.float().cpu() - torch.from_numpy(want)).abs()
    print("%s: mean |err| %.5f, median %.5f, max %.4f" % (name, e.mean().item(), e.median().item(), e.max().item()))
    return e


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_sinpaint_module_hip_matches_golden(dt):
    from test_stroke import _cfg, _net
    cfg, gold = _cfg(), _glue_fixture()
    x = torch.rand(cfg["n"], 5, cfg["size"], cfg["size"], generator=torch.Generator().manual_seed(cfg["seed_x"]))
    out = _on_device(lambda dev: _net("SInpaintGenerator", dev, torch.float32 if dt == "f32" else torch.bfloat16)(x.to(dev)).cpu())
    e = _err("stroke in-painting net %s vs the reference" % dt, out, gold["out"])
    assert torch.isfinite(out).all()
    if dt == "f32":
        assert e.max().item() < 1e-3, e.max().item()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("branch", ["equal", "less"])
def test_inpainting_stroke_orient_hip_matches_golden(branch, dt):
    """Pix2PixModel.inpainting_stroke_orient at crop 32: both nets run at their real 256 x 256 working size"""
    from test_stroke import glue_shim, run_glue
    gold = _glue_fixture()
    rgb, o2 = _on_device(lambda dev: run_glue(glue_shim(dev, torch.float32 if dt == "f32" else torch.bfloat16), branch, dev))
    e_rgb = _err("glue %s %s rgb" % (branch, dt), rgb, gold["glue_%s.out_rgb" % branch])
    e_o2 = _err("glue %s %s orient" % (branch, dt), o2, gold["glue_%s.orient" % branch])
    assert torch.isfinite(rgb).all() and torch.isfinite(o2).all()
    if dt == "f32":
        assert e_rgb.max().item() < 1e-3 and e_o2.max().item() < 2e-3, (e_rgb.max().item(), e_o2.max().item())
