"""-m gpu: the editing extension group on the kernels of mg_mask_edit.hip, and EditSession.edit() on the device.

Every comparison is torch.equal against the numpy contracts of tests/mask_edit_fixtures.py: all outputs are bytes, there is nothing to
round.  Each kernel case runs inside the guard bands of tests/guard_alloc.py (inputs placed, outputs allocated by the operator layer
under the guard), every guard byte is checked, and a second run must be bit-identical.

  morph   2 x 37 x 53 (no multiple of the 16 x 16 tile, smaller than the 50 x 50 element): the ten elements of
          mask_edit_fixtures.elements() -- 1 x 1, the cross, the 5 / 20 / 50 ellipses, the 25 x 25 rectangle, the 7 x 4 "L" with the
          anchor in its first and in its last tap, the two-runs-per-row ring, the full 64 x 64 -- both operations, on random grey
          levels and on single impulses in the four corners and at the centre (two planes a launch; the last plane is empty, which is
          the dilation's all-zero early exit); once at 1 x 512 x 512 with the 50 x 50 ellipse.
  brush   2 x 40 x 56: the segment cases of mask_edit_fixtures.brush_cases() and 700 random segments on 2 x 64 x 64 (three chunks).
  refusals, on the device build of the library, before any launch.
  EditSession.edit() at the small-width configuration of the emulator tests, against the step assembled by hand with masks from the
  numpy contracts, for the stroke route and the reference-orientation route.
With MG_TEST_DRYRUN=1 the same cases run on the CPU against `EditEmulator` (a plumbing check without a GPU)."""
import numpy as np
import pytest
import torch

import guard_alloc as GA
import mask_edit_fixtures as MF
import test_gpu_guard_bands as GB

pytestmark = pytest.mark.gpu

DEV = "cpu" if GB.DRY else "cuda"


@pytest.fixture
def backend():
    """libmichigan_hip.so (or, dry, the emulator with the group added)"""
    from michigan_amd import _cabi
    prev = _cabi.set_backend(MF.EditEmulator() if GB.DRY else None)
    be = _cabi.backend()
    assert be.name == ("emulator" if GB.DRY else "hip")
    yield be
    _cabi.set_backend(prev)


class _Counting:
    """the active backend behind a count of the group's calls (guard_alloc's CountingBackend counts the main table's prefix only)"""

    def __init__(self, inner):
        self.__dict__.update(inner=inner, seen=[], name=inner.name)

    def __getattr__(self, fn):
        target = getattr(self.inner, fn)
        if not fn.startswith("mge_"):
            return target

        def call(*a):
            self.seen.append(fn)
            return target(*a)
        return call


def _guarded(fn, tensors, entry, calls=2):
    """fn(*placed tensors) -> tensors, twice, under the guard; returns the first run's results on the host"""
    from michigan_amd import _cabi
    with GA.guard(count_backend=False) as g:
        counting = _Counting(_cabi.backend())
        prev = _cabi.set_backend(counting)
        try:
            res = fn(*[g.place(t, DEV) for t in tensors])
            again = fn(*[g.place(t, DEV) for t in tensors])
            assert g.check() >= 2 * len(tensors)
        finally:
            _cabi.set_backend(prev)
        assert counting.seen == [entry] * calls, counting.seen
        assert all(torch.equal(a, b) for a, b in zip(res, again)), "two runs are not bit-identical"
        return [r.to("cpu", copy=True) for r in res]


ELEMENTS = list(MF.elements())


@pytest.mark.parametrize("op", [MF.DILATE, MF.ERODE], ids=["dilate", "erode"])
@pytest.mark.parametrize("name", ELEMENTS)
def test_morph_guarded(backend, name, op):
    from michigan_amd import ops
    elem, (ay, ax) = MF.elements()[name]
    inp = MF.morph_inputs(op)
    planes = [inp["grey"]] + [inp["impulses"][k:k + 2] for k in (0, 2, 4)]
    for src in planes:
        assert src.shape == (MF.MORPH_N, MF.MORPH_H, MF.MORPH_W)
        (got,) = _guarded(lambda s, e: (ops.morph_u8(s, e, (ax, ay), op),), [torch.from_numpy(src), torch.from_numpy(elem)], "mge_morph_u8")
        assert got.dtype == torch.uint8 and torch.equal(got, torch.from_numpy(MF.morph_contract(src, elem, (ay, ax), op))), (name, op)


def test_morph_full_size(backend):
    """1 x 512 x 512, the demo's own dilation (inputs.stroke_hole) of a drawn stroke mask and of a grey map; and the erosion"""
    from michigan_amd import inputs
    import stroke_fixtures as SE
    e = inputs.ellipse_element(50)
    stroke = SE.polyline_mask(1, 512, 512, 512)
    grey = MF.grey_planes(1, 512, 512, 9)
    for src in (stroke, grey):
        (got,) = _guarded(lambda s: (inputs.stroke_hole(s),), [torch.from_numpy(src)], "mge_morph_u8")
        assert torch.equal(got, torch.from_numpy(MF.morph_contract(src, e, (25, 25), MF.DILATE)))
    (got,) = _guarded(lambda s: (inputs.erode_u8(s, e),), [torch.from_numpy(grey)], "mge_morph_u8")
    assert torch.equal(got, torch.from_numpy(MF.morph_contract(grey, e, (25, 25), MF.ERODE)))


BRUSH = MF.brush_cases()


@pytest.mark.parametrize("name", list(BRUSH))
def test_brush_guarded(backend, name):
    from michigan_amd import ops
    canvas, segs = BRUSH[name]
    assert canvas.shape == ((2, 64, 64) if name == "random700" else (MF.BRUSH_N, MF.BRUSH_H, MF.BRUSH_W))
    if name == "random700":
        assert len(segs) > 2 * MF.header_defines()["MGE_BRUSH_CHUNK"]

    # the canvas is painted in place: paint the PLACED tensor itself, so the guards around it are the ones that are checked
    if len(segs):
        (got,) = _guarded(lambda c, s: (ops.brush_u8(c, s),), [torch.from_numpy(canvas), torch.from_numpy(segs.astype(np.int32))], "mge_brush_u8")
    else:                                                               # S = 0: an empty list has no bytes to put between guards
        none = torch.empty((0, 8), dtype=torch.int32, device=DEV)
        (got,) = _guarded(lambda c: (ops.brush_u8(c, none),), [torch.from_numpy(canvas)], "mge_brush_u8")
    want = MF.brush_contract(canvas, segs)
    assert torch.equal(got, torch.from_numpy(want)), name
    if name == "empty":
        assert torch.equal(got, torch.from_numpy(canvas))
    else:
        assert (want != canvas).any(), name


def test_brush_through_the_uploader(backend):
    """inputs.brush_u8: the host list, one pinned upload, the [N,1,H,W] view painted in place"""
    from michigan_amd import inputs
    canvas, segs = BRUSH["order"]
    c = torch.from_numpy(canvas).to(DEV).unsqueeze(1).contiguous()
    assert inputs.brush_u8(c, segs.tolist()) is c
    assert torch.equal(c[:, 0].cpu(), torch.from_numpy(MF.brush_contract(canvas, segs)))


def test_refusals_before_any_launch(backend):
    from michigan_amd import inputs, ops
    counting = _Counting(backend)
    from michigan_amd import _cabi
    prev = _cabi.set_backend(counting)
    try:
        canvas = torch.zeros(2, 40, 56, dtype=torch.uint8, device=DEV)
        good = [0, 1, 1, 20, 20, 3, 2, 0]
        for bad in ([0, 1, 1, 20, 20, 0, 2, 0], [0, 1, 1, 20, 20, 256, 2, 0], [0, 8192, 1, 20, 20, 3, 2, 0], [0, 1, 1, 20, -8192, 3, 2, 0], [2, 1, 1, 20, 20, 3, 2, 0]):
            with pytest.raises(ValueError, match="outside the accepted ranges"):
                inputs.brush_u8(canvas, [good, bad])
        src = torch.zeros(2, 37, 53, dtype=torch.uint8, device=DEV)
        with pytest.raises(ValueError, match="at most 64"):
            inputs.dilate_u8(src, np.ones((65, 3), np.uint8))
        with pytest.raises(ValueError, match="anchor"):
            inputs.dilate_u8(src, np.ones((3, 3), np.uint8), anchor=(3, 1))
        with pytest.raises(ValueError, match="anchor"):
            inputs.erode_u8(src, np.ones((3, 3), np.uint8), anchor=(1, -1))
        assert counting.seen == []                                      # refused by the wrappers: the library was not called
        # the library's own checks, behind the wrappers
        e = torch.ones(65, 3, dtype=torch.uint8, device=DEV)
        dst = torch.full_like(src, 7)
        p = MF.pointer
        st = ops._stream(src)
        for args, msg in (((p(src), p(e), 65, 3, 1, 1, 0, p(dst), 2, 37, 53, st), "element"),
                          ((p(src), p(e), 3, 3, 3, 1, 0, p(dst), 2, 37, 53, st), "anchor"),
                          ((p(src), p(e), 3, 3, 1, 3, 0, p(dst), 2, 37, 53, st), "anchor"),
                          ((p(src), p(e), 3, 3, 1, 1, 0, p(src), 2, 37, 53, st), "overlap")):
            with pytest.raises(RuntimeError, match="mge_morph_u8.*" + msg):
                counting.mge_morph_u8(*args)
        for n, h, w in ((0, 40, 56), (2, 8193, 56)):
            with pytest.raises(RuntimeError, match="mge_brush_u8.*bad geometry"):
                counting.mge_brush_u8(p(canvas), p(src), 1, n, h, w, st)
        if DEV == "cuda":
            torch.cuda.synchronize()
        assert not canvas.any() and not src.any() and bool((dst == 7).all())          # nothing ran
    finally:
        _cabi.set_backend(prev)


@pytest.mark.parametrize("use_ref_orient", [False, True], ids=["stroke", "reforient"])
def test_edit_session_on_the_device(backend, use_ref_orient):
    """edit() against the by-hand assembly of tests/test_mask_edit.py, whose masks come from the numpy contracts and are uploaded"""
    import test_mask_edit as TM
    from michigan_amd.model import Pix2PixModel
    opt = TM._options(gpu_ids=[] if GB.DRY else [0])
    torch.manual_seed(0)
    model = Pix2PixModel(opt).to(DEV).eval()
    f = TM.session_files()
    points, sizes = TM.pen_record(erase=True)
    s = TM.open_session(model, opt, f, recon=True, device=DEV)
    result, picture = s.edit(points, sizes, False, use_ref_orient)
    want, want_picture, maps = TM.by_hand(model, opt, f, points, sizes, False, use_ref_orient, True, device=DEV)
    assert result.device.type == DEV and result.dtype == torch.uint8 and tuple(result.shape) == (TM.SIZE, TM.SIZE, 3)
    assert s.used_recon and torch.equal(s.handed[0]["image_tag"].cpu(), f["recon"])
    assert torch.equal(s.mask_m.cpu(), torch.from_numpy(maps["mask_m"]))
    if not use_ref_orient:
        assert torch.equal(s.handed[0]["mask_stroke"].cpu(), torch.from_numpy(maps["stroke"]))
        assert torch.equal(s.handed[0]["mask_hole"].cpu(), torch.from_numpy(maps["hole"]))
    assert torch.equal(result, want) and torch.equal(picture, want_picture)
    assert int(result.max()) > int(result.min())
