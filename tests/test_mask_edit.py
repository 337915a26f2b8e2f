"""CPU: the editing extension group (include/michigan_hip/editing/mask_edit.h) and the headless session on top of it.

1. The contracts of tests/mask_edit_fixtures.py: the structuring elements, the header outside the ledger's regex, the dilation
   contract against scipy.ndimage where scipy is installed, the impulse response, and the case tables against every one-line mutant.
2. The operator layer on `EditEmulator`: shapes, the element cache, what is refused before any call.
3. `michigan_amd.demo.EditSession.edit()` against the same step assembled by hand (contract brush and dilation on the host,
   demo_batch, model(..., 'demo_inference'), the same seeds), torch.equal, for the four mask / orientation choices with and without
   a reconstruction; the launch census; orient_edit; the replay command on a directory written into tmp_path.
The device side is tests/test_gpu_mask_edit.py."""
import json
import os
import random
import re

import numpy as np
import pytest
import torch

import mask_edit_fixtures as MF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def emulator():
    from michigan_amd import _cabi
    em = MF.EditEmulator()
    prev = _cabi.set_backend(em)
    yield em
    _cabi.set_backend(prev)


# ---- 1. contracts ------------------------------------------------------------------------------------------------------------------------
def test_ellipse_elements():
    from michigan_amd import inputs
    assert inputs.ellipse_element(3).tolist() == [[0, 1, 0], [1, 1, 1], [0, 1, 0]]
    assert inputs.ellipse_element(5).tolist() == [[0, 0, 1, 0, 0], [1] * 5, [1] * 5, [1] * 5, [0, 0, 1, 0, 0]]
    assert inputs.ellipse_element(1).tolist() == [[1]]
    for k in (20, 50):
        e = inputs.ellipse_element(k)
        assert e.shape == (k, k) and e.dtype == np.uint8 and set(np.unique(e)) == {0, 1}
        assert e[0].tolist() == [0] * (k // 2) + [1] + [0] * (k - k // 2 - 1)           # row 0: the single pixel at column k / 2
        assert e[k // 2].all()                                                          # row k / 2 is full
    e = inputs.ellipse_element(7, 4)
    assert e.shape == (4, 7) and e[2].all()
    assert inputs.rect_element(25).shape == (25, 25) and inputs.rect_element(25).all() and inputs.rect_element((3, 2)).shape == (2, 3)


def test_ellipse_rows_do_not_hang_on_the_form_of_the_quotient():
    """OpenCV multiplies by a precomputed 1 / r^2 where the docstring divides by r^2: the two agree for every element the kernel takes"""
    from michigan_amd import inputs
    for kh in range(1, 65):
        for kw in range(1, 65):
            r, c = kh // 2, kw // 2
            inv = 1.0 / (r * r) if r else 0.0
            e = inputs.ellipse_element(kw, kh)
            for i in range(kh):
                dy = i - r
                dx = int(round(c * np.sqrt((r * r - dy * dy) * inv))) if abs(dy) <= r else -1
                want = np.zeros(kw, np.uint8)
                if abs(dy) <= r:
                    want[max(c - dx, 0):min(c + dx + 1, kw)] = 1
                assert np.array_equal(e[i], want), (kh, kw, i)


def test_the_header_is_outside_the_ledger():
    """the regex of tests/test_cabi_host.py finds no entry point in the new header; the group is bound in a table of its own"""
    from michigan_amd import _cabi, build
    src = open(os.path.join(ROOT, "include", "michigan_hip", "editing", "mask_edit.h")).read()
    assert re.findall(r"\bmg_[a-z0-9_]+\(", src) == []
    stripped = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.findall(r"\b(mg_[a-z0-9_]+)\s*\(", stripped) == []
    assert set(re.findall(r"\b(mge_[a-z0-9_]+)\s*\(", stripped)) == set(_cabi._EDIT_PROTOS) == {"mge_brush_u8", "mge_morph_u8"}
    assert not set(_cabi._EDIT_PROTOS) & set(_cabi._PROTOS) and not set(_cabi._EDIT_PROTOS) & set(_cabi.EXPORTED_SYMBOLS)
    assert "mg_mask_edit.hip" in build.SOURCES
    d = MF.header_defines()
    assert (d["MGE_BRUSH_MAX_THICKNESS"], d["MGE_BRUSH_MAX_COORD"], d["MGE_MORPH_MAX_K"]) == (MF.MAX_THICKNESS, MF.MAX_COORD, MF.MAX_K)
    assert (d["MGE_MORPH_DILATE"], d["MGE_MORPH_ERODE"]) == (MF.DILATE, MF.ERODE)


def test_the_library_exports_the_group_and_checks_its_arguments():
    """validated before the device is touched, so this runs without one: status, message, and nothing launched"""
    from michigan_amd import _cabi, build, ops
    be = _cabi.HipBackend(build.build(verbose=False))
    buf = torch.zeros(4096, dtype=torch.uint8)
    p, q = MF.pointer(buf), MF.pointer(buf[2048:])
    assert be.mge_brush_u8(p, None, 0, 1, 8, 8, None) == 0                                  # no segments: success without a launch
    with pytest.raises(RuntimeError, match=r"mge_brush_u8 failed \(code 1\): mge_brush_u8: null canvas"):
        be.mge_brush_u8(None, p, 1, 1, 8, 8, None)
    with pytest.raises(RuntimeError, match="null segment list"):
        be.mge_brush_u8(p, None, 1, 1, 8, 8, None)
    for n, h, w in ((0, 8, 8), (1, 0, 8), (1, 8, 8193), (1, 8193, 8)):
        with pytest.raises(RuntimeError, match="bad geometry"):
            be.mge_brush_u8(p, q, 1, n, h, w, None)
    with pytest.raises(RuntimeError, match="bad segment count"):
        be.mge_brush_u8(p, q, -1, 1, 8, 8, None)
    morph = lambda **kw: be.mge_morph_u8(*[dict(dict(src=p, elem=p, kh=3, kw=3, ay=1, ax=1, op=0, dst=q, n=1, h=8, w=8, stream=None), **kw)[k]
                                           for k in ("src", "elem", "kh", "kw", "ay", "ax", "op", "dst", "n", "h", "w", "stream")])
    for kw, msg in ((dict(kh=65), "bad element"), (dict(kw=65), "bad element"), (dict(kh=0), "bad element"), (dict(ay=3), "anchor"), (dict(ax=-1), "anchor"),
                    (dict(op=2), "bad op"), (dict(dst=p), "overlap"), (dict(dst=MF.pointer(buf[32:])), "overlap"), (dict(src=None), "null pointer"),
                    (dict(n=0), "bad geometry")):
        with pytest.raises(RuntimeError, match="mge_morph_u8: .*" + msg):
            morph(**kw)
    with pytest.raises(AttributeError):
        be.mge_not_an_entry_point
    assert (ops.BRUSH_MAX_THICKNESS, ops.BRUSH_MAX_COORD, ops.MORPH_MAX_K) == (MF.MAX_THICKNESS, MF.MAX_COORD, MF.MAX_K)


def test_dilation_contract_is_scipys_with_the_reflected_footprint():
    ndi = pytest.importorskip("scipy.ndimage")
    for op, fn, cval in ((MF.DILATE, ndi.grey_dilation, 0), (MF.ERODE, ndi.grey_erosion, 255)):
        for name, (elem, (ay, ax)) in MF.elements().items():
            kh, kw = elem.shape
            for kind, src in MF.morph_inputs(op).items():
                want = MF.morph_contract(src, elem, (ay, ax), op)
                # scipy's filters read in[y + i - (k // 2 + origin)].  grey_erosion takes the footprint and the origin as given;
                # grey_dilation reflects the footprint, negates the origin and, for an even size, moves it one further
                if op == MF.ERODE:
                    fp, origin = elem, (ay - kh // 2, ax - kw // 2)
                else:
                    fp = elem[::-1, ::-1]
                    origin = tuple(-(a - k // 2) - (1 if k % 2 == 0 else 0) for a, k in ((ay, kh), (ax, kw)))
                got = np.stack([fn(p, footprint=fp.astype(bool), mode="constant", cval=cval, origin=origin) for p in src])
                assert np.array_equal(got, want), (name, op, kind)


def test_the_impulse_response_is_the_reflected_element():
    h, w = MF.MORPH_H, MF.MORPH_W
    for name, (elem, (ay, ax)) in MF.elements().items():
        kh, kw = elem.shape
        got = MF.morph_contract(MF.impulse_planes(h, w), elem, (ay, ax), MF.DILATE)
        for k, (py, px) in enumerate(((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w // 2))):
            want = np.zeros((h, w), np.uint8)
            for i, j in zip(*np.nonzero(elem)):                         # tap (i, j) carries the impulse to p - (i, j) + anchor
                y, x = py - i + ay, px - j + ax
                if 0 <= y < h and 0 <= x < w:
                    want[y, x] = 255
            assert np.array_equal(got[k], want), (name, k)
        assert not got[5].any()


def test_the_morph_cases_reject_every_mutant():
    killed = {m: [] for m in MF.MORPH_MUTANTS}
    for op in (MF.DILATE, MF.ERODE):
        for name, (elem, anchor) in MF.elements().items():
            for kind, src in MF.morph_inputs(op).items():
                want = MF.morph_contract(src, elem, anchor, op)
                for m in MF.MORPH_MUTANTS:
                    if not np.array_equal(MF.morph_contract(src, elem, anchor, op, mutant=m), want):
                        killed[m].append((name, op, kind))
    for m, by in killed.items():
        print("%-12s rejected by %d cases, e.g. %s" % (m, len(by), by[:2]))
    assert all(killed.values()), [m for m, by in killed.items() if not by]
    assert all(op == MF.ERODE for _, op, _ in killed["zero_border"])
    assert {n for n, _, _ in killed["first_run"]} == {"ring9"}           # the one element with two runs in a row


def test_the_brush_cases_reject_every_mutant():
    killed = {m: [] for m in MF.BRUSH_MUTANTS}
    for name, (canvas, segs) in MF.brush_cases().items():
        want = MF.brush_contract(canvas, segs)
        if name == "empty":
            assert np.array_equal(want, canvas)
        for m in MF.BRUSH_MUTANTS:
            if not np.array_equal(MF.brush_contract(canvas, segs, mutant=m), want):
                killed[m].append(name)
    for m, by in killed.items():
        print("%-14s rejected by %s" % (m, by))
    assert all(killed.values()), [m for m, by in killed.items() if not by]


def test_brush_contract_by_hand():
    """4 d^2 <= t^2, counted by hand: thickness 1 is the pixel itself, 2 the plus, 3 the 3 x 3 block, 4 the 13-pixel disc"""
    c = np.zeros((1, 9, 9), np.uint8)
    dot = lambda t: MF.brush_contract(c, [[0, 4, 4, 4, 4, t, 1, 0]])[0]
    assert dot(1).sum() == 1 and dot(1)[4, 4] == 1
    assert dot(2).sum() == 5 and dot(2)[3, 4] == dot(2)[4, 3] == 1 and dot(2)[3, 3] == 0          # d^2 <= 1
    assert dot(3).sum() == 9                                                                    # d^2 <= 2.25: the 3 x 3 block
    assert dot(4).sum() == 13                                                                   # d^2 <= 4
    line = MF.brush_contract(c, [[0, 2, 4, 6, 4, 1, 1, 0]])[0]
    assert line.sum() == 5 and line[4, 2:7].all()
    line3 = MF.brush_contract(c, [[0, 2, 4, 6, 4, 3, 1, 0]])[0]
    assert line3[3:6, 1:8].all() and line3.sum() == 21                                          # the body and a cap column at each end (d^2 = 2 <= 2.25)


# ---- 2. the operator layer ---------------------------------------------------------------------------------------------------------------
def test_wrappers_shapes_cache_and_refusals(emulator):
    from michigan_amd import inputs, ops
    m = torch.from_numpy(MF.grey_planes(2, 11, 13, 3))
    e = inputs.ellipse_element(5)
    want = torch.from_numpy(MF.morph_contract(m.numpy(), e, (2, 2), MF.DILATE))
    assert torch.equal(inputs.dilate_u8(m, e), want)
    assert torch.equal(inputs.dilate_u8(m[0], e), want[0]) and inputs.dilate_u8(m[0], e).shape == (11, 13)
    assert torch.equal(inputs.dilate_u8(m.unsqueeze(1), e), want.unsqueeze(1))
    assert torch.equal(inputs.erode_u8(m, e, anchor=(0, 4)), torch.from_numpy(MF.morph_contract(m.numpy(), e, (4, 0), MF.ERODE)))       # (x, y), as cv2
    assert torch.equal(inputs.stroke_hole(m, 20), torch.from_numpy(MF.morph_contract(m.numpy(), inputs.ellipse_element(20), (10, 10), MF.DILATE)))
    assert torch.equal(inputs.dilate_u8(m, torch.from_numpy(e)), want)
    keys = [k for k in inputs._ELEMENTS if k[1] == (5, 5)]
    assert len(keys) == 1                                                               # one upload for the four calls with this element
    canvas = torch.zeros(2, 1, 11, 13, dtype=torch.uint8)
    segs = [[1, 2, 2, 9, 8, 3, 2, 0], [0, 0, 0, 12, 0, 1, 1, 0]]
    assert inputs.brush_u8(canvas, segs) is canvas
    assert torch.equal(canvas[:, 0], torch.from_numpy(MF.brush_contract(np.zeros((2, 11, 13), np.uint8), segs)))
    assert torch.equal(inputs.brush_u8(canvas.clone(), [s[:7] for s in segs]), canvas)                                   # rows of seven
    assert torch.equal(inputs.brush_u8(canvas.clone(), np.asarray(segs, np.int32)), canvas)
    before = list(emulator.calls)
    assert torch.equal(inputs.brush_u8(canvas.clone(), []), canvas)
    assert emulator.calls[len(before):] == [("mge_brush_u8", None)]                      # the call is made; the entry point launches nothing
    before = list(emulator.calls)
    for bad in ([0, 1, 1, 2, 2, 0, 1, 0], [0, 1, 1, 2, 2, 256, 1, 0], [0, 8192, 1, 2, 2, 3, 1, 0], [0, 1, 1, 2, -8192, 3, 1, 0], [2, 1, 1, 2, 2, 3, 1, 0],
                [-1, 1, 1, 2, 2, 3, 1, 0], [0, 1, 1, 2, 2, 3, 256, 0]):
        with pytest.raises(ValueError, match="outside the accepted ranges"):
            inputs.brush_u8(canvas, [segs[0], bad])
    with pytest.raises(ValueError):
        inputs.brush_u8(canvas.float(), segs)
    with pytest.raises(ValueError, match="contiguous"):
        inputs.brush_u8(canvas[:, :, :, ::2], segs)
    with pytest.raises(ValueError, match="at most 64"):
        inputs.dilate_u8(m, np.ones((65, 3), np.uint8))
    with pytest.raises(ValueError, match="anchor"):
        inputs.dilate_u8(m, e, anchor=(5, 0))
    with pytest.raises(ValueError):
        inputs.dilate_u8(m.float(), e)
    with pytest.raises(ValueError):
        inputs.dilate_u8(m, e.astype(np.float32))
    with pytest.raises(ValueError):
        ops.morph_u8(m, torch.from_numpy(e), (2, 2), 2)
    assert emulator.calls == before                                                      # refused before any call
    with pytest.raises(RuntimeError, match="overlap"):                                   # the entry point's own check, behind the wrappers
        emulator.mge_morph_u8(MF.pointer(m), MF.pointer(torch.from_numpy(e)), 5, 5, 2, 2, 0, MF.pointer(m), 2, 11, 13)


def test_the_element_cache_is_bounded(emulator):
    from michigan_amd import inputs
    m = torch.from_numpy(MF.grey_planes(1, 9, 9, 1))
    first = inputs.rect_element((1, 2))
    for k in range(2, inputs._ELEMENTS_MAX + 6):
        inputs.dilate_u8(m, inputs.rect_element((1, k)))
    assert len(inputs._ELEMENTS) <= inputs._ELEMENTS_MAX
    assert not [key for key in inputs._ELEMENTS if key[1] == first.shape]            # the oldest entries went
    assert torch.equal(inputs.dilate_u8(m, first), torch.from_numpy(MF.morph_contract(m.numpy(), first, (1, 0), MF.DILATE)))


# ---- 3. the session ----------------------------------------------------------------------------------------------------------------------
SIZE = 64


def _options(**over):
    from michigan_amd.model import default_options
    return default_options(**dict(dict(gpu_ids=[], isTrain=False, ngf=8, crop_size=SIZE, load_size=SIZE, compute_dtype="fp32", use_ig=True, use_stroke=True,
                                       inpaint_mode="ref", inpaint_orient=True, no_vgg_loss=True, no_flip=True), **over))


_MODEL = {}


def _model(**over):
    from michigan_amd.model import Pix2PixModel
    key = tuple(sorted(over.items()))
    if key not in _MODEL:
        torch.manual_seed(0)
        _MODEL[key] = Pix2PixModel(_options(**over)).eval()
    return _MODEL[key]


def session_files(size=SIZE, seed=5):
    """decoded files of a target and a reference: label discs, orientations under them, images, a reconstruction"""
    import dataset_fixtures as DF
    t = lambda a: torch.from_numpy(a)
    label, orient, image = DF.sample(seed, size)
    rlabel, _, rimage = DF.sample(seed + 1, size)
    recon = DF.sample(seed + 2, size)[2]
    return dict(image=t(image), label=t(label), orient=t(orient), recon=t(recon), ref_image=t(rimage), ref_label=t(rlabel))


def pen_record(erase, size=SIZE):
    """the UI's record: colour 0 (background) drawn across the hair disc when `erase`, colour 1 (hair) added at the rim, colour 2 two
    strokes inside the hair"""
    c = size // 2
    seg = lambda x0, y0, x1, y1: {"prev": (x0, y0), "curr": (x1, y1)}
    points = [[seg(c - 20, c - 6, c + 4, c - 4), seg(c + 4, c - 4, c + 20, c - 9)] if erase else [],
              [seg(c - 30, c + 12, c - 22, c + 20), seg(4, 4, 9, 5)],
              [seg(c - 8, c + 2, c + 2, c + 8), seg(c + 2, c + 8, c + 12, c + 6), seg(c - 3, c + 14, c + 6, c + 13)]]
    sizes = [[6, 6] if erase else [], [9, 3], [2, 2, 4]]
    return points, sizes


def by_hand(model, opt, f, points, sizes, use_ref_mask, use_ref_orient, recon, device="cpu", seed=1):
    """Ex.edit() assembled from the parent's pieces: the masks from the numpy contracts, then demo_batch and the model"""
    from michigan_amd import inputs
    from michigan_amd.demo import pen_segments
    from michigan_amd.inference import tensor2im
    mask = f["label"].numpy()[None]
    mask_m = MF.brush_contract(mask, pen_segments(points[0], sizes[0], 0) + pen_segments(points[1], sizes[1], 1))
    orient_new = MF.brush_contract(mask_m, pen_segments(points[2], sizes[2], 2))
    orient_new[orient_new == 1] = 0
    orient_new[orient_new == 2] = 1
    hole = MF.morph_contract(orient_new, inputs.ellipse_element(50), (25, 25), MF.DILATE)
    erased = 1 in np.unique(mask - mask_m)                                          # uint8 arithmetic, as the reference's
    tag = f["recon"] if (not use_ref_mask and recon and erased) else f["image"]
    label_tag = mask if use_ref_mask else mask_m
    strokes = {} if use_ref_orient else dict(mask_stroke=torch.from_numpy(orient_new).to(device), mask_hole=torch.from_numpy(hole).to(device))
    model.opt.inpaint_mode = "ref" if use_ref_orient else "stroke"
    data = inputs.demo_batch(opt, label_ref=f["ref_label"].to(device), label_tag=torch.from_numpy(label_tag).to(device), mask_orient=f["label"].to(device),
                             orient_ref=f["orient"].to(device), image_ref=f["ref_image"].to(device), image_tag=tag.to(device),
                             rng=random.Random(seed), generator=torch.Generator(device=device).manual_seed(seed), **strokes)
    generated, picture = model(data, "demo_inference")
    if opt.add_feat_zeros:
        o = int(opt.add_th / 2)
        generated = generated[:, :, o:o + opt.crop_size, o:o + opt.crop_size]
    return tensor2im(generated)[0], picture[0], dict(mask_m=mask_m[0], stroke=orient_new[0], hole=hole[0], erased=erased)


def open_session(model, opt, f, recon, device="cpu", seed=1):
    """the session, with a note of what each edit() hands to its loader (`s.handed`: the keyword arguments of demo_batch)"""
    from michigan_amd.demo import EditSession
    s = EditSession(model, opt, device, rng=random.Random(seed), generator=torch.Generator(device=device).manual_seed(seed))
    s.open_tag(f["image"], f["label"], f["orient"], f["recon"] if recon else None)
    s.open_ref(f["ref_image"], f["ref_label"])
    s.handed, own = [], s.pipe.demo_batch

    def demo_batch(**kw):
        s.handed.append(kw)
        return own(**kw)
    s.pipe.demo_batch = demo_batch
    return s


@pytest.mark.parametrize("recon", [True, False], ids=["recon", "norecon"])
@pytest.mark.parametrize("use_ref_orient", [True, False], ids=["reforient", "stroke"])
@pytest.mark.parametrize("use_ref_mask", [True, False], ids=["origmask", "editedmask"])
def test_edit_is_the_step_assembled_by_hand(emulator, use_ref_mask, use_ref_orient, recon):
    model, opt, f = _model(), _options(), session_files()
    points, sizes = pen_record(erase=True)
    s = open_session(model, opt, f, recon)
    before = len(emulator.calls)
    result, picture = s.edit(points, sizes, use_ref_mask, use_ref_orient)
    mine = [name for name, _ in emulator.calls[before:]]
    assert model.opt.inpaint_mode == ("ref" if use_ref_orient else "stroke")
    want, want_picture, maps = by_hand(model, opt, f, points, sizes, use_ref_mask, use_ref_orient, recon)
    assert maps["erased"] and maps["stroke"].sum() > 20 and maps["hole"].sum() > maps["stroke"].sum()
    assert result.dtype == torch.uint8 and tuple(result.shape) == (SIZE, SIZE, 3) and tuple(picture.shape) == (SIZE, SIZE, 3)
    assert torch.equal(result, want) and torch.equal(picture, want_picture)
    assert torch.equal(s.mask_m, torch.from_numpy(maps["mask_m"])) and torch.equal(s.mask, f["label"])
    assert s.used_recon == (recon and not use_ref_mask)                              # a hair pixel was erased: the reconstruction, when there is one
    # with seeded weights the target image moves the result by less than a grey level, so the choice is read where it is made
    assert len(s.handed) == 1 and torch.equal(s.handed[0]["image_tag"], f["recon"] if s.used_recon else f["image"])
    assert ("mask_stroke" in s.handed[0]) == ("mask_hole" in s.handed[0]) == (not use_ref_orient)
    if not use_ref_orient:
        assert torch.equal(s.handed[0]["mask_stroke"], torch.from_numpy(maps["stroke"])) and torch.equal(s.handed[0]["mask_hole"], torch.from_numpy(maps["hole"]))
    assert mine.count("mge_brush_u8") == 3 and mine.count("mge_morph_u8") == 1
    assert int(result.max()) > int(result.min())


def test_the_reconstruction_is_chosen_only_when_hair_was_erased(emulator):
    model, opt, f = _model(), _options(), session_files()
    points, sizes = pen_record(erase=False)                                          # hair added, none erased: mask - mask_m wraps to 255, never 1
    s = open_session(model, opt, f, recon=True)
    result, picture = s.edit(points, sizes, False, False)
    want, want_picture, maps = by_hand(model, opt, f, points, sizes, False, False, True)
    assert not maps["erased"] and (maps["mask_m"] != f["label"].numpy()).any()
    assert not s.used_recon and torch.equal(result, want) and torch.equal(picture, want_picture)
    assert torch.equal(s.handed[0]["image_tag"], f["image"]) and not torch.equal(f["image"], f["recon"])


def test_add_feat_zeros_window(emulator):
    over = dict(add_feat_zeros=True)                                                  # add_th 64: the padded canvas is 128, a size the generator takes
    model, opt, f = _model(**over), _options(**over), session_files()
    points, sizes = pen_record(erase=True)
    result, picture = open_session(model, opt, f, True).edit(points, sizes, False, False)
    want, want_picture, _ = by_hand(model, opt, f, points, sizes, False, False, True)
    assert tuple(result.shape) == (SIZE, SIZE, 3) and torch.equal(result, want) and torch.equal(picture, want_picture)


class Recording:
    """`EditEmulator` behind a log of EVERY entry point that is called, both prefixes, in order (the emulator's own `calls` notes a
    handful of entry points only, none of the loader's)"""
    name = "emulator"

    def __init__(self):
        self.inner, self.log = MF.EditEmulator(), []

    def __getattr__(self, key):
        fn = getattr(self.inner, key)
        if not key.startswith(("mg_", "mge_")):
            return fn

        def call(*a, **k):
            self.log.append(key)
            return fn(*a, **k)
        return call


# demo_batch with strokes on a pipeline whose tables exist, files stored at the load size (no bicubic resize): 15 calls
STROKE_ROW = (["mg_input_crop_u8"] * 2 + ["mg_orient_to_rgb_u8", "mg_input_crop_u8"] + ["mg_input_crop_u8"] + ["mg_stroke_orient"] + ["mg_input_crop_u8"] * 3
              + ["mg_noise_field_len"] * 2 + ["mg_noise_octaves"] + ["mg_input_crop_u8"] * 3)


def test_launch_census():
    """up to the model call, edit() is the stroke row of demo_batch -- 15 calls -- plus three brush calls and one dilation, in this
    order: brush, brush, (the read-back,) brush, dilation, then the row call for call"""
    from michigan_amd import _cabi
    assert len(STROKE_ROW) == 15
    rec = Recording()
    prev = _cabi.set_backend(rec)
    try:
        model, opt, f = _model(), _options(), session_files()
        points, sizes = pen_record(erase=True)
        s = open_session(model, opt, f, True)
        marks = []

        class Marked:                                                                # notes where the loader's share of the log ends
            opt = model.opt

            def __call__(self, data, mode):
                marks.append(len(rec.log))
                return model(data, mode)
        s.model = Marked()
        s.edit(points, sizes, False, False)                                          # the pipeline's tables exist from here on
        for use_ref_mask, use_ref_orient in ((False, False), (True, False)):
            del rec.log[:], marks[:]
            s.edit(points, sizes, use_ref_mask, use_ref_orient)
            assert len(marks) == 1 and len(rec.log) > marks[0]                       # the model ran, after everything counted here
            assert rec.log[:marks[0]] == ["mge_brush_u8"] * 3 + ["mge_morph_u8"] + STROKE_ROW, rec.log[:marks[0]]
            assert not [c for c in rec.log[marks[0]:] if c.startswith("mge_") or c in STROKE_ROW]
        del rec.log[:]
        m = torch.zeros(1, SIZE, SIZE, dtype=torch.uint8)
        s.pipe.demo_batch(label_ref=f["ref_label"], label_tag=f["label"], mask_orient=f["label"], orient_ref=f["orient"], image_ref=f["ref_image"],
                          image_tag=f["image"], mask_stroke=m, mask_hole=m)
        assert rec.log == STROKE_ROW, rec.log                                        # the row itself, from the parent's loader alone
        del rec.log[:], marks[:]
        s.edit(points, sizes, False, True)                                           # the reference orientation: the row without strokes
        plain = [c for c in STROKE_ROW if c != "mg_stroke_orient"]
        plain = plain[:5] + plain[8:]                                                # ... and without the three stroke crops
        assert rec.log[:marks[0]] == ["mge_brush_u8"] * 3 + ["mge_morph_u8"] + plain, rec.log[:marks[0]]
    finally:
        _cabi.set_backend(prev)


def test_orient_edit_mirrors_the_reference(emulator):
    from michigan_amd.demo import pen_segments
    model, opt, f = _model(), _options(), session_files()
    points, sizes = pen_record(erase=True)
    s = open_session(model, opt, f, False)
    got = s.orient_edit(points, sizes)
    m = MF.brush_contract(f["label"].numpy()[None], pen_segments(points[0], sizes[0], 0) + pen_segments(points[1], sizes[1], 1) + pen_segments(points[2], sizes[2], 2))
    m[m == 1] = 0
    m[m == 2] = 1
    from michigan_amd import inputs
    assert torch.equal(s.mask_m, torch.from_numpy(m[0]))                              # the reference relabels self.mask_m itself
    assert torch.equal(got, torch.from_numpy(MF.morph_contract(m, inputs.ellipse_element(20), (10, 10), MF.DILATE)[0]))
    with pytest.raises(RuntimeError, match="open_tag"):
        from michigan_amd.demo import EditSession
        EditSession(model, opt, "cpu").edit(points, sizes, False, False)


def test_refused_options_stay_refused(emulator):
    """the new dilation is not wired into expand_tag_mask, and a lone mask_stroke still raises"""
    from michigan_amd import inputs
    f = session_files()
    kw = dict(label_ref=f["ref_label"], label_tag=f["label"], mask_orient=f["label"], orient_ref=f["orient"], image_ref=f["ref_image"], image_tag=f["image"])
    with pytest.raises(NotImplementedError, match="expand_tag_mask"):
        inputs.demo_batch(_options(expand_tag_mask=True), **kw)
    with pytest.raises(ValueError, match="together"):
        inputs.demo_batch(_options(), mask_stroke=f["label"], **kw)
    assert "stroke_hole" in inputs.stroke_inputs.__doc__ and "stroke_hole" in inputs.DeviceInputPipeline.demo_batch.__doc__


def test_replay_command(emulator, tmp_path):
    """python -m michigan_amd.demo on a directory written here: the three files, and the result is the session's"""
    from PIL import Image
    import dataset_fixtures as DF
    from michigan_amd import demo
    from michigan_amd.model import Pix2PixModel
    from michigan_amd.synth import synth_state_dict
    root, ck, out = str(tmp_path / "demo"), str(tmp_path / "ck"), str(tmp_path / "out")
    f = session_files()
    for name, (image, label, orient) in (("t", (f["image"], f["label"], f["orient"])), ("r", (f["ref_image"], f["ref_label"], f["orient"]))):
        DF.save(os.path.join(root, "images", name + ".jpg"), image.numpy())
        DF.save(os.path.join(root, "labels", name + ".png"), label.numpy())
        DF.save(os.path.join(root, "orients", name + "_orient_dense.png"), orient.numpy())
    DF.save(os.path.join(root, "images_recon", "t.jpg"), f["recon"].numpy())
    points, sizes = pen_record(erase=True)
    script = str(tmp_path / "edits.json")
    with open(script, "w") as fh:
        json.dump({"mask_points": points, "size_points": sizes, "use_ref_mask": False, "use_ref_orient": False}, fh)
    argv = ["--name", "d", "--checkpoints_dir", ck, "--gpu_ids", "-1", "--compute_dtype", "fp32", "--ngf", "8", "--crop_size", str(SIZE), "--load_size", str(SIZE),
            "--add_feat_zeros", "false", "--which_epoch", "7", "--demo_data_dir", root, "--tag", "t", "--ref", "r", "--edit_script", script, "--out", out, "--seed", "3"]
    opt = demo.parse(argv)
    assert not opt.isTrain and opt.no_flip and opt.use_stroke and opt.inpaint_orient and opt.use_encoder and opt.noise_background and opt.expand_mask_be
    assert demo.parse([a for a in argv if a != "false"]).add_feat_zeros and not opt.add_feat_zeros           # on by default, as the reference's demo
    torch.manual_seed(4)
    model = Pix2PixModel(opt)
    model.save("7")
    for net, fname in ((model.netIG, "InpaintingModel_gen.pth"), (model.netSIG, "SInpaintingModel_gen.pth")):
        torch.save({"generator": synth_state_dict(net.state_dict(), seed=2, gain=1.0)}, os.path.join(ck, "d", fname))
    assert demo.main(argv) == 0
    assert sorted(os.listdir(out)) == ["t_from_r.png", "t_from_r_orient.png", "t_from_r_sheet.jpg"]
    result = np.array(Image.open(os.path.join(out, "t_from_r.png")))
    assert result.shape == (SIZE, SIZE, 3) and np.array(Image.open(os.path.join(out, "t_from_r_orient.png"))).shape == (SIZE, SIZE, 3)
    assert Image.open(os.path.join(out, "t_from_r_sheet.jpg")).size == (5 * SIZE, SIZE)
    from michigan_amd.inference import build_model
    session = demo.open_session(opt, build_model(opt), "t", "r", rng=random.Random(3), generator=torch.Generator().manual_seed(3))
    assert session.recon_tag_img is not None
    again, _ = session.edit(points, sizes, False, False)
    assert session.used_recon and np.array_equal(again.numpy(), result)
    with pytest.raises(ValueError, match="lacks"):
        with open(script, "w") as fh:
            json.dump({"mask_points": points}, fh)
        demo.load_script(script)
