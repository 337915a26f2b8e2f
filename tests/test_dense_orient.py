"""CPU: dense hair-orientation extraction (inputs.dense_orientation, python -m michigan_amd.cal_orientation) against what the
reference's own cal_orientation module computed (tests/golden/dense_orient_{i,ii}.npz, written by
tools/make_dense_orient_golden.py), on the float64 contract emulator of mg_orient_smooth (oracle/cabi_emulator.py,
oracle/contracts.py).  The ledger of the C ABI is tests/test_cabi_host.py.

Comparison rule for level maps (dense_orient_fixtures.rule2): in-mask pixels, circular distance min(d, 255 - d), pixels whose
oracle flow magnitude is below 1e-3 of the set's in-mask maximum excluded (at most 0.5 %); bytes equal on >= 99.5 %, within one level
on all, the angle within 8 x the reference's own fp32-vs-float64 gap; outside the mask every byte equal."""
import os

import numpy as np
import pytest
import torch

import dense_orient_fixtures as DE
import parity_utils as PU
from oracle.cabi_emulator import EmulatorBackend

ULP32 = 2.0 ** -23


@pytest.fixture(scope="module")
def fixtures():
    return {tag: DE.load_set(tag) for tag in ("i", "ii")}


@pytest.fixture
def emulator():
    from michigan_amd import _cabi
    em = EmulatorBackend()
    prev = _cabi.set_backend(em)
    yield em
    _cabi.set_backend(prev)


# ---- 1. the bank and the tables ----------------------------------------------------------------------------------------------------------
def test_dog_bank_is_the_references(fixtures):
    from michigan_amd import ops
    bank = ops.dog_bank()
    assert bank.shape == (32, 17, 17) and bank.dtype == torch.float32
    for tag, fx in fixtures.items():
        ref = torch.from_numpy(fx["bank"])
        bound = max(4 * fx["bank_maxabs_diff"], 2 * ULP32 * float(ref.abs().max()))
        diff = float((bank - ref).abs().max())
        print("set %s: dog_bank max abs diff %.3g (bound %.3g)" % (tag, diff, bound))
        assert diff <= bound
    # x runs along rows: filter 0 (theta = 0) is narrow along the row axis (sigma_h 1 / sigma_l 2) and wide along columns (sigma_y 2)
    assert not torch.equal(bank[0], bank[0].t()) and float(bank[0, 8, 8]) == pytest.approx(1.0)


def test_host_tables():
    import math
    from michigan_amd import ops
    trig = ops.orient_trig_table()
    assert trig.shape == (32, 2) and trig.dtype == torch.float32
    a = torch.arange(32, dtype=torch.float32) * math.pi / 31 * 2                 # (sic) the reference's /31
    assert torch.equal(trig[:, 0], torch.cos(a)) and torch.equal(trig[:, 1], torch.sin(a))
    assert float(trig[31, 0]) == pytest.approx(1.0, abs=1e-6)                     # index 31 comes back to angle 2 pi
    taps = ops.gaussian_taps(4.0)
    assert taps.shape == (33,) and taps.dtype == torch.float32 and torch.equal(taps, taps.flip(0))
    assert float(taps.double().sum()) == pytest.approx(1.0, abs=33 * ULP32)
    x = np.arange(-16, 17, dtype=np.float64)
    want = np.exp(-x * x / 32.0)
    assert np.array_equal(taps.numpy(), (want / want.sum()).astype(np.float32))
    for bad in (0.0, -1.0, 4.5):
        with pytest.raises(ValueError):
            ops.gaussian_taps(bad)


# ---- 2. / 3. the contract against the reference's float64 run, and the mutants the fixtures must reject ----------------------------------
@pytest.mark.parametrize("tag", ["i", "ii"])
def test_contract_matches_the_reference(fixtures, tag):
    fx = fixtures[tag]
    ok, fig = DE.rule2(DE.contract_on_fixture(fx), fx)
    print("set %s: %s" % (tag, fig))
    assert ok, fig
    assert fig["compared"] > 5000


@pytest.mark.parametrize("mutant", DE.MUTANTS)
@pytest.mark.parametrize("tag", ["i", "ii"])
def test_fixtures_reject_the_mutant(fixtures, tag, mutant):
    fx = fixtures[tag]
    ok, fig = DE.rule2(DE.contract_on_fixture(fx, mutant), fx)
    print("set %s, %s: %s" % (tag, mutant, fig))
    assert not ok, "set %s does not notice %s" % (tag, mutant)


# ---- 4. inputs.dense_orientation and the command line, on the emulator -------------------------------------------------------------------
def _through_the_op(fx, emulator, as_u8=True, layout="nhwc"):
    from michigan_amd import inputs
    got = {}
    for geo, rec in fx["geometries"].items():
        image = torch.from_numpy(rec["image"])
        if not as_u8:
            image = DE.image_fp32(image)
        if layout == "nchw":
            image = image.permute(0, 3, 1, 2).contiguous()
        before = {k: emulator.count(k) for k in ("mg_gabor_argmax_fwd", "mg_orient_smooth")}
        u8, angle = inputs.dense_orientation(image, torch.from_numpy(rec["mask"]), return_angle=True)
        assert {k: emulator.count(k) - before[k] for k in before} == {"mg_gabor_argmax_fwd": 1, "mg_orient_smooth": 1}
        assert u8.dtype == torch.uint8 and u8.shape == rec["mask"].shape and angle.dtype == torch.float32
        got[geo] = dict(u8=u8.numpy(), theta=angle.numpy())
    return got


@pytest.mark.parametrize("tag", ["i", "ii"])
def test_dense_orientation_end_to_end_on_the_emulator(fixtures, emulator, tag):
    """The emulator's arg-max is the float64 contract of mg_gabor_argmax_fwd: it can differ from the reference's float64 run only at
    ties, so the whole function is held to rule 2 as well."""
    fx = fixtures[tag]
    got = _through_the_op(fx, emulator)
    ok, fig = DE.rule2(got, fx)
    print("set %s: %s" % (tag, fig))
    assert ok, fig
    for layout, as_u8 in (("nchw", True), ("nhwc", False), ("nchw", False)):
        other = _through_the_op(fx, emulator, as_u8=as_u8, layout=layout)
        for geo in got:
            assert np.array_equal(other[geo]["u8"], got[geo]["u8"]) and np.array_equal(other[geo]["theta"], got[geo]["theta"]), (layout, as_u8, geo)


def test_dense_orientation_feeds_orient_to_rgb_and_needs_no_angle(fixtures, emulator):
    from michigan_amd import inputs
    rec = fixtures["i"]["geometries"]["33x47"]
    image, mask = torch.from_numpy(rec["image"]), torch.from_numpy(rec["mask"])
    u8 = inputs.dense_orientation(image, mask)
    assert torch.is_tensor(u8) and u8.dtype == torch.uint8
    assert torch.equal(u8, inputs.dense_orientation(DE.image_fp32(image), mask))          # uint8 and fp32 images: the same bytes
    rgb = inputs.orient_to_rgb_u8(u8, mask, inputs.orient_rgb_table("cpu"))
    assert rgb.shape == u8.shape + (3,) and rgb.dtype == torch.uint8


def test_mask_rule_and_refusals(fixtures, emulator):
    from michigan_amd import inputs, ops
    rec = fixtures["i"]["geometries"]["33x47"]
    image, mask = torch.from_numpy(rec["image"]), torch.from_numpy(rec["mask"])
    want = inputs.dense_orientation(image, mask)
    # a maximum above 1: thresholded at > 130 (cal_orientation.py:91-92) -- 130 itself is background, 131 is hair
    grey = torch.where(mask != 0, torch.tensor(131), torch.tensor(130)).to(torch.uint8)
    assert torch.equal(inputs.dense_orientation(image, grey), want)
    assert torch.equal(inputs.dense_orientation(image, mask.float() * 255.0), want)
    assert torch.equal(inputs.dense_orientation(image, mask.long()), want)
    assert torch.equal(inputs.dense_orientation(image, mask.float().unsqueeze(1)), want)     # [N,1,H,W] label maps
    assert int(inputs.dense_orientation(image, torch.full_like(mask, 130)).max()) == 0
    fimg = DE.image_fp32(image)
    with pytest.raises(ValueError):
        inputs.dense_orientation(fimg.bfloat16(), mask)
    with pytest.raises(ValueError):
        inputs.dense_orientation(fimg[:, :16], mask[:, :16])                                   # H < 17
    with pytest.raises(ValueError):
        inputs.dense_orientation(fimg[:, :, :16], mask[:, :, :16])                             # W < 17
    with pytest.raises(ValueError):
        inputs.dense_orientation(fimg, mask[:, :-1])
    with pytest.raises(ValueError):
        inputs.dense_orientation(fimg, mask, sigma=4.5)
    before = list(emulator.calls)
    conf, idx = torch.zeros(1, 16, 40), torch.zeros(1, 16, 40, dtype=torch.uint8)
    with pytest.raises(ValueError):
        ops.orient_smooth(conf, idx, idx)
    with pytest.raises(ValueError):
        ops.orient_smooth(torch.zeros(1, 20, 40), idx, idx)
    assert emulator.calls == before                                                       # refused before anything is launched


def _write_pairs(fx, tmp_path, names):
    """<names> copies of the crop's image (PNG: lossless) and 0 / 255 masks in two directories"""
    from PIL import Image
    rec = fx["geometries"]["128x128"]
    (tmp_path / "images").mkdir()
    (tmp_path / "masks").mkdir()
    for name in names:
        Image.fromarray(rec["image"][0]).save(tmp_path / "images" / (name + ".png"))
        Image.fromarray(rec["mask"][0] * 255).save(tmp_path / "masks" / (name + ".png"))
    return rec


def _decoded_passes_rule2(path, fx):
    from PIL import Image
    u8 = np.array(Image.open(path))[None]
    rec = fx["geometries"]["128x128"]
    d = DE.circular(u8[rec["mask"] != 0], rec["u8"][rec["mask"] != 0])
    assert (d == 0).mean() >= 0.995 and d.max() <= 1 and not u8[rec["mask"] == 0].any()
    return u8


def test_command_line_single_file(fixtures, emulator, tmp_path, capsys):
    from michigan_amd import cal_orientation
    _write_pairs(fixtures["ii"], tmp_path, ["67172"])
    out = tmp_path / "out"
    cal_orientation.main(["--image_path", str(tmp_path / "images" / "67172.png"), "--hairmask_path", str(tmp_path / "masks" / "67172.png"),
                          "--orientation_root", str(out), "--device", "cpu"])
    assert sorted(os.listdir(out)) == ["67172.png"] and capsys.readouterr().out.strip() == str(out / "67172.png")
    _decoded_passes_rule2(out / "67172.png", fixtures["ii"])
    assert emulator.count("mg_gabor_argmax_fwd") == 1 and emulator.count("mg_orient_smooth") == 1


def test_command_line_directory_in_batches(fixtures, emulator, tmp_path):
    from PIL import Image
    from michigan_amd import cal_orientation
    rec = _write_pairs(fixtures["ii"], tmp_path, ["a", "b", "c"])
    Image.fromarray(rec["image"][0][:100, :90]).save(tmp_path / "images" / "d.png")            # another size: a batch of its own
    Image.fromarray(rec["mask"][0][:100, :90] * 255).save(tmp_path / "masks" / "d.png")
    written = cal_orientation.run(str(tmp_path / "images"), str(tmp_path / "masks"), str(tmp_path / "out"), device="cpu", batch_size=2)
    assert [os.path.basename(p) for p in written] == ["a.png", "b.png", "c.png", "d.png"]
    maps = [_decoded_passes_rule2(tmp_path / "out" / ("%s.png" % n), fixtures["ii"]) for n in "abc"]
    assert all(np.array_equal(m, maps[0]) for m in maps)
    assert np.array(Image.open(tmp_path / "out" / "d.png")).shape == (100, 90)
    assert emulator.count("mg_gabor_argmax_fwd") == 3 and emulator.count("mg_orient_smooth") == 3             # (a, b), (c), (d)
    os.remove(tmp_path / "masks" / "b.png")
    with pytest.raises(FileNotFoundError):
        cal_orientation.run(str(tmp_path / "images"), str(tmp_path / "masks"), str(tmp_path / "out2"), device="cpu")


# ---- 5. the tiling the GPU cases sit on --------------------------------------------------------------------------------------------------------
def test_the_geometry_mirror_is_the_headers_tile():
    d = PU.header_defines("michigan_hip/preprocess/dense_orient.h")
    assert (d["MG_ORIENT_TILE_H"], d["MG_ORIENT_TILE_W"], d["MG_ORIENT_RADIUS"]) == (DE.TILE_H, DE.TILE_W, DE.RADIUS)
    g = DE.kernel_geometry(2, 33, 31)
    assert (g["tiles_y"], g["tiles_x"], g["blocks"]) == (2, 1, 4)
