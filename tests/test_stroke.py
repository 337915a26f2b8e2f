"""CPU: the stroke route of the interactive demo (inputs.stroke_to_orient / stroke_inputs, ops.stroke_compose / inpaint_finish,
networks.SInpaintGenerator, Pix2PixModel.inpainting_stroke_orient and mode 'demo_inference') against what the reference's own
modules computed (tests/golden/stroke_i.npz, stroke_glue.npz, sinpaint_state_dict_contract.json, written by
tools/make_stroke_golden.py), on the contract emulator of the three entry points (oracle/cabi_emulator.py, oracle/contracts.py).
The ledger of the C ABI is tests/test_cabi_host.py.

Comparison rule for the stroke picture (stroke_fixtures.rule), with tau = 4 x the larger of the reference's own recorded
fp32-against-float64 figures: at every stroke pixel the float64 response of the returned idx is within tau of the float64 maximum and
|conf - max| <= tau; idx is the reference's wherever the float64 top-two gap is >= tau (at most 10 % of the stroke pixels are below);
given idx the RGB bytes are exact; outside the stroke everything is 0; where every response is below -tau, idx and conf are 0."""
import ctypes
import functools
import json
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import parity_utils as PU
import stroke_fixtures as SE
from oracle import contracts as K
from oracle.cabi_emulator import EmulatorBackend


@pytest.fixture(scope="module")
def fixture():
    return SE.load_set("i")


@pytest.fixture(scope="module")
def glue():
    z = np.load(os.path.join(PU.GOLDEN, "stroke_glue.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture
def emulator():
    from michigan_amd import _cabi
    em = EmulatorBackend()
    prev = _cabi.set_backend(em)
    yield em
    _cabi.set_backend(prev)


def _cfg():
    with open(os.path.join(PU.GOLDEN, "inpaint_config.json")) as fh:
        return json.load(fh)


def _net(cls_name, device="cpu", dtype=torch.float32, crop=512):
    from michigan_amd import networks
    from michigan_amd.model import default_options
    from michigan_amd.synth import synth_state_dict
    cfg = _cfg()
    net = getattr(networks, cls_name)(default_options(gpu_ids=[], crop_size=crop)).eval()
    net.load_state_dict(synth_state_dict(net.state_dict(), seed=cfg["seed_w"], gain=cfg["gain"]))
    return net.to(device).set_compute_dtype(dtype)


# ---- 1. the bank and the colour table ----------------------------------------------------------------------------------------------------
def test_bank_and_rgb_table_are_the_references(fixture):
    from michigan_amd import ops
    assert np.array_equal(ops.dog_bank().numpy(), fixture["bank"])                 # the stroke module builds the dense module's bank
    table = ops.stroke_rgb_table()
    assert table.shape == (32, 3) and table.dtype == torch.uint8
    assert np.array_equal(table.numpy(), fixture["rgb_table"])
    assert table[0].tolist() == [255, 127, 127] and table[16].tolist() == [0, 127, 127]      # a = 0: (cos, sin) = (1, 0); a = pi / 2: (-1, 0)


# ---- 2. / 3. the contract against the reference, and the mutants the fixture must reject -------------------------------------------------
def test_contract_matches_the_reference(fixture):
    got = SE.contract_on_fixture(fixture)
    ok, fig = SE.rule(got, fixture)
    print(fig)
    assert ok, fig
    assert fig["stroke_pixels"] > 5000 and fig["clamped_tie_pixels"] >= 2
    seen = set()
    for geo, rec in fixture["geometries"].items():
        s = rec["mask"] != 0
        seen |= set(np.unique(rec["idx"][s]).tolist())
        # the reference's own picture (its fp32 run): bytes equal wherever its float64 run decides the index
        decided = s & (rec["gap"] >= fixture["tau"])
        assert np.array_equal(got[geo]["rgb"][decided], rec["rgb"][decided]) and not rec["rgb"][~s].any()
        assert np.abs(got[geo]["conf"] - rec["conf"]).max() < 1e-12
    assert seen == set(range(32))                                                   # all 32 indices occur inside the strokes


def test_the_tau_is_the_recorded_one(fixture):
    assert fixture["tau"] == 4.0 * max(fixture["ref32_gap_at_flip"], fixture["ref32_resp_err"])
    assert 1e-6 < fixture["tau"] < 1e-4                                             # fp32 rounding of a 289-term sum of O(1) terms


@pytest.mark.parametrize("mutant", SE.MUTANTS)
def test_fixture_rejects_the_mutant(fixture, mutant):
    on = SE.fixture_for(fixture, mutant)
    ok, fig = SE.rule(SE.contract_on_fixture(on), on)
    assert ok, fig                                                                  # the contract passes on what the mutant is judged on
    ok, fig = SE.rule(SE.contract_on_fixture(on, mutant), on)
    print(mutant, fig)
    assert not ok, "the fixture does not notice %s" % mutant


def test_the_references_bank_is_point_symmetric(fixture):
    """why `convolution` is judged on a seeded bank: on this one it is the correlation, bit for bit"""
    assert np.array_equal(fixture["bank"], fixture["bank"][:, ::-1, ::-1])
    assert SE.JUDGED_ON_ASYMMETRIC_BANK == ("convolution",)


# ---- 4. inputs.stroke_to_orient / stroke_inputs on the emulator ----------------------------------------------------------------------------
def test_stroke_to_orient_on_the_emulator(fixture, emulator):
    from michigan_amd import inputs, ops
    got = {}
    for geo, rec in fixture["geometries"].items():
        m = torch.from_numpy(rec["mask"])
        before = emulator.count("mg_stroke_orient")
        rgb = inputs.stroke_to_orient(m)
        assert emulator.count("mg_stroke_orient") == before + 1
        assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == m.shape + (3,)
        for other in (m.float(), m.long(), m.bool(), m.unsqueeze(1).double()):
            assert torch.equal(inputs.stroke_to_orient(other), rgb)
        assert torch.equal(inputs.stroke_to_orient(m[0]), rgb[:1])                  # [H,W]: the reference's single canvas
        r2, idx, conf = ops.stroke_orient(m, want_idx=True, want_conf=True)
        assert torch.equal(r2, rgb) and idx.dtype == torch.uint8 and conf.dtype == torch.float32
        got[geo] = dict(rgb=rgb.numpy(), idx=idx.numpy(), conf=conf.numpy())
    ok, fig = SE.rule(got, fixture)
    print(fig)
    assert ok, fig
    m = torch.from_numpy(fixture["geometries"]["33x47"]["mask"])
    assert torch.equal(inputs.stroke_to_orient(m * 255), inputs.stroke_to_orient(m))           # non-zero = stroke
    with pytest.raises(ValueError):
        inputs.stroke_to_orient(torch.zeros(1, 20, 20).bfloat16())
    with pytest.raises(ValueError):
        ops.stroke_orient(torch.zeros(1, 20, 20))
    with pytest.raises(ValueError):
        ops.stroke_orient(torch.zeros(1, 20, 20, dtype=torch.uint8), bank=ops.dog_bank().bfloat16())


def test_stroke_inputs_are_the_loaders_tensors(fixture, emulator):
    """base_dataset.py:214-238 restated with torch on the reference's own picture"""
    from michigan_amd import inputs
    rec = fixture["geometries"]["70x95"]
    m = torch.from_numpy(rec["mask"])
    g = torch.Generator().manual_seed(5)
    label = (torch.rand(2, 1, 70, 95, generator=g) > 0.3).float()
    hole = (torch.rand(2, 70, 95, generator=g) > 0.5).to(torch.uint8)
    d = inputs.stroke_inputs(m, label, hole)
    picture = inputs.stroke_to_orient(m)
    assert set(d) == {"orient_stroke", "mask_stroke", "hole"}
    assert torch.equal(d["orient_stroke"], picture.permute(0, 3, 1, 2).float().div(255) * label)
    assert torch.equal(d["mask_stroke"], m.float().div(255).unsqueeze(1) * 255.0 * label)
    assert torch.equal(d["hole"], hole.float().div(255).unsqueeze(1) * 255.0 * label)
    assert set(d["mask_stroke"].unique().tolist()) <= {0.0, 1.0}
    assert set(inputs.stroke_inputs(m, label)) == {"orient_stroke", "mask_stroke"}
    with pytest.raises(ValueError):
        inputs.stroke_inputs(m, label[:, :, :-1])
    with pytest.raises(ValueError):
        inputs.stroke_inputs(m, label, hole[:, :-1])


# ---- 5. the two glue entry points on the emulator, against the torch expressions ---------------------------------------------------------
@pytest.mark.parametrize("src,dst", [(32, 256), (256, 32), (48, 256), (256, 48)])
def test_interp_nearest_table_is_f_interpolate(src, dst):
    from michigan_amd import ops
    t = ops.interp_nearest_table(src, dst)
    assert t.dtype == torch.int32 and tuple(t.shape) == (dst,) and int(t.min()) >= 0 and int(t.max()) < src
    x = torch.rand(1, 2, src, src, generator=torch.Generator().manual_seed(src + dst))
    assert torch.equal(F.interpolate(x, size=(dst, dst), mode="nearest"), x[:, :, t.long()][:, :, :, t.long()])
    assert ops.interp_nearest_table(src, src) is None
    with pytest.raises(ValueError):
        ops.interp_nearest_table(0, dst)


def _glue_tensors(n, h, w, seed):
    """non-binary masks: every term of the expressions carries rounding"""
    g = torch.Generator().manual_seed(seed)
    r = lambda c: torch.rand(n, c, h, w, generator=g)
    return dict(orient_rgb=r(3), noise=r(3), hole=r(1), stroke=r(3), stroke_mask=r(1) * 0.7, mask=r(1))


@pytest.mark.parametrize("geom", [(2, 32, 32, 256), (2, 33, 47, None)], ids=["32-256-32", "identity"])
@pytest.mark.parametrize("strokes", [True, False])
def test_compose_and_finish_are_the_torch_expressions(emulator, geom, strokes):
    from michigan_amd import ops
    n, h, w, size = geom
    t = _glue_tensors(n, h, w, 100 + h)
    st, sm = (t["stroke"], t["stroke_mask"]) if strokes else (None, None)
    up = (lambda x: F.interpolate(x, size=(size, size), mode="nearest")) if size else (lambda x: x)
    if strokes:
        rgb = t["orient_rgb"] * (1 - t["hole"]) + t["noise"] * (t["hole"] - sm) + st * sm
        want = torch.cat([rgb, t["hole"], sm], dim=1)
    else:
        want = torch.cat([t["orient_rgb"] * (1 - t["hole"]) + t["noise"] * t["hole"], t["hole"], torch.zeros_like(t["hole"])], dim=1)
    want = up(want)
    for dtype in (torch.float32, torch.bfloat16):
        inp = ops.stroke_compose(t["orient_rgb"], t["noise"], t["hole"], st, sm, size=size, dtype=dtype)
        ho, wo = (size, size) if size else (h, w)
        assert tuple(inp.shape) == (n, ho, wo, 8) and inp.dtype == dtype
        assert torch.equal(inp[..., :5].permute(0, 3, 1, 2), want.to(dtype)) and not inp[..., 5:].any()
    net_out = torch.rand(n, 3, size or h, size or w, generator=torch.Generator().manual_seed(9))
    out, o2 = ops.inpaint_finish(net_out, t["hole"], t["orient_rgb"], t["mask"])
    down = F.interpolate(net_out, size=(h, w), mode="nearest") if size else net_out
    want_out = down * t["hole"] + t["orient_rgb"] * (1 - t["hole"])
    w2 = (want_out[:, :-1] - 0.5) * 2
    want_o2 = torch.stack([w2[:, 1], w2[:, 0]], dim=1) * t["mask"]
    assert torch.equal(out, want_out) and torch.equal(o2, want_o2)
    assert emulator.count("mg_stroke_compose") == 2 and emulator.count("mg_inpaint_finish") == 1


def test_glue_refusals(emulator):
    from michigan_amd import ops
    t = _glue_tensors(1, 8, 8, 3)
    before = list(emulator.calls)
    with pytest.raises(ValueError):
        ops.stroke_compose(t["orient_rgb"], t["noise"], t["hole"], t["stroke"], None)
    with pytest.raises(ValueError):
        ops.stroke_compose(t["orient_rgb"], t["noise"][:, :2], t["hole"])
    with pytest.raises(ValueError):
        ops.stroke_compose(t["orient_rgb"].double(), t["noise"], t["hole"])
    with pytest.raises(TypeError):
        ops.stroke_compose(t["orient_rgb"], t["noise"], t["hole"], dtype=torch.float16)
    with pytest.raises(ValueError):
        ops.inpaint_finish(torch.rand(1, 3, 8, 8).bfloat16(), t["hole"], t["orient_rgb"], t["mask"])
    with pytest.raises(ValueError):
        ops.inpaint_finish(torch.rand(1, 3, 8, 8), t["hole"], t["orient_rgb"], t["mask"][:, :, :4])
    assert emulator.calls == before                                             # refused before anything is launched


# ---- 6. the network, the model ---------------------------------------------------------------------------------------------------------
def test_sinpaint_state_dict_contract():
    """Checkpoint compatibility with the reference's SInpaintingModel_gen.pth: same keys and shapes, in order; ONE implementation."""
    from michigan_amd import networks
    from michigan_amd.model import default_options
    opt = default_options(gpu_ids=[])
    with torch.device("meta"):
        mine = {k: list(v.shape) for k, v in networks.SInpaintGenerator(opt).state_dict().items()}
        sister = {k: list(v.shape) for k, v in networks.InpaintGenerator(opt).state_dict().items()}
    with open(os.path.join(PU.GOLDEN, "sinpaint_state_dict_contract.json")) as fh:
        contract = json.load(fh)
    assert len(contract) == 124 and list(mine.keys()) == list(contract.keys()) and mine == contract
    assert mine["encoder.1.weight_orig"] == [64, 5, 7, 7] and sister["encoder.1.weight_orig"] == [64, 4, 7, 7]
    assert {k: v for k, v in mine.items() if v != sister[k]} == {"encoder.1.weight_orig": [64, 5, 7, 7], "encoder.1.weight_v": [5 * 49]}
    assert networks.find_network_using_name("sinpaint", "generator") is networks.SInpaintGenerator
    assert issubclass(networks.SInpaintGenerator, networks.InpaintGenerator)
    assert networks.SInpaintGenerator.forward is networks.InpaintGenerator.forward       # the channel count is a parameter, not a copy
    with pytest.raises(NotImplementedError):
        networks.SInpaintGenerator(opt, skips=True)


def test_sinpaint_module_on_emulator_matches_golden(emulator, glue):
    cfg = _cfg()
    x = torch.rand(cfg["n"], 5, cfg["size"], cfg["size"], generator=torch.Generator().manual_seed(cfg["seed_x"]))
    out = _net("SInpaintGenerator")(x)
    assert tuple(out.shape) == glue["out"].shape
    err = np.abs(out.numpy() - glue["out"]).max()
    print("SInpaintGenerator on the emulator vs the reference: max abs %.3g" % err)
    assert err < 2e-4                                                                # the bound of tests/test_inpaint.py


def glue_shim(device="cpu", dtype=torch.float32, crop=32):
    from michigan_amd.model import Pix2PixModel
    shim = types.SimpleNamespace(opt=types.SimpleNamespace(crop_size=crop), netIG=_net("InpaintGenerator", device, dtype),
                                 netSIG=_net("SInpaintGenerator", device, dtype))
    shim.inpainting_orient = functools.partial(Pix2PixModel.inpainting_orient, shim)
    return shim


def run_glue(shim, branch, device="cpu"):
    from michigan_amd.model import Pix2PixModel
    t = {k: v.to(device) for k, v in SE.glue_inputs(_cfg()["seed_x"] + 1, 32).items()}
    with torch.no_grad():
        return Pix2PixModel.inpainting_stroke_orient(shim, t["hole"], t["orient_rgb"], t["noise"], t["mask"], t["stroke"], t["stroke_mask"],
                                                     t["mask_orient_rgb_" + branch])


def test_inpainting_stroke_orient_on_emulator_matches_golden(emulator, glue):
    """mask == mask_orient_rgb (pix2pix_model.py:441-442): one pass of the stroke net, held to the bounds tests/test_inpaint.py holds one
    pass of the sister net to on the float64 emulator (rgb 2e-4, orient 4e-4: what the reference's own fp32 arithmetic leaves)"""
    rgb, o2 = run_glue(glue_shim(), "equal")
    e_rgb, e_o2 = np.abs(rgb.numpy() - glue["glue_equal.out_rgb"]).max(), np.abs(o2.numpy() - glue["glue_equal.orient"]).max()
    print("branch equal: rgb %.3g, orient %.3g" % (e_rgb, e_o2))
    assert e_rgb < 2e-4 and e_o2 < 4e-4
    assert emulator.count("mg_stroke_compose") == 1 and emulator.count("mg_inpaint_finish") == 1


def test_inpainting_stroke_orient_first_inpainting_on_emulator(emulator, glue):
    """mask != mask_orient_rgb (pix2pix_model.py:432-439): the first in-painting through the existing inpainting_orient, then the stroke
    net.  Two chained passes: each is held to the one-pass bounds on its own -- the first against what the reference's first pass
    returned (glue_less.first_rgb), the second fed from exactly that -- and the chain as a whole to the bounds the fp32 kernels are
    given for it in tests/test_gpu_stroke.py (rgb 1e-3, orient 2e-3): the reference's fp32 error of the first pass goes through the
    second net, so the one-pass bound does not apply to the chain, and float64 cannot be further off than fp32 may be."""
    assert not np.array_equal(glue["glue_less.out_rgb"], glue["glue_equal.out_rgb"])
    shim = glue_shim()
    rgb, o2 = run_glue(shim, "less")
    e_rgb, e_o2 = np.abs(rgb.numpy() - glue["glue_less.out_rgb"]).max(), np.abs(o2.numpy() - glue["glue_less.orient"]).max()
    print("branch less, the chain: rgb %.3g, orient %.3g" % (e_rgb, e_o2))
    assert e_rgb < 1e-3 and e_o2 < 2e-3
    assert emulator.count("mg_stroke_compose") == 1 and emulator.count("mg_inpaint_finish") == 1
    own, seen = shim.inpainting_orient, []

    def first_pass(*args):
        res = own(*args)
        seen.append(np.abs(res[0].numpy() - glue["glue_less.first_rgb"]).max())
        return torch.from_numpy(glue["glue_less.first_rgb"]), res[1]
    shim.inpainting_orient = first_pass
    rgb, o2 = run_glue(shim, "less")
    e_rgb, e_o2 = np.abs(rgb.numpy() - glue["glue_less.out_rgb"]).max(), np.abs(o2.numpy() - glue["glue_less.orient"]).max()
    print("branch less, pass by pass: first %.3g, then rgb %.3g, orient %.3g" % (seen[0], e_rgb, e_o2))
    assert len(seen) == 1 and seen[0] < 2e-4 and e_rgb < 2e-4 and e_o2 < 4e-4


def _demo_batch(n, size, seed=3, device="cpu"):
    """the demo loader's batch (base_dataset.py:161-262) from seeded tensors, on `device` (the stroke entries are made there)"""
    from michigan_amd import inputs
    from michigan_amd.synth import synth_batch
    d = synth_batch(n, size, seed=seed)
    g = torch.Generator().manual_seed(seed)
    orient_rgb = torch.rand(n, 3, size, size, generator=g) * d["hair"]
    d = {k: v.to(device) for k, v in d.items()}
    hair = d["hair"]
    m = torch.from_numpy(SE.polyline_mask(n, size, size, 900 + size)).to(device)
    hole = torch.clamp(F.max_pool2d(m.float().unsqueeze(1), 9, stride=1, padding=4), 0, 1).to(torch.uint8)[:, 0]
    d.update(inputs.stroke_inputs(m, hair, hole))
    d["orient_rgb"] = orient_rgb.to(device)
    d["orient_rgb_mask"] = hair.clone()
    d["orient"] = torch.zeros(n, 1, size, size, device=device)                                     # the loader's 1-channel map: replaced by the in-painted one
    d.pop("hair")
    return d


def test_demo_inference_shapes_and_dtypes(emulator):
    from michigan_amd.model import Pix2PixModel, default_options
    n, size = 1, 64
    opt = default_options(gpu_ids=[], isTrain=False, ngf=8, crop_size=size, compute_dtype="fp32", use_stroke=True, inpaint_mode="stroke",
                          inpaint_orient=True, no_vgg_loss=True)
    model = Pix2PixModel(opt).eval()
    assert isinstance(model.netSIG, torch.nn.Module) and not model.netSIG.training and not any(p.requires_grad for p in model.netSIG.parameters())
    d = _demo_batch(n, size)
    fake, orient_out = model(d, "demo_inference")
    assert tuple(fake.shape) == (n, 3, size, size) and fake.dtype == torch.float32 and torch.isfinite(fake).all()
    assert tuple(orient_out.shape) == (n, size, size, 3) and orient_out.dtype == torch.uint8
    assert emulator.count("mg_stroke_compose") == 1 and emulator.count("mg_inpaint_finish") == 1
    model.opt.inpaint_mode = "ref"                                                   # the demo flips the mode on the live model (demo.py:342-359)
    fake_ref, orient_ref = model(d, "demo_inference")
    assert tuple(orient_ref.shape) == (n, size, size, 3) and orient_ref.dtype == torch.uint8 and tuple(fake_ref.shape) == tuple(fake.shape)
    assert emulator.count("mg_stroke_compose") == 1                             # the existing inpainting_orient, unchanged
    model.opt.inpaint_mode = "stroke"
    with pytest.raises(ValueError, match="mask_stroke"):
        model({k: v for k, v in d.items() if k != "mask_stroke"}, "demo_inference")
    model.opt.use_ig = False
    d2 = dict(d, orient=torch.rand(n, 1, size, size) * 255)
    fake_plain, none = model(d2, "demo_inference")
    assert none is None and tuple(fake_plain.shape) == (n, 3, size, size)


def test_use_stroke_off_builds_no_netsig(emulator):
    from michigan_amd.model import Pix2PixModel, default_options
    opt = default_options(gpu_ids=[], isTrain=False, ngf=8, crop_size=64, compute_dtype="fp32")
    assert (opt.use_stroke, opt.inpaint_mode, opt.netSIG) == (False, "ref", "sinpaint")
    model = Pix2PixModel(opt)
    assert model.netSIG is None and not any(k.startswith("netSIG") for k in model.state_dict())
    with pytest.raises(RuntimeError, match="use_stroke"):
        model.inpainting_stroke_orient(*[torch.zeros(1, 1, 8, 8)] * 7)


# ---- 7. the tiling the GPU cases sit on --------------------------------------------------------------------------------------------------------
def test_the_geometry_mirror_is_the_headers_tile():
    d = PU.header_defines("michigan_hip/editing/stroke_orient.h")
    assert (d["MG_STROKE_TILE_H"], d["MG_STROKE_TILE_W"], d["MG_STROKE_RADIUS"], d["MG_STROKE_FILTERS"]) == (SE.TILE_H, SE.TILE_W, K.STROKE_RADIUS, 32)
    g = SE.kernel_geometry(2, 17, 15)
    assert (g["tiles_y"], g["tiles_x"], g["blocks"]) == (2, 1, 4)


# ---- 8. argument refusals on the real library: validated before the device is touched, so they run without one --------------------------
def test_argument_refusals_on_the_library():
    from michigan_amd import _cabi, build
    be = _cabi.HipBackend(build.build(verbose=False))
    buf = torch.zeros(4096, dtype=torch.uint8)                                       # host memory: nothing may be launched on it
    p = ctypes.c_void_p(buf.data_ptr())
    with pytest.raises(RuntimeError, match="mg_stroke_orient: null pointer"):
        be.mg_stroke_orient(p, p, None, p, None, None, 1, 8, 8, None)
    with pytest.raises(RuntimeError, match="mg_stroke_orient: null pointer"):
        be.mg_stroke_orient(None, p, p, p, None, None, 1, 8, 8, None)
    with pytest.raises(RuntimeError, match="mg_stroke_orient: bad geometry n=1 h=0 w=8"):
        be.mg_stroke_orient(p, p, p, p, None, None, 1, 0, 8, None)
    with pytest.raises(RuntimeError, match="mg_stroke_orient: n h w = .* does not fit 31 bits"):
        be.mg_stroke_orient(p, p, p, p, None, None, 2, 32768, 32768, None)
    with pytest.raises(RuntimeError, match="mg_stroke_compose: stroke and stroke_mask are given together or not at all"):
        be.mg_stroke_compose(p, p, p, p, None, None, None, 0, 1, 8, 8, 8, 8, p, None)
    with pytest.raises(RuntimeError, match="mg_stroke_compose: stroke and stroke_mask are given together or not at all"):
        be.mg_stroke_compose(p, p, p, None, p, None, None, 0, 1, 8, 8, 8, 8, p, None)
    with pytest.raises(RuntimeError, match="mg_stroke_compose: null pointer"):
        be.mg_stroke_compose(p, None, p, None, None, None, None, 0, 1, 8, 8, 8, 8, p, None)
    with pytest.raises(RuntimeError, match="mg_stroke_compose: bad geometry"):
        be.mg_stroke_compose(p, p, p, None, None, None, None, 0, 1, 0, 8, 8, 8, p, None)
    with pytest.raises(RuntimeError, match="mg_stroke_compose: bad dtype"):
        be.mg_stroke_compose(p, p, p, None, None, None, None, 7, 1, 8, 8, 8, 8, p, None)
    with pytest.raises(RuntimeError, match="mg_stroke_compose: a null table is the identity"):
        be.mg_stroke_compose(p, p, p, None, None, None, None, 0, 1, 8, 8, 16, 16, p, None)
    with pytest.raises(RuntimeError, match="mg_inpaint_finish: null pointer"):
        be.mg_inpaint_finish(p, None, None, p, p, p, 1, 8, 8, 8, 8, p, None, None)
    with pytest.raises(RuntimeError, match="mg_inpaint_finish: bad geometry"):
        be.mg_inpaint_finish(p, None, None, p, p, p, 1, 8, 0, 8, 8, p, p, None)
    with pytest.raises(RuntimeError, match="mg_inpaint_finish: a null table is the identity"):
        be.mg_inpaint_finish(p, None, None, p, p, p, 1, 8, 8, 4, 4, p, p, None)
    assert not buf.any()
