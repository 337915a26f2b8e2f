"""CPU: the style / content terms through every host layer, on the float64 contract emulator of mg_feat_moment_loss_fwd /
mg_feat_moment_loss_bwd (oracle/cabi_emulator.py, oracle/contracts.py), against what the REFERENCE's own StyleContentLoss methods and trainer computed
(tests/golden/style_loss_{i,ii}.npz, trainer_S*.npz from tools/make_style_golden.py).

  1  the emulator contract vs the reference's float64 run: pins the contract in include/michigan_hip/feature_losses.h to the reference;
  2  ops.feat_moment_loss through the C ABI (NCHW views of NHWC storage, strided planes, flag subsets, call counts, lazy backward);
  3  networks.StyleContentLoss;  4 the real library's argument checks;
  5  Pix2PixModel: keys, one vgg(fake) pass, the terms when the reference is not the target, nothing called with both flags off;
  6  this package's trainer vs trainer_S;  7 two ranks over gloo against one rank on the concatenated batch.
The kernels themselves are checked on the GPU (tests/test_gpu_style_loss.py).
"""
import socket

import pytest
import torch

import parity_utils as PU
import style_loss_fixtures as SE
from oracle import contracts as K
from oracle import trainer_parity as TP
from oracle.cabi_emulator import EmulatorBackend

# tests/test_color_loss.py::TOL
TOL = dict(rtol_loss0=2e-4, rtol_later=1e-2, atol_img=2e-4, atol_weight=2 * 4e-4 * 2 + 1e-5)
SMALL = dict(TP.CFGS["A"], ngf=8, ndf=8, crop=64)
MASK_KEYS = ("mask_x", "mask_s", "mask_t")
SETS = SE.make_sets()


@pytest.fixture
def style_emulator():
    from michigan_amd import _cabi
    be = EmulatorBackend()
    prev = _cabi.set_backend(be)
    yield be
    _cabi.set_backend(prev)


def _masks(p, masked):
    return [p[k] for k in MASK_KEYS] if masked else [None] * 3


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["i", "ii"])
@pytest.mark.parametrize("mode", ["plain", "masked"])
def test_contract_matches_the_reference_in_float64(tag, mode):
    p, fx = SETS[tag], SE.load_set(tag)
    weights = tuple(fx["weights"].tolist())
    assert weights == SE.WEIGHTS
    losses, grad = K.style_terms(p["x"], p["s"], p["t"], *_masks(p, mode == "masked"), flags=3, weights=weights)
    want_l, want_g = fx["losses_" + mode], fx["grad_" + mode]
    for k in range(2):
        assert abs(float(losses[k]) - float(want_l[k])) <= 1e-9 * abs(float(want_l[k])), (k, losses, want_l)
    assert float((grad - want_g).norm() / want_g.norm()) <= 1e-9                          # every element
    if tag == "ii" and mode == "masked":
        # "the mask value multiplies": read as a predicate, the fractional rows move each term by far more than the 1e-9 above allows
        pred = K.style_terms(p["x"], p["s"], p["t"], *[(m != 0).float() for m in _masks(p, True)], flags=3)[0]
        for k in range(2):
            assert abs(float(pred[k]) - float(want_l[k])) > 1e-4 * float(want_l[k]), k
        # empty masks: mu = 0, sigma = sqrt(1e-5), nothing is NaN, and the style gradient of the sample with an empty mask_x is exactly 0
        assert float(p["mask_x"][1].sum()) == 0 and float(p["mask_s"][2].sum()) == 0
        style_only = K.style_terms(p["x"], p["s"], None, p["mask_x"], p["mask_s"], None, flags=1)[1]
        assert bool(torch.isfinite(style_only).all()) and float(style_only[1].abs().max()) == 0.0
        assert float((style_only * (p["mask_x"] == 0).unsqueeze(1)).abs().max()) == 0.0
        n, c = p["x"].shape[:2]
        mu, sg, _, _ = K.moments(p["x"].double().reshape(n, c, -1), p["mask_x"].double().reshape(n, -1))
        assert float(mu[1].abs().max()) == 0.0 and float((sg[1] - K.FEAT_EPS ** 0.5).abs().max()) == 0.0


def test_the_fixture_separates_shifted_from_unshifted_sums():
    """What tools/make_style_golden.py asserted when it wrote set ii: the E[x^2] - mu^2 mutant misses the GPU test's fp32 bound."""
    fx = SE.load_set("ii")
    assert fx["mutant_grad_rel_l2"] > max(4 * fx["ref32_grad_rel_l2_plain"], 8 * 2.0 ** -23)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
# The backward reads the forward's table {a, b, mu_x} in fp32 (that is the contract).  Three roundings of factors (a, b, the fp32 dx)
# give 2e-7 like the other fused losses; the rounding of mu_x, half an fp32 ulp of |mu|, enters (x - mu_x) relative to the features'
# standard deviation: 2^-24 |mu| / sigma, with |mu| / sigma <= 1 on set i (unit-scale features) and 8 / 0.25 = 32 on set ii.
GRAD_TOL = {"i": 2e-7 + 2.0 ** -24 * 1, "ii": 2e-7 + 2.0 ** -24 * 32}


def _nchw_view(f, dtype=torch.float32):
    """The towers' output: an NCHW view of NHWC storage."""
    return f.permute(0, 2, 3, 1).contiguous().to(dtype).permute(0, 3, 1, 2)


@pytest.mark.parametrize("tag", ["i", "ii"])
@pytest.mark.parametrize("mode", ["plain", "masked"])
@pytest.mark.parametrize("flags", [1, 2, 3])
def test_ops_feat_moment_loss_on_the_emulator(style_emulator, tag, mode, flags):
    from michigan_amd import ops
    assert (ops.FEAT_STYLE, ops.FEAT_CONTENT) == (1, 2)
    p, fx = SETS[tag], SE.load_set(tag)
    masked = mode == "masked"
    store = p["x"].permute(0, 2, 3, 1).contiguous().requires_grad_(True)
    x = store.permute(0, 3, 1, 2)
    lab = torch.stack(_masks(p, True), dim=1).contiguous()                   # channel views of one label: strided planes
    assert not lab[:, 1].is_contiguous()
    masks = [lab[:, i] for i in range(3)] if masked else [None] * 3
    style, content = ops.feat_moment_loss(x, _nchw_view(p["s"]), _nchw_view(p["t"]), *masks, flags=flags)
    (SE.WEIGHTS[0] * style + SE.WEIGHTS[1] * content).backward()
    want_g = K.style_terms(p["x"], p["s"], p["t"], *_masks(p, masked), flags=flags, weights=SE.WEIGHTS)[1]
    for k, got in enumerate((style, content)):
        if flags & (1 << k):
            want = float(fx["losses_" + mode][k])
            assert abs(float(got.detach()) - want) <= 2e-7 * want                # one rounding to the fp32 output
        else:
            assert float(got.detach()) == 0.0
    g = store.grad.permute(0, 3, 1, 2).double()
    assert float((g - want_g).norm() / want_g.norm()) <= GRAD_TOL[tag]
    if flags == 3:
        assert float((g - fx["grad_" + mode]).norm() / fx["grad_" + mode].norm()) <= GRAD_TOL[tag]
    assert style_emulator.flags("mg_feat_moment_loss_fwd") == [flags] and style_emulator.flags("mg_feat_moment_loss_bwd") == [flags]       # one forward and one backward call
    assert style_emulator.flags("mg_hair_lab_fwd") == [] and style_emulator.flags("mg_hair_lab_bwd") == []


def test_ops_feat_moment_loss_reads_the_view_in_place_and_checks(style_emulator):
    from michigan_amd import ops
    p = SETS["i"]
    seen = []
    orig = style_emulator.mg_feat_moment_loss_fwd
    style_emulator.mg_feat_moment_loss_fwd = lambda d, stream=None: (seen.append((d.x, d.s, d.t)), orig(d, stream))[1]
    x, s, t = _nchw_view(p["x"]).requires_grad_(True), _nchw_view(p["s"]), _nchw_view(p["t"])
    style, content = ops.feat_moment_loss(x, s, t, flags=3)
    assert seen[0] == (x.data_ptr(), s.data_ptr(), t.data_ptr()), "an NCHW view of NHWC storage must not be copied"
    # a plain contiguous NCHW tensor works too (one copy), bf16 features are rounded once
    plain = ops.feat_moment_loss(p["x"].clone(), p["s"], p["t"], flags=3)
    assert float(plain[0]) == float(style.detach()) and float(plain[1]) == float(content.detach())
    bf = ops.feat_moment_loss(_nchw_view(p["x"], torch.bfloat16), _nchw_view(p["s"], torch.bfloat16), None, flags=1)[0]
    r = lambda k: p[k].to(torch.bfloat16).float()
    want = K.style_terms(r("x"), r("s"), None, flags=1)[0][0]
    assert abs(float(bf) - float(want)) <= 2e-7 * float(want)
    with pytest.raises(ValueError, match="flags"):
        ops.feat_moment_loss(x, s, t, flags=0)
    with pytest.raises(ValueError, match="flags"):
        ops.feat_moment_loss(x, s, t, flags=4)
    with pytest.raises(ValueError, match="content features"):
        ops.feat_moment_loss(x, s, None, flags=3)
    with pytest.raises(ValueError, match="does not match"):
        ops.feat_moment_loss(x, s[:, :, :-1], t, flags=1)
    with pytest.raises(ValueError, match="does not match"):
        ops.feat_moment_loss(x, s, t, p["mask_x"][:, :-1], p["mask_s"], flags=1)
    with pytest.raises(ValueError, match="come together"):
        ops.feat_moment_loss(x, s, t, p["mask_x"], None, flags=1)
    with pytest.raises(ValueError, match="multiple of"):
        ops.feat_moment_loss(x[:, :6], s[:, :6], None, flags=1)
    with pytest.raises(ValueError, match="two pixels"):
        ops.feat_moment_loss(x[:, :, :1, :1], s[:, :, :1, :1], None, flags=1)
    # terms not selected need no operands; nothing flows back when no gradient arrives; one arriving gradient leaves the other NULL
    style_emulator.calls.clear()
    style, content = ops.feat_moment_loss(x, None, t, flags=ops.FEAT_CONTENT)
    assert float(style.detach()) == 0.0 and style_emulator.flags("mg_feat_moment_loss_fwd") == [2]
    style, content = ops.feat_moment_loss(x, s, t, *_masks(p, True), flags=3)
    (x.sum() * 0 + 1.0).backward()
    assert style_emulator.flags("mg_feat_moment_loss_bwd") == []
    x.grad = None
    style.backward()
    assert style_emulator.flags("mg_feat_moment_loss_bwd") == [3]
    want = K.style_terms(p["x"], p["s"], None, p["mask_x"], p["mask_s"], None, flags=1)[1]
    assert float((x.grad.double() - want).norm() / want.norm()) <= 2e-7


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
class _Tower(torch.nn.Module):
    """Stands in for VGG19: five NCHW views of NHWC storage at halving resolutions, differentiable, counts its passes."""

    def __init__(self):
        super().__init__()
        self.calls = 0
        g = torch.Generator().manual_seed(9)
        self.mix = [torch.randn(8, 3, generator=g) for _ in range(5)]

    def forward(self, img):
        self.calls += 1
        outs = []
        for i, w in enumerate(self.mix):
            f = torch.nn.functional.avg_pool2d(img, 2 ** i) if i else img
            f = torch.einsum("oc,nchw->nhwo", w, f).contiguous()
            outs.append(f.relu().permute(0, 3, 1, 2))
        return outs


def _images(n=2, size=32, seed=3):
    g = torch.Generator().manual_seed(seed)
    img = lambda: torch.rand(n, 3, size, size, generator=g) * 2 - 1
    lab = lambda: (torch.rand(n, 1, size, size, generator=g) < 0.5).float()
    return img(), img(), img(), lab(), lab()


@pytest.mark.parametrize("remove_background", [False, True])
def test_loss_class_matches_the_reference_formulation(style_emulator, remove_background):
    """The reference's forward (loss.py:697-711) spelled with the float64 contract: content at the last tap only, style summed over the
    five taps, labels resized per tap with nearest sampling, the FAKE features under the STYLE label and the style features under
    the CONTENT label (loss.py:692-693, literally)."""
    import types
    import torch.nn.functional as F
    from michigan_amd import networks
    tower = _Tower()
    crit = networks.StyleContentLoss(types.SimpleNamespace(remove_background=remove_background), vgg=tower)
    assert "vgg" not in dict(crit.named_children()), "a shared tower is not registered a second time"
    fake, style_img, content_img, style_lab, content_lab = _images()
    fake.requires_grad_(True)
    loss_c, loss_s = crit(fake, style_img, content_img, style_lab, content_lab)
    assert tower.calls == 3
    assert style_emulator.flags("mg_feat_moment_loss_fwd") == [1, 1, 1, 1, 3]
    with torch.no_grad():
        ff, sf, cf = tower(fake), tower(style_img), tower(content_img)
    want_s, swapped = 0.0, 0.0
    for i in range(5):
        size = ff[i].shape[2:]
        ms = F.interpolate(style_lab, size=size, mode="nearest")[:, 0] if remove_background else None
        mc = F.interpolate(content_lab, size=size, mode="nearest")[:, 0] if remove_background else None
        want_s += float(K.style_terms(ff[i], sf[i], None, ms, mc, None, flags=1)[0][0])
        swapped += float(K.style_terms(ff[i], sf[i], None, mc, ms, None, flags=1)[0][0])
    want_c = float(K.style_terms(ff[4], None, cf[4], None, None, mc, flags=2)[0][1])
    assert abs(float(loss_s.detach()) - want_s) <= 1e-6 * want_s and abs(float(loss_c.detach()) - want_c) <= 1e-6 * want_c
    if remove_background:
        assert abs(swapped - want_s) > 1e-3 * want_s, "the inputs do not tell the two label assignments apart"
    (loss_c + loss_s).backward()
    assert style_emulator.flags("mg_feat_moment_loss_bwd") == [3, 1, 1, 1, 1] and bool(torch.isfinite(fake.grad).all()) and float(fake.grad.abs().max()) > 0
    # features and masks the caller already has are used as they are; a term that is off runs nothing for it
    tower.calls = 0
    style_emulator.calls.clear()
    loss_c2, loss_s2 = crit(fake, style_img, content_img, style_lab, content_lab, fake_feats=tower(fake), content_feats=cf)
    assert tower.calls == 2 and float(loss_c2.detach()) == float(loss_c.detach()) and float(loss_s2.detach()) == float(loss_s.detach())
    tower.calls = 0
    style_emulator.calls.clear()
    only_c, zero = crit(fake, style_img, content_img, style_lab, content_lab, style=False)
    assert zero == 0 and tower.calls == 2 and style_emulator.flags("mg_feat_moment_loss_fwd") == [2] and float(only_c.detach()) == float(loss_c.detach())


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
def test_entry_points_validate_their_arguments_without_a_gpu():
    """Like tests/test_cabi_host.py: the real library, arguments refused before anything touches a device."""
    from michigan_amd import _cabi, build
    be = _cabi.HipBackend(build.build(verbose=False))
    assert be.mg_feat_moment_workspace(0, 4, 8) == 0 and be.mg_feat_moment_workspace(1, 4, 6) == 0 and be.mg_feat_moment_workspace(1, 4, 8) > 0
    ok = dict(x=64, s=128, t=192, mask_x=256, mask_s=320, mask_t=384, mask_x_nstride=4, mask_s_nstride=4, mask_t_nstride=4, P=4,
              dtype=_cabi.MG_BF16, N=1, C=8, flags=3, out=448, coef=512, ws=576)

    def desc(**over):
        d = _cabi.FeatMomentDesc()
        for k, v in dict(ok, **over).items():
            setattr(d, k, v)
        return d
    fwd = lambda **o: be.mg_feat_moment_loss_fwd(desc(**o), None)
    bwd = lambda **o: be.mg_feat_moment_loss_bwd(desc(**o), None, None, o.pop("dx", 640), None)
    for call in (fwd, bwd):
        with pytest.raises(RuntimeError, match="bad dtype"):
            call(dtype=7)
        with pytest.raises(RuntimeError, match="bad geometry"):
            call(N=0)
        with pytest.raises(RuntimeError, match="bad geometry"):
            call(P=0)
        with pytest.raises(RuntimeError, match="16 bytes of channels"):
            call(C=12)                                                       # bf16: C % 8
        with pytest.raises(RuntimeError, match="16 bytes of channels"):
            call(C=6, dtype=_cabi.MG_F32)
        with pytest.raises(RuntimeError, match="flags"):
            call(flags=0)
        with pytest.raises(RuntimeError, match="flags"):
            call(flags=4)
        with pytest.raises(RuntimeError, match="null pointer"):
            call(x=None)
        with pytest.raises(RuntimeError, match="null pointer"):
            call(coef=None)
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            call(x=68)
        with pytest.raises(RuntimeError, match="sample stride below P"):
            call(mask_x_nstride=3)
        with pytest.raises(RuntimeError, match="sample stride below P"):
            call(mask_t_nstride=3)
        with pytest.raises(RuntimeError, match="content features"):
            call(t=None)
        with pytest.raises(RuntimeError, match="P >= 2"):
            call(P=1, mask_x=None, mask_s=None)
    with pytest.raises(RuntimeError, match="style features"):
        fwd(s=None)
    with pytest.raises(RuntimeError, match="together"):
        fwd(mask_s=None)
    with pytest.raises(RuntimeError, match="sample stride below P"):
        fwd(mask_s_nstride=3)
    with pytest.raises(RuntimeError, match=r"out / ws"):
        fwd(ws=None)
    with pytest.raises(RuntimeError, match=r"out / ws"):
        fwd(out=None)
    with pytest.raises(RuntimeError, match="dx"):
        be.mg_feat_moment_loss_bwd(desc(), None, None, None, None)
    # a term whose bit is clear needs no operands: the checks get as far as the last one
    with pytest.raises(RuntimeError, match=r"out / ws"):
        fwd(flags=1, t=None, mask_t=None, ws=None)
    with pytest.raises(RuntimeError, match=r"out / ws"):
        fwd(flags=2, s=None, mask_x=None, mask_s=None, ws=None)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
def _model(**over):
    from michigan_amd.model import Pix2PixModel
    torch.manual_seed(0)
    return Pix2PixModel(TP.repo_options(SMALL, **over))


def _batch(unpaired=False):
    from michigan_amd.synth import synth_loader_batch
    return synth_loader_batch(1, 64, seed=3, unpaired=unpaired)


def _count_tower(model):
    tower = model.criterionVGG.vgg
    seen = []
    orig = tower.forward
    tower.forward = lambda img: (seen.append(bool(img.requires_grad)), orig(img))[1]
    return seen


@pytest.mark.parametrize("remove_background", [False, True])
def test_model_objective_keys_tower_passes_and_call_counts(style_emulator, remove_background):
    from michigan_amd.model import default_options
    o = default_options()
    assert (o.no_style_loss, o.no_content_loss, o.lambda_style, o.lambda_content) == (True, True, 1.0, 1.0)
    model = _model(no_style_loss=False, no_content_loss=False, lambda_style=0.5, lambda_content=3.0, remove_background=remove_background)
    assert model.criterionStyleContent.vgg is model.criterionVGG.vgg, "one tower for the three losses"
    seen = _count_tower(model)
    losses, fake = model(_batch(), mode="generator")
    assert set(losses) == {"GAN", "GAN_Feat", "VGG", "ORIENT", "content", "style"}
    assert seen.count(True) == 1, "vgg(fake) runs once for VGG, style and content"
    assert len(seen) == 3, "besides vgg(fake): vgg(image_tag) shared with the VGG loss, vgg(image_ref) for style"
    assert style_emulator.flags("mg_feat_moment_loss_fwd") == [1, 1, 1, 1, 3]
    # the values: the loss class alone on the same inputs
    with torch.no_grad():
        d = model.preprocess_input(_batch())
        c, s = model.criterionStyleContent(fake.detach(), d["image_ref"], d["image_tag"], d["input_ref"][:, 1:2], d["input_tag"][:, 1:2])
    assert abs(float(losses["content"].detach()) - 3.0 * float(c)) <= 1e-6 * 3.0 * float(c)
    assert abs(float(losses["style"].detach()) - 0.5 * float(s)) <= 1e-6 * 0.5 * float(s)
    style_emulator.calls.clear()
    sum(losses.values()).backward()
    assert sorted(style_emulator.flags("mg_feat_moment_loss_bwd")) == [1, 1, 1, 1, 3]                             # one backward call per tap
    assert ("_mg_style_masks" in model.__dict__) == remove_background
    model.drop_input_caches()
    assert "_mg_style_masks" not in model.__dict__
    # the reference is not the target: GAN_Feat and VGG go, content and style stay (pix2pix_model.py:292-319)
    seen.clear()
    losses, _ = model(_batch(unpaired=True), mode="generator")
    assert set(losses) == {"GAN", "ORIENT", "content", "style"} and style_emulator.flags("mg_feat_moment_loss_fwd") == [1, 1, 1, 1, 3]
    assert seen.count(True) == 1 and len(seen) == 3
    # at curr_step 2 neither is computed
    model.opt.curr_step = 2
    style_emulator.calls.clear()
    losses, _ = model(_batch(unpaired=True), mode="generator")
    assert set(losses) == {"GAN", "ORIENT"} and style_emulator.flags("mg_feat_moment_loss_fwd") == []
    # one of the two: style alone adds vgg(image_ref) only, content alone adds nothing to the tower passes of the VGG loss
    for over, keys, fwd, passes in ((dict(no_style_loss=False), {"style"}, [1] * 5, 3), (dict(no_content_loss=False), {"content"}, [2], 2)):
        m = _model(**over)
        seen = _count_tower(m)
        style_emulator.calls.clear()
        losses, _ = m(_batch(), mode="generator")
        assert set(losses) == {"GAN", "GAN_Feat", "VGG", "ORIENT"} | keys and style_emulator.flags("mg_feat_moment_loss_fwd") == fwd and len(seen) == passes and seen.count(True) == 1


def test_model_with_both_flags_off_calls_nothing(style_emulator):
    model = _model()
    assert not hasattr(model, "criterionStyleContent")
    seen = _count_tower(model)
    losses, _ = model(_batch(), mode="generator")
    assert set(losses) == {"GAN", "GAN_Feat", "VGG", "ORIENT"}
    assert style_emulator.flags("mg_feat_moment_loss_fwd") == [] and style_emulator.flags("mg_feat_moment_loss_bwd") == [] and len(seen) == 2      # vgg(image_tag), vgg(fake): as before
    sum(losses.values()).backward()
    assert style_emulator.flags("mg_feat_moment_loss_fwd") == [] and style_emulator.flags("mg_feat_moment_loss_bwd") == []
    assert "_mg_style_masks" not in model.__dict__


def test_model_without_the_vgg_loss_owns_a_tower(style_emulator):
    model = _model(no_vgg_loss=True, no_style_loss=False, no_content_loss=False)
    assert not hasattr(model, "criterionVGG") and "vgg" in dict(model.criterionStyleContent.named_children())
    losses, _ = model(_batch(), mode="generator")
    assert set(losses) == {"GAN", "GAN_Feat", "ORIENT", "content", "style"}


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
def test_repo_trainer_matches_reference_golden_with_style_and_content(style_emulator):
    from michigan_amd.model import Pix2PixTrainer
    cfg = dict(TP.CFGS["A"], tag="S")
    torch.manual_seed(0)
    trainer = Pix2PixTrainer(TP.repo_options(cfg, no_style_loss=False, no_content_loss=False))
    SE.load_weights(trainer, cfg)
    rec = SE.drive_style(trainer, cfg)
    gold = PU.load_trainer_golden("S")
    for it, keys in SE.STYLE_LOSS_KEYS.items():
        assert {k.split(".")[-1] for k in gold if k.startswith("it%d.loss." % it)} == set(keys)
    assert {k for k in rec if ".loss." in k} == {k for k in gold if ".loss." in k}, "the trainer reports other losses than the reference"
    assert style_emulator.flags("mg_feat_moment_loss_fwd") == [1, 1, 1, 1, 3] * cfg["iters"]
    TP.compare(rec, gold, **TOL)


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
def test_two_ranks_over_gloo_equal_one_rank_on_the_concatenated_batch():
    import torch.multiprocessing as mp
    import style_dp_worker as worker
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=worker.run, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join()
        assert p.exitcode == 0
    for rank in (0, 1):
        ok = got[rank]
        assert ok["plain_matches"] and ok["grad_matches"] and ok["masked_content_is_per_replica"], ok
