"""CPU: pin the oracle (oracle/michigan_oracle.py).
  * against the golden vectors produced by the reference itself (always; these travel);
  * against the reference's own modules imported from /root/reference (only where that tree exists)."""
import random

import numpy as np
import pytest
import torch

import parity_utils as PU
from oracle import michigan_oracle as O
from oracle import ref_harness as R

needs_ref = pytest.mark.skipif(not R.reference_available(), reason="/root/reference not present (GPU box)")


def _leaf(sd):
    return {k: v.clone().requires_grad_(v.is_floating_point() and "running" not in k and not k.endswith("_u") and not k.endswith("_v"))
            for k, v in sd.items()}


def _golden_setup():
    from michigan_amd import networks
    from michigan_amd.synth import synth_batch, synth_state_dict
    cfg = PU.load_cfg()
    opt = PU.small_opt()
    with torch.device("meta"):
        tmpl = {k: torch.empty(v.shape, dtype=v.dtype, device="cpu") for k, v in networks.SPADEBGenerator(opt).state_dict().items()}
    sd = _leaf(synth_state_dict(tmpl, seed=cfg["seed_w"], gain=cfg["gain"]))
    return cfg, opt, sd, synth_batch(cfg["n"], cfg["crop_size"], seed=cfg["seed_x"])


def test_oracle_generator_matches_golden():
    cfg, opt, sd, b = _golden_setup()
    g = PU.golden("generator_ngf16_c128.npz")
    taps, upd = {}, {}
    random.seed(cfg["seed_py"])
    out = O.spadeb_generator(sd, opt, b["input_ref"], b["orient"], b["image_ref"], b["input_tag"], b["noise"],
                             b["image_tag"], True, upd, taps=taps)
    assert np.abs(out.detach().numpy() - g["out"]).max() < 5e-5
    for k in g.files:
        if k.startswith("buf."):
            assert np.abs(upd[k[4:]].numpy() - g[k]).max() < 1e-5, k
    gy = torch.randn(out.shape, generator=torch.Generator().manual_seed(99))
    (out * gy).sum().backward()
    import json, os
    names = json.load(open(os.path.join(PU.GOLDEN, "generator_param_names.json")))
    norms = np.array([(-1.0 if sd[k].grad is None else sd[k].grad.double().norm().item()) for k in names])
    m = g["grad_norms"] > 0
    assert ((g["grad_norms"] < 0) == (norms < 0)).all()
    rel = np.abs(norms - g["grad_norms"])[m] / (g["grad_norms"][m] + 1e-3 * g["grad_norms"][m].max())
    assert rel.max() < 2e-3


@needs_ref
def test_oracle_matches_reference_modules():
    from michigan_amd.synth import synth_batch, synth_state_dict
    opt = R.make_opt(ngf=8, ndf=8, crop_size=64, random_expand_mask=True)
    G = R.build_generator(opt).train()
    sd = synth_state_dict(G.state_dict(), seed=21, gain=1.1)
    G.load_state_dict(sd)
    b = synth_batch(3, 64, seed=8)
    random.seed(5)
    ref = G(b["input_ref"], orient_mask=b["orient"], image_ref=b["image_ref"], input_tag=b["input_tag"],
            noise=b["noise"], image_tag=b["image_tag"])
    upd = {}
    random.seed(5)
    out = O.spadeb_generator(sd, opt, b["input_ref"], b["orient"], b["image_ref"], b["input_tag"], b["noise"], b["image_tag"], True, upd)
    assert (out - ref).abs().max().item() < 1e-4
    new = G.state_dict()
    assert max((upd[k] - new[k]).abs().max().item() for k in upd) < 1e-5
    # eval mode (running statistics, no power iteration)
    G.eval()
    opt_e = R.make_opt(ngf=8, ndf=8, crop_size=64, isTrain=False)
    G.opt = opt_e
    G.backgroud_enc.opt = opt_e
    with torch.no_grad():
        ref_e = G(b["input_ref"], orient_mask=b["orient"], image_ref=b["image_ref"], input_tag=b["input_tag"],
                  noise=b["noise"], image_tag=b["image_tag"])
        out_e = O.spadeb_generator(new, opt_e, b["input_ref"], b["orient"], b["image_ref"], b["input_tag"], b["noise"], b["image_tag"], False)
    assert (out_e - ref_e).abs().max().item() < 1e-4

    D = R.build_discriminator(opt).train()
    sdd = synth_state_dict(D.state_dict(), seed=22)
    D.load_state_dict(sdd)
    xin = torch.randn(4, 7, 64, 64)
    r, o = D(xin), O.multiscale_discriminator(xin, sdd, True, {})
    assert max((a - c).abs().max().item() for ra, oa in zip(r, o) for a, c in zip(ra, oa)) < 1e-4

    V = R.build_vgg()
    sdv = synth_state_dict(V.state_dict(), seed=23, gain=1.4)
    V.load_state_dict(sdv)
    xi = torch.randn(1, 3, 32, 32)
    assert max((a - c).abs().max().item() for a, c in zip(V(xi), O.vgg19_features(xi, sdv))) < 1e-4

    L = R.losses()
    gl, fl = L.GANLoss("hinge", tensor=torch.FloatTensor, opt=opt), L.GANFeatLoss(opt)
    lab = b["hair"][:2]
    pf, pr = [[t[:2] for t in p] for p in r], [[t[2:] for t in p] for p in r]
    assert abs(float(gl(pr, True, True, label=lab) - O.gan_hinge_loss(pr, True, True, lab, opt.wide_edge))) < 1e-6
    assert abs(float(gl(pf, False, True, label=lab) - O.gan_hinge_loss(pf, False, True, lab, opt.wide_edge))) < 1e-6
    assert abs(float(gl(pf, True, False, label=lab) - O.gan_hinge_loss(pf, True, False, lab, opt.wide_edge))) < 1e-6
    assert abs(float(fl(pf, pr, lab) - O.gan_feat_loss(pf, pr, opt.lambda_feat))) < 1e-6


@needs_ref
def test_state_dict_contract_fixture_is_current():
    """The committed key/shape contract equals what the reference builds today."""
    import json, os
    contract = json.load(open(os.path.join(PU.GOLDEN, "state_dict_contract.json")))
    opt = R.make_opt()
    assert {k: list(v.shape) for k, v in R.build_generator(opt).state_dict().items()} == contract["G"]
    assert {k: list(v.shape) for k, v in R.build_discriminator(opt).state_dict().items()} == contract["D"]


def test_oracle_orientation_loss_matches_reference():
    from michigan_amd.synth import synth_batch
    b = synth_batch(2, 64, seed=3)
    fake = torch.tanh(torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(4)))
    # the reference's L1OLoss (orient_filter gabor) on these inputs, recorded by `python oracle/make_golden.py --oracle`
    want_o, want_c = PU.golden("oracle_reference.npz")["orient_loss"]
    got_o, got_c = O.orientation_loss(fake, b["orient"], b["input_tag"], use_ig=True)
    assert abs(float(want_o) - float(got_o)) < 1e-6 and abs(float(want_c) - float(got_c)) < 1e-5


@needs_ref
def test_orient_random_disturb_matches_reference_and_hip_classes_match_the_oracle():
    """--orient_random_disturb (reference generator.py:98-105,136-140; VERDICT r5 "missing" 5): the oracle against the LIVE reference generator,
    then this repo's generator (contract emulator) against the oracle -- same weights, same inputs, both use_ig forms of the orientation map."""
    from michigan_amd import _cabi, networks
    from michigan_amd.model import default_options
    from michigan_amd.synth import synth_batch, synth_loader_batch, synth_state_dict
    from oracle.cabi_emulator import EmulatorBackend
    for use_ig in (True, False):
        opt = R.make_opt(ngf=8, ndf=8, crop_size=64, random_expand_mask=False, orient_random_disturb=True, use_ig=use_ig)
        G = R.build_generator(opt).train()
        sd = synth_state_dict(G.state_dict(), seed=24, gain=1.1)
        G.load_state_dict(sd)
        b = synth_batch(2, 64, seed=9)
        orient = b["orient"] if use_ig else synth_loader_batch(2, 64, seed=9)["orient"]
        random.seed(5)
        ref = G(b["input_ref"], orient_mask=orient, image_ref=b["image_ref"], input_tag=b["input_tag"], noise=b["noise"], image_tag=b["image_tag"])
        random.seed(5)
        out = O.spadeb_generator(sd, opt, b["input_ref"], orient, b["image_ref"], b["input_tag"], b["noise"], b["image_tag"], True, {})
        assert (out - ref).abs().max().item() < 1e-4
        plain = O.spadeb_generator(sd, R.make_opt(ngf=8, ndf=8, crop_size=64, random_expand_mask=False, use_ig=use_ig), b["input_ref"], orient,
                                   b["image_ref"], b["input_tag"], b["noise"], b["image_tag"], True, {})
        assert (out - plain).abs().max().item() > 1e-3                      # the option really changes the conditioning
        prev = _cabi.set_backend(EmulatorBackend())
        try:
            hopt = default_options(ngf=8, ndf=8, crop_size=64, gpu_ids=[], compute_dtype="fp32", random_expand_mask=False, orient_random_disturb=True, use_ig=use_ig)
            H = networks.SPADEBGenerator(hopt).train()
            H.load_state_dict(sd)
            random.seed(5)
            with torch.no_grad():
                got = H(b["input_ref"], orient_mask=orient, image_ref=b["image_ref"], input_tag=b["input_tag"], noise=b["noise"], image_tag=b["image_tag"])
        finally:
            _cabi.set_backend(prev)
        assert (got.float() - ref).abs().max().item() < 2e-4


@needs_ref
def test_most_upsampling_matches_reference_and_hip_classes_match_the_oracle():
    """--num_upsampling_layers most (reference generator.py:66-68,84,156-159,221-224, encoder.py:276-278,323-327,338-339: a seventh upsample, `up_4` at half
    width, `conv0` / `layer0` in the background encoder, five blend levels): the oracle against the LIVE reference generator, forward and the
    gradients of a few parameters the variant adds, then this repo's generator (contract emulator) against the oracle."""
    from michigan_amd import _cabi, networks
    from michigan_amd.model import default_options
    from michigan_amd.synth import synth_batch, synth_state_dict
    from oracle.cabi_emulator import EmulatorBackend
    opt = R.make_opt(ngf=16, ndf=8, crop_size=256, random_expand_mask=False, num_upsampling_layers="most")
    G = R.build_generator(opt).train()
    sd = synth_state_dict(G.state_dict(), seed=25, gain=1.1)
    assert "up_4.conv_0.weight_orig" in sd and "backgroud_enc.conv0.conv.weight" in sd and sd["conv_img.weight"].shape[1] == 8
    G.load_state_dict(sd)
    b = synth_batch(2, 256, seed=10)
    names = ["up_4.conv_0.weight_orig", "up_4.norm_s.mlp_gamma.weight", "backgroud_enc.conv0.conv.weight", "backgroud_enc.layer0.conv.weight", "conv_img.weight"]
    random.seed(5)
    ref = G(b["input_ref"], orient_mask=b["orient"], image_ref=b["image_ref"], input_tag=b["input_tag"], noise=b["noise"], image_tag=b["image_tag"])
    assert ref.shape == (2, 3, 256, 256)
    gy = torch.randn(ref.shape, generator=torch.Generator().manual_seed(3))
    (ref * gy).sum().backward()
    want = {n: p.grad.clone() for n, p in G.named_parameters() if n in names}
    random.seed(5)
    out = O.spadeb_generator(sd, opt, b["input_ref"], b["orient"], b["image_ref"], b["input_tag"], b["noise"], b["image_tag"], True, {})
    assert (out - ref.detach()).abs().max().item() < 1e-4
    prev = _cabi.set_backend(EmulatorBackend())
    try:
        hopt = default_options(ngf=16, ndf=8, crop_size=256, gpu_ids=[], compute_dtype="fp32", random_expand_mask=False, num_upsampling_layers="most")
        H = networks.SPADEBGenerator(hopt).train()
        assert list(H.state_dict().keys()) == list(G.state_dict().keys())       # same keys, same order as the reference's 'most' generator
        H.load_state_dict(sd)
        random.seed(5)
        got = H(b["input_ref"], orient_mask=b["orient"], image_ref=b["image_ref"], input_tag=b["input_tag"], noise=b["noise"], image_tag=b["image_tag"])
        (got.float() * gy).sum().backward()
        grads = {n: p.grad.clone() for n, p in H.named_parameters() if n in names}
    finally:
        _cabi.set_backend(prev)
    assert (got.detach().float() - ref.detach()).abs().max().item() < 2e-4
    for n in names:
        assert (grads[n] - want[n]).norm().item() <= 2e-3 * want[n].norm().item(), n
