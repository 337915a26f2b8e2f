"""Generate the fixtures of the --balance_Lab weighting by running the REFERENCE's own classes:

    python tools/make_lab_balance_golden.py            (where the reference checkout is; CPU, ~2 min)

  tests/golden/ab_count.npz      the reference's data/ab_count.npy (a 256 x 256 float64 histogram of hair colours over the a/b plane, the
        file --weight_dir names by default), recompressed: data the reference reads at run time.
  tests/golden/lab_balance_i.npz, lab_balance_ii.npz   two seeded input pairs at N=2, 3x96x80 with a 0/1 hair plane and its complement as
        the background plane: the inputs (fp32); S, what HairAvgLabLoss.cal_weight (the variant without mask and replacement) returns
        over all 65536 bin pairs; the three losses and d(w_l lab + w_r rgb + w_b background) / d fake from
        LabColorLoss(balance_Lab=True) / nn.L1Loss / RGBBackgroundL1Loss in FLOAT64 on the fp32-rounded inputs (M cast to float64 as in
        tools/make_color_loss_golden.py; the table inside stays the reference's own fp32); the per-pixel weights; the pixels left out
        of gradient comparisons; and the error of the same classes run in FLOAT32 against their float64 run -- the yardstick of the
        fp32 kernel's bound (tests/test_gpu_lab_balance.py).  Pair i: Lab_weight_th = 10 (the default); pair ii: 1e4, so that the
        weights span their whole range.
  tests/golden/lab_balance_hair.npz   the same for HairAvgLabLoss(balance_Lab=True): three samples whose reference hair has different
        mean colours, one of them with an empty reference mask, Lab_weight_th = 1e4.
  tests/golden/trainer_L.npz, trainer_L_weights.npz, trainer_lab_balance_config.json   the reference's own Pix2PixTrainer on configuration
        A with the README flags as published plus --balance_Lab --weight_dir <the file>, two iterations, recorded like trainer_C.

Nothing of the reference is edited.  Its classes build their table with `self.FloatTensor = torch.cuda.FloatTensor`; the instance
attribute is set to torch.FloatTensor here.  The `1 - mask` of a bool mask is handled by the shim of tools/make_color_loss_golden.py.

What the inputs have to be, each asserted below:
  * uniform random RGB is the wrong input (almost every pixel lands on a bin at the cap): a grey base plus chroma noise is used, at
    least 10 % of the hair pixels get a weight below the cap and at least 30 distinct weights appear;
  * the weight jumps at integer values of a + 128 and b + 128: target pixels within EDGE_MARGIN of one are redrawn until none remains,
    and the margin is at least 4 x the largest |a32 - a64|, |b32 - b64| of the float32 run -- so no pixel is left out for its bin;
  * the only pixels left out of gradient comparisons are the sign() ones of the existing tool, at most EXCLUDE_CAP of them;
  * no RGB colour reaches bin 255 of a or b (the tool scans the RGB cube and says so): bin 255 is covered by hand-made tables in the tests.
"""
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden")

from make_color_loss_golden import EXCLUDE_BELOW, EXCLUDE_CAP, WEIGHTS, _shim_rsub, excluded  # noqa: E402  (same directory)

N, H, W = 2, 96, 80
EDGE_MARGIN = 1e-3
TH = {"i": 10.0, "ii": 1e4}
HAIR_TH = 1e4
HAIR_EDGE_MARGIN = 0.01


def reference_root():
    from oracle import ref_harness as R
    R.setup()
    import models
    return os.path.dirname(os.path.dirname(os.path.abspath(models.__file__)))


def _opt(npy, th):
    return types.SimpleNamespace(balance_Lab=True, weight_dir=npy, Lab_weight_th=th)


def _lab_cls(npy, th, dtype):
    import models.networks.loss as RL
    cls = RL.LabColorLoss(_opt(npy, th))
    cls.FloatTensor = torch.FloatTensor
    cls.M = cls.M.to(dtype)
    return cls


def _hair_cls(npy, th, dtype):
    import models.networks.loss as RL
    cls = RL.HairAvgLabLoss(_opt(npy, th))
    cls.FloatTensor = torch.FloatTensor
    cls.M = cls.M.to(dtype)
    return cls


def reference_table(npy, th):
    """S [256][256]: the reference's cal_weight (HairAvgLabLoss's: no mask, no replacement) on an image whose pixel (i, j) has
    a + 128 = i + 0.25 and b + 128 = j + 0.25"""
    cls = _hair_cls(npy, th, torch.float32)
    lab = torch.zeros(1, 3, 256, 256)
    lab[0, 1] = (torch.arange(256, dtype=torch.float32) - 128 + 0.25).view(256, 1)
    lab[0, 2] = (torch.arange(256, dtype=torch.float32) - 128 + 0.25).view(1, 256)
    return cls.cal_weight(lab)[0, 0].contiguous()


def ab_of(cls, x):
    lab = cls.xyz2lab(cls.rgb2xyz((x + 1) / 2))
    return lab[:, 1], lab[:, 2]


def scan_rgb_cube(npy):
    cls = _lab_cls(npy, 10.0, torch.float64)
    v = torch.linspace(-1, 1, 65, dtype=torch.float64)
    rgb = torch.stack(torch.meshgrid(v, v, v, indexing="ij"), dim=0).reshape(1, 3, 65 * 65, 65)
    a, b = ab_of(cls, rgb)
    lo, hi = float(min(a.min(), b.min())) + 128, float(max(a.max(), b.max())) + 128
    print("RGB cube scan (65^3 colours, corners included): a + 128 in [%.2f, %.2f], b + 128 in [%.2f, %.2f]: no RGB colour reaches bin 255 "
          "(nor bin 0); bin 255 is covered by hand-made tables in the tests" % (float(a.min()) + 128, float(a.max()) + 128, float(b.min()) + 128,
                                                                               float(b.max()) + 128))
    assert 1 < lo and hi < 254
    return lo, hi


def make_pairs(npy):
    """{tag: (fake, real, hair)}: a grey base plus chroma noise, target pixels away from the bin edges"""
    g = torch.Generator().manual_seed(2026)
    cls = _lab_cls(npy, 10.0, torch.float64)
    out = {}
    for tag, sd in (("i", 0.06), ("ii", 0.09)):
        def draw(shape):
            grey = torch.rand(shape[0], 1, *shape[2:], generator=g) * 1.4 - 0.7
            return (grey + sd * torch.randn(shape, generator=g)).clamp(-1, 1)
        real = draw((N, 3, H, W))
        for rounds in range(100):
            a, b = ab_of(cls, real.double())
            near = ((a + 128 - (a + 128).round()).abs() < EDGE_MARGIN) | ((b + 128 - (b + 128).round()).abs() < EDGE_MARGIN)
            if not bool(near.any()):
                break
            fresh = draw((N, 3, H, W))
            real = torch.where(near.unsqueeze(1), fresh, real)
        assert not bool(near.any()), "target pixels remain near a bin edge"
        fake = (real + 0.15 * torch.randn(N, 3, H, W, generator=g)).clamp(-1, 1)
        if tag == "ii":
            fake[:, :, 40:48, 24:32] = real[:, :, 40:48, 24:32]               # an exactly equal patch: sign(0) = 0
        hair = (torch.rand(N, H, W, generator=g) > 0.4).float()
        if tag == "ii":
            hair[:, 40:48, 24:28] = 1                                         # the equal patch on both sides of the mask
            hair[:, 40:48, 28:32] = 0
        print("pair %s: %d redraw round(s)" % (tag, rounds))
        out[tag] = (fake, real, hair)
    return out


def reference_run(npy, th, fake, real, hair, dtype):
    """The reference classes in `dtype`: (losses[3], d(weighted sum)/d fake, (da, db, drgb), per-pixel weight, (a, b) of the target)"""
    import models.networks.loss as RL
    lab_cls, bg_cls = _lab_cls(npy, th, dtype), RL.RGBBackgroundL1Loss()
    f = fake.to(dtype).clone().requires_grad_(True)
    r = real.to(dtype)
    sem = torch.stack([1 - hair, hair], dim=1).to(dtype)                 # the one-hot label: channel 0 = background, 1 = hair
    lab = lab_cls(f, r.detach(), sem[:, 1:2])
    rgb = torch.nn.L1Loss()(f, r.detach())
    bg = bg_cls(f, sem, r)
    (WEIGHTS[0] * lab + WEIGHTS[1] * rgb + WEIGHTS[2] * bg).backward()
    with torch.no_grad():
        lf = lab_cls.xyz2lab(lab_cls.rgb2xyz((f + 1) / 2))
        lr = lab_cls.xyz2lab(lab_cls.rgb2xyz((r + 1) / 2))
        deltas = (lf[:, 1] - lr[:, 1], lf[:, 2] - lr[:, 2], f - r)
        w = lab_cls.cal_weight(lr, sem[:, 1:2].clone())[:, 0]
    return torch.stack([lab, rgb, bg]).detach(), f.grad.detach(), deltas, w.detach(), (lr[:, 1].detach(), lr[:, 2].detach())


def make_color(npy):
    for tag, (fake, real, hair) in make_pairs(npy).items():
        th = TH[tag]
        S = reference_table(npy, th)
        l64, g64, deltas, w64, (a64, b64) = reference_run(npy, th, fake, real, hair, torch.float64)
        l32, g32, _, w32, (a32, b32) = reference_run(npy, th, fake, real, hair, torch.float32)
        ab_err = max(float((a32.double() - a64).abs().max()), float((b32.double() - b64).abs().max()))
        ex = excluded(deltas)
        keep = (~ex).unsqueeze(1).double()
        share = float(ex.double().mean())
        on_hair = hair > 0
        below = float((w64[on_hair] < th).double().mean())
        distinct = int(torch.unique(w64[on_hair]).numel())
        err_loss = ((l32.double() - l64).abs() / l64.abs()).numpy()
        err_grad = float(((g32.double() - g64) * keep).norm() / (g64 * keep).norm())
        err_grad_max = float(((g32.double() - g64) * keep).abs().max() / g64.abs().max())
        print("pair %s (th %g): losses %s | hair pixels below the cap %.3f, distinct weights %d, range [%.4g, %.4g] | largest |ab32 - ab64| %.2e "
              "(margin %.0e) | excluded %.2e | fp32 reference: loss rel %s, grad rel L2 %.2e, max/largest %.2e | weights equal in fp32: %s"
              % (tag, th, l64.numpy(), below, distinct, float(w64[on_hair].min()), float(w64[on_hair].max()), ab_err, EDGE_MARGIN, share, err_loss,
                 err_grad, err_grad_max, bool(torch.equal(w32.double(), w64))))
        assert below >= 0.10, "fewer than 10 % of the hair pixels have a weight below the cap"
        assert distinct >= 30, "fewer than 30 distinct weights"
        assert EDGE_MARGIN >= 4 * ab_err, "the bin-edge margin does not cover the float32 run's Lab error"
        assert torch.equal(w32.double(), w64), "a pixel changes its bin between the float32 and the float64 run"
        assert share <= EXCLUDE_CAP, "too many pixels near a sign change"
        assert bool((w64[~on_hair] == 1).all()) and float(w64.min()) > 0
        if tag == "ii":
            assert float(g64[:, :, 40:48, 24:32].abs().max()) == 0.0 and not bool(ex[:, 40:48, 24:32].any())
        np.savez_compressed(os.path.join(OUT, "lab_balance_%s.npz" % tag), fake=fake.numpy(), real=real.numpy(), hair=hair.numpy().astype(np.uint8),
                            back=(1 - hair).numpy().astype(np.uint8), S=S.numpy(), th=np.array(th), weights=np.array(WEIGHTS),
                            losses=l64.numpy(), grad=g64.numpy(), w=w64.numpy().astype(np.float32), excluded=ex.numpy(),
                            ref32_loss_rel=err_loss, ref32_grad_rel_l2=np.array(err_grad), ref32_grad_max_over_largest=np.array(err_grad_max),
                            ref32_ab_err=np.array(ab_err), edge_margin=np.array(EDGE_MARGIN), exclude_below=np.array(EXCLUDE_BELOW),
                            below_cap=np.array(below), distinct_weights=np.array(distinct))


def hair_inputs(npy):
    """Three samples: the reference hair of samples 0 and 1 has a tinted mean colour whose bin has a weight below the cap of 10, sample 2
    has an EMPTY reference mask (its mean is exactly 0: bin 128, 128)."""
    import hair_lab_fixtures as HE
    g = torch.Generator().manual_seed(2027)
    n = 3

    def image(shift, amp):
        x = amp * (torch.rand(n, 3, H, W, generator=g) * 2 - 1) + torch.tensor(shift).view(n, 3, 1, 1)
        return x.clamp(-1, 1)
    fake = image([(0.4, -0.3, -0.2), (-0.3, 0.35, 0.3), (0.1, 0.3, -0.4)], 0.5)
    ref = image([(0.05, -0.12, -0.30), (0.30, 0.05, -0.15), (-0.3, 0.2, 0.3)], 0.1)          # brown-ish hair colours, little noise
    m_f = torch.stack([HE._ellipse(30, 40, 40, 28), HE._ellipse(36, 36, 42, 22), HE._ellipse(48, 40, 30, 26)])
    m_f[2, 40:44] *= 0.5                                                                     # "the mask value multiplies"
    m_r = torch.stack([HE._ellipse(52, 44, 24, 30), HE._ellipse(40, 40, 30, 30), torch.zeros(H, W)])
    return dict(fake=fake, ref=ref, m_f=m_f, m_r=m_r)


def hair_run(npy, th, p, dtype):
    cls = _hair_cls(npy, th, dtype)
    f = p["fake"].to(dtype).clone().requires_grad_(True)
    loss = cls(f, p["ref"].to(dtype), p["m_f"].to(dtype).unsqueeze(1), p["m_r"].to(dtype).unsqueeze(1))
    loss.backward()
    with torch.no_grad():
        avg = lambda x, m: cls.cal_hair_avg(cls.xyz2lab(cls.rgb2xyz((x + 1) / 2)), m.to(dtype).unsqueeze(1).clone())
        ref_avg = avg(p["ref"].to(dtype), p["m_r"])
        d = (avg(f, p["m_f"]) - ref_avg)[:, 1:, 0, 0]
        w = cls.cal_weight(ref_avg)[:, 0, 0, 0]
    return loss.detach(), f.grad.detach(), (d[:, 0], d[:, 1]), w.detach(), ref_avg[:, 1:, 0, 0].detach()


def make_hair(npy):
    p = hair_inputs(npy)
    S = reference_table(npy, HAIR_TH)
    l64, g64, (da, db), w64, mean64 = hair_run(npy, HAIR_TH, p, torch.float64)
    l32, g32, _, w32, mean32 = hair_run(npy, HAIR_TH, p, torch.float32)
    rounded = dict(p, fake=p["fake"].to(torch.bfloat16).float())
    _, _, (da16, db16), _, _ = hair_run(npy, HAIR_TH, rounded, torch.float64)
    edge = (mean64 + 128 - (mean64 + 128).round()).abs()
    err_grad = float((g32.double() - g64).norm() / g64.norm())
    print("hair (th %g): loss %.8f | reference means + 128 %s | distance to a bin edge %s | weights %s | da %s db %s | fp32 reference: loss rel "
          "%.2e, grad rel L2 %.2e" % (HAIR_TH, float(l64), (mean64 + 128).numpy().round(3).tolist(), edge.numpy().round(3).tolist(), w64.numpy().tolist(),
                                      da.numpy(), db.numpy(), abs(float(l32) - float(l64)) / float(l64), err_grad))
    assert float(p["m_r"][2].sum()) == 0 and bool((mean64[2] == 0).all()), "sample 2: an empty reference mask, its mean exactly 0"
    assert float(edge[:2].min()) >= HAIR_EDGE_MARGIN, "a reference mean is within 0.01 of a bin edge"
    assert torch.equal(w32.double(), w64) and int(torch.unique(w64).numel()) == 3, "three different weights, the same in both precisions"
    assert bool((w64[:2] < 10).all()), "samples 0 and 1 sit on bins below the default cap"
    for t in (da, db, da16, db16):
        assert float(t.abs().min()) >= 1.0, "a per-sample mean difference is too close to the discontinuity of sign()"
    assert torch.equal(torch.sign(da), torch.sign(da16)) and torch.equal(torch.sign(db), torch.sign(db16))
    np.savez_compressed(os.path.join(OUT, "lab_balance_hair.npz"), S=S.numpy(), th=np.array(HAIR_TH), loss=l64.numpy(), grad=g64.numpy(),
                        da=da.numpy(), db=db.numpy(), w=w64.numpy().astype(np.float32), ref_mean=mean64.numpy(),
                        ref32_loss_rel=np.array(abs(float(l32) - float(l64)) / float(l64)), ref32_grad_rel_l2=np.array(err_grad),
                        **{k: v.numpy() for k, v in p.items()})


def make_trainer(npy):
    import lab_balance_fixtures as LB
    from oracle import ref_harness as R
    from oracle import trainer_parity as TP
    R.setup()
    from trainers.pix2pix_trainer import Pix2PixTrainer
    cfg = dict(TP.CFGS["A"], tag="L")
    with tempfile.TemporaryDirectory() as ck:
        opt = R.reference_options(LB.balance_argv(cfg, ck, npy), train=True)
        assert opt.balance_Lab and not opt.no_lab_loss and opt.Lab_weight_th == 10.0 and opt.weight_dir == npy
        torch.manual_seed(0)
        trainer = Pix2PixTrainer(opt)
        trainer.pix2pix_model_on_one_gpu.criterionLabL1.FloatTensor = torch.FloatTensor
        TP.load_weights(trainer, cfg)
        rec = LB.drive_with_lab(trainer, cfg)
    weights = {k: v for k, v in rec.items() if k.startswith(("G.", "D."))}
    np.savez_compressed(os.path.join(OUT, "trainer_L.npz"), **{k: v for k, v in rec.items() if k not in weights})
    np.savez_compressed(os.path.join(OUT, "trainer_L_weights.npz"), **weights)
    with open(os.path.join(OUT, "trainer_lab_balance_config.json"), "w") as fh:
        json.dump({"L": dict(cfg, lambda_lab=opt.lambda_lab, Lab_weight_th=opt.Lab_weight_th, weight_dir="ab_count.npz",
                             flags_removed=["--no_lab_loss"], flags_added=["--balance_Lab", "--weight_dir"])}, fh)
    print("trainer golden L", {k: float(v) for k, v in rec.items() if ".loss." in k})


if __name__ == "__main__":
    _shim_rsub()
    npy = os.path.join(reference_root(), "data", "ab_count.npy")
    raw = np.load(npy)
    assert raw.shape == (256, 256) and raw.dtype == np.float64 and bool(np.isfinite(raw).all()) and raw.min() >= 0
    np.savez_compressed(os.path.join(OUT, "ab_count.npz"), ab_count=raw)
    scan_rgb_cube(npy)
    what = sys.argv[1:] or ["color", "hair", "trainer"]
    if "color" in what:
        make_color(npy)
    if "hair" in what:
        make_hair(npy)
    if "trainer" in what:
        make_trainer(npy)
    for fn in sorted(os.listdir(OUT)):
        if fn.startswith(("lab_balance", "ab_count", "trainer_L", "trainer_lab_balance")):
            size = os.path.getsize(os.path.join(OUT, fn))
            assert size <= 1 << 20, (fn, size)
            print("%8d  %s" % (size, fn))
