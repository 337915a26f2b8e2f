"""Generate the fixture of the DoG orientation loss by running the REFERENCE's own class:

    python tools/make_orient_dog_golden.py            (where the reference checkout is; CPU, a few seconds)

  tests/golden/orient_dog.npz   one seeded batch at N=2, crop 64: a smooth oriented texture as the generated image, an elliptic hair
        mask per sample, the orientation label as (sin 2t, cos 2t) planes (use_ig) and as the 0..255 angle map (not use_ig); for both,
        the two losses of the reference's L1OLoss(orient_filter='dog') and its d(w_o orient + w_c confidence) / d image, in the
        reference's own fp32.

The reference's DoG branch spells the complement of a boolean mask `1 - mask` (loss.py:343), which raises on today's torch; in THIS
process only Tensor.__rsub__ is wrapped as tools/make_color_loss_golden.py does.  Nothing of the reference is restated here: its class
and its DoG_fn are called.

Asserted, for the reference alone (another SEED if one fails): the batch maximum M is attained once; the reference's fp32 values agree
with the float64 contract of tests/orient_dog_fixtures.py within its scalar rule; at most 0.1 % of the hair pixels have top-two
responses so close that the winner differs between the reference's fp32 filters and a float64 run of the same filters."""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "tests", "golden", "orient_dog.npz")

N, S = 2, 64
SEED = 5
WEIGHTS = (10.0, 100.0)               # lambda_orient, lambda_confidence of the reference's defaults
FLIP_CAP = 0.001


def make_batch(seed):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(S, dtype=torch.float32), torch.arange(S, dtype=torch.float32), indexing="ij")
    imgs, angles, masks = [], [], []
    for n in range(N):
        # strands: a grating of period ~5 pixels whose direction turns slowly across the crop
        t0, bend = float(torch.rand((), generator=g)) * math.pi, 0.6 + 0.4 * float(torch.rand((), generator=g))
        theta = t0 + bend * (xx / S - 0.5) + 0.5 * bend * (yy / S - 0.5)
        phase = 2 * math.pi / 5.0 * (xx * torch.cos(theta) + yy * torch.sin(theta))
        tex = 0.55 * torch.sin(phase) + 0.15 * torch.sin(0.37 * phase + 1.0)
        tint = torch.tensor([0.9, 0.7, 0.5]).view(3, 1, 1) * (0.8 + 0.2 * n)
        imgs.append((tex[None] * tint + 0.02 * torch.randn(3, S, S, generator=g)).clamp(-1, 1))
        angles.append(torch.remainder(theta + 0.3 * torch.sin(xx / 9.0 + n), math.pi))
        cy, cx = 30 + 4 * n, 32 - 3 * n
        masks.append(((((yy - cy) / (22 - 4 * n)) ** 2 + ((xx - cx) / (18 + 5 * n)) ** 2) < 1).float())
    img, ang, m = torch.stack(imgs), torch.stack(angles), torch.stack(masks)
    label_ig = torch.stack([torch.sin(2 * ang), torch.cos(2 * ang)], dim=1)
    label_map = torch.round(ang / math.pi * 255)[:, None]
    return img, label_ig, label_map, m


def reference_run(RL, R, img, label, sem, use_ig):
    crit = RL.L1OLoss(R.make_opt(crop_size=S, orient_filter="dog", use_ig=use_ig))
    x = img.clone().requires_grad_(True)
    lo, lc = crit(x, label, sem)
    (WEIGHTS[0] * lo + WEIGHTS[1] * lc).backward()
    return float(lo.detach()), float(lc.detach()), x.grad.detach()


def main():
    import orient_dog_fixtures as DF
    from make_color_loss_golden import _shim_rsub
    from michigan_amd import ops
    from oracle import ref_harness as R
    R.setup()
    RL = R.losses()
    img, label_ig, label_map, m = make_batch(SEED)
    sem = DF.one_hot(m)
    try:
        reference_run(RL, R, img, label_ig, sem, True)
        raise SystemExit("the reference's DoG branch ran without the shim: this torch is not the one the fixture is for")
    except RuntimeError as e:
        print("unshimmed reference:", str(e).splitlines()[0][:110])
    _shim_rsub()
    # the reference's own bank, and the filters' winners in its fp32 and in float64
    bank = torch.cat([RL.DoG_fn(17, 1, 1, torch.ones(1) * (math.pi * k / 32)).float() for k in range(32)], dim=0)[:, 0]
    assert torch.equal(bank, ops.dog_bank()), "ops.dog_bank() is not the reference's DoG_fn"
    r32, r64 = DF.responses(img, bank), DF.responses(img.double(), bank)
    hair = m > 0
    flips = float((r32.argmax(1) != r64.argmax(1))[hair].double().mean())
    top2 = r64.topk(2, dim=1)[0]
    print("winner flips fp32 / float64 under the hair: %.5f; smallest relative top-two margin there: %.3e"
          % (flips, float(((top2[:, 0] - top2[:, 1]) / top2[:, 0].clamp_min(1e-30))[hair].min())))
    assert flips <= FLIP_CAP
    c1 = r64.max(1)[0] * m
    assert int((c1 == c1.max()).sum()) == 1 and float(c1.max()) > 0, "M is attained more than once"
    rec = dict(img=img.numpy(), label_ig=label_ig.numpy(), label_map=label_map.numpy().astype(np.uint8), hair=m.numpy().astype(np.uint8),
               weights=np.array(WEIGHTS), flips=np.array(flips))
    for tag, label, use_ig in (("ig", label_ig, True), ("map", label_map, False)):
        lo, lc, grad = reference_run(RL, R, img, label, sem, use_ig)
        x = img.double().requires_grad_(True)
        co, cc = DF.l1o_contract(x, label, sem, bank)
        (WEIGHTS[0] * co + WEIGHTS[1] * cc).backward()
        gerr = float((grad.double() - x.grad).abs().max() / x.grad.abs().max())
        print("%s: reference fp32 orient %.8f confidence %.8f | float64 contract %.8f %.8f | image gradient: max err / largest %.2e (largest %.3e)"
              % (tag, lo, lc, float(co), float(cc), gerr, float(x.grad.abs().max())))
        assert DF.scalar_close(lo, co, DF.SCALAR_TOL["f32"]) and DF.scalar_close(lc, cc, DF.SCALAR_TOL["f32"])
        rec.update({"losses_" + tag: np.array([lo, lc]), "grad_" + tag: grad.numpy(), "contract_" + tag: np.array([float(co), float(cc)]),
                    "ref32_grad_max_over_largest_" + tag: np.array(gerr)})
    np.savez_compressed(OUT, **rec)
    size = os.path.getsize(OUT)
    assert size <= 1 << 20, size
    print("%8d  %s" % (size, os.path.relpath(OUT, ROOT)))


if __name__ == "__main__":
    main()
