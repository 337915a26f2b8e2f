"""Generate the fixtures of dense orientation extraction by running the REFERENCE's own cal_orientation module:

    python tools/make_dense_orient_golden.py        (where the reference checkout is; CPU, seconds)

  tests/golden/dense_orient_i.npz    seeded strand images (tests/dense_orient_fixtures.make_sets: N = 2 at 17x17, 33x47 and 70x95 under an
        elliptical mask; the fixture holds RESULTS only, the images are regenerated from their seed)
  tests/golden/dense_orient_ii.npz   the 128 x 128 crop at row 206, column 72 of the bundled sample 67172 (image and label; the
        pixels are fixture data)

What runs: the module's DoG_fn and orient().calOrientation (cal_orientation.py:18-80) as imported, and the lines of its script part
from `cal_orient = orient()` to the float map `orient_np` (96-109), read from the reference's file and executed here -- not restated --
once in fp32 (what the script does) and once in float64 on the same fp32 image (the oracle the tests compare against).  The only
change to the imported code is the `F` it sees: conv2d casts the filter, which DoG_fn ends with `.float()`, to the image's dtype,
so that the float64 run convolves in float64; and the index calOrientation returns as fp32 is cast before the script's lines
101-109 use it.  scipy.ndimage.gaussian_filter(sigma 4, mode "mirror", truncate 4.0) stands in for cv2.GaussianBlur(src, (0, 0), 4):
the same 33 taps and the same border (BORDER_REFLECT_101); OpenCV is not installed, so the cv2 leg itself is not pinned.

Per geometry "<h>x<w>/": idx (u8), conf (float64), level (the float map before np.uint8), u8, magnitude (hypot of the smoothed flow)
of the float64 run, u8_fp32 of the fp32 run.  Per set: bank (DoG_fn's 32 kernels), bank_maxabs_diff (ops.dog_bank against it),
magnitude_max, and the reference's own fp32-vs-float64 gaps: ref32_level_gap (largest circular level difference of the float map
over the compared pixels), ref32_unequal_bytes, ref32_argmax_flips (shares).

Asserted here, so that no test needs an exclusion list: the acceptance conditions for the reference alone (its fp32 run against its
float64 run), that the float64 contract of mg_orient_smooth passes rule 2 on both sets, and that every mutant of
tests/dense_orient_fixtures.MUTANTS fails it.
"""
import math
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden")


def reference_module():
    """The reference's cal_orientation module (its top level only builds an argument parser), with cv2 / torchvision / matplotlib
    stubbed where they are missing."""
    from oracle import ref_harness as R
    R.setup()
    for name in ("matplotlib", "matplotlib.pyplot"):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    if R.reference_path() not in sys.path:
        sys.path.insert(0, R.reference_path())
    import cal_orientation as CO
    import torch.nn.functional as F

    class _F:
        @staticmethod
        def conv2d(image, kernel, **kw):
            return F.conv2d(image, kernel.to(image.dtype), **kw)
    CO.F = _F
    return CO


def reference_bank(CO):
    """The 32 kernels calOrientation builds (cal_orientation.py:63-66), fp32 [32,17,17]"""
    ks = []
    for k in range(32):
        theta = torch.nn.Parameter(torch.ones(1) * (math.pi * k / 32), requires_grad=False)
        ks.append(CO.DoG_fn(17, 1, 1, theta).float()[0, 0])
    return torch.stack(ks)


def script_part(CO):
    """The reference's own script lines, read from its file where this tool runs (none of them is restated here): (lines from
    `cal_orient = orient()` through the calOrientation call, lines 101-109 up to the float map `orient_np`)."""
    import textwrap
    with open(CO.__file__) as fh:
        src = fh.read().splitlines()
    at = lambda needle: next(i for i, line in enumerate(src) if needle in line and not line.lstrip().startswith("#"))
    first, split, last = at("cal_orient = orient()"), at("cal_orient.calOrientation(gray)"), at("orient_save = Image.fromarray")
    assert first < split < last
    return textwrap.dedent("\n".join(src[first:split + 1])), textwrap.dedent("\n".join(src[split + 1:last]))


def reference_run(CO, image_u8, mask, dtype):
    """One sample: image_u8 [H,W,3], mask [H,W] in {0, 1} -> dict(idx, conf, level, u8, magnitude) with the arithmetic in `dtype`:
    the reference's script lines executed on image_tensor = ToTensor + Normalize(0.5, 0.5) of the image (fp32, then cast)."""
    from scipy.ndimage import gaussian_filter
    import dense_orient_fixtures as DE
    cv2 = types.SimpleNamespace(GaussianBlur=lambda a, ksize, sigma: gaussian_filter(a, sigma=sigma, mode="mirror", truncate=4.0))
    assert ksize_free(cv2)
    mask = np.array(mask)
    assert mask.max() <= 1                                                 # the > 130 rule of lines 91-92 does not apply to these masks
    head, tail = script_part(CO)
    ns = dict(vars(CO), cv2=cv2, mask=mask, image_tensor=torch.unsqueeze(DE.image_fp32(image_u8).permute(2, 0, 1), 0).to(dtype))
    exec(head, ns)
    idx, conf = ns["orient_tensor"].squeeze().numpy().astype(np.uint8), ns["confidence_tensor"].squeeze().numpy()
    ns["orient_tensor"] = ns["orient_tensor"].to(dtype)                   # calOrientation returns the index as fp32 whatever the image is
    exec(tail, ns)
    magnitude = np.hypot(ns["flow_x"].numpy().astype(np.float64), ns["flow_y"].numpy().astype(np.float64))
    orient_np = ns["orient_np"]
    return dict(idx=idx, conf=conf, level=np.asarray(orient_np, np.float64), u8=np.uint8(orient_np), magnitude=magnitude)


def ksize_free(cv2):
    """the stand-in is called as the script calls it: (array, (0, 0), 4) -- sigma 4, the kernel size left to the library"""
    return cv2.GaussianBlur(np.zeros((40, 40), np.float32), (0, 0), 4).shape == (40, 40)


def crop_of_sample():
    from PIL import Image
    import dense_orient_fixtures as DE
    from oracle import ref_harness as R
    r, c, s = DE.CROP
    root = os.path.join(R.REFERENCE_ROOT, "datasets", "FFHQ_demo")
    image = np.array(Image.open(os.path.join(root, "images", "67172.jpg")).convert("RGB"))[r:r + s, c:c + s]
    label = np.array(Image.open(os.path.join(root, "labels", "67172.png")))[r:r + s, c:c + s]
    return {"%dx%d" % (s, s): dict(image=torch.from_numpy(image.copy())[None], mask=torch.from_numpy(label.copy())[None])}


def make_set(CO, tag, geometries, bank, store_pixels):
    import dense_orient_fixtures as DE
    from michigan_amd import ops
    rec = {"bank": bank.numpy(), "bank_maxabs_diff": np.array(float((ops.dog_bank() - bank).abs().max()))}
    runs = {}
    for geo, p in geometries.items():
        n = p["image"].shape[0]
        r64 = [reference_run(CO, p["image"][i], p["mask"][i].numpy(), torch.float64) for i in range(n)]
        r32 = [reference_run(CO, p["image"][i], p["mask"][i].numpy(), torch.float32) for i in range(n)]
        stack = lambda rs, k: np.stack([r[k] for r in rs])
        runs[geo] = (r64, r32)
        rec.update({geo + "/idx": stack(r64, "idx"), geo + "/conf": stack(r64, "conf"), geo + "/level": stack(r64, "level"),
                    geo + "/u8": stack(r64, "u8"), geo + "/magnitude": stack(r64, "magnitude").astype(np.float32),
                    geo + "/u8_fp32": stack(r32, "u8")})
        if store_pixels:
            rec.update({geo + "/image": p["image"].numpy(), geo + "/mask": p["mask"].numpy().astype(np.uint8)})
    masks = {geo: geometries[geo]["mask"].numpy() != 0 for geo in geometries}
    rec["magnitude_max"] = np.array(max(float(rec[geo + "/magnitude"][masks[geo]].max()) for geo in geometries))
    # the reference's own fp32-vs-float64 gaps under the comparison rule
    d8, dl, flips, pixels, excluded, inmask = [], [], 0, 0, 0, 0
    for geo, (r64, r32) in runs.items():
        keep, ex, im = DE.compared(masks[geo], rec[geo + "/magnitude"], float(rec["magnitude_max"]))
        excluded, inmask = excluded + ex, inmask + im
        d8.append(DE.circular(np.stack([r["u8"] for r in r32])[keep], rec[geo + "/u8"][keep]))
        dl.append(DE.circular(np.stack([r["level"] for r in r32])[keep], rec[geo + "/level"][keep]))
        flips += int((np.stack([r["idx"] for r in r32]) != rec[geo + "/idx"]).sum())
        pixels += rec[geo + "/idx"].size
    d8, dl = np.concatenate(d8), np.concatenate(dl)
    rec.update(ref32_level_gap=np.array(float(dl.max())), ref32_unequal_bytes=np.array(float((d8 != 0).mean())),
               ref32_argmax_flips=np.array(flips / pixels))
    rel_min = min(float((rec[geo + "/magnitude"][masks[geo]]).min()) for geo in geometries) / float(rec["magnitude_max"])
    print("set %s: %d in-mask pixels, %d excluded, smallest relative magnitude %.3g | reference fp32 vs float64: level gap %.3g, unequal bytes %.3g %%, "
          "largest byte difference %g, arg-max flips %.3g | bank max abs diff %.3g"
          % (tag, inmask, excluded, rel_min, dl.max(), 100 * (d8 != 0).mean(), d8.max(), flips / pixels, rec["bank_maxabs_diff"]))
    # acceptance, for the reference alone
    assert excluded / inmask <= DE.MAX_EXCLUDED
    assert (d8 == 0).mean() >= 0.995 and d8.max() <= 1, "the reference's fp32 run misses rule 2 against its float64 run: choose another window"
    assert flips / pixels < 1e-3
    path = os.path.join(OUT, "dense_orient_%s.npz" % tag)
    np.savez_compressed(path, **rec)
    fixture = DE.load_set(tag)
    ok, fig = DE.rule2(DE.contract_on_fixture(fixture), fixture)
    print("  contract on the reference's idx / conf:", fig)
    assert ok, "the float64 contract misses rule 2"
    for mutant in DE.MUTANTS:
        ok, fig = DE.rule2(DE.contract_on_fixture(fixture, mutant), fixture)
        print("  mutant %-28s %s %s" % (mutant, "PASSES" if ok else "fails", {k: fig[k] for k in ("equal", "within1", "angle_gap", "outside_unequal")}))
        assert not ok, "the set does not reject the mutant %s" % mutant
    return path


if __name__ == "__main__":
    import dense_orient_fixtures as DE
    CO = reference_module()
    bank = reference_bank(CO)
    paths = [make_set(CO, "i", DE.make_sets()["i"], bank, store_pixels=False), make_set(CO, "ii", crop_of_sample(), bank, store_pixels=True)]
    for p in paths:
        size = os.path.getsize(p)
        assert size < 1 << 20, (p, size)
        print("%8d  %s" % (size, os.path.basename(p)))
