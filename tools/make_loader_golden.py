"""Generate the fixtures of the device loaders by running the REFERENCE's own loader functions:

    python tools/make_loader_golden.py        (where the reference checkout is; CPU, a few seconds)

  tests/golden/loader_unpaired.npz    Pix2pixDataset.__getitem__ (data/pix2pix_dataset.py:66-194) of a CustomDataset with step = 2
  tests/golden/loader_inference.npz   single_inference_dataLoad (data/base_dataset.py:49-160), each hole rule with and without add_zeros
  tests/golden/loader_demo.npz        demo_inference_dataLoad (:162-276), with and without strokes

What runs: the reference's `data` package as imported, on a tiny dataset written into a temporary directory -- PNG maps, and
images saved losslessly (PNG bytes, under the `.jpg` names the inference loader asks for: Pillow opens by content).  Stubbed from the
outside, as oracle/ref_harness.py does for every fixture: torchvision.transforms (Compose, Lambda, Resize through PIL.Image.resize,
ToTensor, Normalize), cv2.resize (oracle.inputs_oracle.cv2_resize_linear: the `noise` leg stays unpinned), matplotlib (a missing
module), np.float.  The `random` module's randint / random / uniform and np.random.normal are wrapped to RECORD what the functions drew;
they are seeded, never replaced.  Nothing of the reference is restated here.

Geometry: maps and images of the target 40 x 36 (H x W), of the reference sample 36 x 40, load_size 32, crop_size 24, add_th 8,
batch 2 = two runs of the single-sample function.  Per case "<case>/": src/<name> the decoded bytes ([2,...] u8), draws/{x,y,flip}
the get_params draws, draws/{th,centre,nums,u} generate_hole's (u = (centre + 0.5) / nums: the uniform that mg_generate_hole_u8 turns
into that centre), fields the np.random.normal draws of generate_noise back to back, want/<key> the returned tensors.

Asserted here: the seed of the unpaired case draws a reference sample of the OTHER size for both items, an orientation mask of the
target's size (generate_hole combines the two at their stored size), a flipped and an unflipped item, and x != y windows; every pixel
of the demo's strokes is decided by the rule of tests/stroke_fixtures (float64 top-two gap >= tau, or all responses below -tau),
so that the reference's fp32 picture is the only one any arithmetic within tau can return.
"""
import argparse
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch
from PIL import Image, ImageDraw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "tests", "golden")

from make_stroke_golden import save_npz  # noqa: E402

TAG_HW, REF_HW = (40, 36), (36, 40)
LOAD, CROP, ADD_TH, LABEL_NC = 32, 24, 8, 2


def reference_data():
    """data.base_dataset / data.custom_dataset of the reference, and ui_util.cal_orient_stroke for the demo's stroke picture"""
    from oracle import ref_harness as R
    R.setup()
    for name in ("matplotlib", "matplotlib.pyplot"):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    import data.base_dataset as bd
    import data.custom_dataset as cd
    import ui_util.cal_orient_stroke as cs
    return bd, cd, cs


class Draws:
    """records what the reference draws from `random` and np.random.normal while it runs; the generators themselves are untouched"""

    def __init__(self):
        self.log, self.fields = [], []

    def __enter__(self):
        self.saved = (random.randint, random.random, random.uniform, np.random.normal)

        def wrap(kind, fn):
            def call(*a, **k):
                v = fn(*a, **k)
                self.log.append((kind, v))
                return v
            return call

        def normal(*a, **k):
            f = self.saved[3](*a, **k)
            self.fields.append(np.asarray(f, np.float64).reshape(-1))
            return f
        random.randint, random.random, random.uniform = (wrap(k, f) for k, f in zip(("randint", "random", "uniform"), self.saved[:3]))
        np.random.normal = normal
        return self

    def __exit__(self, *exc):
        random.randint, random.random, random.uniform, np.random.normal = self.saved

    def take(self):
        log, fields = self.log, np.concatenate(self.fields)
        self.log, self.fields = [], []
        return log, fields


def ellipse(hw, seed):
    h, w = hw
    r = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = h / 2 + r.uniform(-h / 8, h / 8), w / 2 + r.uniform(-w / 8, w / 8)
    return ((((yy - cy) / (h * r.uniform(0.25, 0.4))) ** 2 + ((xx - cx) / (w * r.uniform(0.25, 0.4))) ** 2) <= 1).astype(np.uint8)


def sample(hw, seed, unknown=False):
    """one sample's three files at hw: (label u8 in {0, 1} (a few 255 = 'unknown' when asked), dense orientation u8, image u8 RGB)"""
    r = np.random.RandomState(1000 + seed)
    label = ellipse(hw, seed)
    orient = (r.randint(0, 256, size=hw) * label).astype(np.uint8)
    image = r.randint(0, 256, size=hw + (3,)).astype(np.uint8)
    image[:3, :3], image[3:6, :3] = 255, 0                                 # bicubic overshoot on both sides: clip8
    if unknown:
        label[hw[0] // 2 - 1:hw[0] // 2 + 1, hw[1] // 2 - 1:hw[1] // 2 + 2] = 255                # inside every crop window
    return label, orient, image


def save(path, arr):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(arr).save(path, format="PNG")
    assert np.array_equal(np.array(Image.open(path)), arr)


def hole_draws(log, orient_mask):
    """(th, centre, nums, u) from the two draws generate_hole made (base_dataset.py:343,347)"""
    from oracle import inputs_oracle as IO
    (k0, th), (k1, centre) = log
    assert (k0, k1) == ("uniform", "randint")
    nums = int((orient_mask != 0).sum())
    u = (centre + 0.5) / nums
    assert IO.hole_center_index(u, nums) == centre
    return th, centre, nums, u


def tensors(d, skip=("path",)):
    out = {}
    for k, v in d.items():
        if k in skip:
            continue
        out[k] = (v.numpy() if torch.is_tensor(v) else np.asarray(v))
    return out


def stack_runs(runs):
    """[{name: array}] of the batch's runs -> {name: stacked}; tensors with the loader's own batch dimension are concatenated"""
    out = {}
    for k in runs[0]:
        vs = [r[k] for r in runs]
        out[k] = np.asarray(vs[0]) if np.ndim(vs[0]) == 0 else (np.concatenate(vs) if np.ndim(vs[0]) == 4 else np.stack(vs))
    return out


def put(rec, case, **groups):
    for group, d in groups.items():
        if isinstance(d, dict):
            for k, v in d.items():
                rec["%s/%s/%s" % (case, group, k)] = np.asarray(v)
        else:
            rec["%s/%s" % (case, group)] = np.asarray(d)


# ---- 1. the unpaired stage's batch -------------------------------------------------------------------------------------------------------
def make_unpaired(bd, cd):
    samples = [sample(TAG_HW, 0), sample(TAG_HW, 1), sample(REF_HW, 2, unknown=True), sample(REF_HW, 3, unknown=True)]
    with tempfile.TemporaryDirectory() as root:
        for i, (label, orient, image) in enumerate(samples):
            save(os.path.join(root, "train_labels", "%d.png" % i), label)
            save(os.path.join(root, "train_dense_orients", "%d.png" % i), orient)
            save(os.path.join(root, "train_images", "%d.png" % i), image)
        opt = argparse.Namespace(data_dir=root, clear="", label_dir="train_labels", image_dir="train_images", orient_dir="train_dense_orients",
                                 instance_dir="", max_dataset_size=1 << 30, no_pairing_check=False, no_instance=True, no_orientation=False,
                                 use_ig=True, preprocess_mode="resize_and_crop", load_size=LOAD, crop_size=CROP, isTrain=True, no_flip=False,
                                 color_jitter=False, label_nc=LABEL_NC)
        ds = cd.CustomDataset()
        ds.initialize(opt, step=2)
        assert len(ds) == 4 and [os.path.basename(p) for p in ds.label_paths] == ["%d.png" % i for i in range(4)]
        for seed in range(1000):
            random.seed(seed)
            np.random.seed(seed)
            runs = []
            try:
                with Draws() as dr:
                    for index in (0, 1):
                        d = ds[index]
                        runs.append((d,) + dr.take())
            except ValueError:                                  # generate_hole on masks of two sizes: not a batch this fixture wants
                continue
            logs = [r[1] for r in runs]
            refs, omasks = [l[3][1] for l in logs], [l[4][1] for l in logs]
            flips = [l[2][1] > 0.5 for l in logs]
            if all(r >= 2 for r in refs) and all(o < 2 for o in omasks) and sorted(flips) == [False, True] and all(l[0][1] != l[1][1] for l in logs) \
                    and omasks[0] != 0 and refs[0] != refs[1]:
                break
        else:
            raise AssertionError("no seed below 1000 draws the batch described in the docstring")
    draws = {k: [] for k in ("x", "y", "flip", "index_ref", "index_orient", "th", "centre", "nums", "u")}
    for (d, log, fields), index in zip(runs, (0, 1)):
        assert [k for k, _ in log] == ["randint", "randint", "random", "randint", "randint", "random", "uniform", "randint"], log
        th, centre, nums, u = hole_draws(log[6:], samples[log[4][1]][0])
        for k, v in zip(draws, (log[0][1], log[1][1], log[2][1], log[3][1], log[4][1], th, centre, nums, u)):
            draws[k].append(v)
        assert os.path.basename(d["path"]) == "%d.png" % log[3][1]
    ir, io = draws["index_ref"], draws["index_orient"]
    src = dict(image=np.stack([samples[i][2] for i in (0, 1)]), label=np.stack([samples[i][0] for i in (0, 1)]),
               orient=np.stack([samples[i][1] for i in (0, 1)]), orient_mask=np.stack([samples[i][0] for i in io]),
               image_ref=np.stack([samples[i][2] for i in ir]), label_ref=np.stack([samples[i][0] for i in ir]))
    rec = {"seed": np.array(seed)}
    put(rec, "step2", src=src, draws=draws, fields=np.stack([r[2] for r in runs]), want=stack_runs([tensors(r[0]) for r in runs]))
    print("unpaired: seed %d, draws %s" % (seed, {k: v for k, v in draws.items() if k != "u"}))
    return rec


# ---- 2. single_inference_dataLoad ----------------------------------------------------------------------------------------------------------
def make_inference(bd):
    rec = {}
    for same in (True, False):
        for zeros in (False, True):
            case = "%s_%s" % ("same" if same else "other", "zeros" if zeros else "plain")
            runs, srcs, draws = [], [], {k: [] for k in ("x", "y", "flip", "th", "centre", "nums", "u")}
            for b in range(2):
                base = 10 * b + (4 if same else 0) + (2 if zeros else 0)
                ref, tag, other = sample(REF_HW, 20 + base, unknown=True), sample(TAG_HW, 21 + base), sample(TAG_HW, 22 + base)
                ori = tag if same else other
                with tempfile.TemporaryDirectory() as root:
                    names = dict(ref="r", tag="t", orient="t" if same else "o")
                    for name, s in (("r", ref), ("t", tag), ("o", other)):
                        save(os.path.join(root, "val_labels", name + ".png"), s[0])
                        save(os.path.join(root, "val_dense_orients", name + "_orient_dense.png"), s[1])
                        save(os.path.join(root, "val_images", name + ".jpg"), s[2])
                    opt = argparse.Namespace(data_dir=root, subset="val", inference_ref_name=names["ref"], inference_tag_name=names["tag"],
                                             inference_orient_name=names["orient"], add_zeros=zeros, add_th=ADD_TH, expand_tag_mask=False,
                                             use_ig=True, no_orientation=False, preprocess_mode="resize_and_crop", load_size=LOAD, crop_size=CROP,
                                             isTrain=False, no_flip=False, color_jitter=False, label_nc=LABEL_NC)
                    random.seed(300 + base)
                    np.random.seed(300 + base)
                    with Draws() as dr:
                        d = bd.single_inference_dataLoad(opt)
                        log, fields = dr.take()
                assert [k for k, _ in log] == ["randint", "randint", "random"] + (["uniform", "randint"] if same else []), log
                for k, v in zip(("x", "y", "flip"), (log[0][1], log[1][1], log[2][1])):
                    draws[k].append(v)
                if same:
                    omask = np.pad(ori[0], ((ADD_TH // 2, ADD_TH - ADD_TH // 2),) * 2) if zeros else ori[0]
                    for k, v in zip(("th", "centre", "nums", "u"), hole_draws(log[3:], omask)):
                        draws[k].append(v)
                runs.append(dict(tensors(d), fields=fields))
                srcs.append(dict(image_ref=ref[2], image_tag=tag[2], label_ref=ref[0], label_tag=tag[0], orient_tag=tag[1], orient_ref=ori[1],
                                 orient_mask=ori[0]))
            want = stack_runs(runs)
            put(rec, case, src=stack_runs(srcs), draws={k: v for k, v in draws.items() if v}, fields=want.pop("fields"), want=want)
            assert want["hole"].shape == (2, 1, CROP, CROP) and want["hole"].any() and want["orient_rgb"].any(), case
            print("inference %-12s draws %s" % (case, {k: v for k, v in draws.items() if v and k != "u"}))
    return rec


# ---- 3. demo_inference_dataLoad --------------------------------------------------------------------------------------------------------------
def decided_stroke(hw, b):
    """a stroke mask u8 [H,W] in {0, 1} all of whose pixels the rule of tests/stroke_fixtures decides, found among straight pen lines"""
    import stroke_fixtures as SE
    fx = SE.load_set("i")
    h, w = hw
    best = None
    for k in range(200):
        r = np.random.RandomState(7000 + 1000 * b + k)
        img = Image.new("L", (w, h), 0)
        p = [(int(r.randint(4, w - 4)), int(r.randint(4, h - 4))) for _ in range(2)]
        ImageDraw.Draw(img).line(p, fill=1, width=int(r.randint(1, 6)))
        m = np.array(img)
        if m.sum() < 12:
            continue
        resp = SE.responses(m[None], fx["bank"])[0]                          # float64 [32,H,W]
        c = np.sort(np.maximum(resp, 0), axis=0)
        ok = ((c[-1] - c[-2]) >= fx["tau"]) | (resp.max(axis=0) < -fx["tau"])
        undecided = int((~ok & (m != 0)).sum())
        if best is None or undecided < best[0]:
            best = (undecided, m, k)
        if undecided == 0:
            return m
    raise AssertionError("no fully decided stroke among 200 lines (best: %d undecided pixels, candidate %d)" % (best[0], best[2]))


def make_demo(bd, cs):
    import torch.nn.functional as F
    rec = {}
    for strokes in (False, True):
        case = "strokes" if strokes else "plain"
        runs, srcs, draws = [], [], {k: [] for k in ("x", "y", "flip")}
        for b in range(2):
            base = 10 * b + (5 if strokes else 0)
            ref, tag, other = sample(REF_HW, 60 + base, unknown=True), sample(TAG_HW, 61 + base), sample(TAG_HW, 62 + base)
            src = dict(label_ref=ref[0], label_tag=tag[0], mask_orient=other[0], orient_ref=other[1], image_ref=ref[2], image_tag=tag[2])
            extra = {}
            if strokes:
                m = decided_stroke(TAG_HW, b)
                with torch.no_grad():
                    picture = np.uint8(cs.orient().stroke_to_orient(m))     # demo.py:325-326
                hole = F.max_pool2d(torch.from_numpy(m)[None, None].float(), 5, stride=1, padding=2)[0, 0].numpy().astype(np.uint8)
                assert picture.shape == TAG_HW + (3,) and picture[m != 0].any() and not picture[m == 0].any()
                src.update(mask_stroke=m, mask_hole=hole)
                extra = dict(orient_stroke=picture, mask_stroke=m, mask_hole=hole)
            opt = argparse.Namespace(expand_tag_mask=False, preprocess_mode="resize_and_crop", load_size=LOAD, crop_size=CROP, isTrain=False,
                                     no_flip=False, color_jitter=False, label_nc=LABEL_NC)
            with tempfile.TemporaryDirectory() as root:
                path = os.path.join(root, "ref_label.png")
                save(path, ref[0])
                random.seed(500 + base)
                np.random.seed(500 + base)
                with Draws() as dr:
                    d = bd.demo_inference_dataLoad(opt, path, tag[0], other[0], other[1], Image.fromarray(ref[2]), Image.fromarray(tag[2]), **extra)
                    log, fields = dr.take()
            assert [k for k, _ in log] == ["randint", "randint", "random"], log
            for k, v in zip(("x", "y", "flip"), (log[0][1], log[1][1], log[2][1])):
                draws[k].append(v)
            runs.append(dict(tensors(d), fields=fields))
            srcs.append(src)
        want = stack_runs(runs)
        put(rec, case, src=stack_runs(srcs), draws=draws, fields=want.pop("fields"), want=want)
        if strokes:
            assert want["orient_stroke"].any() and want["mask_stroke"].any(), "the strokes miss the cropped hair region"
        print("demo %-8s draws %s, keys %s" % (case, draws, sorted(want)))
    return rec


if __name__ == "__main__":
    bd, cd, cs = reference_data()
    for name, rec in (("unpaired", make_unpaired(bd, cd)), ("inference", make_inference(bd)), ("demo", make_demo(bd, cs))):
        path = os.path.join(OUT, "loader_%s.npz" % name)
        save_npz(path, rec)
        size = os.path.getsize(path)
        assert size < 1 << 19, (path, size)                 # well under the limit for a committed file
        print("%8d  %s" % (size, os.path.basename(path)))
