"""Tiny dataset directories for the resident dataset and the two drivers (tests/test_data_resident.py, test_train_driver.py,
test_gpu_train_driver.py; tools/make_dataset_golden.py writes the SAME listing directory for the reference's own CustomDataset).

Everything is written with Pillow from a seeded numpy generator: labels in {0, 1}, PNG maps `<stem>.png` / `<stem>_orient_dense.png`, and
images as PNG bytes (lossless decode) -- under a `.jpg` name where the inference loader asks for one: Pillow opens by content."""
import argparse
import os
import sys

import numpy as np
from PIL import Image

SIZE = 24                                                   # stored size of every map and image
LISTING_STEMS = ("2", "10", "1a", "img_007", "img_12", "0007")
LISTING_CASES = ("walk", "files_list", "max_dataset_size")


def sample(seed, size=SIZE):
    """(label u8 in {0, 1} with a filled disc, orientation u8 under it, image u8 RGB)"""
    r = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:size, 0:size]
    cy, cx = size / 2 + r.uniform(-size / 8, size / 8, size=2)
    label = ((yy - cy) ** 2 + (xx - cx) ** 2 <= (size * r.uniform(0.25, 0.4)) ** 2).astype(np.uint8)
    orient = (r.integers(0, 256, size=(size, size)) * label).astype(np.uint8)
    image = r.integers(0, 256, size=(size, size, 3)).astype(np.uint8)
    return label, orient, image


def save(path, arr):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(arr).save(path, format="PNG")


def write_dataset(root, stems, seed=0, subset="train", image_ext=".png", ext=".png"):
    """<root>/<subset>_{labels,images,dense_orients}/ for `stems`; returns [(label, orient, image)] in the order of `stems`"""
    out = []
    for i, stem in enumerate(stems):
        label, orient, image = sample(1000 * seed + i)
        save(os.path.join(root, subset + "_labels", stem + ext), label)
        save(os.path.join(root, subset + "_dense_orients", stem + "_orient_dense" + ext), orient)
        save(os.path.join(root, subset + "_images", stem + image_ext), image)
        out.append((label, orient, image))
    return out


def dataset_options(root, **over):
    """the loader's option keys with the reference's defaults (data/custom_dataset.py:30-39, options/base_options.py)"""
    d = dict(data_dir=str(root), clear="", label_dir="train_labels", image_dir="train_images", orient_dir="train_dense_orients",
             instance_dir="", max_dataset_size=sys.maxsize, no_pairing_check=False, no_instance=True, no_orientation=False)
    d.update(over)
    return argparse.Namespace(**d)


def write_listing_dir(root, case):
    """The directory of listing case `case`; returns the option overrides that go with it.  Beside the six stems: `3.PNG` (an upper-case
    extension that IS in IMG_EXTENSIONS), `9.Png` (one that is not: the match is case-sensitive) and `notes.txt`."""
    write_dataset(root, LISTING_STEMS, seed=7)
    write_dataset(root, ("3",), seed=8, ext=".PNG", image_ext=".PNG")
    write_dataset(root, ("9",), seed=9, ext=".Png", image_ext=".Png")
    for d in ("train_labels", "train_images", "train_dense_orients"):
        with open(os.path.join(root, d, "notes.txt"), "w") as f:
            f.write("not an image\n")
    if case == "files_list":                       # read instead of walking: a subset, out of order; `9.Png` is listed, so it is taken
        for d, suffix in (("train_labels", ""), ("train_images", ""), ("train_dense_orients", "_orient_dense")):
            with open(os.path.join(root, d, "files.list"), "w") as f:
                for stem, ext in (("img_12", ".png"), ("9", ".Png"), ("10", ".png"), ("0007", ".png"), ("2", ".png")):
                    f.write("%s\n" % os.path.join(root, d, stem + suffix + ext))
    return dict(max_dataset_size=4) if case == "max_dataset_size" else {}


def small_argv(root, ck, name, *extra):
    """the drivers' command line for the configuration of the emulator trainer tests -- dict(TP.CFGS["A"], ngf=8, ndf=8, crop=64): the
    README training flags without the in-painting net and without the Lab term -- at crop 64 / load 72, the smallest geometry the
    generator accepts at num_upsampling_layers='more'"""
    from oracle.ref_harness import README_TRAIN_FLAGS
    return ["--name", name, "--data_dir", str(root), "--checkpoints_dir", str(ck), "--ngf", "8", "--ndf", "8", "--crop_size", "64",
            "--load_size", "72"] + list(README_TRAIN_FLAGS) + [str(a) for a in extra]


def tensor2im_reference(x):
    """util.tensor2im (util/util.py:87-95) as the reference computes it: numpy, fp32, NCHW -> uint8 NHWC"""
    a = x.detach().cpu().float().numpy()
    a = np.clip((np.transpose(a, (0, 2, 3, 1)) + 1) / 2.0 * 255.0, 0, 255)
    return a.astype(np.uint8)


def names(paths):
    return {k: [os.path.basename(p) for p in v] for k, v in paths.items()}
