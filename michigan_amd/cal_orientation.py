"""python -m michigan_amd.cal_orientation --image_path IMG --hairmask_path MASK --orientation_root DIR

The reference's cal_orientation.py (its three arguments, its output name <stem>.png) on the device: inputs.dense_orientation, two
kernel launches per batch.  --image_path may also be a directory; then --hairmask_path is the directory of the equally named .png
masks, and the files are processed in batches of images of equal size.  Decoding and encoding use PIL only.
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch
from PIL import Image

from . import inputs

IMAGE_SUFFIXES = (".jpg", ".jpeg", ".png")


def _pairs(image_path: str, hairmask_path: str):
    """[(image file, mask file)]: one pair, or every image of a directory with the .png of the same stem in the mask directory."""
    if not os.path.isdir(image_path):
        return [(image_path, hairmask_path)]
    if not os.path.isdir(hairmask_path):
        raise ValueError("--image_path is a directory: --hairmask_path must be the directory of the equally named .png masks")
    names = sorted(f for f in os.listdir(image_path) if f.lower().endswith(IMAGE_SUFFIXES))
    pairs = [(os.path.join(image_path, f), os.path.join(hairmask_path, os.path.splitext(f)[0] + ".png")) for f in names]
    missing = [m for _, m in pairs if not os.path.exists(m)]
    if missing:
        raise FileNotFoundError("no hair mask for: %s" % ", ".join(missing))
    return pairs


def _load(image_file: str, mask_file: str):
    image = np.array(Image.open(image_file).convert("RGB"))
    mask = np.array(Image.open(mask_file))
    if mask.ndim == 3:
        mask = mask[..., 0]
    if mask.shape != image.shape[:2]:
        raise ValueError("%s is %s, its mask %s is %s" % (image_file, image.shape[:2], mask_file, mask.shape))
    return torch.from_numpy(image), torch.from_numpy(mask.astype(np.int32))


def run(image_path: str, hairmask_path: str, orientation_root: str, device=None, batch_size: int = 8):
    """Writes <orientation_root>/<stem>.png for every pair; returns the files written."""
    device = torch.device(device if device is not None else "cuda")
    os.makedirs(orientation_root, exist_ok=True)
    written, batch = [], []

    def flush():
        if not batch:
            return
        image = torch.stack([b[1] for b in batch]).to(device)
        # the threshold rule is per file (cal_orientation.py:91-92), so it is applied before the masks of a batch are stacked
        mask = torch.stack([((b[2] > 130) if int(b[2].max()) > 1 else (b[2] != 0)).to(torch.uint8) for b in batch]).to(device)
        orient = inputs.dense_orientation(image, mask).cpu().numpy()
        for (image_file, _, _), o in zip(batch, orient):
            out = os.path.join(orientation_root, os.path.splitext(os.path.basename(image_file))[0] + ".png")
            Image.fromarray(o).save(out)
            written.append(out)
        batch.clear()

    for image_file, mask_file in _pairs(image_path, hairmask_path):
        image, mask = _load(image_file, mask_file)
        if batch and (len(batch) == batch_size or batch[0][1].shape != image.shape):
            flush()
        batch.append((image_file, image, mask))
    flush()
    return written


def main(argv=None):
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--image_path", type=str, default="56000.jpg", help="Path to image, or a directory of images")
    parser.add_argument("--hairmask_path", type=str, default="56000.png", help="Path to hair mask, or the directory of the masks")
    parser.add_argument("--orientation_root", type=str, default="./", help="Root to save hair orientation map")
    parser.add_argument("--device", type=str, default="cuda", help="Device the kernels run on")
    args = parser.parse_args(argv)
    for out in run(args.image_path, args.hairmask_path, args.orientation_root, device=args.device):
        print(out)


if __name__ == "__main__":
    main()
