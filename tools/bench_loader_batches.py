"""Time one batch of each kind the device loaders build (michigan_amd/inputs.py), at BASELINE configs[4]'s geometry: files stored at
512, load 568 -> crop 512, --use_ig.  CUDA events around the whole call (host draws, table look-ups and uploads included), median of
--iters runs after --warmup.  Informational: the reference's CPU loader was never timed on the same machine, so the lines claim no
speed-up (profiles/loader_batches.txt).

    python tools/bench_loader_batches.py [--iters 20] [--warmup 3] [--out profiles/loader_batches.txt]
"""
import argparse
import os
import random
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from michigan_amd import _cabi, inputs
    from michigan_amd.model import default_options
    assert _cabi.backend().name == "hip"
    size, load, cs = 512, 568, 512
    g = torch.Generator().manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(float(size)), torch.arange(float(size)), indexing="ij")

    def files(n, shift):
        label = ((((yy - 256 - shift) / 150) ** 2 + ((xx - 256 + shift) / 120) ** 2) <= 1).to(torch.uint8).expand(n, size, size).contiguous()
        orient = torch.randint(0, 255, (n, size, size), generator=g).to(torch.uint8) * label
        image = torch.randint(0, 256, (n, size, size, 3), generator=g, dtype=torch.uint8)
        return image.cuda(), label.cuda(), orient.cuda()
    gen = torch.Generator(device="cuda").manual_seed(1)
    image, label, orient = files(8, 0)
    image_r, label_r, _ = files(8, 20)
    pipe = inputs.DeviceInputPipeline(default_options(crop_size=cs, load_size=load, use_ig=True), "cuda", rng=random.Random(1), generator=gen)
    lines = ["unpaired batch of 8 (image_ref / label_ref given), stored 512, load 568 -> crop 512: %.3f ms"
             % timed(lambda: pipe(image, label, orient, label_r, image_ref=image_r, label_ref=label_r), a.iters, a.warmup)]
    one = inputs.DeviceInputPipeline(default_options(crop_size=cs, load_size=load, use_ig=True, isTrain=False, add_zeros=True), "cuda",
                                     rng=random.Random(2), generator=gen)
    i1, l1, o1 = files(1, 0)
    i2, l2, o2 = files(1, 20)
    lines.append("inference batch of 1 (add_zeros 64, same_orient), stored 512, load 568 -> crop 512: %.3f ms" % timed(
        lambda: one.inference_batch(image_ref=i2, image_tag=i1, label_ref=l2, label_tag=l1, orient_tag=o1, orient_ref=o1, orient_mask=l1,
                                    same_orient=True), a.iters, a.warmup))
    stroke = torch.zeros(1, size, size, dtype=torch.uint8)
    stroke[0, 200:206, 150:360] = 1
    hole = torch.zeros_like(stroke)
    hole[0, 190:216, 140:370] = 1
    stroke, hole = stroke.cuda(), hole.cuda()
    lines.append("demo batch of 1 (strokes), stored 512, load 568 -> crop 512: %.3f ms" % timed(
        lambda: one.demo_batch(label_ref=l2, label_tag=l1, mask_orient=l2, orient_ref=o2, image_ref=i2, image_tag=i1, mask_stroke=stroke,
                               mask_hole=hole), a.iters, a.warmup))
    text = "".join("%s  (CUDA events, median of %d after %d warm-up runs)\n" % (l, a.iters, a.warmup) for l in lines)
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
