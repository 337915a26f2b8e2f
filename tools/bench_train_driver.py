"""What the dataset layer costs on top of the training step, in ONE process on one GPU:

    python tools/bench_train_driver.py [--samples 64 --size 512 --batch 8 --iters 30 --warmup 5] > profiles/train_driver.txt

  1  writes a synthetic dataset (PNG labels / orientations / images at --size) into a temporary directory;
  2  runs the reference README's training configuration (use_ig with the frozen in-painting net from a seeded file, the Lab term on) in bf16
     through michigan_amd.train.train() and times --iters iterations after --warmup (the device drained at both ends of the window);
  3  runs a trainer of the same options on synth.synth_batch for the same counts, TWICE: the yardstick (the step without any loader) and,
     from the spread of its two repeats, the margin.
Reported: images/s of each leg, decode time and resident bytes, host time and device time per batch() call (HIP events around the call: the
host_phases.py-style split of the loader's share of a step), and the gap between the dataset leg and the yardstick against that margin.
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_dataset(root, m, size, seed=0):
    from PIL import Image
    r = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:size, 0:size]
    for i in range(m):
        cy, cx = size / 2 + r.uniform(-size / 16, size / 16, size=2)
        ry, rx = size * r.uniform(100, 180, size=2) / 512
        label = ((((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2) <= 1).astype(np.uint8)
        orient = (r.integers(0, 256, size=(size, size)) * label).astype(np.uint8)
        image = r.integers(0, 256, size=(size, size, 3), dtype=np.uint8)
        for sub, name, arr in (("train_labels", "%05d.png", label), ("train_dense_orients", "%05d_orient_dense.png", orient),
                               ("train_images", "%05d.png", image)):
            os.makedirs(os.path.join(root, sub), exist_ok=True)
            Image.fromarray(arr).save(os.path.join(root, sub, name % i), format="PNG", compress_level=1)


class Timed:
    """an EpochLoader behind a stopwatch: host and device time of every batch() call, and the wall clock (device drained) at the two
    ends of the timed window"""

    def __init__(self, loader, warmup, iters):
        self.loader, self.warmup, self.iters = loader, warmup, iters
        self.count, self.host, self.events, self.t0, self.t1 = 0, [], [], None, None

    def __len__(self):
        return len(self.loader)

    def set_epoch(self, e):
        self.loader.set_epoch(e)

    def __iter__(self):
        for index in self.loader.indices():
            if self.count == self.warmup:
                torch.cuda.synchronize()
                self.t0 = time.perf_counter()
            if self.count == self.warmup + self.iters:
                torch.cuda.synchronize()
                self.t1 = time.perf_counter()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            h0 = time.perf_counter()
            a.record()
            data = self.loader.dataset.batch(index)
            b.record()
            self.host.append(time.perf_counter() - h0)
            self.events.append((a, b))
            self.count += 1
            yield data


def synth_leg(trainer, batch, size, warmup, iters):
    from michigan_amd.synth import synth_batch
    data = {k: v.cuda() for k, v in synth_batch(batch, size, seed=1234).items()}
    for it in range(warmup + iters):
        if it == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        trainer.run_generator_one_step(data)
        trainer.run_discriminator_one_step(data)
    torch.cuda.synchronize()
    return batch * iters / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--load", type=int, default=568)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ngf", type=int, default=64)
    a = ap.parse_args()
    from michigan_amd import data as D, networks, train
    from michigan_amd.model import Pix2PixTrainer
    from michigan_amd.synth import synth_state_dict
    per_epoch = a.samples // a.batch
    epochs = -(-(a.warmup + a.iters + 1) // per_epoch)
    with tempfile.TemporaryDirectory() as tmp:
        root, ck = os.path.join(tmp, "data"), os.path.join(tmp, "ck")
        t = time.perf_counter()
        write_dataset(root, a.samples, a.size)
        print("dataset: %d samples at %d x %d written in %.1f s" % (a.samples, a.size, a.size, time.perf_counter() - t))
        argv = ("--name bench --batchSize %d --no_confidence_loss --gpu_ids 0 --no_style_loss --no_rgb_loss --no_content_loss --use_encoder "
                "--wide_edge 2 --no_background_loss --noise_background --random_expand_mask --use_ig --load_size %d --crop_size %d "
                "--compute_dtype bf16 --ngf %d --ndf %d --seed 1 --niter %d --print_freq %d --save_latest_freq %d --save_epoch_freq %d"
                % (a.batch, a.load, a.size, a.ngf, a.ngf, epochs, 1 << 30, 1 << 30, 1 << 30)).split() + ["--data_dir", root, "--checkpoints_dir", ck]
        opt = train.parse(argv)
        # the frozen net's pretrained file is a download: a seeded stand-in of the same shapes
        os.makedirs(os.path.join(ck, "bench"))
        ig = networks.define_IG(opt)
        torch.save({"generator": synth_state_dict({k: v.cpu() for k, v in ig.state_dict().items()}, seed=7)},
                   os.path.join(ck, "bench", opt.ig_model_name))
        del ig
        t = time.perf_counter()
        ds = D.ResidentDataset(opt, torch.device("cuda", 0), resident=opt.resident)
        torch.cuda.synchronize()
        print("decode + upload: %.2f s for %d samples (%d threads), resident %.1f MB = %.2f MB per sample"
              % (time.perf_counter() - t, len(ds), min(D.DECODE_THREADS, len(ds)), ds.nbytes / 1e6, ds.nbytes / 1e6 / len(ds)))
        timed = Timed(D.EpochLoader(ds, a.batch, shuffle=True, drop_last=True, seed=1), a.warmup, a.iters)
        out = train.train(opt, loaders=(timed, None))
        dataset_ips = a.batch * a.iters / (timed.t1 - timed.t0)
        torch.cuda.synchronize()
        host = np.array(timed.host[a.warmup:a.warmup + a.iters]) * 1e3
        dev = np.array([x.elapsed_time(y) for x, y in timed.events[a.warmup:a.warmup + a.iters]])
        print("train() over the dataset: %d iterations in %d epochs, last losses %s" % (out["iterations"], out["epochs"],
                                                                                          {k: round(v, 3) for k, v in out["losses"].items()}))
        torch.manual_seed(1)
        trainer = Pix2PixTrainer(train.parse(argv))
        trainer.pix2pix_model_on_one_gpu.load_inpainting()
        synth = [synth_leg(trainer, a.batch, a.size, a.warmup, a.iters) for _ in range(2)]
    ms = lambda ips: 1e3 * a.batch / ips
    spread = abs(ms(synth[0]) - ms(synth[1]))
    gap = ms(dataset_ips) - min(ms(s) for s in synth)
    print("images/s   dataset leg %.1f (%.2f ms per step)   synthetic-batch leg %.1f and %.1f (%.2f and %.2f ms per step)"
          % (dataset_ips, ms(dataset_ips), synth[0], synth[1], ms(synth[0]), ms(synth[1])))
    print("batch(): host %.3f ms median (%.3f max), device %.3f ms median (%.3f max) per call of %d samples"
          % (np.median(host), host.max(), np.median(dev), dev.max(), a.batch))
    print("gap dataset - synthetic: %.2f ms per step; margin = spread of the two synthetic repeats %.2f ms + the loader's device time %.3f ms = %.2f ms"
          % (gap, spread, np.median(dev), spread + np.median(dev)))
    print("the gap is %s the margin" % ("within" if gap <= spread + np.median(dev) else "BEYOND"))


if __name__ == "__main__":
    main()
