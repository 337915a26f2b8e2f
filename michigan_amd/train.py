"""`python -m michigan_amd.train`: the reference's train.py on a dataset directory, without a reference checkout.

    python -m michigan_amd.train --name <experiment> --batchSize 8 --no_confidence_loss --gpu_ids 0 --no_style_loss --no_rgb_loss \
        --no_content_loss --use_encoder --wide_edge 2 --no_background_loss --noise_background --random_expand_mask --use_ig \
        --load_size 568 --crop_size 512 --data_dir <dataset> --checkpoints_dir ./checkpoints
    torchrun --nproc-per-node 8 -m michigan_amd.train ... --batchSize 8        # one process per GPU, batchSize / 8 samples each

Options: every key of `model.default_options()` is settable (`--key value`; booleans as `--flag` or `--flag false`), and the reference's
own spellings parse, so its README command works unchanged.  The flags the reference declares as store-true start from the REFERENCE's
default (off), not from default_options()'s fixture-preserving values: the README command trains with the Lab term on, as published.
Everything else keeps default_options()'s value.  `--use_ig` also sets `inpaint_orient`: the frozen in-painting net runs as in the
reference, loaded from its own file by `Pix2PixModel.load_inpainting()`.

The loop is train.py:41-140 statement for statement (see `train`), IterationCounter's arithmetic and `iter.txt` included, so a run can
be resumed by either code base.  No HTML and no visdom: `--display_freq N` (0 = off) writes the first generated sample as a PNG.
The data comes from `data.ResidentDataset` / `data.EpochLoader`: decoded once, resident, one device-pipeline call per batch.
"""
from __future__ import annotations

import argparse
import os
import random as _random
import sys
import time
from typing import List, Optional

import torch

from . import parallel
from .model import Pix2PixTrainer, default_options

# what options/base_options.py and options/train_options.py (and test_options.py, for inference) declare with action='store_true'
REFERENCE_STORE_TRUE = (
    "weight_norm_G", "contain_dontcare_label", "use_ig", "use_instance_feat", "use_encoder", "use_vae", "noise_background",
    "random_expand_mask", "bf_direct_add", "random_noise_background", "use_stroke", "add_feat_zeros", "orient_random_disturb",
    "no_gan_loss", "no_ganFeat_loss", "no_vgg_loss", "no_background_loss", "no_rgb_loss", "no_lab_loss", "no_TTUR", "no_orient_loss",
    "no_confidence_loss", "no_content_loss", "no_style_loss", "remove_background", "balance_Lab", "unpairTrain", "same_netD_model")
REFERENCE_STORE_TRUE_TEST = ("expand_mask_be",)             # test_options.py only: the training value stays default_options()'s
DRIVER_KEYS = ("isTrain", "inpaint_orient", "curr_step")     # set by the drivers, not from the command line


def str2bool(v: str) -> bool:
    if v.lower() in ("yes", "true", "t", "y", "1"):
        return True
    if v.lower() in ("no", "false", "f", "n", "0"):
        return False
    raise argparse.ArgumentTypeError("Boolean value expected.")


def build_parser(is_train: bool = True) -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m michigan_amd." + ("train" if is_train else "inference"),
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    flags = REFERENCE_STORE_TRUE + (() if is_train else REFERENCE_STORE_TRUE_TEST)
    for key, value in vars(default_options()).items():
        if key in DRIVER_KEYS:
            continue
        if key == "gpu_ids":
            p.add_argument("--gpu_ids", type=str, default="0", help="gpu ids, e.g. 0 or 0,1,2; -1 for the CPU.  One process drives ONE GPU "
                           "(the first id); start one process per GPU with torchrun for more")
        elif key == "compute_dtype":
            p.add_argument("--compute_dtype", choices=("bf16", "fp32"), default=value)
        elif key == "checkpoints_dir":
            p.add_argument("--checkpoints_dir", "----checkpoints_dir", type=str, default=value,
                           help="(the second spelling is the reference README's)")
        elif isinstance(value, bool):
            p.add_argument("--" + key, nargs="?", const=True, type=str2bool, default=False if key in flags else value)
        elif value is None:                                               # a path with no default (weight_dir)
            p.add_argument("--" + key, type=str, default=None)
        else:
            p.add_argument("--" + key, type=type(value), default=value)
    # the loader's options (options/base_options.py, data/custom_dataset.py, data/pix2pix_dataset.py)
    p.add_argument("--batchSize", type=int, default=32, help="the GLOBAL batch: each rank takes batchSize / world")
    p.add_argument("--load_size", type=int, default=512)
    p.add_argument("--preprocess_mode", type=str, default="resize_and_crop")
    p.add_argument("--data_dir", type=str, default="./datasets/FFHQ")
    p.add_argument("--label_dir", type=str, default="train_labels")
    p.add_argument("--image_dir", type=str, default="train_images")
    p.add_argument("--orient_dir", type=str, default="train_dense_orients")
    p.add_argument("--clear", type=str, default="", help="prefix of the three directory names")
    p.add_argument("--max_dataset_size", type=int, default=sys.maxsize)
    p.add_argument("--serial_batches", action="store_true")
    p.add_argument("--no_flip", action="store_true")
    p.add_argument("--no_pairing_check", action="store_true")
    p.add_argument("--color_jitter", action="store_true", help="refused by the device loader")
    p.add_argument("--ig_model_name", type=str, default="InpaintingModel_gen.pth")
    p.add_argument("--sig_model_name", type=str, default="SInpaintingModel_gen.pth")
    p.add_argument("--resident", choices=("device", "host"), default="device", help="where the decoded dataset is kept")
    p.add_argument("--seed", type=int, default=None, help="seed of the weights, the epoch orders and every draw (default: unseeded)")
    if is_train:                                                      # options/train_options.py
        p.add_argument("--continue_train", action="store_true")
        p.add_argument("--which_epoch", type=str, default="latest")
        p.add_argument("--print_freq", type=int, default=100)
        p.add_argument("--save_latest_freq", type=int, default=5000)
        p.add_argument("--save_epoch_freq", type=int, default=1)
        p.add_argument("--display_freq", type=int, default=0, help="0 = off; else the first generated sample as a PNG under web/images/")
        p.add_argument("--D_steps_per_G", type=int, default=1)
        p.add_argument("--G_steps_per_D", type=int, default=1)
        p.add_argument("--no_discriminator", action="store_true")
        p.add_argument("--val_freq", type=int, default=0, help="0 = off; else every N-th epoch rank 0 measures the generator on "
                       "<data_dir>/val_* (michigan_amd.evaluate, protocol reconstruct) and appends the pooled line to val_log.txt")
        p.add_argument("--val_max_samples", type=int, default=64, help="how many val_* samples a validation pass takes (0 = all)")
    return p


def finish_options(opt, is_train: bool):
    """options/base_options.py:212-242 after parsing: isTrain, the gpu id list, and what --use_ig implies here"""
    opt.isTrain = is_train
    opt.curr_step = 1
    opt.gpu_ids = [i for i in (int(s) for s in str(opt.gpu_ids).split(",")) if i >= 0]
    opt.inpaint_orient = bool(opt.use_ig)
    return opt


def parse(argv: Optional[List[str]] = None):
    return finish_options(build_parser(True).parse_args(argv), is_train=True)


class IterationCounter:
    """util/iter_counter.py, its arithmetic kept: `total_steps_so_far` and `epoch_iter` advance by the GLOBAL batch,
    needs_* = (total % freq) < batchSize, and `iter.txt` holds two integers (epoch, iteration within it) written at the same moments.
    `dataset_size` is what the reference passes: len(dataloader), the number of batches of an epoch (train.py:35)."""

    def __init__(self, opt, dataset_size: int, write: bool = True):
        self.opt, self.dataset_size, self.write = opt, dataset_size, write
        self.first_epoch, self.epoch_iter = 1, 0
        self.total_epochs = opt.niter + opt.niter_decay
        self.iter_record_path = os.path.join(opt.checkpoints_dir, opt.name, "iter.txt")
        if opt.isTrain and opt.continue_train:
            try:
                with open(self.iter_record_path) as f:
                    self.first_epoch, self.epoch_iter = (int(v) for v in f.read().replace(",", " ").split())
                print("Resuming from epoch %d at iteration %d" % (self.first_epoch, self.epoch_iter))
            except (OSError, ValueError):
                print("Could not load iteration record at %s. Starting from beginning." % self.iter_record_path)
        self.total_steps_so_far = (self.first_epoch - 1) * dataset_size + self.epoch_iter

    def training_epochs(self):
        return range(self.first_epoch, self.total_epochs + 1)

    def record_epoch_start(self, epoch):
        self.epoch_start_time = self.last_iter_time = time.time()
        self.epoch_iter = 0
        self.current_epoch = epoch

    def record_one_iteration(self):
        now = time.time()
        self.time_per_iter = (now - self.last_iter_time) / self.opt.batchSize
        self.last_iter_time = now
        self.total_steps_so_far += self.opt.batchSize
        self.epoch_iter += self.opt.batchSize

    def _record(self, epoch, it):
        if self.write:
            with open(self.iter_record_path, "w") as f:            # np.savetxt((a, b), fmt='%d'): one integer per line
                f.write("%d\n%d\n" % (epoch, it))
            print("Saved current iteration count at %s." % self.iter_record_path)

    def record_epoch_end(self):
        self.time_per_epoch = time.time() - self.epoch_start_time
        if self.write:
            print("End of epoch %d / %d \t Time Taken: %d sec" % (self.current_epoch, self.total_epochs, self.time_per_epoch))
        if self.current_epoch % self.opt.save_epoch_freq == 0:
            self._record(self.current_epoch + 1, 0)

    def record_current_iter(self):
        self._record(self.current_epoch, self.epoch_iter)

    def needs_saving(self):
        return (self.total_steps_so_far % self.opt.save_latest_freq) < self.opt.batchSize

    def needs_printing(self):
        return (self.total_steps_so_far % self.opt.print_freq) < self.opt.batchSize

    def needs_displaying(self):
        return self.opt.display_freq > 0 and (self.total_steps_so_far % self.opt.display_freq) < self.opt.batchSize


def _floats(losses) -> dict:
    return {k: float(v.detach().float().mean()) if torch.is_tensor(v) else float(v) for k, v in losses.items()}


def format_errors(opt, epoch, i, errors: dict, t) -> str:
    """Visualizer.print_current_errors (util/visualizer.py:116-130)"""
    message = time.asctime(time.localtime(time.time())) + "(step: %d, epoch: %d, iters: %d, time: %.3f) " % (opt.curr_step, epoch, i, t)
    return message + "".join("%s: %.3f " % (k, v) for k, v in errors.items())


def _device(opt) -> torch.device:
    return torch.device("cuda", torch.cuda.current_device()) if len(opt.gpu_ids) > 0 and torch.cuda.is_available() else torch.device("cpu")


def make_loaders(opt, rank: int, world: int):
    """(step-1 loader, step-2 loader or None) over ONE resident copy of the dataset"""
    from .data import EpochLoader, ResidentDataset
    dev = _device(opt)
    generator = None
    rng = _random.Random()
    if opt.seed is not None:
        rng = _random.Random(opt.seed + rank)
        generator = torch.Generator(device=dev)
        generator.manual_seed(opt.seed + rank)
    ds = ResidentDataset(opt, dev, step=1, rng=rng, generator=generator, resident=opt.resident)
    kw = dict(shuffle=not opt.serial_batches, drop_last=opt.isTrain, seed=opt.seed, rank=rank, world=world)
    one = EpochLoader(ds, opt.batchSize // world, **kw)
    two = EpochLoader(ds.at_step(2), opt.batchSize // world, **kw) if opt.unpairTrain else None
    return one, two


def train(opt, loaders=None) -> dict:
    """train.py:26-143.  loaders: (step-1 loader, step-2 loader or None) to use instead of the dataset below opt.data_dir -- iterables of
    batches with len() and, optionally, set_epoch().  Returns {"epochs", "iterations"} run by this call, "losses" (the last ones, as
    floats) and "images_per_s" (global images of the last epoch over its wall time, the device drained at both ends)."""
    if opt.seed is not None:
        torch.manual_seed(opt.seed)
    trainer = Pix2PixTrainer(opt)                                    # joins the data-parallel job when there is one (parallel.init)
    if opt.seed is not None:
        parallel.seed_shared_rng(opt.seed)
    rank, world = parallel.rank(), parallel.world_size()
    if opt.batchSize % world != 0:
        raise ValueError("Batch size %d is wrong. It must be a multiple of the %d ranks." % (opt.batchSize, world))
    trainer.pix2pix_model_on_one_gpu.load_inpainting()
    dataloader, dataloader2 = loaders if loaders is not None else make_loaders(opt, rank, world)
    if opt.unpairTrain and dataloader2 is None:
        raise ValueError("unpairTrain needs the step-2 loader")
    run_dir = os.path.join(opt.checkpoints_dir, opt.name)
    if rank == 0:
        os.makedirs(run_dir, exist_ok=True)
    if opt.continue_train:
        trainer.load(opt.which_epoch)
    iter_counter = IterationCounter(opt, len(dataloader), write=rank == 0)
    log_name = os.path.join(run_dir, "loss_log.txt")
    if rank == 0:
        with open(log_name, "a") as f:
            f.write("================ Training Loss (%s) ================\n" % time.strftime("%c"))
    done = {"epochs": 0, "iterations": 0, "losses": {}, "images_per_s": 0.0}
    sync = (lambda: torch.cuda.synchronize()) if _device(opt).type == "cuda" else (lambda: None)

    def stage(loader, step, epoch):
        """one `for i, data_i in enumerate(dataloader)` of train.py (:45-82 at step 2, :93-132 at step 1)"""
        iter_counter.record_epoch_start(epoch)
        opt.curr_step = step
        trainer.init_losses()
        if hasattr(loader, "set_epoch"):
            loader.set_epoch(epoch)
        for i, data_i in enumerate(loader, start=iter_counter.epoch_iter):
            iter_counter.record_one_iteration()
            if i % opt.D_steps_per_G == 0:
                trainer.run_generator_one_step(data_i)
            if i % opt.G_steps_per_D == 0 and not opt.no_discriminator:
                trainer.run_discriminator_one_step(data_i)
            done["iterations"] += 1
            if iter_counter.needs_printing():
                losses = _floats(trainer.get_latest_losses())
                if rank == 0:
                    message = format_errors(opt, epoch, iter_counter.epoch_iter, losses, iter_counter.time_per_iter)
                    print(message)
                    with open(log_name, "a") as f:
                        f.write("%s\n" % message)
            if iter_counter.needs_displaying() and rank == 0:
                save_generated(trainer, os.path.join(run_dir, "web", "images", "epoch%03d_iter%07d_synthesized_image.png"
                                                     % (epoch, iter_counter.total_steps_so_far)))
            if iter_counter.needs_saving():
                if rank == 0:
                    print("saving the latest model (epoch %d, total_steps %d)" % (epoch, iter_counter.total_steps_so_far))
                trainer.save("latest")                                   # on EVERY rank: parallel.rank0_write is a collective
                iter_counter.record_current_iter()
        trainer.update_learning_rate(epoch)
        iter_counter.record_epoch_end()

    for epoch in iter_counter.training_epochs():
        sync()
        t0, n0 = time.time(), done["iterations"]
        if opt.unpairTrain:
            stage(dataloader2, 2, epoch)
        stage(dataloader, 1, epoch)
        sync()
        done["images_per_s"] = (done["iterations"] - n0) * opt.batchSize / max(time.time() - t0, 1e-9)
        done["epochs"] += 1
        if epoch % opt.save_epoch_freq == 0 or epoch == iter_counter.total_epochs:
            if rank == 0:
                print("saving the model at the end of epoch %d, iters %d" % (epoch, iter_counter.total_steps_so_far))
            trainer.save("latest")
            trainer.save(epoch)
        if getattr(opt, "val_freq", 0) > 0 and epoch % opt.val_freq == 0 and rank == 0:
            validate(opt, trainer.pix2pix_model_on_one_gpu, epoch, os.path.join(run_dir, "val_log.txt"))
    done["losses"] = _floats(trainer.get_latest_losses())
    if rank == 0:
        print("Training was successfully finished.")
    return done


def validate(opt, model, epoch: int, log_name: str) -> dict:
    """--val_freq: evaluate.evaluate(protocol 'reconstruct') over <data_dir>/val_*, capped by --val_max_samples, on `model` in eval();
    the pooled values go to `log_name` as one line and every module goes back to the mode it was in.  Nothing of the training run moves:
    the pass has a random.Random and a torch.Generator of its own (seeded by --seed and the epoch), runs under no_grad with the global
    torch generators forked, in eval() no spectral-norm vector and no running statistic is written, and the job-shared host generator
    (the encoder draws its mask expansion from it while opt.isTrain, in eval() too) is seeded for the pass and put back afterwards.
    The files are cut deterministically: load_size = crop_size, no flip."""
    import copy
    from . import evaluate as E
    dev = next(model.parameters()).device
    vopt = copy.copy(opt)
    vopt.subset, vopt.no_flip, vopt.load_size, vopt.add_zeros = "val", True, opt.crop_size, False
    vopt.batchSize = max(1, opt.batchSize // parallel.world_size())
    seed = (opt.seed if opt.seed is not None else 0) + 7919 * epoch
    generator = torch.Generator(device=dev)
    generator.manual_seed(seed)
    names = E.reconstruct_names(vopt, getattr(opt, "val_max_samples", 0))
    modes = [(m, m.training) for m in model.modules()]              # the frozen nets are in eval() inside a model that trains
    shared = parallel.shared_rng()
    shared_state = shared.getstate()
    model.eval()
    try:
        shared.seed(seed)
        with torch.no_grad(), torch.random.fork_rng(devices=[dev] if dev.type == "cuda" else []):
            result = E.evaluate(vopt, model, names, "reconstruct", rng=_random.Random(seed), generator=generator)
    finally:
        shared.setstate(shared_state)
        for m, mode in modes:
            m.training = mode
    message = "(epoch: %d, samples: %d) " % (epoch, result["samples"]) + "".join(
        "%s: %.4f " % (k, result["pooled"][k]) for k in E.POOLED_KEYS[1:])
    print("validation " + message)
    with open(log_name, "a") as f:
        f.write("%s\n" % message)
    return result


def save_generated(trainer, path: str):
    from PIL import Image
    from .inference import tensor2im
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(tensor2im(trainer.get_latest_generated()[0]).cpu().numpy()).save(path)


def main(argv: Optional[List[str]] = None) -> int:
    opt = parse(argv)
    from .dropin import init_distributed
    in_job = init_distributed()                                       # under torchrun: one process per GPU, pinned to its own
    if not in_job and len(opt.gpu_ids) > 0 and torch.cuda.is_available():
        torch.cuda.set_device(opt.gpu_ids[0])
    print(" ".join(sys.argv))
    train(opt)
    return 0


if __name__ == "__main__":
    sys.exit(main())
