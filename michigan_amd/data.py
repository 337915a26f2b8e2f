"""A dataset directory as device batches: the layer between the files and `inputs.DeviceInputPipeline`.

The reference lists three directories (data/custom_dataset.py:43-70, data/image_folder.py:16-64), sorts and pairs them
(data/pix2pix_dataset.py:23-52) and then decodes, resizes, crops and draws per SAMPLE in `nThreads` worker processes
(pix2pix_dataset.py:66-194, data/__init__.py:41-58).  Here every file is decoded ONCE, the decoded bytes stay resident (FFHQ at 512 x 512:
0.75 MB of image + 2 x 0.25 MB of maps = about 1.3 MB per sample), and a batch is one index gather per map followed by one call of the device
pipeline:

    list_dataset(opt)       the three sorted, paired path lists
    ResidentDataset         the decoded files as three u8 tensors + `batch(indices)`
    EpochLoader             the order of an epoch, per rank: an iterable of batches with `set_epoch`

No new kernel: the launches are the pipeline's (mg_resize_bicubic_u8, mg_input_crop_u8, mg_orient_to_rgb_u8, mg_generate_hole_u8,
mg_noise_octaves).  There is no prefetch thread and no side stream either: the device loader costs 0.54 ms per batch of 8 at 512 x 512
against a 62 ms training step (profiles/r01_input_pipeline.json), so there is nothing to hide behind the step; the loader runs on the
step's stream, in order.
"""
from __future__ import annotations

import os
import random as _random
import re
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence

import torch

from . import parallel
from .inputs import DeviceInputPipeline, upload

# data/image_folder.py:16-19, matched with str.endswith: case-sensitive, and '.TIFF' / '.WEBP' are NOT in the list
IMG_EXTENSIONS = ('.jpg', '.JPG', '.jpeg', '.JPEG', '.png', '.PNG', '.ppm', '.PPM', '.bmp', '.BMP', '.tiff', '.webp')
ORIENT_SUFFIX = "_orient_dense"
DECODE_THREADS = 16


def natural_key(text: str):
    """util.natural_keys (util/util.py:154-164): digit runs compare as integers"""
    return [int(c) if c.isdigit() else c for c in re.split(r'(\d+)', text)]


def _listed(directory: str) -> List[str]:
    """make_dataset(dir, recursive=False, read_cache=True) (data/image_folder.py:36-64): the lines of `files.list` where there is one,
    else every image file below the directory"""
    cache = os.path.join(directory, "files.list")
    if os.path.isfile(cache):
        with open(cache, "r") as f:
            return f.read().splitlines()
    if not (os.path.isdir(directory) or os.path.islink(directory)):
        raise ValueError("%s is not a valid directory" % directory)
    paths = []
    for root, _, names in sorted(os.walk(directory)):
        paths += [os.path.join(root, n) for n in names if n.endswith(IMG_EXTENSIONS)]
    return paths


def _stem(path: str) -> str:
    return os.path.splitext(os.path.basename(path))[0]


def list_dataset(opt) -> Dict[str, List[str]]:
    """CustomDataset.get_paths + Pix2pixDataset.initialize: {"label", "image", "orient"} -> paths, natural-sorted on the FULL path,
    truncated to `max_dataset_size`, the label / image stems checked pair by pair (`paths_match`) unless `no_pairing_check`.

    Stricter than the reference in one place: the reference pairs the orientation files with the labels by sort order ALONE, which
    silently mispairs them as soon as one is missing or the two orders differ ('2B.png' sorts after '2.png', '2B_orient_dense.png' before
    '2_orient_dense.png').  Here the number of orientation files must be the labels', and each stem must be `<label stem>` or
    `<label stem>_orient_dense`; `no_pairing_check` switches that off together with the reference's own check."""
    if getattr(opt, "no_orientation", False):
        raise ValueError("list_dataset: no_orientation is not supported (the device loader always reads the orientation map)")
    if not getattr(opt, "no_instance", True):
        raise ValueError("list_dataset: no_instance=False is not supported (the device loader has no instance-map route)")
    clear = getattr(opt, "clear", "")
    dirs = {k: os.path.join(opt.data_dir, clear + getattr(opt, k + "_dir", d))
            for k, d in (("label", "train_labels"), ("image", "train_images"), ("orient", "train_dense_orients"))}
    paths = {k: _listed(d) for k, d in dirs.items()}
    for other in ("image", "orient"):
        if len(paths["label"]) != len(paths[other]):
            raise ValueError("The #images in %s and %s do not match (%d and %d). Is there something wrong?"
                             % (dirs["label"], dirs[other], len(paths["label"]), len(paths[other])))
    limit = getattr(opt, "max_dataset_size", None)
    for k in paths:
        paths[k].sort(key=natural_key)
        paths[k] = paths[k][:limit]
    if not getattr(opt, "no_pairing_check", False):
        for lab, img, ori in zip(paths["label"], paths["image"], paths["orient"]):
            if _stem(lab) != _stem(img):
                raise ValueError("The label-image pair (%s, %s) do not look like the right pair because the filenames are quite different. "
                                 "Are you sure about the pairing? Use --no_pairing_check to bypass this." % (lab, img))
            if _stem(ori) not in (_stem(lab), _stem(lab) + ORIENT_SUFFIX):
                raise ValueError("The label-orientation pair (%s, %s) do not look like the right pair: the orientation file of <stem> is "
                                 "<stem> or <stem>%s. Use --no_pairing_check to bypass this." % (lab, ori, ORIENT_SUFFIX))
    return paths


def _decode(path: str, rgb: bool) -> torch.Tensor:
    import numpy as np
    from PIL import Image
    with Image.open(path) as im:
        arr = np.array(im.convert("RGB") if rgb else im)
    if arr.dtype != np.uint8 or arr.ndim != (3 if rgb else 2):
        raise ValueError("%s: expected %s, decoded %s %s" % (path, "an RGB image" if rgb else "one 8-bit channel", arr.dtype, arr.shape))
    return torch.from_numpy(arr)


class ResidentDataset:
    """The decoded dataset, resident: `image` u8 [M,Hi,Wi,3], `label` and `orient` u8 [M,Hs,Ws] -- about 1.3 MB per sample for FFHQ at
    512 x 512 (`nbytes` reports the figure of this dataset) -- and `batch(indices)`, Pix2pixDataset.__getitem__ for a whole batch.

    Every file is decoded once with Pillow (images through `.convert("RGB")`; a label or orientation file must decode to one 8-bit channel)
    on a pool of min(16, M) THREADS: not sized by the machine's CPU count, and no worker process, so nothing forks after the GPU is
    initialised.  All maps must have one stored size and all images one stored size (the reference's generate_hole(label, orient_mask)
    combines the maps of two samples pixel by pixel, so it needs equal map sizes too).

    resident="device" keeps the three tensors on `device`; "host" keeps them in pinned host memory and uploads the gathered batch.
    step: 1 = the reference sample is the target, 2 = the unpaired stage's (another sample, drawn per item).  `at_step` returns a view of the
    same resident tensors for the other step: the two loaders of an unpaired run share one decoded copy."""

    def __init__(self, opt, device, step: int = 1, rng: Optional[_random.Random] = None, generator: Optional[torch.Generator] = None,
                 resident: str = "device"):
        if resident not in ("device", "host"):
            raise ValueError("resident must be 'device' or 'host', got %r" % (resident,))
        if step not in (1, 2):
            raise ValueError("step must be 1 or 2, got %r" % (step,))
        self.opt, self.device, self.step, self.resident = opt, torch.device(device), step, resident
        self.rng = rng if rng is not None else _random.Random()
        self.paths = list_dataset(opt)
        m = len(self.paths["label"])
        if m == 0:
            raise ValueError("no sample below %s" % opt.data_dir)
        with ThreadPoolExecutor(max_workers=min(DECODE_THREADS, m)) as pool:
            decoded = {k: list(pool.map(lambda p, rgb=(k == "image"): _decode(p, rgb), self.paths[k])) for k in ("image", "label", "orient")}
        map_size = tuple(decoded["label"][0].shape)
        for k, size in (("image", tuple(decoded["image"][0].shape)), ("label", map_size), ("orient", map_size)):
            for path, t in zip(self.paths[k], decoded[k]):
                if tuple(t.shape) != size:
                    raise ValueError("%s: stored size %s, the dataset's %s have %s" % (
                        path, tuple(t.shape[:2]), "images" if k == "image" else "maps", size[:2]))
        self.image, self.label, self.orient = (self._place(torch.stack(decoded[k])) for k in ("image", "label", "orient"))
        self.pipeline = DeviceInputPipeline(opt, self.device, rng=self.rng, generator=generator)

    def _place(self, t: torch.Tensor) -> torch.Tensor:
        if self.resident == "device":
            return t.to(self.device)
        return t.pin_memory() if self.device.type == "cuda" else t

    def at_step(self, step: int) -> "ResidentDataset":
        if step not in (1, 2):
            raise ValueError("step must be 1 or 2, got %r" % (step,))
        other = object.__new__(ResidentDataset)
        other.__dict__.update(self.__dict__)
        other.step = step
        return other

    def __len__(self) -> int:
        return self.image.shape[0]

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.image, self.label, self.orient))

    def _gather(self, src: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
        """src[idx] on the device: one index gather where the maps are resident, a gather into pinned memory and one upload otherwise"""
        if self.resident == "device" or self.device.type != "cuda":
            return src.index_select(0, idx)
        out = torch.empty((idx.numel(),) + tuple(src.shape[1:]), dtype=src.dtype, pin_memory=src.is_pinned())
        torch.index_select(src, 0, idx, out=out)
        return out.to(self.device, non_blocking=True)

    def batch(self, indices: Sequence[int]) -> Dict[str, object]:
        """The `data` dict of pix2pix_dataset.py:178-188 for the samples `indices`.  Draws, all from the injected `random.Random`, in this
        order: per sample of the batch, `index_ref = randint(0, M-1)` (only at step 2; :76-80) then `index_orient_ref = randint(0, M-1)`
        (always; :124); then the pipeline's own (per sample x, y, flip; with use_ig per sample the hole's threshold, then per sample its
        centre).  The reference's `orient_random_param = random.random()` is compared with `orient_random_th = 2` (:127-131): its other
        orientation branch is dead code, so neither the draw nor the branch exists here.
        Then ONE call of the kept DeviceInputPipeline.  Returned: its dict, `path` (the image paths of the reference samples, as the
        reference returns them) and, for tests, the drawn indices under `_indices`."""
        m = len(self)
        index = [int(i) for i in indices]
        if not index or min(index) < 0 or max(index) >= m:
            raise IndexError("batch indices %s outside the dataset's [0, %d)" % (index, m))
        index_ref, index_orient = [], []
        for i in index:
            index_ref.append(self.rng.randint(0, m - 1) if self.step == 2 else i)
            index_orient.append(self.rng.randint(0, m - 1))
        rows = torch.tensor([index, index_orient, index_ref], dtype=torch.int64)
        if self.resident == "device":
            rows = upload(rows, self.device)                                     # the batch's indices: ONE small copy, through pinned memory
        idx, idx_orient, idx_ref = rows[0], rows[1], rows[2]
        refs = {}
        if self.step == 2:
            refs = dict(image_ref=self._gather(self.image, idx_ref), label_ref=self._gather(self.label, idx_ref))
        data = self.pipeline(self._gather(self.image, idx), self._gather(self.label, idx), self._gather(self.orient, idx),
                             orient_mask=self._gather(self.label, idx_orient), **refs)
        data["path"] = [self.paths["image"][i] for i in index_ref]
        data["_indices"] = {"index": index, "index_ref": index_ref, "index_orient_ref": index_orient}
        return data


class EpochLoader:
    """data.create_dataloader's DataLoader (data/__init__.py:41-58) over a ResidentDataset: iterating yields `dataset.batch(...)` for the
    batches of the current epoch; `len()` is their number.  The order of epoch e is torch.randperm(M) from a generator seeded by
    (seed, e) -- call `set_epoch(e)` before each epoch -- or arange(M) without `shuffle` (the reference's serial_batches).

    batch_size is PER RANK.  With world > 1 the order is truncated to a multiple of world * batch_size and cut into batches of batch_size;
    rank r takes batches r, r + world, ...: the ranks are disjoint, all take the same number of batches, and their union is a prefix of the
    single-rank order.  With world == 1, drop_last decides about a final short batch (the reference: drop_last = opt.isTrain).
    seed: None = a draw from parallel.shared_rng(), the job-shared host RNG, so the ranks agree without a collective of their own (make
    that call at the same point on every rank)."""

    def __init__(self, dataset, batch_size: int, *, shuffle: bool, drop_last: bool, seed: Optional[int] = None, rank: int = 0, world: int = 1):
        if batch_size < 1 or world < 1 or not 0 <= rank < world:
            raise ValueError("EpochLoader: batch_size %r, rank %r of %r" % (batch_size, rank, world))
        self.dataset, self.batch_size, self.shuffle, self.drop_last = dataset, int(batch_size), bool(shuffle), bool(drop_last)
        self.rank, self.world = int(rank), int(world)
        self.seed = int(seed) if seed is not None else parallel.shared_rng().getrandbits(62)
        self.epoch = 0

    def set_epoch(self, epoch: int):
        self.epoch = int(epoch)

    def order(self) -> torch.Tensor:
        m = len(self.dataset)
        if not self.shuffle:
            return torch.arange(m)
        g = torch.Generator()
        g.manual_seed((self.seed * 1000003 + self.epoch) % (1 << 63))
        return torch.randperm(m, generator=g)

    def indices(self) -> List[List[int]]:
        """this rank's batches of the current epoch, as lists of sample indices"""
        order, bs = self.order().tolist(), self.batch_size
        if self.world > 1 or self.drop_last:
            order = order[:len(order) // (self.world * bs) * (self.world * bs)]
        batches = [order[i:i + bs] for i in range(0, len(order), bs)]
        return batches[self.rank::self.world]

    def __len__(self) -> int:
        m, bs = len(self.dataset), self.batch_size
        if self.world > 1 or self.drop_last:
            return m // (self.world * bs)
        return (m + bs - 1) // bs

    def __iter__(self):
        for index in self.indices():
            yield self.dataset.batch(index)
