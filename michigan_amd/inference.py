"""`python -m michigan_amd.inference`: the reference's inference.py without a reference checkout.

    python -m michigan_amd.inference --name MichiGAN --gpu_ids 0 --inference_ref_name 67172 --inference_tag_name 67172 \
        --inference_orient_name 67172 --netG spadeb --which_epoch 50 --use_encoder --noise_background --expand_mask_be --expand_th 5 \
        --use_ig --load_size 512 --crop_size 512 --add_feat_zeros --data_dir <dataset>

The seven files of single_inference_dataLoad (data/base_dataset.py:52-58) are decoded with Pillow and go through
`DeviceInputPipeline.inference_batch`; the model is loaded from `<checkpoints_dir>/<name>/<which_epoch>_net_G.pth` (and the frozen
in-painting net from its own file, `Pix2PixModel.load_inpainting`), put in eval() and run in mode 'inference'; `tensor2im` runs on the
device.  The result goes to `<results_dir>/inpaint_fake_image.jpg` with use_ig, else `fake_image.jpg` (inference.py:53-56;
results_dir defaults to ./inference_samples).  `--pairs_file F` (lines `ref tag orient`) runs the listed triples in batches of up to
batchSize and writes `<tag>_from_<ref>.png` each.  `generate(opt, model, names)` is the importable form.
"""
from __future__ import annotations

import os
import random as _random
import sys
from typing import List, Optional, Sequence, Tuple

import torch

from .inputs import DeviceInputPipeline, _pad_zeros


def tensor2im(image: torch.Tensor) -> torch.Tensor:
    """util.tensor2im (util/util.py:64-95) on the device: [N,C,H,W] (or [C,H,W]) in [-1, 1] -> uint8 [N,H,W,C] (or [H,W,C]),
    clip((x + 1) / 2 * 255, 0, 255) truncated, the reference's operation order in fp32."""
    x = image.detach().float()
    x = torch.clamp((x + 1) / 2.0 * 255.0, 0, 255).to(torch.uint8)
    return x.permute(0, 2, 3, 1).contiguous() if x.dim() == 4 else x.permute(1, 2, 0).contiguous()


def sample_paths(opt, ref: str, tag: str, orient: str) -> dict:
    """the seven paths of single_inference_dataLoad (data/base_dataset.py:50-58), by the pipeline's argument names"""
    base = opt.data_dir + '/' + opt.subset
    return {"label_ref": base + '_labels/' + ref + '.png', "label_tag": base + '_labels/' + tag + '.png',
            "orient_tag": base + '_dense_orients/' + tag + '_orient_dense.png',
            "orient_ref": base + '_dense_orients/' + orient + '_orient_dense.png',
            "orient_mask": base + '_labels/' + orient + '.png',
            "image_ref": base + '_images/' + ref + '.jpg', "image_tag": base + '_images/' + tag + '.jpg'}


def _decode(path: str, rgb: bool) -> torch.Tensor:
    import numpy as np
    from PIL import Image
    if not os.path.isfile(path):
        raise FileNotFoundError("inference input %s does not exist" % path)
    with Image.open(path) as im:
        arr = np.array(im.convert("RGB") if rgb else im)
    if arr.dtype != np.uint8 or arr.ndim != (3 if rgb else 2):
        raise ValueError("%s: expected %s, decoded %s %s" % (path, "an RGB image" if rgb else "one 8-bit channel", arr.dtype, arr.shape))
    return torch.from_numpy(arr)


def _stacked(opt, triples) -> dict:
    out = {}
    for key in ("label_ref", "label_tag", "orient_tag", "orient_ref", "orient_mask", "image_ref", "image_tag"):
        paths = [sample_paths(opt, *t)[key] for t in triples]
        maps = [_decode(p, key.startswith("image")) for p in paths]
        for p, m in zip(paths, maps):
            if m.shape != maps[0].shape:
                raise ValueError("%s: stored size %s, the first sample of its batch has %s (run samples of different sizes in "
                                 "batches of their own: --batchSize 1)" % (p, tuple(m.shape[:2]), tuple(maps[0].shape[:2])))
        out[key] = torch.stack(maps)
    return out


def generated_batches(opt, model, names: Sequence[Tuple[str, str, str]], rng: Optional[_random.Random] = None,
                      generator: Optional[torch.Generator] = None, given_orientation: bool = False):
    """The batch loop of `generate`, as a generator: yields (data, generated fp32 [n,3,H,W]) per batch -- the loader's dict and the
    net's output, remove_background applied, before tensor2im and before the add_th border comes off.  The triples run in batches of
    up to opt.batchSize; a batch holds triples of one hole rule (orient == tag or not, base_dataset.py:116) and of one stored size.
    `data["names"]` lists the batch's triples.  given_orientation (michigan_amd.evaluate): two more maps cut at the batch's own window,
    `orient_given` (the orientation sample's map, uint8 values as fp32 [n,1,H,W]) and `orient_given_mask` (label_tag AND the
    orientation sample's label)."""
    device = next(model.parameters()).device
    pipe = DeviceInputPipeline(opt, device, rng=rng, generator=generator)
    bs = max(1, int(getattr(opt, "batchSize", 1)))
    names = [tuple(t) for t in names]
    i = 0
    while i < len(names):
        same = names[i][2] == names[i][1]
        j = i + 1
        while j < len(names) and j - i < bs and (names[j][2] == names[j][1]) == same:
            j += 1
        files = _stacked(opt, names[i:j])
        data = pipe.inference_batch(same_orient=same, **files)
        if given_orientation:                                                     # after the batch: its draws and launches are untouched
            crop = pipe.last_window.to(device)
            pad = (lambda t: _pad_zeros(t, int(opt.add_th))) if getattr(opt, "add_zeros", False) else (lambda t: t)
            data["orient_given"] = pipe._map(pad(files["orient_ref"]), crop, mode=1)
            data["orient_given_mask"] = pipe._map(pad(files["orient_mask"]), crop, mode=1, unknown_label=int(opt.label_nc), mul=data["label_tag"])
        data["names"] = names[i:j]
        generated = model(data, "inference").float()
        if getattr(opt, "remove_background", False):                              # inference.py:41-42
            label = data["label_tag"].float()
            generated = generated * label + data["image_tag"] * (1 - label)
        yield data, generated
        i = j


def crop_border(opt, image: torch.Tensor) -> torch.Tensor:
    """inference.py:44-48 for a [N,H,W,C] batch: the add_th border comes off under add_feat_zeros / add_zeros"""
    if getattr(opt, "add_feat_zeros", False) or getattr(opt, "add_zeros", False):
        o, c = int(opt.add_th / 2), int(opt.crop_size)
        image = image[:, o:o + c, o:o + c, :]
    return image


def generate(opt, model, names: Sequence[Tuple[str, str, str]], rng: Optional[_random.Random] = None,
             generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """inference.py:33-48 for the (ref, tag, orient) name triples `names`: uint8 [len(names), crop, crop, 3] on the model's device
    (the batches of `generated_batches`, through tensor2im)."""
    return torch.cat([crop_border(opt, tensor2im(generated)).contiguous()
                      for _, generated in generated_batches(opt, model, names, rng=rng, generator=generator)])


def build_model(opt):
    """Pix2PixModel for inference: weights of `which_epoch`, the frozen in-painting net's own file, eval()"""
    from .model import Pix2PixModel
    model = Pix2PixModel(opt)
    if len(opt.gpu_ids) > 0 and torch.cuda.is_available():
        model.cuda()
    model.load(opt.which_epoch)
    model.load_inpainting()
    return model.eval()


def build_inference_parser():
    from .train import build_parser
    p = build_parser(is_train=False)
    p.add_argument("--inference_ref_name", type=str, default="57541", help="which reference sample")
    p.add_argument("--inference_tag_name", type=str, default="56001", help="which target sample")
    p.add_argument("--inference_orient_name", type=str, default="56001", help="which sample's orientation")
    p.add_argument("--subset", type=str, default="val", help="val | train: the prefix of the three directories")
    p.add_argument("--results_dir", type=str, default="./inference_samples")
    p.add_argument("--which_epoch", type=str, default="latest", help="which checkpoint to load (the README command passes 50)")
    p.add_argument("--add_zeros", action="store_true", help="pad the decoded files with add_th zeros (base_dataset.py:69-76)")
    p.add_argument("--expand_tag_mask", action="store_true", help="refused: a 25 x 25 cv2.dilate of the target mask")
    p.add_argument("--pairs_file", type=str, default="", help="lines `ref tag orient`: one <tag>_from_<ref>.png each")
    p.set_defaults(batchSize=1, no_flip=True, serial_batches=True)
    return p


def parse(argv: Optional[List[str]] = None):
    from .train import finish_options
    return finish_options(build_inference_parser().parse_args(argv), is_train=False)


def main(argv: Optional[List[str]] = None) -> int:
    from PIL import Image
    opt = parse(argv)
    model = build_model(opt)
    os.makedirs(opt.results_dir, exist_ok=True)
    if opt.pairs_file:
        with open(opt.pairs_file) as f:
            names = [tuple(line.split()) for line in f if line.strip()]
        bad = [n for n in names if len(n) != 3]
        if bad:
            raise ValueError("%s: every line is `ref tag orient`, got %s" % (opt.pairs_file, bad[0]))
        targets = [os.path.join(opt.results_dir, "%s_from_%s.png" % (tag, ref)) for ref, tag, _ in names]
    else:
        names = [(opt.inference_ref_name, opt.inference_tag_name, opt.inference_orient_name)]
        targets = [os.path.join(opt.results_dir, "inpaint_fake_image.jpg" if opt.use_ig else "fake_image.jpg")]
    rng = generator = None
    if opt.seed is not None:                                          # the window, hole and noise draws, reproducibly
        rng = _random.Random(opt.seed)
        generator = torch.Generator(device=next(model.parameters()).device)
        generator.manual_seed(opt.seed)
    images = generate(opt, model, names, rng=rng, generator=generator).cpu().numpy()
    for (ref, tag, _), image, target in zip(names, images, targets):
        print("process image... %s" % sample_paths(opt, ref, tag, tag)["image_tag"])
        Image.fromarray(image).save(target)
    return 0


if __name__ == "__main__":
    sys.exit(main())
