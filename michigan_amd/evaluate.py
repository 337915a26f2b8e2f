"""`python -m michigan_amd.evaluate`: how good is a trained generator?  (The reference has no counterpart: it stops at pictures.)

    python -m michigan_amd.evaluate --name MichiGAN --which_epoch 50 --data_dir <dataset> --subset val --protocol reconstruct \
        --use_encoder --noise_background --expand_mask_be --use_ig --load_size 512 --crop_size 512 --batchSize 8 --out metrics.json
    python -m michigan_amd.evaluate ... --protocol transfer --pairs_file pairs.txt

The flags are those of `michigan_amd.inference`, plus --protocol, --max_samples and --out.
  reconstruct   every sample s of `<data_dir>/<subset>_*` (listed by data.list_dataset) as the triple (s, s, s): the net rebuilds an image
                from its own mask, orientation and appearance.  Reports PSNR / SSIM of the result against the sample's image, over the
                whole picture and over the hair (label_tag), and what `transfer` reports.
  transfer      the triples `ref tag orient` of --pairs_file.  There is no ground truth, so it reports
                orient_error_deg  the orientation of the result (inputs.dense_orientation under label_tag) against the orientation that
                                  was given -- the orientation sample's map with --use_ig, else the batch's own `orient` -- where
                                  label_tag AND the orientation sample's label: where an orientation was given, not the in-painted hole
                hair_lab          the hair-average Lab distance (ops.hair_lab_losses, its forward value) between the result under
                                  label_tag and image_ref under label_ref
The loop is inference.generated_batches, so a picture measured here is the picture `michigan_amd.inference` writes for the same
seed.  Per batch: the net, tensor2im, the orientation pass, two measurement passes (metrics.image_quality, metrics.orient_distance),
and ONE read-back of a [n, F] float64 table.  The result is one JSON file -- {"protocol", "samples", "pooled": metrics.pooled(rows),
"rows": [one per sample]}; a value that is not finite is written as null -- and one summary line on stdout.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import random as _random
import sys
from typing import List, Optional, Sequence, Tuple

import torch

from . import metrics

POOLED_KEYS = ("samples", "psnr", "psnr_hair", "ssim", "ssim_hair", "orient_error_deg", "hair_lab")
QUALITY_ROW_KEYS = ("psnr", "psnr_hair", "ssim", "ssim_hair", "sse", "sse_hair", "ssim_sum", "ssim_sum_hair", "pixels", "hair_pixels",
                    "ssim_count", "ssim_hair_count", "channels")
COMMON_ROW_KEYS = ("ref", "tag", "orient", "orient_error_deg", "orient_sum", "orient_count", "hair_lab")


def real_u8(image: torch.Tensor) -> torch.Tensor:
    """the loader's image ([N,3,H,W] fp32 in [-1, 1], a uint8 file through Normalize(0.5)) back as uint8 [N,H,W,3], ROUNDED: a file
    stored at the load size comes back byte for byte (tensor2im truncates, which is right for a net's output and one grey level
    short for 254.99998)"""
    x = torch.clamp(torch.round((image.detach().float() + 1) * 127.5), 0, 255).to(torch.uint8)
    return x.permute(0, 2, 3, 1).contiguous()


def reconstruct_names(opt, max_samples: Optional[int] = None) -> List[Tuple[str, str, str]]:
    """(s, s, s) for every sample of <data_dir>/<subset>_{labels,images,dense_orients}, in data.list_dataset's order"""
    from .data import list_dataset
    sub = opt.subset
    listing = argparse.Namespace(data_dir=opt.data_dir, clear=getattr(opt, "clear", ""), label_dir=sub + "_labels", image_dir=sub + "_images",
                                 orient_dir=sub + "_dense_orients", max_dataset_size=sys.maxsize,
                                 no_pairing_check=getattr(opt, "no_pairing_check", False), no_instance=True, no_orientation=False)
    stems = [os.path.splitext(os.path.basename(p))[0] for p in list_dataset(listing)["label"]]
    if max_samples is not None and max_samples > 0:
        stems = stems[:max_samples]
    return [(s, s, s) for s in stems]


def read_pairs(path: str) -> List[Tuple[str, str, str]]:
    with open(path) as f:
        names = [tuple(line.split()) for line in f if line.strip()]
    bad = [n for n in names if len(n) != 3]
    if bad:
        raise ValueError("%s: every line is `ref tag orient`, got %s" % (path, bad[0]))
    return names


def measure_batch(opt, data, generated: torch.Tensor, protocol: str) -> List[dict]:
    """the rows of one batch of inference.generated_batches(..., given_orientation=True): device work, then one read-back"""
    from . import inputs, ops
    from .inference import crop_border, tensor2im
    fake = crop_border(opt, tensor2im(generated)).contiguous()                            # what inference writes: uint8 [n,H,W,3]
    plane = lambda t: crop_border(opt, t.permute(0, 2, 3, 1))[..., 0]                      # a [n,1,H,W] map of the batch -> [n,H,W]
    n = fake.shape[0]
    hair = (plane(data["label_tag"]) == 1)
    hair_u8 = hair.to(torch.uint8).contiguous()
    cols, width = [], []

    def put(t):
        t = t.to(torch.float64).reshape(n, -1)
        cols.append(t)
        width.append(t.shape[1])
    q = None
    if protocol == "reconstruct":
        q = metrics.image_quality(fake, crop_border(opt, real_u8(data["image_tag"])), hair_u8)
        for k in QUALITY_ROW_KEYS[:-1]:
            put(q[k])
    given = data["orient_given"] if getattr(opt, "use_ig", False) else data["orient"]
    given_u8 = torch.clamp(plane(given), 0, 255).to(torch.uint8)
    where = ((plane(data["orient_given_mask"]) == 1) & hair).to(torch.uint8)
    o = metrics.orient_distance(inputs.dense_orientation(fake, hair_u8), given_u8, where)
    for k in ("degrees", "sum", "count"):
        put(o[k])
    hair_ref = (plane(data["label_ref"]) == 1).float()
    image_ref = crop_border(opt, data["image_ref"].permute(0, 2, 3, 1)).permute(0, 3, 1, 2)
    fake_f = crop_border(opt, generated.detach().permute(0, 2, 3, 1)).contiguous()
    with torch.no_grad():
        lab = torch.stack([ops.hair_lab_losses(fake_f[i:i + 1], image_ref[i:i + 1], hair[i:i + 1].float(), hair_ref[i:i + 1])[0] for i in range(n)])
    put(lab)
    table = torch.cat(cols, dim=1).cpu()                                                  # the batch's one read-back
    rows = []
    for i, (ref, tag, orient) in enumerate(data["names"]):
        vals = iter(torch.split(table[i], width))
        row = {"ref": ref, "tag": tag, "orient": orient}
        if q is not None:
            for k in QUALITY_ROW_KEYS[:-1]:
                v = next(vals).tolist()
                row[k] = v if k in ("sse", "sse_hair", "ssim_sum", "ssim_sum_hair") else v[0]
            for k in ("sse", "sse_hair"):
                row[k] = [int(v) for v in row[k]]
            for k in ("pixels", "hair_pixels", "ssim_count", "ssim_hair_count"):
                row[k] = int(row[k])
            row["channels"] = int(q["channels"])
        row["orient_error_deg"] = next(vals).item()
        row["orient_sum"], row["orient_count"] = int(next(vals).item()), int(next(vals).item())
        row["hair_lab"] = next(vals).item()
        rows.append(row)
    return rows


def evaluate(opt, model, names: Sequence[Tuple[str, str, str]], protocol: str = "reconstruct", rng: Optional[_random.Random] = None,
             generator: Optional[torch.Generator] = None) -> dict:
    """{"protocol", "samples", "pooled", "rows"} for the triples `names` (the importable form of the command)"""
    from .inference import generated_batches
    if protocol not in ("reconstruct", "transfer"):
        raise ValueError("evaluate: protocol must be 'reconstruct' or 'transfer', got %r" % (protocol,))
    names = [tuple(t) for t in names]
    if protocol == "reconstruct" and any(not (r == t == o) for r, t, o in names):
        raise ValueError("evaluate: 'reconstruct' runs every sample as (s, s, s); use 'transfer' for other triples")
    rows = []
    for data, generated in generated_batches(opt, model, names, rng=rng, generator=generator, given_orientation=True):
        rows.extend(measure_batch(opt, data, generated, protocol))
    return {"protocol": protocol, "samples": len(rows), "pooled": metrics.pooled(rows), "rows": rows}


def _jsonable(v):
    if isinstance(v, float) and not math.isfinite(v):
        return None
    if isinstance(v, dict):
        return {k: _jsonable(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_jsonable(x) for x in v]
    return v


def write_json(result: dict, path: str):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(_jsonable(result), f, indent=1)
        f.write("\n")


def summary_line(result: dict) -> str:
    p = result["pooled"]
    return "%s: %d samples  " % (result["protocol"], result["samples"]) + "  ".join(
        "%s %.4f" % (k, p[k]) for k in POOLED_KEYS[1:] if isinstance(p[k], float) and not math.isnan(p[k]))


def parse(argv: Optional[List[str]] = None):
    from .inference import build_inference_parser
    from .train import finish_options
    p = build_inference_parser()
    p.prog = "python -m michigan_amd.evaluate"
    p.add_argument("--protocol", choices=("reconstruct", "transfer"), default="reconstruct")
    p.add_argument("--max_samples", type=int, default=0, help="0 = all of them")
    p.add_argument("--out", type=str, default="metrics.json")
    return finish_options(p.parse_args(argv), is_train=False)


def main(argv: Optional[List[str]] = None) -> int:
    from .inference import build_model
    opt = parse(argv)
    if opt.protocol == "transfer":
        if not opt.pairs_file:
            raise ValueError("--protocol transfer needs --pairs_file (lines `ref tag orient`)")
        names = read_pairs(opt.pairs_file)
        if opt.max_samples > 0:
            names = names[:opt.max_samples]
    else:
        names = reconstruct_names(opt, opt.max_samples)
    model = build_model(opt)
    rng = generator = None
    if opt.seed is not None:
        rng = _random.Random(opt.seed)
        generator = torch.Generator(device=next(model.parameters()).device)
        generator.manual_seed(opt.seed)
    result = evaluate(opt, model, names, opt.protocol, rng=rng, generator=generator)
    write_json(result, opt.out)
    print(summary_line(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
