"""`python -m michigan_amd.demo`: the reference's demo.py without Qt -- a headless hair-editing session.

    python -m michigan_amd.demo --name MichiGAN --which_epoch 50 --gpu_ids 0 --demo_data_dir <dir> --tag 67172 --ref 56001 \
        --edit_script edits.json --out ./inference_samples

(use_encoder, noise_background, expand_mask_be, use_ig, use_stroke and add_feat_zeros are on by default, as options/demo_options.py
sets them; `--add_feat_zeros false` switches one off.)

`EditSession` is the state and the logic of demo.py's `Ex` (the window class): what the open_* slots load, and `edit()` / `orient_edit()`
/ `save()` statement for statement, on the device.  The pen record is the UI's own (ui/mouse_event.py:57-64): per colour c,
`mask_points[c]` is a list of {'prev': (x, y), 'curr': (x, y)} and `size_points[c]` the pen width of each segment; colour 0 paints
background, 1 hair, 2 the orientation stroke.  What the reference does with cv2 on the host is two launches here: `inputs.brush_u8`
(make_mask, demo.py:431-435; the package's own integer brush, see include/michigan_hip/editing/mask_edit.h) and `inputs.stroke_hole`
(the 50 x 50 elliptical dilation, demo.py:323-324).  The batch is `DeviceInputPipeline.demo_batch` on one persistent pipeline, the
model runs in mode 'demo_inference'.

The command replays one recorded edit: `<demo_data_dir>/{images,labels,orients,images_recon}/` as demo.py:108-216 reads them for the
target `--tag` and the reference `--ref`, the JSON of `--edit_script` = {"mask_points": [...], "size_points": [...], "use_ref_mask":
bool, "use_ref_orient": bool}, and three files under `--out`: `<tag>_from_<ref>.png` (the result), `<tag>_from_<ref>_orient.png` (the
in-painted orientation picture) and `<tag>_from_<ref>_sheet.jpg` (the five panels of demo.py:421-428).
"""
from __future__ import annotations

import json
import os
import random as _random
import sys
from typing import List, Optional, Sequence

import torch

from . import inputs
from .inference import _decode, tensor2im

HOLE_KSIZE, ORIENT_EDIT_KSIZE = 50, 20                                   # demo.py:323, 471


def pen_segments(points: Sequence[dict], sizes: Sequence[int], colour: int, sample: int = 0) -> List[List[int]]:
    """one colour of the UI's record -> the rows inputs.brush_u8 takes, in the order they were drawn (make_mask's loop)"""
    if len(points) != len(sizes):
        raise ValueError("colour %d: %d segments but %d pen sizes" % (colour, len(points), len(sizes)))
    return [[sample, int(pt["prev"][0]), int(pt["prev"][1]), int(pt["curr"][0]), int(pt["curr"][1]), int(size), colour, 0]
            for pt, size in zip(points, sizes)]


def _colour(record, c: int):
    """record[c] of a list, or of a dict keyed by the colour (JSON object keys are strings); a colour that was never used is empty"""
    if isinstance(record, dict):
        return record.get(c, record.get(str(c), []))
    return record[c] if c < len(record) else []


class EditSession:
    """demo.py's `Ex` without the window.  Every map is a decoded uint8 tensor at its stored size ([H,W] labels and orientations,
    [H,W,3] images), kept on `device`; `model` is a Pix2PixModel built with use_ig (and use_stroke for the stroke route), in eval()."""

    def __init__(self, model, opt, device, rng: Optional[_random.Random] = None, generator: Optional[torch.Generator] = None):
        self.model, self.opt, self.device = model, opt, torch.device(device)
        self.pipe = inputs.DeviceInputPipeline(opt, self.device, rng=rng, generator=generator)    # one pipeline: its tables are built once
        self.mask = self.mask_m = None
        self.tag_img = self.recon_tag_img = self.ref_img = self.ref_label = None
        self.orient = self.orient_mask = self.orient_image = None
        self.vis_stroke = None
        self.used_recon = False
        self.save_datas = {}

    def _dev(self, t, channels: int, name: str) -> torch.Tensor:
        if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.dim() != (2 if channels == 1 else 3) or (channels == 3 and t.shape[-1] != 3):
            raise ValueError("%s: expected a decoded uint8 %s" % (name, "[H,W]" if channels == 1 else "[H,W,3]"))
        return inputs.upload(t.contiguous(), self.device)

    # -- the open_* slots (demo.py:108-293) ---------------------------------------------------------------------------------------------
    def open_tag(self, image, label, orient, recon_image=None):
        """demo.py:130-216: the target's image, its label (the mask to edit), its dense orientation -- whose mask is that label --
        and, when there is one, its reconstruction (images_recon/)."""
        self.tag_img = self._dev(image, 3, "image")
        self.recon_tag_img = None if recon_image is None else self._dev(recon_image, 3, "recon_image")
        self.open_mask(label)
        self.open_orient(orient, label)
        self.orient_image = self.tag_img

    def open_ref(self, image, label):
        self.ref_img, self.ref_label = self._dev(image, 3, "image"), self._dev(label, 1, "label")

    def open_orient(self, orient, orient_mask, image=None):
        """demo.py:218-261: another sample's orientation and the label that masks it (`image`: that sample's picture, for the sheet)"""
        self.orient, self.orient_mask = self._dev(orient, 1, "orient"), self._dev(orient_mask, 1, "orient_mask")
        if image is not None:
            self.orient_image = self._dev(image, 3, "image")

    def open_mask(self, mask):
        self.mask = self._dev(mask, 1, "mask")                              # the original mask
        self.mask_m = self.mask.clone()                                     # the edited mask

    # -- demo.py:431-435 --------------------------------------------------------------------------------------------------------------
    @staticmethod
    def make_mask(mask: torch.Tensor, pts, sizes, colour: int) -> torch.Tensor:
        return inputs.brush_u8(mask, pen_segments(pts, sizes, colour))

    def _ready(self):
        missing = [k for k in ("mask", "tag_img", "ref_img", "ref_label", "orient", "orient_mask") if getattr(self, k) is None]
        if missing:
            raise RuntimeError("EditSession: open_tag and open_ref first (missing: %s)" % ", ".join(missing))

    # -- demo.py:310-379 --------------------------------------------------------------------------------------------------------------
    def edit(self, mask_points, size_points, use_ref_mask: bool, use_ref_orient: bool):
        """Ex.edit(): (result u8 [H,W,3], the in-painted orientation picture u8 [H,W,3]) on the device.  `use_ref_mask` is the UI's
        first radio button (the ORIGINAL mask rather than the edited one), `use_ref_orient` its third (the reference orientation
        rather than the drawn strokes); the choice sets model.opt.inpaint_mode as demo.py:342-359 does."""
        self._ready()
        # get the edited mask
        self.mask_m = self.mask.clone()
        for i in range(2):
            self.mask_m = self.make_mask(self.mask_m, _colour(mask_points, i), _colour(size_points, i), i)
        # process the tag image (demo.py:329-333, decided here, where the edited mask is final and the device has two short launches
        # queued: the step's one read-back waits for nothing else): the reconstruction when the mask was edited, one exists and a
        # hair pixel was erased -- the reference's `1 in np.unique(self.mask - self.mask_m)` on uint8 (a pixel ADDED to the hair
        # wraps to 255, not 1)
        self.used_recon = bool(not use_ref_mask and self.recon_tag_img is not None and ((self.mask - self.mask_m) == 1).any().item())
        tag_image = self.recon_tag_img if self.used_recon else self.tag_img
        # get the edited orient
        orient_new = self.mask_m.clone()
        orient_new = self.make_mask(orient_new, _colour(mask_points, 2), _colour(size_points, 2), 2)
        self.vis_stroke = orient_new.clone()
        orient_new.masked_fill_(orient_new == 1, 0)
        orient_new.masked_fill_(orient_new == 2, 1)
        mask_stroke = orient_new
        mask_hole = inputs.stroke_hole(orient_new, HOLE_KSIZE)
        label_tag = self.mask if use_ref_mask else self.mask_m
        strokes = {} if use_ref_orient else dict(mask_stroke=mask_stroke, mask_hole=mask_hole)
        self.model.opt.inpaint_mode = "ref" if use_ref_orient else "stroke"
        data = self.pipe.demo_batch(label_ref=self.ref_label, label_tag=label_tag, mask_orient=self.orient_mask, orient_ref=self.orient,
                                    image_ref=self.ref_img, image_tag=tag_image, **strokes)
        generated, new_orient_rgb = self.model(data, "demo_inference")
        if getattr(self.opt, "add_feat_zeros", False):
            o, c = int(self.opt.add_th / 2), int(self.opt.crop_size)
            generated = generated[:, :, o:o + c, o:o + c]
        result = tensor2im(generated)[0]
        orient_picture = None if new_orient_rgb is None else new_orient_rgb[0]
        self.save_datas = {"result": result, "ref_img": self.ref_img, "tag_img": self.tag_img, "ori_img": self.orient_image}
        return result, orient_picture

    # -- demo.py:461-472 --------------------------------------------------------------------------------------------------------------
    def orient_edit(self, mask_points, size_points) -> torch.Tensor:
        """Ex.orient_edit(): the strokes painted onto the edited mask IN PLACE (the reference draws on self.mask_m itself and relabels
        it), then the 20 x 20 elliptical dilation; returns the dilated map u8 [H,W]."""
        if self.mask_m is None:
            raise RuntimeError("EditSession: open_tag or open_mask first")
        for i in range(2):
            self.mask_m = self.make_mask(self.mask_m, _colour(mask_points, i), _colour(size_points, i), i)
        orient_new = self.mask_m
        orient_new = self.make_mask(orient_new, _colour(mask_points, 2), _colour(size_points, 2), 2)
        orient_new.masked_fill_(orient_new == 1, 0)
        orient_new.masked_fill_(orient_new == 2, 1)
        return inputs.stroke_hole(orient_new, ORIENT_EDIT_KSIZE)

    # -- demo.py:385-392, 415-428 -----------------------------------------------------------------------------------------------------
    def save_sheet(self, path: str) -> str:
        """Ex.save(): target, reference, the orientation's image, the strokes (hair 255, stroke 127) and the result side by side,
        each crop_size wide, as a JPEG; host Pillow.  `.jpg` is appended unless the path ends in it."""
        from PIL import Image
        if not self.save_datas:
            raise RuntimeError("EditSession.save_sheet: nothing to save before edit()")
        c = int(self.opt.crop_size)
        vis = self.vis_stroke.clone()
        vis.masked_fill_(vis == 1, 255)
        vis.masked_fill_(vis == 2, 127)
        pil = lambda t: Image.fromarray(t.cpu().numpy())
        sheet = Image.new("RGB", (5 * c, c))
        sheet.paste(pil(vis.unsqueeze(-1).expand(-1, -1, 3).contiguous()), box=(3 * c, 0))
        sheet.paste(pil(self.save_datas["tag_img"]), box=(0, 0))
        sheet.paste(pil(self.save_datas["ref_img"]), box=(c, 0))
        sheet.paste(pil(self.save_datas["ori_img"]), box=(2 * c, 0))
        sheet.paste(pil(self.save_datas["result"]), box=(4 * c, 0))
        if not path.endswith(".jpg"):
            path += ".jpg"
        sheet.save(path)
        return path


def sample_paths(opt, name: str) -> dict:
    """the files demo.py:108-216 opens for one sample of <demo_data_dir>"""
    root = opt.demo_data_dir
    return {"image": os.path.join(root, "images", name + ".jpg"), "label": os.path.join(root, "labels", name + ".png"),
            "orient": os.path.join(root, "orients", name + "_orient_dense.png"), "recon": os.path.join(root, "images_recon", name + ".jpg")}


def load_script(path: str) -> dict:
    with open(path) as f:
        script = json.load(f)
    missing = [k for k in ("mask_points", "size_points", "use_ref_mask", "use_ref_orient") if k not in script]
    if missing:
        raise ValueError("%s: the edit script lacks %s" % (path, missing))
    return script


def open_session(opt, model, tag: str, ref: str, rng=None, generator=None) -> EditSession:
    device = next(model.parameters()).device
    session = EditSession(model, opt, device, rng=rng, generator=generator)
    t, r = sample_paths(opt, tag), sample_paths(opt, ref)
    recon = _decode(t["recon"], True) if os.path.exists(t["recon"]) else None
    session.open_tag(_decode(t["image"], True), _decode(t["label"], False), _decode(t["orient"], False), recon)
    session.open_ref(_decode(r["image"], True), _decode(r["label"], False))
    return session


def parse(argv: Optional[List[str]] = None):
    from .train import build_parser, finish_options
    p = build_parser(is_train=False)
    p.prog = "python -m michigan_amd.demo"
    p.add_argument("--which_epoch", type=str, default="50", help="which checkpoint to load (options/demo_options.py)")
    p.add_argument("--expand_tag_mask", action="store_true", help="refused: a 25 x 25 cv2.dilate of the target mask inside the loader")
    p.add_argument("--demo_data_dir", type=str, default="./datasets/FFHQ_demo/", help="images/, labels/, orients/, images_recon/")
    p.add_argument("--tag", type=str, required=True, help="the target sample (the image that is edited)")
    p.add_argument("--ref", type=str, required=True, help="the reference sample (the appearance)")
    p.add_argument("--edit_script", type=str, required=True, help="JSON: mask_points, size_points, use_ref_mask, use_ref_orient")
    p.add_argument("--out", type=str, default="./inference_samples", help="where the three files go")
    # options/demo_options.py:12-30: what the demo switches on by itself (`--flag false` switches one off again)
    p.set_defaults(batchSize=1, no_flip=True, serial_batches=True, name="MichiGAN", use_encoder=True, use_ig=True, noise_background=True,
                   use_stroke=True, expand_mask_be=True, add_feat_zeros=True)
    return finish_options(p.parse_args(argv), is_train=False)


def main(argv: Optional[List[str]] = None) -> int:
    from PIL import Image
    from .inference import build_model
    opt = parse(argv)
    script = load_script(opt.edit_script)
    model = build_model(opt)
    rng = generator = None
    if opt.seed is not None:
        rng = _random.Random(opt.seed)
        generator = torch.Generator(device=next(model.parameters()).device)
        generator.manual_seed(opt.seed)
    session = open_session(opt, model, opt.tag, opt.ref, rng=rng, generator=generator)
    result, orient_picture = session.edit(script["mask_points"], script["size_points"], bool(script["use_ref_mask"]), bool(script["use_ref_orient"]))
    os.makedirs(opt.out, exist_ok=True)
    stem = os.path.join(opt.out, "%s_from_%s" % (opt.tag, opt.ref))
    Image.fromarray(result.cpu().numpy()).save(stem + ".png")
    if orient_picture is not None:
        Image.fromarray(orient_picture.cpu().numpy()).save(stem + "_orient.png")
    session.save_sheet(stem + "_sheet.jpg")
    print("edited %s with the appearance of %s (%s mask, %s orientation%s) -> %s" % (
        opt.tag, opt.ref, "original" if script["use_ref_mask"] else "edited", "reference" if script["use_ref_orient"] else "stroke",
        ", reconstruction as the target" if session.used_recon else "", stem + ".png"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
