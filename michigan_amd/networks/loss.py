"""Losses that consume the hot path's outputs (reference: models/networks/loss.py:19-207).

Reductions run in fp32 on whatever dtype the discriminator / VGG towers produced, as fused HIP launches: the hinge GAN
loss with its wide-edge weight mask (mg_hinge_*, mg_wide_edge_weight), discriminator feature matching and the VGG taps
(mg_l1_mean_*), the orientation loss under either filter bank (mg_gabor_argmax_*, then mg_orient_loss_* / mgl_orient_dog_*), and the image-space Lab colour / background / RGB L1
terms as one pass (mg_color_loss_*), the unpaired stage's hair-average Lab term (mg_hair_lab_*, fused with the background
term in the model), and the style / content terms as fused feature-moment passes over the VGG taps (mg_feat_moment_loss_*).  Under
--balance_Lab the two Lab terms take the histogram weighting as one more operand of the same passes (mgc_*_balanced_*, LabBalance).
Under michigan_amd.dropin style / content stay the reference's own class."""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .architecture import VGG19


class GANLoss(nn.Module):
    def __init__(self, gan_mode, target_real_label=1.0, target_fake_label=0.0, tensor=torch.FloatTensor, opt=None):
        super().__init__()
        if gan_mode not in ("ls", "original", "w", "hinge"):
            raise ValueError("Unexpected gan_mode {}".format(gan_mode))
        self.gan_mode, self.opt = gan_mode, opt
        self.real_label, self.fake_label = target_real_label, target_fake_label

    def get_wide_edges(self, t, th=0.06):
        h, w = t.shape[2], t.shape[3]
        k = max(1, int(h * th))
        p = int(k / 2)
        grown = F.max_pool2d(t, kernel_size=k, stride=1, padding=p)
        shrunk = 1 - F.max_pool2d(1 - t, kernel_size=k, stride=1, padding=p)
        return F.interpolate(grown - shrunk, size=(h, w), mode="nearest")

    def get_weight_mask(self, input, mask):
        label = F.interpolate(mask, size=input.shape[2:], mode="nearest")
        edges = self.get_wide_edges(label)
        return edges * self.opt.wide_edge + (1 - edges)

    def weight_mask(self, input, label):
        """get_weight_mask (loss.py:82-89) for one logit resolution as ONE HIP launch (index work on a 67x67 / 35x35 map)."""
        # the mask depends on the label and the logit resolution only: D's fake and real terms of one step share it
        src = self.__dict__.get("_mg_label_src")
        if src is None or src.data_ptr() != label.data_ptr():
            src = label
        owner = src._base if src._base is not None else src
        key = (id(owner), label.data_ptr(), label._version if not label.is_inference() else -1, tuple(label.shape), tuple(label.stride()),
               input.shape[2], input.shape[3], float(self.opt.wide_edge))
        cache = self.__dict__.setdefault("_mg_wide_edge", {})
        hit = cache.get(key)
        if hit is not None and hit[0]() is owner:
            return hit[1]
        wm = ops.wide_edge_weight(label, input.shape[2], input.shape[3], self.opt.wide_edge)
        if len(cache) >= 8:
            cache.clear()
        import weakref
        cache[key] = (weakref.ref(owner), wm)
        return wm

    def loss(self, input, target_is_real, for_discriminator=True, label=None):
        if self.gan_mode == "original":
            input = input.float()
            target = torch.full_like(input, self.real_label if target_is_real else self.fake_label)
            return F.binary_cross_entropy_with_logits(input, target)
        if self.gan_mode == "ls":
            input = input.float()
            target = torch.full_like(input, self.real_label if target_is_real else self.fake_label)
            return F.mse_loss(input, target)
        if self.gan_mode == "w":
            input = input.float()
            return -input.mean() if target_is_real else input.mean()
        if getattr(self.opt, "remove_background", False):
            input = input.float()
            c = input.shape[1]
            lab = F.interpolate(label, size=input.shape[2:], mode="nearest")
            denom = lab.sum() * c + 1e-5
            if not for_discriminator:
                assert target_is_real, "The generator's hinge loss must be aiming for real"
                return -(input * lab).sum() / denom
            margin = ((input - 1) if target_is_real else (-input - 1)) * lab
            return -torch.clamp_max(margin, 0).sum() / denom
        # hinge (loss.py:96-111): one fused launch per logit map (+ one per batch and resolution for the weight mask)
        fused = input.dtype in (torch.float32, torch.bfloat16) and (input.shape[1] == 1 or input.is_contiguous())
        if not for_discriminator:
            assert target_is_real, "The generator's hinge loss must be aiming for real"
            return ops.hinge_loss(input, None, ops.HINGE_G) if fused else -input.float().mean()
        if fused and (self.opt.wide_edge <= 1.0 or input.shape[1] == 1):
            wm = self.weight_mask(input, label) if self.opt.wide_edge > 1.0 else None
            return ops.hinge_loss(input, wm, ops.HINGE_D_REAL if target_is_real else ops.HINGE_D_FAKE)
        input = input.float()
        margin = torch.clamp_max((input - 1) if target_is_real else (-input - 1), 0)
        if self.opt.wide_edge > 1.0:
            margin = margin * self.get_weight_mask(input, label)
        return -margin.mean()

    def __call__(self, input, target_is_real, for_discriminator=True, label=None):
        self.__dict__["_mg_label_src"] = label                     # identity of the caller's tensor (detach() below makes a new object per call)
        label = label.detach().float() if label is not None else None
        if not isinstance(input, list):
            return self.loss(input, target_is_real, for_discriminator, label)
        vals = []
        for pred in input:
            pred = pred[-1] if isinstance(pred, list) else pred
            vals.append(self.loss(pred, target_is_real, for_discriminator, label))
        if all(v.numel() == 1 for v in vals):                      # every mode here reduces to a scalar per scale: mean over the scales
            return ops.weighted_sum(vals, [1.0 / len(vals)] * len(vals)).reshape(1)     # [1], like the reference's view(bs, -1).mean(dim=1)
        total = 0
        for val in vals:
            bs = 1 if val.dim() == 0 else val.size(0)
            total = total + val.view(bs, -1).mean(dim=1)
        return total / len(input)


class GANFeatLoss(nn.Module):
    """L1 between the discriminator's intermediate features of fake and real, weight lambda_feat / num_D."""

    def __init__(self, opt=None):
        super().__init__()
        self.opt = opt

    def L1_loss_mask(self, input, target, label):
        lab = F.interpolate(label, size=input.shape[2:], mode="nearest")
        return (input * lab - target * lab).abs().sum() / (lab.sum() * input.shape[1] + 1e-5)

    def forward(self, pred_fake, pred_real, label=None):
        num_d = len(pred_fake)
        vals = []
        for i in range(num_d):
            for j in range(len(pred_fake[i]) - 1):
                a, b = pred_fake[i][j], pred_real[i][j].detach()
                stacked = getattr(a, "_mg_stacked", None)
                if stacked is None or getattr(pred_real[i][j], "_mg_stacked", None) is not stacked:
                    stacked = None
                if getattr(self.opt, "remove_background", False):
                    val = self.L1_loss_mask(a.float(), b.float(), label.detach().float())
                elif stacked is not None:
                    val = ops.l1_mean_halves(stacked)             # fake and real are the two halves of one feature map
                else:
                    val = ops.l1_mean(a, b)
                vals.append(val)
        if not vals:
            return pred_fake[0][0].new_zeros(1, dtype=torch.float32)
        return ops.weighted_sum(vals, [self.opt.lambda_feat / num_d] * len(vals)).reshape(1)


class VGGLoss(nn.Module):
    """Weighted L1 over the five VGG19 taps of x and (detached) y."""

    def __init__(self, opt=None, vgg=None):
        super().__init__()
        self.vgg = vgg if vgg is not None else VGG19()
        if torch.cuda.is_available():
            self.vgg = self.vgg.cuda()
        self.weights = [1.0 / 32, 1.0 / 16, 1.0 / 8, 1.0 / 4, 1.0]
        self.opt = opt

    def L1_loss_mask(self, input, target, label):
        lab = F.interpolate(label, size=input.shape[2:], mode="nearest")
        return F.l1_loss(input * lab, target * lab, reduction="sum") / (lab.sum() * input.shape[1] + 1e-5)

    def forward(self, x, y, label=None, y_feats=None, x_feats=None):
        """`y_feats`: the (detached) tower features of y when the caller already has them (model.py computes them on the side stream);
        `x_feats`: the tower features of x, with their graph, when the style / content terms share the pass."""
        if y_feats is None:
            with torch.no_grad():
                y_feats = self.vgg(y)
        if x_feats is None:
            x_feats = self.vgg(x)
        vals = []
        for a, b in zip(x_feats, y_feats):
            if getattr(self.opt, "remove_background", False):
                vals.append(self.L1_loss_mask(a.float(), b.detach().float(), label.detach().float()))
            else:
                vals.append(ops.l1_mean(a, b))
        return ops.weighted_sum(vals, self.weights[:len(vals)])


class L1OLoss(nn.Module):
    """Orientation loss (reference: loss.py:274-385): the dominant orientation of the generated image -- arg-max over 32 oriented
    filter responses of its gray version, weighted by a confidence -- must match the orientation label inside the hair mask.  The mode
    rule is the reference's: 'gabor' in opt.orient_filter selects the Gabor bank with a tanh confidence, anything else the
    difference-of-Gaussians bank that made the dataset's labels, whose confidence is the masked response divided by its maximum over the
    whole batch (one process per GPU: the rank's own maximum, like a DataParallel replica of the reference).  The filter bank, clamp,
    max and arg-max are one HIP launch (ops.gabor_argmax, any 32 x 17 x 17 bank); everything behind it is one fused reduction per mode."""

    def __init__(self, opt, channel_in=1, channel_out=1, stride=1, padding=8):
        super().__init__()
        self.opt = opt
        self.mode = getattr(opt, "orient_filter", "gabor")
        self.numKernels, self.kernel_size = 32, 17
        self.register_buffer("bank", ops.gabor_bank() if "gabor" in self.mode else ops.dog_bank(), persistent=False)

    def forward(self, fake_image0, orientation_label0, input_semantics):
        img = fake_image0.permute(0, 2, 3, 1)                       # zero-copy for the generator's NHWC output
        conf_raw, idx = ops.gabor_argmax(img, self.bank.to(img.device))
        gabor = "gabor" in self.mode
        # everything behind the arg-max -- the confidence, (sin 2a, cos 2a) of the winning filter, the masked L1 against the label,
        # the confidence term -- is one fused reduction (mg_orient_loss_* / mgl_orient_dog_*): ~45 launches of single-channel maps per step before
        if (not self.opt.use_ig) == (orientation_label0.shape[1] == 1) and orientation_label0.shape[1] in (1, 2):
            tail = ops.orient_loss if gabor else ops.orient_loss_dog
            orient_loss, confidence_loss = tail(conf_raw, idx, orientation_label0, input_semantics.detach()[:, 1])
            return orient_loss, confidence_loss
        hair = input_semantics[:, 1:2].float()
        if gabor:
            confidence = ((torch.tanh(conf_raw) + 1) / 2.0).unsqueeze(1)
        else:
            confidence = conf_raw.unsqueeze(1) * hair
            confidence = confidence / torch.max(confidence)
            confidence = confidence * (~(confidence <= 0)).float()
        ang = (idx.float() * (math.pi / self.numKernels)).unsqueeze(1)
        orient_fake = torch.cat([torch.sin(2 * ang), torch.cos(2 * ang)], dim=1) * confidence
        if not self.opt.use_ig:
            lab = orientation_label0.float() / 255 * math.pi
            orient_label = torch.cat([torch.sin(2 * lab), torch.cos(2 * lab)], dim=1)
        else:
            orient_label = orientation_label0.float()
        orient_loss = F.l1_loss(orient_fake * hair, (orient_label * hair).detach())
        if gabor:
            conf = torch.clamp(confidence, 0.001, 1)
            confidence_loss = -torch.sum(torch.log(conf) * hair) / torch.sum(hair)
        else:
            confidence_loss = torch.sum(torch.abs(confidence * hair - hair.detach())) / (torch.sum(hair) + 1e-5)
        return orient_loss, confidence_loss


def _image_nhwc(fake):
    """The generated image as the kernels read it: the generator's NHWC-backed NCHW view is aliased (zero-copy), a plain
    contiguous NCHW image costs one permute().contiguous()."""
    if fake.dtype not in (torch.float32, torch.bfloat16):
        fake = fake.float()
    return fake.permute(0, 2, 3, 1)


class RGBBackgroundL1Loss(nn.Module):
    """L1 between the generated and the target image outside the hair region (reference: loss.py:388-400): mean over
    N*3*H*W of |fake * m - image * m|, m = channel 0 of the one-hot label; not divided by the area of m."""

    def forward(self, fake, input_semantics, image_tag):
        return ops.color_losses(_image_nhwc(fake), image_tag, input_semantics.detach()[:, 0], ops.COLOR_BACKGROUND)[2]


class LabBalance:
    """The weight table of --balance_Lab (cal_weight, loss.py:484-507 and 578-600): the histogram of hair colours over the a/b plane that
    `opt.weight_dir` names (the reference's data/ab_count.npy, 256 x 256 counts) is loaded ONCE, here -- the reference reloads it on every
    call -- and turned into the fp32 table by ops.lab_weight_table with the cap `opt.Lab_weight_th` (default 10) on the device of the
    first call.  One instance may serve both Lab criteria."""

    def __init__(self, opt):
        import numpy as np
        path = getattr(opt, "weight_dir", None)
        if not path:
            raise NotImplementedError("balance_Lab: this package ships no histogram of hair colours: --weight_dir (the reference's "
                                      "data/ab_count.npy; an .npz archive of that one array is taken as well) is required")
        raw = np.load(path)
        if hasattr(raw, "files"):                                 # an .npz archive with one array
            raw = raw[raw.files[0]]
        self.th = float(getattr(opt, "Lab_weight_th", 10.0))
        self.host = ops.lab_weight_table(raw, self.th)
        self._tables = {}

    @classmethod
    def of(cls, opt, shared=None):
        """`shared` if given, a new table under opt.balance_Lab, else None."""
        if shared is not None:
            return shared
        return cls(opt) if getattr(opt, "balance_Lab", False) else None

    def table(self, device):
        device = torch.device(device)
        t = self._tables.get(device)
        if t is None:
            t = self._tables[device] = self.host.to(device)
        return t


class LabColorLoss(nn.Module):
    """L1 between the a and b channels of the generated and the target image in CIE Lab (reference: loss.py:403-532,
    the rgb2xyz / xyz2lab route; L is not part of the loss).  Under `opt.balance_Lab` a pixel's term is weighted by the table entry of
    the target pixel's colour times `mask` (the hair plane [N, 1, H, W]; its value multiplies), 1 where that is 0 (LabBalance;
    `balance`: an instance to share)."""

    def __init__(self, opt, balance=None):
        super().__init__()
        self.balance = LabBalance.of(opt, balance)
        self.opt = opt

    def forward(self, fake, real, mask=None):
        if self.balance is None:
            return ops.color_losses(_image_nhwc(fake), real, None, ops.COLOR_LAB)[0]
        if mask is None:
            raise ValueError("LabColorLoss: under balance_Lab the hair mask [N, 1, H, W] is needed")
        return ops.color_losses(_image_nhwc(fake), real, None, ops.COLOR_LAB, hair=mask.detach()[:, 0], table=self.balance.table(fake.device))[0]


class HairAvgLabLoss(nn.Module):
    """L1 between the mean Lab (a, b) colour of the generated hair inside `mask_fake` and of the reference image's hair inside
    `mask_real`, one pair of means per sample (reference: loss.py:534-621; masks [N, 1, H, W], their values multiply; an empty
    mask divides by 1).  Under `opt.balance_Lab` sample n's term is weighted by the table entry of the reference's mean hair colour
    (LabBalance; `balance`: an instance to share); a zero of the table is a weight of 0 here."""

    def __init__(self, opt, balance=None):
        super().__init__()
        self.balance = LabBalance.of(opt, balance)
        self.opt = opt

    def forward(self, fake, real, mask_fake, mask_real):
        table = self.balance.table(fake.device) if self.balance is not None else None
        return ops.hair_lab_losses(_image_nhwc(fake), real, mask_fake.detach()[:, 0], mask_real.detach()[:, 0], flags=ops.HAIR_LAB, table=table)[0]


class StyleContentLoss(nn.Module):
    """Content and style terms of the generator objective (reference: loss.py:624-711): `forward` returns (loss_c, loss_s) like the
    reference.  Content is the mean squared error between the relu5_1 features of the generated and of the content image; style sums,
    over the five VGG19 taps, the MSE of the per-(sample, channel) means plus the MSE of the standard deviations of the generated and
    the style image's features.  One fused pass per tap (ops.feat_moment_loss).

    Under `opt.remove_background` the labels [N, 1, H, W] are resized to each tap with nearest sampling and their VALUE multiplies.
    loss.py:692-693 is reproduced literally: the FAKE features' moments are taken under the STYLE label and the style features' under
    the CONTENT label (the reference passes `style_label` to the first operand of calc_style_loss, which is the fake tap); the content
    term is taken under the content label.

    `vgg`: a tower to share (the reference owns a second one with the same pretrained weights).  `fake_feats` / `content_feats`: the
    tower's features of fake_image (with their graph) / content_image when the caller already has them; `masks`: the resized labels
    `resized_labels` returned for these inputs (they depend on the inputs alone: the model builds them once per step)."""

    def __init__(self, opt=None, vgg=None):
        super().__init__()
        if vgg is not None:
            self.__dict__["vgg"] = vgg                            # shared with its owner (VGGLoss): not registered a second time
        else:
            self.vgg = VGG19()
            if torch.cuda.is_available():
                self.vgg = self.vgg.cuda()
        self.opt = opt

    @staticmethod
    def resized_labels(style_label, content_label, sizes):
        """[(style plane, content plane) fp32 [N, h, w]] for every (h, w) of `sizes`: F.interpolate(label, size, mode='nearest')."""
        out = []
        for size in sizes:
            out.append(tuple(F.interpolate(lab.detach().float(), size=size, mode="nearest")[:, 0] for lab in (style_label, content_label)))
        return out

    def forward(self, fake_image, style_image, content_image, style_label=None, content_label=None, fake_feats=None, content_feats=None,
                masks=None, style=True, content=True):
        if fake_feats is None:
            fake_feats = self.vgg(fake_image)
        last = len(fake_feats) - 1
        with torch.no_grad():
            style_feats = self.vgg(style_image) if style else None
            if content and content_feats is None:
                content_feats = self.vgg(content_image)
        if getattr(self.opt, "remove_background", False) and masks is None:
            masks = self.resized_labels(style_label, content_label, [f.shape[2:] for f in fake_feats])
        loss_c, vals = 0, []
        for i, x in enumerate(fake_feats):
            flags = (ops.FEAT_STYLE if style else 0) | (ops.FEAT_CONTENT if content and i == last else 0)
            if not flags:
                continue
            m_style, m_content = masks[i] if masks is not None else (None, None)
            s, c = ops.feat_moment_loss(x, style_feats[i] if style else None, content_feats[i] if flags & ops.FEAT_CONTENT else None,
                                        m_style, m_content, m_content, flags=flags)
            if flags & ops.FEAT_STYLE:
                vals.append(s)
            if flags & ops.FEAT_CONTENT:
                loss_c = c
        loss_s = ops.weighted_sum(vals, [1.0] * len(vals)) if vals else 0
        return loss_c, loss_s
