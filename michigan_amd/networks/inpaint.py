"""The frozen orientation in-painting network (`--use_ig`): inference only.

Reference: models/networks/generator.py:450-575 (`ResnetBlock`, `SelfAttention`, `InpaintGenerator`, skips=False), :577-665
(`SInpaintGenerator`, the same body on five input channels) and their callers models/pix2pix_model.py:407-464.  Parameters, buffers and nn.Sequential indices are the reference's, so its
`InpaintingModel_gen.pth` checkpoints load unchanged.  The network runs at 256x256 without gradients:
7x7 / 4x4-stride-2 / dilated 3x3 / transposed 4x4 convolutions on the MFMA tap-list kernels (the transposed ones as
per-parity-class gathers), InstanceNorm(+ReLU/LeakyReLU) on the fused norm kernels, reflection padding on the gather
kernel; the self-attention over the 4096 positions is one flash-style MFMA kernel (ops.self_attention, csrc/mg_attention.hip:
QK^T -> online softmax -> PV per 128-query workgroup, the [4096, 4096] score matrix never exists).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops
from .base_network import BaseNetwork
from .layers import HipConv2d


def _frozen_weight(m: nn.Module) -> torch.Tensor:
    """The weight an eval-mode forward of `m` would use, computed ONCE per weight state.  torch's spectral_norm pre-hook recomputes
    sigma = u . (W v) and W / sigma at every forward (eval mode: no power iteration, generator.py:452-461 via nn.utils.spectral_norm)
    -- for the frozen in-painting net that was ~60 rocBLAS gemv + ~60 dot + ~80 weight re-packs per training step for values that
    never change.  The result is a non-trainable Parameter, so ops.pack_weight's version-keyed cache keeps its GEMM image too."""
    wo = getattr(m, "weight_orig", None)
    if wo is None:
        return m.weight
    key = (wo.data_ptr(), wo._version, m.weight_u._version, m.weight_v._version, wo.device, wo.dtype)
    hit = m.__dict__.get("_mg_frozen")
    if hit is not None and hit[0] == key:
        return hit[1]
    w = None
    for hook in m._forward_pre_hooks.values():
        if hasattr(hook, "compute_weight"):                       # torch.nn.utils.spectral_norm.SpectralNorm
            with torch.no_grad():
                w = hook.compute_weight(m, do_power_iteration=False)
    if w is None:
        raise RuntimeError("spectral-normed module without its spectral_norm hook")
    w = nn.Parameter(w.detach().clone(), requires_grad=False)
    m.__dict__["_mg_frozen"] = (key, w)
    return w


class InferConv2d(nn.Conv2d):
    """nn.Conv2d parameters, inference-only forward (any dilation) on NHWC."""

    def forward(self, x, act=ops.ACT_NONE, slope=0.2, weight=None):
        if self.padding_mode != "zeros" or self.groups != 1 or self.kernel_size[0] != self.kernel_size[1]:
            raise NotImplementedError("InferConv2d: zero padding, groups 1, square kernels only")
        return ops.conv2d_infer(x, self.weight if weight is None else weight, self.bias, stride=self.stride[0], padding=self.padding[0],
                                dilation=self.dilation[0], act=act, slope=slope)

    def infer(self, x, act=ops.ACT_NONE, slope=0.2):
        """forward() of the frozen net: in eval mode the (spectral-normed) weight comes from _frozen_weight and the module's pre-hooks
        are not run; in training mode this is an ordinary call."""
        if self.training:
            return self(x, act=act, slope=slope)
        return InferConv2d.forward(self, x, act=act, slope=slope, weight=_frozen_weight(self))


class InferConvTranspose2d(nn.ConvTranspose2d):
    """nn.ConvTranspose2d parameters ([Cin, Cout, k, k]; spectral_norm picks dim=1 for this class, as in the
    reference), inference-only forward on NHWC."""

    def forward(self, x, weight=None):
        if self.output_padding != (0, 0) or self.groups != 1 or self.dilation != (1, 1):
            raise NotImplementedError("InferConvTranspose2d: no output padding / groups / dilation")
        return ops.conv_transpose2d_infer(x, self.weight if weight is None else weight, self.bias, stride=self.stride[0], padding=self.padding[0])

    def infer(self, x):
        if self.training:
            return self(x)
        return InferConvTranspose2d.forward(self, x, weight=_frozen_weight(self))


def _sn(m):
    return nn.utils.spectral_norm(m)


class ResnetBlock(nn.Module):
    """x + IN(conv3x3(reflpad1(relu(IN(conv3x3_dil2(reflpad2(x)))))))  (generator.py:450-464)."""

    def __init__(self, dim):
        super().__init__()
        self.conv_block = nn.Sequential(
            nn.ReflectionPad2d(2), _sn(InferConv2d(dim, dim, 3, stride=1, padding=0, dilation=2)), nn.InstanceNorm2d(dim),
            nn.ReLU(True), nn.ReflectionPad2d(1), _sn(InferConv2d(dim, dim, 3, stride=1, padding=0)), nn.InstanceNorm2d(dim))

    def forward(self, x):                                   # NHWC
        cb = self.conv_block
        y = cb[1].infer(ops.reflect_pad(x, 2))
        y = ops.instance_norm_act_infer(y, act=ops.ACT_RELU)
        y = cb[5].infer(ops.reflect_pad(y, 1))
        return ops.instance_norm_act_infer(y, act=ops.ACT_NONE, resid=x)          # x + IN(...): the skip rides in the apply launch


class SelfAttention(nn.Module):
    """cat([x, V softmax(Q^T K)^T]) over the H*W positions (generator.py:467-486); 1x1 projections on the conv kernels."""

    def __init__(self, dim, downsample=4):
        super().__init__()
        self.query_conv = InferConv2d(dim, dim // downsample, 1)
        self.key_conv = InferConv2d(dim, dim // downsample, 1)
        self.value_conv = InferConv2d(dim, dim, 1)
        self.softmax = nn.Softmax(dim=-1)

    def forward(self, x):                                   # NHWC
        n, h, w, c = x.shape
        q = self.query_conv.infer(x).reshape(n, h * w, -1)
        k = self.key_conv.infer(x).reshape(n, h * w, -1)
        v = self.value_conv.infer(x).reshape(n, h * w, c)
        y = torch.empty((n, h, w, 2 * c), dtype=x.dtype, device=x.device)     # [x | attention] (generator.py:485), written in place
        y[..., :c] = x
        ops.self_attention(q, k, v, out=y.reshape(n, h * w, 2 * c)[:, :, c:])
        return y


class InpaintGenerator(BaseNetwork):
    """The frozen in-painting body; `in_channels` is what the first convolution reads: 4 (RGB-coded orientation + hole) here, 5 in
    SInpaintGenerator (+ the stroke mask)."""
    in_channels = 4

    def __init__(self, opt, blocks=12, skips=False):
        super().__init__()
        if skips:
            raise NotImplementedError("%s: the skip-connection variant is not used by the reference's options" % type(self).__name__)
        self.skips = skips
        self.encoder = nn.Sequential(
            nn.ReflectionPad2d(3), _sn(InferConv2d(self.in_channels, 64, 7, padding=0)), nn.InstanceNorm2d(64), nn.LeakyReLU(0.2, True),
            _sn(InferConv2d(64, 128, 4, stride=2, padding=1)), nn.InstanceNorm2d(128), nn.LeakyReLU(0.2, True),
            _sn(InferConv2d(128, 256, 4, stride=2, padding=1)), nn.InstanceNorm2d(256), nn.LeakyReLU(0.2, True))
        self.middle = nn.Sequential(*[ResnetBlock(256) for _ in range(blocks)], SelfAttention(256))
        self.decoder = nn.Sequential(
            _sn(InferConvTranspose2d(512, 128, 4, stride=2, padding=1)), nn.InstanceNorm2d(128), nn.ReLU(True),
            _sn(InferConvTranspose2d(128, 64, 4, stride=2, padding=1)), nn.InstanceNorm2d(64), nn.ReLU(True),
            nn.ReflectionPad2d(3), InferConv2d(64, 3, 7, padding=0))

    @torch.no_grad()
    def forward(self, x):                                   # NCHW [N, in_channels, H, W] -> NCHW [N, 3, H, W] in [0, 1]
        return self.forward_nhwc8(ops.pad_channels(ops.to_nhwc(x, self.compute_dtype), 8))

    @torch.no_grad()
    def forward_nhwc8(self, y):
        """The same on an input already in the kernels' layout: [N, H, W, 8] in the compute dtype, channels in_channels .. 7 zero
        (what ops.stroke_compose writes)."""
        if y.dim() != 4 or y.shape[-1] != 8 or y.dtype != self.compute_dtype:
            raise ValueError("%s.forward_nhwc8: expected [N,H,W,8] %s, got %s %s" % (type(self).__name__, self.compute_dtype, tuple(y.shape), y.dtype))
        e, d = self.encoder, self.decoder
        y = ops.instance_norm_act(e[1].infer(ops.reflect_pad(y, 3)), act=ops.ACT_LRELU, slope=0.2)
        y = ops.instance_norm_act(e[4].infer(y), act=ops.ACT_LRELU, slope=0.2)
        y = ops.instance_norm_act(e[7].infer(y), act=ops.ACT_LRELU, slope=0.2)
        y = self.middle(y)
        y = ops.instance_norm_act(d[0].infer(y), act=ops.ACT_RELU)
        y = ops.instance_norm_act(d[3].infer(y), act=ops.ACT_RELU)
        y = d[7].infer(ops.reflect_pad(y, 3), act=ops.ACT_TANH)
        return (ops.to_nchw(y).float()[:, :3] + 1) / 2


class SInpaintGenerator(InpaintGenerator):
    """The stroke in-painting net (`--use_stroke`, `--netSIG sinpaint`; generator.py:577-665): the same body on five input channels
    (RGB-coded orientation, hole, stroke mask), so the reference's SInpaintingModel_gen.pth loads unchanged."""
    in_channels = 5
