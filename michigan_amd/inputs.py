"""The input pipeline on the device.

The reference prepares every sample on loader worker processes with PIL / numpy / cv2
(data/pix2pix_dataset.py:66-194, data/base_dataset.py:335-456) and `Pix2PixModel.preprocess_input`
(models/pix2pix_model.py:209-254) one-hot encodes on the GPU with scatter_.  At 8 x ~90 images/s the
`nThreads` CPU workers cannot keep up (generate_noise alone is seven cv2.resize calls per sample), so the
same arithmetic runs here as HIP kernels of libmichigan_hip.so on u8 maps that were uploaded once:

    crop_u8            get_transform's Resize(NEAREST) + crop + flip + ToTensor (+ Normalize / "* 255")
    onehot_labels      preprocess_input's zeros().scatter_(1, label.long(), 1.0)
    orient_to_rgb_u8   trans_orient_to_rgb
    generate_hole_u8   generate_hole
    generate_noise     generate_noise (multi-octave, cv2.resize INTER_LINEAR)
    resize_bicubic_u8  get_transform's Resize(BICUBIC) for images (Pillow's 8-bit resampler)
    dense_orientation  cal_orientation.py: the uint8 orientation map itself, from an image and its hair mask
    stroke_to_orient   ui_util/cal_orient_stroke.py: the RGB-coded orientation picture of a drawn stroke mask
    stroke_inputs      demo_inference_dataLoad's orient_stroke / mask_stroke / hole tensors (base_dataset.py:214-238)
    brush_u8           demo.py:431-435: the recorded pen segments painted onto a u8 map (the package's own capsule brush)
    dilate_u8 / erode_u8 / stroke_hole   cv2.dilate / cv2.erode with any element; demo.py:323-324, the stroke widened into its hole

`DeviceInputPipeline` strings them together into the `data` dict of pix2pix_dataset.py:178-188 (paired, and with image_ref /
label_ref the unpaired stage's), `inference_batch` into single_inference_dataLoad's (base_dataset.py:49-160) and `demo_batch` into
demo_inference_dataLoad's (:162-276): every mode Pix2PixModel.forward accepts has its loader here.  The three are compositions of
the entry points above -- a kernel fused over one batch kind would need an entry point of its own.  The random
DRAWS stay on the host and follow the reference (random.randint / random.random / random.uniform of a
`random.Random`); only the Gaussian noise fields come from the device generator.  There is no CPU path:
every function goes through the C ABI (`_cabi.backend()`), which raises if the library is missing.
"""
from __future__ import annotations

import ctypes
import random as _random
from typing import Dict, Optional

import torch

from . import _cabi as C


def _p(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(t: torch.Tensor):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream) if t.is_cuda else None


def _u8(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.uint8:
        raise TypeError("expected a uint8 tensor (decoded image / label bytes)")
    return t.contiguous()


def upload(t: torch.Tensor, device) -> torch.Tensor:
    """A small host tensor (a batch's draws, its sample indices) on `device` WITHOUT draining the stream: a plain `.to(device)` from
    pageable memory synchronises the stream it copies on, so a loader that runs once per training step would wait for the whole
    previous step at its first draw.  Through pinned memory the copy is one more entry of the stream."""
    device = torch.device(device)
    if device.type != "cuda" or t.is_cuda:
        return t.to(device)
    return t.pin_memory().to(device, non_blocking=True)


def nearest_table(src: int, dst: int, device) -> Optional[torch.Tensor]:
    """Pillow's nearest-neighbour source index for each of `dst` output coordinates (None = identity)."""
    if src == dst:
        return None
    host = torch.empty(dst, dtype=torch.int32)
    C.backend().mg_nearest_table(src, dst, _p(host))
    return host.to(device)


def orient_rgb_table(device) -> torch.Tensor:
    host = torch.empty(256, 3, dtype=torch.float64)
    C.backend().mg_orient_rgb_table(_p(host))
    return host.to(device)


def bicubic_table(in_size: int, out_size: int, device):
    """Pillow's bicubic windows / 22-bit coefficients for one axis: (bounds [out,2], coef [out,k], k) on `device`."""
    be = C.backend()
    k = int(be.mg_bicubic_ksize(in_size, out_size))
    bounds = torch.empty(out_size, 2, dtype=torch.int32)
    coef = torch.empty(out_size, k, dtype=torch.int32)
    be.mg_bicubic_table(in_size, out_size, _p(bounds), _p(coef))
    return bounds.to(device), coef.to(device), k


def resize_bicubic_u8(src: torch.Tensor, size, tables=None) -> torch.Tensor:
    """transforms.Resize(osize, Image.BICUBIC) on u8 images [N,Hs,Ws,C] -> [N,H,W,C] (Pillow-exact, two passes)."""
    src = _u8(src)
    n, hs, ws, c = src.shape
    h, w = (size, size) if isinstance(size, int) else size
    if (h, w) == (hs, ws):
        return src
    xt, yt = tables if tables is not None else (bicubic_table(ws, w, src.device), bicubic_table(hs, h, src.device))
    tmp = torch.empty((n, hs, w, c), dtype=torch.uint8, device=src.device)
    dst = torch.empty((n, h, w, c), dtype=torch.uint8, device=src.device)
    C.backend().mg_resize_bicubic_u8(_p(src), _p(tmp), _p(dst), _p(xt[0]), _p(xt[1]), xt[2], _p(yt[0]), _p(yt[1]), yt[2],
                                     n, hs, ws, h, w, c, _stream(src))
    return dst


def crop_u8(src: torch.Tensor, crop: torch.Tensor, size, *, mode: int, unknown_label: int = -1,
            ytab: Optional[torch.Tensor] = None, xtab: Optional[torch.Tensor] = None,
            mul: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """src u8 [N,Hs,Ws,C] (or [N,Hs,Ws]); crop int32 [N,3] = (x0, y0, flip) -> fp32 [N,C,H,W].
    mode 0: image (ToTensor + Normalize 0.5/0.5); 1: label-like map (`* 255.0`, 255 -> unknown_label);
    2: ToTensor only.  `mul` [N,1,H,W] multiplies all channels.  `out`: a contiguous fp32 [N,C,H,W] on src's device to
    write into (the rows of a larger batch whose samples come from sources of different sizes)."""
    src = _u8(src)
    if src.dim() == 3:
        src = src.unsqueeze(-1)
    n, hs, ws, c = src.shape
    h, w = (size, size) if isinstance(size, int) else size
    if tuple(crop.shape) != (n, 3):
        raise ValueError("crop must be [N, 3] = (x0, y0, flip)")
    crop_host = crop if not crop.is_cuda else None      # the window is validated on the host BEFORE it is uploaded (the draws are made there)
    crop = crop.to(device=src.device, dtype=torch.int32).contiguous()
    if mul is not None:
        mul = mul.to(torch.float32).contiguous()
        if mul.numel() != n * h * w:
            raise ValueError("mul must be [N, 1, H, W]")
    lim_h = hs if ytab is None else ytab.numel()
    lim_w = ws if xtab is None else xtab.numel()
    if crop_host is not None and (int(crop_host[:, 1].max()) + h > lim_h or int(crop_host[:, 0].max()) + w > lim_w or int(crop_host.min()) < 0):
        raise ValueError("crop window outside the (resized) source")
    if out is None:
        out = torch.empty((n, c, h, w), dtype=torch.float32, device=src.device)
    elif tuple(out.shape) != (n, c, h, w) or out.dtype != torch.float32 or out.device != src.device or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous fp32 {(n, c, h, w)} on {src.device}")
    C.backend().mg_input_crop_u8(_p(src), _p(out), _p(crop), _p(ytab), _p(xtab), _p(mul), n, hs, ws, c, h, w,
                                 mode, unknown_label, _stream(src))
    return out


def onehot_labels(label: torch.Tensor, nc: int) -> torch.Tensor:
    """pix2pix_model.py:231-246: label [N,1,H,W] (class index as float or integer) -> fp32 one-hot [N,nc,H,W]."""
    n, one, h, w = label.shape
    if one != 1:
        raise ValueError("label map must have one channel")
    lab = label.to(torch.float32).contiguous()
    out = torch.empty((n, nc, h, w), dtype=torch.float32, device=lab.device)
    C.backend().mg_onehot_labels(_p(lab), _p(out), n, h * w, nc, _stream(lab))
    return out


def orient_to_rgb_u8(orient: torch.Tensor, label: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """base_dataset.py:363-385: u8 orientation + u8 label [N,H,W] -> RGB-coded u8 image [N,H,W,3]."""
    orient, label = _u8(orient), _u8(label)
    out = torch.empty(orient.shape + (3,), dtype=torch.uint8, device=orient.device)
    C.backend().mg_orient_to_rgb_u8(_p(orient), _p(label), _p(table), _p(out), orient.numel(), _stream(orient))
    return out


def generate_hole_u8(mask: torch.Tensor, orient_mask: torch.Tensor, th: torch.Tensor, u: torch.Tensor,
                     want_info: bool = False):
    """base_dataset.py:335-361 for a batch: mask / orient_mask u8 [N,H,W]; th[n] = uniform(0.5, 1.2) draw,
    u[n] in [0,1) picks the centre among orient_mask's non-zero pixels.  Returns u8 [N,H,W] (and the
    int32 [N,4] {nums, centre row, centre column, rr} when want_info)."""
    mask, orient_mask = _u8(mask), _u8(orient_mask)
    n, h, w = mask.shape
    th = th.to(device=mask.device, dtype=torch.float64).contiguous()
    u = u.to(device=mask.device, dtype=torch.float64).contiguous()
    hole = torch.empty_like(mask)
    info = torch.empty((n, 4), dtype=torch.int32, device=mask.device) if want_info else None
    C.backend().mg_generate_hole_u8(_p(mask), _p(orient_mask), _p(th), _p(u), _p(hole), _p(info), n, h, w, _stream(mask))
    return (hole, info) if want_info else hole


def noise_field_len(size: int) -> int:
    return int(C.backend().mg_noise_field_len(size))


def noise_from_fields(fields: torch.Tensor, size: int) -> torch.Tensor:
    """fields float64 [N, noise_field_len(size)] (octaves back to back, each [s,s,3]) -> fp32 [N,3,size,size]."""
    n = fields.shape[0]
    fields = fields.to(torch.float64).contiguous()
    if fields.shape[1] != noise_field_len(size):
        raise ValueError("fields has the wrong length for this size")
    out = torch.empty((n, 3, size, size), dtype=torch.float32, device=fields.device)
    C.backend().mg_noise_octaves(_p(fields), _p(out), n, size, _stream(fields))
    return out


def generate_noise(n: int, size: int, device, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """base_dataset.py:387-396 for a batch: np.random.normal(0.5, 0.25) fields drawn on the device."""
    fields = torch.randn((n, noise_field_len(size)), dtype=torch.float64, device=device, generator=generator) * 0.25 + 0.5
    return noise_from_fields(fields, size)


_DOG_BANKS = {}


def dense_orientation(image: torch.Tensor, mask: torch.Tensor, sigma: float = 4.0, return_angle: bool = False):
    """cal_orientation.py for a batch on the device: the uint8 dense orientation map [N,H,W] of `image` under the hair `mask` --
    what orient_to_rgb_u8, DeviceInputPipeline and the orientation loss read (with return_angle also the fp32 angle in [0, pi]).

    image: fp32 in [-1, 1], [N,3,H,W] or [N,H,W,3], or uint8 RGB in either layout (converted as ToTensor + Normalize(0.5) do, in fp32,
    so that the gray image keeps the reference's roundings).  bf16 is refused: an 8-bit mantissa moves the arg-max over the filters.
    mask: integer or float [N,H,W]; a mask whose maximum is above 1 is thresholded at > 130 (cal_orientation.py:91-92).
    Two launches: mg_gabor_argmax_fwd under ops.dog_bank (calOrientation, lines 60-80), then mg_orient_smooth (lines 101-109)."""
    from . import ops
    if image.dim() != 4 or (image.shape[-1] != 3 and image.shape[1] != 3):
        raise ValueError(f"dense_orientation: image must be [N,3,H,W] or [N,H,W,3], got {tuple(image.shape)}")
    if image.dtype == torch.uint8:
        image = ((image.to(torch.float32) / 255) - 0.5) / 0.5
    elif image.dtype != torch.float32:
        raise ValueError(f"dense_orientation: image must be fp32 or uint8, got {image.dtype} (bf16 moves the arg-max)")
    if image.shape[-1] != 3:
        image = image.permute(0, 2, 3, 1)
    n, h, w, _ = image.shape
    if mask.dim() == 4 and mask.shape[1] == 1:
        mask = mask[:, 0]
    if tuple(mask.shape) != (n, h, w):
        raise ValueError(f"dense_orientation: mask {tuple(mask.shape)} does not match the image's {(n, h, w)}")
    if h <= ops.ORIENT_RADIUS or w <= ops.ORIENT_RADIUS:
        raise ValueError(f"dense_orientation: H and W must be at least {ops.ORIENT_RADIUS + 1}, got {h} x {w}")
    ops.gaussian_taps(sigma)                                              # refuses sigma before anything is launched
    mask = mask.to(image.device)
    hair = ((mask > 130) if float(mask.max()) > 1 else (mask != 0)).to(torch.uint8)
    dev = str(image.device)
    if dev not in _DOG_BANKS:
        _DOG_BANKS[dev] = ops.dog_bank(image.device)
    with torch.no_grad():
        conf, idx = ops.gabor_argmax(image.contiguous(), _DOG_BANKS[dev])
    return ops.orient_smooth(conf, idx, hair, sigma=sigma, want_angle=return_angle)


def _stroke_mask_u8(mask_stroke: torch.Tensor) -> torch.Tensor:
    """[N,H,W] / [H,W] / [N,1,H,W] of any integer or float dtype -> uint8 [N,H,W], np.uint8's truncation for float maps"""
    m = mask_stroke
    if m.dim() == 2:
        m = m.unsqueeze(0)
    if m.dim() == 4 and m.shape[1] == 1:
        m = m[:, 0]
    if m.dim() != 3:
        raise ValueError(f"a stroke mask must be [H,W], [N,H,W] or [N,1,H,W], got {tuple(mask_stroke.shape)}")
    if m.dtype == torch.bfloat16 or m.dtype == torch.float16:
        raise ValueError(f"a stroke mask must be an integer, fp32 or fp64 map, got {m.dtype}")
    return m.to(torch.uint8).contiguous()


def stroke_to_orient(mask_stroke: torch.Tensor) -> torch.Tensor:
    """np.uint8(orient().stroke_to_orient(m)) (ui_util/cal_orient_stroke.py:133-149; demo.py:326) for a batch on the device:
    mask_stroke [N,H,W] (or [H,W], [N,1,H,W]), non-zero = stroke (the reference's masks are in {0, 1}) -> the RGB-coded orientation picture u8 [N,H,W,3], black outside the stroke.
    One launch (mg_stroke_orient); a tile of the canvas without a stroke pixel costs nothing but its zeros."""
    from . import ops
    return ops.stroke_orient(_stroke_mask_u8(mask_stroke))     # non-zero = stroke; nothing is read back: a pen lift does not wait for the device


def stroke_inputs(mask_stroke: torch.Tensor, label_tag: torch.Tensor, mask_hole: Optional[torch.Tensor] = None, *,
                  crop: Optional[torch.Tensor] = None, ytab: Optional[torch.Tensor] = None,
                  xtab: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """The stroke entries of demo_inference_dataLoad's batch (base_dataset.py:214-238) at the size of label_tag [N,1,H,W] (the class
    index map as fp32): orient_stroke [N,3,H,W] = ToTensor(stroke picture) * label_tag, mask_stroke [N,1,H,W] = ToTensor(mask) * 255 *
    label_tag and, when mask_hole is given (the dilated stroke, demo.py:323-324: `stroke_hole` makes it), hole likewise.
    Without `crop` the stroke mask has label_tag's size (the demo works at the crop size).  With `crop` (host int32 [N,3], the loader's
    window) the masks are at their stored size and take transform_label's resize (`ytab` / `xtab`: nearest_table of their height /
    width, None = identity) and crop; the stroke picture is made at the stored size, as the reference makes it (demo.py:325-326)."""
    m = _stroke_mask_u8(mask_stroke)
    n = m.shape[0]
    label = label_tag.to(device=m.device, dtype=torch.float32)
    if label.dim() != 4 or label.shape[:2] != (n, 1) or (crop is None and tuple(label.shape[2:]) != tuple(m.shape[1:])):
        raise ValueError(f"stroke_inputs: label_tag must be {(n, 1) + tuple(m.shape[1:])}, got {tuple(label_tag.shape)}")
    h, w = label.shape[2:]
    if crop is None:
        crop = torch.zeros((n, 3), dtype=torch.int32)                       # no crop, no flip: the demo works at the crop size
    out = {"orient_stroke": crop_u8(stroke_to_orient(m), crop, (h, w), mode=2, ytab=ytab, xtab=xtab, mul=label),
           "mask_stroke": crop_u8(m, crop, (h, w), mode=1, ytab=ytab, xtab=xtab, mul=label)}
    if mask_hole is not None:
        hm = _stroke_mask_u8(mask_hole.to(m.device))
        if hm.shape != m.shape:
            raise ValueError(f"stroke_inputs: mask_hole {tuple(mask_hole.shape)} does not match the stroke mask's {tuple(m.shape)}")
        out["hole"] = crop_u8(hm, crop, (h, w), mode=1, ytab=ytab, xtab=xtab, mul=label)
    return out


def ellipse_element(k_w: int, k_h: Optional[int] = None):
    """cv2.getStructuringElement(cv2.MORPH_ELLIPSE, (k_w, k_h)) restated on the host: a numpy u8 [k_h, k_w] of 0 / 1 (k_h defaults
    to k_w).  OpenCV's published rule: r = k_h // 2, c = k_w // 2; row i, with dy = i - r, is empty when |dy| > r and else set on
    [max(c - dx, 0), min(c + dx + 1, k_w)) for dx = round-half-even(c * sqrt((r^2 - dy^2) / r^2)) in double (r == 0: dx = 0).  Its
    default anchor is (k_w // 2, k_h // 2).  This reproduces the well-known 3 x 3 element (a cross) and the 5 x 5 one (full but for
    the four corners of the first and last row, which hold their middle pixel only).  It COULD NOT be compared with OpenCV on any
    machine of this project (none has it), so larger elements are this formula's, not a recorded cv2 result; a caller that has
    OpenCV may pass its own element to dilate_u8 / erode_u8."""
    import math
    import numpy as np
    kw = int(k_w)
    kh = kw if k_h is None else int(k_h)
    if kw < 1 or kh < 1:
        raise ValueError(f"ellipse_element: bad size {k_w} x {k_h}")
    r, c = kh // 2, kw // 2
    out = np.zeros((kh, kw), np.uint8)
    for i in range(kh):
        dy = i - r
        if abs(dy) <= r:
            dx = int(round(c * math.sqrt((r * r - dy * dy) / (r * r)))) if r else 0      # round(): half to even, as cvRound
            out[i, max(c - dx, 0):min(c + dx + 1, kw)] = 1
    return out


def rect_element(k):
    """cv2.getStructuringElement(cv2.MORPH_RECT, (k, k)) (or (k_w, k_h) for a pair): a numpy u8 array of ones"""
    import numpy as np
    kw, kh = (k, k) if isinstance(k, int) else k
    if int(kw) < 1 or int(kh) < 1:
        raise ValueError(f"rect_element: bad size {k}")
    return np.ones((int(kh), int(kw)), np.uint8)


_ELEMENTS: Dict[tuple, torch.Tensor] = {}
_ELEMENTS_MAX = 16                              # the demo uses two elements; a caller that sweeps elements must not pile up device tensors


def _element_on(element, device) -> torch.Tensor:
    """a structuring element (host numpy / torch u8 [kh,kw], or a device tensor) on `device`: one pinned upload per distinct element,
    the last _ELEMENTS_MAX of them kept"""
    if torch.is_tensor(element) and element.device.type != "cpu":
        return element.to(device)
    import numpy as np
    e = np.ascontiguousarray(element.numpy() if torch.is_tensor(element) else element)
    if e.dtype != np.uint8 or e.ndim != 2 or e.size == 0:
        raise ValueError(f"a structuring element is a uint8 [kh,kw] array, got {e.dtype} {e.shape}")
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:                      # 'cuda' and 'cuda:0' are one device: one entry
        device = torch.device("cuda", torch.cuda.current_device())
    key = (str(device), e.shape, e.tobytes())
    if key not in _ELEMENTS:
        while len(_ELEMENTS) >= _ELEMENTS_MAX:
            _ELEMENTS.pop(next(iter(_ELEMENTS)))                            # the oldest entry (dicts keep insertion order)
        _ELEMENTS[key] = upload(torch.from_numpy(e.copy()), device)
    return _ELEMENTS[key]


def _u8_planes(t: torch.Tensor, name: str) -> torch.Tensor:
    """[H,W] / [N,H,W] / [N,1,H,W] uint8 -> a [N,H,W] view of it (morphology and the brush work on byte maps only)"""
    if not torch.is_tensor(t) or t.dtype != torch.uint8:
        raise ValueError(f"{name}: expected a uint8 map, got {getattr(t, 'dtype', type(t).__name__)}")
    if t.dim() == 2:
        return t.unsqueeze(0)
    if t.dim() == 4 and t.shape[1] == 1:
        return t[:, 0]
    if t.dim() != 3:
        raise ValueError(f"{name}: expected [H,W], [N,H,W] or [N,1,H,W], got {tuple(t.shape)}")
    return t


def _morph(mask: torch.Tensor, element, anchor, op: int, name: str) -> torch.Tensor:
    from . import ops
    m = _u8_planes(mask, name)
    elem = _element_on(element, m.device)
    if anchor is None:
        anchor = (elem.shape[1] // 2, elem.shape[0] // 2)                 # cv2's Point(-1, -1): the element's centre
    return ops.morph_u8(m.contiguous(), elem, anchor, op).view(mask.shape)


def dilate_u8(mask: torch.Tensor, element, anchor=None) -> torch.Tensor:
    """cv2.dilate(mask, element, anchor=anchor) with the default border on the device (one launch of mge_morph_u8): mask u8 [H,W],
    [N,H,W] or [N,1,H,W] of any grey level -> a new map of the same shape.  `element`: a host u8 [kh,kw] array (ellipse_element,
    rect_element, or OpenCV's own), uploaded once per distinct element, at most 64 x 64; `anchor` (x, y), default the centre."""
    from . import ops
    return _morph(mask, element, anchor, ops.MORPH_DILATE, "dilate_u8")


def erode_u8(mask: torch.Tensor, element, anchor=None) -> torch.Tensor:
    """cv2.erode, as dilate_u8 (taps outside the image are left out of the minimum: cv2's default border)."""
    from . import ops
    return _morph(mask, element, anchor, ops.MORPH_ERODE, "erode_u8")


def brush_segments(segments, n: int, h: int, w: int) -> torch.Tensor:
    """The host side of brush_u8: `segments` (a list of rows or an integer array [S,8] / [S,7] = sample, x0, y0, x1, y1, thickness,
    value[, 0]) checked against the ranges of include/michigan_hip/editing/mask_edit.h for an [n,h,w] canvas -> int32 [S,8] on the
    host.  The C entry point cannot read the device list back, so this is where a bad segment is refused."""
    import numpy as np
    from . import ops
    a = np.asarray(segments if len(segments) else np.zeros((0, 8)), dtype=np.int64)
    if a.ndim != 2 or a.shape[1] not in (7, 8):
        raise ValueError(f"brush_u8: segments must be [S,8] = (sample, x0, y0, x1, y1, thickness, value, 0), got {a.shape}")
    if a.shape[1] == 7:
        a = np.concatenate([a, np.zeros((a.shape[0], 1), np.int64)], axis=1)
    if a.shape[0]:
        bad = ((a[:, 0] < 0) | (a[:, 0] >= n) | (np.abs(a[:, 1:5]) > ops.BRUSH_MAX_COORD).any(axis=1) | (a[:, 5] < 1) |
               (a[:, 5] > ops.BRUSH_MAX_THICKNESS) | (a[:, 6] < 0) | (a[:, 6] > 255))
        if bad.any():
            i = int(np.argmax(bad))
            raise ValueError("brush_u8: segment %d %s is outside the accepted ranges (0 <= sample < %d, |x|, |y| <= %d, 1 <= thickness <= %d, "
                             "0 <= value <= 255)" % (i, a[i, :7].tolist(), n, ops.BRUSH_MAX_COORD, ops.BRUSH_MAX_THICKNESS))
    return torch.from_numpy(a.astype(np.int32))


def brush_u8(canvas: torch.Tensor, segments) -> torch.Tensor:
    """demo.py:431-435 (make_mask: one cv2.line per recorded segment) on the device, IN PLACE: canvas u8 [H,W], [N,H,W] or [N,1,H,W],
    contiguous; `segments` as brush_segments takes them, applied in order (a pixel keeps the value of the last segment that covers
    it).  One pinned upload and one launch (mge_brush_u8); no segments, no launch.  The brush is the package's own integer capsule
    (the header states it), not cv2.line's polygon.  Returns the canvas."""
    from . import ops
    m = _u8_planes(canvas, "brush_u8")
    if not canvas.is_contiguous():
        raise ValueError("brush_u8: the canvas is painted in place and must be contiguous")
    segs = brush_segments(segments, *m.shape)
    ops.brush_u8(m, upload(segs, m.device))
    return canvas


def stroke_hole(mask_stroke: torch.Tensor, ksize: int = 50) -> torch.Tensor:
    """demo.py:323-324 as one call: cv2.dilate(np.uint8(mask_stroke), getStructuringElement(MORPH_ELLIPSE, (ksize, ksize))) -- the
    `mask_hole` that stroke_inputs / demo_batch take beside the stroke mask (demo.py:471-472 is ksize=20).  u8 in, u8 out."""
    return dilate_u8(mask_stroke, ellipse_element(ksize))


def _decoded(t, name: str, channels: int, n: Optional[int] = None) -> torch.Tensor:
    """A decoded file for the loaders below: uint8 [N,H,W] or [H,W] (channels == 1), [N,H,W,3] or [H,W,3] (channels == 3), on any
    device.  Returns it with the batch dimension; anything else is a ValueError, raised on the host before anything is uploaded."""
    if not torch.is_tensor(t):
        raise ValueError(f"{name}: expected a uint8 tensor, got {type(t).__name__}")
    if t.dtype != torch.uint8:
        raise ValueError(f"{name}: expected the decoded uint8 bytes, got {t.dtype}")
    want = 2 if channels == 1 else 3
    if t.dim() == want:
        t = t.unsqueeze(0)
    if t.dim() != want + 1 or (channels == 3 and t.shape[-1] != 3) or min(t.shape) < 1:
        raise ValueError(f"{name}: expected {'[N,H,W] or [H,W]' if channels == 1 else '[N,H,W,3] or [H,W,3]'}, got {tuple(t.shape)}")
    if n is not None and t.shape[0] != n:
        raise ValueError(f"{name}: batch of {t.shape[0]}, the other maps have {n}")
    return t


def _same_size(maps: Dict[str, torch.Tensor]):
    """maps that one reference function combines pixel by pixel at their stored size"""
    sizes = {k: tuple(v.shape[1:3]) for k, v in maps.items()}
    if len(set(sizes.values())) > 1:
        raise ValueError("these maps must have one size: %s" % sizes)


def _pad_zeros(t: torch.Tensor, th: int) -> torch.Tensor:
    """pad_zeros (base_dataset.py:28-47) on u8 [N,H,W] / [N,H,W,C]: H + th by W + th, the map int(th / 2) from the top left"""
    o = int(th / 2)
    out = t.new_zeros((t.shape[0], t.shape[1] + th, t.shape[2] + th) + tuple(t.shape[3:]))
    out[:, o:o + t.shape[1], o:o + t.shape[2]] = t
    return out


def _loader_device(tensors) -> torch.device:
    """where inference_batch / demo_batch work: the device of the first map that is on one, else the current device of the backend"""
    for t in tensors:
        if torch.is_tensor(t) and t.is_cuda:
            return t.device
    return torch.device("cuda", torch.cuda.current_device()) if C.backend().name == "hip" else torch.device("cpu")


class DeviceInputPipeline:
    """Pix2pixDataset.__getitem__ (pix2pix_dataset.py:66-194) for a whole batch on the device.  Inputs are the decoded bytes at
    their stored size: images u8 [N,Hs,Ws,3] (bicubic-resized to load size here, Pillow-exact), label / orientation maps u8
    [N,Hs,Ws] (nearest-resized).  Without image_ref / label_ref this is step 1 (the reference is the target); with them it is the
    unpaired stage's batch (step 2, `index_ref` another sample, :75-100).  WHICH sample is the reference, and whose mask
    `orient_mask` is (:124-126), stays the dataset's choice: the caller draws the indices and hands over the decoded files.
    `inference_batch` and `demo_batch` are base_dataset.py's two single-sample loaders on the same launches."""

    def __init__(self, opt, device, rng: Optional[_random.Random] = None, generator: Optional[torch.Generator] = None):
        self.opt, self.device = opt, torch.device(device)
        self.rng = rng if rng is not None else _random.Random()
        self.generator = generator
        self.load_size = int(getattr(opt, "load_size", opt.crop_size))
        self.crop_size = int(opt.crop_size)
        self.flip = bool(getattr(opt, "isTrain", True)) and not bool(getattr(opt, "no_flip", False))
        self.table = orient_rgb_table(self.device)
        self._tabs: Dict[int, Optional[torch.Tensor]] = {}
        self._btabs = {}

    def _tab(self, src: int):
        if src not in self._tabs:
            self._tabs[src] = nearest_table(src, self.load_size, self.device)
        return self._tabs[src]

    def _tabs_for(self, hs: int, ws: int):
        """(ytab, xtab) of a map stored at hs x ws.  mg_input_crop_u8 takes both tables or none, so where one axis is at the load
        size already its identity is written out."""
        yt, xt = self._tab(hs), self._tab(ws)
        if (yt is None) != (xt is None):
            ident = torch.arange(self.load_size, dtype=torch.int32, device=self.device)
            yt, xt = (ident if yt is None else yt), (ident if xt is None else xt)
        return yt, xt

    def draw_params(self, n: int) -> torch.Tensor:
        """get_params (base_dataset.py:398-416), 'resize_and_crop': the same three draws per sample."""
        rows = []
        for _ in range(n):
            x = self.rng.randint(0, max(0, self.load_size - self.crop_size))
            y = self.rng.randint(0, max(0, self.load_size - self.crop_size))
            flip = self.rng.random() > 0.5
            rows.append([x, y, int(flip and self.flip)])
        return torch.tensor(rows, dtype=torch.int32)

    def _window(self, n: int) -> torch.Tensor:
        """the batch's draws, checked on the host, before the upload"""
        crop_h = self.draw_params(n)
        if int(crop_h[:, :2].min()) < 0 or int(crop_h[:, :2].max()) + self.crop_size > self.load_size:
            raise ValueError("crop window outside the load_size x load_size source")
        self.last_window = crop_h                                               # for a caller that cuts further maps at the same window (michigan_amd.evaluate)
        return crop_h

    def _resized(self, image: torch.Tensor) -> torch.Tensor:
        """Resize(osize, BICUBIC), base_dataset.py:421-424"""
        if image.shape[1] != self.load_size or image.shape[2] != self.load_size:
            key = (image.shape[1], image.shape[2])
            if key not in self._btabs:
                self._btabs[key] = (bicubic_table(key[1], self.load_size, self.device), bicubic_table(key[0], self.load_size, self.device))
            image = resize_bicubic_u8(image, self.load_size, self._btabs[key])
        return image

    def _image(self, image: torch.Tensor, crop: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """transform_image: an image stored at any size through the tables of that size"""
        return crop_u8(self._resized(image.to(self.device)), crop, self.crop_size, mode=0, out=out)

    def _map(self, src: torch.Tensor, crop: torch.Tensor, *, mode: int, unknown_label: int = -1, mul: Optional[torch.Tensor] = None,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """transform_label: a map (or an RGB picture) stored at any size through the tables of that size"""
        yt, xt = self._tabs_for(src.shape[1], src.shape[2])
        return crop_u8(src.to(self.device), crop, self.crop_size, mode=mode, unknown_label=unknown_label, ytab=yt, xtab=xt, mul=mul, out=out)

    def _each(self, fn, sources, crop: torch.Tensor, channels: int, **kw) -> torch.Tensor:
        """a batch whose samples are stored at different sizes: one launch per sample into its rows of the batch"""
        out = torch.empty((len(sources), channels, self.crop_size, self.crop_size), dtype=torch.float32, device=self.device)
        for i, s in enumerate(sources):
            fn(s, crop[i:i + 1], out=out[i:i + 1], **kw)
        return out

    def _check_options(self, what: str):
        if getattr(self.opt, "color_jitter", False):
            raise NotImplementedError(f"{what}: color_jitter (torchvision's ColorJitter on the reference image) is not implemented")
        mode = getattr(self.opt, "preprocess_mode", "resize_and_crop")
        if mode != "resize_and_crop":
            raise NotImplementedError(f"{what}: preprocess_mode {mode!r}; only 'resize_and_crop' is implemented")
        if self.crop_size > self.load_size:                                     # get_params would draw x = y = 0: no window fits
            raise ValueError(f"{what}: crop window outside the load size ({self.crop_size} > {self.load_size})")

    def __call__(self, image: torch.Tensor, label: torch.Tensor, orient: torch.Tensor, orient_mask: Optional[torch.Tensor] = None,
                 image_ref=None, label_ref=None) -> Dict[str, torch.Tensor]:
        """image_ref / label_ref (both or neither): the decoded files of the reference sample, [N,Hr,Wr,3] / [N,Hr,Wr], or a
        sequence of N per-sample tensors [Hr,Wr,3] / [Hr,Wr] where their sizes differ within the batch.  They take the target's
        window and flip (the reference reuses `params` and `transform_label`) through the tables of their own size."""
        opt, dev, cs = self.opt, self.device, self.crop_size
        self._check_options("DeviceInputPipeline")
        if (image_ref is None) != (label_ref is None):
            raise ValueError("image_ref and label_ref are given together (the reference sample's two files), or neither")
        n = image.shape[0]
        for name, t in (("label", label), ("orient", orient), ("orient_mask", orient_mask)):       # combined pixel by pixel at the stored size
            if t is not None and (t.shape[0] != n or tuple(t.shape[1:3]) != tuple(label.shape[1:3])):
                raise ValueError(f"{name} {tuple(t.shape)} does not match the batch: {n} samples, label {tuple(label.shape)}")
        if image_ref is not None:
            listed = isinstance(image_ref, (list, tuple))
            if listed != isinstance(label_ref, (list, tuple)):
                raise ValueError("image_ref and label_ref are both batches or both sequences of per-sample tensors")
            if listed:
                if len(image_ref) != n or len(label_ref) != n:
                    raise ValueError(f"image_ref / label_ref: {len(image_ref)} / {len(label_ref)} samples, the batch has {n}")
                image_ref = [_decoded(t, "image_ref[%d]" % i, 3, 1) for i, t in enumerate(image_ref)]
                label_ref = [_decoded(t, "label_ref[%d]" % i, 1, 1) for i, t in enumerate(label_ref)]
            else:
                image_ref, label_ref = _decoded(image_ref, "image_ref", 3, n), _decoded(label_ref, "label_ref", 1, n)
        image, label, orient = (t.to(dev) for t in (image, label, orient))
        image = self._resized(image)
        crop_h = self._window(n)
        crop = upload(crop_h, dev)
        yt, xt = self._tab(label.shape[1]), self._tab(label.shape[2])
        unknown = int(opt.label_nc)
        label_t = crop_u8(label, crop, cs, mode=1, unknown_label=unknown, ytab=yt, xtab=xt)
        image_t = crop_u8(image, crop, cs, mode=0)
        data = {"label_tag": label_t, "label_ref": label_t, "image_tag": image_t, "image_ref": image_t, "instance": 0,
                "orient": crop_u8(orient, crop, cs, mode=1, ytab=yt, xtab=xt)}
        if getattr(opt, "use_ig", False):
            om = label if orient_mask is None else orient_mask.to(dev)
            rgb = orient_to_rgb_u8(orient, label, self.table)
            data["orient_rgb"] = crop_u8(rgb, crop, cs, mode=2, ytab=yt, xtab=xt, mul=label_t)
            th = torch.tensor([self.rng.uniform(0.5, 1.2) for _ in range(n)], dtype=torch.float64)
            u = torch.tensor([self.rng.random() for _ in range(n)], dtype=torch.float64)
            hole = generate_hole_u8(label, om, upload(th, dev), upload(u, dev))
            data["hole"] = crop_u8(hole, crop, cs, mode=1, ytab=yt, xtab=xt)
        else:
            data["orient_rgb"], data["hole"] = torch.tensor(0), 0
        data["noise"] = generate_noise(n, cs, dev, self.generator)
        if image_ref is not None:                                               # pix2pix_dataset.py:80-83,96-100
            if isinstance(image_ref, list):
                data["label_ref"] = self._each(self._map, label_ref, crop, 1, mode=1, unknown_label=unknown)
                data["image_ref"] = self._each(self._image, image_ref, crop, 3)
            else:
                data["label_ref"] = self._map(label_ref, crop, mode=1, unknown_label=unknown)
                data["image_ref"] = self._image(image_ref, crop)
        return data

    def inference_batch(self, *, image_ref, image_tag, label_ref, label_tag, orient_tag, orient_ref, orient_mask,
                        same_orient: bool) -> Dict[str, torch.Tensor]:
        """single_inference_dataLoad (base_dataset.py:49-160) from its seven decoded files; the keys it returns, except `path`.
        same_orient: `opt.inference_orient_name == opt.inference_tag_name`, the hole rule's case (:116)."""
        opt, dev = self.opt, self.device
        self._check_options("inference_batch")
        if getattr(opt, "expand_tag_mask", False):
            raise NotImplementedError("inference_batch: expand_tag_mask (a 25 x 25 cv2.dilate of the target mask) is not implemented")
        label_tag = _decoded(label_tag, "label_tag", 1)
        n = label_tag.shape[0]
        label_ref, orient_tag, orient_ref, orient_mask = (_decoded(t, k, 1, n) for k, t in (
            ("label_ref", label_ref), ("orient_tag", orient_tag), ("orient_ref", orient_ref), ("orient_mask", orient_mask)))
        image_ref, image_tag = _decoded(image_ref, "image_ref", 3, n), _decoded(image_tag, "image_tag", 3, n)
        ig = bool(getattr(opt, "use_ig", False))
        if ig:          # trans_orient_to_rgb (:107) and generate_hole (:117-118) combine them at their stored size
            _same_size({"label_tag": label_tag, "orient_mask": orient_mask, "orient_ref": orient_ref})
        if getattr(opt, "add_zeros", False):                                    # :69-76, before anything else
            th = int(opt.add_th)
            label_ref, label_tag, orient_mask, orient_tag, orient_ref, image_ref, image_tag = (
                _pad_zeros(t, th) for t in (label_ref, label_tag, orient_mask, orient_tag, orient_ref, image_ref, image_tag))
        crop = self._window(n).to(dev)
        unknown = int(opt.label_nc)
        label_tag, orient_mask = label_tag.to(dev), orient_mask.to(dev)
        data = {"label_ref": self._map(label_ref, crop, mode=1, unknown_label=unknown),
                "label_tag": self._map(label_tag, crop, mode=1, unknown_label=unknown), "instance": torch.tensor(0)}
        label_t = data["label_tag"]
        if ig and not getattr(opt, "no_orientation", False):                    # :106-112: the picture of orient_ref under ITS mask
            rgb = orient_to_rgb_u8(orient_ref.to(dev), orient_mask, self.table)
            data["orient_rgb"] = self._map(rgb, crop, mode=2, mul=label_t)
        else:
            data["orient_rgb"] = torch.tensor(0)
        if not ig:
            data["hole"] = torch.tensor(0)
        elif same_orient:                                                       # :116-120
            t = torch.tensor([self.rng.uniform(0.5, 1.2) for _ in range(n)], dtype=torch.float64)
            u = torch.tensor([self.rng.random() for _ in range(n)], dtype=torch.float64)
            data["hole"] = self._map(generate_hole_u8(label_tag, orient_mask, t, u), crop, mode=1)
        else:                                                                   # :122: label_tag - orient_mask * label_tag
            data["hole"] = label_t - self._map(orient_mask, crop, mode=1, unknown_label=unknown, mul=label_t)
        data["noise"] = generate_noise(n, self.crop_size, dev, self.generator)
        data["image_ref"] = self._image(image_ref, crop)
        data["image_tag"] = self._image(image_tag, crop)
        data["orient"] = self._map(orient_tag, crop, mode=1)
        return data

    def demo_batch(self, *, label_ref, label_tag, mask_orient, orient_ref, image_ref, image_tag, mask_stroke=None,
                   mask_hole=None) -> Dict[str, torch.Tensor]:
        """demo_inference_dataLoad (base_dataset.py:162-276); the keys it returns, except `path`.  Its `orient_stroke` argument
        (demo.py:325-326) is derived here from mask_stroke; mask_hole, the dilated stroke (demo.py:323-324), is `stroke_hole(mask_stroke)`
        and stays an argument: the two are given together or not at all (michigan_amd.demo.EditSession passes both)."""
        opt, dev = self.opt, self.device
        self._check_options("demo_batch")
        if getattr(opt, "expand_tag_mask", False):
            raise NotImplementedError("demo_batch: expand_tag_mask (a 25 x 25 cv2.dilate of the target mask) is not implemented")
        if (mask_stroke is None) != (mask_hole is None):
            raise ValueError("mask_stroke and mask_hole are given together (the stroke and its dilation), or neither")
        label_tag = _decoded(label_tag, "label_tag", 1)
        n = label_tag.shape[0]
        label_ref, mask_orient, orient_ref = (_decoded(t, k, 1, n) for k, t in (
            ("label_ref", label_ref), ("mask_orient", mask_orient), ("orient_ref", orient_ref)))
        image_ref, image_tag = _decoded(image_ref, "image_ref", 3, n), _decoded(image_tag, "image_tag", 3, n)
        _same_size({"mask_orient": mask_orient, "orient_ref": orient_ref})       # trans_orient_to_rgb (:207)
        if mask_stroke is not None:
            mask_stroke, mask_hole = _decoded(mask_stroke, "mask_stroke", 1, n), _decoded(mask_hole, "mask_hole", 1, n)
            _same_size({"mask_stroke": mask_stroke, "mask_hole": mask_hole})
        crop_h = self._window(n)
        crop = crop_h.to(dev)
        unknown = int(opt.label_nc)
        mask_orient = mask_orient.to(dev)
        data = {"label_ref": self._map(label_ref, crop, mode=1, unknown_label=unknown),
                "label_tag": self._map(label_tag, crop, mode=1, unknown_label=unknown), "instance": torch.tensor(0)}
        label_t = data["label_tag"]
        rgb = orient_to_rgb_u8(orient_ref.to(dev), mask_orient, self.table)
        data["orient_rgb"] = self._map(rgb, crop, mode=2, mul=label_t)
        data["orient_rgb_mask"] = self._map(mask_orient, crop, mode=1, unknown_label=unknown, mul=label_t)           # :211
        if mask_stroke is None:
            data["hole"] = label_t - data["orient_rgb_mask"]                    # :216
            data["orient_stroke"], data["mask_stroke"] = torch.tensor(0), torch.tensor(0)
        else:
            yt, xt = self._tabs_for(mask_stroke.shape[1], mask_stroke.shape[2])
            data.update(stroke_inputs(mask_stroke.to(dev), label_t, mask_hole, crop=crop_h, ytab=yt, xtab=xt))
        data["noise"] = generate_noise(n, self.crop_size, dev, self.generator)
        data["image_ref"] = self._image(image_ref, crop)
        data["image_tag"] = self._image(image_tag, crop)
        data["orient"] = self._map(orient_ref, crop, mode=1)                    # :259: the demo's orientation is the reference's
        return data


def inference_batch(opt, *, image_ref, image_tag, label_ref, label_tag, orient_tag, orient_ref, orient_mask, same_orient,
                    rng: Optional[_random.Random] = None, generator: Optional[torch.Generator] = None) -> Dict[str, torch.Tensor]:
    """single_inference_dataLoad (base_dataset.py:49-160) for decoded uint8 maps on any device ([H,W] / [H,W,3], or with a leading
    batch dimension): DeviceInputPipeline.inference_batch on a pipeline of its own.  A caller that loads batch after batch keeps
    one pipeline and calls its method: the index tables are then built once."""
    dev = _loader_device((label_tag, image_tag, image_ref))
    return DeviceInputPipeline(opt, dev, rng=rng, generator=generator).inference_batch(
        image_ref=image_ref, image_tag=image_tag, label_ref=label_ref, label_tag=label_tag, orient_tag=orient_tag, orient_ref=orient_ref,
        orient_mask=orient_mask, same_orient=same_orient)


def demo_batch(opt, *, label_ref, label_tag, mask_orient, orient_ref, image_ref, image_tag, mask_stroke=None, mask_hole=None,
               rng: Optional[_random.Random] = None, generator: Optional[torch.Generator] = None) -> Dict[str, torch.Tensor]:
    """demo_inference_dataLoad (base_dataset.py:162-276) for decoded uint8 maps on any device: DeviceInputPipeline.demo_batch on a
    pipeline of its own (an interactive caller keeps one pipeline and calls its method)."""
    dev = _loader_device((label_tag, image_tag, image_ref))
    return DeviceInputPipeline(opt, dev, rng=rng, generator=generator).demo_batch(
        label_ref=label_ref, label_tag=label_tag, mask_orient=mask_orient, orient_ref=orient_ref, image_ref=image_ref, image_tag=image_tag,
        mask_stroke=mask_stroke, mask_hole=mask_hole)


