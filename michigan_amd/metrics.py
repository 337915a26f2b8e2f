"""Image-quality measurements on the device: PSNR, SSIM and orientation agreement of uint8 batches.

    q = metrics.image_quality(fake_u8, real_u8, mask=hair_u8)       # [N,H,W,C] (or [H,W,C]) uint8, mask [N,H,W] (or [H,W])
    q["psnr"], q["psnr_hair"], q["ssim"], q["ssim_hair"]            # float64 [N]
    o = metrics.orient_distance(orient_a, orient_b, mask)           # o["degrees"] float64 [N]
    metrics.pooled(rows)                                            # dataset values from pooled sums

The image pass is one fused HIP pass over the bytes (ops.image_quality_u8; include/michigan_hip/evaluation/quality.h defines every
term); what is left here is arithmetic on [N, C] tensors.  Conventions:
  * SSIM is Wang et al. 2004 as scikit-image computes it for uint8 data with gaussian_weights: the normalised Gaussian window of 11
    taps and sigma 1.5, population variances, C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2, the map taken only where the window lies
    inside the image and averaged there; several channels: the mean over channels of the per-channel means.
  * PSNR is 10 log10(255^2 P C / SSE) over the P pixels and C channels counted: inf at SSE == 0.
  * The hair variants count the pixels with mask != 0 (SSIM: the valid-region pixels whose own mask byte is non-zero); a count of 0
    gives nan.
Nothing is read back here: every value is a tensor on the inputs' device.
"""
from __future__ import annotations

import math
from typing import Dict, Iterable, Optional

import numpy as np
import torch

from . import ops

PEAK = 255.0


def gaussian_window(k: int = 11, sigma: float = 1.5) -> np.ndarray:
    """The normalised Gaussian of k taps in float64: exp(-(i - k // 2)^2 / (2 sigma^2)) / sum."""
    k = int(k)
    if k < 1 or k % 2 == 0:
        raise ValueError("gaussian_window: k must be odd and positive, got %d" % k)
    if not sigma > 0:
        raise ValueError("gaussian_window: sigma must be positive, got %r" % (sigma,))
    x = np.arange(k, dtype=np.float64) - (k // 2)
    g = np.exp(-(x * x) / (2.0 * float(sigma) * float(sigma)))
    return g / g.sum()


def _ratio(num: torch.Tensor, den: torch.Tensor) -> torch.Tensor:
    """num / den in float64; 0 / 0 = nan, x / 0 = inf"""
    return num.to(torch.float64) / den.to(torch.float64)


def _psnr(sse: torch.Tensor, terms: torch.Tensor) -> torch.Tensor:
    """10 log10(255^2 terms / sse): inf at sse == 0 < terms, nan at terms == 0"""
    return 10.0 * torch.log10(_ratio(PEAK * PEAK * terms.to(torch.float64), sse))


def image_quality(a: torch.Tensor, b: torch.Tensor, mask: Optional[torch.Tensor] = None, window=None) -> Dict[str, torch.Tensor]:
    """PSNR and SSIM of a against b, full image and under `mask`, per sample.  a, b uint8 [N,H,W,C] or [H,W,C], 1 <= C <= 4; mask uint8
    [N,H,W] or [H,W] (non-zero = hair) or None (the hair variants then equal the full ones); window: the taps (default
    gaussian_window()).  Returns float64 [N] psnr, psnr_hair, ssim, ssim_hair and the raw terms they come from: int64 [N,C] sse,
    sse_hair, float64 [N,C] ssim_sum, ssim_sum_hair, int64 [N] pixels, hair_pixels, ssim_count, ssim_hair_count, and `channels`."""
    if not (torch.is_tensor(a) and torch.is_tensor(b)) or a.dim() != b.dim() or a.dim() not in (3, 4):
        raise ValueError("image_quality: a and b must be uint8 [N,H,W,C] or [H,W,C] tensors of one shape")
    if a.dim() == 3:
        a, b = a.unsqueeze(0), b.unsqueeze(0)
        if mask is not None:
            if not torch.is_tensor(mask) or mask.dim() != 2:
                raise ValueError("image_quality: with [H,W,C] images the mask must be uint8 [H,W]")
            mask = mask.unsqueeze(0)
    win = gaussian_window() if window is None else window
    out_int, out_ssim = ops.image_quality_u8(a, b, mask, win)
    n, h, w, c = a.shape
    r = int(np.asarray(win).size) // 2
    dev = a.device
    sse, sse_hair = out_int[:, :, 0], out_int[:, :, 1]
    hair_pixels, ssim_hair_count = out_int[:, 0, 2], out_int[:, 0, 3]
    pixels = torch.full((n,), h * w, dtype=torch.int64, device=dev)
    ssim_count = torch.full((n,), (h - 2 * r) * (w - 2 * r), dtype=torch.int64, device=dev)
    ssim_sum, ssim_sum_hair = out_ssim[:, :, 0], out_ssim[:, :, 1]
    return {
        "psnr": _psnr(sse.sum(1), pixels * c), "psnr_hair": _psnr(sse_hair.sum(1), hair_pixels * c),
        "ssim": _ratio(ssim_sum, ssim_count.unsqueeze(1)).mean(1), "ssim_hair": _ratio(ssim_sum_hair, ssim_hair_count.unsqueeze(1)).mean(1),
        "sse": sse, "sse_hair": sse_hair, "ssim_sum": ssim_sum, "ssim_sum_hair": ssim_sum_hair,
        "pixels": pixels, "hair_pixels": hair_pixels, "ssim_count": ssim_count, "ssim_hair_count": ssim_hair_count, "channels": c,
    }


def orient_distance(a: torch.Tensor, b: torch.Tensor, mask: torch.Tensor) -> Dict[str, torch.Tensor]:
    """Mean angular disagreement of two orientation maps under `mask`, per sample.  a, b, mask uint8 [N,H,W] or [H,W]; a map codes
    the angle as v / 255 * pi, so the distance of two codes is min(d, 255 - d), d = |a - b|.  Returns float64 [N] `degrees`
    (sum / count * 180 / 255; nan at count 0) and int64 [N] `sum`, `count`."""
    if not (torch.is_tensor(a) and torch.is_tensor(b) and torch.is_tensor(mask)) or a.dim() not in (2, 3):
        raise ValueError("orient_distance: a, b and mask must be uint8 [N,H,W] or [H,W] tensors of one shape")
    if a.dim() == 2:
        if b.dim() != 2 or mask.dim() != 2:
            raise ValueError("orient_distance: a, b and mask must be uint8 [N,H,W] or [H,W] tensors of one shape")
        a, b, mask = a.unsqueeze(0), b.unsqueeze(0), mask.unsqueeze(0)
    out = ops.orient_distance_u8(a, b, mask)
    total, count = out[:, 0], out[:, 1]
    return {"degrees": _ratio(total, count) * (180.0 / ops.ORIENT_PERIOD), "sum": total, "count": count}


# what a row (one sample, host numbers) may carry, and what pooled() makes of the rows that carry it
ROW_KEYS = ("sse", "pixels", "sse_hair", "hair_pixels", "ssim_sum", "ssim_count", "ssim_sum_hair", "ssim_hair_count", "channels",
            "orient_sum", "orient_count", "hair_lab")


def _log_psnr(sse: float, terms: float) -> float:
    if terms <= 0:
        return float("nan")
    return float("inf") if sse <= 0 else 10.0 * math.log10(PEAK * PEAK * terms / sse)


def pooled(rows: Iterable[dict]) -> dict:
    """Dataset values from pooled sums over per-sample rows (host numbers; `sse`, `ssim_sum` and their hair forms are per-channel
    lists or their totals):
      psnr / psnr_hair            10 log10(255^2 sum(P C) / sum(SSE)): one perfect sample cannot make it infinite
      ssim / ssim_hair            sum(ssim_sum) / sum(count C): weighted by the pixels each sample counts
      orient_error_deg            sum(orient_sum) / sum(orient_count) * 180 / 255
      hair_lab                    the plain mean over the rows that carry one
    A value whose rows are absent, or whose pooled count is 0, is nan.  `samples` is the number of rows."""
    tot = lambda v: float(np.sum(v))
    acc = dict.fromkeys(("sse", "terms", "sse_hair", "terms_hair", "ssim_sum", "ssim_terms", "ssim_sum_hair", "ssim_hair_terms", "orient_sum", "orient_count",
                         "hair_lab", "hair_lab_rows"), 0.0)
    samples = 0
    for row in rows:
        samples += 1
        if "sse" in row:
            c = int(row["channels"])
            acc["sse"] += tot(row["sse"]); acc["terms"] += float(row["pixels"]) * c
            acc["sse_hair"] += tot(row["sse_hair"]); acc["terms_hair"] += float(row["hair_pixels"]) * c
            acc["ssim_sum"] += tot(row["ssim_sum"]); acc["ssim_terms"] += float(row["ssim_count"]) * c
            acc["ssim_sum_hair"] += tot(row["ssim_sum_hair"]); acc["ssim_hair_terms"] += float(row["ssim_hair_count"]) * c
        if "orient_sum" in row:
            acc["orient_sum"] += float(row["orient_sum"]); acc["orient_count"] += float(row["orient_count"])
        if row.get("hair_lab") is not None:
            acc["hair_lab"] += float(row["hair_lab"]); acc["hair_lab_rows"] += 1
    div = lambda num, den: num / den if den > 0 else float("nan")
    return {
        "samples": samples,
        "psnr": _log_psnr(acc["sse"], acc["terms"]), "psnr_hair": _log_psnr(acc["sse_hair"], acc["terms_hair"]),
        "ssim": div(acc["ssim_sum"], acc["ssim_terms"]), "ssim_hair": div(acc["ssim_sum_hair"], acc["ssim_hair_terms"]),
        "orient_error_deg": div(acc["orient_sum"], acc["orient_count"]) * (180.0 / ops.ORIENT_PERIOD),
        "hair_lab": div(acc["hair_lab"], acc["hair_lab_rows"]),
    }
