"""Helpers of tests/test_quality.py (CPU) and tests/test_gpu_quality.py (-m gpu): the float64 numpy contracts of the two entry points of
the quality extension group (include/michigan_hip/evaluation/quality.h), their one-line mutants, the case tables both files run, the
derivation of the SSIM bound, and `QualityEmulator`: oracle/cabi_emulator.py's EmulatorBackend (with the editing group of
tests/mask_edit_fixtures.py) plus mgq_* from those contracts -- the group is outside the versioned table, so the emulator under oracle/
does not carry it.

The integer terms (squared errors, counts, orientation sums) are int64 arithmetic: every comparison against them is torch.equal.

THE SSIM BOUND, per map value, for the order of operations the kernel uses (u = 2^-53; k taps; the window's taps are non-negative and sum to
S = 1 up to rounding; M is the largest magnitude of what a moment averages: 255 for mu, 65025 for E[aa], E[bb], E[ab], all exact integers):
  1. A moment is two chained passes of k fused multiply-adds from +0.  Every partial sum is at most S M, each fma rounds once, so a pass
     adds at most k u M, and the y pass carries the x pass' error through weights that sum to 1:  |moment - exact| <= 2 k u M.
  2. The contract below multiplies and adds separately (numpy has no fma): 2 roundings a tap, 4 k u M per moment.  Kernel against contract:
     dM <= 6 k u M, which is 6.5e-10 for the second moments and 2.6e-12 for the means at k = 15 -- below the 2e-9 the issue allows for
     any order.
  3. var = E - mu mu (two roundings of magnitude <= 65025 u each):  dvar <= dE + 2 * 255 * dmu + 2 * 65025 u = 6.5e-10 + 1.3e-9 + 1.5e-11.
     The covariance likewise.  "A few times" the moment's error: about 2e-9.
  4. The four factors.  n1 = (2 mu_a) mu_b + C1 and d1 = mu_a mu_a + mu_b mu_b + C1 are at least C1 = 6.5025 and move by at most
     4 * 255 * dmu + 3 * 130050 u = 2.7e-9: relative error <= 4.2e-10 each.  d2 = var_a + var_b + C2 is at least C2 = 58.5225 (minus the
     rounding of a variance that is exactly 0) and moves by at most 2 dvar + 2 u * 130050 = 4e-9: relative error 6.8e-11.  n2 = 2 cov + C2
     may be small or negative, so its error counts absolutely: |n1 dn2 / (d1 d2)| <= dn2 / C2 = 6.8e-11, because n1 <= d1.
  5. |ssim| <= 1, so |dssim| <= 4.2e-10 + 4.2e-10 + 6.8e-11 + 6.8e-11 + the three roundings of the quotient (3 u) = 9.8e-10 <= 1e-9
     at k = 15; every term is proportional to k, so k = 11 gives 7.2e-10.
  6. The sums add `count` such values, |partial| <= count, each addition rounds once in either order: count^2 u more, which stays under
     the remaining 2e-11 * count for every count below 1.8e5 (the largest here is 54 * 54).
Hence |ssim_sum_hip - ssim_sum_contract| <= 1e-9 * count, the bound the issue sets; `ssim_bound(k)` evaluates steps 1 to 5 and the CPU
test holds it to 1e-9.  No pivot is subtracted anywhere, so the issue's pivot mutant has nothing to mutate."""
import ctypes

import numpy as np
import torch

from mask_edit_fixtures import EditEmulator
from oracle.cabi_emulator import _addr, _view

TILE, MIN_K, MAX_K, MAX_C, WS_SLOTS, INT_TERMS, SSIM_TERMS, PERIOD = 16, 3, 15, 4, 6, 4, 2, 255
C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
SSIM_TOL = 1e-9                                                        # per counted map value: the issue's bound, derived above


def ssim_bound(k):
    """steps 1-5 of the module docstring as arithmetic -> the bound on one map value, kernel against contract"""
    u = 2.0 ** -53
    d_mu, d_e = 6 * k * u * 255.0, 6 * k * u * 65025.0
    d_var = d_e + 2 * 255.0 * d_mu + 2 * 65025.0 * u
    rel_1 = (4 * 255.0 * d_mu + 3 * 130050.0 * u) / C1
    rel_d2 = (2 * d_var + 2 * 130050.0 * u) / C2
    abs_n2 = (2 * d_var + 2 * 130050.0 * u) / C2
    return 2 * rel_1 + rel_d2 + abs_n2 + 3 * u


def gaussian(k=11, sigma=1.5):
    x = np.arange(k, dtype=np.float64) - k // 2
    g = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return g / g.sum()


# ---- image quality ---------------------------------------------------------------------------------------------------------------------
def _blur(z, win):
    """the separable window over the valid region: along x, then along y; taps in ascending order from 0"""
    k = len(win)
    h, w = z.shape[-2:]
    t = np.zeros(z.shape[:-1] + (w - k + 1,))
    for j in range(k):
        t = t + win[j] * z[..., j:j + w - k + 1]
    o = np.zeros(z.shape[:-2] + (h - k + 1, w - k + 1))
    for i in range(k):
        o = o + win[i] * t[..., i:i + h - k + 1, :]
    return o


def blur_four_loops(z, win):
    """the same moment as the plain double sum over the k x k window (a second opinion; 2-D input)"""
    k = len(win)
    h, w = z.shape
    o = np.zeros((h - k + 1, w - k + 1))
    for y in range(h - k + 1):
        for x in range(w - k + 1):
            for i in range(k):
                for j in range(k):
                    o[y, x] += win[i] * win[j] * z[y + i, x + j]
    return o


def ssim_map(a, b, win, mutant=None):
    """a, b float64 [..., H, W] -> the map over the valid region [..., H - k + 1, W - k + 1]"""
    win = np.asarray(win, np.float64)
    k = len(win)
    if mutant == "window_shift":
        win = np.roll(win, 1)
    mu_a, mu_b = _blur(a, win), _blur(b, win)
    e_aa, e_bb, e_ab = _blur(a * a, win), _blur(b * b, win), _blur(a * b, win)
    var_a, var_b, cov = e_aa - mu_a * mu_a, e_bb - mu_b * mu_b, e_ab - mu_a * mu_b
    if mutant == "sample_variance":
        norm = (k * k) / (k * k - 1.0)
        var_a, var_b, cov = var_a * norm, var_b * norm, cov * norm
    c1, c2 = (C2, C1) if mutant == "c1_c2_swapped" else (C1, C2)
    return (((2.0 * mu_a) * mu_b + c1) * (2.0 * cov + c2)) / (((mu_a * mu_a + mu_b * mu_b) + c1) * ((var_a + var_b) + c2))


def quality_contract(a, b, mask, win, mutant=None):
    """a, b u8 [N,H,W,C], mask u8 [N,H,W] or None, win k taps -> (int64 [N,C,4] = sse, sse_mask, mask_count, valid_mask_count;
    float64 [N,C,2] = ssim_sum, ssim_sum_mask)"""
    a, b = np.asarray(a, np.uint8), np.asarray(b, np.uint8)
    n, h, w, c = a.shape
    k = len(win)
    r = k // 2
    m = np.ones((n, h, w), bool) if mask is None else np.asarray(mask) != 0
    d = a.astype(np.int64) - b.astype(np.int64)
    sq = np.transpose(d * d, (0, 3, 1, 2))                             # [N,C,H,W]
    valid = np.zeros((h, w), bool)
    valid[r:h - r, r:w - r] = True
    out_int = np.zeros((n, c, 4), np.int64)
    out_int[:, :, 0] = sq.sum((2, 3))
    region = m & valid if mutant == "sse_mask_valid_only" else m
    out_int[:, :, 1] = (sq * region[:, None]).sum((2, 3))
    out_int[:, :, 2] = m.sum((1, 2))[:, None]
    out_int[:, :, 3] = (m & valid).sum((1, 2))[:, None]
    fa, fb = (np.transpose(t, (0, 3, 1, 2)).astype(np.float64) for t in (a, b))
    smap = ssim_map(fa, fb, win, mutant)                               # [N,C,H-2r,W-2r]
    centre = m[:, 0:h - 2 * r, 0:w - 2 * r] if mutant == "mask_at_corner" else m[:, r:h - r, r:w - r]
    if mutant == "valid_y":                                            # the region begins one row late
        smap, centre = smap[:, :, 1:], centre[:, 1:]
    if mutant == "valid_x":
        smap, centre = smap[:, :, :, 1:], centre[:, :, 1:]
    out_ssim = np.zeros((n, c, 2))
    out_ssim[:, :, 0] = smap.sum((2, 3))
    out_ssim[:, :, 1] = (smap * centre[:, None]).sum((2, 3))
    return out_int, out_ssim


QUALITY_MUTANTS = ("window_shift", "valid_y", "valid_x", "c1_c2_swapped", "sample_variance", "mask_at_corner", "sse_mask_valid_only")
SHAPES = ((11, 11), (11, 43), (12, 27), (26, 26), (27, 37), (43, 11), (64, 64))        # valid regions of 1, 2, 16, 17, 27 and 33 (and 54) at k = 11
KINDS = ("random", "bright", "smooth", "constant")
# (H, W, N, C): every shape at N, C in {1, 3}, both together and crossed
GEOMETRIES = tuple((h, w, n, c) for i, (h, w) in enumerate(SHAPES) for n, c in (((1, 1), (3, 3)) if i % 2 == 0 else ((1, 3), (3, 1)))) + \
    ((27, 37, 1, 3), (27, 37, 3, 1), (12, 27, 1, 3), (12, 27, 3, 1))


def image_pair(kind, n, h, w, c, seed):
    r = np.random.default_rng(seed)
    shape = (n, h, w, c)
    if kind == "random":
        return r.integers(0, 256, shape).astype(np.uint8), r.integers(0, 256, shape).astype(np.uint8)
    if kind == "bright":                                               # bright and flat: where E[x^2] - mu^2 cancels
        return r.integers(250, 256, shape).astype(np.uint8), r.integers(250, 256, shape).astype(np.uint8)
    if kind == "smooth":
        yy, xx = np.mgrid[0:h, 0:w]
        base = 128 + 100 * np.sin(xx / 5.0 + np.arange(c)[:, None, None]) * np.cos(yy / 7.0 + np.arange(n)[:, None, None, None])     # [N,C,H,W]
        sm = np.transpose(base, (0, 2, 3, 1)).astype(np.uint8)
        return sm, np.clip(sm.astype(np.int64) + r.integers(-8, 9, shape), 0, 255).astype(np.uint8)
    if kind == "constant":
        return np.full(shape, 255, np.uint8), np.full(shape, 254, np.uint8)
    raise KeyError(kind)


def hair_mask(n, h, w, seed, k=11):
    """u8 [N,H,W], about 40 % in, values 1 and 255 both; the image centre, which is inside the valid region for every H, W >= k, is in"""
    r = np.random.default_rng(seed)
    m = (r.random((n, h, w)) < 0.4).astype(np.uint8) * r.choice(np.array([1, 255], np.uint8), size=(n, h, w))
    m[:, h // 2, w // 2] = 1
    return m


def quality_cases():
    """{id: (a, b, mask or None, window)}: the four kinds with a mask at every geometry, without one at two, k = 3 and k = 15 once each,
    and the empty mask"""
    out = {}
    g11 = gaussian()
    for gi, (h, w, n, c) in enumerate(GEOMETRIES):
        for ki, kind in enumerate(KINDS):
            a, b = image_pair(kind, n, h, w, c, 100 * gi + ki)
            out["%s-%dx%dx%dx%d" % (kind, n, h, w, c)] = (a, b, hair_mask(n, h, w, 7 * gi + ki), g11)
    for h, w, n, c in ((27, 37, 3, 3), (11, 11, 1, 1)):
        a, b = image_pair("random", n, h, w, c, 900 + h)
        out["nomask-%dx%dx%dx%d" % (n, h, w, c)] = (a, b, None, g11)
    a, b = image_pair("smooth", 3, 27, 37, 3, 901)
    out["k3-3x27x37x3"] = (a, b, hair_mask(3, 27, 37, 31, k=3), gaussian(3, 1.5))
    a, b = image_pair("random", 1, 27, 37, 3, 902)
    out["k15-1x27x37x3"] = (a, b, hair_mask(1, 27, 37, 32, k=15), gaussian(15, 1.5))
    a, b = image_pair("random", 3, 27, 37, 3, 903)
    out["emptymask-3x27x37x3"] = (a, b, np.zeros((3, 27, 37), np.uint8), g11)
    return out


# ---- orientation agreement ---------------------------------------------------------------------------------------------------------------
def orient_contract(a, b, mask, mutant=None):
    """a, b, mask u8 [N,H,W] -> int64 [N,2] = (sum of min(d, 255 - d) under the mask, count)"""
    d = np.abs(np.asarray(a, np.uint8).astype(np.int64) - np.asarray(b, np.uint8).astype(np.int64))
    if mutant != "no_wrap":
        d = np.minimum(d, (256 if mutant == "period_256" else PERIOD) - d)
    m = np.asarray(mask) != 0
    return np.stack([(d * m).sum((1, 2)), m.sum((1, 2))], axis=1).astype(np.int64)


ORIENT_MUTANTS = ("period_256", "no_wrap")


def orient_cases():
    """{id: (a, b, mask)}: random maps at a ragged size (bytes), at sizes whose planes take 16 bytes a lane, more than one chunk of 16384
    pixels, a == b, the pair (0, 255), and the empty mask"""
    r = np.random.default_rng(17)
    rand = lambda n, h, w: r.integers(0, 256, (n, h, w)).astype(np.uint8)
    out = {}
    for n, h, w in ((1, 11, 11), (3, 27, 37), (3, 64, 64), (2, 16, 16), (2, 144, 160), (1, 129, 131)):
        out["random-%dx%dx%d" % (n, h, w)] = (rand(n, h, w), rand(n, h, w), hair_mask(n, h, w, n + h))
    a = rand(3, 27, 37)
    out["same-3x27x37"] = (a, a.copy(), hair_mask(3, 27, 37, 5))
    out["0-255-2x16x16"] = (np.zeros((2, 16, 16), np.uint8), np.full((2, 16, 16), 255, np.uint8), np.ones((2, 16, 16), np.uint8))
    out["emptymask-3x27x37"] = (rand(3, 27, 37), rand(3, 27, 37), np.zeros((3, 27, 37), np.uint8))
    return out


# ---- the emulator ----------------------------------------------------------------------------------------------------------------------
def workspace_bytes(n, h, w, c):
    if n < 1 or h < 1 or w < 1 or not 1 <= c <= MAX_C or n * h * w * c >= 1 << 31:
        return 0
    return n * (-(-h // TILE)) * (-(-w // TILE)) * c * WS_SLOTS * 8


class QualityEmulator(EditEmulator):
    """EmulatorBackend + the editing group + the quality group, from the contracts above.  Argument checks as the header states them; a
    refused call is in the log too, as the base class keeps it."""

    def mgq_quality_workspace(self, n, h, w, c):
        return workspace_bytes(n, h, w, c)

    def mgq_image_quality_u8(self, a, b, mask, window, k, ws, out_int, out_ssim, n, h, w, c, stream=None):
        fn = "mgq_image_quality_u8"
        self._note(fn)
        if not (_addr(a) and _addr(b) and _addr(window) and _addr(ws) and _addr(out_int) and _addr(out_ssim)):
            self._fail(fn, "null pointer")
        if not (MIN_K <= k <= MAX_K and k % 2 == 1):
            self._fail(fn, "bad window length")
        if not 1 <= c <= MAX_C:
            self._fail(fn, "bad channel count")
        if n < 1 or h < 1 or w < 1 or n * h * w * c >= 1 << 31:
            self._fail(fn, "bad geometry")
        if h < k or w < k:
            self._fail(fn, "the image is smaller than the window")
        win = _view(window, (k,), torch.float64).numpy().copy()
        m = _view(mask, (n, h, w), torch.uint8)
        oi, os_ = quality_contract(_view(a, (n, h, w, c), torch.uint8).numpy(), _view(b, (n, h, w, c), torch.uint8).numpy(),
                                   None if m is None else m.numpy(), win)
        _view(out_int, (n, c, INT_TERMS), torch.int64)[:] = torch.from_numpy(oi)
        _view(out_ssim, (n, c, SSIM_TERMS), torch.float64)[:] = torch.from_numpy(os_)
        return 0

    def mgq_orient_distance_u8(self, a, b, mask, out, n, h, w, stream=None):
        fn = "mgq_orient_distance_u8"
        self._note(fn)
        if not (_addr(a) and _addr(b) and _addr(mask) and _addr(out)):
            self._fail(fn, "null pointer")
        if n < 1 or h < 1 or w < 1 or n * h * w >= 1 << 31:
            self._fail(fn, "bad geometry")
        res = orient_contract(*[_view(p, (n, h, w), torch.uint8).numpy() for p in (a, b, mask)])
        _view(out, (n, 2), torch.int64)[:] = torch.from_numpy(res)
        return 0


def header_defines():
    """{name: int} of the integer MGQ_ #defines of include/michigan_hip/evaluation/quality.h"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "michigan_hip", "evaluation", "quality.h")) as fh:
        return {k: int(v) for k, v in re.findall(r"#define\s+(MGQ_[A-Z0-9_]+)\s+(\d+)\b", fh.read())}


def pointer(t):
    return ctypes.c_void_p(t.data_ptr())
