"""Helpers of tests/test_mask_edit.py (CPU) and tests/test_gpu_mask_edit.py (-m gpu): the numpy contracts of the two entry points of
the editing extension group (include/michigan_hip/editing/mask_edit.h), their one-line mutants, the case tables both files run, and
`EditEmulator`: oracle/cabi_emulator.py's EmulatorBackend with mge_brush_u8 and mge_morph_u8 added from those contracts (the group is
outside the versioned table, so the emulator under oracle/ does not carry it).

brush_contract is int64 arithmetic only and morph_contract uint8 maxima / minima only: there is nothing to round, so every comparison
against them is array_equal / torch.equal."""
import ctypes

import numpy as np
import torch

from oracle.cabi_emulator import EmulatorBackend, _addr, _view

MAX_COORD, MAX_THICKNESS, MAX_K = 8191, 255, 64


# ---- the brush -------------------------------------------------------------------------------------------------------------------------
def covered(xx, yy, x0, y0, x1, y1, t, mutant=None):
    """the capsule test of the header at the int64 pixel grids xx, yy -> bool"""
    xx, yy = xx.astype(np.int64), yy.astype(np.int64)
    dx, dy = np.int64(x1 - x0), np.int64(y1 - y0)
    qx, qy = xx - x0, yy - y0
    L2, dot = dx * dx + dy * dy, qx * dx + qy * dy
    t2 = np.int64(t) * np.int64(t)
    four = np.int64(1 if mutant == "radius" else 4)                   # mutant: the thickness taken as a radius
    le = (lambda a, b: a < b) if mutant == "lt" else (lambda a, b: a <= b)
    near = le(four * (qx * qx + qy * qy), t2)
    ex, ey = qx - dx, qy - dy
    far = le(four * (ex * ex + ey * ey), t2)
    cross = qx * dy - qy * dx
    side = le(four * cross * cross, t2 * L2)
    if L2 == 0:
        return near
    if mutant == "no_caps":                                            # an infinite line
        return side
    if mutant == "no_far_cap":                                         # the dot >= L2 branch dropped
        return np.where(dot <= 0, near, side)
    return np.where(dot <= 0, near, np.where(dot >= L2, far, side))


def brush_contract(canvas, segs, mutant=None):
    """canvas u8 [N,H,W], segs integer [S,8] = (sample, x0, y0, x1, y1, thickness, value, 0) -> the painted copy"""
    out = np.array(canvas, dtype=np.uint8, copy=True)
    n, h, w = out.shape
    yy, xx = np.mgrid[0:h, 0:w]
    rows = np.asarray(segs, dtype=np.int64).reshape(-1, 8)
    for s in (rows[::-1] if mutant == "reversed" else rows):
        k, x0, y0, x1, y1, t, val = (int(v) for v in s[:7])
        assert 0 <= k < n and 1 <= t <= MAX_THICKNESS and max(abs(x0), abs(y0), abs(x1), abs(y1)) <= MAX_COORD and 0 <= val <= 255
        c = covered(xx, yy, x0, y0, x1, y1, t, mutant)
        if mutant == "ignore_sample":
            out[:, c] = val
        else:
            out[k][c] = val
    return out


BRUSH_MUTANTS = ("lt", "no_caps", "no_far_cap", "reversed", "radius", "ignore_sample")
BRUSH_N, BRUSH_H, BRUSH_W = 2, 40, 56


def brush_cases():
    """{id: (canvas u8 [N,H,W], segs int64 [S,8])} at 2 x 40 x 56, and 700 random segments on 2 x 64 x 64 (three LDS chunks)"""
    n, h, w = BRUSH_N, BRUSH_H, BRUSH_W
    r = np.random.default_rng(41)
    blank = lambda: r.integers(0, 2, size=(n, h, w)).astype(np.uint8)             # a label map underneath: untouched pixels must survive
    seg = lambda k, x0, y0, x1, y1, t, v: [k, x0, y0, x1, y1, t, v, 0]
    cases = {
        "dots": [seg(0, 5, 5, 5, 5, 1, 2), seg(0, 20, 9, 20, 9, 2, 2), seg(1, 30, 20, 30, 20, 15, 2), seg(0, 16, 16, 16, 16, 3, 7)],
        "axis": [seg(0, 3, 10, 40, 10, 1, 2), seg(0, 3, 20, 40, 20, 4, 2), seg(1, 12, 2, 12, 37, 5, 2), seg(1, 30, 35, 30, 3, 2, 2)],
        "diagonal": [seg(0, 4, 4, 30, 30, 3, 2), seg(1, 50, 4, 20, 34, 6, 2), seg(0, 40, 2, 44, 38, 7, 1), seg(1, 2, 30, 50, 33, 8, 2)],
        "thickness": [seg(0, 6, 6 + 3 * t, 48, 8 + 3 * t, t, 2) for t in range(1, 11)] + [seg(1, 10, 20, 45, 22, 15, 2), seg(1, 10, 5, 45, 6, 14, 1)],
        "outside": [seg(0, -20, 10, 12, 14, 5, 2), seg(0, 45, 20, 90, 25, 6, 2), seg(1, 20, -30, 24, 8, 7, 2), seg(1, 30, 30, 33, 70, 4, 2),
                    seg(0, -50, -50, -10, -10, 9, 2), seg(1, -8000, 20, 8000, 21, 3, 2), seg(0, 70, 60, 90, 90, 15, 2)],
        "order": [seg(0, 5, 20, 50, 20, 9, 2), seg(0, 27, 3, 27, 37, 9, 1), seg(0, 20, 20, 35, 20, 3, 0), seg(1, 5, 5, 50, 35, 11, 1),
                  seg(1, 5, 35, 50, 5, 11, 2)],
        "sample1": [seg(1, 8, 8, 48, 30, 6, 2)],
        "empty": [],
    }
    out = {k: (blank(), np.asarray(v, np.int64).reshape(-1, 8)) for k, v in cases.items()}
    rows = np.stack([r.integers(0, 2, 700), r.integers(-10, 74, 700), r.integers(-10, 74, 700), r.integers(-10, 74, 700),
                     r.integers(-10, 74, 700), r.integers(1, 16, 700), r.integers(0, 3, 700), np.zeros(700, np.int64)], axis=1)
    out["random700"] = (r.integers(0, 2, size=(2, 64, 64)).astype(np.uint8), rows.astype(np.int64))
    return out


# ---- morphology ------------------------------------------------------------------------------------------------------------------------
DILATE, ERODE = 0, 1


def morph_contract(src, elem, anchor, op, mutant=None):
    """src u8 [N,H,W], elem u8 [kh,kw], anchor (ay, ax): dst[y,x] = max / min over taps (i, j) of src[y + i - ay, x + j - ax] inside
    the image; 0 / 255 when none is"""
    src, elem = np.asarray(src, np.uint8), np.asarray(elem, np.uint8)
    ay, ax = anchor
    if mutant == "flipped":                                            # a convolution: the impulse response is the element itself
        elem, ay, ax = elem[::-1, ::-1], elem.shape[0] - 1 - ay, elem.shape[1] - 1 - ax
    if mutant == "transposed":
        elem, ay, ax = elem.T, ax, ay
    kh, kw = elem.shape
    if mutant == "anchor_x":
        ax = ax + 1 if ax + 1 < kw else max(ax - 1, 0)
    if mutant == "anchor_y":
        ay = ay + 1 if ay + 1 < kh else max(ay - 1, 0)
    if mutant == "binary":
        src = np.where(src != 0, 255, 0).astype(np.uint8)
    n, h, w = src.shape
    ident = 0 if op == DILATE else 255
    border = 0 if mutant == "zero_border" else ident                   # mutant: taps outside the image read as 0 under erosion too
    pad = np.full((n, h + kh - 1, w + kw - 1), border, np.uint8)
    pad[:, ay:ay + h, ax:ax + w] = src
    out = np.full((n, h, w), ident, np.uint8)
    pick = np.maximum if op == DILATE else np.minimum
    for i in range(kh):
        on = np.flatnonzero(elem[i])
        if mutant == "first_run" and len(on):                          # only the first run of a row
            stop = np.flatnonzero(np.diff(on) > 1)
            on = on[:stop[0] + 1] if len(stop) else on
        for j in on:
            out = pick(out, pad[:, i:i + h, j:j + w])
    return out


MORPH_MUTANTS = ("flipped", "transposed", "anchor_x", "anchor_y", "zero_border", "first_run", "binary")
MORPH_N, MORPH_H, MORPH_W = 2, 37, 53


def elements():
    """{id: (elem u8 [kh,kw], anchor (ay, ax))}: the elements of the issue"""
    from michigan_amd import inputs
    centre = lambda e: (e.shape[0] // 2, e.shape[1] // 2)
    ell = {k: inputs.ellipse_element(k) for k in (3, 5, 20, 50)}
    L = np.zeros((7, 4), np.uint8)
    L[:, 0] = 1
    L[6, :] = 1
    ring = np.ones((9, 9), np.uint8)
    ring[2:7, 2:7] = 0
    ring[0, 0] = ring[8, 8] = 0                                        # not symmetric under a transpose of a flip either
    out = {"1x1": (np.ones((1, 1), np.uint8), (0, 0)), "cross3": (ell[3], centre(ell[3])), "ellipse5": (ell[5], centre(ell[5])),
           "ellipse20": (ell[20], centre(ell[20])), "ellipse50": (ell[50], centre(ell[50])),
           "rect25": (inputs.rect_element(25), (12, 12)), "L7x4-first": (L, (0, 0)), "L7x4-last": (L, (6, 3)), "ring9": (ring, (4, 4)),
           "full64": (np.ones((64, 64), np.uint8), (32, 32))}
    return out


def impulse_planes(h, w, low=False):
    """u8 [6,h,w]: one impulse (255 on 0; with `low`, 0 on 255) in each corner and at the centre, and one plane without any"""
    m = np.zeros((6, h, w), np.uint8)
    for k, (y, x) in enumerate(((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w // 2))):
        m[k, y, x] = 255
    return (255 - m) if low else m


def grey_planes(n, h, w, seed):
    """random grey levels with flat patches of 0 and of 255 (so that both identities occur in the input itself)"""
    r = np.random.default_rng(seed)
    m = r.integers(0, 256, size=(n, h, w)).astype(np.uint8)
    m[:, : h // 3, : w // 4] = 0
    m[:, -h // 4:, -w // 3:] = 255
    m[0, h // 2, w // 2] = 0
    return m


def morph_inputs(op):
    """{kind: u8 [*,37,53]}: the random grey pair and the six impulse planes (run two at a time on the device)"""
    return {"grey": grey_planes(MORPH_N, MORPH_H, MORPH_W, 7), "impulses": impulse_planes(MORPH_H, MORPH_W, low=op == ERODE)}


# ---- the emulator ----------------------------------------------------------------------------------------------------------------------
class EditEmulator(EmulatorBackend):
    """EmulatorBackend + the editing extension group, from the contracts above.  Argument checks as the header states them (a refused
    call is in the log too, as the base class keeps it); the per-segment ranges, which the library leaves to the uploader, are
    asserted here, where the list is host memory."""

    def mge_brush_u8(self, canvas, segs, s, n, h, w, stream=None):
        self._note("mge_brush_u8")
        if not _addr(canvas):
            self._fail("mge_brush_u8", "null canvas")
        if s < 0 or n < 1 or not (1 <= h <= MAX_COORD + 1 and 1 <= w <= MAX_COORD + 1) or n * h * w >= 1 << 31:
            self._fail("mge_brush_u8", "bad geometry")
        if s == 0:
            return 0
        if not _addr(segs):
            self._fail("mge_brush_u8", "null segment list")
        c = _view(canvas, (n, h, w), torch.uint8)
        c[:] = torch.from_numpy(brush_contract(c.numpy(), _view(segs, (s, 8), torch.int32).numpy()))
        return 0

    def mge_morph_u8(self, src, elem, kh, kw, ay, ax, op, dst, n, h, w, stream=None):
        self._note("mge_morph_u8", op)
        if not (_addr(src) and _addr(elem) and _addr(dst)):
            self._fail("mge_morph_u8", "null pointer")
        if op not in (DILATE, ERODE):
            self._fail("mge_morph_u8", "bad op")
        if not (1 <= kh <= MAX_K and 1 <= kw <= MAX_K):
            self._fail("mge_morph_u8", "bad element")
        if not (0 <= ay < kh and 0 <= ax < kw):
            self._fail("mge_morph_u8", "anchor outside the element")
        if n < 1 or h < 1 or w < 1 or n * h * w >= 1 << 31:
            self._fail("mge_morph_u8", "bad geometry")
        if abs(_addr(src) - _addr(dst)) < n * h * w:
            self._fail("mge_morph_u8", "src and dst overlap")
        res = morph_contract(_view(src, (n, h, w), torch.uint8).numpy(), _view(elem, (kh, kw), torch.uint8).numpy(), (ay, ax), op)
        _view(dst, (n, h, w), torch.uint8)[:] = torch.from_numpy(res)
        return 0


def header_defines():
    """{name: int} of the integer MGE_ #defines of include/michigan_hip/editing/mask_edit.h"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "michigan_hip", "editing", "mask_edit.h")) as fh:
        return {k: int(v) for k, v in re.findall(r"#define\s+(MGE_[A-Z_]+)\s+(\d+)\b", fh.read())}


def pointer(t):
    return ctypes.c_void_p(t.data_ptr())
