"""TEST INFRASTRUCTURE ONLY -- fixtures of the dense-orientation tests: the comparison rule for level maps (`rule2`, `compared`,
`circular`), the seeded strand images of tests/golden/dense_orient_i.npz (`make_sets`: the fixtures hold only what the reference
computed on them), the fixture loader, the float64 contract run over a fixture with one thing broken (`contract_on_fixture`,
`MUTANTS`) and `kernel_geometry`, the mirror of the kernel's tiling.  The contract itself is oracle/contracts.smooth_contract.
"""
import math
import os

import numpy as np
import torch

from oracle.contracts import ORIENT_RADIUS as RADIUS, argmax_contract, smooth_contract
from parity_utils import GOLDEN

MIN_REL_MAGNITUDE = 1e-3                 # pixels whose oracle flow magnitude is below this share of the in-mask maximum are not compared
MAX_EXCLUDED = 0.005
SYNTHETIC_SHAPES = ((17, 17), (33, 47), (70, 95))
CROP = (206, 72, 128)                    # set ii: row, column, side of the crop of sample 67172


def circular(a, b):
    """distance of two level maps on the circle of 255 levels (theta is an angle modulo pi)"""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return np.minimum(d, 255.0 - d)


def compared(mask, magnitude, magnitude_max):
    """(boolean map of the pixels the rule compares, number excluded, number in the mask): in-mask pixels whose oracle flow
    magnitude hypot(bx, by) is at least MIN_REL_MAGNITUDE of the SET's in-mask maximum."""
    m = np.asarray(mask) != 0
    keep = m & (np.asarray(magnitude, np.float64) >= MIN_REL_MAGNITUDE * magnitude_max)
    return keep, int(m.sum() - keep.sum()), int(m.sum())


def rule2(got, fixture, angle_factor=8.0):
    """Acceptance rule 2 over every geometry of a fixture (load_set): got = {geometry: dict(u8, theta)}.  Bytes equal on >= 99.5 % of
    the compared pixels, within one level on all of them, the angle within angle_factor x the reference's own fp32-vs-float64 gap;
    at most 0.5 % of the in-mask pixels excluded.  The rule looks at in-mask pixels only, which cannot see the final mask multiply, so
    this adds: outside the mask every byte equals the reference's (0).  Returns (passed, figures)."""
    d, gap, excluded, inmask, outside = [], [], 0, 0, 0
    for geo, rec in fixture["geometries"].items():
        keep, ex, im = compared(rec["mask"], rec["magnitude"], fixture["magnitude_max"])
        excluded, inmask = excluded + ex, inmask + im
        out = np.asarray(rec["mask"]) == 0
        outside += int((np.asarray(got[geo]["u8"])[out] != rec["u8"][out]).sum())
        d.append(circular(np.asarray(got[geo]["u8"])[keep], rec["u8"][keep]))
        gap.append(circular(np.asarray(got[geo]["theta"], np.float64)[keep] * 255.0 / math.pi, rec["level"][keep]))
    d, gap = np.concatenate(d), np.concatenate(gap)
    fig = dict(excluded=excluded / inmask, equal=float((d == 0).mean()), within1=float((d <= 1).mean()), worst=float(d.max()),
               angle_gap=float(gap.max()), angle_bound=angle_factor * fixture["ref32_level_gap"], compared=int(d.size), outside_unequal=outside)
    ok = outside == 0 and fig["excluded"] <= MAX_EXCLUDED and fig["equal"] >= 0.995 and fig["within1"] == 1.0 and fig["angle_gap"] <= fig["angle_bound"]
    return ok, fig


MUTANTS = ("edge_duplicating_reflection", "angle_step_pi_32", "taps_25", "no_mask_multiply", "bank_xy_swapped", "round_to_uint8")


def contract_on_fixture(fixture, mutant=None):
    """{geometry: dict(u8, theta)}: smooth_contract with the host tables of michigan_amd.ops, fed with the reference's idx and conf (as
    the fp32 the kernel takes).  `mutant` (one of MUTANTS) breaks one thing the fixtures must notice."""
    from michigan_amd import ops
    assert mutant is None or mutant in MUTANTS
    trig, taps = ops.orient_trig_table().numpy(), ops.gaussian_taps(4.0).numpy()
    if mutant == "angle_step_pi_32":
        a = torch.arange(32, dtype=torch.float32) * math.pi / 32 * 2
        trig = torch.stack([torch.cos(a), torch.sin(a)], dim=1).numpy()
    if mutant == "taps_25":                                  # cv2's rule for an 8-bit source: ksize = round(sigma * 3 * 2 + 1) | 1
        x = np.arange(-12, 13, dtype=np.float64)
        t = np.exp(-x * x / 32.0)
        taps = (t / t.sum()).astype(np.float32)
    out = {}
    for geo, rec in fixture["geometries"].items():
        conf, idx = rec["conf"], rec["idx"]
        if mutant == "bank_xy_swapped":
            conf, idx = argmax_contract(image_fp32(torch.from_numpy(rec["image"])), torch.from_numpy(fixture["bank"]).transpose(1, 2).contiguous())
        out[geo] = smooth_contract(conf.astype(np.float32), idx, rec["mask"], trig, taps, reflect101=mutant != "edge_duplicating_reflection",
                                   mask_multiply=mutant != "no_mask_multiply", truncate=mutant != "round_to_uint8")
    return out


# ---- the inputs of the fixtures ----------------------------------------------------------------------------------------------------------
def strand_image(n, h, w, seed):
    """uint8 RGB [n,h,w,3] of hair-like strands: a grating of ~5 pixel wavelength along an orientation field that bends across the
    image, a slow brightness ramp and +-6 levels of seeded noise; and the elliptical uint8 mask [n,h,w] (0 / 1)."""
    g = torch.Generator().manual_seed(seed)
    y = torch.arange(h, dtype=torch.float64).view(1, h, 1)
    x = torch.arange(w, dtype=torch.float64).view(1, 1, w)
    phi0 = torch.rand(n, 1, 1, generator=g, dtype=torch.float64) * math.pi
    bend = 0.5 + torch.rand(n, 1, 1, generator=g, dtype=torch.float64)
    lam = 4.5 + 2.0 * torch.rand(n, 1, 1, generator=g, dtype=torch.float64)
    phi = phi0 + bend * torch.sin(y / max(h, 40) * 2.2 + x / max(w, 40) * 1.3)
    # phase advances across the strands; integrating the bend exactly does not matter for a test image
    phase = 2 * math.pi * (x * torch.cos(phi) + y * torch.sin(phi)) / lam
    lum = 120 + 70 * torch.sin(phase) + 20 * torch.sin(y / 9.0 + x / 13.0) + 12 * (torch.rand(n, h, w, generator=g, dtype=torch.float64) - 0.5)
    tint = torch.tensor([1.0, 0.85, 0.7], dtype=torch.float64).view(1, 1, 1, 3)
    img = (lum.unsqueeze(-1) * tint).round().clamp(0, 255).to(torch.uint8)
    cy, cx = (h - 1) / 2.0, (w - 1) / 2.0
    mask = ((((y - cy) / (0.46 * h)) ** 2 + ((x - cx) / (0.42 * w)) ** 2) <= 1.0).expand(n, h, w).to(torch.uint8)
    return img.contiguous(), mask.contiguous()


def make_sets():
    """{"i": {"17x17": dict(image u8 [2,h,w,3], mask u8 [2,h,w]), "33x47": ..., "70x95": ...}} -- set ii is pixels of the bundled
    sample and lives in its fixture."""
    return {"i": {"%dx%d" % (h, w): dict(zip(("image", "mask"), strand_image(2, h, w, 1000 + h))) for h, w in SYNTHETIC_SHAPES}}


def image_fp32(image_u8):
    """ToTensor + Normalize(0.5, 0.5) in fp32 (cal_orientation.py:93): u8 [N,H,W,3] -> fp32 [N,H,W,3] in [-1, 1]"""
    return ((image_u8.to(torch.float32) / 255) - 0.5) / 0.5


def load_set(tag):
    """tests/golden/dense_orient_<tag>.npz as {geometry: record} + {"bank", "bank_maxabs_diff"}; a record is a dict of arrays
    (idx, conf, level, u8, magnitude, mask, image; scalars as Python numbers).  The synthetic set's image and mask are regenerated
    from their seed."""
    z = np.load(os.path.join(GOLDEN, "dense_orient_%s.npz" % tag))
    out = {"geometries": {}}
    for k in z.files:
        v = z[k] if z[k].ndim else z[k].item()
        if "/" in k:
            geo, name = k.split("/")
            out["geometries"].setdefault(geo, {})[name] = v
        else:
            out[k] = v
    if tag == "i":
        for geo, p in make_sets()["i"].items():
            out["geometries"][geo].update(image=p["image"].numpy(), mask=p["mask"].numpy())
    return out


# ---- the kernel's tiling (michigan_amd/csrc/mg_orient_smooth.hip), for the tests that sit on its edges --------------------------------
TILE_H, TILE_W = 32, 32


def kernel_geometry(n, h, w):
    """dict(tile_h, tile_w, tiles_y, tiles_x, blocks, patch_h, patch_w): a workgroup owns a tile_h x tile_w output tile and loads it
    with a 16-pixel halo.  tests/test_gpu_dense_orient.py asserts TILE_H / TILE_W against the header's MG_ORIENT_TILE_*, which the
    kernel is compiled from, so a change of the tile that this mirror misses fails loudly instead of moving the cases off the edges."""
    ty, tx = -(-h // TILE_H), -(-w // TILE_W)
    return dict(tile_h=TILE_H, tile_w=TILE_W, tiles_y=ty, tiles_x=tx, blocks=n * ty * tx, patch_h=TILE_H + 2 * RADIUS, patch_w=TILE_W + 2 * RADIUS)
