"""TEST INFRASTRUCTURE ONLY -- fixtures of the stroke-editing tests: the comparison rule of tests/test_stroke.py (`rule`), the seeded
polyline masks of tests/golden/stroke_i.npz (`make_masks`: the fixture holds only what the reference computed on them), the seeded
inputs of the glue entry points (`glue_inputs`), the fixture loader, the float64 contract run over a fixture with one thing broken
(`contract_on_fixture`, `MUTANTS`) and `kernel_geometry`, the mirror of the kernel's tiling.  The contracts themselves are
oracle/contracts.stroke_contract, compose_contract and finish_contract.
"""
import os

import numpy as np
import torch

from oracle.contracts import STROKE_MUTANTS as MUTANTS, responses, stroke_contract
from parity_utils import GOLDEN

SHAPES = ((17, 17), (33, 47), (70, 95), (128, 128))
WIDTHS = (1, 15)                         # the pen widths of the UI
MAX_UNDECIDED = 0.10                     # share of stroke pixels whose float64 top-two gap is below tau
TAU_FACTOR = 4.0                         # a 289-term fp32 sum taken in another order may err a few times more than ATen's


def rule(got, fixture, max_undecided=MAX_UNDECIDED):
    """The comparison rule over every geometry of the fixture (load_set): got = {geometry: dict(rgb, idx, conf)}.  With tau = 4 x the
    larger of the reference's own fp32-against-float64 figures:
      * at every stroke pixel the float64 response of the returned idx is within tau of the float64 maximum, and |conf - max| <= tau;
      * idx is the reference's (its float64 run) wherever the float64 top-two gap is >= tau; at most 10 % of the stroke pixels are below;
      * given idx, the RGB bytes are rgb_table[idx] exactly; outside the stroke every byte, idx and conf is 0;
      * where every float64 response is below -tau, idx and conf are 0: the clamp ties all 32 exactly at 0 in any arithmetic that is
        within tau, so "the first" is decided there although the gap is 0 (this is what sees an arg-max taken before the clamp, or
        the last one taken).
    max_undecided=None: the cap on undecided pixels is a condition on the FIXTURE's masks (the tool asserts it); the small masks of the
    guarded GPU cases are judged without it.  Returns (passed, figures)."""
    tau = fixture["tau"]
    short, conf_err, wrong, undecided, pixels, bytes_wrong, outside, tie_pixels, tie_wrong = 0.0, 0.0, 0, 0, 0, 0, 0, 0, 0
    for geo, rec in fixture["geometries"].items():
        g = got[geo]
        s = rec["mask"] != 0
        resp = np.maximum(rec["resp"], 0.0)
        top = resp.max(axis=1)
        idx = np.asarray(g["idx"]).astype(np.int64)
        taken = np.take_along_axis(resp, idx[:, None], axis=1)[:, 0]
        if s.any():
            short = max(short, float((top - taken)[s].max()))
            conf_err = max(conf_err, float(np.abs(np.asarray(g["conf"], np.float64) - top)[s].max()))
        decided = s & (rec["gap"] >= tau)
        wrong += int((idx != rec["idx"])[decided].sum())
        undecided += int((s & ~decided).sum())
        pixels += int(s.sum())
        bytes_wrong += int((np.asarray(g["rgb"])[s] != fixture["rgb_table"][idx[s]]).sum())
        tie = s & (rec["resp"].max(axis=1) < -tau)
        tie_pixels += int(tie.sum())
        tie_wrong += int(((idx != 0) | (np.asarray(g["conf"]) != 0))[tie].sum())
        outside += int(np.asarray(g["rgb"])[~s].astype(bool).sum() + idx[~s].astype(bool).sum() + (np.asarray(g["conf"])[~s] != 0).sum())
    fig = dict(tau=tau, response_short=short, conf_err=conf_err, idx_wrong_where_decided=wrong, undecided=undecided / max(pixels, 1), stroke_pixels=pixels,
               rgb_bytes_wrong=bytes_wrong, outside_nonzero=outside, clamped_tie_pixels=tie_pixels, clamped_tie_wrong=tie_wrong)
    ok = (short <= tau and conf_err <= tau and wrong == 0 and (max_undecided is None or fig["undecided"] <= max_undecided) and bytes_wrong == 0 and outside == 0 and tie_wrong == 0)
    return ok, fig


# The reference's bank is point-symmetric bit for bit (DoG_fn squares the rotated coordinates), so on it a convolution IS the
# correlation and no fixture of the reference can tell them apart.  That mutant is judged on a seeded bank without the symmetry,
# where the oracle is the float64 contract itself (F.conv2d, the operator the reference calls, is a correlation).
JUDGED_ON_ASYMMETRIC_BANK = ("convolution",)


def asymmetric_bank(seed=77):
    bank = (torch.randn(32, 17, 17, generator=torch.Generator().manual_seed(seed)) * 0.1).numpy()
    assert not np.array_equal(bank, bank[:, ::-1, ::-1])
    return bank


def asymmetric_fixture(fixture, bank=None):
    """the fixture's masks under a seeded bank without point symmetry (or `bank`): idx / gap / resp are the float64 contract's"""
    bank = asymmetric_bank() if bank is None else bank
    out = dict(fixture, bank=bank, geometries={})
    for geo, rec in fixture["geometries"].items():
        resp = responses(rec["mask"], bank)
        c = np.sort(np.maximum(resp, 0.0), axis=1)
        s = rec["mask"] != 0
        out["geometries"][geo] = dict(mask=rec["mask"], resp=resp, idx=np.where(s, np.maximum(resp, 0.0).argmax(axis=1), 0).astype(np.uint8),
                                      gap=np.where(s, c[:, -1] - c[:, -2], 0.0))
    return out


def pseudo_fixture(mask, bank, like):
    """a fixture of one geometry ("case") whose oracle is the float64 contract on `mask` under `bank`; tau and the colour table are
    those of the fixture `like`"""
    return asymmetric_fixture(dict(like, geometries={"case": dict(mask=np.asarray(mask))}), bank=np.asarray(bank))


def fixture_for(fixture, mutant):
    return asymmetric_fixture(fixture) if mutant in JUDGED_ON_ASYMMETRIC_BANK else fixture


def contract_on_fixture(fixture, mutant=None):
    from michigan_amd import ops
    return {geo: stroke_contract(rec["mask"], fixture["bank"], ops.stroke_rgb_table().numpy(), mutant) for geo, rec in fixture["geometries"].items()}


# ---- the inputs of the fixture -------------------------------------------------------------------------------------------------------
def polyline_mask(n, h, w, seed):
    """uint8 [n,h,w] in {0, 1}: per sample three to five seeded polylines drawn with PIL.ImageDraw.line, pen widths 1 .. 15 (the UI's
    range), as the demo's scene draws a stroke.  Width and direction vary so that all 32 filter indices occur."""
    from PIL import Image, ImageDraw
    rng = np.random.RandomState(seed)
    out = np.zeros((n, h, w), np.uint8)
    for i in range(n):
        img = Image.new("L", (w, h), 0)
        draw = ImageDraw.Draw(img)
        for _ in range(int(rng.randint(3, 6))):
            k = int(rng.randint(2, 5))
            pts = np.stack([rng.uniform(-2, w + 2, k), rng.uniform(-2, h + 2, k)], axis=1)
            # log-uniform from 1 to an eighth of the canvas, at most the UI's 15: a wider pen would cover a small canvas, and the
            # interiors of the widest pens are flat -- genuinely undecided pixels, which the rule caps at 10 %
            width = int(round(min(WIDTHS[1], max(2, min(h, w) // 8)) ** rng.uniform(0, 1)))
            draw.line([tuple(p) for p in pts.round().astype(int).tolist()], fill=1, width=width)
        if i == 0 and min(h, w) >= 64:
            # a dot inside a closed square polyline of pen 1, three pixels away: at the dot every filter's negative lobes outweigh its
            # centre, all 32 responses are below zero and the clamp ties them (the tool asserts that this happens)
            cy, cx, a = h - 10, 10, 3
            draw.line([(cx - a, cy - a), (cx + a, cy - a), (cx + a, cy + a), (cx - a, cy + a), (cx - a, cy - a)], fill=1, width=1)
            draw.line([(cx, cy), (cx, cy)], fill=1, width=1)
        out[i] = np.array(img)
    return out


def make_masks():
    """{"17x17": u8 [2,17,17], "33x47": ..., "70x95": ..., "128x128": ...}"""
    return {"%dx%d" % (h, w): polyline_mask(2, h, w, 4000 + 10 * h + w) for h, w in SHAPES}


def glue_inputs(seed, crop=32):
    """the seeded inputs of both glue branches (tests/test_stroke.py regenerates them): non-binary hole / stroke masks are legal
    arithmetic and exercise every term"""
    g = torch.Generator().manual_seed(seed)
    r = lambda c: torch.rand(1, c, crop, crop, generator=g)
    hole, orient_rgb, noise = (r(1) > 0.6).float(), r(3), r(3)
    mask = (r(1) > 0.3).float()
    stroke, stroke_mask = r(3), (r(1) > 0.8).float() * hole
    return dict(hole=hole, orient_rgb=orient_rgb, noise=noise, mask=mask, stroke=stroke, stroke_mask=stroke_mask,
                mask_orient_rgb_equal=mask.clone(), mask_orient_rgb_less=mask * (r(1) > 0.25).float())


def load_set(tag="i"):
    """tests/golden/stroke_<tag>.npz as {"geometries": {geometry: record}, "bank", "rgb_table", "ref32_gap_at_flip", "ref32_resp_err", "tau"};
    a record holds the reference's rgb (u8 [N,H,W,3], its fp32 run) and idx / conf / gap of its float64 run; the mask is regenerated from
    its seed, and resp (float64 [N,32,H,W]) is computed here from the mask and the fixture's bank."""
    z = np.load(os.path.join(GOLDEN, "stroke_%s.npz" % tag))
    out = {"geometries": {}}
    for k in z.files:
        v = z[k] if z[k].ndim else z[k].item()
        if "/" in k:
            geo, name = k.split("/")
            out["geometries"].setdefault(geo, {})[name] = v
        else:
            out[k] = v
    for geo, m in make_masks().items():
        out["geometries"][geo].update(mask=m, resp=responses(m, out["bank"]))
    out["tau"] = TAU_FACTOR * max(out["ref32_gap_at_flip"], out["ref32_resp_err"])
    return out


# ---- the kernel's tiling (michigan_amd/csrc/mg_stroke.hip), for the tests that sit on its edges -----------------------------------------
TILE_H, TILE_W = 16, 16


def kernel_geometry(n, h, w):
    """dict(tile_h, tile_w, tiles_y, tiles_x, blocks): a workgroup owns a tile_h x tile_w output tile and loads it with an 8-pixel halo.
    tests/test_gpu_stroke.py asserts TILE_H / TILE_W against the header's MG_STROKE_TILE_*, which the kernel is compiled from."""
    ty, tx = -(-h // TILE_H), -(-w // TILE_W)
    return dict(tile_h=TILE_H, tile_w=TILE_W, tiles_y=ty, tiles_x=tx, blocks=n * ty * tx)
