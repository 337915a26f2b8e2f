"""Generate the fixtures of the stroke route by running the REFERENCE's own modules:

    python tools/make_stroke_golden.py        (where the reference checkout is; CPU, about a minute)

  tests/golden/stroke_i.npz     seeded polyline masks (tests/stroke_fixtures.make_masks: N = 2 at 17x17, 33x47, 70x95 and 128x128, drawn with
        PIL.ImageDraw.line, pen widths 1 .. 15; the fixture holds RESULTS only, the masks are regenerated from their seed)
  tests/golden/stroke_glue.npz  the reference's SInpaintGenerator (eval, synth_state_dict weights, the recipe of inpaint_config.json) on a
        seeded 5-channel 64 x 64 input, and the unbound Pix2PixModel.inpainting_stroke_orient at crop 32 on both of its branches
        (mask == mask_orient_rgb, and not: there also what the first in-painting returned, glue_less.first_rgb)
  tests/golden/sinpaint_state_dict_contract.json   the 124 keys and shapes of its state_dict, in order

What runs: ui_util/cal_orient_stroke.py as imported -- orient().stroke_to_orient(mask) as demo.py:325-326 calls it (fp32; np.uint8 of
its result is the picture), and orient().calOrientation on the same mask as a float64 image (the oracle the tests compare against).
The only change to the imported code is the `F` it sees: conv2d casts the filter, which DoG_fn ends with `.float()`, to the image's
dtype, so that the float64 run correlates in float64, and keeps a copy of each of the 32 responses it returns -- the module keeps
only their arg-max.  Nothing of the reference is restated here.

Per geometry "<h>x<w>/": rgb (u8 [2,h,w,3], the fp32 run), idx (u8), conf (float64), gap (float32: the top-two gap of the clamped
responses) of the float64 run.  Per set: bank (DoG_fn's 32 kernels), rgb_table (u8 [32,3]: the colour the fp32 run gave each of its
indices), and the reference's own fp32-against-float64 figures over the stroke pixels: ref32_gap_at_flip (largest float64 top-two gap
at a pixel where its fp32 arg-max differs) and ref32_resp_err (largest response difference).

Asserted here, so that no test needs an exclusion list: all 32 indices occur inside the strokes, each with one colour; at most 10 % of
the stroke pixels have a float64 top-two gap below tau; the reference's fp32 run meets the rule of tests/stroke_fixtures.rule against
its float64 run; the float64 contract meets it; every mutant of tests/stroke_fixtures.MUTANTS fails it (`convolution` on a seeded bank:
the reference's bank is point-symmetric bit for bit, which is asserted too, so on it a convolution is the correlation).
"""
import json
import math
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden")


def save_npz(path, rec):
    """np.savez_compressed with a fixed member date: the same arrays give the same bytes on any day"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(rec):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(rec[name]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), compress_type=zipfile.ZIP_DEFLATED)


class Recorder:
    """stands in for the module's `F`: conv2d in the image's dtype, a copy of every response kept"""

    def __init__(self):
        self.responses = []

    def conv2d(self, image, kernel, **kw):
        import torch.nn.functional as F
        r = F.conv2d(image, kernel.to(image.dtype), **kw)
        self.responses.append(r.detach().clone())
        return r

    def take(self):
        r, self.responses = self.responses, []
        assert len(r) == 32
        return torch.cat(r, dim=1)[0].numpy()                         # [32, H, W]


def reference_module():
    """ui_util/cal_orient_stroke.py (its top level only defines), with cv2 / torchvision / matplotlib stubbed where they are missing"""
    from oracle import ref_harness as R
    R.setup()
    for name in ("matplotlib", "matplotlib.pyplot"):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    import ui_util.cal_orient_stroke as CS
    CS.F = Recorder()
    return CS


def reference_bank(CS):
    """The 32 kernels calOrientation builds (cal_orient_stroke.py:88-92), fp32 [32,17,17]"""
    ks = []
    for k in range(32):
        theta = torch.nn.Parameter(torch.ones(1) * (math.pi * k / 32), requires_grad=False)
        ks.append(CS.DoG_fn(17, 1, 1, theta).float()[0, 0])
    return torch.stack(ks)


def reference_run(CS, mask):
    """One sample, mask u8 [H,W] in {0, 1} -> (rgb u8 [H,W,3] and responses [32,H,W] of the fp32 run, responses of the float64 run)"""
    with torch.no_grad():
        rgb = np.uint8(CS.orient().stroke_to_orient(mask))
        r32 = CS.F.take()
        CS.orient().calOrientation(torch.from_numpy(mask.astype(np.float64))[None, None])
        r64 = CS.F.take()
    assert r32.dtype == np.float32 and r64.dtype == np.float64
    return rgb, r32, r64


def summarise(resp):
    """clamp, first arg-max, max and top-two gap of responses [32,H,W] -- what calOrientation keeps, and the gap"""
    c = np.maximum(resp, 0)
    top2 = np.sort(c, axis=0)[-2:]
    return c.argmax(axis=0).astype(np.uint8), c.max(axis=0), (top2[1] - top2[0])


def make_stroke_set(CS, tag="i"):
    import stroke_fixtures as SE
    from michigan_amd import ops
    bank = reference_bank(CS)
    rec = {"bank": bank.numpy()}
    table = np.full((32, 3), -1, np.int64)
    gap_at_flip, resp_err, undecided_px, pixels = 0.0, 0.0, [], 0
    ref32 = {}
    for geo, masks in SE.make_masks().items():
        runs = [reference_run(CS, m) for m in masks]
        s = masks != 0
        rgb = np.stack([r[0] for r in runs])
        s32 = [summarise(r[1]) for r in runs]
        s64 = [summarise(r[2]) for r in runs]
        idx32, conf32 = np.stack([a[0] for a in s32]), np.stack([a[1] for a in s32])
        idx64, conf64, gap64 = (np.stack([a[i] for a in s64]) for i in range(3))
        rec.update({geo + "/rgb": rgb, geo + "/idx": np.where(s, idx64, 0).astype(np.uint8), geo + "/conf": np.where(s, conf64, 0.0),
                    geo + "/gap": np.where(s, gap64, 0.0).astype(np.float32)})
        ref32[geo] = dict(rgb=rgb, idx=np.where(s, idx32, 0), conf=np.where(s, conf32, 0.0))
        assert not rgb[~s].any(), "the reference's picture is not black outside the stroke"
        for k in range(32):                                           # the colour of each index, from the picture itself
            colours = np.unique(rgb[s & (idx32 == k)], axis=0)
            assert len(colours) <= 1, (geo, k, colours)
            if len(colours):
                assert table[k, 0] < 0 or (table[k] == colours[0]).all(), (geo, k)
                table[k] = colours[0]
        flips = s & (idx32 != idx64)
        if flips.any():
            gap_at_flip = max(gap_at_flip, float(gap64[flips].max()))
        d = np.abs(np.stack([r[1] for r in runs]).astype(np.float64) - np.stack([r[2] for r in runs]))
        resp_err = max(resp_err, float(d[np.broadcast_to(s[:, None], d.shape)].max()))
        pixels += int(s.sum())
        undecided_px.append(gap64[s])
        print("  %-8s stroke pixels %6d (%.1f %% of the canvas), fp32 arg-max flips %d" % (geo, s.sum(), 100 * s.mean(), flips.sum()))
    assert (table >= 0).all(), "indices that never occur inside a stroke: %s" % np.nonzero(table[:, 0] < 0)[0]
    rec.update(rgb_table=table.astype(np.uint8), ref32_gap_at_flip=np.array(gap_at_flip), ref32_resp_err=np.array(resp_err))
    assert np.array_equal(rec["rgb_table"], ops.stroke_rgb_table().numpy()), "ops.stroke_rgb_table is not the reference's colouring"
    path = os.path.join(OUT, "stroke_%s.npz" % tag)
    save_npz(path, rec)
    fx = SE.load_set(tag)
    tau = fx["tau"]
    undecided = float((np.concatenate(undecided_px) < tau).mean())
    print("set %s: %d stroke pixels | reference fp32 vs float64: gap at flip %.3g, response error %.3g -> tau %.3g | undecided %.2f %% | dog_bank max abs diff %.3g"
          % (tag, pixels, gap_at_flip, resp_err, tau, 100 * undecided, float((ops.dog_bank() - bank).abs().max())))
    assert undecided <= SE.MAX_UNDECIDED
    ok, fig = SE.rule(ref32, fx)
    print("  the reference's fp32 run:", fig)
    assert ok, "the reference's fp32 run misses the rule against its float64 run"
    ok, fig = SE.rule(SE.contract_on_fixture(fx), fx)
    print("  the float64 contract:   ", fig)
    assert ok, "the float64 contract misses the rule"
    assert fig["clamped_tie_pixels"] >= 2, "no stroke pixel with every response below zero: the clamp's tie is not exercised"
    assert np.array_equal(rec["bank"], rec["bank"][:, ::-1, ::-1]), "the bank is no longer point-symmetric: judge `convolution` on the fixture"
    for mutant in SE.MUTANTS:
        on = SE.fixture_for(fx, mutant)                               # `convolution`: a seeded bank without the reference bank's symmetry
        ok, fig = SE.rule(SE.contract_on_fixture(on), on)
        assert ok, fig
        ok, fig = SE.rule(SE.contract_on_fixture(on, mutant), on)
        print("  mutant %-20s %s %s" % (mutant, "PASSES" if ok else "fails", {k: fig[k] for k in ("response_short", "idx_wrong_where_decided", "rgb_bytes_wrong", "outside_nonzero", "clamped_tie_wrong")}))
        assert not ok, "the set does not reject the mutant %s" % mutant
    return path


def make_glue():
    from oracle import ref_harness as R
    from michigan_amd.synth import synth_state_dict
    R.setup()
    from models.networks.generator import SInpaintGenerator
    from models.pix2pix_model import Pix2PixModel
    with open(os.path.join(OUT, "inpaint_config.json")) as fh:
        cfg = json.load(fh)
    opt = R.make_opt()
    sig = SInpaintGenerator(opt).eval()
    sig.load_state_dict(synth_state_dict(sig.state_dict(), seed=cfg["seed_w"], gain=cfg["gain"]))
    ig = R.build_inpaint(opt).eval()
    ig.load_state_dict(synth_state_dict(ig.state_dict(), seed=cfg["seed_w"], gain=cfg["gain"]))
    x = torch.rand(cfg["n"], 5, cfg["size"], cfg["size"], generator=torch.Generator().manual_seed(cfg["seed_x"]))
    with torch.no_grad():
        rec = {"out": sig(x).numpy()}
    crop = 32
    shim = types.SimpleNamespace(opt=types.SimpleNamespace(crop_size=crop), netIG=ig, netSIG=sig)
    first = []

    def inpainting_orient(*args):                                     # the method itself; what it returned is kept (the `less` branch's first stage)
        res = Pix2PixModel.inpainting_orient(shim, *args)
        first.append(res[0].numpy().copy())
        return res
    shim.inpainting_orient = inpainting_orient
    import stroke_fixtures as SE
    t = SE.glue_inputs(cfg["seed_x"] + 1, crop)
    for branch in ("equal", "less"):
        with torch.no_grad():
            rgb, o2 = Pix2PixModel.inpainting_stroke_orient(shim, t["hole"], t["orient_rgb"], t["noise"], t["mask"], t["stroke"], t["stroke_mask"],
                                                            t["mask_orient_rgb_" + branch])
        rec.update({"glue_%s.out_rgb" % branch: rgb.numpy(), "glue_%s.orient" % branch: o2.numpy()})
    assert not np.array_equal(rec["glue_equal.out_rgb"], rec["glue_less.out_rgb"]) and len(first) == 1
    rec["glue_less.first_rgb"] = first[0]                             # orient_rgb_1 of pix2pix_model.py:438: what the second net was fed from
    path = os.path.join(OUT, "stroke_glue.npz")
    save_npz(path, rec)
    contract = os.path.join(OUT, "sinpaint_state_dict_contract.json")
    with open(contract, "w") as fh:
        json.dump({k: list(v.shape) for k, v in sig.state_dict().items()}, fh)
    assert len(sig.state_dict()) == 124
    print("stroke glue: net out mean %.4f std %.4f" % (rec["out"].mean(), rec["out"].std()))
    return [path, contract]


if __name__ == "__main__":
    CS = reference_module()
    paths = [make_stroke_set(CS)] + make_glue()
    for p in paths:
        size = os.path.getsize(p)
        assert size < 1 << 20, (p, size)
        print("%8d  %s" % (size, os.path.basename(p)))
