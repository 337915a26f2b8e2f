"""The stroke route, measured (GPU box):   python tools/bench_stroke_edit.py [--reps 100] [--cpu-reps 3] [--out FILE]

  * inputs.stroke_to_orient (one launch of mg_stroke_orient) at 1 x 512 x 512 -- one pen lift: seeded polylines of
    tests/stroke_fixtures.py, pens 1 .. 15, a few percent of the canvas -- at 8 x 512 x 512 of such canvases, on an empty canvas
    (every tile leaves at once: the launch and the zeros) and on a full one (no tile is skipped: the filter loop's own rate).
    Device events around `--reps` calls after a warm-up, five windows, median and spread.  A time per CALL, launch gap included, not a
    kernel time.  Beside it what the shapes say: the share of 16 x 16 tiles that hold a stroke pixel, and the fp32 FMAs those do.
  * the two glue launches at 1 x 512 x 512 <-> 256 x 256 (bf16 input of the net), and a whole Pix2PixModel(mode='demo_inference')
    stroke step at crop 512 with random weights (both frozen nets at 256 x 256 and the generator), bf16, host clock around a
    synchronised call.
  * the bf16 run of the stroke net and of both glue branches against the reference's fixture (tests/golden/stroke_glue.npz): mean /
    median / max |err|, the figures tests/test_gpu_stroke.py prints and does not yet bound.
The comparison line is the same canvas through the reference pipeline restated on the CPU (cal_orient_stroke.py:85-149 as torch:
32 conv2d calls, cat, clamp, arg-max, sin / cos, three mask multiplies, the byte conversion), timed in the same script with a host
clock.  The kernel is never compared against itself.  profiles/stroke_edit.txt is this script's output.
"""
import argparse
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import michigan_amd  # noqa: F401,E402
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from michigan_amd import inputs, ops  # noqa: E402

H = W = 512


def reference_pipeline(mask, bank):
    """cal_orient_stroke.py:85-149 on the CPU: mask u8 [H,W] in {0, 1} -> the float picture [H,W,3] the demo converts to uint8"""
    m = torch.from_numpy(np.uint8(mask * 255)).float().div(255)[None, None]
    res = torch.cat([F.conv2d(m, bank[k].view(1, 1, 17, 17), padding=8).clone() for k in range(32)], dim=1)
    res[res < 0] = 0
    a = (torch.argmax(res, dim=1).float() * math.pi / 32).unsqueeze(1)
    two = torch.cat([torch.sin(2 * a), torch.cos(2 * a)], dim=1) * m
    o, lab = two[0] * m[0], m[0]
    rgb = torch.cat([(o[1] * lab[0] + (1 - lab[0]) * -1)[None], (o[0] * lab[0] + (1 - lab[0]) * -1)[None], (o[0] * 0 * lab[0] + (1 - lab[0]) * -1)[None]], dim=0)
    return (np.transpose(rgb.numpy(), (1, 2, 0)) + 1) / 2.0 * 255.0


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def windows(fn, reps, nwin=5):
    for _ in range(10):
        fn()
    t = [timed(fn, reps) for _ in range(nwin)]
    return statistics.median(t), min(t), max(t)


def active_tiles(mask, th, tw):
    n, h, w = mask.shape
    m = np.zeros((n, -(-h // th) * th, -(-w // tw) * tw), bool)
    m[:, :h, :w] = mask != 0
    return int(m.reshape(n, m.shape[1] // th, th, m.shape[2] // tw, tw).any(axis=(2, 4)).sum()), n * (m.shape[1] // th) * (m.shape[2] // tw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--step-reps", type=int, default=10)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    assert args.reps >= 50
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    import stroke_fixtures as SE
    import test_stroke as TS
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    us = lambda t: "%8.1f us [%7.1f, %7.1f]" % (t[0] * 1e6, t[1] * 1e6, t[2] * 1e6)
    say("stroke editing, %d x %d canvases, %s, %d calls per window, 5 windows (median [min, max])" % (H, W, torch.cuda.get_device_name(0), args.reps))
    masks = {"one edit, 1 x": SE.polyline_mask(1, H, W, 512), "eight edits, 8 x": SE.polyline_mask(8, H, W, 513),
             "empty canvas, 1 x": np.zeros((1, H, W), np.uint8), "full canvas, 1 x": np.ones((1, H, W), np.uint8)}
    for name, m in masks.items():
        d = torch.from_numpy(m).cuda()
        t = windows(lambda: inputs.stroke_to_orient(d), args.reps)
        act, tiles = active_tiles(m, SE.TILE_H, SE.TILE_W)
        px = int((m != 0).sum())
        say("  inputs.stroke_to_orient, %-18s %s   stroke %5.2f %% of the canvas, %5d of %5d tiles filtered, %.3f GFLOP of fp32 FMAs at the stroke pixels (%.2f TFLOP/s)"
            % (name, us(t), 100.0 * px / m.size, act, tiles, px * 32 * 289 * 2e-9, px * 32 * 289 * 2 / t[0] * 1e-12))
    # the two glue launches
    t = TS._glue_tensors(1, H, W, 1)
    t = {k: v.cuda() for k, v in t.items()}
    net_out = torch.rand(1, 3, 256, 256, device="cuda")
    c = windows(lambda: ops.stroke_compose(t["orient_rgb"], t["noise"], t["hole"], t["stroke"], t["stroke_mask"], size=(256, 256), dtype=torch.bfloat16), args.reps)
    f = windows(lambda: ops.inpaint_finish(net_out, t["hole"], t["orient_rgb"], t["mask"]), args.reps)
    say("  ops.stroke_compose 512^2 -> 256^2 NHWC8 bf16    %s" % us(c))
    say("  ops.inpaint_finish 256^2 -> 512^2               %s" % us(f))
    # a whole demo_inference stroke step
    from michigan_amd.model import Pix2PixModel, default_options
    opt = default_options(gpu_ids=[0], isTrain=False, crop_size=H, compute_dtype="bf16", use_stroke=True, inpaint_mode="stroke", inpaint_orient=True, no_vgg_loss=True)
    torch.manual_seed(0)
    model = Pix2PixModel(opt).cuda().eval()
    batch = TS._demo_batch(1, H, device="cuda")
    for _ in range(3):
        model(batch, "demo_inference")
    ts = []
    for _ in range(args.step_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fake, orient_out = model(batch, "demo_inference")
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    say("  Pix2PixModel(mode='demo_inference'), inpaint_mode 'stroke', crop 512, bf16, batch 1 (stroke net at 256^2 + generator)   %8.2f ms [%.2f, %.2f] over %d steps"
        % (statistics.median(ts) * 1e3, min(ts) * 1e3, max(ts) * 1e3, len(ts)))
    stroke = SE.polyline_mask(1, H, W, 512)
    dm = torch.from_numpy(stroke).cuda()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    inputs.stroke_inputs(dm, batch["input_tag"][:, 1:2])
    torch.cuda.synchronize()
    say("  inputs.stroke_inputs (picture + the two loader tensors, 3 launches), host clock, one call   %8.1f us" % ((time.perf_counter() - t0) * 1e6))
    # bf16 against the reference's fixture
    import test_gpu_stroke as GS
    gold, cfg = GS._glue_fixture(), TS._cfg()
    x = torch.rand(cfg["n"], 5, cfg["size"], cfg["size"], generator=torch.Generator().manual_seed(cfg["seed_x"]))
    for dt, name in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        out = TS._net("SInpaintGenerator", "cuda", dt)(x.cuda()).cpu()
        e = (out - torch.from_numpy(gold["out"])).abs()
        say("  SInpaintGenerator %s vs the reference's fixture: mean |err| %.5f, median %.5f, max %.4f" % (name, e.mean(), e.median(), e.max()))
        shim = TS.glue_shim("cuda", dt)
        for branch in ("equal", "less"):
            rgb, o2 = TS.run_glue(shim, branch, "cuda")
            e1 = (rgb.cpu() - torch.from_numpy(gold["glue_%s.out_rgb" % branch])).abs()
            e2 = (o2.cpu() - torch.from_numpy(gold["glue_%s.orient" % branch])).abs()
            say("  inpainting_stroke_orient %s, branch %-5s: rgb mean %.5f, median %.5f, max %.4f | orient mean %.5f, median %.5f, max %.4f"
                % (name, branch, e1.mean(), e1.median(), e1.max(), e2.mean(), e2.median(), e2.max()))
    # the same canvas through the restated reference on the CPU
    cbank = ops.dog_bank()
    want = np.uint8(reference_pipeline(stroke[0], cbank))
    tc = []
    for _ in range(args.cpu_reps):
        t0 = time.perf_counter()
        reference_pipeline(stroke[0], cbank)
        tc.append(time.perf_counter() - t0)
    cpu = statistics.median(tc)
    one = windows(lambda: inputs.stroke_to_orient(dm), args.reps)
    say("  reference pipeline on the CPU (torch %d threads), the one-edit canvas   %8.1f ms [%.1f, %.1f] over %d runs  = %.0f x the launch"
        % (torch.get_num_threads(), cpu * 1e3, min(tc) * 1e3, max(tc) * 1e3, len(tc), cpu / one[0]))
    got = inputs.stroke_to_orient(dm).cpu().numpy()[0]
    s = stroke[0] != 0
    say("  same results: stroke pixels whose three bytes are equal %.4f %%, outside the stroke %d non-zero bytes"
        % (100 * (got[s] == want[s]).all(axis=-1).mean(), int((got[~s] != 0).sum())))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
