"""The headless editing session, measured (GPU box):   python tools/bench_edit_session.py [--reps 200] [--step-reps 20] [--out FILE]

  * mge_brush_u8 at 1 x 512 x 512: 200 seeded pen segments of thickness 1 .. 15 (polylines, the UI's pens), through ops.brush_u8 with
    the list already on the device.  mge_morph_u8 with the 50 x 50 ellipse at 1 x 512 x 512 and 8 x 512 x 512: on a drawn stroke mask
    (what the demo dilates: most tiles see an all-zero halo and leave) and on a dense grey map (no tile leaves: the tap walk's own
    rate), dilation and erosion.  Device events around `--reps` calls (the brush: 100 x as many) after a warm-up, five windows, median and spread: a time per
    CALL, launch gap included, not a kernel time.  Beside it what the shapes say: segments kept per tile, taps per pixel.
    `--kernels-only` runs just these calls (for a kernel trace taken in a run of its own).
  * EditSession.edit() end to end at crop 512 in bf16 (random weights, stroke route, the edited mask, a reconstruction image), host
    clock around a synchronised call: three brush calls, the dilation, the one read-back, demo_batch, the model, the byte conversion.
    The baseline, in the same process and alternating with it: the same step assembled by hand from what existed before the session
    -- the two masks made on the host BEFOREHAND (outside the clock: the most favourable case for the baseline, which on the GPU
    image has no OpenCV to make them with), then inside the clock their upload, demo_batch, the model and the byte conversion.
    Both produce the same bytes (asserted).  Acceptance: median(edit) - median(baseline) <= max(baseline) - min(baseline).
profiles/edit_session.txt is this script's output.
"""
import argparse
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import michigan_amd  # noqa: F401,E402
import numpy as np  # noqa: E402
import torch  # noqa: E402
from michigan_amd import inputs, ops  # noqa: E402

H = W = 512


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


def pen_walk(n_segments, seed, lo=96, hi=416):
    """a pen record of the UI's kind: polylines of 10 segments, steps of up to 24 pixels, pens 1 .. 15, inside [lo, hi)^2"""
    r = random.Random(seed)
    points, sizes = [], []
    while len(points) < n_segments:
        x, y, size = r.randrange(lo, hi), r.randrange(lo, hi), r.randint(1, 15)
        for _ in range(min(10, n_segments - len(points))):
            nx, ny = min(max(x + r.randint(-24, 24), lo), hi - 1), min(max(y + r.randint(-24, 24), lo), hi - 1)
            points.append({"prev": (x, y), "curr": (nx, ny)})
            sizes.append(size)
            x, y = nx, ny
    return points, sizes


def kept_per_tile(segs, tile=16):
    """mean / max number of segments whose pen-widened box meets a 16 x 16 tile (what a workgroup walks)"""
    s = np.asarray(segs, np.int64)
    r = (s[:, 5] + 1) // 2
    x0, x1 = np.minimum(s[:, 1], s[:, 3]) - r, np.maximum(s[:, 1], s[:, 3]) + r
    y0, y1 = np.minimum(s[:, 2], s[:, 4]) - r, np.maximum(s[:, 2], s[:, 4]) + r
    counts = [int(((x0 <= tx + tile - 1) & (x1 >= tx) & (y0 <= ty + tile - 1) & (y1 >= ty)).sum()) for ty in range(0, H, tile) for tx in range(0, W, tile)]
    return statistics.mean(counts), max(counts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--step-reps", type=int, default=20)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    assert args.reps >= 50
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    import mask_edit_fixtures as MF
    import stroke_fixtures as SE
    import test_mask_edit as TM
    from michigan_amd.demo import EditSession, pen_segments
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    us = lambda t: "%8.1f us [%7.1f, %7.1f]" % (t[0] * 1e6, t[1] * 1e6, t[2] * 1e6)
    say("editing session, %d x %d canvases, %s, %d calls per window, 5 windows (median [min, max])" % (H, W, torch.cuda.get_device_name(0), args.reps))
    # the brush
    points, sizes = pen_walk(200, 7)
    segs = pen_segments(points, sizes, 2)
    dsegs = inputs.upload(inputs.brush_segments(segs, 1, H, W), "cuda")
    canvas = torch.zeros(1, H, W, dtype=torch.uint8, device="cuda")
    brush_reps = 100 * args.reps                                           # a call of a few microseconds: a window of 0.1 s, not of 1 ms
    t = windows(lambda: ops.brush_u8(canvas, dsegs), brush_reps)
    want = MF.brush_contract(np.zeros((1, H, W), np.uint8), segs)
    assert np.array_equal(canvas.cpu().numpy(), want)
    mean_kept, max_kept = kept_per_tile(segs)
    say("  ops.brush_u8 (mge_brush_u8), 200 segments, pens 1 .. 15, 1 x           %s   %d calls per window; %.2f %% of the canvas painted, segments kept per tile: mean %.1f, max %d"
        % (us(t), brush_reps, 100.0 * (want != 0).mean(), mean_kept, max_kept))
    # the dilation / erosion
    e = inputs.ellipse_element(50)
    taps = int(e.sum())
    for n in (1, 8):
        stroke = torch.from_numpy(SE.polyline_mask(n, H, W, 512 + n)).cuda()
        grey = torch.from_numpy(MF.grey_planes(n, H, W, 9)).cuda()
        grey[:, : H // 3, : W // 4] = 1                                    # no all-zero halo anywhere: every tile walks its taps
        live = int((inputs.stroke_hole(stroke) != 0).sum())
        for name, fn in (("dilate, a stroke mask", lambda: inputs.stroke_hole(stroke)), ("dilate, dense grey", lambda: inputs.dilate_u8(grey, e)),
                         ("erode, dense grey", lambda: inputs.erode_u8(grey, e))):
            t = windows(fn, args.reps)
            px = n * H * W
            say("  mge_morph_u8 50 x 50 ellipse (%d taps), %-22s %d x   %s   %.2f G tap reads/s over all pixels%s"
                % (taps, name + ",", n, us(t), px * taps / t[0] * 1e-9, "   (hole %.1f %% of the canvas)" % (100.0 * live / px) if "stroke" in name else ""))
    if args.kernels_only:
        return
    # edit() end to end against the by-hand step
    from michigan_amd.inference import tensor2im
    from michigan_amd.model import Pix2PixModel, default_options
    opt = default_options(gpu_ids=[0], isTrain=False, crop_size=H, load_size=H, compute_dtype="bf16", use_ig=True, use_stroke=True, inpaint_mode="stroke",
                          inpaint_orient=True, no_vgg_loss=True, no_flip=True)
    torch.manual_seed(0)
    model = Pix2PixModel(opt).cuda().eval()
    f = TM.session_files(size=H, seed=5)
    rec_points = [pen_walk(20, 1, 200, 312)[0], pen_walk(20, 2, 120, 392)[0], pen_walk(40, 3, 180, 332)[0]]
    rec_sizes = [pen_walk(20, 1, 200, 312)[1], pen_walk(20, 2, 120, 392)[1], pen_walk(40, 3, 180, 332)[1]]
    session = EditSession(model, opt, "cuda", rng=random.Random(1), generator=torch.Generator(device="cuda").manual_seed(1))
    session.open_tag(f["image"], f["label"], f["orient"], f["recon"])
    session.open_ref(f["ref_image"], f["ref_label"])
    # the host-made masks of the baseline, from the numpy contracts, before the clock
    mask = f["label"].numpy()[None]
    mask_m = MF.brush_contract(mask, pen_segments(rec_points[0], rec_sizes[0], 0) + pen_segments(rec_points[1], rec_sizes[1], 1))
    stroke = MF.brush_contract(mask_m, pen_segments(rec_points[2], rec_sizes[2], 2))
    stroke[stroke == 1] = 0
    stroke[stroke == 2] = 1
    hole = MF.morph_contract(stroke, e, (25, 25), MF.DILATE)
    erased = 1 in np.unique(mask - mask_m)
    host = {k: torch.from_numpy(v).pin_memory() for k, v in (("label_tag", mask_m), ("mask_stroke", stroke), ("mask_hole", hole))}
    pipe = inputs.DeviceInputPipeline(opt, "cuda", rng=random.Random(1), generator=torch.Generator(device="cuda").manual_seed(1))
    dev = {k: v.cuda() for k, v in f.items()}

    def baseline():
        up = {k: v.to("cuda", non_blocking=True) for k, v in host.items()}
        model.opt.inpaint_mode = "stroke"
        data = pipe.demo_batch(label_ref=dev["ref_label"], label_tag=up["label_tag"], mask_orient=dev["label"], orient_ref=dev["orient"],
                               image_ref=dev["ref_image"], image_tag=dev["recon"] if erased else dev["image"], mask_stroke=up["mask_stroke"],
                               mask_hole=up["mask_hole"])
        generated, picture = model(data, "demo_inference")
        return tensor2im(generated)[0], picture[0]

    def edit():
        return session.edit(rec_points, rec_sizes, False, False)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    for _ in range(3):
        baseline(), edit()
    # same seeds from here: the two must produce the same bytes
    for g in (pipe.generator, session.pipe.generator):
        g.manual_seed(11)
    (_, (rb, pb)), (_, (re_, pe)) = clock(baseline), clock(edit)
    assert torch.equal(rb, re_) and torch.equal(pb, pe), "edit() and the by-hand step disagree"
    assert session.used_recon == bool(erased)
    tb, te = [], []
    for _ in range(args.step_reps):                                        # alternating: what else the machine does falls on both
        tb.append(clock(baseline)[0])
        te.append(clock(edit)[0])
    mb, me = statistics.median(tb), statistics.median(te)
    say("  by hand: upload of three host-made 512^2 masks + demo_batch + model('demo_inference') + tensor2im, crop 512, bf16   %8.2f ms [%.2f, %.2f] over %d steps"
        % (mb * 1e3, min(tb) * 1e3, max(tb) * 1e3, len(tb)))
    say("  EditSession.edit(): 80 pen segments in 3 brush calls + 50 x 50 dilation + the read-back + the same                    %8.2f ms [%.2f, %.2f] over %d steps"
        % (me * 1e3, min(te) * 1e3, max(te) * 1e3, len(te)))
    spread = max(tb) - min(tb)
    say("  edit() - by hand = %+.3f ms; the baseline's own spread is %.3f ms: %s   (same bytes: result and orientation picture torch.equal)"
        % ((me - mb) * 1e3, spread * 1e3, "within it" if me - mb <= spread else "OUTSIDE it"))
    # what the clock above left out of the baseline: making the masks on a host without OpenCV (Pillow's line, scipy's dilation)
    try:
        from PIL import Image, ImageDraw
        from scipy import ndimage
    except ImportError:
        say("  host-made masks (Pillow + scipy): not measured, scipy is not installed")
    else:
        def host_masks():
            im = Image.fromarray(f["label"].numpy().copy())
            draw = ImageDraw.Draw(im)
            for c in range(3):
                for pt, size in zip(rec_points[c], rec_sizes[c]):
                    draw.line([tuple(pt["prev"]), tuple(pt["curr"])], fill=c, width=size)
            m = np.array(im)
            m[m == 1] = 0
            m[m == 2] = 1
            return ndimage.grey_dilation(m, footprint=e[::-1, ::-1].astype(bool), mode="constant", cval=0, origin=(-1, -1))
        th = []
        for _ in range(3):
            t0 = time.perf_counter()
            host_masks()
            th.append(time.perf_counter() - t0)
        say("  for scale, NOT part of the baseline above: one stroke mask and its hole made on the host with Pillow's ImageDraw.line and "
            "scipy.ndimage.grey_dilation   %8.2f ms [%.2f, %.2f] over 3 runs (other brush, same element)" % (statistics.median(th) * 1e3, min(th) * 1e3, max(th) * 1e3))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
