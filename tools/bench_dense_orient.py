"""Dense orientation extraction, measured (GPU box):   python tools/bench_dense_orient.py [--reps 100] [--cpu-reps 2] [--out FILE]

The two launches of inputs.dense_orientation at 8 x 512 x 512 (seeded strand images of tests/dense_orient_fixtures.py under an
elliptical mask, fp32 NHWC on the device):
  * mg_gabor_argmax_fwd under ops.dog_bank and mg_orient_smooth, each alone and the pair back to back, through the operator layer on
    prepared tensors; device events around `--reps` calls after a warm-up, five windows, median and spread.  A time per CALL, launch
    gap included, not a kernel time.
  * what the shapes say the smoothing pass must move: 7 bytes a pixel of device memory (conf 4, idx 1, mask 1 read, one byte
    written), and per 32 x 32 tile the LDS wave-instructions and FMAs counted from the kernel's loops; printed beside the time.
The comparison line is the same batch through the reference pipeline restated on the CPU (cal_orientation.py:60-110 as torch +
scipy: 32 conv2d calls, cat, arg-max, two gaussian_filter calls per image standing in for cv2.GaussianBlur), timed in the same
script with a host clock.  The kernel is never compared against itself.  profiles/dense_orient.txt is this script's output.
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

N, H, W = 8, 512, 512


def reference_pipeline(image, mask, bank):
    """cal_orientation.py:60-110 for a batch on the CPU: image fp32 [N,3,H,W] in [-1, 1], mask [N,H,W] in {0, 1} -> uint8 [N,H,W]"""
    from scipy.ndimage import gaussian_filter
    fake = (image + 1) / 2.0 * 255
    gray = (0.299 * fake[:, 0] + 0.587 * fake[:, 1] + 0.144 * fake[:, 2]).unsqueeze(1)
    res = torch.cat([F.conv2d(gray, bank[k].view(1, 1, 17, 17), padding=8).clone() for k in range(32)], dim=1)
    res[res < 0] = 0
    idx, conf = torch.argmax(res, dim=1).float(), torch.max(res, dim=1)[0]
    ang = idx * math.pi / 31 * 2
    m = mask.float()
    out = []
    for i in range(image.shape[0]):
        fx = torch.from_numpy(gaussian_filter((torch.cos(ang[i]) * conf[i] * m[i]).numpy(), sigma=4, mode="mirror", truncate=4.0))
        fy = torch.from_numpy(gaussian_filter((torch.sin(ang[i]) * conf[i] * m[i]).numpy(), sigma=4, mode="mirror", truncate=4.0))
        th = torch.atan2(fy, fx) * 0.5
        th[th < 0] += math.pi
        out.append(np.uint8(th.numpy() * 255. / math.pi * mask[i].numpy()))
    return np.stack(out)


def timed(fn, reps):
    """Seconds per call: device events around `reps` calls."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--cpu-reps", type=int, default=2)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    assert args.reps >= 50
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    import dense_orient_fixtures as DE
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    image_u8, mask = DE.strand_image(N, H, W, 512)
    image = DE.image_fp32(image_u8)                                        # fp32 NHWC
    dimage, dmask = image.cuda(), mask.cuda()
    bank = ops.dog_bank("cuda")
    conf, idx = ops.gabor_argmax(dimage, bank)
    say("dense orientation extraction, %d x %d x %d fp32, %s, %d calls per window, 5 windows (median [min, max])"
        % (N, H, W, torch.cuda.get_device_name(0), args.reps))
    pix = N * H * W
    with torch.no_grad():
        g = windows(lambda: ops.gabor_argmax(dimage, bank), args.reps)
        s = windows(lambda: ops.orient_smooth(conf, idx, dmask), args.reps)
        sa = windows(lambda: ops.orient_smooth(conf, idx, dmask, want_angle=True), args.reps)
        both = windows(lambda: inputs.dense_orientation(dimage, dmask), args.reps)
    us = lambda t: "%8.1f us [%7.1f, %7.1f]" % (t[0] * 1e6, t[1] * 1e6, t[2] * 1e6)
    say("  mg_gabor_argmax_fwd (DoG bank)        %s   %.1f TFLOP/s of the 32 x 289 x 2 fp32 contraction" % (us(g), pix * 32 * 289 * 2 / g[0] * 1e-12))
    tiles = N * -(-H // DE.TILE_H) * -(-W // DE.TILE_W)
    say("  mg_orient_smooth                      %s   %.0f GB/s of the 7 B/pixel it must move (%.1f MB); %d tiles, %.2f us per tile per CU at 256 CUs"
        % (us(s), pix * 7 / s[0] * 1e-9, pix * 7e-6, tiles, s[0] * 1e6 / (tiles / 256.0)))
    say("  mg_orient_smooth + fp32 angle         %s" % us(sa))
    say("  inputs.dense_orientation (both, + mask threshold and its host read)  %s" % us(both))
    # per tile, from the kernel's loops (michigan_amd/csrc/mg_orient_smooth.hip): 256 threads = 4 waves
    lds_wi = 2 * (64 * 64 // 64) + 4 * 40 + 4 * 8 + 4 * 36
    fma = (64 * 32 + 32 * 32) * 33 * 2
    say("  per tile: %d LDS wave-instructions (64 b64 table gathers and 64 b64 stores of the flow, 160 b64 loads + 32 b64 stores in the row pass, 144 b64 loads in the "
        "column pass), %d FMAs = %d wave-instructions, 1024 atan2f; %d bytes of LDS, 3 workgroups a CU" % (lds_wi, fma, fma // 64, 64 * 65 * 8 + 64 * 33 * 8 + 32 * 8))
    # the same batch through the restated reference on the CPU
    cimage, cbank = image.permute(0, 3, 1, 2).contiguous(), ops.dog_bank()
    want = reference_pipeline(cimage, mask, cbank)
    t = []
    for _ in range(args.cpu_reps):
        t0 = time.perf_counter()
        reference_pipeline(cimage, mask, cbank)
        t.append(time.perf_counter() - t0)
    cpu = statistics.median(t)
    say("  reference pipeline on the CPU (torch %d threads + scipy), same batch   %8.1f ms [%.1f, %.1f] over %d runs  = %.0f x the two launches"
        % (torch.get_num_threads(), cpu * 1e3, min(t) * 1e3, max(t) * 1e3, len(t), cpu / (g[0] + s[0])))
    got = inputs.dense_orientation(dimage, dmask).cpu().numpy()
    m = mask.numpy() != 0
    d = np.abs(got[m].astype(np.int32) - want[m].astype(np.int32))
    d = np.minimum(d, 255 - d)
    say("  same results: in-mask bytes equal %.4f %%, within one level %.4f %%, outside the mask %d non-zero bytes"
        % (100 * (d == 0).mean(), 100 * (d <= 1).mean(), int((got[~m] != 0).sum())))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
