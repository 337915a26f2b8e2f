"""The evaluation pass, measured (GPU box):   python tools/bench_quality.py [--reps 200] [--step-reps 10] [--out FILE]

  * ops.image_quality_u8 (mgq_image_quality_u8: the tile launch and the join) with a hair mask and ops.orient_distance_u8
    (mgq_orient_distance_u8: a memset node and a launch) at 1 x 512^2 x 3 and 8 x 512^2 x 3.  Device events around `--reps` calls after a
    warm-up, five windows, median and spread: a time per CALL, launch gaps and the wrapper's three allocations included, not a kernel
    time.  Beside it the bytes the call has to move (2 N H W C + N H W for the image pass, 3 N H W for the orientation pass) and the
    share of the HBM roof (8 TB/s) that time amounts to.
  * The same SSIM as an eager torch float64 composition on the same GPU, written here: five grouped conv2d pairs (x then y) over
    float64 [N,C,H,W] tensors, the map, the two sums.  Alternated with the fused call window by window in the same process; its sums
    are held to the fused ones at 1e-9 per counted pixel before anything is timed.
  * What `evaluate` costs per sample beside the generator's forward, crop 512, bf16, random weights, batch 4: host clock around a
    synchronised call of model(data, 'inference') and of evaluate.measure_batch (tensor2im, the orientation pass, the two measurement
    passes, the per-sample Lab distance, the one read-back) on the same batch, alternated.
`--rehearse` runs the whole script at a toy size on the CPU against the contract emulator (a plumbing check: its times mean nothing).
profiles/quality_metrics.txt is this script's output.
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
import torch.nn.functional as F  # noqa: E402
from michigan_amd import metrics, ops  # noqa: E402

HBM_PEAK = 8.0e12                                                        # bytes / s


def eager_ssim_sums(a, b, mask, win):
    """[N,C] ssim_sum and ssim_sum under the mask, in eager torch float64: what the fused pass replaces"""
    c, k = a.shape[3], win.numel()
    r = k // 2
    x, y = a.permute(0, 3, 1, 2).double(), b.permute(0, 3, 1, 2).double()
    kx, ky = win.view(1, 1, 1, k).repeat(c, 1, 1, 1), win.view(1, 1, k, 1).repeat(c, 1, 1, 1)
    blur = lambda z: F.conv2d(F.conv2d(z, kx, groups=c), ky, groups=c)
    mu_a, mu_b, e_aa, e_bb, e_ab = blur(x), blur(y), blur(x * x), blur(y * y), blur(x * y)
    var_a, var_b, cov = e_aa - mu_a * mu_a, e_bb - mu_b * mu_b, e_ab - mu_a * mu_b
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    smap = ((2 * mu_a * mu_b + c1) * (2 * cov + c2)) / ((mu_a * mu_a + mu_b * mu_b + c1) * (var_a + var_b + c2))
    centre = (mask[:, r:mask.shape[1] - r, r:mask.shape[2] - r] != 0).unsqueeze(1)
    return smap.sum((2, 3)), (smap * centre).sum((2, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--step-reps", type=int, default=10)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--rehearse", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    dev = "cpu" if args.rehearse else "cuda"
    if args.rehearse:
        import quality_fixtures as QF
        from michigan_amd import _cabi
        _cabi.set_backend(QF.QualityEmulator())
        size, batches, reps, step_reps, crop = 32, (1, 2), 2, 1, 64
    else:
        assert torch.cuda.is_available(), "this measurement needs the GPU"
        assert args.reps >= 50
        size, batches, reps, step_reps, crop = 512, (1, 8), args.reps, args.step_reps, 512
    sync = (lambda: None) if args.rehearse else torch.cuda.synchronize
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn, n):
        if args.rehearse:
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            return (time.perf_counter() - t0) / n
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        sync()
        a.record()
        for _ in range(n):
            fn()
        b.record()
        sync()
        return a.elapsed_time(b) * 1e-3 / n

    def alternated(fns, n_each, nwin=5):
        """five windows of each function, window by window in turn -> [(median, min, max)]"""
        for fn in fns:
            for _ in range(3):
                fn()
        t = [[] for _ in fns]
        for _ in range(nwin):
            for i, (fn, n) in enumerate(zip(fns, n_each)):
                t[i].append(timed(fn, n))
        return [(statistics.median(v), min(v), max(v)) for v in t]

    us = lambda t: "%9.1f us [%8.1f, %8.1f]" % (t[0] * 1e6, t[1] * 1e6, t[2] * 1e6)
    say("%sevaluation pass, %d x %d images, %s, %d calls per window (eager: %d), 5 alternated windows (median [min, max])"
        % ("REHEARSAL ON THE CPU, times mean nothing: " if args.rehearse else "", size, size, "cpu" if args.rehearse else torch.cuda.get_device_name(0), reps, max(reps // 10, 1)))
    win = metrics.gaussian_window()
    twin = torch.from_numpy(win).to(dev)
    g = torch.Generator().manual_seed(3)
    speedups = []
    for n in batches:
        a = torch.randint(0, 256, (n, size, size, 3), generator=g, dtype=torch.uint8).to(dev)
        noise = torch.randint(-8, 9, (n, size, size, 3), generator=g)
        b = torch.clamp(a.cpu().long() + noise, 0, 255).to(torch.uint8).to(dev)
        mask = (torch.rand((n, size, size), generator=g) < 0.3).to(torch.uint8).to(dev)
        oa = torch.randint(0, 256, (n, size, size), generator=g, dtype=torch.uint8).to(dev)
        ob = torch.randint(0, 256, (n, size, size), generator=g, dtype=torch.uint8).to(dev)
        fused = lambda: ops.image_quality_u8(a, b, mask, win)
        orient = lambda: ops.orient_distance_u8(oa, ob, mask)
        fns, counts = [fused, orient], [reps, reps]
        eager_note = None
        if not args.kernels_only:
            try:
                es, em = eager_ssim_sums(a, b, mask, twin)
                oi, os_ = fused()
                valid = (size - 10) ** 2
                err = max(float((es - os_[:, :, 0]).abs().max()) / valid, float(((em - os_[:, :, 1]).abs() / oi[:, :, 3].clamp(min=1)).max()))
                assert err <= 1e-9, "the eager composition and the fused pass disagree: %.3e per counted pixel" % err
                fns.append(lambda: eager_ssim_sums(a, b, mask, twin))
                counts.append(max(reps // 10, 1))
            except (RuntimeError, NotImplementedError) as e:                   # e.g. no float64 convolution on this build
                eager_note = "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:120])
        t = alternated(fns, counts)
        q_bytes, o_bytes = 2 * n * size * size * 3 + n * size * size, 3 * n * size * size
        say("  ops.image_quality_u8 (2 launches), k = 11, mask, %d x %d^2 x 3   %s   %.2f MB to move: %.1f %% of the HBM roof"
            % (n, size, us(t[0]), q_bytes * 1e-6, 100.0 * q_bytes / HBM_PEAK / t[0][0]))
        say("  ops.orient_distance_u8 (memset + 1 launch),       %d x %d^2       %s   %.2f MB to move: %.1f %% of the HBM roof"
            % (n, size, us(t[1]), o_bytes * 1e-6, 100.0 * o_bytes / HBM_PEAK / t[1][0]))
        if len(t) > 2:
            say("  the same SSIM sums in eager torch float64 (10 grouped conv2d), %d x %d^2 x 3   %s   fused is %.1f x faster (medians; agreement %.1e per counted pixel)"
                % (n, size, us(t[2]), t[2][0] / t[0][0], err))
            speedups.append(t[2][0] / t[0][0])
        elif eager_note:
            say("  the same SSIM sums in eager torch float64: not measured (%s)" % eager_note)
    if args.kernels_only:
        return
    # evaluate per sample beside the generator's forward
    import dataset_fixtures as DF
    import tempfile
    from michigan_amd import evaluate, inference
    from michigan_amd.model import Pix2PixModel, default_options
    bs = 2 if args.rehearse else 4
    over = dict(ngf=8, compute_dtype="fp32", gpu_ids=[]) if args.rehearse else dict(compute_dtype="bf16", gpu_ids=[0])
    opt = default_options(isTrain=False, crop_size=crop, load_size=crop, no_vgg_loss=True, no_flip=True, use_ig=False, **over)
    with tempfile.TemporaryDirectory() as root:
        opt.data_dir, opt.subset, opt.batchSize = root, "val", bs
        stems = ["s%d" % i for i in range(bs)]
        for i, stem in enumerate(stems):
            label, orient_map, image = DF.sample(40 + i, crop)
            DF.save(os.path.join(root, "val_labels", stem + ".png"), label)
            DF.save(os.path.join(root, "val_dense_orients", stem + "_orient_dense.png"), orient_map)
            DF.save(os.path.join(root, "val_images", stem + ".jpg"), image)
        torch.manual_seed(0)
        model = Pix2PixModel(opt).to(dev).eval()
        names = [(s, s, s) for s in stems]
        gen = torch.Generator(device=dev).manual_seed(1)
        (data, generated), = list(inference.generated_batches(opt, model, names, rng=random.Random(1), generator=gen, given_orientation=True))

    def clock(fn):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return time.perf_counter() - t0

    forward = lambda: model(data, "inference")
    measure = lambda: evaluate.measure_batch(opt, data, generated, "reconstruct")
    for _ in range(2):
        forward(), measure()
    tf, tm = [], []
    for _ in range(step_reps):
        tf.append(clock(forward))
        tm.append(clock(measure))
    mf, mm = statistics.median(tf), statistics.median(tm)
    say("  generator forward, model(data, 'inference'), crop %d, %s, batch %d          %8.2f ms [%.2f, %.2f] over %d steps = %.2f ms a sample"
        % (crop, over["compute_dtype"], bs, mf * 1e3, min(tf) * 1e3, max(tf) * 1e3, len(tf), mf * 1e3 / bs))
    say("  evaluate.measure_batch (tensor2im, orientation pass, both measurement passes, Lab, read-back), same batch   %8.2f ms [%.2f, %.2f] over %d steps = %.2f ms a sample: %.0f %% on top of the forward"
        % (mm * 1e3, min(tm) * 1e3, max(tm) * 1e3, len(tm), mm * 1e3 / bs, 100.0 * mm / mf))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
