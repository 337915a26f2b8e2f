"""The balanced colour pass against the plain one, measured (GPU box):   python tools/bench_lab_balance.py [out.txt] [--no-step] [--kernels-only N]

(a) ops.color_losses with and without a weight table (mgc_color_loss_balanced_* against mg_color_loss_*), flags lab | rgb | background,
    at 8 x 512^2 with a bf16 and an fp32 NHWC8 image, forward alone (two launches, under no_grad) and forward + backward (three
    launches), both in one process, alternating, each a host clock around N calls ending in a device synchronise.  The comparison is the
    plain pass of the same run; no target was set in advance.
    The algorithmic bytes are computed from the shapes.  Per pixel the plain forward reads the image (8 channels of its dtype), the target
    (12) and the background plane (4); the backward reads the same and writes the image gradient.  The balanced pass adds the hair plane
    (4 B) and one gather from the table (4 B) to each.  GB/s = those bytes over the time of the whole CALL -- launches and the autograd
    plumbing included -- so it is a rate of the call, not of a kernel; the kernels' own times come from a kernel trace of this script run
    with --kernels-only (profiles/lab_balance.txt carries both).  The operands (up to 126 MB) fit the 256 MB last-level cache, so the HBM
    roof (8.0 TB/s spec, about 6.3 TB/s achievable) bounds a cold pass, not necessarily this warm loop.
(b) the full bs 8 / 512^2 bf16 G+D step with no_lab_loss=False, with and without balance_Lab, interleaved in one process.
The table comes from a seeded synthetic histogram shaped like the shipped one (a peak around grey), so that the tool needs no data file;
the target is a grey base plus chroma noise, the input under which neighbouring pixels share bins as hair pixels do.
"""
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import michigan_amd  # noqa: F401,E402
import numpy as np  # noqa: E402
import torch  # noqa: E402
from michigan_amd import ops  # noqa: E402

BS, SIZE, CH = 8, 512, 8
HBM_SPEC, HBM_ACHIEVABLE = 8.0e12, 6.3e12


def synthetic_counts(seed=7):
    """float64 [256, 256]: a histogram with the shape of the reference's (a sharp peak at grey, nothing far from it)"""
    rng = np.random.default_rng(seed)
    a, b = np.meshgrid(np.arange(256) - 128.0, np.arange(256) - 128.0, indexing="ij")
    dens = 3e6 * np.exp(-0.5 * ((a - 3) ** 2 / 8.0 ** 2 + (b - 8) ** 2 / 12.0 ** 2))
    return np.floor(dens * rng.uniform(0.7, 1.3, size=dens.shape))


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def call_bytes(esize, balanced, backward):
    per_pixel = CH * esize + 12 + 4 + (8 if balanced else 0)
    fwd = BS * SIZE * SIZE * per_pixel
    return fwd + (fwd + BS * SIZE * SIZE * CH * esize if backward else 0)


def operands(dtype):
    g = torch.Generator().manual_seed(5)
    grey = torch.rand(BS, 1, SIZE, SIZE, generator=g) * 1.4 - 0.7
    real = (grey + 0.08 * torch.randn(BS, 3, SIZE, SIZE, generator=g)).clamp(-1, 1).cuda()
    hair = (torch.rand(BS, 1, SIZE, SIZE, generator=g) > 0.4).float()
    sem = torch.cat([1 - hair, hair], dim=1).cuda()
    img = torch.zeros(BS, SIZE, SIZE, CH, dtype=dtype)
    img[..., :3] = (real.cpu().permute(0, 2, 3, 1) + 0.15 * torch.randn(BS, SIZE, SIZE, 3, generator=g)).clamp(-1, 1).to(dtype)
    return img.cuda().requires_grad_(True), real, sem


def passes(img, real, sem, table):
    kw = dict(hair=sem[:, 1], table=table)

    def fwd(extra):
        def fn():
            with torch.no_grad():
                ops.color_losses(img, real, sem[:, 0], 7, **extra)
        return fn

    def both(extra):
        def fn():
            img.grad = None
            lab, rgb, back = ops.color_losses(img, real, sem[:, 0], 7, **extra)
            (lab + rgb + back).backward()
        return fn
    return {("plain", "fwd"): fwd({}), ("balanced", "fwd"): fwd(kw), ("plain", "fwd+bwd"): both({}), ("balanced", "fwd+bwd"): both(kw)}


def bench_kernels(lines, reps=5, n=200):
    table = ops.lab_weight_table(synthetic_counts(), 10.0, device="cuda")
    for dtype in (torch.bfloat16, torch.float32):
        img, real, sem = operands(dtype)
        fns = passes(img, real, sem, table)
        for fn in fns.values():
            timed(fn, 10)
        with torch.no_grad():
            vals = {"plain": torch.stack(ops.color_losses(img, real, sem[:, 0], 7)).tolist(),
                    "balanced": torch.stack(ops.color_losses(img, real, sem[:, 0], 7, hair=sem[:, 1], table=table)).tolist()}
        times = {k: [] for k in fns}
        for _ in range(reps):                                                # alternate the four
            for k, fn in fns.items():
                times[k].append(timed(fn, n))
        name = str(dtype).split(".")[1]
        for what in ("fwd", "fwd+bwd"):
            med = {}
            for kind in ("plain", "balanced"):
                ts = times[(kind, what)]
                med[kind] = statistics.median(ts)
                nb = call_bytes(img.element_size(), kind == "balanced", what == "fwd+bwd")
                lines.append("color_losses %-8s %-7s %s NHWC%d %dx%d^2: %.1f us per call (min %.1f, max %.1f) | %.1f MB algorithmic -> %.0f GB/s of the whole "
                             "call = %.1f %% of the 6.3 TB/s achievable | values %s"
                             % (kind, what, name, CH, BS, SIZE, 1e6 * med[kind], 1e6 * min(ts), 1e6 * max(ts), nb / 1e6, nb / med[kind] / 1e9,
                                100 * nb / med[kind] / HBM_ACHIEVABLE, ["%.5f" % v for v in vals[kind]]))
                print(lines[-1], flush=True)
            extra = call_bytes(img.element_size(), True, what == "fwd+bwd") / call_bytes(img.element_size(), False, what == "fwd+bwd")
            lines.append("  balanced / plain %s %s: x%.3f by wall time; x%.3f by algorithmic bytes" % (what, name, med["balanced"] / med["plain"], extra))
            print(lines[-1], flush=True)


def kernels_only(n):
    """for a kernel trace: n calls of each pass, nothing timed"""
    table = ops.lab_weight_table(synthetic_counts(), 10.0, device="cuda")
    for dtype in (torch.bfloat16, torch.float32):
        img, real, sem = operands(dtype)
        for fn in passes(img, real, sem, table).values():
            for _ in range(n):
                fn()
    torch.cuda.synchronize()


def bench_step(lines):
    from michigan_amd.model import Pix2PixTrainer, default_options
    from michigan_amd.synth import synth_batch
    data = {k: v.cuda() for k, v in synth_batch(BS, SIZE, seed=1234).items()}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "ab_count.npy")
        np.save(path, synthetic_counts())
        trainers = {}
        for name, on in (("balance_Lab off", False), ("balance_Lab on", True)):
            torch.manual_seed(0)
            trainers[name] = Pix2PixTrainer(default_options(crop_size=SIZE, gpu_ids=[0], compute_dtype="bf16", no_lab_loss=False, balance_Lab=on,
                                                            weight_dir=path if on else None))

    def step(tr):
        tr.run_generator_one_step(data)
        tr.run_discriminator_one_step(data)
    for tr in trainers.values():
        for _ in range(3):
            step(tr)
    times = {k: [] for k in trainers}
    for rep in range(4):
        for name, tr in trainers.items():
            step(tr)
            times[name].append(timed(lambda: step(tr), 6))
    for name, ts in times.items():
        lines.append("G+D step bf16 bs%d %d^2, Lab term on, %s: %s ms/step (median %.2f) | lab = %.4f"
                     % (BS, SIZE, name, ["%.2f" % (1e3 * t) for t in ts], 1e3 * statistics.median(ts), float(trainers[name].get_latest_losses()["lab"].detach())))
        print(lines[-1], flush=True)
    a, b = times["balance_Lab off"], times["balance_Lab on"]
    lines.append("balance_Lab on - off: %+.2f ms/step (mean of %d interleaved pairs); spread of the step without it: %.2f ms (max - min)"
                 % (1e3 * (sum(b) - sum(a)) / len(a), len(a), 1e3 * (max(a) - min(a))))
    print(lines[-1], flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this is a GPU measurement"
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--kernels-only" in sys.argv:
        kernels_only(int(sys.argv[sys.argv.index("--kernels-only") + 1]))
        sys.exit(0)
    lines = []
    bench_kernels(lines)
    if "--no-step" not in sys.argv:
        bench_step(lines)
    if args:
        with open(args[0], "w") as fh:
            fh.write("\n".join(lines) + "\n")
