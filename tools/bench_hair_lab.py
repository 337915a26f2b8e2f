"""The fused hair-average Lab / background loss of the unpaired stage, measured (GPU box):   python tools/bench_hair_lab.py [--no-step]

(a) ops.hair_lab_losses forward + backward (3 launches) at 8 x 512^2, bf16 and fp32 image in the NHWC3 layout the generator writes and in
    NHWC8, masks = the ellipses of synth_batch(unpaired=True), against the same mathematics spelled in eager torch on the GPU (torch.where
    for the knee, sums over dim (2, 3); NOT the reference's boolean-mask index assignments, each of which synchronises the host), both
    timed as a host clock around N calls ending in a device synchronise, alternating.  The algorithmic bytes are computed from the shapes
    and the mask fractions (what the kernels must touch: a pixel whose mask is 0 is not read), and GB/s = those bytes over the time of
    the whole call -- three launches and the autograd plumbing included, so it is a rate of the call, not of a kernel;
(b) the bs 8 / 512^2 bf16 G+D step of the unpaired stage (unpairTrain, curr_step = 2), and in the same process the default step
    (curr_step = 1, unpairTrain off) from two trainer instances interleaved (A B U A B U ...): A against B is the spread of the
    default step on identical code, against which a comparison of the default step with the parent commit (bench.py) is read.
One line per measurement; the lines kept under profiles/ are this script's output.
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import michigan_amd  # noqa: F401,E402
import torch  # noqa: E402
from michigan_amd import ops  # noqa: E402
from michigan_amd.model import Pix2PixTrainer, default_options  # noqa: E402
from michigan_amd.synth import synth_batch  # noqa: E402

BS, SIZE = 8, 512
KNEE = 0.008856


def eager_hair_lab_losses(fake, ref, m_f, m_r, tgt, m_b):
    """(hairAvgLab, background) of NCHW images and [N, 1, H, W] masks in eager torch, fp32 arithmetic."""
    m = torch.tensor([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]], device=fake.device)
    m = m / m.sum(dim=1, keepdim=True)

    def mean_ab(x, mask):
        xyz = torch.einsum("rc,nchw->nrhw", m, (x + 1) / 2)
        f = torch.where(xyz > KNEE, xyz.clamp_min(KNEE).pow(1.0 / 3.0), 7.787 * xyz + 0.137931)
        ab = torch.stack([500 * (f[:, 0] - f[:, 1]), 200 * (f[:, 1] - f[:, 2])], dim=1)
        s = mask.sum(dim=(2, 3))
        return (ab * mask).sum(dim=(2, 3)) / torch.where(s == 0, torch.ones_like(s), s)
    fake = fake.float()
    hair = (mean_ab(fake, m_f) - mean_ab(ref, m_r)).abs().mean()
    return hair, (fake * m_b - tgt * m_b).abs().mean()


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def algorithmic_bytes(n_pix, ch, esize, frac_f, frac_r, frac_b):
    """Bytes the three launches must touch.  A pixel's RGB costs one 4-element access when the pixel is quad-aligned, else three scalars."""
    rgb = (4 if ch % 4 == 0 else 3) * esize
    touched = min(1.0, frac_f + frac_b)                    # one-hot label: every pixel is hair or background
    fwd = n_pix * (3 * 4 + rgb * touched + 12 * frac_r + 12 * frac_b)          # three mask planes, img, ref where m_r, tgt where m_b
    bwd = n_pix * (2 * 4 + rgb * touched + 12 * frac_b + ch * esize)          # two mask planes, img, tgt where m_b, dimg written whole
    return fwd + bwd


def bench_kernels():
    b = synth_batch(BS, SIZE, seed=1234, unpaired=True)
    ref, tgt = b["image_ref"].cuda(), b["image_tag"].cuda()
    sem_tag, sem_ref = b["input_tag"].cuda(), b["input_ref"].cuda()
    frac_f, frac_r = float(sem_tag[:, 1].mean()), float(sem_ref[:, 1].mean())
    g = torch.Generator().manual_seed(5)
    print("masks of synth_batch(%d, %d, unpaired=True): tag hair fraction %.3f, reference hair fraction %.3f" % (BS, SIZE, frac_f, frac_r), flush=True)
    # C = 3 is what the generator's last convolution writes (the layout inside the training step), C = 8 the padded layout
    for dtype, ch in ((torch.bfloat16, 3), (torch.float32, 3), (torch.bfloat16, 8), (torch.float32, 8)):
        img = torch.zeros(BS, SIZE, SIZE, ch, dtype=dtype)
        img[..., :3] = (torch.rand(BS, SIZE, SIZE, 3, generator=g) * 2 - 1).to(dtype)
        img = img.cuda().requires_grad_(True)
        nchw = img.detach().permute(0, 3, 1, 2)[:, :3].requires_grad_(True)          # the view the eager spelling gets

        def fused():
            img.grad = None
            hair, back = ops.hair_lab_losses(img, ref, sem_tag[:, 1], sem_ref[:, 1], tgt, sem_tag[:, 0], 3)
            (hair + back).backward()

        def eager():
            nchw.grad = None
            hair, back = eager_hair_lab_losses(nchw, ref, sem_tag[:, 1:2], sem_ref[:, 1:2], tgt, sem_tag[:, 0:1])
            (hair + back).backward()
        for fn in (fused, eager):
            timed(fn, 5)
        with torch.no_grad():
            a = torch.stack(ops.hair_lab_losses(img.detach(), ref, sem_tag[:, 1], sem_ref[:, 1], tgt, sem_tag[:, 0], 3)).tolist()
            e = [float(v) for v in eager_hair_lab_losses(nchw.detach(), ref, sem_tag[:, 1:2], sem_ref[:, 1:2], tgt, sem_tag[:, 0:1])]
        tf, te = [], []
        for _ in range(5):                                                           # alternate: fused, eager, fused, ...
            tf.append(timed(fused, 50))
            te.append(timed(eager, 50))
        nbytes = algorithmic_bytes(BS * SIZE * SIZE, ch, img.element_size(), frac_f, frac_r, 1 - frac_f)
        med = statistics.median(tf)
        print("hair_lab_losses fwd+bwd %s NHWC%d 8x512^2: fused %.1f us (min %.1f, max %.1f; %.0f MB algorithmic -> %.0f GB/s of the whole call) | "
              "eager torch %.1f us (min %.1f, max %.1f) | x%.1f | values fused %s eager %s"
              % (str(dtype).split(".")[1], ch, 1e6 * med, 1e6 * min(tf), 1e6 * max(tf), nbytes / 1e6, nbytes / med / 1e9,
                 1e6 * statistics.median(te), 1e6 * min(te), 1e6 * max(te), statistics.median(te) / med,
                 ["%.5f" % v for v in a], ["%.5f" % v for v in e]), flush=True)


def bench_step():
    paired = {k: v.cuda() for k, v in synth_batch(BS, SIZE, seed=1234).items()}
    unpaired = {k: v.cuda() for k, v in synth_batch(BS, SIZE, seed=1234, unpaired=True).items()}
    trainers = {}
    for name, over, data in (("default (a)", {}, paired), ("default (b)", {}, paired), ("unpairTrain curr_step=2", dict(unpairTrain=True, curr_step=2), unpaired)):
        torch.manual_seed(0)
        trainers[name] = (Pix2PixTrainer(default_options(crop_size=SIZE, gpu_ids=[0], compute_dtype="bf16", **over)), data)

    def step(name):
        tr, data = trainers[name]
        tr.run_generator_one_step(data)
        tr.run_discriminator_one_step(data)
    for name in trainers:
        for _ in range(3):
            step(name)
    times = {k: [] for k in trainers}
    for rep in range(4):
        for name in trainers:
            step(name)
            times[name].append(timed(lambda: step(name), 6))
    for name, ts in times.items():
        print("G+D step bf16 bs%d %d^2, %s: %s ms/step (median %.2f)" % (BS, SIZE, name, ["%.2f" % (1e3 * t) for t in ts], 1e3 * statistics.median(ts)),
              flush=True)
    a, b = times["default (a)"], times["default (b)"]
    losses = {k: round(float(v.detach().float().mean()), 4) for k, v in trainers["unpairTrain curr_step=2"][0].get_latest_losses().items()}
    print("default step, two instances of identical code: (b) - (a) %+.2f ms/step (mean of %d interleaved pairs), spread max - min %.2f ms over both; "
          "unpaired step losses %s" % (1e3 * (sum(b) - sum(a)) / len(a), len(a), 1e3 * (max(a + b) - min(a + b)), losses), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this is a GPU measurement"
    bench_kernels()
    if "--no-step" not in sys.argv:
        bench_step()
