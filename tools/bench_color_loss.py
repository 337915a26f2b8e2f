"""The fused Lab / RGB / background loss, measured (GPU box):   python tools/bench_color_loss.py [--no-step]

(a) ops.color_losses forward + backward (3 launches) at 8 x 512^2, bf16 and fp32 image in the NHWC3 and NHWC8 layouts, against the same mathematics spelled
    in eager torch on the GPU in its fastest fair form (torch.where for the knee; NOT the reference's boolean-mask index assignments,
    each of which synchronises the host), both timed as a host clock around N calls ending in a device synchronise, alternating;
(b) the full bs 8 / 512^2 bf16 G+D step with no_lab_loss=False against the same trainer with it on True, interleaved in one
    process (A B A B ...), so that the difference can be read against the run-to-run spread of the step.
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


def eager_color_losses(fake, real, back):
    """(lab, rgb, background) of an NCHW image pair in eager torch, fp32 arithmetic."""
    m = torch.tensor([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]], device=fake.device)
    m = m / m.sum(dim=1, keepdim=True)

    def ab(x):
        xyz = torch.einsum("rc,nchw->nrhw", m, (x + 1) / 2)
        f = torch.where(xyz > KNEE, xyz.clamp_min(KNEE).pow(1.0 / 3.0), 7.787 * xyz + 0.137931)
        return torch.stack([500 * (f[:, 0] - f[:, 1]), 200 * (f[:, 1] - f[:, 2])], dim=1)
    fake = fake.float()
    lab = (ab(fake) - ab(real)).abs().mean()
    rgb = (fake - real).abs().mean()
    bk = back.unsqueeze(1)
    return lab, rgb, (fake * bk - real * bk).abs().mean()


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def bench_kernels():
    g = torch.Generator().manual_seed(5)
    real = (torch.rand(BS, 3, SIZE, SIZE, generator=g) * 2 - 1).cuda()
    sem = (torch.rand(BS, 1, SIZE, SIZE, generator=g) > 0.4).float()
    sem = torch.cat([sem, 1 - sem], dim=1).cuda()
    # C = 3 is what the generator's last convolution writes (the layout inside the training step), C = 8 the padded layout
    for dtype, ch in ((torch.bfloat16, 3), (torch.float32, 3), (torch.bfloat16, 8), (torch.float32, 8)):
        img = torch.zeros(BS, SIZE, SIZE, ch, dtype=dtype)
        img[..., :3] = (torch.rand(BS, SIZE, SIZE, 3, generator=g) * 2 - 1).to(dtype)
        img = img.cuda().requires_grad_(True)
        nchw = img.detach().permute(0, 3, 1, 2)[:, :3].requires_grad_(True)          # the view the eager spelling gets

        def fused():
            img.grad = None
            lab, rgb, back = ops.color_losses(img, real, sem[:, 0], 7)
            (lab + rgb + back).backward()

        def eager():
            nchw.grad = None
            lab, rgb, back = eager_color_losses(nchw, real, sem[:, 0])
            (lab + rgb + back).backward()
        for fn in (fused, eager):
            timed(fn, 5)
        with torch.no_grad():
            a = torch.stack(ops.color_losses(img.detach(), real, sem[:, 0], 7)).tolist()
            b = [float(v) for v in eager_color_losses(nchw.detach(), real, sem[:, 0])]
        tf, te = [], []
        for _ in range(5):                                                           # alternate: fused, eager, fused, ...
            tf.append(timed(fused, 50))
            te.append(timed(eager, 50))
        mb = BS * SIZE * SIZE * (2 * ch * img.element_size() + 3 * 4 + 4) * 1.5 / 1e6   # image read twice + written once, target and plane read twice
        print("color_losses fwd+bwd %s NHWC%d 8x512^2: fused %.1f us (min %.1f, max %.1f; ~%.0f MB moved) | eager torch %.1f us (min %.1f, max %.1f) | "
              "x%.1f | values fused %s eager %s" % (str(dtype).split(".")[1], ch, 1e6 * statistics.median(tf), 1e6 * min(tf), 1e6 * max(tf), mb,
                                                  1e6 * statistics.median(te), 1e6 * min(te), 1e6 * max(te), statistics.median(te) / statistics.median(tf),
                                                  ["%.5f" % v for v in a], ["%.5f" % v for v in b]), flush=True)


def bench_step():
    data = {k: v.cuda() for k, v in synth_batch(BS, SIZE, seed=1234).items()}
    trainers = {}
    for name, off in (("no_lab_loss=True", True), ("no_lab_loss=False", False)):
        torch.manual_seed(0)
        trainers[name] = Pix2PixTrainer(default_options(crop_size=SIZE, gpu_ids=[0], compute_dtype="bf16", no_lab_loss=off))

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
        print("G+D step bf16 bs%d %d^2, %s: %s ms/step (median %.2f)" % (BS, SIZE, name, ["%.2f" % (1e3 * t) for t in ts], 1e3 * statistics.median(ts)),
              flush=True)
    a, b = times["no_lab_loss=True"], times["no_lab_loss=False"]
    print("Lab term on - off: %+.2f ms/step (mean of %d interleaved pairs); spread of the step without it: %.2f ms (max - min); lab = %.4f"
          % (1e3 * (sum(b) - sum(a)) / len(a), len(a), 1e3 * (max(a) - min(a)), float(trainers["no_lab_loss=False"].get_latest_losses()["lab"].detach())), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this is a GPU measurement"
    bench_kernels()
    if "--no-step" not in sys.argv:
        bench_step()
