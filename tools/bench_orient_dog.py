"""The tail of the DoG orientation loss, measured (GPU box):   python tools/bench_orient_dog.py [out.txt]

ops.orient_loss_dog forward + backward (3 + 1 launches) at 8 x 512^2 with a 2-plane label and the hair plane of a one-hot, against two
baselines on the same GPU in the same process, alternating: (i) the same tail spelled as eager torch ops on the GPU (the expression of
networks.L1OLoss for the label shapes outside the fused condition, which is the reference's line by line), (ii) the Gabor tail
(ops.orient_loss, 2 + 1 launches).  Each is a host clock around N calls ending in a device synchronise.  The algorithmic bytes are
computed from the shapes: per pixel the maximum pass reads R and m (8), the partial pass R, idx, the label planes and m (9 + 4 planes),
the backward the same and writes 4.  GB/s = those bytes over the time of the whole call -- four launches and the autograd plumbing
included, so it is a rate of the call, not of a kernel; 36 MB of operands also fit the 256 MB last-level cache, so the HBM roof
(8.0 TB/s spec, about 6.3 TB/s achievable) bounds a cold pass, not necessarily this warm loop.
The condition is only that the fused tail is not slower than the eager composition; the script asserts it.  One line per measurement;
profiles/orient_dog.txt is this script's output plus the step times of bench.py."""
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import michigan_amd  # noqa: F401,E402
import torch  # noqa: E402
from michigan_amd import ops  # noqa: E402

BS, SIZE = 8, 512
HBM_SPEC, HBM_ACHIEVABLE = 8.0e12, 6.3e12


def eager_tail(conf_raw, idx, label, hair):
    hair = hair.unsqueeze(1)
    confidence = conf_raw.unsqueeze(1) * hair
    confidence = confidence / torch.max(confidence)
    confidence = confidence * (~(confidence <= 0)).float()
    ang = (idx.float() * (math.pi / 32)).unsqueeze(1)
    fake = torch.cat([torch.sin(2 * ang), torch.cos(2 * ang)], dim=1) * confidence
    orient = torch.nn.functional.l1_loss(fake * hair, label * hair)
    return orient, torch.sum(torch.abs(confidence * hair - hair)) / (torch.sum(hair) + 1e-5)


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def algorithmic_bytes(n_pix, label_ch):
    return n_pix * ((4 + 4) + (4 + 1 + 4 * label_ch + 4) + (4 + 1 + 4 * label_ch + 4) + 4)


def main(out_path=None):
    assert torch.cuda.is_available(), "this is a GPU measurement"
    g = torch.Generator().manual_seed(3)
    R = (torch.rand(BS, SIZE, SIZE, generator=g) * 6).cuda().requires_grad_(True)
    idx = torch.randint(0, 32, (BS, SIZE, SIZE), generator=g, dtype=torch.uint8).cuda()
    t = torch.rand(BS, SIZE, SIZE, generator=g) * math.pi
    label = torch.stack([torch.sin(2 * t), torch.cos(2 * t)], dim=1).cuda()
    m = (torch.rand(BS, SIZE, SIZE, generator=g) < 0.4).float()
    sem = torch.stack([1 - m, m], dim=1).cuda()
    hair = sem[:, 1]

    def run(tail):
        def fn():
            R.grad = None
            lo, lc = tail(R, idx, label, hair)
            (lo * 10 + lc * 100).backward()
        return fn
    fns = {"fused DoG tail": run(ops.orient_loss_dog), "eager DoG tail": run(eager_tail), "fused Gabor tail": run(ops.orient_loss)}
    vals = {}
    for name, fn in fns.items():
        timed(fn, 5)
        with torch.no_grad():
            tail = {"fused DoG tail": ops.orient_loss_dog, "eager DoG tail": eager_tail, "fused Gabor tail": ops.orient_loss}[name]
            vals[name] = ["%.6f" % float(v) for v in tail(R.detach(), idx, label, hair)]
        fn()
        vals[name].append("|dR| %.6e" % float(R.grad.abs().sum()))
    times = {k: [] for k in fns}
    for _ in range(5):                                                     # alternate the three
        for name, fn in fns.items():
            times[name].append(timed(fn, 100))
    nbytes = algorithmic_bytes(BS * SIZE * SIZE, 2)
    lines = []
    for name, ts in times.items():
        med = statistics.median(ts)
        line = "%s fwd+bwd fp32 %dx%d^2: %.1f us (min %.1f, max %.1f)" % (name, BS, SIZE, 1e6 * med, 1e6 * min(ts), 1e6 * max(ts))
        if name == "fused DoG tail":
            line += " | %.1f MB algorithmic -> %.0f GB/s of the whole call = %.1f %% of the 8.0 TB/s HBM spec, %.1f %% of the 6.3 TB/s achievable" % (
                nbytes / 1e6, nbytes / med / 1e9, 100 * nbytes / med / HBM_SPEC, 100 * nbytes / med / HBM_ACHIEVABLE)
        lines.append(line + " | values " + " ".join(vals[name]))
    fused, eager, gabor = (statistics.median(times[k]) for k in fns)
    lines.append("eager / fused DoG x%.1f; fused DoG / fused Gabor x%.2f" % (eager / fused, fused / gabor))
    text = "\n".join(lines)
    print(text, flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text + "\n")
    assert fused <= eager, "the fused tail is slower than the eager composition"


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
