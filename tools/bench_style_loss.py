"""The fused style / content feature-moment kernels, measured (GPU box):   python tools/bench_style_loss.py [--masked] [--no-step]

(a) per VGG tap shape at bs 8 / 512^2 in bf16 -- [8,512^2,64], [8,256^2,128], [8,128^2,256], [8,64^2,512], [8,32^2,512]; style at
    every tap, content at the last one, as the model calls it -- the time of
      * mg_feat_moment_loss_fwd (two launches) and mg_feat_moment_loss_bwd (one launch), called through the C ABI on prepared buffers,
      * the reference's torch-op formulation (calc_mean_std / calc_style_loss / calc_content_loss of loss.py:624-694, or their
        remove_background forms with --masked) on the SAME GPU tensors: forward under autograd, and forward + backward (the backward
        is the difference) -- what a user runs today,
    both arms in one process, alternating, device events around batches of calls.  GB/s = algorithmic bytes (each feature map the
    term needs read once forward; read once and dx written once backward; masks at 4 bytes a pixel) over that time: a rate of the
    call, launch gaps included, not of a kernel.
(b) the bs 8 / 512^2 bf16 G+D step with both terms on against the default step, two trainers interleaved in one process.
One line per measurement; profiles/style_loss.txt is this script's output.
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import michigan_amd  # noqa: F401,E402
import torch  # noqa: E402
from michigan_amd import _cabi, ops  # noqa: E402

BS = 8
TAPS = [(512, 64), (256, 128), (128, 256), (64, 512), (32, 512)]
EPS = 1e-5


def reference_terms(x, s, t, masks, content):
    """loss.py:624-694 on NCHW tensors: (style, content or None)."""
    n, c = x.shape[:2]
    if masks is None:
        def mean_std(f):
            v = f.reshape(n, c, -1)
            return v.mean(dim=2), (v.var(dim=2) + EPS).sqrt()
        (mx, sx), (ms, ss) = mean_std(x), mean_std(s)
        style = torch.nn.functional.mse_loss(mx, ms) + torch.nn.functional.mse_loss(sx, ss)
        return style, (torch.nn.functional.mse_loss(x, t) if content else None)

    def mean_std_mask(f, mask):
        m1 = mask.reshape(n, 1, -1)
        f1 = f.reshape(n, c, -1) * m1
        mean = (f1.sum(dim=2) / (m1.sum(dim=2) + EPS)).reshape(n, c, 1)
        var = (((f1 - mean) * m1) ** 2).sum(dim=2) / (m1.sum(dim=2) + EPS) + EPS
        return mean.reshape(n, c), var.sqrt()
    m_style, m_content = masks
    (mx, sx), (ms, ss) = mean_std_mask(x, m_style), mean_std_mask(s, m_content)
    style = torch.nn.functional.mse_loss(mx, ms) + torch.nn.functional.mse_loss(sx, ss)
    if not content:
        return style, None
    return style, ((x * m_content - t * m_content) ** 2).sum() / (m_content.sum() * c + EPS)


def timed(fn, n):
    """Seconds per call: device events around n calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / n


def bench_taps(masked):
    g = torch.Generator().manual_seed(11)
    be = _cabi.backend()
    print("taps at bs %d, bf16, %s; per call, median of 5 alternating rounds" % (BS, "remove_background masks (hair fraction ~0.4)" if masked else "unmasked"), flush=True)
    for i, (hw, c) in enumerate(TAPS):
        content = i == len(TAPS) - 1
        flags = ops.FEAT_STYLE | (ops.FEAT_CONTENT if content else 0)
        feats = lambda: torch.randn(BS, hw, hw, c, generator=g).relu_().to(torch.bfloat16).cuda()
        x, s = feats(), feats()
        t = feats() if content else None
        masks = None
        if masked:
            masks = [(torch.rand(BS, hw, hw, generator=g) < 0.4).float().cuda() for _ in range(2)]      # style label, content label
        out = torch.empty(2, dtype=torch.float32, device="cuda")
        coef = torch.empty(4 * BS * c, dtype=torch.float32, device="cuda")
        ws = torch.empty(int(be.mg_feat_moment_workspace(BS, hw * hw, c)), dtype=torch.uint8, device="cuda")
        dx = torch.empty_like(x)
        m3 = (masks[0], masks[1], masks[1]) if masked else (None, None, None)
        desc = ops._feat_desc(x, s, t, m3, flags, out, coef, ws)
        one = torch.ones(1, dtype=torch.float32, device="cuda")
        stream = ops._stream(x)
        fwd = lambda: be.mg_feat_moment_loss_fwd(desc, stream)
        bwd = lambda: be.mg_feat_moment_loss_bwd(desc, ops._p(one), ops._p(one) if content else None, ops._p(dx), stream)
        xv = x.permute(0, 3, 1, 2).requires_grad_(True)
        sv, tv = s.permute(0, 3, 1, 2), (t.permute(0, 3, 1, 2) if content else None)
        mv = [m.unsqueeze(1) for m in masks] if masked else None

        def ref_fwd():
            st, co = reference_terms(xv, sv, tv, mv, content)
            return st + co if content else st

        def ref_both():
            xv.grad = None
            ref_fwd().backward()
        for fn in (fwd, bwd, ref_fwd, ref_both):
            timed(fn, 3)
        fwd()
        torch.cuda.synchronize()
        got = out.tolist()
        st, co = reference_terms(xv.detach().float(), sv.float(), tv.float() if content else None, [m.float() for m in mv] if masked else None, content)
        want = [float(st), float(co) if content else 0.0]
        reps = 20 if hw >= 256 else 100
        tf, tb, rf, rb = [], [], [], []
        for _ in range(5):
            tf.append(timed(fwd, reps))
            rf.append(timed(ref_fwd, max(reps // 4, 5)))
            tb.append(timed(bwd, reps))
            rb.append(timed(ref_both, max(reps // 4, 5)))
        med = statistics.median
        tensor = BS * hw * hw * c * 2
        frac = 0.4 if masked else 1.0
        mask_bytes = BS * hw * hw * 4
        fwd_bytes = tensor * frac * (3 if content else 2) + (mask_bytes * (3 if content else 2) if masked else 0)
        bwd_bytes = tensor * frac * (2 if content else 1) + tensor + (mask_bytes * (2 if content else 1) if masked else 0)
        ref_bwd = med(rb) - med(rf)
        print("tap %d [%d,%d^2,%d] flags %d: fwd %.1f us (min %.1f; %.0f MB -> %.0f GB/s) | bwd %.1f us (min %.1f; %.0f MB -> %.0f GB/s) | "
              "torch ops fwd %.1f us, bwd %.1f us | fwd x%.1f, bwd x%.1f | values fused %s fp32 torch %s"
              % (i + 1, BS, hw, c, flags, 1e6 * med(tf), 1e6 * min(tf), fwd_bytes / 1e6, fwd_bytes / med(tf) / 1e9, 1e6 * med(tb), 1e6 * min(tb),
                 bwd_bytes / 1e6, bwd_bytes / med(tb) / 1e9, 1e6 * med(rf), 1e6 * ref_bwd, med(rf) / med(tf), ref_bwd / med(tb),
                 ["%.6f" % v for v in got], ["%.6f" % v for v in want]), flush=True)
        del x, s, t, dx, xv, sv, tv, ws


def bench_step():
    from michigan_amd.model import Pix2PixTrainer, default_options
    from michigan_amd.synth import synth_batch
    data = {k: v.cuda() for k, v in synth_batch(BS, 512, seed=1234).items()}
    trainers = {}
    for name, over in (("default", {}), ("style + content on", dict(no_style_loss=False, no_content_loss=False))):
        torch.manual_seed(0)
        trainers[name] = Pix2PixTrainer(default_options(crop_size=512, gpu_ids=[0], compute_dtype="bf16", **over))

    def step(name):
        trainers[name].run_generator_one_step(data)
        trainers[name].run_discriminator_one_step(data)
    for name in trainers:
        for _ in range(3):
            step(name)
    times = {k: [] for k in trainers}
    for _ in range(4):
        for name in trainers:
            step(name)
            times[name].append(timed(lambda: step(name), 5))
    for name, ts in times.items():
        print("G+D step bf16 bs%d 512^2, %s: %s ms/step (median %.2f)" % (BS, name, ["%.2f" % (1e3 * t) for t in ts], 1e3 * statistics.median(ts)), flush=True)
    losses = {k: round(float(v.detach().float().mean()), 4) for k, v in trainers["style + content on"].get_latest_losses().items()}
    print("both terms on - default: %+.2f ms/step (medians); losses %s"
          % (1e3 * (statistics.median(times["style + content on"]) - statistics.median(times["default"])), losses), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this is a GPU measurement"
    bench_taps("--masked" in sys.argv)
    if "--no-step" not in sys.argv:
        bench_step()
