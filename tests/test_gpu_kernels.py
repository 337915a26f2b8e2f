"""-m gpu: every HIP entry point, called through the C ABI / op layer, against the
contract emulator (oracle/cabi_emulator.py) on identical inputs.

Tolerances (stated per dtype):
  f32  : |hip - ref| <= 2e-5 * max|ref|   (fp32 MFMA = exact fma, two-level sums; only the
         summation order differs from the float64 emulator)
  bf16 : |hip - ref| <= 2^-7 * max|ref|   (one bf16 ulp at the top of the range:
         both sides round an fp32/fp64 accumulation to bf16 once)
That bound is one ulp of the LARGEST value; tests/test_gpu_exact_sums.py holds the bf16 kernels tighter -- bit equality with the
once-rounded float64 value on operands whose sums are exact -- and is where "rounds once" itself is pinned.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16}
TOL = {"f32": 2e-5, "bf16": 2.0 ** -7}


def _close(name, got, ref, tol):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert got.shape == ref.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    err = (got - ref).abs().max().item()
    scale = max(ref.abs().max().item(), 1e-6)
    assert np.isfinite(err) and err <= tol * scale, f"{name}: max err {err:.3e} > {tol:.1e} * {scale:.3e}"


def _both(fn, tensors, grads_of=()):
    """Run fn on cuda tensors with the HIP backend and on cpu copies with the emulator."""
    from michigan_amd import _cabi
    from oracle.cabi_emulator import EmulatorBackend
    outs = []
    dry = os.environ.get("MG_TEST_DRYRUN") == "1"       # CPU-only plumbing check of this file (emulator both sides)
    for dev, be in (("cpu" if dry else "cuda", EmulatorBackend() if dry else None), ("cpu", EmulatorBackend())):
        prev = _cabi.set_backend(be)
        try:
            if be is None:
                assert _cabi.backend().name == "hip"
            args = [t.detach().to(dev).requires_grad_(t.requires_grad) if torch.is_tensor(t) else t for t in tensors]
            res = fn(*args)
            if dev == "cuda":
                torch.cuda.synchronize()
            outs.append((res, args))
        finally:
            _cabi.set_backend(prev)
    return outs


def test_probe_mfma_fragment_layout(hip_backend):
    out = torch.zeros(3, 64, 16, device="cuda")
    hip_backend.mg_probe_mfma_layout(out.data_ptr(), None)
    torch.cuda.synchronize()
    out = out.cpu()
    lane = torch.arange(64)[:, None]
    reg = torch.arange(16)[None, :]
    row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)          # C/D row held by (lane, reg)
    col = (lane & 31).expand(64, 16)
    assert torch.equal(out[0], row.float()), "bf16 32x32x16: A row != lane&31 or C/D row map differs"
    assert torch.equal(out[1], col.float()), "bf16 32x32x16: B col != lane&31 or C/D col map differs"
    assert torch.equal(out[2], row.float()), "f32 32x32x2: fragment map differs"


def test_probe_ds_read_tr16(hip_backend):
    src = torch.arange(256, dtype=torch.int16, device="cuda")
    dst = torch.zeros(256, dtype=torch.int16, device="cuda")
    hip_backend.mg_probe_tr16(src.data_ptr(), dst.data_ptr(), None)
    torch.cuda.synchronize()
    got = dst.cpu().view(64, 4)
    m = src.cpu().view(4, 16, 4)                               # [group][lane i][elem e]
    l = torch.arange(16)
    exp = torch.stack([torch.stack([m[g, 4 * j + (l >> 2), l & 3] for j in range(4)], dim=1) for g in range(4)]).view(64, 4)
    assert torch.equal(got, exp), f"ds_read_b64_tr_b16 map differs from the assumed one:\n{got[:16]}"


CONV_CASES = [
    # cin, cout, k, stride, pad, H, W, N
    (128, 128, 3, 1, 1, 24, 20, 2),     # 128x128 tile, full K chunks
    (64, 64, 3, 1, 1, 33, 17, 1),       # 64x256 tile
    (48, 200, 3, 1, 1, 9, 13, 2),       # K tail (48 = 32 + 16), ragged Cout
    (4, 128, 3, 1, 1, 16, 16, 2),       # tiny Cin (SPADE mlp_shared)
    (64, 3, 3, 1, 1, 20, 20, 2),        # Cout 3 (conv_img), 32-row tile, scalar stores
    (7, 64, 4, 2, 2, 21, 19, 2),        # D layer 0: 4x4 s2 p2, odd size
    (64, 128, 4, 2, 2, 17, 17, 2),      # D s2
    (256, 512, 4, 1, 2, 10, 9, 1),      # D s1 p2
    (512, 1, 4, 1, 2, 9, 9, 2),         # D head
    (3, 64, 7, 1, 0, 22, 22, 1),        # 7x7 (background encoder, pre-padded)
    (64, 128, 4, 2, 0, 18, 18, 1),      # 4x4 s2 on reflect-padded input
    (24, 40, 3, 2, 1, 16, 16, 2),       # partial-conv trunk 3x3 s2
    (1024, 512, 1, 1, 0, 8, 8, 2),      # conv_s 1x1
    (16, 32, 3, 1, 1, 12, 12, 2),       # packed taps: 2 (bf16) taps per K chunk, 8 taps per wgrad N tile
    (32, 64, 3, 1, 1, 10, 10, 1),       # Cin == one bf16 chunk; wgrad packs 4 taps per tile
    (8, 128, 7, 1, 3, 14, 14, 1),       # 49 taps, packed (ragged last chunk: 49 = 12*4 + 1)
    (2048, 128, 3, 1, 1, 8, 8, 2),      # low-resolution long-K: split-K forward (gamma/beta dgrad shape)
    (1024, 1024, 3, 1, 1, 8, 8, 2),     # 1024-channel block at the 8x8 latent: split-K forward and dgrad
    (512, 200, 3, 1, 1, 7, 5, 1),       # split-K with ragged pixels / channels
]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv2d_fwd_bwd(case, dt):
    from michigan_amd import ops
    cin, cout, k, s, p, H, W, N = case
    g = torch.Generator().manual_seed(1234)
    x = torch.randn(N, H, W, cin, generator=g).to(DT[dt]).requires_grad_()
    w = (torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5).requires_grad_()
    b = torch.randn(cout, generator=g).requires_grad_()

    def fn(x, w, b):
        y = ops.conv2d(x, w, b, stride=s, padding=p, act=ops.ACT_LRELU)
        gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(7)).to(y.dtype).to(y.device)
        gx, gw, gb = torch.autograd.grad(y, (x, w, b), gy)
        return y, gx, gw, gb

    (hip, _), (ref, _) = _both(fn, (x, w, b))
    for name, a, r in zip(("y", "dx", "dw", "db"), hip, ref):
        _close(f"conv {case} {dt} {name}", a, r, TOL[dt] * (4 if name in ("dw", "db") and dt == "bf16" else 1))


def test_fp32_conv_sums_are_two_level(hip_backend):
    """The fp32 kernels' accuracy property, pinned: every output of a K = 9216-term convolution (1024 channels x 3x3, the hot path's
    longest reduction) is a two-level sum -- 16-term blocks from zero, then the block sums (csrc/mg_conv_common.h mma_f32_chunk, round
    4) -- not ONE sequential fp32 chain.  tools/fp32_chain_error.py: rms error of such a dot product against float64 4.4e-7 two-level,
    1.2e-6 as one chain (what rounds 1-3 did: 2x ATen's forward error, and with it the ReLU sign flips that dominated the fp32
    gradient distance).  Forward (halo kernel), data gradient (same kernel, transposed weights) and weight gradient (pixels as K:
    8 x 32 x 32 = 8192 terms per split-free sum) against float64 on the same fp32 values; bounds = 1.5x the two-level figure."""
    from michigan_amd import ops
    g = torch.Generator().manual_seed(77)
    N, H, W, C = 8, 32, 32, 1024
    x = torch.relu(torch.randn(N, H, W, C, generator=g)).requires_grad_()
    w = (torch.randn(64, C, 3, 3, generator=g) / (9 * C) ** 0.5).requires_grad_()
    gy = torch.randn(N, H, W, 64, generator=g)
    xc, wc = x.detach().cuda().requires_grad_(), w.detach().cuda().requires_grad_()
    y = ops.conv2d(xc, wc, None, stride=1, padding=1)
    gx, gw = torch.autograd.grad(y, (xc, wc), gy.cuda())
    torch.cuda.synchronize()
    xd, wd = x.detach().double().permute(0, 3, 1, 2).requires_grad_(), w.detach().double().requires_grad_()
    yd = torch.nn.functional.conv2d(xd, wd, None, stride=1, padding=1)
    gxd, gwd = torch.autograd.grad(yd, (xd, wd), gy.double().permute(0, 3, 1, 2))
    rms = lambda a, b: float(((a.double().cpu() - b).norm() / b.norm()))
    e_y = rms(y.permute(0, 3, 1, 2), yd.detach())
    e_dx = rms(gx.permute(0, 3, 1, 2), gxd)
    e_dw = rms(gw, gwd)
    print("fp32 two-level sums, rms relative error vs float64: y %.2e  dx %.2e  dw %.2e" % (e_y, e_dx, e_dw))
    # measured on MI355X: y 4.2e-7, dx 1.3e-7, dw 1.4e-7; the -DMG_F32_ONE_CHAIN=1 build: 1.17e-6, 4.2e-7, 2.8e-7 (fails all three)
    assert e_y < 6.6e-7, e_y            # K = 9216: the numpy model gives 4.4e-7 two-level, 1.2e-6 as one chain
    assert e_dx < 2.5e-7, e_dx          # K = 576 (64 channels x 9 taps)
    assert e_dw < 2.1e-7, e_dw          # K = 8192 pixels, shortened by the split-K


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_conv2d_residual_and_tanh(dt):
    from michigan_amd import ops
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 12, 12, 64, generator=g).to(DT[dt]).requires_grad_()
    r = torch.randn(2, 12, 12, 96, generator=g).to(DT[dt]).requires_grad_()
    w = (torch.randn(96, 64, 3, 3, generator=g) / 24).requires_grad_()

    def fn(x, r, w):
        y = ops.conv2d(x, w, None, padding=1, resid=r)
        gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(3)).to(y.dtype).to(y.device)
        gx, gr, gw = torch.autograd.grad(y, (x, r, w), gy)
        return y, gx, gr, gw

    (hip, _), (ref, _) = _both(fn, (x, r, w))
    for name, a, rr in zip(("y", "dx", "dres", "dw"), hip, ref):
        _close(f"resid {dt} {name}", a, rr, TOL[dt] * (4 if name == "dw" and dt == "bf16" else 1))

    def fn2(x, w3):
        y = ops.conv2d(x, w3, None, padding=1, act=ops.ACT_TANH)
        gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(3)).to(y.dtype).to(y.device)
        gx, gw = torch.autograd.grad(y, (x, w3), gy)
        return y, gx, gw
    w3 = (torch.randn(3, 64, 3, 3, generator=g) / 24).requires_grad_()
    (hip, _), (ref, _) = _both(fn2, (x, w3))
    for name, a, rr in zip(("y", "dx", "dw"), hip, ref):
        _close(f"tanh {dt} {name}", a, rr, TOL[dt] * (4 if name == "dw" and dt == "bf16" else 1))


@pytest.mark.parametrize("tr", [True, False], ids=["tr16", "gather"])
def test_wgrad_bf16_both_fragment_paths(tr):
    from michigan_amd import ops
    old = ops.WGRAD_USE_TR
    ops.WGRAD_USE_TR = tr
    try:
        g = torch.Generator().manual_seed(11)
        x = torch.randn(2, 19, 23, 136, generator=g).bfloat16()
        dy = torch.randn(2, 19, 23, 200, generator=g).bfloat16()

        def fn(x, dy):
            return (ops.conv_wgrad(x, dy, 3, 3, 1, 1),)
        (hip, _), (ref, _) = _both(fn, (x, dy))
        _close(f"wgrad tr={tr}", hip[0], ref[0], 2e-3)
    finally:
        ops.WGRAD_USE_TR = old


# 3x3 / stride 1 / pad 1 weight gradient on the kernel-row workgroup kernel (mg_wgrad3x3.hip): every tile variant
# (64/128 rows x 64/128 cols), W = 16 (two image rows per stage), 32 and 64, channel counts that are not tile
# multiples, one and several splits, with and without the fused bias gradient.
@pytest.mark.parametrize("want_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("N,H,W,cin,cg", [
    (2, 16, 16, 128, 128), (1, 8, 32, 64, 256), (1, 6, 64, 128, 64), (2, 4, 16, 64, 64),
    (1, 32, 32, 136, 200), (3, 16, 32, 72, 72), (1, 2, 16, 256, 128), (2, 64, 64, 128, 256)],
    ids=lambda v: str(v))
def test_wgrad3x3_kernel_row_tiles(N, H, W, cin, cg, want_bias):
    from michigan_amd import ops
    g = torch.Generator().manual_seed(N * 1000 + H * 10 + cin)
    x = torch.randn(N, H, W, cin, generator=g).bfloat16()
    dy = torch.randn(N, H, W, cg, generator=g).bfloat16()

    def fn(x, dy):
        r = ops.conv_wgrad(x, dy, 3, 3, 1, 1, want_bias=want_bias)
        return r if want_bias else (r,)
    (hip, _), (ref, _) = _both(fn, (x, dy))
    for name, a, r in zip(("dw", "dbias"), hip, ref):
        _close(f"wgrad3x3 {(N, H, W, cin, cg)} {name}", a, r, 2e-3)
    if not os.environ.get("MG_TEST_DRYRUN"):
        from michigan_amd import _cabi
        with _cabi.options({_cabi.OPT_WGRAD3X3: 0}):               # same problem on the generic kernel
            gen = fn(x.cuda(), dy.cuda())
        _close(f"wgrad3x3 vs generic {(N, H, W, cin, cg)}", hip[0], gen[0].cpu(), 2e-3)


def test_wgrad3x3_race_screen():
    """Same screen for the weight-gradient LDS-DMA ring: 30 repetitions of a chip-filling problem, each against the
    fp32 reference computed by torch (split-K atomics change the summation order, hence a tolerance, not equality)."""
    from michigan_amd import ops
    g = torch.Generator().manual_seed(17)
    x = torch.randn(8, 128, 128, 128, generator=g).bfloat16().cuda()
    dy = torch.randn(8, 128, 128, 256, generator=g).bfloat16().cuda()
    xf = torch.nn.functional.pad(x.float().permute(0, 3, 1, 2), (1, 1, 1, 1))
    ref = torch.stack([torch.einsum("nchw,nkhw->kc", xf[:, :, ky:ky + 128, kx:kx + 128], dy.float().permute(0, 3, 1, 2))
                       for ky in range(3) for kx in range(3)])                     # [9, Cg, Cin]
    scale = ref.abs().max().item()
    bad = 0
    for _ in range(30):
        dw = ops.conv_wgrad(x, dy, 3, 3, 1, 1)
        bad += int((dw - ref).abs().max().item() > 2e-3 * scale)
    assert bad == 0, f"{bad} of 30 runs differ from the reference"


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("C,H,W", [(64, 20, 24), (32, 16, 16), (48, 9, 11), (256, 8, 8), (16, 12, 12)])
def test_spade_modulate_fwd_bwd(C, H, W, dt):
    from michigan_amd import ops
    g = torch.Generator().manual_seed(C)
    x = (torch.randn(2, H, W, C, generator=g) * 1.5 + 0.3).to(DT[dt]).requires_grad_()
    actv = torch.randn(2, H, W, 128, generator=g).clamp_min(0).to(DT[dt]).requires_grad_()
    wg = (torch.randn(C, 128, 3, 3, generator=g) / 34).requires_grad_()
    wb = (torch.randn(C, 128, 3, 3, generator=g) / 34).requires_grad_()
    bg = (torch.randn(C, generator=g) * 0.1).requires_grad_()
    bb = (torch.randn(C, generator=g) * 0.1).requires_grad_()

    def fn(x, actv, wg, bg, wb, bb):
        mean, rstd, cnt, _ = ops.batch_stats(x)
        h = ops.spade_modulate(x, actv, wg, bg, wb, bb, mean, rstd, cnt, act=ops.ACT_LRELU)
        gh = torch.randn(h.shape, generator=torch.Generator().manual_seed(9)).to(h.dtype).to(h.device)
        grads = torch.autograd.grad(h, (x, actv, wg, bg, wb, bb), gh)
        return (h, mean, rstd) + grads

    (hip, _), (ref, _) = _both(fn, (x, actv, wg, bg, wb, bb))
    names = ("h", "mean", "rstd", "dx", "dactv", "dwg", "dbg", "dwb", "dbb")
    for name, a, r in zip(names, hip, ref):
        loose = dt == "bf16" and name in ("dx", "dactv", "dwg", "dbg", "dwb", "dbb")
        _close(f"spade C={C} {dt} {name}", a, r, TOL[dt] * (6 if loose else 1) if name not in ("mean", "rstd") else 1e-5)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_channel_stats_wide_and_grouped(dt):
    from michigan_amd import ops
    g = torch.Generator().manual_seed(2)
    for shape, groups in (((1, 37, 29, 2048), 1), ((3, 33, 17, 128), 3), ((2, 129, 129, 64), 2), ((8, 8, 8, 1024), 1)):
        x = (torch.randn(shape, generator=g) + 0.5).to(DT[dt])

        for shift in (False, True):
            def fn(x):
                return (ops.channel_sums(x, groups, shift),)
            (hip, _), (ref, _) = _both(fn, (x,))
            _close(f"stats {shape} g={groups} {dt} shift={shift}", hip[0], ref[0], 1e-5)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_instance_norm_act(dt):
    from michigan_amd import ops
    g = torch.Generator().manual_seed(4)
    x = (torch.randn(4, 33, 35, 128, generator=g) * 2 + 1).to(DT[dt]).requires_grad_()

    def fn(x):
        y = ops.instance_norm_act(x, act=ops.ACT_LRELU)
        gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(6)).to(y.dtype).to(y.device)
        (gx,) = torch.autograd.grad(y, x, gy)
        return y, gx
    (hip, _), (ref, _) = _both(fn, (x,))
    _close(f"inorm {dt} y", hip[0], ref[0], TOL[dt])
    _close(f"inorm {dt} dx", hip[1], ref[1], TOL[dt] * 2)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("op", ["upsample2x", "avgpool3s2", "maxpool2"])
def test_resampling(op, dt):
    from michigan_amd import ops
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 17, 21, 24, generator=g).to(DT[dt]).requires_grad_()

    def fn(x):
        y = getattr(ops, op)(x)
        gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(1)).to(y.dtype).to(y.device)
        (gx,) = torch.autograd.grad(y, x, gy)
        return y, gx
    (hip, _), (ref, _) = _both(fn, (x,))
    _close(f"{op} {dt} y", hip[0], ref[0], TOL[dt])
    _close(f"{op} {dt} dx", hip[1], ref[1], TOL[dt])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_blend_and_adam(dt):
    from michigan_amd import ops
    g = torch.Generator().manual_seed(10)
    bgf = torch.randn(2, 9, 9, 64, generator=g).to(DT[dt]).requires_grad_()
    x = torch.randn(2, 9, 9, 64, generator=g).to(DT[dt]).requires_grad_()
    hair = (torch.rand(2, 9, 9, 1, generator=g) > 0.5).float()
    back = (torch.rand(2, 9, 9, 1, generator=g) > 0.5).float()

    def fn(bgf, x, hair, back):
        y = ops.blend(bgf, x, hair, back, act=ops.ACT_LRELU)
        gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(1)).to(y.dtype).to(y.device)
        return (y,) + torch.autograd.grad(y, (bgf, x), gy)
    (hip, _), (ref, _) = _both(fn, (bgf, x, hair, back))
    for a, r in zip(hip, ref):
        _close(f"blend {dt}", a, r, TOL[dt])
    if dt == "f32":
        p = torch.randn(10007, generator=g)
        gr = torch.randn(10007, generator=g)

        def fa(p, gr):
            p, m, v = p.clone(), torch.zeros_like(p), torch.zeros_like(p)
            for step in (1, 2, 3):
                ops.adam_step(p, gr, m, v, lr=1e-3, beta1=0.0, beta2=0.9, eps=1e-8, step=step)
            return p, m, v
        (hip, _), (ref, _) = _both(fa, (p, gr))
        for a, r in zip(hip, ref):
            _close("adam", a, r, 1e-6)
        # and against torch.optim.Adam itself
        q = torch.nn.Parameter(p.clone().cuda())
        opt = torch.optim.Adam([q], lr=1e-3, betas=(0.0, 0.9))
        for _ in range(3):
            q.grad = gr.cuda()
            opt.step()
        _close("adam vs torch.optim", hip[0], q.data, 1e-6)
        # beta1 = 0 (the reference's TTUR setting): exp_avg must be the gradient EXACTLY, also when this step's gradient is many orders
        # of magnitude below the previous one (torch's two-branch lerp: g - (g - m) * 0; the one-branch form m + (g - m) rounds g away
        # and the sign-like update g / (|g| + eps) then steps on the rounding)
        grs = [torch.randn(10007, generator=g), torch.randn(10007, generator=g) * 1e-9, torch.randn(10007, generator=g) * 1e-3]
        pc, mc, vc = p.clone().cuda(), torch.zeros(10007, device="cuda"), torch.zeros(10007, device="cuda")
        q = torch.nn.Parameter(p.clone().cuda())
        opt = torch.optim.Adam([q], lr=1e-3, betas=(0.0, 0.9))
        for step, gr_ in enumerate(grs, 1):
            ops.adam_step(pc, gr_.cuda(), mc, vc, lr=1e-3, beta1=0.0, beta2=0.9, eps=1e-8, step=step)
            q.grad = gr_.cuda()
            opt.step()
            assert torch.equal(mc, gr_.cuda()), step
            assert torch.equal(mc, opt.state[q]["exp_avg"]), step
            _close("adam (changing gradient scale) vs torch.optim, step %d" % step, pc, q.data, 1e-6)


def test_conv_matches_miopen_large_bf16():
    """Size-independent check at a BASELINE-sized layer (128->128 3x3 at 256^2, N=2): HIP conv vs
    torch's own GPU conv (fp32), plus linearity conv(a*x) == a*conv(x)."""
    from michigan_amd import ops
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 256, 256, 128, generator=g).bfloat16().cuda()
    w = (torch.randn(128, 128, 3, 3, generator=g) / 34).cuda()
    y = ops.conv2d(x, w, None, padding=1).float()
    ref = torch.nn.functional.conv2d(x.float().permute(0, 3, 1, 2), w.bfloat16().float(), padding=1).permute(0, 2, 3, 1)
    _close("conv vs torch gpu", y, ref, 2.0 ** -7)
    y2 = ops.conv2d(x * 2, w, None, padding=1).float()
    _close("linearity", y2, 2 * y, 2.0 ** -7)


@pytest.mark.parametrize("variant,opts", [("halo16", {"OPT_CONV_HALO": 1, "OPT_CONV_HALO_BIG": 1}), ("halo8", {"OPT_CONV_HALO": 1, "OPT_CONV_HALO_BIG": 0}),
                                          ("generic", {"OPT_CONV_HALO": 0, "OPT_CONV_HALO_BIG": 0})])
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_conv_race_screen(variant, opts, with_bias, dt):
    """The LDS-DMA pipelines order their loads with counted vmcnt + barriers only; a missing edge shows up as rare
    wrong tiles that depend on timing.  40 repetitions of a chip-filling conv (8 x 256^2, 128 -> 128), each compared
    with torch's fp32 conv: every run must agree (this caught the halo kernel going wrong ~10-90 % of the runs once a
    ds_write of the epilogue parameters had been added to its prologue; they are staged by LDS-DMA since)."""
    from michigan_amd import ops, _cabi
    g = torch.Generator().manual_seed(3)
    x = torch.randn(8, 256, 256, 128, generator=g).to(DT[dt]).cuda()
    w = (torch.randn(128, 128, 3, 3, generator=g) / 34).cuda()
    b = torch.randn(128, generator=g).cuda() if with_bias else None
    wr = w if dt == "f32" else w.bfloat16().float()
    ref = torch.nn.functional.conv2d(x.float().permute(0, 3, 1, 2), wr, b, padding=1).permute(0, 2, 3, 1)
    thr = 2e-3 if dt == "f32" else 0.06
    with _cabi.options({getattr(_cabi, k): v for k, v in opts.items()}):
        bad = 0
        for _ in range(40):
            y = ops.conv2d(x, w, b, padding=1).float()
            bad += int(((y - ref).abs() > thr).sum() > 0)
    assert bad == 0, f"{variant}: {bad} of 40 runs had wrong tiles"


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("N,H,W,C,P", [(2, 9, 11, 8, 3), (1, 16, 16, 64, 1), (2, 5, 7, 12, 2), (1, 4, 4, 8, 3)])
def test_reflect_pad_fwd_bwd(N, H, W, C, P, dt):
    from michigan_amd import ops
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(N, H, W, C, generator=g).to(DT[dt]).requires_grad_()

    def fn(x):
        y = ops.reflect_pad(x, P)
        gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(5)).to(y.dtype).to(y.device)
        (gx,) = torch.autograd.grad(y, x, gy)
        return y, gx
    (hip, _), (ref, _) = _both(fn, (x,))
    _close(f"reflect pad y {dt}", hip[0], ref[0], 0.0 if dt == "f32" else TOL[dt])
    _close(f"reflect pad dx {dt}", hip[1], ref[1], TOL[dt])
    want = torch.nn.functional.pad(x.detach().float().permute(0, 3, 1, 2), (P, P, P, P), mode="reflect").permute(0, 2, 3, 1)
    _close("reflect pad vs torch", hip[0], want, 0.0 if dt == "f32" else TOL[dt])


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("shape", [(64, 7, 4, 4), (128, 4, 3, 3), (256, 128, 3, 3)], ids=str)
def test_fused_spectral_norm_matches_torch(shape, train):
    """FusedSpectralNorm (gemv + mg_sn_* kernels) vs torch.nn.utils.spectral_norm on the same module state:
    normalised weight, in-place updated u / v buffers and the gradient w.r.t. weight_orig."""
    import copy
    import torch.nn as nn
    from torch.nn.utils import spectral_norm as torch_sn
    from michigan_amd.networks.spectral import spectral_norm as fused_sn
    torch.manual_seed(shape[0] + shape[1])
    base = nn.Conv2d(shape[1], shape[0], shape[2])
    ref, mine = torch_sn(copy.deepcopy(base)).cuda(), fused_sn(copy.deepcopy(base)).cuda()
    mine.load_state_dict(ref.state_dict())
    ref.train(train); mine.train(train)
    gy = torch.randn(shape, device="cuda")
    outs = []
    for m in (ref, mine):
        for hook in m._forward_pre_hooks.values():
            hook(m, None)                                   # the pre-forward hook computes m.weight
        w = m.weight
        (gw,) = torch.autograd.grad(w, m.weight_orig, gy)
        outs.append((w.detach(), m.weight_u.clone(), m.weight_v.clone(), gw))
    for name, a, b in zip(("weight", "u", "v", "grad"), outs[1], outs[0]):
        _close(f"spectral {shape} {name}", a, b, 2e-5)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("cin,cout,H,W,big", [(128, 128, 200, 176, 1), (128, 128, 200, 176, 0), (64, 64, 203, 181, 1),
                                               (32, 200, 150, 210, 1), (256, 136, 97, 131, 0)], ids=str)
def test_halo_conv_ragged_geometry(cin, cout, H, W, big, dt):
    """The halo-tile kernels only engage on chip-filling launches, which the small contract cases above never are:
    images whose height / width are not multiples of the 16x16 (or 8x16) tile and ragged channel counts, forward and
    data gradient, against torch's own fp32 convolution."""
    from michigan_amd import ops, _cabi
    g = torch.Generator().manual_seed(cin + H)
    x = torch.randn(4, H, W, cin, generator=g).to(DT[dt]).cuda().requires_grad_()
    w = (torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)).cuda()
    b = torch.randn(cout, generator=g).cuda()
    gy = torch.randn(4, H, W, cout, generator=g).to(DT[dt]).cuda()
    with _cabi.options({_cabi.OPT_CONV_HALO_BIG: big}):
        y = ops.conv2d(x, w, b, padding=1, act=ops.ACT_LRELU)
        (dx,) = torch.autograd.grad(y, x, gy)
    xr = x.detach().float().permute(0, 3, 1, 2).contiguous()
    wr = w if dt == "f32" else w.bfloat16().float()
    yr = torch.nn.functional.leaky_relu(torch.nn.functional.conv2d(xr, wr, b, padding=1), 0.2)
    # data gradient written out (the adjoint of a stride-1 conv is the transposed conv); act' through the output the
    # kernel stored, which is what its backward is defined on
    yq = y.detach().float().permute(0, 3, 1, 2)             # (pre-activations within rounding of 0 may differ in sign)
    dpre = gy.float().permute(0, 3, 1, 2) * torch.where(yq > 0, 1.0, 0.2)
    if dt == "bf16":
        dpre = dpre.bfloat16().float()
    dxr = torch.nn.functional.conv_transpose2d(dpre, wr, padding=1)
    _close(f"halo ragged y {dt}", y, yr.permute(0, 2, 3, 1), 2e-5 if dt == "f32" else TOL[dt])
    _close(f"halo ragged dx {dt}", dx, dxr.permute(0, 2, 3, 1), 5e-5 if dt == "f32" else TOL[dt])


@pytest.mark.parametrize("cout,H,W,act,with_bias", [(128, 72, 64, "relu", True), (64, 45, 96, "lrelu", False),
                                                     (96, 128, 32, "none", True), (128, 61, 128, "relu", True)], ids=str)
def test_thin_conv_8_channel_input(cout, H, W, act, with_bias):
    """The register-weight kernel for 3x3 convs over an 8-channel bf16 map (SPADE's mlp_shared): heights that are not
    multiples of its 8-row tile, 64 / 96 / 128 output channels, every fused activation, against torch's fp32 convolution
    and against the tap-list kernel it replaces (OPT_CONV_THIN = 0)."""
    from michigan_amd import ops, _cabi
    g = torch.Generator().manual_seed(cout + H)
    x = torch.randn(4, H, W, 8, generator=g).bfloat16().cuda()
    w = (torch.randn(cout, 8, 3, 3, generator=g) / 8).cuda()
    b = torch.randn(cout, generator=g).cuda() if with_bias else None
    code = {"relu": ops.ACT_RELU, "lrelu": ops.ACT_LRELU, "none": ops.ACT_NONE}[act]
    y = ops.conv2d(x, w, b, padding=1, act=code)
    with _cabi.options({_cabi.OPT_CONV_THIN: 0}):
        y_taps = ops.conv2d(x, w, b, padding=1, act=code)
    yr = torch.nn.functional.conv2d(x.float().permute(0, 3, 1, 2), w.bfloat16().float(), b, padding=1)
    yr = {"relu": torch.relu, "lrelu": lambda t: torch.nn.functional.leaky_relu(t, 0.2), "none": lambda t: t}[act](yr)
    _close("thin conv vs torch", y, yr.permute(0, 2, 3, 1), TOL["bf16"])
    _close("thin conv vs tap-list kernel", y, y_taps, TOL["bf16"])


@pytest.mark.parametrize("cg,H,W,want_bias", [(128, 72, 64, True), (64, 45, 96, True), (128, 61, 128, False), (64, 128, 32, True)], ids=str)
def test_thin_wgrad_8_channel_input(cg, H, W, want_bias):
    """Weight (and bias) gradient of the same layers: register-accumulator kernel vs torch's fp32 autograd on the same
    bf16 operands and vs the generic kernel (OPT_CONV_THIN = 0); heights that are not multiples of its 4-row tile."""
    from michigan_amd import ops, _cabi
    g = torch.Generator().manual_seed(cg + H)
    x = torch.randn(4, H, W, 8, generator=g).bfloat16().cuda()
    dy = torch.randn(4, H, W, cg, generator=g).bfloat16().cuda()
    res = ops.conv_wgrad(x, dy, 3, 3, 1, 1, want_bias=want_bias)
    with _cabi.options({_cabi.OPT_CONV_THIN: 0}):
        res_taps = ops.conv_wgrad(x, dy, 3, 3, 1, 1, want_bias=want_bias)
    w = torch.zeros(cg, 8, 3, 3, device="cuda", requires_grad=True)
    b = torch.zeros(cg, device="cuda", requires_grad=True)
    torch.nn.functional.conv2d(x.float().permute(0, 3, 1, 2), w, b, padding=1).backward(dy.float().permute(0, 3, 1, 2))
    dw_ref = w.grad.permute(2, 3, 0, 1).reshape(9, cg, 8)
    dw, dw_taps = (res[0], res_taps[0]) if want_bias else (res, res_taps)
    _close("thin wgrad vs torch", dw, dw_ref, 1e-4)
    _close("thin wgrad vs generic kernel", dw, dw_taps, 1e-4)
    if want_bias:
        _close("thin dbias vs torch", res[1], b.grad, 1e-4)


THIN_TAPS_CASES = [  # N, H, W, cout, k, stride, pad, act, bias   (8-channel bf16 input; the layers of the step + ragged variants;
    # every case has >= 64 forward tiles of 8 x 32 pixels and >= 64 gradient tiles of 4 x 32, the kernels' dispatch thresholds)
    (4, 70, 70, 64, 7, 1, 0, "relu", True),      # BackgroundEncode2.conv1 on a reflect-padded map (valid 7x7)
    (4, 128, 96, 64, 4, 2, 2, "lrelu", True),    # discriminator layer 0: 4x4 / stride 2 / pad 2 -> 65 x 49 (ragged tiles)
    (4, 128, 128, 64, 3, 2, 1, "none", False),   # appearance encoder layer 1: 3x3 / stride 2
    (2, 130, 75, 128, 5, 1, 2, "relu", True),    # two 64-channel halves, odd sizes
    (3, 41, 100, 96, 3, 1, 1, "lrelu", True),    # 3x3 / stride 1 whose width the register-weight kernel does not take
    (2, 67, 100, 64, 5, 1, 2, "none", True),     # 5x5: the 4-block column groups of the gradient kernel
]


@pytest.mark.parametrize("case", THIN_TAPS_CASES, ids=lambda c: "x".join(map(str, c)))
def test_thin_taps_conv_and_wgrad_any_window(case):
    """The LDS-weight kernels for ANY <= 7x7 window over an 8-channel bf16 map (7x7 first conv, 4x4 / stride-2 discriminator input
    conv, 3x3 / stride-2 encoder input conv): forward against torch's fp32 convolution and against the tap-list kernel
    (OPT_CONV_THIN = 1); weight / bias gradients (64-channel dY) against torch's fp32 autograd and the generic kernel."""
    from michigan_amd import ops, _cabi
    N, H, W, cout, k, stride, pad, act, with_bias = case
    g = torch.Generator().manual_seed(H * 7 + W + cout)
    x = torch.randn(N, H, W, 8, generator=g).bfloat16().cuda()
    w = (torch.randn(cout, 8, k, k, generator=g) / (2.0 * k)).cuda()
    b = torch.randn(cout, generator=g).cuda() if with_bias else None
    code = {"relu": ops.ACT_RELU, "lrelu": ops.ACT_LRELU, "none": ops.ACT_NONE}[act]
    y = ops.conv2d(x, w, b, stride=stride, padding=pad, act=code)
    with _cabi.options({_cabi.OPT_CONV_THIN: 1}):
        y_taps = ops.conv2d(x, w, b, stride=stride, padding=pad, act=code)
    yr = torch.nn.functional.conv2d(x.float().permute(0, 3, 1, 2), w.bfloat16().float(), b, stride=stride, padding=pad)
    yr = {"relu": torch.relu, "lrelu": lambda t: torch.nn.functional.leaky_relu(t, 0.2), "none": lambda t: t}[act](yr)
    assert tuple(y.shape) == tuple(yr.permute(0, 2, 3, 1).shape)
    _close("thin taps conv vs torch", y, yr.permute(0, 2, 3, 1), TOL["bf16"])
    _close("thin taps conv vs tap-list kernel", y, y_taps, TOL["bf16"])
    if cout != 64:
        return
    dy = torch.randn(N, yr.shape[2], yr.shape[3], 64, generator=g).bfloat16().cuda()
    res = ops.conv_wgrad(x, dy, k, k, stride, pad, want_bias=with_bias)
    res2 = ops.conv_wgrad(x, dy, k, k, stride, pad, want_bias=with_bias)
    with _cabi.options({_cabi.OPT_CONV_THIN: 1}):
        res_taps = ops.conv_wgrad(x, dy, k, k, stride, pad, want_bias=with_bias)
    wz = torch.zeros(64, 8, k, k, device="cuda", requires_grad=True)
    bz = torch.zeros(64, device="cuda", requires_grad=True)
    torch.nn.functional.conv2d(x.float().permute(0, 3, 1, 2), wz, bz, stride=stride, padding=pad).backward(dy.float().permute(0, 3, 1, 2))
    dw_ref = wz.grad.permute(2, 3, 0, 1).reshape(k * k, 64, 8)
    dw, dw2, dw_taps = (res[0], res2[0], res_taps[0]) if with_bias else (res, res2, res_taps)
    _close("thin taps wgrad vs torch", dw, dw_ref, 1e-4)
    _close("thin taps wgrad vs generic kernel", dw, dw_taps, 1e-4)
    assert torch.equal(dw, dw2), "slab sums in workgroup order: two launches must agree bit for bit"
    prev = ops.WGRAD_DETERMINISTIC
    ops.set_deterministic(True)                       # the caller's slab workspace + the library's finishing pass: the same sums in the same order
    try:
        res_det = ops.conv_wgrad(x, dy, k, k, stride, pad, want_bias=with_bias)
    finally:
        ops.set_deterministic(prev)
    assert torch.equal(dw, res_det[0] if with_bias else res_det)
    if with_bias:
        assert torch.equal(res[1], res_det[1])
    if with_bias:
        _close("thin taps dbias vs torch", res[1], bz.grad, 1e-4)


@pytest.mark.parametrize("case", [("img", 3, 3, 1, 1), ("dgrad3x3", 8, 3, 1, 1), ("dgrad4x4s2", 8, 4, 2, 2), ("dgrad3x3s2", 8, 3, 2, 1)], ids=lambda c: c[0])
def test_few_output_channel_convs_over_64_channels(case):
    """The 16-row MFMA kernel for <= 16 GEMM rows over a 64-channel bf16 input (mg_conv_dot.hip): conv_img (64 -> 3, tanh) forward and
    the data gradients that end in an 8-channel network input (stride 1, and the four parity classes of a stride-2 conv with strided
    stores), ragged tiles, against torch fp32 and against the tap-list kernel (OPT_CONV_DOT = 1)."""
    from michigan_amd import ops, _cabi
    name, cnarrow, k, stride, pad = case
    g = torch.Generator().manual_seed(len(name) + k)
    if name == "img":
        x = torch.randn(3, 72, 100, 64, generator=g).bfloat16().cuda()
        w = (torch.randn(3, 64, 3, 3, generator=g) / 24).cuda()
        b = torch.randn(3, generator=g).cuda()
        y = ops.conv2d(x, w, b, padding=1, act=ops.ACT_TANH)
        with _cabi.options({_cabi.OPT_CONV_DOT: 1}):
            y_taps = ops.conv2d(x, w, b, padding=1, act=ops.ACT_TANH)
        yr = torch.tanh(torch.nn.functional.conv2d(x.float().permute(0, 3, 1, 2), w.bfloat16().float(), b, padding=1)).permute(0, 2, 3, 1)
        _close("few-output conv vs torch", y[..., :3], yr, TOL["bf16"])
        _close("few-output conv vs tap-list kernel", y, y_taps, TOL["bf16"])
        return
    # data gradient of an 8 -> 64 conv: 64 "input" channels (dy), 8 output channels (dx)
    x = torch.randn(3, 70, 96, 8, generator=g).bfloat16().cuda().requires_grad_(True)
    w = (torch.randn(64, 8, k, k, generator=g) / (3.0 * k)).cuda()
    y = ops.conv2d(x, w, None, stride=stride, padding=pad)
    gy = torch.randn(y.shape, generator=g).bfloat16().cuda()
    (dx,) = torch.autograd.grad(y, x, gy)
    with _cabi.options({_cabi.OPT_CONV_DOT: 1}):
        y2 = ops.conv2d(x, w, None, stride=stride, padding=pad)
        (dx_taps,) = torch.autograd.grad(y2, x, gy)
    xr = x.detach().float().permute(0, 3, 1, 2).requires_grad_(True)
    yr = torch.nn.functional.conv2d(xr, w.bfloat16().float(), None, stride=stride, padding=pad)
    (dxr,) = torch.autograd.grad(yr, xr, gy.float().permute(0, 3, 1, 2))
    _close("few-output dgrad vs torch", dx, dxr.permute(0, 2, 3, 1), TOL["bf16"])
    _close("few-output dgrad vs tap-list kernel", dx, dx_taps, TOL["bf16"])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("slope", [0.0, 0.2])
def test_data_gradient_with_folded_activation_mask(dt, slope):
    """mg_conv_desc.mask_slope: the data gradient of a 3x3 conv multiplied in its epilogue by the backward mask of the ReLU (0) /
    LeakyReLU (slope) whose output the conv consumed -- halo kernel, ragged sizes -- against the two-step computation."""
    from michigan_amd import ops
    tdt = torch.float32 if dt == "f32" else torch.bfloat16
    g = torch.Generator().manual_seed(int(slope * 10) + 3)
    n, h, w, cin, cout = 2, 40, 48, 128, 128
    x = torch.randn(n, h, w, cin, generator=g).to(tdt).cuda()             # the activation output the conv consumed (only its sign matters)
    dy = torch.randn(n, h, w, cout, generator=g).to(tdt).cuda()
    wgt = (torch.randn(cout, cin, 3, 3, generator=g) / 24).cuda()
    wt = ops.pack_weight(wgt, None, tdt, ops._roundup(cin, 128), cout, 1)
    plain = ops.conv_dgrad(dy, wt, 3, 3, 1, 1, (h, w), cin)
    masked = ops.conv_dgrad(dy, wt, 3, 3, 1, 1, (h, w), cin, relu_mask=x, mask_slope=slope)
    ops._RELU_MASKED.pop(masked.data_ptr(), None)
    want = torch.where(x.float() > 0, plain.float(), plain.float() * slope)
    _close(f"masked dgrad slope {slope} {dt}", masked, want, 1e-6 if dt == "f32" else TOL["bf16"])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("C,H,W", [(64, 200, 176), (136, 97, 131)], ids=str)
def test_spade_halo_ragged_geometry(C, H, W, dt):
    """SPADE epilogue on the halo-tile kernel (chip-filling, ragged tiles and channels): forward and the full backward
    (batch statistics included) against torch autograd on the written-out formula, fp32 on the GPU."""
    from michigan_amd import ops
    g = torch.Generator().manual_seed(C)
    x = (torch.randn(4, H, W, C, generator=g) * 1.5 + 0.3).to(DT[dt]).cuda().requires_grad_()
    actv = torch.randn(4, H, W, 128, generator=g).clamp_min(0).to(DT[dt]).cuda().requires_grad_()
    wg = (torch.randn(C, 128, 3, 3, generator=g) / 34).cuda().requires_grad_()
    wb = (torch.randn(C, 128, 3, 3, generator=g) / 34).cuda().requires_grad_()
    bg = (torch.randn(C, generator=g) * 0.1).cuda().requires_grad_()
    bb = (torch.randn(C, generator=g) * 0.1).cuda().requires_grad_()
    gh = torch.randn(4, H, W, C, generator=g).to(DT[dt]).cuda()
    mean, rstd, cnt, _ = ops.batch_stats(x)
    h = ops.spade_modulate(x, actv, wg, bg, wb, bb, mean, rstd, cnt, act=ops.ACT_NONE)
    got = torch.autograd.grad(h, (x, actv, wg, wb, bg, bb), gh)

    q = (lambda t: t.bfloat16().float()) if dt == "bf16" else (lambda t: t)
    xr = x.detach().float().permute(0, 3, 1, 2).contiguous().requires_grad_()
    ar = actv.detach().float().permute(0, 3, 1, 2).contiguous().requires_grad_()
    wgr, wbr = q(wg.detach()).requires_grad_(), q(wb.detach()).requires_grad_()
    bgr, bbr = bg.detach().clone().requires_grad_(), bb.detach().clone().requires_grad_()
    mu = xr.mean(dim=(0, 2, 3), keepdim=True)
    var = xr.var(dim=(0, 2, 3), unbiased=False, keepdim=True)
    gam = torch.nn.functional.conv2d(ar, wgr, bgr, padding=1)
    bet = torch.nn.functional.conv2d(ar, wbr, bbr, padding=1)
    hr = (xr - mu) / torch.sqrt(var + 1e-5) * (1 + gam) + bet
    want = torch.autograd.grad(hr, (xr, ar, wgr, wbr, bgr, bbr), gh.float().permute(0, 3, 1, 2))
    tol = 1e-4 if dt == "f32" else TOL[dt]
    _close(f"spade halo h {dt}", h, hr.permute(0, 2, 3, 1), tol)
    _close(f"spade halo dx {dt}", got[0], want[0].permute(0, 2, 3, 1), tol * 4)
    _close(f"spade halo dactv {dt}", got[1], want[1].permute(0, 2, 3, 1), tol * 4)
    for name, a, b in zip(("dwg", "dwb", "dbg", "dbb"), got[2:], want[2:]):
        _close(f"spade halo {name} {dt}", a, b, 2e-3 if dt == "f32" else 6 * TOL[dt])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_l1_mean_fused(dt):
    from michigan_amd import ops
    g = torch.Generator().manual_seed(12)
    a = torch.randn(3, 37, 29, 64, generator=g).to(DT[dt]).requires_grad_()
    b = torch.randn(3, 37, 29, 64, generator=g).to(DT[dt])

    def fn(a, b):
        loss = ops.l1_mean(a.permute(0, 3, 1, 2), b.permute(0, 3, 1, 2)) * 3.0
        (ga,) = torch.autograd.grad(loss, a)
        return loss.reshape(1), ga
    (hip, _), (ref, _) = _both(fn, (a, b))
    _close(f"l1 {dt} loss", hip[0], ref[0], 1e-5)
    _close(f"l1 {dt} grad", hip[1], ref[1], TOL[dt])
    want = torch.nn.functional.l1_loss(a.detach().float(), b.float()) * 3.0
    _close(f"l1 {dt} vs torch", hip[0], want.reshape(1), 1e-5)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_gabor_argmax_and_orientation_loss(dt):
    """Filter-bank kernel vs its contract (values, arg-max agreement, image gradient) and the whole L1OLoss vs the oracle."""
    import argparse
    from michigan_amd import networks, ops
    from michigan_amd.synth import synth_batch
    from oracle import michigan_oracle as O
    g = torch.Generator().manual_seed(21)
    img = torch.tanh(torch.randn(2, 75, 83, 3, generator=g)).to(DT[dt]).requires_grad_()

    def fn(img):
        bank = ops.gabor_bank(img.device)
        conf, idx = ops.gabor_argmax(img, bank)
        gc = torch.rand(conf.shape, generator=torch.Generator().manual_seed(2)).to(conf.device)
        (gi,) = torch.autograd.grad(conf, img, gc)
        return conf, idx.float(), gi
    (hip, _), (ref, _) = _both(fn, (img,))
    _close(f"gabor conf {dt}", hip[0], ref[0], 1e-4)
    agree = (hip[1].cpu() == ref[1].cpu()).float().mean().item()
    assert agree > 0.999, f"arg-max agreement {agree}"
    _close(f"gabor dimg {dt}", hip[2], ref[2], 5e-3 if dt == "f32" else 2e-2)

    b = synth_batch(2, 96, seed=6)
    fake = torch.tanh(torch.randn(2, 3, 96, 96, generator=g))
    want_o, want_c = O.orientation_loss(fake, b["orient"], b["input_tag"], use_ig=True)
    crit = networks.L1OLoss(argparse.Namespace(use_ig=True, orient_filter="gabor")).cuda()
    f2 = fake.permute(0, 2, 3, 1).contiguous().to(DT[dt]).cuda()
    got_o, got_c = crit(f2.permute(0, 3, 1, 2), b["orient"].cuda(), b["input_tag"].cuda())
    tol = 1e-4 if dt == "f32" else 2e-2
    assert abs(float(want_o) - float(got_o)) < tol * max(1.0, abs(float(want_o)))
    assert abs(float(want_c) - float(got_c)) < tol * max(1.0, abs(float(want_c)))


@pytest.mark.parametrize("epi", ["plain", "plain+resid", "spade"])
def test_wide_epilogue_stores_are_bit_identical_to_quad_stores(epi):
    """OPT_CONV_WIDE: the half-wave quad exchange (v_permlane32_swap) + 16-byte stores against the 8-byte-per-quad
    stores it replaces, bf16, on a halo-kernel shape and a generic-kernel shape -- same bits (only the store width changes)."""
    from michigan_amd import _cabi, ops
    g = torch.Generator().manual_seed(31)
    outs = []
    for v in (1, 0):
        with _cabi.options({_cabi.OPT_CONV_WIDE: v}):
            res = []
            for (n, h, w, cin, cout, k, s, p) in [(2, 48, 64, 64, 128, 3, 1, 1), (2, 33, 29, 64, 72, 4, 2, 1)]:
                gg = torch.Generator().manual_seed(n * h + cout)
                x = torch.randn(n, h, w, cin, generator=gg).bfloat16().cuda()
                wt = (torch.randn(cout, cin, k, k, generator=gg) / (cin * k * k) ** 0.5).cuda()
                b = torch.randn(cout, generator=gg).cuda()
                if epi == "spade" and k == 3:
                    c = cout // 2
                    xin = torch.randn(n, h, w, c, generator=gg).bfloat16().cuda()
                    mean, rstd = torch.randn(c, generator=gg).cuda(), (torch.rand(c, generator=gg) + 0.5).cuda()
                    wb = (torch.randn(c, cin, 3, 3, generator=gg) / 24).cuda()
                    y = ops.spade_modulate(xin, x, wt[:c].contiguous(), b[:c].contiguous(), wb, b[c:2 * c].contiguous(), mean, rstd,
                                           float(n * h * w), act=ops.ACT_LRELU)
                elif epi == "spade":
                    continue
                else:
                    ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
                    r = torch.randn(n, ho, wo, cout, generator=gg).bfloat16().cuda() if epi == "plain+resid" else None
                    y = ops.conv2d(x, wt, b, stride=s, padding=p, act=ops.ACT_LRELU, resid=r)
                res.append(y.detach().clone())
            torch.cuda.synchronize()
            outs.append(res)
    for a, b_ in zip(*outs):
        assert torch.equal(a.view(torch.int16), b_.view(torch.int16))


def test_side_stream_weight_gradient_survives_inplace_gradient_accumulation():
    """ops.sink_wgrad: a conv's dy is ALSO the gradient of its residual input; the autograd engine adds the next gradient that arrives
    for that input INTO the tensor it holds the last reference to.  In stream order that write follows the wgrad's reads; with the
    weight gradient on the side stream it races them unless sink_wgrad keeps dy referenced until its launch has finished (round 5:
    G_middle_1.conv_1's gradient came out at cosine 0.78 in the bs 8 / 512^2 test).  Here the side queue is made to LAG (a spin kernel
    in front of it), a residual conv's input receives a second gradient, and the side-stream result must equal the in-stream one."""
    from michigan_amd import ops
    from michigan_amd.networks.layers import HipConv2d
    from michigan_amd.optim import FlatAdam
    g = torch.Generator().manual_seed(23)
    conv = HipConv2d(128, 128, kernel_size=3, padding=1).cuda()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(128, 128, 3, 3, generator=g) / 34)
        conv.bias.copy_(torch.randn(128, generator=g) * 0.1)
    optim = FlatAdam(conv.parameters(), lr=1e-4)
    x0 = torch.randn(4, 64, 64, 128, generator=g).bfloat16().cuda()
    gy = torch.randn(4, 64, 64, 128, generator=g).bfloat16().cuda()
    prev = ops.WGRAD_SIDE_STREAM
    res = {}
    try:
        for side in (False, True, True):
            ops.WGRAD_SIDE_STREAM = side
            optim.zero_grad()
            x = x0.clone().requires_grad_()
            h = x * 1.0                                           # a non-leaf: its gradient is accumulated in the engine's input buffer
            if side:
                with torch.cuda.stream(ops.side_stream(x.device)):
                    torch.cuda._sleep(40_000_000)                # ~20 ms: every side-stream launch of this backward starts late
            u = h * 2.0
            y = conv(u, resid=h)                                  # the conv's backward hands ONLY dres (== its dy) to h: the first gradient
            z = y * 1.0                                           #   to arrive there, engine-owned (the conv's dy is no user tensor) ...
            z.backward(gy)                                        # ... and `u = 2 h`'s backward then adds 2 du INTO it, in place
            optim.finalize_grads()
            torch.cuda.synchronize()
            res.setdefault(side, []).append((conv.weight.grad.detach().float().clone(), x.grad.detach().float().clone()))
    finally:
        ops.WGRAD_SIDE_STREAM = prev
    (w0, dx0), = res[False]
    for w1, dx1 in res[True]:
        assert torch.equal(dx0, dx1)
        rel = ((w1 - w0).norm() / w0.norm()).item()
        assert rel < 1e-4, rel                                   # fp32 atomics in another order: ~1e-7; the race gave O(1)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_hinge_loss_and_wide_edge_weight_fused(dt):
    """mg_wide_edge_weight (bit-exact vs the reference's interpolate / max_pool2d formula, incl. the
    even-window (h + 1)^2 pooled map and non-square label sizes) and mg_hinge_fwd/bwd in the three modes, plus the GANLoss
    module on a [fake | real] pair against the plain-torch restatement of loss.py:60-140."""
    import argparse
    import torch.nn.functional as F
    from michigan_amd import networks, ops
    g = torch.Generator().manual_seed(31)
    label = (torch.rand(3, 1, 96, 80, generator=g) > 0.55).float()
    for (h, w) in ((67, 67), (35, 35), (66, 52), (17, 19), (8, 8)):
        x = (torch.randn(3, 1, h, w, generator=g) * 1.5).to(DT[dt]).requires_grad_()

        def fn(x, label):
            wm = ops.wide_edge_weight(label, h, w, 2.0)
            outs = [wm]
            for mode in (ops.HINGE_G, ops.HINGE_D_REAL, ops.HINGE_D_FAKE):
                loss = ops.hinge_loss(x, None if mode == ops.HINGE_G else wm, mode)
                (gx,) = torch.autograd.grad(loss * 2.0, x)
                outs += [loss.reshape(1), gx]
            return outs
        (hip, _), (ref, _) = _both(fn, (x, label))
        assert torch.equal(hip[0].cpu(), ref[0]), (h, w)                       # index / byte work: bit-exact
        for i in (1, 3, 5):
            _close(f"hinge {dt} loss {h}x{w} mode {i // 2}", hip[i], ref[i], 1e-5)
            _close(f"hinge {dt} grad {h}x{w} mode {i // 2}", hip[i + 1], ref[i + 1], TOL[dt])
    # the module, as pix2pix_model.py:571-575 calls it, vs plain torch
    opt = argparse.Namespace(wide_edge=2.0, remove_background=False)
    crit = networks.GANLoss("hinge", opt=opt)
    preds = [[(torch.randn(4, 1, s, s, generator=g)).to(DT[dt]).cuda()] for s in (67, 35)]
    lab = (torch.rand(4, 1, 128, 128, generator=g) > 0.5).float().cuda()
    got = crit(preds, False, for_discriminator=True, label=lab)
    want = 0
    for (p,) in preds:
        s = p.shape[2]
        k = max(1, int(s * 0.06)); pd = int(k / 2)
        t = F.interpolate(lab, size=(s, s), mode="nearest")
        e = F.interpolate(F.max_pool2d(t, k, 1, pd) - (1 - F.max_pool2d(1 - t, k, 1, pd)), size=(s, s), mode="nearest")
        want = want + -(torch.clamp_max(-p.float() - 1, 0) * (e * 2.0 + (1 - e))).mean()
    assert abs(float(got) - float(want) / 2) < 1e-5


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_gradient_sink_drain_matches_autograd_path(dt):
    """mg_grad_drain (GEMM-order arena -> reference-layout gradients: plain 3x3 / 1x1 / 4x4-s2 / 7x7 windows, a spectral-normed
    conv with its sigma-backward, a fused SPADE gamma|beta pair, biases) on the HIP kernels vs the contract emulator, and the
    sink path vs the plain autograd path (fill + unpack + sn_bwd + accumulate) on the same device."""
    import torch.nn as nn
    from michigan_amd import ops
    from michigan_amd.networks.layers import HipConv2d
    from michigan_amd.networks.normalization import SPADE
    from michigan_amd.networks.spectral import spectral_norm
    from michigan_amd.optim import FlatAdam

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.c7 = HipConv2d(8, 24, 7, padding=3)
            self.c3 = spectral_norm(HipConv2d(24, 40, 3, padding=1))
            self.c1 = spectral_norm(HipConv2d(40, 72, 1, bias=False))
            self.sp = SPADE("spadesyncbatch3x3", 72, 4)
            self.c4 = HipConv2d(72, 16, 4, stride=2, padding=2)

        def forward(self, x, seg):
            h = self.c7(x, act=ops.ACT_LRELU)
            h = self.c3(h, act=ops.ACT_RELU)
            h = self.c1(h)
            h = self.sp(h, seg, act=ops.ACT_LRELU)
            return self.c4(h)

    torch.manual_seed(5)
    net0 = Net()
    sd = {k: v.clone() for k, v in net0.state_dict().items()}
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 20, 28, 8, generator=g).to(DT[dt])
    seg = (torch.rand(2, 4, 20, 28, generator=g) > 0.5).float()
    gy = torch.randn(2, 11, 15, 16, generator=g).to(DT[dt])

    def run(sink):
        def fn(x, seg, gy):
            net = Net().to(x.device)
            net.load_state_dict(sd)
            opt = FlatAdam(net.parameters(), lr=1e-3, grad_sink=sink)
            for _ in range(2):                                  # two backward passes accumulate before one drain
                (net(x, seg).float() * gy.float()).sum().backward()
            opt.sync_grads()
            assert (len(opt._slot_list) > 0) == sink
            if sink:
                assert float(opt.gemm.abs().max()) == 0.0       # the drain re-zeroes what it read
            return [opt.flat_grad.clone()]
        return _both(fn, (x, seg, gy))
    (hip_s, _), (emu_s, _) = run(True)
    (hip_a, _), (emu_a, _) = run(False)
    tol = 2e-4 if dt == "f32" else 2.0 ** -6
    _close(f"sink {dt}: hip vs emulator", hip_s[0], emu_s[0], tol)
    _close(f"sink {dt}: sink vs autograd path (hip)", hip_s[0], hip_a[0], 2e-4 if dt == "f32" else 2.0 ** -7)
    _close(f"sink {dt}: sink vs autograd path (emulator)", emu_s[0], emu_a[0], 1e-5)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_batched_spectral_norm_and_pack_match_contract(dt):
    """mg_sn_power_iteration + mg_pack_weights (network-wide spectral norm / GEMM-image launches) and the arena re-pack on the
    HIP kernels vs the contract emulator: three optimiser iterations of a small net with two spectral-normed convs (3x3 with
    bias, 1x1 without), a SPADE pair and plain 7x7 / 4x4-s2 convs; from the second iteration on the batched paths are live."""
    import torch.nn as nn
    from michigan_amd import ops
    from michigan_amd.networks import spectral
    from michigan_amd.networks.layers import HipConv2d
    from michigan_amd.networks.normalization import SPADE
    from michigan_amd.optim import FlatAdam

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.c7 = HipConv2d(8, 24, 7, padding=3)
            self.c3 = spectral.spectral_norm(HipConv2d(24, 40, 3, padding=1))
            self.c1 = spectral.spectral_norm(HipConv2d(40, 72, 1, bias=False))
            self.sp = SPADE("spadesyncbatch3x3", 72, 4)
            self.c4 = HipConv2d(72, 16, 4, stride=2, padding=2)

        def forward(self, x, seg):
            spectral.prepare(self)
            h = self.c7(x, act=ops.ACT_LRELU)
            h = self.c3(h, act=ops.ACT_RELU)
            h = self.c1(h)
            h = self.sp(h, seg, act=ops.ACT_LRELU)
            return self.c4(h)

    torch.manual_seed(6)
    sd = {k: v.clone() for k, v in Net().state_dict().items()}
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 20, 28, 8, generator=g).to(DT[dt])
    seg = (torch.rand(2, 4, 20, 28, generator=g) > 0.5).float()
    gy = torch.randn(2, 11, 15, 16, generator=g).to(DT[dt])

    def fn(x, seg, gy):
        from michigan_amd import _cabi
        be = _cabi.backend()
        n = {"sn": 0, "pack": 0}
        o1, o2 = be.mg_sn_power_iteration, be.mg_pack_weights
        be.mg_sn_power_iteration = lambda *a: (n.__setitem__("sn", n["sn"] + 1), o1(*a))[1]
        be.mg_pack_weights = lambda *a: (n.__setitem__("pack", n["pack"] + 1), o2(*a))[1]
        try:
            net = Net().to(x.device)
            net.load_state_dict(sd)
            opt = FlatAdam(net.parameters(), lr=1e-3)
            outs = []
            for it in range(3):
                opt.zero_grad()
                out = net(x, seg)
                (out.float() * gy.float()).sum().backward()
                opt.step()
                outs.append(out.detach().float().clone())
            with torch.no_grad():
                net.eval()
                outs.append(net(x, seg).float().clone())          # eval mode: sigma from the stored u, v
            assert n["sn"] >= 3 and n["pack"] >= 4, n
            return outs + [net.c3.weight_u.clone(), net.c1.weight_v.clone(), opt.flat.clone()]
        finally:
            be.mg_sn_power_iteration, be.mg_pack_weights = o1, o2
    # ordered split-K sums on the device: behind sign-like Adam updates (lr 1e-3) the last bits of a near-zero gradient decide a
    # whole weight step, and fp32 atomics would make that -- hence passes 1..3 -- depend on the run
    prev = ops.WGRAD_DETERMINISTIC
    ops.set_deterministic(True)
    try:
        (hip, _), (ref, _) = _both(fn, (x, seg, gy))
    finally:
        ops.set_deterministic(prev)
    for i in range(4):
        _close(f"batched weights {dt}: output of pass {i}", hip[i], ref[i], (5e-4 if i == 0 else 3e-3) if dt == "f32" else 2.0 ** -5)
    # u, v after three optimiser steps: the weights they were iterated on already differ by a few sign-like Adam updates in bf16
    _close(f"batched weights {dt}: u", hip[4], ref[4], 1e-4 if dt == "f32" else 5e-3)
    _close(f"batched weights {dt}: v", hip[5], ref[5], 1e-4 if dt == "f32" else 5e-3)
    assert ((hip[6].cpu() - ref[6]).abs() > 2.5e-3).float().mean() < 0.01       # Adam (lr 1e-3): sign-like updates, see trainer_parity.compare


def test_batched_spectral_norm_unaligned_layer():
    """The power-iteration kernels' 4-byte fallback: a spectral-normed 3x3 conv over 3 input channels (cols = 27: rows of W are not
    16-byte aligned) next to an aligned one, three training passes (the batched path is live from the second), HIP vs the contract."""
    import torch.nn as nn
    from michigan_amd import ops
    from michigan_amd.networks import spectral
    from michigan_amd.networks.layers import HipConv2d

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.a = spectral.spectral_norm(HipConv2d(3, 24, 3, padding=1))
            self.b = spectral.spectral_norm(HipConv2d(24, 16, 3, padding=1))

        def forward(self, x):
            spectral.prepare(self)
            return self.b(self.a(x, act=ops.ACT_LRELU))

    torch.manual_seed(11)
    sd = {k: v.clone() for k, v in Net().state_dict().items()}
    x = torch.randn(2, 12, 16, 8, generator=torch.Generator().manual_seed(2))
    x[..., 3:] = 0

    def fn(x):
        net = Net().to(x.device)
        net.load_state_dict(sd)
        outs = []
        for _ in range(3):
            out = net(x)
            out.float().sum().backward()
            outs.append(out.detach().float().clone())
        return outs + [net.a.weight_u.clone(), net.a.weight_v.clone(), net.b.weight_v.clone()]
    (hip, _), (ref, _) = _both(fn, (x,))
    for i, (h, r) in enumerate(zip(hip, ref)):
        _close(f"unaligned spectral layer: value {i}", h, r, 1e-4)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("up", [False, True])
def test_spade_pair_with_folded_upsample(dt, up):
    """spade_modulate_pair (two SPADE modulations of one x as one autograd node; `up`: x read through the nearest-2x index map by
    the fused conv epilogue, mg_norm_bwd_reduce_up and mg_norm_bwd_apply2) on the HIP kernels vs the contract emulator, and
    against the unfused composition upsample2x -> spade_modulate x 2 (autograd adds the two dx, up2 adjoint) on the same device."""
    from michigan_amd import ops
    g = torch.Generator().manual_seed(41)
    n, hs, ws, c, ca = 2, 18, 22, 64, 128
    h, w = (2 * hs, 2 * ws) if up else (hs, ws)
    x = torch.randn(n, hs, ws, c, generator=g).to(DT[dt]).requires_grad_()
    a0 = torch.randn(n, h, w, ca, generator=g).clamp_min(0).to(DT[dt]).requires_grad_()
    a1 = torch.randn(n, h, w, ca, generator=g).clamp_min(0).to(DT[dt]).requires_grad_()
    ws_ = [torch.randn(c, ca, 3, 3, generator=g).mul_(0.03).requires_grad_() for _ in range(4)]
    bs_ = [torch.randn(c, generator=g).mul_(0.1).requires_grad_() for _ in range(4)]
    gy0 = torch.randn(n, h, w, c, generator=g).to(DT[dt])
    gy1 = torch.randn(n, h, w, c, generator=g).to(DT[dt])

    def run(fused):
        def fn(x, a0, a1, w0, w1, w2, w3, b0, b1, b2, b3, gy0, gy1):
            src = x
            mean, rstd, count, _ = ops.batch_stats_finish(ops.batch_stats_begin(src.detach(), up=up))
            if fused:
                h0, h1 = ops.spade_modulate_pair(src, ((a0, w0, b0, w1, b1), (a1, w2, b2, w3, b3)), mean, rstd, count,
                                                 acts=(ops.ACT_LRELU, ops.ACT_NONE), up=up)
            else:
                xf = ops.upsample2x(src) if up else src
                h0 = ops.spade_modulate(xf, a0, w0, b0, w1, b1, mean, rstd, count, act=ops.ACT_LRELU)
                h1 = ops.spade_modulate(xf, a1, w2, b2, w3, b3, mean, rstd, count, act=ops.ACT_NONE)
            loss = (h0.float() * gy0.float()).sum() + (h1.float() * gy1.float()).sum()
            grads = torch.autograd.grad(loss, [x, a0, a1, w0, w1, w2, w3, b0, b1, b2, b3])
            return [h0, h1] + list(grads)
        return _both(fn, (x, a0, a1, *ws_, *bs_, gy0, gy1))
    (hip_f, _), (emu_f, _) = run(True)
    (hip_u, _), (emu_u, _) = run(False)
    names = ["h0", "h1", "dx", "dactv0", "dactv1", "dwg0", "dwb0", "dwg1", "dwb1", "dbg0", "dbb0", "dbg1", "dbb1"]
    tol = {"f32": 5e-5, "bf16": 2.0 ** -6}[dt]
    for i, nm in enumerate(names):
        _close(f"pair {dt} up={up} {nm}: hip vs emulator", hip_f[i], emu_f[i], tol)
        _close(f"pair {dt} up={up} {nm}: fused vs unfused (emulator)", emu_f[i], emu_u[i], 1e-6 if dt == "f32" else 2.0 ** -6)
        _close(f"pair {dt} up={up} {nm}: fused vs unfused (hip)", hip_f[i], hip_u[i], tol * (4 if nm == "dx" and dt == "bf16" else 1))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_relu_tap_and_masked_maxpool_backward(dt):
    """A ReLU output with two consumers (act_tap -> mg_grad_sum_act) and a max-pool whose backward carries the producing ReLU's
    mask (mg_maxpool2_bwd relu_input): conv+ReLU -> {2x2 max-pool -> conv, loss tap} on the HIP kernels vs the contract
    emulator and, in fp32, vs torch autograd of the same graph."""
    import torch.nn.functional as F
    from michigan_amd import ops
    g = torch.Generator().manual_seed(51)
    x = torch.randn(2, 12, 20, 16, generator=g).to(DT[dt]).requires_grad_()
    w1 = torch.randn(32, 16, 3, 3, generator=g).mul_(0.1).requires_grad_()
    w2 = torch.randn(24, 32, 3, 3, generator=g).mul_(0.1).requires_grad_()
    gt = torch.randn(2, 12, 20, 32, generator=g).to(DT[dt])
    gp = torch.randn(2, 6, 10, 24, generator=g).to(DT[dt])

    def fn(x, w1, w2, gt, gp):
        y = ops.conv2d(x, w1, None, padding=1, act=ops.ACT_RELU)
        y1, y2 = ops.act_tap(y)
        z = ops.conv2d(ops.maxpool2(y1), w2, None, padding=1)
        loss = (z.float() * gp.float()).sum() + (y2.float() * gt.float()).sum()
        return [y, z] + list(torch.autograd.grad(loss, [x, w1, w2]))
    (hip, _), (ref, _) = _both(fn, (x, w1, w2, gt, gp))
    for i, nm in enumerate(["y", "z", "dx", "dw1", "dw2"]):
        _close(f"relu tap {dt} {nm}", hip[i], ref[i], 5e-5 if dt == "f32" else 2.0 ** -6)
    if dt == "f32":
        xt = x.detach().permute(0, 3, 1, 2).requires_grad_()
        y = F.relu(F.conv2d(xt, w1, padding=1))
        z = F.conv2d(F.max_pool2d(y, 2), w2, padding=1)
        loss = (z * gp.permute(0, 3, 1, 2)).sum() + (y * gt.permute(0, 3, 1, 2)).sum()
        want = torch.autograd.grad(loss, [xt, w1, w2])
        _close("relu tap f32 dx vs torch", hip[2], want[0].permute(0, 2, 3, 1), 1e-4)
        _close("relu tap f32 dw1 vs torch", hip[3], want[1], 1e-4)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_glue_kernels_match_contract(dt):
    """mg_glue.hip (the fused per-pixel passes around the convolutions) vs the contract emulator, whose contracts are written with the
    torch ops the host stack used to call (F.interpolate, F.max_pool2d, F.conv2d on the mask, ...): index / mask work bit-exact,
    value work within the dtype's rounding."""
    from michigan_amd import ops
    g = torch.Generator().manual_seed(77)
    td = DT[dt]
    # nearest pyramid: planes that are channel slices of NCHW tensors, ragged target sizes, zero-padded channels
    seg = torch.cat([(torch.rand(3, 2, 72, 60, generator=g) > 0.5).float(), torch.randn(3, 2, 72, 60, generator=g)], dim=1)
    sizes = [(9, 8), (18, 15), (36, 30), (72, 60), (50, 41)]

    def pyr(seg):
        outs = ops.nearest_pyramid(ops.planes_of(seg), sizes, 8, td)
        outs += ops.nearest_pyramid([seg[:, 1]], [(int(72 / d), int(60 / d)) for d in (8, 4, 2)], 1, torch.float32)
        return outs
    (hip, _), (ref, _) = _both(pyr, (seg,))
    for a, b in zip(hip, ref):
        assert torch.equal(a.cpu().view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32), b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32))
    # partial-conv mask chain + per-pixel affine (forward and both gradients)
    mask = (torch.rand(2, 40, 36, 1, generator=g) > 0.6).float()
    x = torch.randn(2, 40, 36, 16, generator=g).to(td).requires_grad_()
    raw = torch.randn(2, 20, 18, 24, generator=g).to(td).requires_grad_()
    bias = torch.randn(24, generator=g).requires_grad_()

    def pc(mask, x, raw, bias):
        sc, up = ops.pconv_mask(mask, 3, 2, 1)
        y0 = ops.pixel_affine(x, mask)
        y1 = ops.pixel_affine(raw, sc, bias, up)
        gx, = torch.autograd.grad(y0.float().square().sum(), x)
        graw, gb = torch.autograd.grad((y1.float() * 0.5).square().sum(), (raw, bias))
        return sc, up, y0, y1, gx, graw, gb
    (hip, _), (ref, _) = _both(pc, (mask, x, raw, bias))
    assert torch.equal(hip[0].cpu(), ref[0]) and torch.equal(hip[1].cpu(), ref[1])
    for i, name in ((2, "x*m"), (3, "raw*scale+b*m'"), (4, "d x"), (5, "d raw")):
        _close(f"pixel_affine {dt} {name}", hip[i], ref[i], TOL[dt])
    _close(f"pixel_affine {dt} d bias", hip[6], ref[6], 2e-2 if dt == "bf16" else 1e-4)
    # background-encoder input: dilation windows up to 33, ragged image size, both modes
    image, noise = torch.rand(2, 3, 70, 90, generator=g) * 2 - 1, torch.rand(2, 3, 70, 90, generator=g)
    m2 = torch.zeros(2, 2, 70, 90)
    m2[:, 1, 20:45, 30:70] = 1.0
    m2[:, 0] = 1 - m2[:, 1]
    for k, mode in ((5, 0), (25, 0), (33, 0), (1, 1)):
        def bgc(image, noise, m2):
            return ops.bg_compose(image, noise, m2[:, 1] if mode == 0 else m2[:, 0], k, mode, td)
        (hip, _), (ref, _) = _both(bgc, (image, noise, m2))
        assert torch.equal(hip[1].cpu(), ref[1]), (k, mode)
        _close(f"bg_compose {dt} k={k}", hip[0], ref[0], TOL[dt])
    # masked mean over the reference region written over the target region (ImageEncoder3's tail), forward and adjoint
    feat = torch.randn(3, 16, 12, 72, generator=g).to(td).requires_grad_()
    lref, ltag = (torch.rand(3, 16, 12, 1, generator=g) > 0.6).float(), (torch.rand(3, 16, 12, 1, generator=g) > 0.4).float()
    lref[2] = 0                                                            # an empty reference region: the area clamps to 1

    def mmf(feat, lref, ltag):
        out = ops.masked_mean_fill(feat, lref, ltag)
        gx, = torch.autograd.grad((out * out).sum(), feat)
        return out, gx
    (hip, _), (ref, _) = _both(mmf, (feat, lref, ltag))
    _close(f"masked_mean_fill {dt}", hip[0], ref[0], 1e-5)
    _close(f"masked_mean_fill {dt} adjoint", hip[1], ref[1], TOL[dt])
    # orientation-loss tail: both label forms, gradient of either output
    conf_raw = (torch.randn(2, 48, 40, generator=g) * 1.5).requires_grad_()
    idx = torch.randint(0, 32, (2, 48, 40), generator=g, dtype=torch.uint8)
    sem = torch.zeros(2, 2, 48, 40)
    sem[:, 1, 10:40, 8:30] = 1.0
    for label in (torch.randn(2, 2, 48, 40, generator=g).clamp(-1, 1), torch.randint(0, 255, (2, 1, 48, 40), generator=g).float()):
        def ol(conf_raw, idx, label, sem):
            lo, lc = ops.orient_loss(conf_raw, idx, label, sem[:, 1])
            g0, = torch.autograd.grad(lo * 3.0, conf_raw, retain_graph=True)
            g1, = torch.autograd.grad(lo + lc * 0.25, conf_raw)
            return lo.reshape(1), lc.reshape(1), g0, g1
        (hip, _), (ref, _) = _both(ol, (conf_raw, idx, label, sem))
        for i in range(4):
            _close(f"orient_loss {label.shape[1]}ch out {i}", hip[i], ref[i], 2e-5)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_batch_stats_keep_the_variance_under_a_large_mean(hip_backend, dt):
    """VERDICT r3 (parity before speed): var = E[x^2] - E[x]^2 on fp32 sums loses mean^2 / var x 6e-8 of the variance.  The
    reduction now accumulates x - x[g, 0, c] (pivot-shifted fp32 partial sums per chunk), adds and un-shifts them in fp64 and keeps fp64
    sums up to finalize (sync_batchnorm/batchnorm.py:128-145 computes the same one-pass formula on fp32 sums; batchnorm_reimpl.py:18-74 is the
    two-pass yardstick).  mean^2 / var = 1.4e6 in fp32 (the old path: ~9 % error on rstd^-2), 4e3 on bf16-representable values;
    both paths (fused finalize, stats + all-reduce-able fp64 sums + finalize) against float64 on the same values: 2e-6."""
    from michigan_amd import ops
    g = torch.Generator().manual_seed(17)
    for (n, h, w, c, groups) in ((4, 48, 40, 64, 1), (2, 31, 17, 24, 2), (2, 64, 64, 1024, 1)):
        if dt == "f32":
            x = 300.0 + 0.25 * torch.randn(n, h, w, c, generator=g)
        else:
            x = (128.0 + torch.randint(-4, 5, (n, h, w, c), generator=g).float()).to(torch.bfloat16)     # spacing 1 at 128..256: exact
        x = x.to(DT[dt]).cuda()
        xr = x.double().reshape(groups, -1, c)
        count = float(xr.shape[1])
        var = xr.var(1, unbiased=False)
        rstd_ref = (var + 1e-5).rsqrt()
        rm, rv = (torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")) if groups == 1 else (None, None)
        mean_a, rstd_a, sums_a = ops.stats_finalize(x, groups, count, 1e-5, 0.1, rm, rv)
        assert sums_a.dtype == torch.float64
        rel = ((rstd_a.double() - rstd_ref) / rstd_ref).abs().max().item()
        assert rel < 2e-6, (dt, n, h, w, c, groups, rel)
        assert ((mean_a.double() - xr.mean(1)).abs().max().item()) < 1e-4
        if groups == 1:
            unb = var[0] * count / (count - 1)
            assert ((rv.double() - (0.9 + 0.1 * unb)) / (0.9 + 0.1 * unb)).abs().max().item() < 2e-6
            mean_b, rstd_b, _, sums_b = ops.batch_stats_finish((ops.channel_sums(x, shift=True), None, count, c), 1e-5, 0.0)
            assert ((rstd_b.double() - rstd_ref[0]) / rstd_ref[0]).abs().max().item() < 2e-6
            assert torch.equal(sums_b.reshape(-1), sums_a.reshape(-1))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_stats_finalize_fused_is_bit_identical_to_the_three_launch_path(hip_backend, dt):
    """mg_channel_stats_finalize (stage 2 finalizes) == mg_channel_stats + (sums *= scale) + mg_norm_finalize, bit for bit: batch
    norm (G = 1, running statistics, the x4 upsample scale) and instance norm (G = N), vec and non-vec channel geometries."""
    from michigan_amd import ops
    from michigan_amd import _cabi as C
    g = torch.Generator().manual_seed(9)
    for (n, h, w, c, groups, scale) in ((4, 24, 20, 64, 1, 1.0), (2, 16, 16, 1024, 1, 4.0), (3, 33, 17, 128, 3, 1.0), (2, 9, 7, 24, 2, 1.0)):
        x = (torch.randn(n, h, w, c, generator=g) * 2 + 0.5).to(DT[dt]).cuda()
        count = float(x.numel() // (groups * c)) * scale
        rm0, rv0 = torch.randn(c, generator=g).cuda(), torch.rand(c, generator=g).cuda() + 0.5
        rm_a, rv_a = (rm0.clone(), rv0.clone()) if groups == 1 else (None, None)
        mean_a, rstd_a, sums_a = ops.stats_finalize(x, groups, count, 1e-5, 0.1, rm_a, rv_a, scale)
        sums_b = ops.channel_sums(x, groups=groups, shift=True)
        if scale != 1.0:
            sums_b.mul_(scale)
        mean_b = torch.empty((groups, c), device="cuda"); rstd_b = torch.empty((groups, c), device="cuda")
        rm_b, rv_b = (rm0.clone(), rv0.clone()) if groups == 1 else (None, None)
        C.backend().mg_norm_finalize(ops._p(sums_b), groups, c, count, 1e-5, 0.1, ops._p(rm_b), ops._p(rv_b), ops._p(mean_b), ops._p(rstd_b), ops._stream(x))
        torch.cuda.synchronize()
        for a, b in ((sums_a, sums_b), (mean_a, mean_b), (rstd_a, rstd_b)) + (((rm_a, rm_b), (rv_a, rv_b)) if groups == 1 else ()):
            assert torch.equal(a.reshape(-1), b.reshape(-1)), (n, h, w, c, groups)
        xr = x.float().reshape(groups, -1, c)
        _close(f"stats_finalize mean {dt}", mean_a, xr.mean(1).reshape(groups, c) , 1e-4)


@pytest.mark.parametrize("shape", [(8, 32, 32, 1024, 1024), (8, 64, 64, 1024, 512), (8, 64, 64, 128, 2048), (8, 16, 16, 1024, 1024), (8, 128, 128, 512, 256)],
                         ids=lambda s: "x%dx%d_%d_to_%d" % (s[1], s[2], s[3], s[4]))
def test_wgrad_wide_channels_match_torch_gpu(shape):
    """the bf16 3x3 weight-gradient kernel (`wgrad3x3_kernel`, kernel-row tiles, split-K with fp32 atomics) at the
    BENCHMARKED channel counts (1024 / 512 / the 2048-row fused gamma|beta image) -- its contract tests stop at 256 channels.  Same
    bf16 operands into torch's own fp32 GPU convolution weight gradient; both accumulate in fp32, so they agree to summation-order
    rounding: 2e-3 of the largest element (the bias gradient: column sums of dy, same bound)."""
    from michigan_amd import ops
    n, h, w, cin, cout = shape
    g = torch.Generator().manual_seed(11)
    x = torch.randn(n, h, w, cin, generator=g).bfloat16().cuda()
    dy = (torch.randn(n, h, w, cout, generator=g) / 8).bfloat16().cuda()
    dw, db = ops.conv_wgrad(x, dy, 3, 3, 1, 1, want_bias=True)
    got = ops.unpack_wgrad(dw, (cout, cin, 3, 3))
    ref = torch.nn.grad.conv2d_weight(x.float().permute(0, 3, 1, 2), (cout, cin, 3, 3), dy.float().permute(0, 3, 1, 2), padding=1)
    _close("wgrad3x3 vs torch gpu", got, ref, 2e-3)
    _close("bias gradient", db[:cout], dy.float().sum((0, 1, 2)), 2e-3)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_self_attention_matches_contract(hip_backend, dt):
    """mg_self_attention (flash-style QK^T -> online softmax -> PV, mg_attention.hip) vs the float64 contract softmax(q k^T) v of
    generator.py:467-485 on identical operands: the in-painting net's real geometry (4096 positions), a one-tile problem, ragged
    lengths (masked last key tile, partial query tile), peaky scores (|q . k| up to ~100: the running-max rescale fires late in the
    key loop -- one key row is planted near the END that dominates one query), operands that are column slices of one fused
    [q | k | v] projection, and the output written into the second half of a wider buffer."""
    from michigan_amd import ops
    g = torch.Generator().manual_seed(21)
    tol = 2e-5 if dt == "f32" else 2.0 ** -8           # bf16: the output's own rounding (the probabilities carry 16 mantissa bits)
    for (n, L, scale, fused) in ((2, 4096, 0.35, False), (1, 256, 1.0, False), (3, 200, 0.5, True), (1, 333, 1.5, False), (2, 64, 0.2, True)):
        q = (torch.randn(n, L, 64, generator=g) * scale).to(DT[dt])
        k = (torch.randn(n, L, 64, generator=g) * scale).to(DT[dt])
        v = torch.randn(n, L, 256, generator=g).to(DT[dt])
        k[:, L - 5] = (4.0 * q[:, 7].float()).to(DT[dt])               # query 7's maximum arrives in the last key tile

        def fn(q, k, v):
            if fused:
                qkv = torch.cat([q, k, v], dim=2).contiguous()
                q, k, v = qkv[:, :, :64], qkv[:, :, 64:128], qkv[:, :, 128:]
            buf = torch.zeros((q.shape[0], q.shape[1], 512), dtype=v.dtype, device=v.device)
            ops.self_attention(q, k, v, out=buf[:, :, 256:])
            return (buf,)
        (hip, _), (ref, _) = _both(fn, (q, k, v))
        assert torch.equal(hip[0][:, :, :256].cpu(), torch.zeros_like(ref[0][:, :, :256])), "wrote outside its half of the rows"
        _close(f"self_attention {dt} n={n} L={L}", hip[0][:, :, 256:], ref[0][:, :, 256:], tol)


def test_halo64_matches_the_shipped_halo_kernel_bitwise(hip_backend):
    """csrc/mg_conv_halo64.hip (3x3 convolutions over exactly 64 input channels: weights in registers, strips of 16x16 tiles per workgroup)
    against the kernel it replaces (OPT_CONV_HALO64 = 0: conv3x3_halo_kernel<bf16, PLAIN, 1, 2> / <2, 2>): same K order, so BITWISE equal --
    every epilogue case it takes ({no aux} x {none, relu, lrelu}, residual, ReLU mask and LeakyReLU mask of a data gradient), 64 -> 64 and
    64 -> 128, several strip splits (batch 1: eight segments per row band; batch 3: an odd number of workgroups, no XCD remap), non-square
    images, image borders on all four sides; and against the float64 contract for one case.  Shapes that the new kernel does not take
    (ragged tiles, too few tiles) must still run (on the shipped kernel)."""
    from michigan_amd import _cabi, ops
    be = hip_backend
    g = torch.Generator().manual_seed(11)

    def both(fn):
        outs = []
        for on in (1, 0):
            with _cabi.options({_cabi.OPT_CONV_HALO64: on}, be):
                outs.append(fn().clone())
        torch.cuda.synchronize()
        return outs

    launches = {"n": 0}
    orig = be.mg_conv_taps
    for n, h, w, cout in ((1, 512, 512, 64), (3, 256, 384, 64), (8, 512, 512, 64), (2, 512, 512, 128), (4, 256, 512, 64)):
        x = torch.randn(n, h, w, 64, generator=g).to(torch.bfloat16).cuda()
        wt = (torch.randn(cout, 64, 3, 3, generator=g) * 0.05).cuda()
        b = torch.randn(cout, generator=g).cuda()
        res = torch.randn(n, h, w, cout, generator=g).to(torch.bfloat16).cuda()
        with torch.no_grad():
            for act in (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LRELU):
                new, old = both(lambda: ops.conv2d_infer(x, wt, b, padding=1, act=act, slope=0.2))
                assert torch.equal(new, old), ("act", act, n, h, w, cout)
            new, old = both(lambda: ops.conv2d_infer(x, wt, None, padding=1, resid=res))
            assert torch.equal(new, old), ("resid", n, h, w, cout)
            # data gradients: dy has 64 channels, dx `cout` channels, masked by the (Leaky)ReLU output the forward conv consumed
            wd = (torch.randn(64, cout, 3, 3, generator=g) * 0.05).cuda()                 # forward weight [Cout_fwd = 64, Cin_fwd = cout]
            img = ops.pack_weight(wd, None, torch.bfloat16, ops._roundup(cout, 128), 64, 1)
            mask = torch.randn(n, h, w, cout, generator=g).to(torch.bfloat16).cuda()
            for ms in (0.0, 0.2):
                new, old = both(lambda: ops.conv_dgrad(x, img, 3, 3, 1, 1, (h, w), cout, relu_mask=mask, mask_slope=ms))
                assert torch.equal(new, old), ("mask", ms, n, h, w, cout)
            new, old = both(lambda: ops.conv_dgrad(x, img, 3, 3, 1, 1, (h, w), cout))
            assert torch.equal(new, old), ("dgrad", n, h, w, cout)
    # the new kernel really ran: its launches are shorter than the shipped kernel's on the benchmarked shape (also a smoke timing)
    x = torch.randn(8, 512, 512, 64, generator=g).to(torch.bfloat16).cuda()
    wt = (torch.randn(64, 64, 3, 3, generator=g) * 0.05).cuda()
    b = torch.zeros(64).cuda()
    times = []
    with torch.no_grad():
        for on in (1, 0):
            with _cabi.options({_cabi.OPT_CONV_HALO64: on}, be):
                for _ in range(3):
                    ops.conv2d_infer(x, wt, b, padding=1, act=ops.ACT_RELU)
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(10):
                    ops.conv2d_infer(x, wt, b, padding=1, act=ops.ACT_RELU)
                e.record(); torch.cuda.synchronize()
                times.append(s.elapsed_time(e) / 10 * 1e3)
    print("64 -> 64 @ 8x512^2 (bias + ReLU): halo64 %.1f us, shipped halo kernel %.1f us; %.2f TB/s of algorithmic traffic" % (times[0], times[1], 2 * x.numel() * 2 / times[0] / 1e6))
    assert times[0] < times[1]
    # contract check of one case against the float64 emulator
    from oracle.cabi_emulator import EmulatorBackend
    xs = torch.randn(2, 512, 512, 64, generator=g).to(torch.bfloat16)
    ws = (torch.randn(64, 64, 3, 3, generator=g) * 0.05)
    bs = torch.randn(64, generator=g)
    with torch.no_grad():
        got = ops.conv2d_infer(xs.cuda(), ws.cuda(), bs.cuda(), padding=1, act=ops.ACT_RELU).float().cpu()
    prev = _cabi.set_backend(EmulatorBackend())
    try:
        with torch.no_grad():
            want = ops.conv2d_infer(xs, ws, bs, padding=1, act=ops.ACT_RELU).float()
    finally:
        _cabi.set_backend(prev)
    assert (got - want).abs().max().item() <= 2.0 ** -8 * want.abs().max().item()
    # race screen: the kernel hands patches and auxiliary quads through LDS-DMA behind one barrier per tile -- 150 launches of a residual case on a
    # busy GPU (a second stream streams HBM beside it) must all give the first launch's bytes
    xr = torch.randn(4, 512, 512, 64, generator=g).to(torch.bfloat16).cuda()
    rr = torch.randn(4, 512, 512, 64, generator=g).to(torch.bfloat16).cuda()
    junk = torch.empty(1 << 27, dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    with torch.no_grad():
        first = ops.conv2d_infer(xr, wt, b, padding=1, resid=rr).clone()
        bad = 0
        for it in range(150):
            if it % 10 == 0:
                with torch.cuda.stream(side):
                    junk.add_(1.0)
            bad += int(not torch.equal(ops.conv2d_infer(xr, wt, b, padding=1, resid=rr), first))
    torch.cuda.synchronize()
    assert bad == 0, "%d of 150 launches differ from the first" % bad
    # not taken: ragged tiles (520 = 32.5 tiles) and a launch with too few tiles -- still correct through the shipped kernels
    with torch.no_grad():
        for n, h, w in ((2, 520, 512), (1, 128, 128)):
            x = torch.randn(n, h, w, 64, generator=g).to(torch.bfloat16).cuda()
            new, old = both(lambda: ops.conv2d_infer(x, wt, b, padding=1))
            assert torch.equal(new, old)
