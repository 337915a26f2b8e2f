"""-m gpu: the fp32 summation order of the scalar-sum kernels is the one michigan_amd/csrc/mg_reduce.h documents.

The census tests (tests/test_gpu_census.py) hold every reduction to "each element exactly once" on operands that are exact in any order;
here the operands are order-SENSITIVE (seeded normals) and a numpy model reproduces the documented order bit for bit:

    a thread's strided sequential sum  ->  the wave tree o = 32 .. 1 as lane 0 sees it  ->  the join of the wave sums, left to right.

Three entry points whose per-element terms are exact, so the model needs no kernel arithmetic:
  mg_l1_mean_fwd      b = 0: a term is |a|, the four values of a quad are added in order; `partial` bit for bit, then `out` against the
                      model's fp64 finish cast to float
  mg_orient_loss_fwd  the hair-sum row of the workspace is the model of s_hair += hv
  mg_sn_normalize     t holds 8 significant bits, so t * t is exact (contracted into an fma or not); ss is visible only through
                      dst = t / max(sqrt(ss), eps) (a correctly rounded sqrt and quotient), so dst is compared against the model's ss:
                      1024-thread stride, wave tree, left-to-right join of 16
The inputs must discriminate: for every case the model is also evaluated with the pairwise join and as one plain left-to-right sum over
all elements, and at least one of the two has to differ in bits from the documented order (checked before the kernel's result is looked at).

The fp64 halving trees are NOT pinned here: an order change in fp64 over at most 1024 fp32 partials almost never survives the cast to
float.  They are held by mg_grad_drain's double output (tests/test_gpu_census.py) and by comparing every output before against after a
change of these kernels.  The pairwise join of mg_feat_moments.hip is held by the style-loss tests.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32 = np.float32
OL_BLOCKS = 1024                   # row stride of mg_orient_loss_fwd's workspace: OL_BLOCKS in michigan_amd/csrc/mg_glue.hip


@pytest.fixture
def backend(hip_backend):
    """Always the GPU library: the contract emulator has no summation order to hold."""
    return hip_backend


def seq_sum(x):
    """Sequential fp32 sum along the last axis, starting from +0."""
    return np.add.accumulate(x.astype(F32), axis=-1, dtype=F32)[..., -1]


def by_thread(vals, grid, nt):
    """vals [items, per] -> [grid, nt, trips * per]: what thread t of workgroup b adds, in its order (item i belongs to thread i % (grid * nt);
    a trip past the end adds +0, which changes no bit of a sum that started at +0)."""
    n, per = vals.shape
    trips = -(-n // (grid * nt))
    pad = np.zeros((trips * grid * nt, per), F32)
    pad[:n] = vals
    return pad.reshape(trips, grid, nt, per).transpose(1, 2, 0, 3).reshape(grid, nt, trips * per)


def wave_tree(v):
    """[..., 64 * nw] thread sums -> [..., nw]: lane 0 of v[l] += v[l ^ o], o = 32 .. 1 (lane l < o only ever needs lanes below 2 o)."""
    v = v.reshape(v.shape[:-1] + (-1, 64)).copy()
    for o in (32, 16, 8, 4, 2, 1):
        v[..., :o] = v[..., :o] + v[..., o:2 * o]
    return v[..., 0]


def join(w, pairwise=False):
    if not pairwise:
        return seq_sum(w)
    while w.shape[-1] > 1:
        w = w[..., 0::2] + w[..., 1::2]
    return w[..., 0]


def model(vals, grid, nt):
    """Per-workgroup sums in the documented order, and the two orders it must be told apart from."""
    th = by_thread(vals, grid, nt)
    waves = wave_tree(seq_sum(th))
    plain = seq_sum(th.reshape(grid, nt, -1, vals.shape[1]).transpose(0, 2, 1, 3).reshape(grid, -1))     # in element order
    return join(waves), join(waves, pairwise=True), plain


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def _grid(items, cap=1024):
    return min(-(-items // 256), cap)


def _normals(seed, shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(F32)


def l1_model(a_f32):
    """a_f32: the operand as fp32 values, [nquads, 4]."""
    nq = a_f32.shape[0]
    grid = _grid(nq)
    doc, pair, plain = model(np.abs(a_f32), grid, 256)
    s = np.zeros(256, np.float64)
    for i0 in range(0, grid, 256):                       # thread t adds partial[t], partial[t + 256], ... in double
        p = doc[i0:i0 + 256].astype(np.float64)
        s[:p.size] += p
    for o in (128, 64, 32, 16, 8, 4, 2, 1):
        s[:o] += s[o:2 * o]
    return doc, pair, plain, F32(s[0] * (1.0 / (4.0 * nq)))


def l1_operand(dt, nq):
    a = torch.from_numpy(_normals(100 + nq, (nq, 4)))
    return a.to(torch.bfloat16) if dt == "bf16" else a


def orient_operands(N, H, W):
    rng = np.random.default_rng(200 + H)
    HW = H * W
    return {"conf": rng.standard_normal((N, HW)).astype(F32), "idx": rng.integers(0, 32, (N, HW)).astype(np.uint8),
            "label": rng.uniform(-1, 1, (N, 2, HW)).astype(F32), "hair": rng.standard_normal((N, HW)).astype(F32)}


def sn_operand(n):
    return torch.from_numpy(_normals(300 + n, (n,))).to(torch.bfloat16).float().numpy()      # 8 significant bits: t * t is exact


def sn_model(t, eps):
    out = []
    for ss in model((t * t).reshape(-1, 1), 1, 1024):
        out.append(t / np.maximum(np.sqrt(ss[0], dtype=F32), F32(eps)))
    return out


L1_Q, ORIENT_HW, SN_N, SN_EPS = (257, 65537), ((17, 16), (67, 35)), (1025, 4489), 1e-12


def discriminates(doc, pair, plain):
    return not same(doc, pair) or not same(doc, plain)


@pytest.mark.parametrize("nq", L1_Q)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_l1_mean_adds_in_the_documented_order(backend, dt, nq):
    from michigan_amd import _cabi, ops
    a = l1_operand(dt, nq)
    doc, pair, plain, want_out = l1_model(a.float().numpy())
    assert discriminates(doc, pair, plain)
    a = a.cuda()
    b = torch.zeros_like(a)
    out, partial = torch.empty(1, dtype=torch.float32, device="cuda"), torch.zeros(1024, dtype=torch.float32, device="cuda")
    _cabi.backend().mg_l1_mean_fwd(ops._p(a), ops._p(b), ops._dt(a), a.numel(), ops._p(out), ops._p(partial), ops._stream(a))
    got = partial.cpu().numpy()[:doc.size]
    assert same(got, doc), f"l1 partial {dt} nq={nq}: {int((bits(got) != bits(doc)).sum())} of {doc.size} workgroup sums differ from the documented order"
    assert same(out.cpu().numpy(), want_out), (out.item(), float(want_out))


@pytest.mark.parametrize("H,W", ORIENT_HW)
def test_orient_loss_hair_sum_adds_in_the_documented_order(backend, H, W):
    from michigan_amd import _cabi, ops
    N, HW = 3, H * W
    o = orient_operands(N, H, W)
    grid = _grid(N * HW, OL_BLOCKS)
    doc, pair, plain = model(o["hair"].reshape(-1, 1), grid, 256)
    assert discriminates(doc, pair, plain)
    d = {k: torch.from_numpy(v).cuda() for k, v in o.items()}
    out, ws = torch.empty(3, dtype=torch.float32, device="cuda"), torch.zeros(3 * OL_BLOCKS, dtype=torch.float32, device="cuda")
    _cabi.backend().mg_orient_loss_fwd(ops._p(d["conf"]), ops._p(d["idx"]), ops._p(d["label"]), 2, 2 * HW, ops._p(d["hair"]), HW, N, HW,
                                       ops._p(out), ops._p(ws), ops._stream(d["conf"]))
    got = ws.cpu().numpy()[2 * OL_BLOCKS:2 * OL_BLOCKS + grid]
    assert same(got, doc), f"orient hair row {H}x{W}: {int((bits(got) != bits(doc)).sum())} of {grid} workgroup sums differ from the documented order"


@pytest.mark.parametrize("n", SN_N)
def test_sn_normalize_adds_in_the_documented_order(backend, n):
    from michigan_amd import _cabi, ops
    t = sn_operand(n)
    doc, pair, plain = sn_model(t, SN_EPS)
    assert discriminates(doc, pair, plain)
    td = torch.from_numpy(t).cuda()
    dst = torch.empty_like(td)
    _cabi.backend().mg_sn_normalize(ops._p(td), n, SN_EPS, ops._p(dst), None, None, ops._stream(td))
    got = dst.cpu().numpy()
    assert same(got, doc), f"sn_normalize n={n}: {int((bits(got) != bits(doc)).sum())} of {n} quotients differ from the documented order's"
