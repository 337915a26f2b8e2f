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

The per-channel (column) sums of mg_norm.hip follow the header's second order:

    thread row tr adds pixels p0 + tr, p0 + tr + rows, ... of its chunk sequentially from +0  ->  rows are added in ascending order.

The fp32 `partial` workspace [G][chunk][2][C] is held to that model bit for bit; stat_geom() below mirrors StatGeom / vec_geom_ok of
michigan_amd/csrc/mg_norm.hip (chunking; thread rows of the channel-resident "vec" and of the quad kernels).  Exact per-element terms again:
  mg_channel_stats       shift = 0: x and x * x; x holds <= 12 significant bits (fp32) or is bf16, so the square is exact, fma or not
  mg_norm_bwd_reduce     mean = 0, rstd = 1, act none, no h / g1 / dgb: dh and dh * x; at both values of OPT_NORM_BWD_VEC on a vec-capable
                         geometry.  The two kernels give the same bits where their thread rows are as many (fp32: VEC = 4 is the quad);
                         bf16 C = 32 has 64 vec rows against 32 quad rows, two different orders, and each is held to its own model
  mg_norm_bwd_reduce_up  the same with x the half-resolution source, read at (y >> 1, x >> 1)
Operands: seeded normals x 2^k, k uniform in -8 .. 8 per element (without the exponent spread as few as 1 of 32 columns tells the orders
apart).  Discrimination is checked first: per half of `partial`, at least a quarter of the entries must differ in bits from the chunk summed
in plain pixel order (where rows > 1) and from a pairwise tree over the chunk's pixels.  COLUMN_CASES have 3, 5, 3, 3 chunks and the _up
case 4, each with a ragged last row trip.  The fp64 finish: `sums` equals the float64 sum of `partial` over the chunks (plus the un-shift,
0 here), which is exact in any order for operands this narrow.

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


# =====================================================================================================================
# column sums (mg_norm.hip): the row join of mg_reduce.h
# =====================================================================================================================
def stat_geom(dt, G, P, C):
    """StatGeom stat_geom(G, P, C) and vec_geom_ok<T>(C) of michigan_amd/csrc/mg_norm.hip: (chunk, nchunks, quad rows, vec rows or None)."""
    tpr = min(C // 4, 256)
    rpb = 256 // tpr
    want = max(min(-(-1536 // G), -(-P // (rpb * 16)), 512), 1)
    chunk = -(-P // want)
    vec = 8 if dt == "bf16" else 4
    cv = C // vec
    vec_rows = 256 // cv if C % vec == 0 and cv <= 256 and 256 % cv == 0 else None
    return chunk, -(-P // chunk), rpb, vec_rows


def column_operand(seed, shape, dt):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(shape) * np.exp2(rng.integers(-8, 9, shape))
    if dt == "bf16":
        return torch.from_numpy(v.astype(F32)).to(torch.bfloat16)
    m, e = np.frexp(v)
    return torch.from_numpy(np.ldexp(np.round(m * 4096.0) / 4096.0, e).astype(F32))          # 12 significant bits


def pairwise_rows(t):
    """[n, ...] -> the pairwise tree over axis 0 (an odd level is padded with +0)."""
    while t.shape[0] > 1:
        if t.shape[0] & 1:
            t = np.concatenate([t, np.zeros_like(t[:1])])
        t = t[0::2] + t[1::2]
    return t[0]


def column_model(terms, chunk, rows):
    """terms [G, P, C] fp32 (exact per-element terms) -> (documented, plain pixel order, pairwise), each [G, nchunks, C]."""
    G, P, C = terms.shape
    out = []
    for g in range(G):
        per = []
        for p0 in range(0, P, chunk):
            t = terms[g, p0:p0 + chunk]
            trips = -(-t.shape[0] // rows)
            pad = np.zeros((trips * rows, C), F32)
            pad[:t.shape[0]] = t                                             # a row's missing last trip adds +0: no bit changes
            own = seq_sum(pad.reshape(trips, rows, C).transpose(1, 2, 0))     # [rows, C]: row tr adds p0 + tr, p0 + tr + rows, ...
            per.append((seq_sum(own.T), seq_sum(t.T), pairwise_rows(t)))
        out.append([np.stack(z) for z in zip(*per)])
    return [np.stack(z) for z in zip(*out)]


def check_discriminates(tag, doc, plain, pair, rows):
    for name, alt in (("plain pixel order", plain), ("pairwise tree", pair)):
        if name == "plain pixel order" and rows == 1:
            continue                                                        # one thread row adds in pixel order
        differ = int((bits(doc) != bits(alt)).sum())
        if 4 * differ < doc.size:
            raise RuntimeError(f"{tag}: only {differ} of {doc.size} entries tell the documented order from the {name}")


def column_case(tag, dt, x, dh, chunk, nchunks, rows_list, run, x_terms=None):
    """run(i) -> (partial [G, nchunks, 2, C] fp32, sums [G, 2, C]) for rows_list[i]; dh None: the statistics terms x, x * x."""
    xf = (x if x_terms is None else x_terms).float().numpy()
    halves = (xf, xf * xf) if dh is None else (dh.float().numpy(), dh.float().numpy() * xf)
    models = {}
    for rows in set(rows_list):
        models[rows] = [column_model(h, chunk, rows) for h in halves]
        for name, (doc, plain, pair) in zip(("sum", "sum of products"), models[rows]):
            assert doc.shape[1] == nchunks
            check_discriminates(f"{tag} rows={rows} {name}", doc, plain, pair, rows)
    got = []
    for i, rows in enumerate(rows_list):
        partial, sums = run(i)
        partial, sums = partial.cpu().numpy(), sums.cpu().numpy()
        for k, name in enumerate(("sum", "sum of products")):
            doc = models[rows][k][0]
            differ = int((bits(partial[:, :, k]) != bits(doc)).sum())
            print(f"[order] {tag} rows={rows} {name}: {differ} of {doc.size} partial sums differ from the documented order")
            assert differ == 0, f"{tag} rows={rows} {name}: {differ} of {doc.size} partial sums differ from the documented order"
        want = np.add.accumulate(partial.astype(np.float64), axis=1)[:, -1]          # [G, 2, C]: exact for these operands
        assert np.array_equal(sums, want.astype(sums.dtype)), f"{tag} rows={rows}: sums is not the float64 sum of partial"
        got.append(partial)
    for i in range(1, len(got)):
        if rows_list[i] == rows_list[0]:
            assert same(got[i], got[0]), f"{tag}: the two kernels differ in bits at equal thread rows"


# (dtype, C, G, P): vec cv 8 rows 32 | vec cv 4 rows 64 | quad tpr 6 rpb 42 | quad tpr 256, two channel trips, rows 1
COLUMN_CASES = [("f32", 32, 2, 1500), ("bf16", 32, 1, 2100), ("f32", 24, 1, 1400), ("f32", 1032, 1, 40)]
COLUMN_ROWS = {("f32", 32): (32, 32), ("bf16", 32): (32, 64), ("f32", 24): (42, None), ("f32", 1032): (1, None)}      # (quad, vec)


def _geom(dt, G, P, C, be):
    chunk, nchunks, rpb, vec_rows = stat_geom(dt, G, P, C)
    assert (rpb, vec_rows) == COLUMN_ROWS[(dt, C)] and nchunks >= 3, (chunk, nchunks, rpb, vec_rows)
    assert all(chunk % r for r in (rpb, vec_rows) if r and r > 1), "no ragged last row trip"
    assert int(be.mg_stats_workspace(G, P, C)) == G * nchunks * 2 * C * 4, "stat_geom() here no longer mirrors mg_norm.hip"
    return chunk, nchunks, rpb, vec_rows


@pytest.mark.parametrize("dt,C,G,P", COLUMN_CASES)
def test_channel_stats_add_in_the_documented_order(backend, dt, C, G, P):
    from michigan_amd import ops
    chunk, nchunks, rpb, vec_rows = _geom(dt, G, P, C, backend)
    x = column_operand(400 + C + P, (G, P, C), dt)
    xd = x.cuda()

    def run(i):
        partial = torch.full((G, nchunks, 2, C), float("nan"), dtype=torch.float32, device="cuda")
        sums = torch.empty((G, 2, C), dtype=torch.float64, device="cuda")
        backend.mg_channel_stats(ops._p(xd), ops._dt(xd), G, P, C, 0, ops._p(sums), ops._p(partial), ops._stream(xd))
        return partial, sums
    column_case(f"stats {dt} C={C} G={G} P={P}", dt, x, None, chunk, nchunks, [vec_rows or rpb], run)


def _bwd_reduce_case(backend, tag, dt, C, G, P, up=None):
    from michigan_amd import _cabi, ops
    chunk, nchunks, rpb, vec_rows = _geom(dt, G, P, C, backend)
    dh = column_operand(500 + C + P, (G, P, C), dt)
    if up is None:
        x = x_full = column_operand(600 + C + P, (G, P, C), dt)
    else:
        n, hh, ww = up
        x = column_operand(600 + C + P, (n, hh // 2, ww // 2, C), dt)
        yy, xx = np.arange(hh) >> 1, np.arange(ww) >> 1
        x_full = x[:, yy][:, :, xx].reshape(1, P, C)                         # what pixel (y, x) reads: the source at (y >> 1, x >> 1)
    dhd, xd = dh.cuda(), x.cuda()
    mean, rstd = torch.zeros((G, C), dtype=torch.float32, device="cuda"), torch.ones((G, C), dtype=torch.float32, device="cuda")
    variants = [(0, rpb)] + ([(1, vec_rows)] if vec_rows else [])             # (OPT_NORM_BWD_VEC, thread rows of the kernel it selects)

    def run(i):
        partial = torch.full((G, nchunks, 2, C), float("nan"), dtype=torch.float32, device="cuda")
        sums = torch.empty((G, 2, C), dtype=torch.float32, device="cuda")
        with _cabi.options({_cabi.OPT_NORM_BWD_VEC: variants[i][0]}):
            if up is None:
                backend.mg_norm_bwd_reduce(ops._p(dhd), None, ops._p(xd), None, ops._dt(xd), G, P, C, ops._p(mean), ops._p(rstd), 0, 0.0,
                                           None, ops._p(sums), ops._p(partial), ops._stream(xd))
            else:
                backend.mg_norm_bwd_reduce_up(ops._p(dhd), None, ops._p(xd), None, ops._dt(xd), up[0], up[1], up[2], C, ops._p(mean), ops._p(rstd), 0, 0.0,
                                              None, ops._p(sums), ops._p(partial), ops._stream(xd))
        return partial, sums
    column_case(tag, dt, x, dh, chunk, nchunks, [r for _, r in variants], run, x_terms=x_full)


@pytest.mark.parametrize("dt,C,G,P", COLUMN_CASES)
def test_norm_bwd_reduce_adds_in_the_documented_order(backend, dt, C, G, P):
    _bwd_reduce_case(backend, f"bwd reduce {dt} C={C} G={G} P={P}", dt, C, G, P)


def test_norm_bwd_reduce_up_adds_in_the_documented_order(backend):
    _bwd_reduce_case(backend, "bwd reduce up f32 C=32 1x40x40", "f32", 32, 1, 1600, up=(1, 40, 40))
