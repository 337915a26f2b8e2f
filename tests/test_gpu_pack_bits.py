"""-m gpu: the batched GEMM-image launch (mg_pack_weights) against the per-image mg_pack_weight, bit for bit.

The batched kernel is data movement (permute + zero-pad + cast + gamma|beta row interleave) plus, where a spectral-norm sigma is
given, one true division per element; the per-image kernel gathers by destination index and is the yardstick.  So every image of ONE
batched launch must be ``torch.equal`` to ``mg_pack_weight`` of the torch-divided tensor: there is no tolerance in this file.

The layers cover every path of the tile code: windows 1x1 / 3x3 / 4x4 / 7x7 (the wide T = 1 tile, the T <= 16 tile, the 7x7 sub-tiles),
images narrower and wider than one 128-column tile, rows and columns that are no multiple of the tile, the SPADE pair (two tensors,
[32 gamma | 32 beta] row blocks), and a 3-channel layer whose rows of 27 floats take the 4-byte loads.  rows_p / cols_p are what ops asks
for; further images have spare padding columns, or a column count that is no multiple of eight at a start aligned to one column pair
only (column-pair stores).  Mode 2 (W / sigma in the reference layout) lands 4 bytes past a 16-byte boundary, as inside SpectralPlan's buffer, and on one.
Every destination lies in a sentinel-filled buffer whose sentinels must survive.
MG_TEST_DRYRUN=1 runs the contract emulator in place of the GPU (plumbing check on a machine without one).
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DRY = os.environ.get("MG_TEST_DRYRUN") == "1"
DEV = "cpu" if DRY else "cuda"
SENTINEL = -1024.0                       # exact in bf16; no weight or quotient comes near it
GUARD = 64                               # elements on either side of a destination (a multiple of 16 bytes in both dtypes)

# (cout, cin, k, two tensors)
LAYERS = [(40, 24, 3, False), (72, 136, 3, True), (16, 72, 4, False), (24, 8, 7, False), (72, 40, 1, False), (24, 3, 3, False)]


@pytest.fixture
def backend(request):
    return request.getfixturevalue("emulator_backend" if DRY else "hip_backend")


def _r(v, m):
    return (v + m - 1) // m * m


def _geometry(cout, cin, two, mode):
    """rows_p, cols_p as ops.conv2d / conv_dgrad / spade_modulate ask for them (channels of an activation are padded to 8)."""
    gemm_rows = 2 * _r(cout, 32) if two else cout
    if mode == 0:
        return _r(gemm_rows, 128), _r(cin, 8)
    return _r(_r(cin, 8), 128), gemm_rows if two else _r(cout, 8)


def test_batched_pack_equals_per_image_pack(backend):
    from michigan_amd import _cabi as C, ops

    be = C.backend()
    g = torch.Generator().manual_seed(31)
    sigma = torch.tensor([1.7], dtype=torch.float32, device=DEV)
    jobs = []                            # (name, w0, w1, sigma or None, dtype, rows_p, cols_p, mode, offset of the image in its buffer)
    for cout, cin, k, two in LAYERS:
        w0 = torch.randn(cout, cin, k, k, generator=g).to(DEV)
        w1 = torch.randn(cout, cin, k, k, generator=g).to(DEV) if two else None
        for mode in (0, 1):
            rows_p, cols_p = _geometry(cout, cin, two, mode)
            for dtype in (torch.bfloat16, torch.float32):
                for sg in (None, sigma):
                    jobs.append((f"{cout}x{cin}x{k}x{k} mode {mode} {dtype} sigma {sg is not None}", w0, w1, sg, dtype, rows_p, cols_p, mode, GUARD))
        # spare padding columns (16-byte stores), then a width that is no multiple of 8 at a start aligned to a column pair only
        rows_p, cols_p = _geometry(cout, cin, two, 0)
        jobs.append((f"{cout}x{cin}x{k}x{k} spare columns", w0, w1, sigma, torch.bfloat16, rows_p, cols_p + 72, 0, GUARD))
        jobs.append((f"{cout}x{cin}x{k}x{k} ragged columns", w0, w1, None, torch.bfloat16, rows_p, cols_p + 2, 0, GUARD + 2))
        rows_p, cols_p = _geometry(cout, cin, two, 1)
        jobs.append((f"{cout}x{cin}x{k}x{k} mode 1 ragged columns", w0, w1, sigma, torch.float32, rows_p + 3, cols_p + 6, 1, GUARD + 2))
    copies = []                          # mode 2: (name, w, sigma or None, offset)
    for cout, cin, k, two in LAYERS:
        w = torch.randn(cout, cin, k, k, generator=g).to(DEV)
        copies.append((f"{cout}x{cin}x{k}x{k} mode 2, 4 bytes past a 16-byte boundary", w, sigma, GUARD + 1))
    copies.append(("mode 2 aligned", copies[0][1], sigma, GUARD))
    copies.append(("mode 2 without sigma", copies[1][1], None, GUARD + 1))

    table = ops.DeviceTable(C.PackJob, len(jobs) + len(copies), DEV)
    rows = table.begin_update()
    counts, bufs, first = [], [], 0
    for row, (name, w0, w1, sg, dtype, rows_p, cols_p, mode, off) in zip(rows, jobs):
        taps = w0.shape[2] * w0.shape[3]
        n = taps * rows_p * cols_p
        buf = torch.full((off + n + GUARD,), SENTINEL, dtype=dtype, device=DEV)
        assert buf.data_ptr() % 16 == 0
        dst = buf[off:off + n]
        nb = int(be.mg_pack_job_blocks(mode, w0.shape[0], w0.shape[1], taps, rows_p, cols_p))
        assert nb > 0, name
        row.w0, row.w1, row.dst, row.sigma = w0.data_ptr(), (w1.data_ptr() if w1 is not None else None), dst.data_ptr(), (sg.data_ptr() if sg is not None else None)
        row.dtype = ops._dtype_code(dtype)
        row.cout, row.cin, row.taps = w0.shape[0], w0.shape[1], taps
        row.rows_p, row.cols_p, row.mode, row.first_block = rows_p, cols_p, mode, first
        counts.append(nb)
        first += nb
        bufs.append(buf)
    for row, (name, w, sg, off) in zip(rows[len(jobs):], copies):
        n = w.numel()
        buf = torch.full((off + n + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
        assert buf.data_ptr() % 16 == 0
        nb = int(be.mg_pack_job_blocks(2, w.shape[0], w.shape[1], w.shape[2] * w.shape[3], 0, 0))
        assert nb > 0, name
        row.w0, row.w1, row.dst, row.sigma = w.data_ptr(), None, buf[off:].data_ptr(), (sg.data_ptr() if sg is not None else None)
        row.dtype = C.MG_F32
        row.cout, row.cin, row.taps = w.shape[0], w.shape[1], w.shape[2] * w.shape[3]
        row.rows_p, row.cols_p, row.mode, row.first_block = 0, 0, 2, first
        counts.append(nb)
        first += nb
        bufs.append(buf)
    bmap = ops.block_map(counts, DEV)
    be.mg_pack_weights(table.upload(), len(counts), ops._p(bmap), first, ops._stream(bmap))

    failures = []
    for (name, w0, w1, sg, dtype, rows_p, cols_p, mode, off), buf in zip(jobs, bufs):
        taps = w0.shape[2] * w0.shape[3]
        n = taps * rows_p * cols_p
        d0 = w0 / sg if sg is not None else w0
        d1 = None if w1 is None else (w1 / sg if sg is not None else w1)
        want = ops._pack_weight(d0, d1, dtype, rows_p, cols_p, mode)          # the per-image kernel
        if not torch.equal(buf[off:off + n].view(taps, rows_p, cols_p), want):
            bad = (buf[off:off + n].view(taps, rows_p, cols_p).float() != want.float()).nonzero()
            failures.append(f"{name}: {bad.shape[0]} of {n} elements differ, first at (t, r, c) = {bad[0].tolist()}")
        if not (bool((buf[:off] == SENTINEL).all()) and bool((buf[off + n:] == SENTINEL).all())):
            failures.append(f"{name}: a sentinel around the image was overwritten")
    for (name, w, sg, off), buf in zip(copies, bufs[len(jobs):]):
        n = w.numel()
        want = (w / sg if sg is not None else w).reshape(-1)
        if not torch.equal(buf[off:off + n], want):
            failures.append(f"{name}: {(buf[off:off + n] != want).sum().item()} of {n} elements differ")
        if not (bool((buf[:off] == SENTINEL).all()) and bool((buf[off + n:] == SENTINEL).all())):
            failures.append(f"{name}: a sentinel around the copy was overwritten")
    assert not failures, "\n".join(failures)
