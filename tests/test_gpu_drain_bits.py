"""-m gpu: mg_grad_drain (GEMM-order gradient arena -> reference-layout gradients) held to its arithmetic.

For a slot without spectral norm the drain is a permutation and ONE fp32 add per element (dst[co][ci][t] += g), so the result must be
``torch.equal`` to ``dst + g`` un-permuted, the bias rows likewise, and the GEMM image must be all zeros afterwards: no tolerance.
For a spectral-normed slot dst += (g - s u[co] v[ci, t]) / sigma with s = sum(g * W_sn): compared with the float64 formula, and two
runs must agree bit for bit (s is a fixed-order sum: the ranks of a data-parallel job have to get the same bits).

Tolerance of the spectral-normed slot: the kernel rounds s to fp32, forms su = s * u, then (g - su * v) * (1 / sigma) and the add,
five roundings of at most 2^-24 relative each on terms no larger than |g| + |s u v| / sigma + |dst|; the sum s itself (8640 products
in fp32 groups of at most four, then double) adds below 2^-23 of sum|g w|.  With the operands below every term is O(1..4) against a
largest result of about 4, so 1e-6 of the largest |reference| leaves a factor of two over that bound.

All slots go through ONE launch: plain 3x3, swapped roles (16-byte and 4-byte rows), the SPADE pair with its bias rows, T = 1 / 16 /
49, a 3-channel layer (runs of 27 floats: 4-byte accesses) and the spectral-normed one.
MG_TEST_DRYRUN=1 runs the contract emulator in place of the GPU (plumbing check on a machine without one).
"""
import ctypes
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DRY = os.environ.get("MG_TEST_DRYRUN") == "1"
DEV = "cpu" if DRY else "cuda"

# name, cout, cin, taps, rows, cols, swapped, two tensors, bias rows, spectral norm
SLOTS = [
    ("plain 3x3", 40, 24, 9, 64, 24, 0, False, True, False),
    ("swapped roles", 24, 8, 9, 24, 8, 1, False, False, False),
    ("swapped roles, odd rows", 22, 8, 9, 27, 8, 1, False, False, False),
    ("SPADE pair", 72, 136, 9, 256, 136, 0, True, True, False),
    ("1x1", 72, 40, 1, 128, 40, 0, False, False, False),
    ("4x4", 16, 72, 16, 64, 72, 0, False, True, False),
    ("7x7", 24, 8, 49, 64, 8, 0, False, True, False),
    ("3 input channels", 24, 3, 9, 64, 8, 0, False, False, False),
    ("spectral-normed", 40, 24, 9, 64, 24, 0, False, True, True),
]


@pytest.fixture
def backend(request):
    return request.getfixturevalue("emulator_backend" if DRY else "hip_backend")


def _gemm_rows(cout, two):
    co = torch.arange(cout)
    return 64 * (co // 32) + co % 32 if two else co


def _make(gen):
    """Per slot: the GEMM image (zero where a weight-gradient kernel writes nothing), bias rows, preset destinations."""
    data = []
    for name, cout, cin, T, rows, cols, swapped, two, bias, sn in SLOTS:
        r = _gemm_rows(cout, two)
        g = [torch.randn(cout, cin, T, generator=gen) for _ in range(2 if two else 1)]          # reference layout
        img = torch.zeros(T, rows, cols)
        for which, gw in enumerate(g):
            img[:, r + 32 * which, :cin] = gw.permute(2, 0, 1)
        if swapped:
            img = img.permute(0, 2, 1).contiguous()                                            # [T][cols][rows]
        db = torch.zeros(rows)
        gb = [torch.randn(cout, generator=gen) for _ in g]
        for which, b in enumerate(gb):
            db[r + 32 * which] = b
        dst = [torch.randn(cout, cin, T, generator=gen) for _ in g]
        dbias = [torch.randn(cout, generator=gen) for _ in g]
        extra = None
        if sn:
            u = torch.nn.functional.normalize(torch.randn(cout, generator=gen), dim=0)
            v = torch.nn.functional.normalize(torch.randn(cin * T, generator=gen), dim=0)
            extra = (0.05 * torch.randn(cout, cin, T, generator=gen), u, v, torch.tensor([1.3]))
        data.append(dict(g=g, img=img, db=db if bias else None, gb=gb, dst=dst, dbias=dbias, sn=extra))
    return data


def _run(data):
    """One mg_grad_drain launch over fresh device copies; returns per slot (destinations, bias destinations, image, bias rows)."""
    from michigan_amd import _cabi as C, ops

    be = C.backend()
    dev = [dict(img=d["img"].clone().to(DEV), db=None if d["db"] is None else d["db"].clone().to(DEV),
                dst=[t.clone().to(DEV) for t in d["dst"]], dbias=[t.clone().to(DEV) for t in d["dbias"]],
                sn=None if d["sn"] is None else [t.clone().to(DEV) for t in d["sn"]]) for d in data]
    counts = [int(be.mg_grad_slot_blocks(cout, cin, 2 if two else 1)) for _, cout, cin, _, _, _, _, two, _, _ in SLOTS]
    assert all(c > 0 for c in counts)
    nblk = sum(counts)
    sdot = torch.zeros(1 + nblk, dtype=torch.float64, device=DEV)
    table = ops.DeviceTable(C.GradSlot, len(SLOTS), DEV)
    first = 0
    for e, (name, cout, cin, T, rows, cols, swapped, two, bias, sn), d, nb in zip(table.begin_update(), SLOTS, dev, counts):
        e.gemm = d["img"].data_ptr()
        e.dbias_gemm = d["db"].data_ptr() if bias else None
        e.dst0, e.dst1 = d["dst"][0].data_ptr(), (d["dst"][1].data_ptr() if two else None)
        e.dbias0 = d["dbias"][0].data_ptr() if bias else None
        e.dbias1 = d["dbias"][1].data_ptr() if bias and two else None
        if sn:
            w_sn, u, v, sigma = d["sn"]
            e.w_sn, e.u, e.v, e.sigma, e.s = w_sn.data_ptr(), u.data_ptr(), v.data_ptr(), sigma.data_ptr(), sdot.data_ptr()
        else:
            e.w_sn = e.u = e.v = e.sigma = e.s = None
        e.cout, e.cin, e.taps, e.rows, e.cols, e.swapped = cout, cin, T, rows, cols, swapped
        e.first_block = first
        first += nb
    bmap = ops.block_map(counts, DEV)
    be.mg_grad_drain(table.upload(), len(SLOTS), ops._p(bmap), nblk, ctypes.c_void_p(sdot.data_ptr() + 8), ops._stream(bmap))
    return [dict(dst=[t.cpu() for t in d["dst"]], dbias=[t.cpu() for t in d["dbias"]], img=d["img"].cpu(),
                 db=None if d["db"] is None else d["db"].cpu()) for d in dev]


def test_drain_is_one_add_per_element_and_a_fixed_order_dot(backend):
    data = _make(torch.Generator().manual_seed(17))
    got, again = _run(data), _run(data)
    failures = []
    for (name, cout, cin, T, rows, cols, swapped, two, bias, sn), d, o, o2 in zip(SLOTS, data, got, again):
        if not bool((o["img"] == 0).all()):
            failures.append(f"{name}: {int((o['img'] != 0).sum())} elements of the GEMM image were not re-zeroed")
        if bias:
            if not bool((o["db"] == 0).all()):
                failures.append(f"{name}: the bias rows were not re-zeroed")
            for which in range(2 if two else 1):
                if not torch.equal(o["dbias"][which], d["dbias"][which] + d["gb"][which]):
                    failures.append(f"{name}: bias gradient {which} is not dbias + g")
        for which in range(2 if two else 1):
            if not torch.equal(o["dst"][which], o2["dst"][which]):
                failures.append(f"{name}: two runs differ in tensor {which}")
            if not sn:
                want = d["dst"][which] + d["g"][which]                       # one fp32 add
                if not torch.equal(o["dst"][which], want):
                    bad = (o["dst"][which] != want).nonzero()
                    failures.append(f"{name}: tensor {which}: {bad.shape[0]} elements are not dst + g, first at (co, ci, t) = {bad[0].tolist()}")
            else:
                w_sn, u, v, sigma = (t.double() for t in d["sn"])
                g64 = d["g"][which].double()
                s = (g64 * w_sn).sum()
                want = d["dst"][which].double() + (g64 - s * u[:, None, None] * v.view(1, cin, T)) / sigma
                err = float((o["dst"][which].double() - want).abs().max() / want.abs().max())
                print(f"{name}: max |got - float64| / max |float64| = {err:.3e}")
                if not err <= 1e-6:
                    failures.append(f"{name}: {err:.3e} of the largest reference value, over 1e-6")
    assert not failures, "\n".join(failures)
