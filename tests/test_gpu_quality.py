"""-m gpu: the quality extension group on the kernels of mg_quality.hip, and the evaluation driver on the device.

  image quality   the case table of tests/quality_fixtures.py: (H, W) on the edges of the 16 x 16 tile and of the valid region at k = 11
                  -- (11,11), (11,43), (12,27), (26,26), (27,37), (43,11), (64,64): valid regions of 1, 2, 16, 17, 27, 33 and 54 -- N and
                  C in {1, 3}, random / bright low-variance / smooth-plus-noise / constant pairs under a mask, two cases without one,
                  k = 3 and k = 15 once each, the empty mask, and one case through strided and offset views.
                  EXACT (torch.equal): the squared errors and every count against the int64 contract; identical images give
                  ssim_sum == count bit for bit, masked and not; two runs of every case are bit-identical.
                  BOUNDED: |ssim_sum - contract| <= 1e-9 * count, the bound derived in tests/quality_fixtures.py.
  orientation     the cases of quality_fixtures.orient_cases(): ragged planes (bytes), planes that take 16 bytes a lane, more than one
                  chunk, a == b and the pair (0, 255) giving 0, the empty mask: torch.equal, two runs bit-identical.
  guard bands     each entry point at its smallest and at one ragged shape inside the guard bands of tests/guard_alloc.py: inputs
                  placed, outputs and workspace allocated by the operator layer under the guard, every guard byte checked.
  the driver      evaluate (protocol reconstruct) on the tiny dataset at crop 64 with a small generator: finite rows, equal to
                  metrics.* called by hand on what inference.generate returns for the same seed.
With MG_TEST_DRYRUN=1 the same cases run on the CPU against `QualityEmulator` (a plumbing check without a GPU)."""
import math
import random

import numpy as np
import pytest
import torch

import dataset_fixtures as DF
import guard_alloc as GA
import quality_fixtures as QF
import test_gpu_guard_bands as GB

pytestmark = pytest.mark.gpu

DEV = "cpu" if GB.DRY else "cuda"
CASES = QF.quality_cases()
ORIENT = QF.orient_cases()
_REFERENCE = {}


def reference(name):
    """the contract of a case, computed once and shared"""
    if name not in _REFERENCE:
        a, b, mask, win = CASES[name]
        _REFERENCE[name] = tuple(torch.from_numpy(t) for t in QF.quality_contract(a, b, mask, win))
    return _REFERENCE[name]


@pytest.fixture
def backend():
    """libmichigan_hip.so (or, dry, the emulator with the group added)"""
    from michigan_amd import _cabi
    prev = _cabi.set_backend(QF.QualityEmulator() if GB.DRY else None)
    be = _cabi.backend()
    assert be.name == ("emulator" if GB.DRY else "hip")
    yield be
    _cabi.set_backend(prev)


def dev(t):
    return None if t is None else torch.from_numpy(t).to(DEV)


def counts(name):
    a, _, _, win = CASES[name]
    n, h, w, c = a.shape
    return (h - len(win) + 1) * (w - len(win) + 1)


def check_quality(name, got_int, got_ssim):
    want_int, want_ssim = reference(name)
    got_int, got_ssim = got_int.cpu(), got_ssim.cpu()
    assert got_int.dtype == torch.int64 and got_ssim.dtype == torch.float64
    assert torch.equal(got_int, want_int), name                                         # squared errors and counts: exact
    count = torch.stack([torch.full_like(want_int[:, :, 3], counts(name)), want_int[:, :, 3]], dim=2).to(torch.float64)
    err = (got_ssim - want_ssim).abs()
    print("%s: max |ssim_sum - contract| / count = %.3e (bound %.1e)" % (name, float((err / count.clamp(min=1)).max()), QF.SSIM_TOL))
    assert bool((err <= QF.SSIM_TOL * count).all()), (name, float((err / count.clamp(min=1)).max()))
    assert bool(torch.isfinite(got_ssim).all())


@pytest.mark.parametrize("name", list(CASES))
def test_image_quality_cases(backend, name):
    from michigan_amd import ops
    a, b, mask, win = CASES[name]
    ta, tb, tm = dev(a), dev(b), dev(mask)
    first = ops.image_quality_u8(ta, tb, tm, win)
    again = ops.image_quality_u8(ta, tb, tm, win)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1]), "two runs are not bit-identical"
    check_quality(name, *first)
    # identical images: every map value is exactly 1.0, so the sums are the counts, bit for bit
    si, ss = ops.image_quality_u8(ta, ta.clone(), tm, win)
    want_int = reference(name)[0]
    assert not si[:, :, :2].any() and torch.equal(si[:, :, 2:].cpu(), want_int[:, :, 2:])
    assert torch.equal(ss[:, :, 0].cpu(), torch.full(ss.shape[:2], float(counts(name)), dtype=torch.float64)), name
    assert torch.equal(ss[:, :, 1].cpu(), want_int[:, :, 3].to(torch.float64)), name


def test_image_quality_through_views(backend):
    """strided and offset views are made dense by the wrapper: the same bits as the dense case"""
    from michigan_amd import metrics
    name = "smooth-3x27x37x3"
    a, b, mask, win = CASES[name]
    n, h, w, c = a.shape
    big = torch.zeros(n + 1, h + 2, w + 3, c + 1, dtype=torch.uint8, device=DEV)
    big[1:, 1:h + 1, 2:w + 2, :c] = dev(a)
    va = big[1:, 1:h + 1, 2:w + 2, :c]
    vb = dev(np.ascontiguousarray(np.transpose(b, (0, 3, 1, 2)))).permute(0, 2, 3, 1)                    # NCHW memory behind an NHWC view
    wide = torch.zeros(n, h, 2 * w + 1, dtype=torch.uint8, device=DEV)
    wide[:, :, 1::2] = dev(mask)
    vm = wide[:, :, 1::2]
    assert not va.is_contiguous() and not vb.is_contiguous() and not vm.is_contiguous() and va.storage_offset() > 0
    q = metrics.image_quality(va, vb, vm)
    want_int, _ = reference(name)
    check_quality(name, torch.stack([q["sse"], q["sse_hair"], q["hair_pixels"][:, None].expand(-1, c), q["ssim_hair_count"][:, None].expand(-1, c)], dim=2),
                  torch.stack([q["ssim_sum"], q["ssim_sum_hair"]], dim=2))
    dense = metrics.image_quality(dev(a), dev(b), dev(mask))
    assert all(torch.equal(q[k], dense[k]) for k in ("psnr", "psnr_hair", "ssim", "ssim_hair", "ssim_sum", "sse_hair"))
    assert bool(torch.isfinite(q["psnr"]).all()) and q["psnr"].device.type == DEV
    one = metrics.image_quality(va[1], vb[1], vm[1])                                                  # [H,W,C]: a view at an odd byte offset
    assert torch.equal(one["ssim_sum"], dense["ssim_sum"][1:2]) and torch.equal(one["sse"], dense["sse"][1:2])


@pytest.mark.parametrize("name", list(ORIENT))
def test_orient_distance_cases(backend, name):
    from michigan_amd import metrics, ops
    a, b, mask = ORIENT[name]
    want = torch.from_numpy(QF.orient_contract(a, b, mask))
    ta, tb, tm = dev(a), dev(b), dev(mask)
    got, again = ops.orient_distance_u8(ta, tb, tm), ops.orient_distance_u8(ta, tb, tm)
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), want) and torch.equal(got, again), name
    same = ops.orient_distance_u8(ta, ta.clone(), tm).cpu()
    assert not same[:, 0].any() and torch.equal(same[:, 1], want[:, 1])                                 # a == b gives 0
    if name.startswith("0-255"):
        assert not want[:, 0].any() and want[:, 1].tolist() == [256, 256]                               # 0 and 255 are one angle
        assert metrics.orient_distance(ta, tb, tm)["degrees"].tolist() == [0.0, 0.0]
    # a sample-aligned and a byte-offset view of the same planes: both load paths give the same sums
    if a.shape[0] > 1:
        tail = ops.orient_distance_u8(ta[1:], tb[1:], tm[1:]).cpu()
        assert torch.equal(tail, want[1:]), name
    if (a.shape[1] * a.shape[2]) % 16 == 0:                                                             # planes of 16-byte rows at an odd address: bytes again
        odd = lambda t: torch.cat([t.new_zeros(1), t.flatten()])[1:].view(t.shape)
        assert odd(ta).data_ptr() % 2 == 1 and torch.equal(ops.orient_distance_u8(odd(ta), odd(tb), odd(tm)).cpu(), want), name


class _Counting:
    """the active backend behind a count of the group's calls"""

    def __init__(self, inner):
        self.__dict__.update(inner=inner, seen=[], name=inner.name)

    def __getattr__(self, fn):
        target = getattr(self.inner, fn)
        if not fn.startswith("mgq_") or fn == "mgq_quality_workspace":
            return target

        def call(*a):
            self.seen.append(fn)
            return target(*a)
        return call


def _guarded(fn, tensors, entry):
    """fn(*placed tensors) -> tensors, twice, under the guard; returns the first run's results on the host"""
    from michigan_amd import _cabi
    with GA.guard(count_backend=False) as g:
        counting = _Counting(_cabi.backend())
        prev = _cabi.set_backend(counting)
        try:
            res = fn(*[g.place(t, DEV) for t in tensors])
            again = fn(*[g.place(t, DEV) for t in tensors])
            assert g.check() > 2 * len(tensors)                                         # the inputs, and the outputs and workspace of ops.py
        finally:
            _cabi.set_backend(prev)
        assert counting.seen == [entry] * 2, counting.seen
        assert all(torch.equal(a, b) for a, b in zip(res, again)), "two runs are not bit-identical"
        return [r.to("cpu", copy=True) for r in res]


@pytest.mark.parametrize("name", ["random-1x11x11x1", "smooth-3x27x37x3", "nomask-3x27x37x3", "k15-1x27x37x3"])
def test_image_quality_guarded(backend, name):
    """the smallest shape and a ragged one: outputs, workspace and the bytes around them; the workspace is written in full (a slot left
    at its 0xFF fill would reach the sums as a NaN or as a huge count)"""
    from michigan_amd import ops
    a, b, mask, win = CASES[name]
    tensors = [torch.from_numpy(t) for t in (a, b) + (() if mask is None else (mask,))]
    got = _guarded(lambda *t: ops.image_quality_u8(t[0], t[1], t[2] if len(t) > 2 else None, win), tensors, "mgq_image_quality_u8")
    check_quality(name, *got)


@pytest.mark.parametrize("name", ["random-1x11x11", "random-3x27x37", "random-3x64x64", "random-2x144x160"])
def test_orient_distance_guarded(backend, name):
    from michigan_amd import ops
    a, b, mask = ORIENT[name]
    (got,) = _guarded(lambda x, y, m: (ops.orient_distance_u8(x, y, m),), [torch.from_numpy(t) for t in (a, b, mask)], "mgq_orient_distance_u8")
    assert torch.equal(got, torch.from_numpy(QF.orient_contract(a, b, mask))), name


def test_refusals_before_any_launch(backend):
    from michigan_amd import _cabi, metrics
    counting = _Counting(backend)
    prev = _cabi.set_backend(counting)
    try:
        a = torch.zeros(2, 16, 16, 3, dtype=torch.uint8, device=DEV)
        m = torch.zeros(2, 16, 16, dtype=torch.uint8, device=DEV)
        for args, kw in (((a.float(), a), {}), ((a, a.permute(0, 3, 1, 2)), {}), ((a[:, :10], a[:, :10]), {}), ((a, a), dict(window=np.ones(4) / 4)),
                         ((torch.zeros(2, 16, 16, 5, dtype=torch.uint8, device=DEV),) * 2, {}), ((a, a), dict(mask=m[:1])), ((a, a), dict(mask=m.cpu() if DEV == "cuda" else m[:, :8]))):
            with pytest.raises(ValueError):
                metrics.image_quality(*args, **kw)
        with pytest.raises(ValueError):
            metrics.orient_distance(m, m, m[:, :8])
        assert counting.seen == []
    finally:
        _cabi.set_backend(prev)


def test_evaluate_on_the_device(backend, tmp_path):
    """`python -m michigan_amd.evaluate --protocol reconstruct` at crop 64, ngf 8: finite rows, equal to metrics.* by hand"""
    import json
    from michigan_amd import evaluate, inference, metrics
    from michigan_amd.model import Pix2PixModel
    root, ck, out = str(tmp_path / "data"), str(tmp_path / "ck"), str(tmp_path / "metrics.json")
    stems = ("v0", "v1", "v2")
    DF.write_dataset(root, stems, seed=6, subset="val", image_ext=".jpg")
    argv = DF.small_argv(root, ck, "e", "--compute_dtype", "fp32", "--gpu_ids", "-1" if GB.DRY else "0", "--load_size", 64, "--which_epoch", 7, "--seed", 8,
                         "--batchSize", 2, "--out", out)
    opt = evaluate.parse(argv)
    torch.manual_seed(2)
    Pix2PixModel(opt).save("7")
    assert evaluate.main(argv) == 0
    with open(out) as fh:
        result = json.load(fh)
    assert result["samples"] == 3 and [r["tag"] for r in result["rows"]] == list(stems)
    for row in result["rows"]:
        assert all(row[k] is not None and math.isfinite(row[k]) for k in ("psnr", "psnr_hair", "ssim", "ssim_hair", "orient_error_deg", "hair_lab"))
        assert row["ssim_count"] == 54 * 54 and 0 < row["ssim_hair_count"] and 0 < row["orient_count"] and 0 <= row["orient_error_deg"] <= 90
    assert all(result["pooled"][k] is not None and math.isfinite(result["pooled"][k]) for k in evaluate.POOLED_KEYS)
    model = inference.build_model(opt)
    names = [(s, s, s) for s in stems]
    device = next(model.parameters()).device
    assert device.type == DEV
    fakes = inference.generate(opt, model, names, rng=random.Random(8), generator=torch.Generator(device=device).manual_seed(8))
    datas = [d for d, _ in inference.generated_batches(opt, model, names, rng=random.Random(8), generator=torch.Generator(device=device).manual_seed(8))]
    real = torch.cat([evaluate.real_u8(d["image_tag"]) for d in datas])
    hair = torch.cat([(d["label_tag"][:, 0] == 1).to(torch.uint8) for d in datas])
    q = metrics.image_quality(fakes, real, hair)
    for i, row in enumerate(result["rows"]):
        assert row["sse"] == q["sse"][i].tolist() and row["sse_hair"] == q["sse_hair"][i].tolist() and row["ssim_sum"] == q["ssim_sum"][i].tolist()
        assert row["psnr"] == q["psnr"][i].item() and row["ssim"] == q["ssim"][i].item() and row["ssim_hair"] == q["ssim_hair"][i].item()
    assert int(fakes.max()) > int(fakes.min())
