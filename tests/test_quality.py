"""CPU: the quality extension group (include/michigan_hip/evaluation/quality.h), michigan_amd.metrics, the evaluation driver and
--val_freq, on `QualityEmulator` (tests/quality_fixtures.py).

1. The contracts: the moments against the four-loop window and scipy.ndimage.correlate1d, hand-counted values, the derived bound, the
   case tables against every one-line mutant, and the mask condition of the inputs.
2. The ledger: the header outside the versioned table, its #defines against their Python mirrors, the library's exports and its
   argument checks (validated before the device is touched, so they run without one).
3. metrics.* on the emulator: conventions, views, refusals before any backend call.
4. `python -m michigan_amd.evaluate`, both protocols, and `train --val_freq 1`, on the tiny dataset of tests/dataset_fixtures.py.
The device side is tests/test_gpu_quality.py."""
import json
import math
import os
import random
import re

import numpy as np
import pytest
import torch

import dataset_fixtures as DF
import quality_fixtures as QF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = QF.quality_cases()
ORIENT = QF.orient_cases()


@pytest.fixture
def emulator():
    from michigan_amd import _cabi
    em = QF.QualityEmulator()
    prev = _cabi.set_backend(em)
    yield em
    _cabi.set_backend(prev)


# ---- 1. contracts ------------------------------------------------------------------------------------------------------------------------
def test_moments_against_the_four_loops_and_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    r = np.random.default_rng(3)
    for k, (h, w) in ((11, (14, 19)), (3, (5, 4)), (15, (16, 17))):
        win = QF.gaussian(k)
        rad = k // 2
        z = r.integers(0, 256, (h, w)).astype(np.float64)
        for f in (z, z * z):
            got = QF._blur(f, win)
            assert got.shape == (h - k + 1, w - k + 1)
            assert np.abs(got - QF.blur_four_loops(f, win)).max() <= 8 * k * 2.0 ** -53 * f.max()
            full = ndi.correlate1d(ndi.correlate1d(f, win, axis=1, mode="constant"), win, axis=0, mode="constant")
            assert np.abs(got - full[rad:h - rad, rad:w - rad]).max() <= 8 * k * 2.0 ** -53 * f.max()
    skew = np.array([0.5, 0.3, 0.2])                                   # not symmetric: a correlation, tap j reads x + j - r
    z = np.zeros((3, 3))
    z[1, 2] = 1.0
    assert QF._blur(z, skew)[0, 0] == skew[1] * skew[2]


def test_contract_by_hand():
    win = QF.gaussian(3)
    a = np.full((1, 3, 3, 1), 10, np.uint8)
    b = np.full((1, 3, 3, 1), 13, np.uint8)
    m = np.zeros((1, 3, 3), np.uint8)
    m[0, 0, 0] = m[0, 1, 1] = 7
    oi, os_ = QF.quality_contract(a, b, m, win)
    assert oi.tolist() == [[[81, 18, 2, 1]]]                            # 9 pixels of 3^2; two under the mask; one of them valid
    want = (2 * 10 * 13 + QF.C1) / (10 * 10 + 13 * 13 + QF.C1)          # flat images: the variances vanish
    assert abs(os_[0, 0, 0] - want) < 1e-12 and abs(os_[0, 0, 1] - want) < 1e-12
    oi, os_ = QF.quality_contract(a, b, None, win)
    assert oi.tolist() == [[[81, 81, 9, 1]]] and os_[0, 0, 0] == os_[0, 0, 1]
    same = QF.quality_contract(a, a, m, win)
    assert same[0].tolist() == [[[0, 0, 2, 1]]] and same[1].tolist() == [[[1.0, 1.0]]]
    o = QF.orient_contract(np.array([[[0, 10, 200, 5]]], np.uint8), np.array([[[255, 250, 10, 5]]], np.uint8), np.array([[[1, 1, 9, 0]]], np.uint8))
    assert o.tolist() == [[0 + 15 + 65, 3]]                             # |0 - 255| = 255 -> 0; 240 -> 15; 190 -> 65


def test_identical_images_give_exactly_one_per_pixel():
    """numerator and denominator are formed from the same bits: the map is 1.0 exactly, and a sum of ones is exact"""
    for name, (a, b, mask, win) in CASES.items():
        oi, os_ = QF.quality_contract(a, a, mask, win)
        n, h, w, c = a.shape
        r = len(win) // 2
        assert np.array_equal(os_[:, :, 0], np.full((n, c), float((h - 2 * r) * (w - 2 * r)))), name
        assert np.array_equal(os_[:, :, 1], oi[:, :, 3].astype(np.float64)), name
        assert not oi[:, :, :2].any()


def test_the_bound_is_derived_and_holds_for_every_window():
    assert QF.ssim_bound(15) <= QF.SSIM_TOL and QF.ssim_bound(11) < QF.ssim_bound(15) and QF.ssim_bound(11) > 1e-10
    assert all(len(win) <= QF.MAX_K for _, _, _, win in CASES.values())
    assert max((a.shape[1] - 2) * (a.shape[2] - 2) for a, _, _, _ in CASES.values()) < 1.8e5        # step 6 of the derivation


def test_case_inputs():
    kinds = {name.split("-")[0] for name in CASES}
    assert kinds == {"random", "bright", "smooth", "constant", "nomask", "k3", "k15", "emptymask"}
    shapes = {(a.shape[1], a.shape[2]) for a, _, _, _ in CASES.values()}
    assert shapes == set(QF.SHAPES)
    for hw in QF.SHAPES:                                                # N and C in {1, 3} at every shape
        seen = {(a.shape[0], a.shape[3]) for a, _, _, _ in CASES.values() if a.shape[1:3] == hw}
        assert {n for n, _ in seen} == {1, 3} and {c for _, c in seen} == {1, 3}, hw
    assert sorted({(h - 10) for h, w in QF.SHAPES} | {(w - 10) for h, w in QF.SHAPES}) == [1, 2, 16, 17, 27, 33, 54]
    for name, (a, b, mask, win) in CASES.items():
        r = len(win) // 2
        assert a.dtype == b.dtype == np.uint8 and a.shape == b.shape and abs(win.sum() - 1) < 1e-15
        if name.startswith("bright"):
            assert a.min() >= 250 and b.min() >= 250
        if name.startswith("smooth"):
            assert np.abs(a.astype(int) - b.astype(int)).max() <= 8 and a.std() > 20
        if name.startswith("constant"):
            assert (a == 255).all() and (b == 254).all()
        if name.startswith("emptymask"):
            assert mask is not None and not mask.any()
        elif mask is not None:                                          # THE MASK CONDITION: a valid-region hair pixel in every sample
            inner = mask[:, r:a.shape[1] - r, r:a.shape[2] - r]
            assert (inner.reshape(len(mask), -1) != 0).any(1).all(), name
            assert set(np.unique(mask)) == {0, 1, 255}, name
    for name, (a, b, mask) in ORIENT.items():
        assert a.shape == b.shape == mask.shape and (name.startswith("emptymask") or (mask.reshape(len(mask), -1) != 0).any(1).all())


def test_the_quality_cases_reject_every_mutant():
    """at the GPU test's bound: an integer term that differs at all, or an ssim sum that differs by 1000 bounds, on at least one case"""
    killed = {m: [] for m in QF.QUALITY_MUTANTS}
    for name, (a, b, mask, win) in CASES.items():
        oi, os_ = QF.quality_contract(a, b, mask, win)
        count = np.stack([np.full(oi.shape[:2], (a.shape[1] - len(win) + 1) * (a.shape[2] - len(win) + 1)), oi[:, :, 3]], axis=2)
        for m in QF.QUALITY_MUTANTS:
            mi, ms = QF.quality_contract(a, b, mask, win, mutant=m)
            if not np.array_equal(mi, oi) or (np.abs(ms - os_) >= 1000 * QF.SSIM_TOL * np.maximum(count, 1)).any():
                killed[m].append(name)
    for m, by in killed.items():
        print("%-20s rejected by %d cases, e.g. %s" % (m, len(by), by[:3]))
    assert all(killed.values()), [m for m, by in killed.items() if not by]
    ssim_only = ("window_shift", "valid_y", "valid_x", "c1_c2_swapped", "sample_variance", "mask_at_corner")
    for m in ssim_only:                                                 # these never touch an integer term: the ssim bound alone rejects them
        a, b, mask, win = CASES[killed[m][0]]
        assert np.array_equal(QF.quality_contract(a, b, mask, win, mutant=m)[0], QF.quality_contract(a, b, mask, win)[0]), m
    assert not [n for n in killed["sse_mask_valid_only"] if n.startswith("emptymask")]


def test_the_orient_cases_reject_every_mutant():
    killed = {m: [] for m in QF.ORIENT_MUTANTS}
    for name, (a, b, mask) in ORIENT.items():
        want = QF.orient_contract(a, b, mask)
        if name.startswith(("same", "0-255")):
            assert not want[:, 0].any() and want[:, 1].all()
        for m in QF.ORIENT_MUTANTS:
            if not np.array_equal(QF.orient_contract(a, b, mask, mutant=m), want):
                killed[m].append(name)
    assert all(killed.values()), killed
    assert "0-255-2x16x16" in killed["period_256"] and "0-255-2x16x16" in killed["no_wrap"]


# ---- 2. the ledger -----------------------------------------------------------------------------------------------------------------------
def test_the_header_is_outside_the_ledger_and_its_defines_match():
    from michigan_amd import _cabi, build, ops
    src = open(os.path.join(ROOT, "include", "michigan_hip", "evaluation", "quality.h")).read()
    stripped = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.findall(r"\b(mg_[a-z0-9_]+)\s*\(", stripped) == []
    names = {"mgq_quality_workspace", "mgq_image_quality_u8", "mgq_orient_distance_u8"}
    assert set(re.findall(r"\b(mgq_[a-z0-9_]+)\s*\(", stripped)) == set(_cabi._QUALITY_PROTOS) == names
    assert not names & set(_cabi._PROTOS) and not names & set(_cabi.EXPORTED_SYMBOLS) and not names & set(_cabi._EDIT_PROTOS)
    assert "mg_quality.hip" in build.SOURCES and "mgq_quality_workspace" in _cabi._EXTENSION_NO_STATUS and _cabi._NO_STATUS <= set(_cabi.EXPORTED_SYMBOLS)
    d = QF.header_defines()
    assert d == {"MGQ_TILE": QF.TILE, "MGQ_MIN_K": QF.MIN_K, "MGQ_MAX_K": QF.MAX_K, "MGQ_MAX_C": QF.MAX_C, "MGQ_WS_SLOTS": QF.WS_SLOTS,
                 "MGQ_INT_TERMS": QF.INT_TERMS, "MGQ_SSIM_TERMS": QF.SSIM_TERMS, "MGQ_ORIENT_PERIOD": QF.PERIOD}
    assert (ops.QUALITY_TILE, ops.QUALITY_MIN_K, ops.QUALITY_MAX_K, ops.QUALITY_MAX_C, ops.QUALITY_WS_SLOTS, ops.QUALITY_INT_TERMS, ops.QUALITY_SSIM_TERMS,
            ops.ORIENT_PERIOD) == (QF.TILE, QF.MIN_K, QF.MAX_K, QF.MAX_C, QF.WS_SLOTS, QF.INT_TERMS, QF.SSIM_TERMS, QF.PERIOD)


def test_the_library_exports_the_group_and_checks_its_arguments():
    """validated before the device is touched, so this runs without one: status, message, and nothing launched"""
    from michigan_amd import _cabi, build
    be = _cabi.HipBackend(build.build(verbose=False))
    for n, h, w, c in ((1, 11, 11, 1), (3, 27, 37, 3), (8, 512, 512, 3), (2, 16, 17, 4)):
        assert be.mgq_quality_workspace(n, h, w, c) == QF.workspace_bytes(n, h, w, c) > 0
    for n, h, w, c in ((0, 11, 11, 1), (1, 11, 11, 5), (1, 11, 11, 0), (1, 0, 11, 1), (8, 16384, 16384, 1)):
        assert be.mgq_quality_workspace(n, h, w, c) == QF.workspace_bytes(n, h, w, c) == 0
    buf = torch.zeros(8192, dtype=torch.uint8)
    p = QF.pointer(buf)
    win = np.ascontiguousarray(QF.gaussian(11))
    wp = QF.pointer(torch.from_numpy(win))
    base = dict(a=p, b=p, mask=None, window=wp, k=11, ws=p, out_int=p, out_ssim=p, n=1, h=11, w=11, c=1, stream=None)
    order = ("a", "b", "mask", "window", "k", "ws", "out_int", "out_ssim", "n", "h", "w", "c", "stream")
    for kw, msg in ((dict(a=None), "null pointer"), (dict(window=None), "null pointer"), (dict(ws=None), "null pointer"), (dict(out_ssim=None), "null pointer"),
                    (dict(k=10), "bad window length"), (dict(k=1), "bad window length"), (dict(k=17), "bad window length"), (dict(c=5), "bad channel count"),
                    (dict(c=0), "bad channel count"), (dict(n=0), "bad geometry"), (dict(h=10), "smaller than the window"), (dict(w=10), "smaller than the window"),
                    (dict(n=1 << 20, h=1 << 10, w=1 << 10), "bad geometry"), (dict(ws=QF.pointer(buf[4:])), "8-byte aligned")):
        with pytest.raises(RuntimeError, match=r"mgq_image_quality_u8 failed \(code 1\): mgq_image_quality_u8: .*" + msg):
            be.mgq_image_quality_u8(*[dict(base, **kw)[k] for k in order])
    for args, msg in (((None, p, p, p, 1, 8, 8, None), "null pointer"), ((p, p, None, p, 1, 8, 8, None), "null pointer"), ((p, p, p, p, 0, 8, 8, None), "bad geometry"),
                      ((p, p, p, p, 1 << 20, 1 << 10, 1 << 10, None), "bad geometry"), ((p, p, p, QF.pointer(buf[4:]), 1, 8, 8, None), "8-byte aligned")):
        with pytest.raises(RuntimeError, match="mgq_orient_distance_u8: .*" + msg):
            be.mgq_orient_distance_u8(*args)
    assert not buf.any()
    with pytest.raises(AttributeError):
        be.mgq_not_an_entry_point


# ---- 3. metrics on the emulator ------------------------------------------------------------------------------------------------------------
def test_gaussian_window():
    from michigan_amd import metrics
    g = metrics.gaussian_window()
    assert g.dtype == np.float64 and g.shape == (11,) and np.array_equal(g, QF.gaussian(11, 1.5)) and np.array_equal(g, g[::-1]) and abs(g.sum() - 1) < 1e-15
    assert np.array_equal(metrics.gaussian_window(5, 0.8), QF.gaussian(5, 0.8))
    for bad in ((10, 1.5), (0, 1.5), (11, 0.0)):
        with pytest.raises(ValueError):
            metrics.gaussian_window(*bad)


def test_image_quality_conventions(emulator):
    from michigan_amd import metrics
    a, b, mask, win = CASES["random-3x27x37x3"]
    ta, tb, tm = torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(mask)
    q = metrics.image_quality(ta, tb, tm)
    oi, os_ = QF.quality_contract(a, b, mask, win)
    n, h, w, c = a.shape
    assert torch.equal(q["sse"], torch.from_numpy(oi[:, :, 0])) and torch.equal(q["sse_hair"], torch.from_numpy(oi[:, :, 1]))
    assert torch.equal(q["ssim_sum"], torch.from_numpy(os_[:, :, 0])) and torch.equal(q["ssim_sum_hair"], torch.from_numpy(os_[:, :, 1]))
    assert q["pixels"].tolist() == [h * w] * n and q["ssim_count"].tolist() == [17 * 27] * n and q["channels"] == 3
    assert q["hair_pixels"].tolist() == (mask != 0).sum((1, 2)).tolist() and q["ssim_hair_count"].tolist() == oi[:, 0, 3].tolist()
    for k in ("psnr", "psnr_hair", "ssim", "ssim_hair"):
        assert q[k].dtype == torch.float64 and tuple(q[k].shape) == (n,)
    want_psnr = 10 * np.log10(255.0 ** 2 * h * w * c / oi[:, :, 0].sum(1))
    assert np.allclose(q["psnr"].numpy(), want_psnr, rtol=1e-14, atol=0)
    assert np.allclose(q["psnr_hair"].numpy(), 10 * np.log10(255.0 ** 2 * oi[:, 0, 2] * c / oi[:, :, 1].sum(1)), rtol=1e-14, atol=0)
    assert np.allclose(q["ssim"].numpy(), (os_[:, :, 0] / (17 * 27)).mean(1), rtol=1e-14, atol=0)            # the mean over channels of the per-channel means
    assert np.allclose(q["ssim_hair"].numpy(), (os_[:, :, 1] / oi[:, :, 3]).mean(1), rtol=1e-14, atol=0)
    # [H,W,C] and a single sample agree; no mask: the hair variants are the full ones
    one = metrics.image_quality(ta[1], tb[1], tm[1])
    assert all(torch.equal(one[k], q[k][1:2]) for k in ("psnr", "psnr_hair", "ssim", "ssim_hair", "sse", "ssim_sum_hair"))
    free = metrics.image_quality(ta, tb)
    assert torch.equal(free["psnr"], free["psnr_hair"]) and torch.equal(free["ssim"], free["ssim_hair"]) and torch.equal(free["psnr"], q["psnr"])
    # identical images: inf and exactly 1; an empty mask: nan
    same = metrics.image_quality(ta, ta, tm)
    assert torch.isinf(same["psnr"]).all() and torch.isinf(same["psnr_hair"]).all() and (same["ssim"] == 1).all() and (same["ssim_hair"] == 1).all()
    empty = metrics.image_quality(ta, tb, torch.zeros_like(tm))
    assert torch.isnan(empty["psnr_hair"]).all() and torch.isnan(empty["ssim_hair"]).all() and torch.equal(empty["psnr"], q["psnr"])
    # views are made dense by the wrapper
    big = torch.zeros(n, h + 2, w + 3, c + 1, dtype=torch.uint8)
    big[:, 1:h + 1, 2:w + 2, :c] = ta
    v = metrics.image_quality(big[:, 1:h + 1, 2:w + 2, :c], tb.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1), tm)
    assert torch.equal(v["ssim_sum"], q["ssim_sum"]) and torch.equal(v["sse_hair"], q["sse_hair"])
    # another window
    q3 = metrics.image_quality(ta, tb, tm, window=metrics.gaussian_window(3, 1.5))
    assert torch.equal(q3["ssim_sum"], torch.from_numpy(QF.quality_contract(a, b, mask, QF.gaussian(3))[1][:, :, 0])) and q3["ssim_count"].tolist() == [25 * 35] * n


def test_orient_distance_conventions(emulator):
    from michigan_amd import metrics
    a, b, mask = ORIENT["random-3x27x37"]
    o = metrics.orient_distance(torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(mask))
    want = QF.orient_contract(a, b, mask)
    assert torch.equal(o["sum"], torch.from_numpy(want[:, 0])) and torch.equal(o["count"], torch.from_numpy(want[:, 1]))
    assert np.allclose(o["degrees"].numpy(), want[:, 0] / want[:, 1] * 180 / 255, rtol=1e-14, atol=0) and o["degrees"].dtype == torch.float64
    one = metrics.orient_distance(torch.from_numpy(a[2]), torch.from_numpy(b[2]), torch.from_numpy(mask[2]))
    assert torch.equal(one["sum"], o["sum"][2:3])
    z, f = torch.zeros(1, 4, 4, dtype=torch.uint8), torch.full((1, 4, 4), 255, dtype=torch.uint8)
    assert metrics.orient_distance(z, f, torch.ones_like(z))["degrees"].tolist() == [0.0]                # 0 and 255 are the same angle
    assert metrics.orient_distance(z, torch.full_like(z, 128), torch.ones_like(z))["degrees"].tolist() == pytest.approx([127 * 180 / 255], rel=1e-15)
    assert torch.isnan(metrics.orient_distance(z, f, z)["degrees"]).all()


class Recording:
    """a backend that refuses to be called: what raises ValueError must raise before it gets here"""
    name = "emulator"

    def __init__(self):
        self.log = []

    def __getattr__(self, key):
        def call(*a, **k):
            self.log.append(key)
            raise AssertionError("backend called: " + key)
        return call


def test_refusals_raise_before_any_backend_call():
    from michigan_amd import _cabi, metrics
    rec = Recording()
    prev = _cabi.set_backend(rec)
    try:
        a = torch.zeros(2, 16, 16, 3, dtype=torch.uint8)
        m = torch.zeros(2, 16, 16, dtype=torch.uint8)
        for args, kw in (((a.float(), a), {}), ((a, a.to(torch.int16)), {}),                                       # wrong dtype
                         ((a, a), dict(mask=m.bool())), ((a, a), dict(mask=m.float())),
                         ((a[0, 0], a[0, 0]), {}), ((a.unsqueeze(0), a.unsqueeze(0)), {}), ((a, a[:, :, :, :2]), {}), ((a, a[:1]), {}),      # wrong layout
                         ((a[:, :10], a[:, :10]), {}), ((a[:, :, :10], a[:, :, :10]), {}),                           # H < k, W < k
                         ((a, a), dict(window=np.ones(10) / 10)), ((a, a), dict(window=np.ones(17) / 17)), ((a, a), dict(window=np.ones(1))),   # even k, k out of range
                         ((a, a), dict(window=np.ones((3, 3)) / 9)), ((a, a), dict(window=[0.5, float("nan"), 0.5])),
                         ((torch.zeros(2, 16, 16, 5, dtype=torch.uint8),) * 2, {}),                                   # C > 4
                         ((a, a), dict(mask=m[:1])), ((a, a), dict(mask=m[:, :8])), ((a, a), dict(mask=m.unsqueeze(1))), ((a[0], a[0]), dict(mask=m)),   # mask shape
                         ((a.numpy(), a.numpy()), {})):
            with pytest.raises(ValueError):
                metrics.image_quality(*args, **kw)
        for args in ((m.float(), m, m), (m, m.float(), m), (m, m, m.bool()), (m, m[:1], m), (m, m, m[:, :8]), (m, m, None), (m[0], m, m), (m.unsqueeze(1), m.unsqueeze(1), m.unsqueeze(1))):
            with pytest.raises(ValueError):
                metrics.orient_distance(*args)
        assert rec.log == []
    finally:
        _cabi.set_backend(prev)


def test_pooled_is_built_from_sums():
    from michigan_amd import metrics
    rows = [dict(sse=[0, 0, 0], sse_hair=[0, 0, 0], pixels=100, hair_pixels=10, ssim_sum=[64.0, 64.0, 64.0], ssim_sum_hair=[4.0, 4.0, 4.0], ssim_count=64,
                 ssim_hair_count=4, channels=3, orient_sum=0, orient_count=10, hair_lab=1.0),                  # a perfect sample: psnr inf
            dict(sse=[300, 300, 300], sse_hair=[90, 0, 0], pixels=100, hair_pixels=30, ssim_sum=[32.0, 32.0, 16.0], ssim_sum_hair=[6.0, 6.0, 6.0], ssim_count=64,
                 ssim_hair_count=12, channels=3, orient_sum=510, orient_count=30, hair_lab=3.0)]
    p = metrics.pooled(rows)
    assert p["samples"] == 2 and math.isfinite(p["psnr"])
    assert p["psnr"] == 10 * math.log10(255.0 ** 2 * 600 / 900) and p["psnr_hair"] == 10 * math.log10(255.0 ** 2 * 120 / 90)
    assert p["ssim"] == (192 + 80) / (128 * 3) and p["ssim_hair"] == (12 + 18) / (16 * 3)
    assert p["orient_error_deg"] == 510 / 40 * 180 / 255 and p["hair_lab"] == 2.0
    assert metrics.pooled(rows[:1])["psnr"] == float("inf")
    t = metrics.pooled([dict(orient_sum=5, orient_count=0, hair_lab=0.5)])                                  # a transfer row: no ground truth
    assert math.isnan(t["psnr"]) and math.isnan(t["ssim_hair"]) and math.isnan(t["orient_error_deg"]) and t["hair_lab"] == 0.5
    assert math.isnan(metrics.pooled([])["psnr"]) and metrics.pooled([])["samples"] == 0


# ---- 4. the drivers ----------------------------------------------------------------------------------------------------------------------
STEMS = ("v0", "v1", "v2")


def evaluate_argv(root, ck, *extra):
    return DF.small_argv(root, ck, "e", "--compute_dtype", "fp32", "--gpu_ids", "-1", "--load_size", 64, "--which_epoch", 7, "--seed", 8, *extra)


def saved_model(opt):
    from michigan_amd import inference
    from michigan_amd.model import Pix2PixModel
    torch.manual_seed(2)
    Pix2PixModel(opt).save("7")
    return inference.build_model(opt)


def check_rows_reproduce_pooled(result):
    from michigan_amd import metrics
    rows, p = result["rows"], result["pooled"]
    assert result["samples"] == len(rows) == p["samples"]
    tot = lambda k: sum(r[k] for r in rows)
    assert abs(p["orient_error_deg"] - tot("orient_sum") / tot("orient_count") * 180 / 255) < 1e-12
    assert abs(sum(r["orient_error_deg"] * r["orient_count"] for r in rows) / tot("orient_count") - p["orient_error_deg"]) < 1e-9
    assert abs(p["hair_lab"] - tot("hair_lab") / len(rows)) < 1e-12
    if result["protocol"] == "reconstruct":
        c = rows[0]["channels"]
        assert abs(sum(r["ssim"] * r["ssim_count"] for r in rows) / tot("ssim_count") - p["ssim"]) < 1e-12          # rows times counts
        assert abs(sum(r["ssim_hair"] * r["ssim_hair_count"] for r in rows) / tot("ssim_hair_count") - p["ssim_hair"]) < 1e-12
        assert abs(p["psnr"] - 10 * math.log10(255.0 ** 2 * tot("pixels") * c / sum(sum(r["sse"]) for r in rows))) < 1e-12
        assert abs(p["psnr_hair"] - 10 * math.log10(255.0 ** 2 * tot("hair_pixels") * c / sum(sum(r["sse_hair"]) for r in rows))) < 1e-12
        for r in rows:
            assert abs(r["psnr"] - 10 * math.log10(255.0 ** 2 * r["pixels"] * c / sum(r["sse"]))) < 1e-9
    assert p == metrics.pooled(rows) or all(p[k] == v or (math.isnan(p[k]) and math.isnan(v)) for k, v in metrics.pooled(rows).items())


def test_evaluate_both_protocols(emulator, tmp_path):
    from michigan_amd import evaluate, inference, metrics
    root, ck = str(tmp_path / "data"), str(tmp_path / "ck")
    DF.write_dataset(root, STEMS, seed=6, subset="val", image_ext=".jpg")
    out = str(tmp_path / "m" / "metrics.json")
    argv = evaluate_argv(root, ck, "--batchSize", 2, "--out", out)
    opt = evaluate.parse(argv)
    assert opt.protocol == "reconstruct" and opt.max_samples == 0 and opt.subset == "val" and not opt.isTrain and opt.no_flip
    assert evaluate.reconstruct_names(opt) == [(s, s, s) for s in STEMS] and evaluate.reconstruct_names(opt, 2) == [(s, s, s) for s in STEMS[:2]]
    model = saved_model(opt)
    before = len(emulator.calls)
    assert evaluate.main(argv) == 0
    mine = [name for name, _ in emulator.calls[before:]]
    assert mine.count("mgq_image_quality_u8") == 2 and mine.count("mgq_orient_distance_u8") == 2          # once a batch: batches of 2 and 1
    with open(out) as fh:
        result = json.load(fh)
    assert set(result) == {"protocol", "samples", "pooled", "rows"} and result["protocol"] == "reconstruct" and result["samples"] == 3
    assert set(result["pooled"]) == set(evaluate.POOLED_KEYS)
    for row in result["rows"]:
        assert set(row) == set(evaluate.COMMON_ROW_KEYS) | set(evaluate.QUALITY_ROW_KEYS)
        assert row["ref"] == row["tag"] == row["orient"] and len(row["sse"]) == len(row["ssim_sum"]) == 3 and row["channels"] == 3
        assert all(math.isfinite(row[k]) for k in ("psnr", "psnr_hair", "ssim", "ssim_hair", "orient_error_deg", "hair_lab"))
        assert row["pixels"] == 64 * 64 and row["ssim_count"] == 54 * 54 and 0 < row["ssim_hair_count"] <= row["hair_pixels"] < 64 * 64
        assert 0 < row["orient_count"] <= row["hair_pixels"] and 0 <= row["orient_error_deg"] <= 90 and -1 <= row["ssim"] <= 1 and row["psnr"] > 0
    check_rows_reproduce_pooled(result)
    # the rows are metrics.* by hand on what inference.generate returns for the same seed
    gen = torch.Generator().manual_seed(8)
    fakes = inference.generate(opt, model, [(s, s, s) for s in STEMS], rng=random.Random(8), generator=gen)
    gen = torch.Generator().manual_seed(8)
    datas = [d for d, _ in inference.generated_batches(opt, model, [(s, s, s) for s in STEMS], rng=random.Random(8), generator=gen)]
    real = torch.cat([evaluate.real_u8(d["image_tag"]) for d in datas])
    hair = torch.cat([(d["label_tag"][:, 0] == 1).to(torch.uint8) for d in datas])
    q = metrics.image_quality(fakes, real, hair)
    for i, row in enumerate(result["rows"]):
        assert row["sse"] == q["sse"][i].tolist() and row["ssim_sum"] == q["ssim_sum"][i].tolist() and row["psnr"] == q["psnr"][i].item()
        assert row["ssim_hair"] == q["ssim_hair"][i].item() and row["hair_pixels"] == int(q["hair_pixels"][i])
    # real_u8 gives the stored bytes back where nothing was resized
    x = torch.arange(256, dtype=torch.uint8).reshape(1, 16, 16, 1).expand(1, 16, 16, 3)
    assert torch.equal(evaluate.real_u8(((x.float() / 255 - 0.5) / 0.5).permute(0, 3, 1, 2)), x)
    # transfer: no ground truth
    pairs = str(tmp_path / "pairs.txt")
    with open(pairs, "w") as f:
        f.write("v0 v1 v2\nv1 v2 v2\n\nv2 v0 v1\n")
    out2 = str(tmp_path / "transfer.json")
    assert evaluate.main(evaluate_argv(root, ck, "--protocol", "transfer", "--pairs_file", pairs, "--out", out2, "--max_samples", 3)) == 0
    with open(out2) as fh:
        result = json.load(fh)
    assert result["protocol"] == "transfer" and result["samples"] == 3 and [(r["ref"], r["tag"], r["orient"]) for r in result["rows"]] == [
        ("v0", "v1", "v2"), ("v1", "v2", "v2"), ("v2", "v0", "v1")]
    assert all(set(r) == set(evaluate.COMMON_ROW_KEYS) for r in result["rows"])
    assert result["pooled"]["psnr"] is None and result["pooled"]["ssim"] is None and result["pooled"]["orient_error_deg"] is not None
    for k in ("psnr", "psnr_hair", "ssim", "ssim_hair"):
        result["pooled"][k] = float("nan")
    check_rows_reproduce_pooled(result)
    with pytest.raises(ValueError, match="pairs_file"):
        evaluate.main(evaluate_argv(root, ck, "--protocol", "transfer"))
    with pytest.raises(ValueError, match="reconstruct"):
        evaluate.evaluate(opt, model, [("v0", "v1", "v1")], "reconstruct")


LOSSES = re.compile(r"\(step: \d, epoch: \d+, iters: \d+, time: \d+\.\d{3}\) (.*)$")


def test_val_freq_changes_nothing_of_the_training_run(emulator, tmp_path):
    from michigan_amd import train
    root = str(tmp_path / "data")
    DF.write_dataset(root, ("a0", "a1", "a2", "a3"), seed=3)
    DF.write_dataset(root, STEMS, seed=6, subset="val", image_ext=".jpg")
    runs = {}
    for name, extra in (("plain", ()), ("val", ("--val_freq", 1, "--val_max_samples", 2))):
        ck = str(tmp_path / name)
        opt = train.parse(DF.small_argv(root, ck, "t", "--compute_dtype", "fp32", "--gpu_ids", "-1", "--batchSize", 2, "--seed", 5, "--print_freq", 2,
                                        "--save_latest_freq", 100, "--niter", 2, *extra))
        assert opt.val_freq == (1 if extra else 0)
        before = len(emulator.calls)
        train.train(opt)
        calls = [n for n, _ in emulator.calls[before:]]
        with open(os.path.join(ck, "t", "loss_log.txt")) as f:
            lines = [LOSSES.search(l).group(1) for l in f if not l.startswith("=")]
        runs[name] = dict(calls=calls, lines=lines, nets={n: torch.load(os.path.join(ck, "t", "2_net_%s.pth" % n)) for n in "GD"},
                          optim=torch.load(os.path.join(ck, "t", "2_optim.pth")), dir=os.path.join(ck, "t"))
    plain, val = runs["plain"], runs["val"]
    assert not os.path.exists(os.path.join(plain["dir"], "val_log.txt")) and not [c for c in plain["calls"] if c.startswith("mgq_")]
    assert val["calls"].count("mgq_image_quality_u8") == 2 and val["calls"].count("mgq_orient_distance_u8") == 2      # one batch of 2 an epoch
    assert len(plain["lines"]) == 4 and plain["lines"] == val["lines"]                                    # the same losses, line for line
    for n in "GD":                                                      # weights, spectral-norm vectors and running statistics alike
        assert set(plain["nets"][n]) == set(val["nets"][n])
        assert all(torch.equal(plain["nets"][n][k], val["nets"][n][k]) for k in plain["nets"][n]), n

    def same(x, y):
        if torch.is_tensor(x):
            return torch.equal(x, y)
        if isinstance(x, dict):
            return set(x) == set(y) and all(same(x[k], y[k]) for k in x)
        if isinstance(x, (list, tuple)):
            return len(x) == len(y) and all(same(u, v) for u, v in zip(x, y))
        return x == y
    assert same(plain["optim"], val["optim"])
    with open(os.path.join(val["dir"], "val_log.txt")) as f:
        log = f.read().splitlines()
    assert len(log) == 2 and log[0].startswith("(epoch: 1, samples: 2) psnr: ") and log[1].startswith("(epoch: 2, samples: 2) psnr: ")
    assert all(k + ": " in log[0] for k in ("psnr", "psnr_hair", "ssim", "ssim_hair", "orient_error_deg", "hair_lab"))
    assert "nan" not in log[0] and "inf" not in log[0]
