"""CPU: the device loaders of every batch kind Pix2PixModel.forward accepts -- DeviceInputPipeline with image_ref / label_ref (the
unpaired stage, pix2pix_dataset.py:66-194 at step 2), inputs.inference_batch (single_inference_dataLoad, base_dataset.py:49-160) and
inputs.demo_batch (demo_inference_dataLoad, :162-276) -- on the contract emulator, against what the REFERENCE's own functions
returned for the same decoded files and the same draws (tests/golden/loader_*.npz from tools/make_loader_golden.py).  The rule of
comparison is tests/loader_fixtures.compare: torch.equal, no tolerance; `noise` through check_noise.  The same fixtures run on the
device in tests/test_gpu_loader_batches.py."""
import random

import pytest
import torch

import loader_fixtures as LF

DATASET_KEYS = {"label_tag", "label_ref", "instance", "image_tag", "image_ref", "orient", "hole", "orient_rgb", "noise"}
DEMO_KEYS = DATASET_KEYS | {"orient_rgb_mask", "orient_stroke", "mask_stroke"}
C, L, TH, TW, RH, RW = LF.CROP, LF.LOAD, 40, 36, 36, 40      # the fixture's geometry: target files 40 x 36, reference files 36 x 40


class Recording:
    """the emulator behind a log of every mg_* call: (name, its integer arguments); pointers and streams are left out"""
    name = "emulator"

    def __init__(self):
        from oracle.cabi_emulator import EmulatorBackend
        self.inner, self.log = EmulatorBackend(), []

    def __getattr__(self, key):
        fn = getattr(self.inner, key)
        if not key.startswith("mg_"):
            return fn

        def call(*a, **k):
            self.log.append((key,) + tuple(v for v in a if type(v) is int))
            return fn(*a, **k)
        return call


@pytest.fixture
def recording():
    from michigan_amd import _cabi
    be = Recording()
    prev = _cabi.set_backend(be)
    yield be
    _cabi.set_backend(prev)


# ---- 1. the three batch kinds against the reference's own functions ---------------------------------------------------------------------
@pytest.mark.parametrize("as_list", [False, True], ids=["batched", "per-sample"])
def test_unpaired_batch_is_the_datasets_at_step_two(emulator_backend, as_list):
    data, case = LF.run_unpaired("cpu", as_list=as_list)
    assert set(data) == DATASET_KEYS and data["instance"] == 0 and type(data["instance"]) is int
    LF.compare(data, case["want"])
    LF.check_noise(data, case, "cpu")
    assert not torch.equal(data["image_ref"], data["image_tag"]) and not torch.equal(data["label_ref"], data["label_tag"])
    assert float(data["label_ref"].max()) == LF.LABEL_NC               # the reference files hold 'unknown' pixels: 255 -> label_nc
    assert sorted(float(v) > 0.5 for v in case["draws"]["flip"]) == [False, True]


@pytest.mark.parametrize("name", LF.INFERENCE_CASES)
def test_inference_batch_is_single_inference_dataload(emulator_backend, name):
    data, case = LF.run_inference(name, "cpu")
    assert set(data) == DATASET_KEYS
    LF.compare(data, case["want"])
    LF.check_noise(data, case, "cpu")
    assert data["instance"].dtype == torch.int64 and data["instance"].dim() == 0
    assert data["hole"].shape == (2, 1, C, C) and float(data["hole"].abs().max()) > 0


@pytest.mark.parametrize("name", LF.DEMO_CASES)
def test_demo_batch_is_demo_inference_dataload(emulator_backend, name):
    data, case = LF.run_demo(name, "cpu")
    assert set(data) == DEMO_KEYS
    LF.compare(data, case["want"])
    LF.check_noise(data, case, "cpu")
    if name == "plain":
        assert all(data[k].dim() == 0 and data[k].dtype == torch.int64 for k in ("orient_stroke", "mask_stroke"))
    else:
        assert data["orient_stroke"].shape == (2, 3, C, C) and float(data["orient_stroke"].max()) > 0
        assert set(data["mask_stroke"].unique().tolist()) == {0.0, 1.0}


def test_inference_batch_adds_the_batch_dimension_and_honours_use_ig(emulator_backend):
    from michigan_amd import inputs
    case = LF.load("inference")["other_plain"]
    one = {k: torch.from_numpy(v[0]) for k, v in case["src"].items()}
    draws = {k: v[:1] for k, v in case["draws"].items()}
    data = inputs.inference_batch(LF.options(isTrain=False), same_orient=False, rng=LF.ReplayRng(draws, hole=False), **one)
    LF.compare(data, {k: (v[:1] if v.ndim else v) for k, v in case["want"].items()})
    data, _ = LF.run_inference("same_plain", "cpu", use_ig=False)                     # :112,125: torch.tensor(0) twice, and no hole draws
    for k in ("hole", "orient_rgb"):
        assert torch.is_tensor(data[k]) and data[k].dim() == 0 and data[k].dtype == torch.int64 and int(data[k]) == 0
    want = {k: v for k, v in LF.load("inference")["same_plain"]["want"].items() if k not in ("hole", "orient_rgb")}
    LF.compare({k: v for k, v in data.items() if k not in ("hole", "orient_rgb")}, want)


# ---- 2. without the reference slot nothing changes ------------------------------------------------------------------------------------------
def _parent_log(n):
    """what the pipeline's __call__ issued before it knew of a reference slot, written out for the fixture's geometry (images and maps
    stored at 40 x 36, load 32, crop 24, use_ig): the constructor's table, the image's bicubic tables and resize, the maps' index
    tables, then label, image, orient, picture (2 launches), hole (2 launches), noise"""
    crop = lambda hs, ws, c, mode, unknown: ("mg_input_crop_u8", n, hs, ws, c, C, C, mode, unknown)
    return [("mg_orient_rgb_table",),
            ("mg_bicubic_ksize", TW, L), ("mg_bicubic_table", TW, L), ("mg_bicubic_ksize", TH, L), ("mg_bicubic_table", TH, L),
            None,                                                          # mg_resize_bicubic_u8: its window sizes are the table's
            ("mg_nearest_table", TH, L), ("mg_nearest_table", TW, L),
            crop(TH, TW, 1, 1, LF.LABEL_NC), crop(L, L, 3, 0, -1), crop(TH, TW, 1, 1, -1),
            ("mg_orient_to_rgb_u8", n * TH * TW), crop(TH, TW, 3, 2, -1),
            ("mg_generate_hole_u8", n, TH, TW), crop(TH, TW, 1, 1, -1),
            ("mg_noise_field_len", C), ("mg_noise_field_len", C), ("mg_noise_octaves", n, C)]


def test_without_a_reference_slot_the_call_log_is_the_parents(recording):
    data, case = LF.run_unpaired("cpu", refs=False)
    want, log = _parent_log(2), recording.log
    assert len(log) == len(want), log
    for got, w in zip(log, want):
        if w is None:
            assert got[0] == "mg_resize_bicubic_u8" and got[-6:] == (2, TH, TW, L, L, 3), got
        else:
            assert got == w
    assert data["image_ref"] is data["image_tag"] and data["label_ref"] is data["label_tag"]
    ref = {k: v for k, v in case["want"].items() if k not in ("image_ref", "label_ref")}          # every other entry is the same batch
    LF.compare({k: v for k, v in data.items() if k in ref}, ref)
    # with the slot: the same sequence first, then three launches (label; resize + crop of the image) through the tables of its size
    del recording.log[:]
    LF.run_unpaired("cpu")
    extra = recording.log[len(want):]
    assert [e[0] for e in recording.log[:len(want)]] == [(w[0] if w else "mg_resize_bicubic_u8") for w in want]
    assert [e[0] for e in extra] == ["mg_input_crop_u8", "mg_bicubic_ksize", "mg_bicubic_table", "mg_bicubic_ksize", "mg_bicubic_table",
                                     "mg_resize_bicubic_u8", "mg_input_crop_u8"], extra
    assert extra[0] == ("mg_input_crop_u8", 2, RH, RW, 1, C, C, 1, LF.LABEL_NC) and extra[-1] == ("mg_input_crop_u8", 2, L, L, 3, C, C, 0, -1)


def test_host_draw_order_is_unchanged_by_the_reference_slot(emulator_backend):
    """draw_params, then th, then u -- from a real random.Random, with and without the slot the same windows and the same hole"""
    from michigan_amd import inputs
    s = LF.sources(LF.load("unpaired")["step2"], "cpu")
    runs = []
    for kw in ({}, dict(image_ref=s["image_ref"], label_ref=s["label_ref"])):
        pipe = inputs.DeviceInputPipeline(LF.options(), "cpu", rng=random.Random(11), generator=LF.generator("cpu"))
        runs.append((pipe(s["image"], s["label"], s["orient"], s["orient_mask"], **kw), pipe.rng.random()))
    (a, ra), (b, rb) = runs
    assert ra == rb
    for k in ("label_tag", "image_tag", "orient", "orient_rgb", "hole", "noise"):
        assert torch.equal(a[k], b[k]), k


# ---- 3. what is refused, on the host, before anything is uploaded --------------------------------------------------------------------------
def test_argument_checks(recording):
    from michigan_amd import inputs
    s = LF.sources(LF.load("unpaired")["step2"], "cpu")
    pipe = inputs.DeviceInputPipeline(LF.options(), "cpu", rng=random.Random(0))
    launches = lambda: [e for e in recording.log if e[0] in ("mg_input_crop_u8", "mg_resize_bicubic_u8", "mg_orient_to_rgb_u8", "mg_generate_hole_u8")]
    call = lambda **kw: pipe(s["image"], s["label"], s["orient"], s["orient_mask"], **kw)
    with pytest.raises(ValueError, match="together"):
        call(image_ref=s["image_ref"])
    with pytest.raises(ValueError, match="together"):
        call(label_ref=s["label_ref"])
    with pytest.raises(ValueError, match="uint8"):
        call(image_ref=s["image_ref"].float(), label_ref=s["label_ref"])
    with pytest.raises(ValueError, match="label_ref"):
        call(image_ref=s["image_ref"], label_ref=s["label_ref"][:1])
    with pytest.raises(ValueError, match="image_ref"):
        call(image_ref=s["image_ref"][..., :2], label_ref=s["label_ref"])
    with pytest.raises(ValueError, match="sequences"):
        call(image_ref=list(s["image_ref"]), label_ref=s["label_ref"])
    with pytest.raises(ValueError, match="does not match"):
        pipe(s["image"], s["label"], s["orient"][:, :-1], s["orient_mask"])
    with pytest.raises(ValueError, match="does not match"):
        pipe(s["image"], s["label"], s["orient"], s["orient_mask"][:, :, :-1])
    with pytest.raises(NotImplementedError, match="color_jitter"):
        inputs.DeviceInputPipeline(LF.options(color_jitter=True), "cpu")(s["image"], s["label"], s["orient"], image_ref=s["image_ref"], label_ref=s["label_ref"])
    with pytest.raises(ValueError, match="crop window"):                     # a window larger than the load size
        inputs.DeviceInputPipeline(LF.options(crop_size=L + 8), "cpu", rng=random.Random(0))(s["image"], s["label"], s["orient"])
    assert launches() == []

    inf = LF.sources(LF.load("inference")["same_plain"], "cpu")
    run = lambda opt=None, **over: inputs.inference_batch(opt or LF.options(isTrain=False), same_orient=True, rng=random.Random(0), **dict(inf, **over))
    with pytest.raises(ValueError, match="one size"):
        run(orient_mask=inf["orient_mask"][:, :-1])
    with pytest.raises(ValueError, match="one size"):
        run(orient_ref=inf["orient_ref"][:, :, :-1])
    with pytest.raises(ValueError, match="uint8"):
        run(label_tag=inf["label_tag"].float())
    with pytest.raises(ValueError, match="image_tag"):
        run(image_tag=inf["image_tag"][..., 0])
    with pytest.raises(ValueError, match="batch of 1"):
        run(orient_tag=inf["orient_tag"][:1])
    with pytest.raises(ValueError, match="crop window"):
        run(LF.options(isTrain=False, crop_size=L + 8))
    with pytest.raises(NotImplementedError, match="expand_tag_mask"):
        run(LF.options(isTrain=False, expand_tag_mask=True))
    with pytest.raises(NotImplementedError, match="color_jitter"):
        run(LF.options(isTrain=False, color_jitter=True))
    with pytest.raises(NotImplementedError, match="preprocess_mode"):
        run(LF.options(isTrain=False, preprocess_mode="scale_width_and_crop"))

    demo = LF.sources(LF.load("demo")["strokes"], "cpu")
    run = lambda opt=None, **over: inputs.demo_batch(opt or LF.options(isTrain=False), rng=random.Random(0), **dict(demo, **over))
    with pytest.raises(ValueError, match="together"):
        run(mask_hole=None)
    with pytest.raises(ValueError, match="together"):
        run(mask_stroke=None)
    with pytest.raises(ValueError, match="one size"):
        run(mask_hole=demo["mask_hole"][:, :-1])
    with pytest.raises(ValueError, match="one size"):
        run(mask_orient=demo["mask_orient"][:, :-1])
    with pytest.raises(ValueError, match="uint8"):
        run(mask_stroke=demo["mask_stroke"].float())
    with pytest.raises(TypeError):
        run(orient_stroke=demo["mask_stroke"])                               # derived here, never accepted
    with pytest.raises(NotImplementedError, match="expand_tag_mask"):
        run(LF.options(isTrain=False, expand_tag_mask=True))
    assert launches() == []


# ---- 4. the batches feed the model's modes -------------------------------------------------------------------------------------------------------
def _files(n, size, seed):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(size), torch.arange(size), indexing="ij")
    label = (((yy - size // 2) ** 2 + (xx - size // 2 + 3) ** 2) < (size // 3) ** 2).to(torch.uint8).expand(n, size, size).contiguous()
    orient = torch.randint(0, 256, (n, size, size), generator=g).to(torch.uint8) * label
    return torch.randint(0, 256, (n, size, size, 3), generator=g, dtype=torch.uint8), label, orient


def _model_options(**over):
    from oracle import trainer_parity as TP
    return TP.repo_options(dict(TP.CFGS["A"], ngf=8, ndf=8, crop=64), load_size=68, **over)


def test_an_unpaired_batch_trains_the_model_at_step_two(emulator_backend):
    from michigan_amd import inputs
    from michigan_amd.model import Pix2PixModel
    opt = _model_options(unpairTrain=True, curr_step=2)
    torch.manual_seed(0)
    model = Pix2PixModel(opt)
    image, label, orient = _files(1, 72, 1)
    image_ref, label_ref, _ = _files(1, 80, 2)
    data = inputs.DeviceInputPipeline(opt, "cpu", rng=random.Random(3), generator=LF.generator("cpu"))(image, label, orient, image_ref=image_ref,
                                                                                                        label_ref=label_ref)
    assert data["image_ref"].shape == (1, 3, 64, 64) and not torch.equal(data["image_ref"], data["image_tag"])
    batch = {k: v for k, v in data.items() if torch.is_tensor(v)}           # the DataLoader's collate makes tensors of `instance` / `hole`
    losses, fake = model(batch, mode="generator")
    assert set(losses) == {"GAN", "ORIENT", "hairAvgLab", "background"}
    assert fake.shape == (1, 3, 64, 64) and bool(torch.isfinite(fake.float()).all())
    assert all(bool(torch.isfinite(v.detach().float()).all()) for v in losses.values())


def test_an_inference_batch_runs_mode_inference(emulator_backend):
    from michigan_amd import inputs
    from michigan_amd.model import Pix2PixModel
    opt = _model_options(isTrain=False)
    torch.manual_seed(0)
    model = Pix2PixModel(opt).eval()
    image_tag, label_tag, orient_tag = _files(1, 72, 4)
    image_ref, label_ref, _ = _files(1, 80, 5)
    data = inputs.inference_batch(opt, image_ref=image_ref[0], image_tag=image_tag[0], label_ref=label_ref[0], label_tag=label_tag[0],
                                  orient_tag=orient_tag[0], orient_ref=orient_tag[0], orient_mask=label_tag[0], same_orient=True,
                                  rng=random.Random(5), generator=LF.generator("cpu"))
    out = model(data, mode="inference")
    assert out.shape == (1, 3, 64, 64) and bool(torch.isfinite(out.float()).all())
