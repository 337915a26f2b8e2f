"""-m gpu: the device loaders of the three batch kinds (DeviceInputPipeline with a reference slot, inputs.inference_batch,
inputs.demo_batch) through libmichigan_hip.so on the fixtures of tests/test_loader_batches.py -- what the reference's own loader
functions returned (tests/golden/loader_*.npz) -- with the same rule: torch.equal for every entry, `noise` through
loader_fixtures.check_noise.  One extra case has three reference samples of three stored sizes in one batch, which goes through a
table set per size; it is held to the contract emulator on identical buffers and to Pillow's own resize / crop / transpose."""
import random

import numpy as np
import pytest
import torch

import loader_fixtures as LF

pytestmark = pytest.mark.gpu


def test_unpaired_batch_on_the_device(hip_backend):
    for as_list in (False, True):
        data, case = LF.run_unpaired("cuda", as_list=as_list)
        torch.cuda.synchronize()
        assert all(v.is_cuda for k, v in data.items() if k not in ("instance",) and v.dim())
        LF.compare(data, case["want"])
    LF.check_noise(data, case, "cuda")


@pytest.mark.parametrize("name", LF.INFERENCE_CASES)
def test_inference_batch_on_the_device(hip_backend, name):
    data, case = LF.run_inference(name, "cuda")
    torch.cuda.synchronize()
    LF.compare(data, case["want"])
    LF.check_noise(data, case, "cuda")


def test_inference_batch_uploads_host_maps(hip_backend):
    """decoded files on the host: the batch is built on the current device all the same"""
    from michigan_amd import inputs
    case = LF.load("inference")["other_zeros"]
    data = inputs.inference_batch(LF.options(isTrain=False, add_zeros=True), same_orient=False, rng=LF.ReplayRng(case["draws"], hole=False),
                                  generator=LF.generator("cuda"), **LF.sources(case, "cpu"))
    torch.cuda.synchronize()
    assert data["image_tag"].is_cuda
    LF.compare(data, case["want"])


@pytest.mark.parametrize("name", LF.DEMO_CASES)
def test_demo_batch_on_the_device(hip_backend, name):
    data, case = LF.run_demo(name, "cuda")
    torch.cuda.synchronize()
    LF.compare(data, case["want"])
    LF.check_noise(data, case, "cuda")


def test_three_reference_sizes_in_one_batch():
    """40 x 36, 36 x 40 and 32 x 48 (one axis at the load size already: its index table is the identity, its bicubic pass a copy)"""
    from PIL import Image
    from michigan_amd import _cabi, inputs
    from oracle.cabi_emulator import EmulatorBackend
    case = LF.load("unpaired")["step2"]
    g = torch.Generator().manual_seed(17)
    tag = {k: torch.from_numpy(np.concatenate([v, v[:1]])) for k, v in case["src"].items() if k in ("image", "label", "orient", "orient_mask")}
    sizes = [(40, 36), (36, 40), (32, 48)]
    image_ref = [torch.randint(0, 256, s + (3,), generator=g, dtype=torch.uint8) for s in sizes]
    label_ref = [torch.randint(0, 2, s, generator=g, dtype=torch.uint8) for s in sizes]
    label_ref[2][10:20, 20:30] = 255
    outs = []
    for dev, be in (("cuda", None), ("cpu", EmulatorBackend())):
        prev = _cabi.set_backend(be)
        try:
            assert _cabi.backend().name == ("hip" if be is None else "emulator")
            pipe = inputs.DeviceInputPipeline(LF.options(), dev, rng=random.Random(23), generator=LF.generator(dev))
            outs.append(pipe(tag["image"], tag["label"], tag["orient"], tag["orient_mask"], image_ref=image_ref, label_ref=label_ref))
            if dev == "cuda":
                torch.cuda.synchronize()
        finally:
            _cabi.set_backend(prev)
    hip, emu = outs
    for k in ("image_ref", "label_ref", "image_tag", "label_tag", "orient", "orient_rgb", "hole"):
        assert hip[k].shape == emu[k].shape and torch.equal(hip[k].cpu(), emu[k]), k
    assert hip["image_ref"].shape == (3, 3, LF.CROP, LF.CROP) and float(hip["label_ref"][2].max()) == LF.LABEL_NC
    twin = random.Random(23)
    for i in range(3):                                               # the reference's own calls, on the box
        x, y, flip = twin.randint(0, LF.LOAD - LF.CROP), twin.randint(0, LF.LOAD - LF.CROP), twin.random() > 0.5
        img = Image.fromarray(image_ref[i].numpy()).resize((LF.LOAD, LF.LOAD), Image.BICUBIC).crop((x, y, x + LF.CROP, y + LF.CROP))
        lab = Image.fromarray(label_ref[i].numpy()).resize((LF.LOAD, LF.LOAD), Image.NEAREST).crop((x, y, x + LF.CROP, y + LF.CROP))
        if flip:
            img, lab = img.transpose(Image.FLIP_LEFT_RIGHT), lab.transpose(Image.FLIP_LEFT_RIGHT)
        want = torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1).float().div(255).sub_(0.5).div_(0.5)
        assert torch.equal(hip["image_ref"][i].cpu(), want), i
        want = torch.from_numpy(np.asarray(lab).copy())[None].float().div(255) * 255.0
        want[want == 255] = LF.LABEL_NC
        assert torch.equal(hip["label_ref"][i].cpu(), want), i
