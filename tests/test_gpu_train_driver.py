"""-m gpu: the resident dataset and the two native drivers on the device, at ngf 8 / ndf 8 / crop 64 / load 72 (the smallest geometry the
generator accepts at num_upsampling_layers='more') over the 5-sample dataset of tests/dataset_fixtures.py.

  1  ResidentDataset.batch on the device against the same call on the contract emulator with the same draws, at steps 1 and 2: every key
     bit-identical except `noise` -- whose fields come from the device's generator -- which is the device generator's own fields through
     mg_noise_octaves bit for bit, and within tests/test_gpu_inputs.py's noise tolerance (1e-6) of the emulator on those fields;
  2  `train.train` end to end in fp32 and bf16 (losses finite, weights and the power iteration moved, the checkpoint reloads, a resumed
     run continues from iter.txt), and bit-reproducible under deterministic weight gradients;
  3  the inference driver: the saved PNG is generate()'s tensor, which is tensor2im of the model's output.
The host logic of all three is covered on the CPU (tests/test_data_resident.py, tests/test_train_driver.py)."""
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

import dataset_fixtures as DF
from oracle import trainer_parity as TP

pytestmark = pytest.mark.gpu

STEMS = ("a0", "a1", "a2", "a3", "a4")
NOISE_ATOL = 1e-6                                           # tests/test_gpu_inputs.py::test_noise_octaves_match_oracle


def loader_options(root, **over):
    o = dict(vars(DF.dataset_options(root)), load_size=72, no_flip=False, preprocess_mode="resize_and_crop")
    o.update(over)
    return TP.repo_options(dict(TP.CFGS["A"], ngf=8, ndf=8, crop=64), **o)


# ---- 1 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resident", ["device", "host"])
@pytest.mark.parametrize("step", [1, 2])
def test_batch_on_the_device_is_the_emulators(hip_backend, tmp_path, step, resident):
    from michigan_amd import _cabi, data, inputs
    from oracle.cabi_emulator import EmulatorBackend
    root = str(tmp_path)
    DF.write_dataset(root, STEMS, seed=3)
    opt = loader_options(root, use_ig=True, inpaint_orient=False)
    seed = 20 + step

    def two_batches(device, where):
        gen = torch.Generator(device=device)
        gen.manual_seed(seed)
        ds = data.ResidentDataset(opt, device, step=step, rng=random.Random(seed), generator=gen, resident=where)
        return ds, [ds.batch([4, 1]), ds.batch([0, 2, 3])]

    ds, got = two_batches("cuda", resident)
    torch.cuda.synchronize()
    assert ds.image.is_cuda == (resident == "device") and (resident == "device" or ds.image.is_pinned())
    prev = _cabi.set_backend(EmulatorBackend())
    try:
        _, want = two_batches("cpu", "device")
        gen = torch.Generator(device="cuda")
        gen.manual_seed(seed)
        for g, w in zip(got, want):
            assert set(g) == set(w) and g["_indices"] == w["_indices"] and g["path"] == w["path"]
            for k, v in w.items():
                if k in ("noise", "_indices", "path"):
                    continue
                if torch.is_tensor(v):
                    assert g[k].is_cuda == (v.dim() > 0) and g[k].dtype == v.dtype and torch.equal(g[k].cpu(), v), k
                else:
                    assert type(g[k]) is type(v) and g[k] == v, k
            n = g["noise"].shape[0]
            fields = torch.randn((n, inputs.noise_field_len(64)), dtype=torch.float64, device="cuda", generator=gen) * 0.25 + 0.5
            ref = inputs.noise_from_fields(fields.cpu(), 64)                            # the emulator, on the device's fields
            assert g["noise"].dtype == torch.float32 and tuple(g["noise"].shape) == (n, 3, 64, 64)
            err = float((g["noise"].cpu() - ref).abs().max())
            print("step %d %s: noise max abs err vs the emulator %.3e" % (step, resident, err))
            assert err <= NOISE_ATOL, err
            _cabi.set_backend(None)
            assert torch.equal(g["noise"], inputs.noise_from_fields(fields, 64)), "noise is not mg_noise_octaves of the generator's fields"
            _cabi.set_backend(EmulatorBackend())
            assert float(g["hole"].max()) > 0 and float(g["orient_rgb"].max()) > 0
        if step == 2:
            assert got[0]["label_ref"] is not got[0]["label_tag"]
    finally:
        _cabi.set_backend(prev)


# ---- 2 --------------------------------------------------------------------------------------------------------------------------------
def run(root, ck, name, dtype, *extra):
    from michigan_amd import train
    return train.train(train.parse(DF.small_argv(root, ck, name, "--compute_dtype", dtype, "--gpu_ids", 0, "--batchSize", 2, "--seed", 5,
                                                 "--print_freq", 2, "--save_latest_freq", 4, *extra)))


def iter_txt(ck, name):
    with open(os.path.join(ck, name, "iter.txt")) as f:
        return tuple(int(v) for v in f.read().split())


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_train_driver_end_to_end(hip_backend, tmp_path, dtype):
    from michigan_amd import train
    from michigan_amd.model import Pix2PixTrainer
    root, ck = str(tmp_path / "data"), str(tmp_path / "ck")
    DF.write_dataset(root, STEMS, seed=3)
    out = run(root, ck, "t", dtype, "--niter", 2)
    assert out["epochs"] == 2 and out["iterations"] == 4 and out["images_per_s"] > 0
    assert set(out["losses"]) == {"GAN", "GAN_Feat", "VGG", "ORIENT", "D_Fake", "D_real"}
    print(dtype, out)
    assert all(np.isfinite(v) for v in out["losses"].values()), out["losses"]
    assert iter_txt(ck, "t") == (3, 0)
    load = lambda epoch, net: torch.load(os.path.join(ck, "t", "%s_net_%s.pth" % (epoch, net)))
    for net in ("G", "D"):
        one, two = load(1, net), load(2, net)
        assert all(bool(torch.isfinite(v).all()) for v in two.values() if v.is_floating_point()), net
        moved = [k for k in one if not torch.equal(one[k], two[k])]
        assert any(k.endswith(("weight", "weight_orig")) for k in moved) and any(k.endswith("weight_u") for k in moved), (net, moved[:5])
    # the checkpoint reloads into a fresh trainer
    opt = train.parse(DF.small_argv(root, ck, "t", "--compute_dtype", dtype, "--gpu_ids", 0))
    torch.manual_seed(99)
    fresh = Pix2PixTrainer(opt)
    latest = load("latest", "G")
    assert any(not torch.equal(v.cpu(), latest[k]) for k, v in fresh.pix2pix_model.netG.state_dict().items())
    fresh.load("latest")
    assert all(torch.equal(v.cpu(), latest[k]) for k, v in fresh.pix2pix_model.netG.state_dict().items())
    assert all(torch.equal(v.cpu(), load("latest", "D")[k]) for k, v in fresh.pix2pix_model.netD.state_dict().items())
    del fresh
    # resumed from iter.txt: epoch 3 only
    out = run(root, ck, "t", dtype, "--niter", 3, "--continue_train")
    assert out["epochs"] == 1 and out["iterations"] == 2 and iter_txt(ck, "t") == (4, 0)
    assert all(np.isfinite(v) for v in out["losses"].values()), out["losses"]
    three = load(3, "G")
    assert any(not torch.equal(three[k], latest[k]) for k in latest)


def test_two_runs_from_the_same_seeds_are_bitwise_equal(hip_backend, tmp_path):
    from michigan_amd import ops
    root = str(tmp_path / "data")
    DF.write_dataset(root, STEMS, seed=3)
    prev = ops.set_deterministic(True)                        # what MG_DETERMINISTIC=1 sets at import
    try:
        files = []
        for name in ("a", "b"):
            ck = str(tmp_path / name)
            run(root, ck, "t", "bf16", "--niter", 1)
            files.append({net: torch.load(os.path.join(ck, "t", "latest_net_%s.pth" % net)) for net in ("G", "D")})
    finally:
        ops.set_deterministic(prev)
    for net in ("G", "D"):
        differ = [k for k, v in files[0][net].items() if not torch.equal(v, files[1][net][k])]
        assert not differ, (net, differ[:5])


# ---- 3 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zeros", [False, True], ids=["plain", "add_feat_zeros"])
def test_inference_driver_writes_what_generate_returns(hip_backend, tmp_path, zeros):
    from michigan_amd import inference
    from michigan_amd.inputs import DeviceInputPipeline
    from michigan_amd.model import Pix2PixModel
    root, ck, results = str(tmp_path / "data"), str(tmp_path / "ck"), str(tmp_path / "out")
    samples = dict(zip("rto", DF.write_dataset(root, ("r", "t", "o"), seed=6, subset="val", image_ext=".jpg")))
    argv = DF.small_argv(root, ck, "i", "--compute_dtype", "fp32", "--gpu_ids", 0, "--load_size", 64, "--which_epoch", 7, "--results_dir", results,
                         "--batchSize", 2, "--seed", 8, *(("--add_feat_zeros",) if zeros else ()))
    opt = inference.parse(argv)
    torch.manual_seed(2)
    Pix2PixModel(opt).save("7")
    model = inference.build_model(opt)
    assert next(model.parameters()).is_cuda and not model.training
    triples = [("r", "t", "o"), ("o", "r", "t")]              # one batch of two: neither takes the orientation of its own target

    def seeded():
        gen = torch.Generator(device="cuda")
        gen.manual_seed(8)
        return dict(rng=random.Random(8), generator=gen)

    got = inference.generate(opt, model, triples, **seeded())
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (2, 64, 64, 3)
    # by hand: the same batch through the pipeline and the model, tensor2im with torch ops
    t = lambda k, pick: torch.stack([torch.from_numpy(samples[pick(tr)][k]) for tr in triples])
    ref, tag, ori = (lambda tr: tr[0]), (lambda tr: tr[1]), (lambda tr: tr[2])
    data = DeviceInputPipeline(opt, "cuda", **seeded()).inference_batch(
        image_ref=t(2, ref), image_tag=t(2, tag), label_ref=t(0, ref), label_tag=t(0, tag), orient_tag=t(1, tag), orient_ref=t(1, ori),
        orient_mask=t(0, ori), same_orient=False)
    fake = model(data, "inference").float()
    assert tuple(fake.shape) == ((2, 3, 128, 128) if zeros else (2, 3, 64, 64)) and bool(torch.isfinite(fake).all())
    want = torch.clamp((fake + 1) / 2.0 * 255.0, 0, 255).to(torch.uint8).permute(0, 2, 3, 1)
    if zeros:
        want = want[:, 32:96, 32:96]
    assert torch.equal(got, want)
    assert np.array_equal(got.cpu().numpy(), (DF.tensor2im_reference(fake)[:, 32:96, 32:96] if zeros else DF.tensor2im_reference(fake)))
    assert int(got.max()) > int(got.min())
    # the command writes exactly that tensor
    pairs = str(tmp_path / "pairs.txt")
    with open(pairs, "w") as f:
        f.write("r t o\no r t\n")
    assert inference.main(argv + ["--pairs_file", pairs]) == 0
    assert sorted(os.listdir(results)) == ["r_from_o.png", "t_from_r.png"]
    for k, name in enumerate(("t_from_r.png", "r_from_o.png")):
        assert np.array_equal(np.array(Image.open(os.path.join(results, name))), got[k].cpu().numpy()), name
