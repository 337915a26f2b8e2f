"""CPU: michigan_amd.data -- a dataset directory as batches -- on the contract emulator.

  1  list_dataset against the order the REFERENCE's own CustomDataset.initialize listed the same directory in
     (tests/golden/dataset_listing.json from tools/make_dataset_golden.py: names only), and its errors;
  2  ResidentDataset: the decoded tensors bit for bit, the refusals, and batch() bit-identical, key by key, to a hand-made call of
     DeviceInputPipeline whose indices come from a second random.Random consumed in the documented order;
  3  EpochLoader: batches per epoch, epoch orders, serial order, and the rank split.
The same batches run on the device in tests/test_gpu_train_driver.py."""
import json
import os
import random

import numpy as np
import pytest
import torch

import dataset_fixtures as DF
from oracle import trainer_parity as TP

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dataset_listing.json")
STEMS = ("a0", "a1", "a2", "a3", "a4")


def loader_options(root, **over):
    o = dict(vars(DF.dataset_options(root)), load_size=72, no_flip=False, preprocess_mode="resize_and_crop")
    o.update(over)
    return TP.repo_options(dict(TP.CFGS["A"], ngf=8, ndf=8, crop=64), **o)


# ---- 1. listing -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", DF.LISTING_CASES)
def test_listing_is_the_references(tmp_path, case):
    from michigan_amd import data
    with open(GOLDEN) as f:
        want = json.load(f)[case]
    over = DF.write_listing_dir(str(tmp_path), case)
    got = data.list_dataset(DF.dataset_options(tmp_path, **over))
    assert DF.names(got) == want
    assert all(os.path.isabs(p) and os.path.isfile(p) for v in got.values() for p in v)
    if case == "walk":                                     # the upper-case extension of the list is taken, the others are not
        assert "3.PNG" in want["label"] and not any(n.startswith(("9.", "notes")) for n in want["label"])
        assert len(want["label"]) == len(DF.LISTING_STEMS) + 1


def test_listing_errors(tmp_path):
    from michigan_amd import data
    root = str(tmp_path)
    DF.write_dataset(root, ("1", "2", "3"))
    opt = lambda **over: DF.dataset_options(root, **over)
    assert len(data.list_dataset(opt())["label"]) == 3
    for key in ("no_orientation",):
        with pytest.raises(ValueError, match=key):
            data.list_dataset(opt(**{key: True}))
    with pytest.raises(ValueError, match="no_instance"):
        data.list_dataset(opt(no_instance=False))
    # label / image stems
    os.rename(os.path.join(root, "train_images", "2.png"), os.path.join(root, "train_images", "2x.png"))
    with pytest.raises(ValueError, match="label-image pair"):
        data.list_dataset(opt())
    assert DF.names(data.list_dataset(opt(no_pairing_check=True)))["image"] == ["1.png", "2x.png", "3.png"]
    os.rename(os.path.join(root, "train_images", "2x.png"), os.path.join(root, "train_images", "2.png"))
    # orientation stems: the reference pairs these by sort order alone
    od = os.path.join(root, "train_dense_orients")
    os.rename(os.path.join(od, "3_orient_dense.png"), os.path.join(od, "4_orient_dense.png"))
    with pytest.raises(ValueError, match="label-orientation pair"):
        data.list_dataset(opt())
    assert DF.names(data.list_dataset(opt(no_pairing_check=True)))["orient"][-1] == "4_orient_dense.png"
    os.rename(os.path.join(od, "4_orient_dense.png"), os.path.join(od, "3.png"))              # the bare stem is accepted too
    assert DF.names(data.list_dataset(opt()))["orient"][-1] == "3.png"
    # counts
    os.remove(os.path.join(root, "train_images", "1.png"))
    with pytest.raises(ValueError, match="do not match"):
        data.list_dataset(opt())
    with pytest.raises(ValueError, match="do not match"):
        data.list_dataset(opt(no_pairing_check=True))
    with pytest.raises(ValueError, match="not a valid directory"):
        data.list_dataset(opt(label_dir="nowhere"))


# ---- 2. ResidentDataset ---------------------------------------------------------------------------------------------------------------
@pytest.fixture
def five(tmp_path):
    return str(tmp_path), DF.write_dataset(str(tmp_path), STEMS, seed=3)


def test_decoded_tensors_are_the_files(emulator_backend, five):
    from michigan_amd import data
    root, samples = five
    ds = data.ResidentDataset(loader_options(root), "cpu")
    assert len(ds) == 5 and ds.image.dtype == ds.label.dtype == ds.orient.dtype == torch.uint8
    assert tuple(ds.image.shape) == (5, 24, 24, 3) and tuple(ds.label.shape) == tuple(ds.orient.shape) == (5, 24, 24)
    for i, (label, orient, image) in enumerate(samples):
        assert np.array_equal(ds.label[i].numpy(), label) and np.array_equal(ds.orient[i].numpy(), orient)
        assert np.array_equal(ds.image[i].numpy(), image)
    assert ds.nbytes == 5 * 24 * 24 * 5
    assert set(ds.label.unique().tolist()) == {0, 1}
    with pytest.raises(ValueError, match="resident"):
        data.ResidentDataset(loader_options(root), "cpu", resident="disk")


def test_mixed_sizes_and_wrong_channels_name_the_file(emulator_backend, five):
    from michigan_amd import data
    root, _ = five
    path = os.path.join(root, "train_labels", "a2.png")
    DF.save(path, DF.sample(1, size=20)[0])
    with pytest.raises(ValueError, match="a2.png"):
        data.ResidentDataset(loader_options(root), "cpu")
    DF.save(path, DF.sample(1)[2])                                              # three channels where one is expected
    with pytest.raises(ValueError, match=r"a2\.png.*one 8-bit channel"):
        data.ResidentDataset(loader_options(root), "cpu")
    DF.save(path, DF.sample(1)[0])
    other = os.path.join(root, "train_images", "a3.png")
    DF.save(other, np.zeros((20, 24, 3), np.uint8))
    with pytest.raises(ValueError, match="a3.png"):
        data.ResidentDataset(loader_options(root), "cpu")


def hand_made(opt, ds, index, step, seed, device="cpu"):
    """batch(index) written out: the index draws from a random.Random(seed) in the documented order (per sample: index_ref at step 2,
    then index_orient_ref), then ONE DeviceInputPipeline call on the same generator state"""
    from michigan_amd.inputs import DeviceInputPipeline
    rng = random.Random(seed)
    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    m, refs, orefs = len(ds), [], []
    for i in index:
        refs.append(rng.randint(0, m - 1) if step == 2 else i)
        orefs.append(rng.randint(0, m - 1))
    to = lambda t, idx: t[torch.tensor(idx)].to(device)
    kw = dict(image_ref=to(ds.image, refs), label_ref=to(ds.label, refs)) if step == 2 else {}
    data = DeviceInputPipeline(opt, device, rng=rng, generator=gen)(
        to(ds.image, index), to(ds.label, index), to(ds.orient, index), orient_mask=to(ds.label, orefs), **kw)
    return data, refs, orefs


def same_batch(got, want, skip=()):
    assert set(got) - {"path", "_indices"} == set(want)
    for k, v in want.items():
        if k in skip:
            continue
        if torch.is_tensor(v):
            assert torch.is_tensor(got[k]) and got[k].dtype == v.dtype and torch.equal(got[k].cpu(), v.cpu()), k
        else:
            assert type(got[k]) is type(v) and got[k] == v, k


@pytest.mark.parametrize("resident", ["device", "host"])
@pytest.mark.parametrize("use_ig", [True, False])
@pytest.mark.parametrize("step", [1, 2])
def test_batch_is_one_pipeline_call(emulator_backend, five, step, use_ig, resident):
    from michigan_amd import data
    root, _ = five
    opt = loader_options(root, use_ig=use_ig, inpaint_orient=False)
    seed = 11 + step
    gen = torch.Generator()
    gen.manual_seed(seed)
    ds = data.ResidentDataset(opt, "cpu", step=step, rng=random.Random(seed), generator=gen, resident=resident)
    got = ds.batch([4, 1])
    want, refs, orefs = hand_made(opt, ds, [4, 1], step, seed)
    same_batch(got, want)
    assert got["_indices"] == {"index": [4, 1], "index_ref": refs, "index_orient_ref": orefs}
    assert got["path"] == [os.path.join(root, "train_images", STEMS[i] + ".png") for i in refs]
    assert tuple(got["image_tag"].shape) == (2, 3, 64, 64) and tuple(got["label_tag"].shape) == (2, 1, 64, 64)
    if step == 1:
        assert got["label_ref"] is got["label_tag"] and got["image_ref"] is got["image_tag"] and refs == [4, 1]
    else:
        assert got["label_ref"] is not got["label_tag"]
    if use_ig:
        assert tuple(got["hole"].shape) == (2, 1, 64, 64) and tuple(got["orient_rgb"].shape) == (2, 3, 64, 64)
    # the second batch goes on from the same generators
    again = ds.batch([0, 2])
    assert not torch.equal(again["noise"], got["noise"])


def test_index_draws_stay_in_range_and_the_step_view_shares_the_bytes(emulator_backend, five):
    from michigan_amd import data
    root, _ = five
    ds = data.ResidentDataset(loader_options(root, use_ig=False), "cpu", step=1, rng=random.Random(5))
    two = ds.at_step(2)
    assert two.step == 2 and ds.step == 1 and two.image is ds.image and two.pipeline is ds.pipeline
    seen_ref, seen_orient = set(), set()
    for _ in range(40):
        d = two.batch([0, 1, 2, 3, 4])["_indices"]
        seen_ref.update(d["index_ref"])
        seen_orient.update(d["index_orient_ref"])
    assert seen_ref == seen_orient == {0, 1, 2, 3, 4}                           # randint(0, M - 1): both ends, nothing outside
    with pytest.raises(IndexError):
        ds.batch([5])
    with pytest.raises(IndexError):
        ds.batch([])


# ---- 3. EpochLoader -------------------------------------------------------------------------------------------------------------------
class Counted:
    """a dataset that returns the indices it was asked for"""

    def __init__(self, m):
        self.m = m

    def __len__(self):
        return self.m

    def batch(self, index):
        return list(index)


def test_epoch_loader_batches_and_orders():
    from michigan_amd.data import EpochLoader
    ld = EpochLoader(Counted(5), 2, shuffle=True, drop_last=True, seed=3)
    first = list(ld)
    assert len(ld) == 2 and [len(b) for b in first] == [2, 2] and len({i for b in first for i in b}) == 4
    keep = EpochLoader(Counted(5), 2, shuffle=True, drop_last=False, seed=3)
    got = list(keep)
    assert len(keep) == 3 and [len(b) for b in got] == [2, 2, 1] and sorted(i for b in got for i in b) == [0, 1, 2, 3, 4]
    assert got[:2] == first                                                     # the same seed and epoch: the same order
    orders = []
    for e in (1, 2, 1):
        keep.set_epoch(e)
        orders.append([i for b in keep for i in b])
    assert orders[0] == orders[2] and orders[0] != orders[1]
    assert orders[0] == torch.randperm(5, generator=torch.Generator().manual_seed((3 * 1000003 + 1) % (1 << 63))).tolist()
    other = EpochLoader(Counted(64), 2, shuffle=True, drop_last=True, seed=4)
    mine = EpochLoader(Counted(64), 2, shuffle=True, drop_last=True, seed=3)
    assert list(other) != list(mine)
    serial = EpochLoader(Counted(5), 2, shuffle=False, drop_last=False, seed=3)
    serial.set_epoch(7)
    assert list(serial) == [[0, 1], [2, 3], [4]]
    assert isinstance(EpochLoader(Counted(5), 2, shuffle=True, drop_last=True).seed, int)          # default: the job-shared host RNG
    with pytest.raises(ValueError):
        EpochLoader(Counted(5), 2, shuffle=True, drop_last=True, rank=2, world=2)


@pytest.mark.parametrize("world", [2, 4])
def test_epoch_loader_rank_split(world):
    from michigan_amd.data import EpochLoader
    m, bs = 18, 2                                                               # 18: the tail past a multiple of world * bs is dropped
    single = EpochLoader(Counted(m), bs, shuffle=True, drop_last=True, seed=9)
    single.set_epoch(2)
    order = [i for b in single for i in b]
    ranks = []
    for r in range(world):
        ld = EpochLoader(Counted(m), bs, shuffle=True, drop_last=False, seed=9, rank=r, world=world)
        ld.set_epoch(2)
        batches = list(ld)
        assert len(batches) == len(ld) == m // (world * bs) and all(len(b) == bs for b in batches)
        ranks.append(batches)
    flat = [[i for b in batches for i in b] for batches in ranks]
    assert all(len(f) == len(flat[0]) for f in flat)
    assert len({i for f in flat for i in f}) == sum(len(f) for f in flat)                        # disjoint
    usable = m // (world * bs) * (world * bs)
    assert {i for f in flat for i in f} == set(order[:usable])                                   # the documented prefix
    for k in range(len(ranks[0])):                                              # global step k = batches k*world ... of the order
        assert [i for r in range(world) for i in ranks[r][k]] == order[k * world * bs:(k + 1) * world * bs]


def test_epoch_loader_on_sixteen_samples_is_even():
    from michigan_amd.data import EpochLoader
    for world in (2, 4):
        sets = [[i for b in EpochLoader(Counted(16), 2, shuffle=True, drop_last=True, seed=1, rank=r, world=world) for i in b]
                for r in range(world)]
        assert all(len(s) == 16 // world for s in sets) and sorted(i for s in sets for i in s) == list(range(16))
