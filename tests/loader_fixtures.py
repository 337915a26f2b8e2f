"""Helpers of tests/test_loader_batches.py (CPU, contract emulator) and tests/test_gpu_loader_batches.py (-m gpu): the fixtures that
tools/make_loader_golden.py recorded from the reference's own loader functions (tests/golden/loader_{unpaired,inference,demo}.npz),
a `random.Random` stand-in that replays the draws those functions made, and one runner per batch kind.

Comparison rule (compare): the key set is the reference's without `path`; every tensor is torch.equal to the recorded one, dtype and
shape included -- label, hole and orientation maps are byte-exact restatements, image and orient_rgb floats are single IEEE operations
in the reference's order (the contract mg_input_crop_u8 states).  `noise` is the exception (check_noise): its cv2.resize leg is not
pinned anywhere (OpenCV is not installed where the fixtures are made), so it is compared with inputs.noise_from_fields on the same
fields, and the recorded fields with the recorded result at the bar tests/test_gpu_inputs.py already states for that kernel."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LOAD, CROP, ADD_TH, LABEL_NC = 32, 24, 8, 2
NOISE_ATOL_HIP = 1e-6                        # tests/test_gpu_inputs.py::test_noise_octaves_match_oracle; 0 on the emulator (the same function)
_CACHE = {}


def load(kind):
    """{case: {"src": {name: u8 array}, "draws": {name: array}, "fields": float64 [N, L], "want": {key: array}}}, read once"""
    if kind not in _CACHE:
        z = np.load(os.path.join(GOLDEN, "loader_%s.npz" % kind))
        out = {}
        for k in z.files:
            parts = k.split("/")
            if len(parts) == 1:
                continue
            rec = out.setdefault(parts[0], {"src": {}, "draws": {}, "want": {}})
            if len(parts) == 2:
                rec[parts[1]] = z[k]
            else:
                rec[parts[1]][parts[2]] = z[k]
        _CACHE[kind] = out
    return _CACHE[kind]


class ReplayRng:
    """the part of random.Random the loaders use, returning the reference's recorded draws in the order the loaders ask for them:
    per sample randint x, randint y, random (flip); then per sample uniform (th); then per sample random (u)"""

    def __init__(self, draws, hole):
        n = len(draws["x"])
        q = []
        for i in range(n):
            q += [("randint", int(draws["x"][i])), ("randint", int(draws["y"][i])), ("random", float(draws["flip"][i]))]
        if hole:
            q += [("uniform", float(v)) for v in draws["th"]] + [("random", float(v)) for v in draws["u"]]
        self.queue = q

    def _next(self, kind):
        assert self.queue, "the loader drew more than the reference did (%s)" % kind
        k, v = self.queue.pop(0)
        assert k == kind, "the loader asked for %s where the reference drew %s" % (kind, k)
        return v

    def randint(self, a, b):
        v = self._next("randint")
        assert a <= v <= b
        return v

    def random(self):
        return self._next("random")

    def uniform(self, a, b):
        v = self._next("uniform")
        assert a <= v <= b
        return v

    def done(self):
        assert not self.queue, "draws of the reference the loader never asked for: %s" % self.queue


def options(**over):
    from michigan_amd.model import default_options
    return default_options(**dict(dict(crop_size=CROP, load_size=LOAD, use_ig=True, label_nc=LABEL_NC, add_th=ADD_TH, gpu_ids=[]), **over))


def generator(device, seed=1):
    return torch.Generator(device=device).manual_seed(seed)


def sources(case, device):
    return {k: torch.from_numpy(v).to(device) for k, v in case["src"].items()}


def compare(got, want, skip=("noise",)):
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k, w in want.items():
        if k in skip:
            continue
        g = got[k]
        w = torch.from_numpy(np.asarray(w))
        if not torch.is_tensor(g):                                   # the dataset's `instance` (and `hole` without use_ig): a plain 0
            assert w.dim() == 0 and type(g) is int and g == int(w), (k, g)
            continue
        assert g.dtype == w.dtype and tuple(g.shape) == tuple(w.shape), (k, g.dtype, tuple(g.shape), w.dtype, tuple(w.shape))
        assert torch.equal(g.cpu(), w), "%s: %d of %d elements differ, max abs %.3e" % (
            k, int((g.cpu() != w).sum()), w.numel(), float((g.cpu().double() - w.double()).abs().max()))


def check_noise(data, case, device, seed=1):
    from michigan_amd import _cabi, inputs
    want = torch.from_numpy(case["want"]["noise"])
    n = want.shape[0]
    assert data["noise"].dtype == want.dtype and tuple(data["noise"].shape) == tuple(want.shape)
    fields = torch.randn((n, inputs.noise_field_len(CROP)), dtype=torch.float64, device=device, generator=generator(device, seed)) * 0.25 + 0.5
    assert torch.equal(data["noise"], inputs.noise_from_fields(fields, CROP)), "noise is not generate_noise of the generator's fields"
    ref = inputs.noise_from_fields(torch.from_numpy(case["fields"]).to(device), CROP).cpu()
    atol = NOISE_ATOL_HIP if _cabi.backend().name == "hip" else 0.0
    assert float((ref - want).abs().max()) <= atol, float((ref - want).abs().max())


def run_unpaired(device, refs=True, case=None, as_list=False):
    from michigan_amd import inputs
    case = case or load("unpaired")["step2"]
    s = sources(case, device)
    rng = ReplayRng(case["draws"], hole=True)
    pipe = inputs.DeviceInputPipeline(options(isTrain=True, no_flip=False), device, rng=rng, generator=generator(device))
    kw = {}
    if refs:
        kw = dict(image_ref=s["image_ref"], label_ref=s["label_ref"])
        if as_list:
            kw = {k: list(v) for k, v in kw.items()}
    data = pipe(s["image"], s["label"], s["orient"], s["orient_mask"], **kw)
    rng.done()
    return data, case


def run_inference(name, device, **over):
    from michigan_amd import inputs
    case = load("inference")[name]
    same, zeros = name.startswith("same"), name.endswith("zeros")
    rng = ReplayRng(case["draws"], hole=same and over.get("use_ig", True))
    data = inputs.inference_batch(options(isTrain=False, add_zeros=zeros, **over), same_orient=same, rng=rng, generator=generator(device),
                                  **sources(case, device))
    rng.done()
    return data, case


def run_demo(name, device):
    from michigan_amd import inputs
    case = load("demo")[name]
    rng = ReplayRng(case["draws"], hole=False)
    data = inputs.demo_batch(options(isTrain=False), rng=rng, generator=generator(device), **sources(case, device))
    rng.done()
    return data, case


INFERENCE_CASES = ("same_plain", "same_zeros", "other_plain", "other_zeros")
DEMO_CASES = ("plain", "strokes")
