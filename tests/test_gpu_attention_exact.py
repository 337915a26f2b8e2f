"""-m gpu: mg_self_attention (csrc/mg_attention.hip) held bit for bit where its value is exact, and to a per-element bound where it is not.

test_self_attention_matches_contract judges random operands by |hip - ref| <= tol * max|ref|, where max|ref| is set by the one planted row: every
other row is compared at more than half of its own size.  Nothing there pins what the kernel's layout rests on -- each P column meets the V row of
the same key (through the key-order gather of ds_read_tr16_b64 from the swizzled image), each key is counted exactly once (ragged last tile, both
half-waves, both LDS buffers), the rescale wipes exactly what it should.  Here (operands, references, the bound and its derivation:
tests/attention_operands.py):

  test_permutation_attention_is_a_gather          scores >= 128 apart: weights in {0, 1}, out == v[:, perm] (torch.equal), seven permutations that
                                                  put the selected key in the first, a middle and the last tile, before and after the query's
                                                  own, and -- over all lengths together -- at every key slot for every query lane
  test_class_attention_is_the_class_mean          equal scores inside power-of-two classes spread over the tiles: out == the once-rounded float64 mean
  test_strided_operands_and_untouched_neighbours  column slices at pitches 72 / 80 / 264, the output at a 4-element offset inside a sentinel-filled
                                                  buffer of pitch 264; the refusals of the entry point
  test_weighted_rows_stay_within_their_bound      realistic and cancelling ("pairs") operands: |hip - ref64| <= bound elementwise

L in {1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 257, 333} (32 / 64: the key tile of fp32 / bf16, 128: the query tile, from 129 on the ring
reuses a buffer, 1 and 31: one ragged tile) with N in {1, 3}, and L = 4096 once per dtype at N = 1.  neg = 1 puts every real score below 0, the
score of a key past L.  Wrong kernels are not run on the GPU: tests/test_attention_operands.py mutates a CPU model of the kernel instead and checks
that these comparisons reject each mutation.  MG_TEST_DRYRUN=1 runs the contract emulator in place of the GPU.

MEASURED (MI355X; worst error / bound over the elements of each case and the share of elements that differ from the once-rounded float64
reference, as printed by test_weighted_rows_stay_within_their_bound on lines marked "[hip]": the CPU model and the emulator print "[cpu model]"
and "[emulator]").  In bf16 the bound of an element whose interval [ref - b, ref + b] rounds
to a single value IS the rounding error of the reference: a ratio of 1.000 there says "every such element holds the once-rounded reference".
  realistic f32  N=3 L=129  scale=0.1    0.008   82.53 %          realistic bf16 N=3 L=129  scale=0.1    1.000   0.20 %
  realistic f32  N=3 L=129  scale=3.0    0.004   24.63 %          realistic bf16 N=3 L=129  scale=3.0    0.108   0.02 %
  realistic f32  N=3 L=200  scale=1.0    0.005   76.81 %          realistic bf16 N=3 L=200  scale=1.0    1.000   0.04 %
  realistic f32  N=1 L=4096 scale=0.35   0.003   95.42 %          realistic bf16 N=1 L=4096 scale=0.35   1.000   0.22 %
  pairs     f32  N=3 L=64                0.084   61.58 %          pairs     bf16 N=3 L=64                1.000   0.00 %
  pairs     f32  N=3 L=130               0.074   61.55 %          pairs     bf16 N=3 L=130               1.000   0.00 %
  pairs     f32  N=3 L=258               0.088   61.19 %          pairs     bf16 N=3 L=258               1.000   0.00 %
  pairs     f32  N=1 L=4096              0.081   61.30 %          pairs     bf16 N=1 L=4096              1.000   0.00 %
The fp32 ratios are what a worst-case (linear in the number of terms) accumulation bound leaves of a kernel whose errors add like a random walk;
nothing contradicts the assumed 2 ulp of v_exp_f32 (on "pairs" in fp32, where few keys count and that term is a large part of the bound, the
kernel uses 9 % of it).
"""
import functools
import os

import pytest
import torch

import attention_operands as A
import exact_operands as X

pytestmark = pytest.mark.gpu

DRY = os.environ.get("MG_TEST_DRYRUN") == "1"
DEV = "cpu" if DRY else "cuda"
N_LIST = (1, 3)
L_BIG = 4096
WEIGHTED = [("realistic", L, scale) for L, scale in A.REALISTIC] + [("pairs", L, 1.0) for L in A.PAIRS_L]
SENTINEL = {"f32": 0x7FC00A5A, "bf16": 0x7FC5}                  # quiet NaNs with a payload: no arithmetic produces them
INT = {"f32": torch.int32, "bf16": torch.int16}


def install_emulator():
    """The contract emulator (oracle/cabi_emulator.py); returns the backend it replaced."""
    from michigan_amd import _cabi
    from oracle.cabi_emulator import EmulatorBackend
    return _cabi.set_backend(EmulatorBackend())


@pytest.fixture
def backend(request):
    if not DRY:
        yield request.getfixturevalue("hip_backend")
        return
    request.getfixturevalue("emulator_backend")
    from michigan_amd import _cabi
    prev = install_emulator()
    yield
    _cabi.set_backend(prev)


class _Report:
    """Collects every mismatch of a case, so that one run names them all."""

    def __init__(self, quiet=False):
        self.failures, self.compared, self.lines, self.quiet = [], 0, [], quiet

    def _try(self, fn):
        self.compared += 1
        try:
            fn()
        except AssertionError as e:
            self.failures.append(str(e))

    def equal(self, tag, got, want):
        """torch.equal(got, want): the stored values, +0 and -0 alike."""
        self._try(lambda: X.assert_bits(tag, got, want.double(), want.dtype))

    def bits(self, tag, got, ref64, dtype):
        self._try(lambda: X.assert_bits(tag, got, ref64, dtype))

    def within(self, tag, got, ref64, bnd, who):
        """who: what computed `got` ("hip", "emulator", "cpu model"): printed, so that only a kernel's figures reach the MEASURED block."""
        got = got.detach().cpu()
        tag = f"[{who}] {tag}"
        rt = A.ratio(got, ref64, bnd)
        worst = float(rt.max())
        off = float((got != ref64.to(got.dtype)).double().mean())          # (bf16: the bound of an element whose interval rounds to one value IS its rounding error)
        self.lines.append(f"{tag}: worst error / bound {worst:.3f}, {off:.2%} of the elements differ from the once-rounded reference")
        if not self.quiet:
            print("MEASURED " + self.lines[-1])

        def check():
            bad = ~(rt <= 1)
            assert not bool(bad.any()), f"{tag}: {int(bad.sum())} of {rt.numel()} elements exceed their bound, the worst by a factor {worst:.4g}"
        self._try(check)
        return worst

    def done(self):
        assert not self.failures, "\n".join(self.failures[:40]) + f"\n({len(self.failures)} mismatches)"


def accepts(check):
    """True when a comparison of this file (`check(rep)`) passes: what tests/test_attention_operands.py asks about a mutant's output."""
    rep = _Report(quiet=True)
    check(rep)
    return not rep.failures


def run(o, dev):
    from michigan_amd import ops
    return ops.self_attention(o["q"].to(dev), o["k"].to(dev), o["v"].to(dev)).cpu()


# =====================================================================================================================
# the cases (each asserts the preconditions of its operands before it looks at a result)
# =====================================================================================================================
def gather_case(rep, dt, N, L, dev, perms=A.PERMS, negs=(0, 1), attend=run):
    for perm in perms:
        for neg in negs:
            o = A.gather_operands(dt, N, L, perm, neg)
            rep.equal(f"gather {dt} N={N} L={L} {perm} neg={neg}", attend(o, dev), o["ref"])


def class_case(rep, dt, N, L, dev, negs=(0, 1), attend=run):
    for neg in negs:
        o = A.class_operands(dt, N, L, neg)
        rep.bits(f"classes {dt} N={N} L={L} neg={neg}", attend(o, dev), o["ref"], A.DT[dt])


def strided(o, dt, dev):
    """(out, whole output buffer [N L + BQ, 264] as integers): q, k, v as column slices of wider tensors, out inside a sentinel-filled buffer
    that goes on for one query tile of rows behind the last sample's (where a store that forgot `qrow < L` would land)."""
    from michigan_amd import ops
    N, L = o["q"].shape[:2]
    wide = {}
    for name, pitch, at in (("q", 72, 8), ("k", 80, 16), ("v", 264, 8)):
        w = torch.full((N, L, pitch), 3.0, dtype=A.DT[dt])
        w[:, :, at:at + o[name].shape[2]] = o[name]
        wide[name] = w.to(dev)[:, :, at:at + o[name].shape[2]]
    buf = torch.full((N * L + A.BQ, 264), SENTINEL[dt], dtype=INT[dt]).to(dev)
    out = buf[:N * L].view(N, L, 264).view(A.DT[dt])[:, :, 4:4 + A.DV]
    assert [wide[n].stride(1) for n in "qkv"] == [72, 80, 264] and out.stride(1) == 264 and out.data_ptr() % 16 == 8 * (1 + (dt == "f32")) % 16
    ops.self_attention(wide["q"], wide["k"], wide["v"], out=out)
    return out.cpu(), buf.cpu()


def strided_case(rep, dt, L, dev, perms=A.PERMS, attend=strided):
    for perm in perms:
        o = A.gather_operands(dt, 3, L, perm, 1)
        tag = f"strided gather {dt} N=3 L={L} {perm}"
        out, buf = attend(o, dt, dev)
        rep.equal(tag, out, o["ref"])
        rep._try(lambda: neighbours_untouched(tag, buf, dt))


def neighbours_untouched(tag, buf, dt):
    rows = buf.shape[0] - A.BQ
    keep = torch.cat([buf[:rows, :4].reshape(-1), buf[:rows, 4 + A.DV:].reshape(-1), buf[rows:].reshape(-1)])
    bad = int((keep != SENTINEL[dt]).sum())
    assert bad == 0, f"{tag}: {bad} elements outside the output slice changed"


def refusal_case(dt):
    """No launch: every one of these is refused by the entry point's argument checks, with mg_last_error in the message."""
    from michigan_amd import ops
    t, odd = A.DT[dt], (68 if dt == "bf16" else 66)

    def z(*shape):
        return torch.zeros(shape, dtype=t, device="cuda")
    q, k, v = z(1, 8, 64), z(1, 8, 64), z(1, 8, 256)
    one = 4 // q.element_size()                                            # 4 bytes
    for what, said, call in (("a pitch that breaks 16-byte rows", "row pitches", lambda: ops.self_attention(z(1, 8, odd)[:, :, :64], k, v)),
                             ("ldo % 4 != 0", "row pitches", lambda: ops.self_attention(q, k, v, out=z(1, 8, 258)[:, :, :256])),
                             ("a q pointer off by 4 bytes", "misaligned pointer", lambda: ops.self_attention(z(1, 8, 72)[:, :, one:one + 64], k, v)),
                             ("d_qk != 64", "built for d_qk", lambda: ops.self_attention(z(1, 8, 32), z(1, 8, 32), v)),
                             ("N = 65536", "bad geometry", lambda: ops.self_attention(z(65536, 1, 64), z(65536, 1, 64), z(65536, 1, 256)))):
        with pytest.raises(RuntimeError, match="mg_self_attention failed.*mg_self_attention: " + said):      # the check it names, not another one
            call()
            pytest.fail(f"mg_self_attention accepted {what}")


@functools.lru_cache(maxsize=None)
def weighted_reference(kind, dt, L, scale):
    """(operands, float64 reference, bound), built once: the reference at L = 4096 is the cost of these tests."""
    N = 1 if L == L_BIG else 3
    o = A.weighted_operands(kind, dt, N, L, scale)
    ref, bnd = A.bound(o["q"], o["k"], o["v"], dt)
    if kind == "pairs":
        A.check_pairs(f"pairs {dt} L={L}", o, ref)
    return o, ref, bnd


def weighted_case(rep, kind, dt, L, scale, dev, attend=run, who=None):
    from michigan_amd import _cabi
    o, ref, bnd = weighted_reference(kind, dt, L, scale)
    tag = f"{kind} {dt} N={o['q'].shape[0]} L={L}" + (f" scale={scale}" if kind == "realistic" else "")
    return rep.within(tag, attend(o, dev), ref, bnd, who or _cabi.backend().name)


# =====================================================================================================================
# the tests
# =====================================================================================================================
@pytest.mark.parametrize("L", A.LENGTHS + (L_BIG,))
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_permutation_attention_is_a_gather(backend, dt, L):
    rep = _Report()
    if L == L_BIG:
        gather_case(rep, dt, 1, L, DEV, perms=("shuffle",), negs=(1,))
    else:
        for N in N_LIST:
            gather_case(rep, dt, N, L, DEV)
    rep.done()


@pytest.mark.parametrize("L", A.LENGTHS + (L_BIG,))
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_class_attention_is_the_class_mean(backend, dt, L):
    rep = _Report()
    for N in ((1,) if L == L_BIG else N_LIST):
        class_case(rep, dt, N, L, DEV)
    rep.done()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_strided_operands_and_untouched_neighbours(backend, dt):
    rep = _Report()
    for L in (65, 200):
        strided_case(rep, dt, L, DEV)
    rep.done()
    if not DRY:                                                            # (the emulator has no argument checks)
        refusal_case(dt)


@pytest.mark.parametrize("case", WEIGHTED, ids=lambda c: f"{c[0]}-L{c[1]}-x{c[2]:g}")
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_weighted_rows_stay_within_their_bound(backend, dt, case):
    rep = _Report()
    weighted_case(rep, case[0], dt, case[1], case[2], DEV)
    rep.done()
