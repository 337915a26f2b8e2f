"""CPU: the C-ABI shared library builds for gfx950, loads, and exports exactly what the headers under include/ declare; the ledger
of the one symbol table (michigan_amd/_cabi.py), the descriptor mirrors and the contract emulator (oracle/cabi_emulator.py)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib_path():
    from michigan_amd import build
    return build.build(verbose=False)


def _declared_symbols():
    """every mg_*( declared in a header under include/, sub-folders included, comments stripped"""
    names = set()
    for folder, _, files in os.walk(os.path.join(ROOT, "include")):
        for fn in files:
            if fn.endswith(".h"):
                src = open(os.path.join(folder, fn)).read()
                src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
                names |= set(re.findall(r"\b(mg_[a-z0-9_]+)\s*\(", src))
    return names


def test_library_exports_every_declared_symbol(lib_path):
    from michigan_amd import _cabi
    lib = ctypes.CDLL(lib_path)
    declared = _declared_symbols()
    assert len(declared) >= 20
    for name in declared | set(_cabi.EXPORTED_SYMBOLS):
        assert hasattr(lib, name), f"{name} declared in include/ but not exported"


def test_ctypes_mirror_matches_header(lib_path):
    """One table: what the headers under include/ declare is what michigan_amd/_cabi.py binds, each name once."""
    from michigan_amd import _cabi
    assert set(_cabi.EXPORTED_SYMBOLS) == _declared_symbols() == set(_cabi._PROTOS)
    assert len(_cabi.EXPORTED_SYMBOLS) == len(set(_cabi.EXPORTED_SYMBOLS))
    assert _cabi._NO_STATUS <= set(_cabi.EXPORTED_SYMBOLS)
    be = _cabi.HipBackend(lib_path)
    assert be.mg_abi_version() == _cabi.MG_ABI_VERSION
    with open(os.path.join(ROOT, "include", "michigan_hip.h")) as fh:
        assert re.search(r"#define\s+MG_ABI_VERSION\s+%d\b" % _cabi.MG_ABI_VERSION, fh.read())
    assert be.mg_stats_workspace(1, 8 * 512 * 512, 128) > 0
    with pytest.raises(AttributeError):
        be.mg_not_an_entry_point


def test_descriptor_mirrors_match_the_library(lib_path):
    from michigan_amd import _cabi
    be = _cabi.HipBackend(lib_path)
    mirrors = (_cabi.ConvDesc, _cabi.WgradDesc, _cabi.GradSlot, _cabi.PackJob, _cabi.SnLayer, _cabi.NormApply2Desc, _cabi.PyramidDesc,
               _cabi.FeatMomentDesc)
    assert _cabi.DESC_MIRRORS == mirrors
    assert [be.mg_sizeof_desc(which) for which in range(8)] == [ctypes.sizeof(m) for m in mirrors]
    assert be.mg_sizeof_desc(8) == -1
    # mg_feat_moment_desc by hand: 6 pointers, 4 int64, 4 int32, 3 pointers, no padding
    assert ctypes.sizeof(_cabi.FeatMomentDesc) == 6 * 8 + 4 * 8 + 4 * 4 + 3 * 8
    # by reference: exactly the entry points whose first parameter is a descriptor
    assert _cabi._BY_REF == {"mg_conv_taps", "mg_conv_wgrad", "mg_wgrad_det_workspace", "mg_norm_bwd_apply2", "mg_nearest_pyramid",
                             "mg_feat_moment_loss_fwd", "mg_feat_moment_loss_bwd"}


def test_emulator_mirrors_the_table():
    """The contract emulator implements the table, no more and no less, but for the collectives and the probes."""
    from michigan_amd import _cabi
    from oracle.cabi_emulator import EmulatorBackend
    emulated = {name for name in dir(EmulatorBackend) if name.startswith("mg_")}
    absent = {fn for fn in _cabi.EXPORTED_SYMBOLS if fn.startswith(("mg_comm_", "mg_allreduce_", "mg_probe_"))}
    assert len(absent) == 8
    assert emulated == set(_cabi.EXPORTED_SYMBOLS) - absent, sorted(emulated ^ (set(_cabi.EXPORTED_SYMBOLS) - absent))
    assert all(callable(getattr(EmulatorBackend, name)) for name in emulated)


def test_argument_validation_without_gpu(lib_path):
    """Entry points validate their arguments before touching the device: bad descriptors come back
    as error codes with a message (translated to RuntimeError), never as a crash."""
    from michigan_amd import _cabi
    be = _cabi.HipBackend(lib_path)
    d = _cabi.ConvDesc()
    with pytest.raises(RuntimeError, match="null tensor pointer"):
        be.mg_conv_taps(d, None)
    d.in_, d.wt, d.out = 64, 64, 64
    d.dtype, d.ntaps, d.Cin = _cabi.MG_BF16, 9, 12
    with pytest.raises(RuntimeError, match="multiple of 8"):
        be.mg_conv_taps(d, None)
    w = _cabi.WgradDesc()
    with pytest.raises(RuntimeError, match="null tensor pointer"):
        be.mg_conv_wgrad(w, None)
    with pytest.raises(RuntimeError, match="bad geometry"):
        be.mg_channel_stats(64, _cabi.MG_F32, 1, 100, 6, 1, 64, 64, None)
    # group (iv), collectives: arguments are checked before RCCL is even looked for
    with pytest.raises(RuntimeError, match="null"):
        be.mg_comm_unique_id(None)
    with pytest.raises(RuntimeError, match="null communicator"):
        be.mg_allreduce_stats(0, 64, 16, 1, None)
    with pytest.raises(RuntimeError, match="null communicator"):
        be.mg_allreduce_grads(0, 64, 16, None)


def test_kernels_are_gfx950_code_objects(lib_path):
    blob = open(lib_path, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in blob
    assert b"gfx942" not in blob and b"sm_" not in blob[:0]


def _header_options():
    src = open(os.path.join(ROOT, "include", "michigan_hip.h")).read()
    body = re.search(r"enum mg_option \{(.*?)\};", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return {name: int(num) for name, num in re.findall(r"\b(MG_OPT_[A-Z0-9_]+)\s*=\s*(\d+)", body)}


# defaults of the parent's definitions (the `int g_mg_* = N;` the table replaced), carried here as the pin
OPTION_DEFAULTS = {1: 1, 2: 1, 3: 1, 4: 1, 5: 1, 7: 1, 19: 1, 22: 1, 6: 2, 8: 2, 18: 32, 24: 64}
RETIRED_KEYS = (0, 9, 17)
PROBE_KEYS = (10, 12, 13, 14, 15, 21, 23)


def test_option_names_mirror_the_header():
    from michigan_amd import _cabi
    header = _header_options()
    mirror = {"MG_" + k: v for k, v in vars(_cabi).items() if k.startswith("OPT_")}
    assert len(header) >= len(OPTION_DEFAULTS) + len(PROBE_KEYS)
    assert mirror == header
    assert len(set(header.values())) == len(header), "two switches share a number"
    assert set(OPTION_DEFAULTS) | set(PROBE_KEYS) == set(header.values())
    probes = {v for k, v in header.items() if k.startswith("MG_OPT_PROBE_")}
    assert probes == set(PROBE_KEYS)


def test_options_defaults_ranges_and_gating(lib_path):
    """mg_get_option on a freshly loaded library returns the defaults; set checks the range and reads back; the product
    library refuses retired and MG_PROBES-only keys, by set and by get."""
    from michigan_amd import _cabi
    be = _cabi.HipBackend(lib_path)
    for key, want in OPTION_DEFAULTS.items():
        assert _cabi.get_option(key, be) == want, key

    def accepts(key, v):
        be.mg_set_option(key, v)
        assert _cabi.get_option(key, be) == v, (key, v)

    def refuses(key, v):
        before = _cabi.get_option(key, be) if key in OPTION_DEFAULTS else None
        with pytest.raises(RuntimeError, match=r"unknown key/value %d/%d" % (key, v)):
            be.mg_set_option(key, v)
        if before is not None:
            assert _cabi.get_option(key, be) == before, "a refused value was stored"

    try:
        accepts(6, 0); accepts(6, 2); refuses(6, 3)
        accepts(18, 1); accepts(18, 1024); refuses(18, 0); refuses(18, 1025)
        accepts(24, 0); accepts(24, 4096); refuses(24, 48); refuses(24, 4128)
        for key in (1, 2, 3, 4, 5, 7, 19, 22):
            refuses(key, -1); refuses(key, 2)
            accepts(key, 0); accepts(key, 1)
        for key in RETIRED_KEYS + PROBE_KEYS + (11, 16, 20, 25, -1, 1 << 20):
            for v in (0, 1):
                refuses(key, v)
            with pytest.raises(RuntimeError, match="mg_get_option"):
                _cabi.get_option(key, be)
        with pytest.raises(RuntimeError, match="mg_get_option"):
            be.mg_get_option(1, None)
    finally:
        for key, v in OPTION_DEFAULTS.items():
            be.mg_set_option(key, v)


def test_options_scope_restores_what_it_read(lib_path):
    from michigan_amd import _cabi
    be = _cabi.HipBackend(lib_path)
    thin, stripe = _cabi.OPT_CONV_THIN, _cabi.OPT_WGRAD3X3_STRIPE
    be.mg_set_option(thin, 1)                       # not the default: the scope must put back THIS, not a remembered 2
    try:
        with pytest.raises(ZeroDivisionError):
            with _cabi.options({thin: 0, stripe: 128}, be):
                assert (_cabi.get_option(thin, be), _cabi.get_option(stripe, be)) == (0, 128)
                1 / 0
        assert (_cabi.get_option(thin, be), _cabi.get_option(stripe, be)) == (1, 64)
        with _cabi.options({thin: 2}, be):
            assert _cabi.get_option(thin, be) == 2
        assert _cabi.get_option(thin, be) == 1
        with pytest.raises(RuntimeError, match="unknown key/value"):      # a refused value inside the set: what was set before it is undone
            with _cabi.options({stripe: 32, thin: 7}, be):
                pass
        assert (_cabi.get_option(thin, be), _cabi.get_option(stripe, be)) == (1, 64)
    finally:
        be.mg_set_option(thin, OPTION_DEFAULTS[thin])


def test_emulator_options_read_back():
    from michigan_amd import _cabi
    from oracle.cabi_emulator import EmulatorBackend
    em = EmulatorBackend()
    assert em.mg_abi_version() == _cabi.MG_ABI_VERSION
    assert _cabi.get_option(_cabi.OPT_CONV_THIN, em) == 0           # never set: 0, the emulator keeps no list of defaults
    with _cabi.options({_cabi.OPT_CONV_THIN: 1}, em):
        assert _cabi.get_option(_cabi.OPT_CONV_THIN, em) == 1
    assert _cabi.get_option(_cabi.OPT_CONV_THIN, em) == 0
