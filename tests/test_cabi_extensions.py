"""CPU: the extension groups of the C ABI (include/michigan_hip/*.h) held to the obligations of the core table
(tests/test_cabi_host.py, tests/test_guard_alloc.py): every declared mg_*( is mirrored in michigan_amd/_cabi.py, exported by the
library, and -- where it writes device memory -- has a guarded case in tests/test_gpu_style_guard_bands.py.  The core table itself
stays what those two tests pin: folding the two tables into one is a later change that moves MG_ABI_VERSION and those tests."""
import ctypes
import glob
import os
import re

import test_gpu_style_guard_bands as SGB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_DEVICE_WRITE = {"mg_ext_version", "mg_feat_moment_workspace"}


def _declared(pattern):
    names = set()
    for path in glob.glob(os.path.join(ROOT, "include", pattern)):
        with open(path) as fh:
            text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
        names |= set(re.findall(r"\b(mg_[a-z0-9_]+)\s*\(", text))
    return names


def test_extension_mirror_matches_the_extension_headers():
    from michigan_amd import _cabi, build
    ext = _declared(os.path.join("michigan_hip", "*.h"))
    assert ext and set(_cabi.EXTENSION_SYMBOLS) == ext == set(_cabi._EXT_PROTOS)
    assert len(_cabi.EXTENSION_SYMBOLS) == len(set(_cabi.EXTENSION_SYMBOLS))
    lib = ctypes.CDLL(build.build(verbose=False))
    for fn in _cabi.EXTENSION_SYMBOLS:
        assert hasattr(lib, fn), "%s is declared but not exported" % fn
    be = _cabi.HipBackend(build.build(verbose=False))
    assert be.mg_ext_version() == _cabi.MG_EXT_FEATURE_LOSSES
    with open(os.path.join(ROOT, "include", "michigan_hip", "feature_losses.h")) as fh:
        assert re.search(r"#define\s+MG_EXT_FEATURE_LOSSES\s+%d\b" % _cabi.MG_EXT_FEATURE_LOSSES, fh.read())
    # the descriptor: 6 pointers, 4 int64, 4 int32, 3 pointers, no padding
    assert ctypes.sizeof(_cabi.FeatMomentDesc) == 6 * 8 + 4 * 8 + 4 * 4 + 3 * 8


def test_the_core_table_is_untouched():
    from michigan_amd import _cabi
    core = _declared("*.h")
    assert set(_cabi.EXPORTED_SYMBOLS) == core and _cabi.MG_ABI_VERSION == 9
    assert not set(_cabi.EXTENSION_SYMBOLS) & core and not set(_cabi._EXT_PROTOS) & set(_cabi._PROTOS)


def test_every_device_writing_extension_symbol_has_a_guarded_case():
    from michigan_amd import _cabi
    ext = set(_cabi.EXTENSION_SYMBOLS)
    assert NO_DEVICE_WRITE <= ext
    covered = {ep for c in SGB.CASES for ep in c.covers}
    assert covered <= ext and not covered & NO_DEVICE_WRITE
    missing = sorted(ext - NO_DEVICE_WRITE - covered)
    assert not missing, "extension entry points without a guarded case in tests/test_gpu_style_guard_bands.py: %s" % missing
    assert len({c.id for c in SGB.CASES}) == len(SGB.CASES)
