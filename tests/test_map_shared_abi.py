"""CPU: the switch that lets joint map priors and the map's handle forms run on a handle that exchanges shared objects (include/obvi_map_shared.h) is declared
under the obvi_map_ prefix in a header of its own -- exactly one function, none in the obvi_ba_ namespace the oracle mirrors -- exported by libobvi_ba.so, and
refuses bad arguments without a device.  No older header declares it; the header builds on the resident map's header, as every map header does (it names the
two handle forms in words: tests/test_map_update_abi.py and tests/test_map_extend_abi.py keep every other header from spelling their entries or file names)."""
import ctypes as C
import os
import re
import sys

import helpers
from map_support import header as _header

sys.path.insert(0, helpers.ROOT)
import __graft_entry__ as entry  # noqa: E402

SYMBOLS = ["obvi_map_allow_exchange"]


def test_the_header_declares_the_one_entry_and_the_library_exports_it():
    assert entry.abi_symbols("obvi_map_shared.h", "obvi_map_") == SYMBOLS
    assert entry.abi_symbols("obvi_map_shared.h", "obvi_ba_") == []                 # nothing there for the oracle to mirror
    lib = C.CDLL(helpers.PRODUCT_LIB)
    assert hasattr(lib, SYMBOLS[0])


def test_the_header_builds_on_the_resident_map_and_no_older_header_declares_the_entry():
    assert re.findall(r'#include\s+"([^"]+)"', _header("obvi_map_shared.h")) == ["obvi_map_resident.h"]
    for other in sorted(os.listdir(os.path.join(helpers.ROOT, "include"))):
        if other != "obvi_map_shared.h":
            assert SYMBOLS[0] not in entry.abi_symbols(other, "obvi_map_"), other
            assert "obvi_map_shared.h" not in re.findall(r'#include\s+"([^"]+)"', _header(other)), other   # it includes the older headers, never the reverse


def test_bad_arguments_are_refused_without_a_device():
    lib = C.CDLL(helpers.PRODUCT_LIB)
    lib.obvi_map_allow_exchange.restype = C.c_int
    for on in (0, 1, 2, -1):
        assert lib.obvi_map_allow_exchange(C.c_void_p(), C.c_int32(on)) == -1       # a null handle: OBVI_ERR_INVALID_ARGUMENT
    # (a value other than 0 / 1 beside a live handle: tests/test_gpu_map_shared.py)


def test_build_checks_the_export():
    src = open(os.path.join(helpers.ROOT, "__graft_entry__.py")).read()
    assert 'abi_symbols("obvi_map_shared.h", "obvi_map_")' in src


def test_the_python_binding_has_the_method():
    import obvi_ba
    assert callable(getattr(obvi_ba.BundleAdjuster, "map_allow_exchange", None))
