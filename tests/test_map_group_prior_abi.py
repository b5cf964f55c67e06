"""CPU: obvi_map_set_group_priors (include/obvi_map_group_prior.h) is declared under the obvi_map_ prefix in a header of its own, exported by
libobvi_ba.so, and refuses a null handle without a device.  The new header includes obvi_map_prior.h, never the reverse, and stays out of
include/obvi_ba.h: the oracle mirrors that header and does not know the factor."""
import ctypes as C
import os
import re
import sys

import helpers
from map_support import header as _header

sys.path.insert(0, helpers.ROOT)
import __graft_entry__ as entry  # noqa: E402


def test_the_group_prior_entry_is_declared_and_exported():
    assert entry.abi_symbols("obvi_map_group_prior.h", "obvi_map_") == ["obvi_map_set_group_priors"]
    assert entry.abi_symbols("obvi_map_group_prior.h", "obvi_ba_") == []            # nothing there for the oracle to mirror
    txt = _header("obvi_map_group_prior.h")
    assert re.search(r"OBVI_FACTOR_MAP_GROUP_PRIOR\s*=\s*10\b", txt)
    assert re.search(r'#include\s+"obvi_map_prior\.h"', txt)
    for other in ("obvi_map_prior.h", "obvi_ba.h"):
        assert "group_prior" not in _header(other) and "GROUP_PRIOR" not in _header(other), other
    assert hasattr(C.CDLL(helpers.PRODUCT_LIB), "obvi_map_set_group_priors")


def test_a_null_handle_is_refused_without_a_device():
    lib = C.CDLL(helpers.PRODUCT_LIB)
    lib.obvi_map_set_group_priors.restype = C.c_int
    null = C.c_void_p()
    for n in (0, 1):
        assert lib.obvi_map_set_group_priors(null, C.c_int64(n), null, null, null, null, C.c_double(1.0)) == -1


def test_the_python_constants_follow_the_header():
    import obvi_ba
    txt = _header("obvi_map_group_prior.h")
    assert obvi_ba.FACTOR_MAP_GROUP_PRIOR == 10
    assert int(re.search(r"OBVI_MAP_GROUP_MAX_ROWS\s*=\s*(\d+)", txt).group(1)) == obvi_ba.MAP_GROUP_MAX_ROWS == 2048
