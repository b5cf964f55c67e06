"""CPU: obvi_map_set_pair_priors (include/obvi_map_prior.h) is declared under its own prefix, exported by libobvi_ba.so, and refuses a null handle
without a device.  The header stays out of include/obvi_ba.h: the oracle mirrors that header and does not know the factor."""
import ctypes as C
import os
import re
import sys

import helpers

sys.path.insert(0, helpers.ROOT)
import __graft_entry__ as entry  # noqa: E402


def test_the_pair_prior_entry_is_declared_and_exported():
    assert entry.abi_symbols("obvi_map_prior.h", "obvi_map_") == ["obvi_map_set_pair_priors"]
    assert entry.abi_symbols("obvi_map_prior.h", "obvi_ba_") == []                  # nothing there for the oracle to mirror
    txt = open(os.path.join(helpers.ROOT, "include", "obvi_map_prior.h")).read()
    assert re.search(r"OBVI_FACTOR_MAP_PAIR_PRIOR\s*=\s*9\b", txt) and re.search(r"OBVI_MAP_PAIR_JOINT\s*=\s*0\b", txt) and re.search(r"OBVI_MAP_PAIR_CONDITIONAL\s*=\s*1\b", txt)
    assert "obvi_map_" not in open(os.path.join(helpers.ROOT, "include", "obvi_ba.h")).read()
    assert hasattr(C.CDLL(helpers.PRODUCT_LIB), "obvi_map_set_pair_priors")


def test_a_null_handle_is_refused_without_a_device():
    lib = C.CDLL(helpers.PRODUCT_LIB)
    lib.obvi_map_set_pair_priors.restype = C.c_int
    null = C.c_void_p()
    for n in (0, 1):
        assert lib.obvi_map_set_pair_priors(null, C.c_int64(n), null, null, null, null, null, null, C.c_double(1.0)) == -1
