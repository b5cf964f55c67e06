"""CPU: the device-resident map (include/obvi_map_resident.h) is declared under the obvi_map_ prefix in a header of its own -- exactly four functions, none of
them in the obvi_ba_ namespace the oracle mirrors -- exported by libobvi_ba.so, and refuses null arguments and malformed maps without a device.  The new header
includes obvi_map_group_prior.h, never the reverse, and what obvi_map_group_prior.h, obvi_map_prior.h and obvi_ba.h declare is what they declared before."""
import ctypes as C
import os
import re
import sys

import numpy as np

import helpers
from map_support import header as _header

sys.path.insert(0, helpers.ROOT)
import __graft_entry__ as entry  # noqa: E402

SYMBOLS = ["obvi_map_create", "obvi_map_destroy", "obvi_map_num_objects", "obvi_map_set_group_priors_from_map"]


def _lib():
    lib = C.CDLL(helpers.PRODUCT_LIB)
    lib.obvi_map_create.restype = C.c_int
    lib.obvi_map_destroy.restype = None
    lib.obvi_map_num_objects.restype = C.c_int64
    lib.obvi_map_set_group_priors_from_map.restype = C.c_int
    return lib


def test_the_header_declares_the_four_entries_and_the_library_exports_them():
    assert entry.abi_symbols("obvi_map_resident.h", "obvi_map_") == SYMBOLS
    assert entry.abi_symbols("obvi_map_resident.h", "obvi_ba_") == []               # nothing there for the oracle to mirror
    txt = _header("obvi_map_resident.h")
    assert re.search(r'#include\s+"obvi_map_group_prior\.h"', txt)
    assert re.search(r"typedef\s+struct\s+obvi_map\s+obvi_map\s*;", txt)
    lib = C.CDLL(helpers.PRODUCT_LIB)
    for s in SYMBOLS:
        assert hasattr(lib, s), s


def test_the_older_headers_declare_what_they_declared():
    assert entry.abi_symbols("obvi_map_group_prior.h", "obvi_map_") == ["obvi_map_set_group_priors"]
    for other in ("obvi_map_group_prior.h", "obvi_map_prior.h", "obvi_ba.h"):
        txt = _header(other)
        assert "map_resident" not in txt and "from_map" not in txt and "obvi_map_create" not in txt, other


def test_null_handle_and_null_map_are_refused_without_a_device():
    lib = _lib()
    null = C.c_void_p()
    fake = C.c_void_p(8)                                                            # never dereferenced: the other argument is null
    for n in (0, 1):
        assert lib.obvi_map_set_group_priors_from_map(null, null, C.c_int64(n), null, null, null, C.c_double(1.0)) == -1
        assert lib.obvi_map_set_group_priors_from_map(null, fake, C.c_int64(n), null, null, null, C.c_double(1.0)) == -1


def test_create_refuses_malformed_maps_before_any_device_work():
    lib = _lib()
    mean, cov = np.zeros((2, 7)), np.eye(14)
    pm, pc = mean.ctypes.data_as(C.c_void_p), cov.ctypes.data_as(C.c_void_p)
    out = C.c_void_p(1)
    assert lib.obvi_map_create(C.c_int32(0), C.c_int32(7), C.c_int64(2), pm, pc, None) == -1            # null out
    for args in ((7, 0, pm, pc), (7, -3, pm, pc), (8, 2, pm, pc), (7, 2, None, pc), (7, 2, pm, None)):
        out.value = 1
        assert lib.obvi_map_create(C.c_int32(0), C.c_int32(args[0]), C.c_int64(args[1]), args[2], args[3], C.byref(out)) == -1, args[:2]
        assert not out.value                                                                               # *out is NULL on every failure
    # above 1 GiB of covariance: refused on the count alone (11 586 rows and more; the pointers are never read that far)
    out.value = 1
    assert lib.obvi_map_create(C.c_int32(0), C.c_int32(7), C.c_int64(1656), pm, pc, C.byref(out)) == -1 and not out.value
    # not finite: OBVI_ERR_NUMERICAL, still before the device is asked for
    for bad_mean in (True, False):
        m2, c2 = mean.copy(), cov.copy()
        if bad_mean:
            m2[1, 3] = np.inf
        else:
            c2[5, 9] = np.nan
        out.value = 1
        assert lib.obvi_map_create(C.c_int32(0), C.c_int32(7), C.c_int64(2), m2.ctypes.data_as(C.c_void_p), c2.ctypes.data_as(C.c_void_p), C.byref(out)) == -6 and not out.value
    lib.obvi_map_destroy(None)                                                                             # a no-op
    assert lib.obvi_map_num_objects(None) == -1


def test_the_python_binding_has_the_map():
    import obvi_ba
    assert hasattr(obvi_ba, "Map") and hasattr(obvi_ba.BundleAdjuster, "set_map_group_priors_from_map")
    for name in ("create", "close", "n_objects", "__enter__", "__exit__"):
        assert hasattr(obvi_ba.Map, name), name
