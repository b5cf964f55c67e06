"""CPU: obvi_cov_compute_pairs and its debug form obvi_cov_debug_compute_pairs (include/obvi_cov_pairs.h, which include/obvi_cov.h includes) is declared to callers of the covariance header, exported by
libobvi_ba.so, and refuses null arguments without a device."""
import ctypes as C
import os
import re
import sys

import helpers

sys.path.insert(0, helpers.ROOT)
import __graft_entry__ as entry  # noqa: E402


def test_the_declared_pairs_entry_is_declared_and_exported():
    assert entry.abi_symbols("obvi_cov_pairs.h", "obvi_cov_") == ["obvi_cov_compute_pairs", "obvi_cov_debug_compute_pairs"]
    cov = open(os.path.join(helpers.ROOT, "include", "obvi_cov.h")).read()
    assert re.search(r'^#include "obvi_cov_pairs.h"', cov, flags=re.M)          # whoever includes the covariance header sees the declaration
    assert hasattr(C.CDLL(helpers.PRODUCT_LIB), "obvi_cov_compute_pairs") and hasattr(C.CDLL(helpers.PRODUCT_LIB), "obvi_cov_debug_compute_pairs")


def test_null_arguments_are_refused_without_a_device():
    lib = C.CDLL(helpers.PRODUCT_LIB)
    lib.obvi_cov_compute_pairs.restype = C.c_int
    null = C.c_void_p()
    assert lib.obvi_cov_compute_pairs(null, C.c_int64(0), null, null, null, null) == -1
    assert lib.obvi_cov_compute_pairs(null, C.c_int64(1), null, null, null, null) == -1
    # the debug form: no handle, no buffer for the system, pairs announced without their arrays
    lib.obvi_cov_debug_compute_pairs.restype = C.c_int
    buf = (C.c_double * 4)()
    assert lib.obvi_cov_debug_compute_pairs(null, C.c_int64(0), null, null, null, null, null, buf, null, C.c_int32(2), null) == -1
    assert lib.obvi_cov_debug_compute_pairs(null, C.c_int64(0), null, null, null, null, null, null, null, C.c_int32(0), null) == -1
    assert lib.obvi_cov_debug_compute_pairs(null, C.c_int64(1), null, null, null, null, null, buf, null, C.c_int32(2), null) == -1
