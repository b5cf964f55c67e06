"""CPU: the selected-inversion covariance entries (include/obvi_cov.h) are part of libobvi_ba.so's ABI, refuse null arguments without a
device, and stay out of obvi_ba.h (whose every name the oracle mirrors)."""
import ctypes as C
import hashlib
import os
import sys

import helpers

sys.path.insert(0, helpers.ROOT)
import __graft_entry__ as entry  # noqa: E402

COV = ["obvi_cov_compute", "obvi_cov_cross_blocks", "obvi_cov_get_stats", "obvi_cov_object_blocks", "obvi_cov_on_pattern", "obvi_cov_point_blocks",
       "obvi_cov_pose_blocks"]


def test_every_function_of_the_covariance_header_is_exported():
    names = entry.abi_symbols("obvi_cov.h", "obvi_cov_")
    assert names == COV
    lib = C.CDLL(helpers.PRODUCT_LIB)
    assert [n for n in names if not hasattr(lib, n)] == []


def test_the_covariance_entries_are_not_part_of_the_mirrored_header():
    """tests/test_abi.py::test_oracle_mirrors_the_abi asks the oracle for a twin of every obvi_ba_* name in obvi_ba.h: the new entries have
    their own header and prefix, and obvi_ba.h declares exactly the 43 names it declared before them plus obvi_ba_debug_reduced_solve, which the oracle does mirror (digest of the sorted list)."""
    names = entry.abi_symbols()
    assert len(names) == 44 and hashlib.sha256(" ".join(names).encode()).hexdigest()[:16] == "2837b0377bdf0305"
    assert "obvi_cov_" not in open(os.path.join(helpers.ROOT, "include", "obvi_ba.h")).read()


def test_null_arguments_are_refused_without_a_device():
    lib = C.CDLL(helpers.PRODUCT_LIB)
    for n in COV:
        getattr(lib, n).restype = C.c_int
    null = C.c_void_p()
    n1 = C.c_int64(1)
    assert lib.obvi_cov_compute(null) == -1
    for name in ("obvi_cov_pose_blocks", "obvi_cov_object_blocks", "obvi_cov_point_blocks"):
        assert getattr(lib, name)(null, n1, null, null) == -1
    assert lib.obvi_cov_cross_blocks(null, n1, null, null, null, null, null, null) == -1
    assert lib.obvi_cov_on_pattern(null, n1, null, null, null, null, null) == -1
    assert lib.obvi_cov_get_stats(null, null, null, null) == -1
