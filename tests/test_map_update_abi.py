"""CPU: the way back into a device-resident map (include/obvi_map_update.h) is declared under the obvi_map_ prefix in a header of its own -- exactly three
functions, none of them in the obvi_ba_ namespace the oracle mirrors -- exported by libobvi_ba.so, and refuses null arguments without a device.  The new header
includes obvi_map_resident.h, never the reverse.  And the yardstick of tests/test_gpu_map_update.py is itself held: the update formula against the information
form, both in long double, on the inputs the GPU tests use (this one test passes without the feature: it tests the reference, not the product)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import helpers
import map_update_cases as cases
from map_support import header as _header

sys.path.insert(0, helpers.ROOT)
import __graft_entry__ as entry  # noqa: E402

SYMBOLS = ["obvi_map_condition", "obvi_map_condition_on_handle", "obvi_map_get"]


def test_the_header_declares_the_three_entries_and_the_library_exports_them():
    assert entry.abi_symbols("obvi_map_update.h", "obvi_map_") == SYMBOLS
    assert entry.abi_symbols("obvi_map_update.h", "obvi_ba_") == []                 # nothing there for the oracle to mirror
    lib = C.CDLL(helpers.PRODUCT_LIB)
    for s in SYMBOLS:
        assert hasattr(lib, s), s


def test_the_header_includes_the_resident_map_and_no_older_header_mentions_it():
    assert re.search(r'#include\s+"obvi_map_resident\.h"', _header("obvi_map_update.h"))
    for other in sorted(os.listdir(os.path.join(helpers.ROOT, "include"))):
        if other != "obvi_map_update.h":
            txt = _header(other)
            assert "map_update" not in txt and "obvi_map_condition" not in txt and "obvi_map_get" not in txt, other


def test_null_arguments_and_an_empty_window_are_refused_without_a_device():
    lib = C.CDLL(helpers.PRODUCT_LIB)
    for name in SYMBOLS:
        getattr(lib, name).restype = C.c_int
    null, fake = C.c_void_p(), C.c_void_p(8)                                        # fake: never dereferenced, another argument is refused first
    idx = np.zeros(1, np.uint32).ctypes.data_as(C.c_void_p)
    mu, cv = np.zeros(7).ctypes.data_as(C.c_void_p), np.eye(7).ctypes.data_as(C.c_void_p)
    out = C.c_void_p(1)
    assert lib.obvi_map_get(null, mu, cv) == -1
    # (a null map or out beside a live handle: test_gpu_map_update.py -- the refusal is written into the handle's last error)
    for h, m, o, k in ((null, fake, C.byref(out), 1), (null, null, C.byref(out), 1), (null, fake, None, 1), (null, fake, C.byref(out), 0), (null, fake, C.byref(out), -2)):
        out.value = 1
        assert lib.obvi_map_condition(h, m, C.c_int64(k), idx, mu, cv, o) == -1
        assert o is None or not out.value                                           # *out is NULL on every failure
        out.value = 1
        assert lib.obvi_map_condition_on_handle(h, m, C.c_int64(k), idx, idx, o) == -1
        assert o is None or not out.value


def test_the_python_binding_has_the_three_methods():
    import obvi_ba
    for name in ("get", "condition", "condition_on"):
        assert callable(getattr(obvi_ba.Map, name, None)), name


@pytest.mark.parametrize("which,od,k", cases.EDGE_CASES)
def test_the_yardstick_is_held_by_the_update_formula_in_long_double(which, od, k):
    mean, cov = cases.map_of(which, od)
    sel, m, P = cases.edge_case(which, od, k)
    mu_ref, C_ref = cases.edge_reference(which, od, k)
    mu, Cn = cases.update_formula(mean, cov, sel, m, P, od, dtype=np.longdouble)
    eC = float(np.abs(Cn - C_ref).max() / np.abs(C_ref).max())
    em = float(np.abs(mu - mu_ref).max() / np.abs(mu_ref).max())
    print("%s map, od %d, k %d: covariance %.2e  means %.2e" % (which, od, k, eC, em))
    assert eC <= 1e-14 and em <= 1e-14
