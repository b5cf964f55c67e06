"""CPU: a device-resident map that grows (include/obvi_map_extend.h) is declared under the obvi_map_ prefix in a header of its own -- exactly three functions,
none of them in the obvi_ba_ namespace the oracle mirrors -- exported by libobvi_ba.so, and refuses bad arguments without a device.  The header includes
obvi_map_resident.h and no other header names it.  And the yardstick of tests/test_gpu_map_extend.py is itself held: the extension formula against the
information form, both in long double, on the inputs the GPU tests use, at the bar tests/test_map_update_abi.py sets for the same check (1e-14)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import helpers
import map_extend_cases as cases
from map_support import header as _header

sys.path.insert(0, helpers.ROOT)
import __graft_entry__ as entry  # noqa: E402

SYMBOLS = ["obvi_map_extend", "obvi_map_extend_on_handle", "obvi_map_select"]


def test_the_header_declares_the_three_entries_and_the_library_exports_them():
    assert entry.abi_symbols("obvi_map_extend.h", "obvi_map_") == SYMBOLS
    assert entry.abi_symbols("obvi_map_extend.h", "obvi_ba_") == []                 # nothing there for the oracle to mirror
    lib = C.CDLL(helpers.PRODUCT_LIB)
    for s in SYMBOLS:
        assert hasattr(lib, s), s


def test_the_header_includes_the_resident_map_alone_and_no_other_header_mentions_it():
    txt = _header("obvi_map_extend.h")
    assert re.findall(r'#include\s+"([^"]+)"', txt) == ["obvi_map_resident.h"]
    for other in sorted(os.listdir(os.path.join(helpers.ROOT, "include"))):
        if other != "obvi_map_extend.h":
            txt = _header(other)
            assert "map_extend" not in txt and "obvi_map_extend" not in txt and "obvi_map_select" not in txt, other


def test_bad_arguments_are_refused_without_a_device():
    lib = C.CDLL(helpers.PRODUCT_LIB)
    for name in SYMBOLS:
        getattr(lib, name).restype = C.c_int
    null, fake = C.c_void_p(), C.c_void_p(8)                                        # fake: never dereferenced, another argument is refused first
    idx = np.zeros(1, np.uint32).ctypes.data_as(C.c_void_p)
    mu, cv = np.zeros(14).ctypes.data_as(C.c_void_p), np.eye(14).ctypes.data_as(C.c_void_p)
    out = C.c_void_p(1)
    # (the same beside a live handle: test_gpu_map_extend.py -- the refusal is written into the handle's last error)
    for m, o, k_old, k_new in ((fake, C.byref(out), 1, 1), (null, C.byref(out), 0, 1), (fake, None, 1, 1), (fake, C.byref(out), 1, 0), (fake, C.byref(out), 1, -3),
                               (fake, C.byref(out), -1, 1), (null, C.byref(out), 1, 1)):
        out.value = 1
        assert lib.obvi_map_extend(null, m, C.c_int64(k_old), idx, C.c_int64(k_new), mu, cv, o) == -1
        assert o is None or not out.value                                           # *out is NULL on every failure
        out.value = 1
        assert lib.obvi_map_extend_on_handle(null, m, C.c_int64(k_old), idx, idx, C.c_int64(k_new), idx, o) == -1
        assert o is None or not out.value
    for m, o, k in ((fake, C.byref(out), 1), (null, C.byref(out), 1), (fake, None, 1), (fake, C.byref(out), 0)):
        out.value = 1
        assert lib.obvi_map_select(null, m, C.c_int64(k), idx, o) == -1
        assert o is None or not out.value


def test_the_python_binding_has_the_five_methods():
    import obvi_ba
    for name in ("extend", "extend_on", "select", "from_posterior", "from_handle"):
        assert callable(getattr(obvi_ba.Map, name, None)), name


@pytest.mark.parametrize("which,od,k_old,k_new", cases.EXTEND_CASES)
def test_the_yardstick_is_held_by_the_extension_formula_in_long_double(which, od, k_old, k_new):
    mean, cov = cases.map_of(which, od)
    sel, m, P = cases.extend_case(which, od, k_old, k_new)
    mu_ref, C_ref = cases.extend_reference(which, od, k_old, k_new)
    mu, Cn = cases.extension_formula(mean, cov, sel, k_new, m, P, od, dtype=np.longdouble)
    eC = float(np.abs(Cn - C_ref).max() / np.abs(C_ref).max())
    em = float(np.abs(mu - mu_ref).max() / np.abs(mu_ref).max())
    mu64, C64 = cases.extension_formula(mean, cov, sel, k_new, m, P, od)
    e64 = max(float(np.abs(C64 - C_ref).max() / np.abs(C_ref).max()), float(np.abs(mu64 - mu_ref).max() / np.abs(mu_ref).max()))
    print("%s map, od %d, %d old + %d new: covariance %.2e  means %.2e;  numpy's fp64 evaluation %.2e" % (which, od, k_old, k_new, eC, em, e64))
    assert eC <= 1e-14 and em <= 1e-14
    assert np.linalg.eigvalsh(np.asarray(C_ref, dtype=np.float64)).min() > 0
