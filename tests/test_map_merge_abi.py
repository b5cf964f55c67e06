"""CPU: the merge of duplicate objects of a device-resident map (include/obvi_map_merge.h) is declared under the obvi_map_ prefix in a header of its own --
exactly one function, nothing in the obvi_ba_ namespace the oracle mirrors -- exported by libobvi_ba.so, and refuses bad arguments without a device.  The header
includes obvi_map_resident.h alone, no other header names it, and it names none of the neighbouring entries the other headers' tests reserve for their owners.
And the yardstick of tests/test_gpu_map_merge.py is itself held: the merge formula against the null-space / information form, both in long double, on the inputs
the GPU tests use, at the bar tests/test_map_update_abi.py sets for the same check (1e-14); numpy's fp64 evaluation of the formula within 1e-12 -- a condition on
the inputs: a case that breaks it is replaced, the GPU bar (1e-11) is not moved.

Measured: the long-double formula within 2.5e-16 (covariance) and 3.7e-16 (means) of the yardstick on every case; numpy's fp64 evaluation within 2.5e-13, the
worst case small, od 9, groups 4 4 4 3 3 3 3."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import helpers
import map_merge_cases as cases
from map_support import header as _header

sys.path.insert(0, helpers.ROOT)
import __graft_entry__ as entry  # noqa: E402

SYMBOLS = ["obvi_map_merge"]
RESERVED = ["map_update", "obvi_map_condition", "obvi_map_get", "map_extend", "obvi_map_extend", "obvi_map_select"]


def test_the_header_declares_the_one_entry_and_the_library_exports_it():
    assert entry.abi_symbols("obvi_map_merge.h", "obvi_map_") == SYMBOLS
    assert entry.abi_symbols("obvi_map_merge.h", "obvi_ba_") == []                  # nothing there for the oracle to mirror
    lib = C.CDLL(helpers.PRODUCT_LIB)
    for s in SYMBOLS:
        assert hasattr(lib, s), s


def test_the_header_includes_the_resident_map_alone_and_no_other_header_mentions_it():
    txt = _header("obvi_map_merge.h")
    assert re.findall(r'#include\s+"([^"]+)"', txt) == ["obvi_map_resident.h"]
    for word in RESERVED:
        assert word not in txt, word
    for other in sorted(os.listdir(os.path.join(helpers.ROOT, "include"))):
        if other != "obvi_map_merge.h":
            assert "map_merge" not in _header(other), other


def test_bad_arguments_are_refused_without_a_device():
    lib = C.CDLL(helpers.PRODUCT_LIB)
    lib.obvi_map_merge.restype = C.c_int
    null, fake = C.c_void_p(), C.c_void_p(8)                                        # fake: never dereferenced, another argument is refused first
    idx = np.zeros(1, np.uint32).ctypes.data_as(C.c_void_p)
    where = np.full(4, 77, np.uint32)
    out = C.c_void_p(1)
    # (the same beside a live handle: test_gpu_map_merge.py -- the refusal is written into the handle's last error)
    for m, o, q, drop, keep in ((fake, C.byref(out), 1, idx, idx), (null, C.byref(out), 1, idx, idx), (fake, None, 1, idx, idx), (fake, C.byref(out), 0, idx, idx),
                                (fake, C.byref(out), -2, idx, idx), (fake, C.byref(out), 1, None, idx), (fake, C.byref(out), 1, idx, None)):
        out.value = 1
        assert lib.obvi_map_merge(null, m, C.c_int64(q), drop, keep, None, None, where.ctypes.data_as(C.c_void_p), o) == -1
        assert o is None or not out.value                                           # *out is NULL on every failure
    assert (where == 77).all()


def test_the_python_binding_has_the_method():
    import obvi_ba
    assert callable(getattr(obvi_ba.Map, "merge", None))


@pytest.mark.parametrize("which,od,key,noisy", cases.CASES)
def test_the_yardstick_is_held_by_the_merge_formula_in_long_double(which, od, key, noisy):
    mean, cov = cases.map_of(which, od)
    drop, keep, offset, noise = cases.merge_case(which, od, key, noisy)
    mu_ref, C_ref = cases.merge_reference(which, od, key, noisy)
    assert mu_ref.shape == (len(mean) - len(drop), od) and C_ref.shape == (mu_ref.size, mu_ref.size)
    mu, Cn = cases.merge_formula(mean, cov, drop, keep, offset, noise, od, dtype=np.longdouble)
    eC = float(np.abs(Cn - C_ref).max() / np.abs(C_ref).max())
    em = float(np.abs(mu - mu_ref).max() / np.abs(mu_ref).max())
    mu64, C64 = cases.merge_formula(mean, cov, drop, keep, offset, noise, od)
    e64 = max(float(np.abs(C64 - C_ref).max() / np.abs(C_ref).max()), float(np.abs(mu64 - mu_ref).max() / np.abs(mu_ref).max()))
    print("%s map, od %d, groups %s%s (%d pair rows, %d rows left): covariance %.2e  means %.2e;  numpy's fp64 evaluation %.2e"
          % (which, od, key, ", noise" if noisy else "", len(drop) * od, mu_ref.size, eC, em, e64))
    assert eC <= 1e-14 and em <= 1e-14
    assert e64 <= 1e-12                                                             # the inputs are ones fp64 can be held to 1e-11 on
    assert np.linalg.eigvalsh(np.asarray(C_ref, dtype=np.float64)).min() > 0


def test_two_independent_estimates_fuse_by_their_informations():
    """A closed form: on a block-diagonal two-object map an exact merge with d = 0 is the product of two Gaussians, (S1^-1 + S2^-1)^-1 and the
    information-weighted mean -- whichever of the two survives."""
    od = 7
    rng = np.random.default_rng(12)
    A, B = rng.normal(size=(2, od, od))
    S1, S2 = A @ A.T + od * np.eye(od), B @ B.T + od * np.eye(od)
    cov = np.zeros((2 * od, 2 * od))
    cov[:od, :od], cov[od:, od:] = S1, S2
    mean = rng.normal(size=(2, od))
    L1, L2 = cases.inv_ld(S1), cases.inv_ld(S2)
    C_want = cases.inv_ld(L1 + L2)
    m_want = C_want @ (L1 @ mean[0] + L2 @ mean[1])
    for drop, keep in ((0, 1), (1, 0)):
        d, k = np.array([drop], np.uint32), np.array([keep], np.uint32)
        for got in (cases.merge_formula(mean, cov, d, k, None, None, od, dtype=np.longdouble),
                    cases.yardstick(mean, cov, cases.inv_ld(cov), d, k, np.zeros((1, od)), None, od)):
            assert got[0].shape == (1, od) and got[1].shape == (od, od)
            assert np.abs(got[1] - C_want).max() <= 1e-14 * np.abs(C_want).max()
            assert np.abs(got[0].ravel() - m_want).max() <= 1e-14 * np.abs(m_want).max()
    assert list(cases.new_index(2, np.array([0]), np.array([1]))[0]) == [0, 0]
