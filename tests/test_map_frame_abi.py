"""CPU: the move of a device-resident map into another frame and the join of two maps (include/obvi_map_frame.h) are declared under the obvi_map_ prefix in
a header of their own -- exactly two functions, nothing in the obvi_ba_ namespace the oracle mirrors -- exported by libobvi_ba.so, and refuse null arguments
without a device (the refusals that need a handle to read a block size from are in tests/test_gpu_map_frame.py).  The header includes obvi_map_resident.h alone,
no other header names it, and it names none of the neighbouring entries the other headers' tests reserve for their owners.
And the reference of tests/test_gpu_map_frame.py is itself held: the closed-form Jacobians of tests/map_frame_cases.py against central differences of g in long
double (h = 1e-5, one Richardson step: truncation and round-off both under 1e-13, so 1e-9 only catches wrong formulas); the formula in long double against the
information-form yardstick (1e-14, the bar of tests/test_map_merge_abi.py for the same kind of check); numpy's fp64 evaluation of the formula within 1e-14 of
the yardstick -- a condition on the inputs: a case that breaks it is replaced, the GPU bar (1e-12) is not moved.  The chain's claims -- exactly the planted
pairs, B's own objects closer to their true places after the merge than after the move alone -- are held on the long-double chain before any device runs it.

Measured (largest difference over the largest entry of the yardstick): see DESIGN.md 4c.8."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import helpers
import map_frame_cases as cases
from map_support import header as _header

sys.path.insert(0, helpers.ROOT)
import __graft_entry__ as entry  # noqa: E402

LD = np.longdouble
SYMBOLS = ["obvi_map_join", "obvi_map_transform"]
RESERVED = ["map_merge", "map_match", "map_update", "map_extend", "obvi_map_condition", "obvi_map_get", "obvi_map_extend", "obvi_map_select"]


def test_the_header_declares_the_two_entries_and_the_library_exports_them():
    assert entry.abi_symbols("obvi_map_frame.h", "obvi_map_") == SYMBOLS
    assert entry.abi_symbols("obvi_map_frame.h", "obvi_ba_") == []                  # nothing there for the oracle to mirror
    lib = C.CDLL(helpers.PRODUCT_LIB)
    for s in SYMBOLS:
        assert hasattr(lib, s), s


def test_the_header_includes_the_resident_map_alone_and_no_other_header_mentions_it():
    txt = _header("obvi_map_frame.h")
    assert re.findall(r'#include\s+"([^"]+)"', txt) == ["obvi_map_resident.h"]
    for word in RESERVED:
        assert word not in txt, word
    for other in sorted(os.listdir(os.path.join(helpers.ROOT, "include"))):
        if other != "obvi_map_frame.h":
            assert "map_frame" not in _header(other), other


def test_null_arguments_are_refused_without_a_device():
    lib = C.CDLL(helpers.PRODUCT_LIB)
    lib.obvi_map_transform.restype = C.c_int
    lib.obvi_map_join.restype = C.c_int
    null, fake = C.c_void_p(), C.c_void_p(8)                                        # fake: never dereferenced, the null handle is refused first
    t = np.zeros(6).ctypes.data_as(C.c_void_p)
    out = C.c_void_p(1)
    for m, tr, o in ((fake, t, C.byref(out)), (null, t, C.byref(out)), (fake, None, C.byref(out)), (fake, t, None)):
        out.value = 1
        assert lib.obvi_map_transform(null, m, tr, None, o) == -1
        assert o is None or not out.value                                           # *out is NULL on every failure
    for a, b, o in ((fake, fake, C.byref(out)), (null, fake, C.byref(out)), (fake, null, C.byref(out)), (fake, fake, None)):
        out.value = 1
        assert lib.obvi_map_join(null, a, b, o) == -1
        assert o is None or not out.value


def test_the_python_binding_has_both_methods():
    import obvi_ba
    assert callable(getattr(obvi_ba.Map, "transform", None)) and callable(getattr(obvi_ba.Map, "join", None))


# ---- the reference of the GPU tests is itself held --------------------------------------------------------------------------------------------------------
def central(f, x, h=LD(1e-5)):
    """d f / d x [len(f)][len(x)] by central differences with one Richardson step, long double."""
    x = np.asarray(x, dtype=LD)
    cols = []
    for i in range(len(x)):
        e = np.zeros(len(x), dtype=LD)
        e[i] = h
        d1, d2 = (f(x + e) - f(x - e)) / (2 * h), (f(x + 2 * e) - f(x - 2 * e)) / (4 * h)
        cols.append((4 * d1 - d2) / 3)
    return np.array(cols, dtype=LD).T


@pytest.mark.parametrize("od,tname", [(od, t) for od in (7, 9) for t in cases.TRANSFORMS[od]])
def test_the_closed_form_jacobians_are_the_derivatives_of_g(od, tname):
    mean, _ = cases.case_map("small", od)
    T = np.asarray(cases.transform_of(tname, od), dtype=LD)
    K = od - 3
    J, Ji, G = cases.jacobians(T, mean, od)
    worst = 0.0
    for o in range(len(mean)):
        x = np.asarray(mean[o], dtype=LD)
        Jn = central(lambda v: cases.g(T, v, od), x)
        Gn = central(lambda v: cases.g(v, x, od), T)
        Jo = np.eye(od, dtype=LD)
        Jo[:K, :K] = J[o]
        Go = np.zeros((od, cases.DT[od]), dtype=LD)
        Go[:K] = G[o]
        scale = max(1.0, float(np.abs(Go).max()))
        worst = max(worst, float(np.abs(Jn - Jo).max()), float(np.abs(Gn - Go).max()) / scale, float(np.abs(J[o] @ Ji[o] - np.eye(K)).max()))
    print("od %d, %s: J_o, G_o against central differences, J_o J_o^-1 against I: %.2e" % (od, tname, worst))
    assert worst <= 1e-9


@pytest.mark.parametrize("which,od,tname,with_sigma", cases.CASES)
def test_the_yardstick_is_held_by_the_formula_in_long_double_and_numpy_stays_within_the_condition(which, od, tname, with_sigma):
    mean, cov, T, Sigma = cases.case_inputs(which, od, tname, with_sigma)
    mu_ref, C_ref = cases.reference(which, od, tname, with_sigma)
    mu, Cn = cases.formula(mean, cov, T, Sigma, od, dtype=LD)
    eC, em = cases.errors(mu, Cn, mu_ref, C_ref)
    mu64, C64 = cases.formula(mean, cov, T, Sigma, od)
    e64 = max(cases.errors(mu64, C64, mu_ref, C_ref))
    print("%s map, od %d, %s%s (%d rows): the long-double formula within %.2e of the yardstick; numpy's fp64 evaluation within %.2e"
          % (which, od, tname, ", Sigma" if with_sigma else "", len(C_ref), eC, e64))
    assert eC <= 1e-14 and em == 0.0                                                # the means are g itself
    assert e64 <= 1e-14                                                             # the inputs are ones fp64 can be held to 1e-12 on
    assert np.linalg.eigvalsh(np.asarray(C_ref, dtype=np.float64)).min() > 0


def test_the_sub_maps_reference_is_a_slice_of_the_large_maps():
    od, n = 7, 12
    mean, cov, T, Sigma = cases.case_inputs("large", od, "generic", True)
    mu, Cn = cases.formula(*cases.leading(mean, cov, n, od), T, Sigma, od, dtype=LD)
    full = cases.formula(mean, cov, T, Sigma, od, dtype=LD)
    assert np.array_equal(mu, full[0][:n]) and np.abs(Cn - full[1][:n * od, :n * od]).max() <= 1e-18 * np.abs(Cn).max()


def test_the_chain_finds_the_planted_pairs_and_pulls_the_unmatched_objects_into_place():
    ch = cases.chain()
    ref = cases.chain_reference()
    assert sorted(ref.pairs) == sorted(cases.planted(ch)) and len(ref.pairs) == cases.N_SHARED
    assert sorted(zip(ref.keep.tolist(), ref.drop.tolist())) == sorted(cases.planted(ch))
    d = np.asarray(ch.T_est - ch.T_true, dtype=LD)
    assert d @ cases.inv_ld(ch.Sigma) @ d < 1.0                                      # the estimate of the transform is off by less than its Sigma
    n_a = len(ch.mean_a)
    moved = cases.extra_distances(ch, ref.moved_mean[cases.N_SHARED:])
    fused = cases.extra_distances(ch, ref.fused_mean[n_a:])                          # the 8 copies are dropped: B's own objects follow A's
    print("B's own objects, centre distance from the truth: after the move %s, after the merge %s" % (np.round(moved, 4), np.round(fused, 4)))
    assert len(fused) == cases.N_EXTRA and (fused < moved).all()
    # numpy's fp64 run of the same chain: the same pairs, within 1e-12 of the long-double one
    r64 = cases.run_chain(ch, dtype=np.float64)
    assert r64.pairs == ref.pairs and np.array_equal(r64.drop, ref.drop)
    e64 = max(cases.errors(r64.fused_mean, r64.fused_cov, ref.fused_mean, ref.fused_cov))
    print("the chain in numpy's fp64 within %.2e of the long-double chain" % e64)
    assert e64 <= 1e-12
