"""CPU: the bounding-box data association (include/obvi_bbox_frontend.h) is declared under the obvi_bbox_frontend_ prefix in a header of its own, exported by
libobvi_ba.so and bound in obvi_ba.py; the device entry refuses bad arguments before any device work and leaves its outputs untouched; the greedy assignment
needs no device and is tested here in full against the restatement of tests/bbox_frontend_cases.py; and that restatement is itself held on a hand-computed case."""
import ctypes as C
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

import bbox_frontend_cases as cases
import helpers

sys.path.insert(0, helpers.ROOT)
import __graft_entry__ as entry  # noqa: E402

SYMBOLS = ["obvi_bbox_frontend_assign", "obvi_bbox_frontend_associate", "obvi_bbox_frontend_lds_feature_limit"]
I64, U8, F64 = C.POINTER(C.c_int64), C.POINTER(C.c_uint8), C.POINTER(C.c_double)
SENTINEL = cases.SENTINEL


def test_the_header_declares_the_entries_the_library_exports_them_and_the_binding_has_both():
    assert entry.abi_symbols("obvi_bbox_frontend.h", "obvi_bbox_frontend_") == SYMBOLS
    assert entry.abi_symbols("obvi_bbox_frontend.h", "obvi_ba_") == []               # nothing there for the oracle to mirror
    assert '#include "obvi_frontend.h"' in open(os.path.join(helpers.ROOT, "include", "obvi_bbox_frontend.h")).read()
    lib = C.CDLL(helpers.PRODUCT_LIB)
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    lib.obvi_bbox_frontend_lds_feature_limit.restype = C.c_int64
    assert lib.obvi_bbox_frontend_lds_feature_limit() > 64
    import obvi_ba
    assert callable(getattr(obvi_ba.BundleAdjuster, "bbox_associate", None)) and callable(getattr(obvi_ba, "bbox_assign", None))
    with pytest.raises(obvi_ba.ObviError, match="served by libobvi_ba.so only"):
        obvi_ba.bbox_assign(np.ones((1, 1)), np.ones((1, 1)), 0, library=helpers.PRODUCT_LIB, prefix="oracle_")


# ---- the device entry: refusals, which come before any device work -------------------------------------------------------------------------------------
Call, REFUSALS = cases.Call, cases.REFUSALS


def test_a_null_handle_is_refused():
    c = Call()
    assert c.run(None) == -1 and c.untouched()


@pytest.mark.parametrize("name", [r[0] for r in REFUSALS])
def test_every_refusal_of_associate_comes_before_the_device_and_leaves_the_outputs_untouched(name):
    """The entry judges its arguments before it looks at the handle, so a refusal is observed here without a device: beside a NULL handle a non-finite value is
    answered with OBVI_ERR_NUMERICAL (-6), not with the NULL handle's -1.  (The same refusals beside a live handle, where a valid call succeeds and the message
    lands in the handle's last error: tests/test_gpu_bbox_frontend.py.)"""
    _, change, status = next(r for r in REFUSALS if r[0] == name)
    c = Call()
    change(c)
    assert c.run(None) == status and c.untouched()


# ---- the assignment: host only -----------------------------------------------------------------------------------------------------------------------------
def assign_raw(is_match, score, n_pending, n_box=None, n_cand=None, null=()):
    lib = C.CDLL(helpers.PRODUCT_LIB)
    lib.obvi_bbox_frontend_assign.restype = C.c_int
    m, s = np.ascontiguousarray(is_match, np.uint8), np.ascontiguousarray(score, np.float64)
    nb, nc = (m.shape if m.ndim == 2 else (0, 0))
    nb, nc = (nb if n_box is None else n_box), (nc if n_cand is None else n_cand)
    assigned, is_new = np.full(max(1, nb), -77, np.int64), np.full(max(1, nb), SENTINEL, np.uint8)
    args = {"m": m.ctypes.data_as(U8), "s": s.ctypes.data_as(F64), "a": assigned.ctypes.data_as(I64), "n": is_new.ctypes.data_as(U8)}
    for k in null:
        args[k] = None
    rc = lib.obvi_bbox_frontend_assign(C.c_int64(nb), C.c_int64(nc), C.c_int64(n_pending), args["m"], args["s"], args["a"], args["n"])
    return rc, assigned, is_new


def want(is_match, score, n_pending):
    is_match, score = np.asarray(is_match), np.asarray(score, np.float64)
    return cases.greedily_assign([[(c, float(score[b, c])) for c in range(is_match.shape[1]) if is_match[b, c]] for b in range(is_match.shape[0])], n_pending)


def got(assigned, is_new, n_box):
    return [(bool(n), int(a)) for a, n in zip(assigned[:n_box], is_new[:n_box])]


def test_every_refusal_of_assign_leaves_the_outputs_untouched():
    m, s = [[1, 0], [1, 1]], [[0.5, 0.0], [0.25, 0.75]]
    for name in ("m", "s", "a", "n"):
        rc, a, n = assign_raw(m, s, 3, null=(name,))
        assert rc == -1 and (a == -77).all() and (n == SENTINEL).all(), name
    for kw in (dict(n_box=-1), dict(n_cand=-1), dict(n_pending=-1)):
        args = dict(is_match=m, score=s, n_pending=3)
        args.update(kw)
        rc, a, n = assign_raw(**args)
        assert rc == -1 and (a == -77).all() and (n == SENTINEL).all(), kw
    rc, a, n = assign_raw(m, [[0.5, 0.0], [np.nan, 0.75]], 3)
    assert rc == -6 and (a == -77).all() and (n == SENTINEL).all()
    rc, a, n = assign_raw(m, [[0.5, np.nan], [0.25, 0.75]], 3)                       # a NaN where there is no match is never read
    assert rc == 0 and got(a, n, 2) == want(m, s, 3)


@pytest.mark.parametrize("seed", range(8))
def test_assign_is_the_restated_greedy_rule(seed):
    rng = np.random.default_rng(4100 + seed)
    nb, nc, n_pending = int(rng.integers(1, 14)), int(rng.integers(1, 20)), int(rng.integers(0, 9))
    m = (rng.uniform(size=(nb, nc)) < [0.1, 0.4, 0.8, 1.0][seed % 4]).astype(np.uint8)
    s = np.round(rng.uniform(0, 1, (nb, nc)), 1 if seed % 2 else 12)                 # odd seeds: many exact ties
    s[m == 0] = np.nan
    rc, a, n = assign_raw(m, s, n_pending)
    w = want(m, s, n_pending)
    assert rc == 0 and got(a, n, nb) == w
    taken = [c for new, c in w if not new]
    assert len(set(taken)) == len(taken)                                             # no candidate claimed twice
    assert [c for new, c in w if new] == list(range(n_pending, n_pending + sum(new for new, _ in w)))


def test_hand_built_assignments():
    # two boxes want one object: the better score takes it, the loser opens a new pending object
    rc, a, n = assign_raw([[1], [1]], [[0.4], [0.6]], 7)
    assert rc == 0 and got(a, n, 2) == [(True, 7), (False, 0)]
    # ... unless the loser has a second choice
    rc, a, n = assign_raw([[1, 1], [1, 0]], [[0.4, 0.1], [0.6, 0.0]], 7)
    assert got(a, n, 2) == [(False, 1), (False, 0)]
    # an exact tie: the lower box index first
    rc, a, n = assign_raw([[1], [1]], [[0.5], [0.5]], 2)
    assert got(a, n, 2) == [(False, 0), (True, 2)]
    # ... then the lower candidate index: box 0 takes candidate 0 and box 1, tied on both, is left candidate 1
    rc, a, n = assign_raw([[1, 1], [1, 1]], [[0.5, 0.5], [0.5, 0.5]], 2)
    assert got(a, n, 2) == [(False, 0), (False, 1)]
    # boxes without a match among boxes with matches: the new ids count up in box order
    rc, a, n = assign_raw([[0, 0], [1, 0], [0, 0], [0, 1], [0, 0]], np.full((5, 2), 0.3), 4)
    assert got(a, n, 5) == [(True, 4), (False, 0), (True, 5), (False, 1), (True, 6)]
    # no candidates at all, and no boxes
    rc, a, n = assign_raw(np.zeros((3, 0)), np.zeros((3, 0)), 1)
    assert rc == 0 and got(a, n, 3) == [(True, 1), (True, 2), (True, 3)]
    rc, a, n = assign_raw(np.zeros((0, 4)), np.zeros((0, 4)), 1, n_box=0, n_cand=4)
    assert rc == 0 and (a == -77).all() and (n == SENTINEL).all()
    rc, a, n = assign_raw(np.zeros((0, 4)), np.zeros((0, 4)), 1, n_box=0, n_cand=4, null=("m", "s", "a", "n"))
    assert rc == 0


def test_the_binding_of_assign():
    import obvi_ba
    a, n = obvi_ba.bbox_assign([[1, 1], [1, 0]], [[0.4, 0.1], [0.6, np.nan]], 7, library=helpers.PRODUCT_LIB)
    assert list(a) == [1, 0] and list(n) == [0, 0]
    a, n = obvi_ba.bbox_assign(np.zeros((0, 3)), np.zeros((0, 3)), 7, library=helpers.PRODUCT_LIB)
    assert len(a) == len(n) == 0
    with pytest.raises(obvi_ba.ObviError):
        obvi_ba.bbox_assign([[1]], [[np.nan]], 0, library=helpers.PRODUCT_LIB)


# ---- the restatement is itself held -----------------------------------------------------------------------------------------------------------------------
def test_the_restatement_on_a_hand_computed_case():
    """A box holding 6 features (ids 1..6 of 8) against a candidate of 3 views with overlaps 0, 2 and 5:
         view 0 {7, 8, 100}                 n = 0                      no term
         view 1 {1, 2, 101, 102}            n = 2   2 / (6 + 4 - 2) = 1/4
         view 2 {2, 3, 4, 5, 6, 103, 104}   n = 5   5 / (6 + 7 - 5) = 5/8
       score (1/4 + 5/8) / 3 = 7/24; the largest overlap is 5."""
    case = dict(feat_id=[1, 2, 3, 4, 5, 6, 7, 8], feat_pixel=[[10 + i, 20.0] for i in range(6)] + [[40.0, 20.0], [10.0, 60.0]], box_corners=[[10.0, 15.0, 18.0, 22.0]],
                box_label=[2], cand_label=[2, 3, 2], views=[[[7, 8, 100], [1, 2, 101, 102], [2, 3, 4, 5, 6, 103, 104]], [[1, 2, 3, 4, 5, 6]], []],
                inflation=0.0, min_overlap=5.0)
    r = cases.restate(case)
    assert list(r.in_box[0]) == [1, 1, 1, 1, 1, 1, 0, 0] and r.count[0] == 6
    assert list(r.overlap[0]) == [0, 2, 5, 6]
    assert list(r.is_match[0]) == [1, 0, 0]                                          # the second: another class, whatever it shares; the third: no views
    assert Fraction(r.score[0, 0]).limit_denominator(1000) == Fraction(7, 24) and abs(r.score[0, 0] - 7 / 24) <= 2 ** -53
    assert cases.restate(dict(case, min_overlap=5.5)).is_match.sum() == 0            # the threshold is a double
    assert cases.assign_restated(r, 4) == [(False, 0)]


def test_the_scene_of_the_gpu_round_has_well_separated_competitors():
    case, r = cases.scene()
    assert len(case["feat_id"]) == 300 and len(case["box_corners"]) == 9 and len(case["views"]) == 12 and sum(len(v) for v in case["views"]) == 40
    assert len(set(int(x) for x in case["cand_label"])) == 3
    assert cases.competing_scores_are_apart(r, 100.0)
    out = cases.assign_restated(r, case["n_pending"])
    assert any(new for new, _ in out) and sum(not new for new, _ in out) >= 5
    assert (r.is_match.sum(axis=0) >= 2).any()                                       # two boxes compete for one candidate
