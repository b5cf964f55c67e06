"""CPU: the match of duplicate objects of a device-resident map (include/obvi_map_match.h) is declared under the obvi_map_ prefix in a header of its own --
exactly two functions, nothing in the obvi_ba_ namespace the oracle mirrors -- exported by libobvi_ba.so, and refuses bad arguments without a device.  The header
includes obvi_map_resident.h alone, no other header names it, and it names none of the neighbouring entries the other headers' tests reserve for their owners.
The resolver needs no device and is tested here in full, against a plain restatement of its greedy rule.
And the reference of tests/test_gpu_map_match.py is itself held: the formula in long double against the constrained least squares of tests/map_match_cases.py at
the bar tests/test_map_update_abi.py sets for the same kind of check (1e-14 relative); numpy's fp64 evaluation of the formula within 1e-12 of the long-double
one -- a condition on the inputs: a case that breaks it is replaced, the GPU bar (1e-12) is not moved.

Measured: the long-double formula within 2.9e-17 of the yardstick on every pair evaluated; numpy's fp64 evaluation within 7.5e-16 on the four maps and the four
masks, 4.1e-16 on the planted maps; the smallest relative gap between two neighbours of a sorted reference 4.5e-8."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import helpers
import map_match_cases as cases
from map_support import header as _header

sys.path.insert(0, helpers.ROOT)
import __graft_entry__ as entry  # noqa: E402

SYMBOLS = ["obvi_map_match", "obvi_map_match_resolve"]
RESERVED = ["map_merge", "map_update", "obvi_map_condition", "obvi_map_get", "map_extend", "obvi_map_extend", "obvi_map_select"]
U32, F64 = C.POINTER(C.c_uint32), C.POINTER(C.c_double)


def test_the_header_declares_the_two_entries_and_the_library_exports_them():
    assert entry.abi_symbols("obvi_map_match.h", "obvi_map_") == SYMBOLS
    assert entry.abi_symbols("obvi_map_match.h", "obvi_ba_") == []                  # nothing there for the oracle to mirror
    lib = C.CDLL(helpers.PRODUCT_LIB)
    for s in SYMBOLS:
        assert hasattr(lib, s), s


def test_the_header_includes_the_resident_map_alone_and_no_other_header_mentions_it():
    txt = _header("obvi_map_match.h")
    assert re.findall(r'#include\s+"([^"]+)"', txt) == ["obvi_map_resident.h"]
    for word in RESERVED:
        assert word not in txt, word
    for other in sorted(os.listdir(os.path.join(helpers.ROOT, "include"))):
        if other != "obvi_map_match.h":
            assert "map_match" not in _header(other), other


def test_bad_arguments_of_the_match_are_refused_without_a_device():
    lib = C.CDLL(helpers.PRODUCT_LIB)
    lib.obvi_map_match.restype = C.c_int
    null, fake = C.c_void_p(), C.c_void_p(8)                                        # fake: never dereferenced, another argument is refused first
    a, b, s, w = np.full(4, 77, np.uint32), np.full(4, 77, np.uint32), np.full(4, 77.0), np.full(4, 77.0)
    counts = np.full(3, 77, np.int64)
    pa, pb, ps, pw, pc = (x.ctypes.data_as(C.c_void_p) for x in (a, b, s, w, counts))
    # (the same beside a live handle: test_gpu_map_match.py -- the refusal is written into the handle's last error)
    for m, cap, oa, ob, os_, ow, oc in ((fake, 4, pa, pb, ps, pw, pc), (null, 4, pa, pb, ps, pw, pc), (fake, 4, pa, pb, ps, pw, None), (fake, -1, pa, pb, ps, pw, pc),
                                        (fake, 4, None, pb, ps, pw, pc), (fake, 4, pa, None, ps, pw, pc), (fake, 4, pa, pb, None, pw, pc), (fake, 4, pa, pb, ps, None, pc),
                                        (fake, 0, None, None, None, None, pc)):
        for gate, dist, period, mask in ((1.0, np.inf, 0.0, 0), (np.nan, 1.0, 0.0, 0), (1.0, -1.0, 0.0, 0), (1.0, 1.0, -1.0, 0), (1.0, 1.0, 0.0, 1 << 9)):
            assert lib.obvi_map_match(null, m, None, C.c_uint32(mask), C.c_double(gate), C.c_double(dist), C.c_double(period), C.c_int64(cap), oa, ob, os_, ow, oc) == -1
    assert (a == 77).all() and (b == 77).all() and (s == 77).all() and (w == 77).all() and (counts == 77).all()


# ---- the resolver: host only ---------------------------------------------------------------------------------------------------------------------------------
def resolve_raw(od, a, b, stat, max_pairs, n_pairs=None, null=()):
    """(rc, drop, keep, sel, q) of a raw call; the outputs start as sentinels."""
    lib = C.CDLL(helpers.PRODUCT_LIB)
    lib.obvi_map_match_resolve.restype = C.c_int
    a, b, stat = np.ascontiguousarray(a, np.uint32), np.ascontiguousarray(b, np.uint32), np.ascontiguousarray(stat, np.float64)
    room = max(1, max_pairs, len(a))
    drop, keep, sel = (np.full(room, 0xABCD1234, np.uint32) for _ in range(3))
    q = C.c_int64(-77)
    args = {"a": a.ctypes.data_as(U32), "b": b.ctypes.data_as(U32), "stat": stat.ctypes.data_as(F64), "drop": drop.ctypes.data_as(U32), "keep": keep.ctypes.data_as(U32),
            "sel": sel.ctypes.data_as(U32), "q": C.byref(q)}
    for k in null:
        args[k] = None
    rc = lib.obvi_map_match_resolve(C.c_int32(od), C.c_int64(len(a) if n_pairs is None else n_pairs), args["a"], args["b"], args["stat"], C.c_int64(max_pairs),
                                    args["drop"], args["keep"], args["sel"], args["q"])
    return rc, drop, keep, sel, q.value


def greedy(a, b, stat, max_pairs):
    """The rule of the header, restated."""
    FREE, KEEP, DROPPED = 0, 1, 2
    state, out = {}, []
    for i in sorted(range(len(a)), key=lambda i: (stat[i], a[i], b[i], i)):
        if len(out) == max_pairs:
            break
        if state.get(a[i], FREE) in (FREE, KEEP) and state.get(b[i], FREE) == FREE:
            state[a[i]], state[b[i]] = KEEP, DROPPED
            out.append((b[i], a[i], i))
    return out


def untouched(drop, keep, sel, q):
    return (drop == 0xABCD1234).all() and (keep == 0xABCD1234).all() and (sel == 0xABCD1234).all() and q == -77


def test_every_refusal_of_the_resolver_leaves_the_outputs_untouched():
    a, b, s = [0, 1], [1, 2], [1.0, 2.0]
    for name in ("a", "b", "stat", "drop", "keep", "sel", "q"):
        rc, *out = resolve_raw(7, a, b, s, 4, null=(name,))
        assert rc == -1 and untouched(*out), name
    for kw in (dict(n_pairs=-1), dict(max_pairs=0), dict(max_pairs=-3), dict(od=5), dict(od=8), dict(a=[1, 1]), dict(a=[0, 3])):   # a >= b: equal, above
        args = dict(od=7, a=a, b=b, stat=s, max_pairs=4)
        args.update(kw)
        rc, *out = resolve_raw(**args)
        assert rc == -1 and untouched(*out), kw
    for bad in (-1e-300, np.nan, np.inf, -np.inf):
        rc, *out = resolve_raw(7, a, b, [1.0, bad], 4)
        assert rc == -6 and untouched(*out), bad
    # the cap of the fusing entry: max_pairs od rows
    assert resolve_raw(7, a, b, s, 293)[0] == -1 and resolve_raw(7, a, b, s, 292)[0] == 0       # 2051 > 2048; 2044
    assert resolve_raw(0, a, b, s, 293)[0] == -1 and resolve_raw(0, a, b, s, 292)[0] == 0       # a block size of 0 reads 7
    assert resolve_raw(9, a, b, s, 228)[0] == -1 and resolve_raw(9, a, b, s, 227)[0] == 0       # 2052; 2043
    rc, drop, keep, sel, q = resolve_raw(7, [], [], [], 4)
    assert rc == 0 and q == 0 and (drop == 0xABCD1234).all()


@pytest.mark.parametrize("seed", range(8))
def test_the_resolver_is_the_greedy_rule_and_its_output_is_what_the_fusing_entry_accepts(seed):
    rng = np.random.default_rng(900 + seed)
    n, p = int(rng.integers(4, 40)), int(rng.integers(1, 120))
    a, b = rng.integers(0, n - 1, p), rng.integers(0, n, p)
    a, b = np.minimum(a, b), np.maximum(a, b)
    b = np.where(a == b, b + 1, b)
    stat = np.round(rng.uniform(0, 4, p), 1 if seed % 2 else 12)                    # odd seeds: many ties
    max_pairs = [292, 3, 1, 7][seed % 4]
    rc, drop, keep, sel, q = resolve_raw(7, a, b, stat, max_pairs)
    want = greedy(list(a), list(b), list(stat), max_pairs)
    assert rc == 0 and q == len(want) <= max_pairs
    assert [(int(d), int(k), int(i)) for d, k, i in zip(drop[:q], keep[:q], sel[:q])] == [(int(d), int(k), int(i)) for d, k, i in want]
    assert (drop[q:] == 0xABCD1234).all() and (keep[q:] == 0xABCD1234).all() and (sel[q:] == 0xABCD1234).all()
    assert len(set(drop[:q])) == q                                                   # no object dropped twice
    assert not set(drop[:q]) & set(keep[:q])                                         # no dropped object kept
    assert (drop[:q] != keep[:q]).all()
    assert all(a[i] == k and b[i] == d for d, k, i in zip(drop[:q], keep[:q], sel[:q]))


def test_a_chain_loses_its_later_link_ties_go_by_index_and_the_cap_stops_it():
    # b into a, then c into b: the second is dropped whichever comes first in the input
    for order in ((0, 1), (1, 0)):
        a, b, s = np.array([3, 5])[list(order)], np.array([5, 9])[list(order)], np.array([1.0, 2.0])[list(order)]
        rc, drop, keep, sel, q = resolve_raw(7, a, b, s, 10)
        assert rc == 0 and q == 1 and (drop[0], keep[0], sel[0]) == (5, 3, order.index(0))
    # ... and when c into b is the better pair, it is b into a that goes
    rc, drop, keep, sel, q = resolve_raw(7, [3, 5], [5, 9], [2.0, 1.0], 10)
    assert q == 1 and (drop[0], keep[0], sel[0]) == (9, 5, 1)
    # a survivor takes several: (1, 4) and (1, 6) both
    rc, drop, keep, sel, q = resolve_raw(7, [1, 1], [4, 6], [2.0, 1.0], 10)
    assert q == 2 and list(drop[:2]) == [6, 4] and list(keep[:2]) == [1, 1] and list(sel[:2]) == [1, 0]
    # ties in stat: (a, b) decides, not the input order -- (2, 9) and (2, 7) and (1, 9) at the same stat: (1, 9) first, then (2, 7); (2, 9) finds 9 dropped
    rc, drop, keep, sel, q = resolve_raw(7, [2, 2, 1], [9, 7, 9], [1.0, 1.0, 1.0], 10)
    assert q == 2 and list(zip(drop[:2], keep[:2], sel[:2])) == [(9, 1, 2), (7, 2, 1)]
    # max_pairs
    rc, drop, keep, sel, q = resolve_raw(7, [0, 2, 4, 6], [1, 3, 5, 7], [4.0, 3.0, 2.0, 1.0], 2)
    assert q == 2 and list(drop[:2]) == [7, 5] and drop[2] == 0xABCD1234
    rc, drop, keep, sel, q = resolve_raw(9, [0, 2, 4, 6], [1, 3, 5, 7], [4.0, 3.0, 2.0, 1.0], 4)
    assert q == 4 and list(sel[:4]) == [3, 2, 1, 0]


def test_the_python_binding_has_both():
    import obvi_ba
    assert callable(getattr(obvi_ba.Map, "match", None)) and callable(getattr(obvi_ba, "map_match_resolve", None))
    drop, keep, sel = obvi_ba.map_match_resolve(7, [3, 5, 0], [5, 9, 2], [1.0, 2.0, 0.5], library=helpers.PRODUCT_LIB)
    assert list(drop) == [2, 5] and list(keep) == [0, 3] and list(sel) == [2, 0]
    drop, keep, sel = obvi_ba.map_match_resolve(9, [], [], [], library=helpers.PRODUCT_LIB)
    assert len(drop) == len(keep) == len(sel) == 0
    with pytest.raises(obvi_ba.ObviError):
        obvi_ba.map_match_resolve(7, [3], [3], [1.0], library=helpers.PRODUCT_LIB)
    with pytest.raises(obvi_ba.ObviError, match="served by libobvi_ba.so only"):
        obvi_ba.map_match_resolve(7, [0], [1], [1.0], library=helpers.PRODUCT_LIB, prefix="oracle_")


# ---- the reference of the GPU tests is itself held --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,od,mask", [(w, od, m) for od in (7, 9) for w in ("small", "large") for m in ("all", "centre")])
def test_the_yardstick_is_held_by_the_formula_in_long_double(which, od, mask):
    ref = cases.reference(which, od, mask)
    idx = cases.yardstick_pairs(which, od)
    want = cases.yardstick_reference(which, od, mask)
    assert len(idx) == (276 if which == "small" else 40) and not ref.singular.any()
    e = float((np.abs(ref.stat[idx] - want) / want).max())
    print("%s map, od %d, mask %s: the formula within %.2e of the constrained least squares on %d pairs" % (which, od, mask, e, len(idx)))
    assert e <= 1e-14


def test_a_wrapped_pair_is_the_least_squares_with_the_wrap_as_its_constraint():
    """w enters the yardstick as the right-hand side of the constraint x_b - x_a = w e_3; the formula takes it out of d."""
    od, a, b = 7, 4, 19
    mean, cov = (np.array(x) for x in cases.map_of("small", od))
    mean[b, 3] += cases.YAW_TURN
    ref = cases.formula(mean, cov, od, 0, float(np.pi))
    i = int(np.flatnonzero((ref.a == a) & (ref.b == b))[0])
    assert ref.yaw[i] == np.pi
    want = cases.yardstick(mean, cases.map_information("small", od), od, a, b, 0, w=np.longdouble(np.pi))
    assert abs(ref.stat[i] - want) <= 1e-14 * want
    assert abs(cases.formula(mean, cov, od, 0, 0.0).stat[i] - want) > 0.1 * want                       # ... and without the wrap it is another number


CONDITION = [(w, od, m, 0.0) for od in (7, 9) for w in ("small", "large", "planted", "copies") for m in cases.MASKS] + [("planted_yaw", 7, "all", 0.0), ("planted_yaw", 7, "all", float(np.pi))]


@pytest.mark.parametrize("which,od,mask,period", CONDITION)
def test_numpy_in_fp64_stays_within_the_condition_on_the_inputs(which, od, mask, period):
    mean, cov = cases.case_map(which, od)
    ref = cases.reference(which, od, mask, period)
    got = cases.formula(mean, cov, od, cases.mask_of(mask, od), period, dtype=np.float64)
    assert np.array_equal(got.singular, ref.singular) and np.array_equal(got.a, ref.a)
    assert [(int(a), int(b)) for a, b in zip(ref.a[ref.singular], ref.b[ref.singular])] == (cases.COPIES_SINGULAR if which == "copies" else [])
    ok = ~ref.singular
    e = float((np.abs(got.stat[ok] - ref.stat[ok]) / ref.stat[ok]).max())
    v = np.sort(ref.stat[ok])
    gap = float(((v[1:] - v[:-1]) / v[1:]).min())
    print("%s map, od %d, mask %s, period %.3g: numpy's fp64 evaluation within %.2e of the long-double formula; smallest relative gap of the sorted reference %.2e"
          % (which, od, mask, period, e, gap))
    assert e <= 1e-12                                                                # the inputs are ones fp64 can be held to 1e-12 on
    for gate in cases.gates(ref):                                                    # every gate the GPU tests use separates its neighbours by 1e-9
        below, above = v[v <= gate], v[v > gate]
        assert gate > 0 and (len(below) == 0 or gate - below[-1] >= 0.4e-9 * gate) and (len(above) == 0 or above[0] - gate >= 0.4e-9 * gate)


def test_the_sub_maps_reference_is_a_slice_of_the_large_maps():
    od, n = 7, 12
    mean, cov = cases.map_of("large", od)
    sub = cases.formula(*cases.leading_map(mean, cov, n, od), od)
    cut = cases.leading(cases.reference("large", od), n)
    assert np.array_equal(sub.a, cut.a) and np.array_equal(sub.b, cut.b) and np.array_equal(sub.stat, cut.stat)


def test_the_planted_copies_are_where_the_labels_say():
    for od in (7, 9):
        lab = cases.planted_labels(od)
        ref = cases.reference("planted", od)
        t = cases.tested(ref, lab)
        assert [(int(a), int(b)) for a, b in zip(ref.a[t], ref.b[t])] == sorted(cases.planted_pairs(od))
    ref, wrapped = cases.reference("planted_yaw", 7), cases.reference("planted_yaw", 7, "all", float(np.pi))
    a, b = cases.planted_pairs(7)[2]
    i = int(np.flatnonzero((ref.a == a) & (ref.b == b))[0])
    assert wrapped.yaw[i] == np.pi and wrapped.stat[i] < 0.2 * ref.stat[i]
