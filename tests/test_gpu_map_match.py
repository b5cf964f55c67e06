"""GPU (-m gpu): duplicate objects of a device-resident map proposed on the device (include/obvi_map_match.h) through the C ABI, on a handle that lends only
its device, stream and workspaces.  The reference is the header's formula in long double (tests/map_match_cases.py; held against a constrained least squares on
the CPU by tests/test_map_match_abi.py) -- never the product.  Bars: every reported statistic within 1e-12 relative of the reference (numpy's fp64 evaluation of
the same formula is within 7.5e-16 on these inputs; three orders over that for another order of the sums); the reported set, its order, the yaw offsets and the
three counts exact -- every gate and distance lies midway between two neighbours of the sorted reference, at least 1e-9 apart, so membership is never a matter
of rounding; and bit-equality where the contract promises it.

Measured on the MI355X: the worst reported statistic within 8.8e-16 of the reference (large map, od 7, whole block; od 9: 6.9e-16), 3.0e-16 ..
7.1e-16 on every other map and mask."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (loaded before libobvi_ba.so: torch brings its own HIP runtime, and the one that is loaded first is the one that finds the device)

import helpers
import map_match_cases as cases
import obvi_ba
from map_update_cases import N_SMALL
from test_gpu_map_resident import N_MAP, the_map
from map_support import det_objects_only, last_error, objects_only, status_of

pytestmark = pytest.mark.gpu

T = obvi_ba.FACTOR_MAP_GROUP_PRIOR
INF = float("inf")


def device_map(name, od, n=None):
    mean, cov = cases.case_map(name, od)
    if n is not None:
        mean, cov = cases.leading_map(mean, cov, n, od)
    return obvi_ba.Map.create(mean, cov, object_block_size=od, library=helpers.PRODUCT_LIB)


@functools.lru_cache(maxsize=None)
def lender(od, deterministic=False):
    """A handle that only lends its stream and workspaces; one per block size for the whole module."""
    return (det_objects_only if deterministic else objects_only)(np.zeros((1, od)), od)


def check(mp, ba, ref, od, mask, gate, labels=None, dist=INF, period=0.0, capacity=None):
    """One call against the reference; returns the largest relative error of a reported statistic (0 if none is reported)."""
    found, counts = cases.expected(ref, gate, labels, dist)
    a, b, s, w, got = mp.match(ba, gate, labels, cases.mask_of(mask, od), dist, period, capacity)
    assert got == counts, (got, counts)
    want = np.flatnonzero(found)[:counts[0] if capacity is None else min(capacity, counts[0])]
    assert np.array_equal(a, ref.a[want]) and np.array_equal(b, ref.b[want])        # the set, and its (a, b) order: the reference's pairs are in that order
    assert (a < b).all() and all((a[i], b[i]) < (a[i + 1], b[i + 1]) for i in range(len(a) - 1))
    assert np.array_equal(w, ref.yaw[want])
    assert not ref.singular[want].any()
    return float((np.abs(s - ref.stat[want]) / ref.stat[want]).max()) if len(want) else 0.0


# ---- 1. every map and mask against the formula in long double -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,od,mask", [(w, od, m) for od in (7, 9) for w in ("small", "large", "planted", "copies") for m in cases.MASKS])
def test_the_reported_pairs_and_their_statistics(which, od, mask):
    ref = cases.reference(which, od, mask)
    ba = lender(od)
    worst = 0.0
    with device_map(which, od) as mp:
        for gate in cases.gates(ref):                                               # none, one, about twenty, all
            worst = max(worst, check(mp, ba, ref, od, mask, gate))
        _, _, _, _, counts = mp.match(ba, cases.gates(ref)[-1], row_mask=cases.mask_of(mask, od))
    n = len(cases.case_map(which, od)[0])
    singular = len(cases.COPIES_SINGULAR) if which == "copies" else 0
    assert counts == (n * (n - 1) // 2 - singular, n * (n - 1) // 2, singular)     # the exact copies are counted, never reported, and disturb no other pair
    print("%s map, od %d, mask %s (%d pairs): statistics within %.2e of the long-double formula" % (which, od, mask, n * (n - 1) // 2, worst))
    assert worst <= 1e-12


# ---- 2. the block edges of the pair kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("od", [7, 9])
def test_leading_sub_maps_of_one_to_thirty_three_objects(od):
    full = cases.reference("large", od)
    ba = lender(od)
    worst = 0.0
    for n in range(1, cases.N_SWEEP + 1):
        ref = cases.leading(full, n)
        with device_map("large", od, n) as mp:
            if n == 1:
                assert mp.match(ba, 1.0)[4] == (0, 0, 0) and mp.match(ba, 1.0, capacity=4)[4] == (0, 0, 0)
                continue
            p = n * (n - 1) // 2
            for count in sorted({p // 2, p}):                                       # half of the pairs, all of them (n = 2: none, then the one)
                gate, _ = cases.midpoint(ref.stat, count)
                worst = max(worst, check(mp, ba, ref, od, "all", gate))
    print("od %d, sub-maps of 1 .. %d objects: statistics within %.2e" % (od, cases.N_SWEEP, worst))
    assert worst <= 1e-12


def test_a_row_of_one_sweep_of_candidates_and_of_one_more():
    """The scatter walks a row's candidates 256 at a time: row 0 of 257 objects has exactly one sweep of them, of 258 objects one more than a sweep."""
    od = 7
    full = cases.reference("sweep", od)
    assert not full.singular.any()
    ba = lender(od)
    worst = 0.0
    for n in (cases.N_EDGE - 1, cases.N_EDGE):
        ref = cases.leading(full, n)
        assert int((ref.a == 0).sum()) == n - 1 and n - 1 in (256, 257)
        p = n * (n - 1) // 2
        with device_map("sweep", od, n) as mp:
            worst = max(worst, check(mp, ba, ref, od, "all", cases.midpoint(ref.stat, p // 2)[0]))   # half of the pairs
            gate, found = cases.midpoint(ref.stat, p)                                                 # all of them: row 0 reports every candidate
            assert found == p
            for capacity in (None, 256, 257):                                                         # 256: the reported prefix ends at the sweep's edge
                worst = max(worst, check(mp, ba, ref, od, "all", gate, capacity=capacity))
    print("od %d, sub-maps of %d and %d objects: statistics within %.2e" % (od, cases.N_EDGE - 1, cases.N_EDGE, worst))
    assert worst <= 1e-12


# ---- 3. capacity ----------------------------------------------------------------------------------------------------------------------------------------------
def test_a_capacity_below_the_count_reports_a_prefix_and_the_whole_count():
    od = 7
    ref = cases.reference("large", od)
    gate, found = cases.midpoint(ref.stat, 20)
    ba = lender(od)
    with device_map("large", od) as mp:
        for capacity in (0, 1, found - 1, found, found + 5, None):
            assert check(mp, ba, ref, od, "all", gate, capacity=capacity) <= 1e-12
        a, b, s, w, counts = mp.match(ba, gate, capacity=0)                         # count only: NULL arrays
        assert len(a) == len(b) == len(s) == len(w) == 0 and counts[0] == found
        # behind the reported pairs the caller's arrays are not written
        lib = ba._lib
        lib.obvi_map_match.restype = C.c_int
        ia, ib, st, yw = np.full(found + 3, 77, np.uint32), np.full(found + 3, 77, np.uint32), np.full(found + 3, 77.0), np.full(found + 3, 77.0)
        cnt = np.zeros(3, np.int64)
        rc = lib.obvi_map_match(ba._h, mp._m, None, C.c_uint32(0), C.c_double(gate), C.c_double(INF), C.c_double(0.0), C.c_int64(found + 3),
                                *(x.ctypes.data_as(C.c_void_p) for x in (ia, ib, st, yw, cnt)))
        assert rc == 0 and cnt[0] == found and (ia[found:] == 77).all() and (ib[found:] == 77).all() and (st[found:] == 77).all() and (yw[found:] == 77).all()
        assert (ia[:found] < ib[:found]).all()


# ---- 4. labels and the centre distance --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("od", [7, 9])
def test_labels_and_the_centre_distance_decide_what_is_tested(od):
    ref = cases.reference("large", od, "centre")
    gate = cases.gates(ref)[-1]                                                     # everything tested is found
    rng = np.random.default_rng(60 + od)
    ba = lender(od)
    with device_map("large", od) as mp:
        distinct = np.arange(N_MAP, dtype=np.int32)
        assert mp.match(ba, gate, distinct)[4] == (0, 0, 0)                         # all labels distinct: nothing is tested
        classes = rng.integers(0, 5, N_MAP).astype(np.int32)
        assert check(mp, ba, ref, od, "centre", gate, labels=classes) <= 1e-12
        one_out = np.zeros(N_MAP, np.int32)
        one_out[17] = -1                                                            # a negative label takes its object out of every pair
        assert check(mp, ba, ref, od, "centre", gate, labels=one_out) <= 1e-12
        assert cases.expected(ref, gate, one_out)[1][1] == (N_MAP - 1) * (N_MAP - 2) // 2
        both_out = one_out.copy()
        both_out[40] = -1                                                           # ... and two negative labels are no pair either
        assert check(mp, ba, ref, od, "centre", gate, labels=both_out) <= 1e-12
        for count in (0, 1, len(ref.a) // 2, len(ref.a)):
            D, k = cases.midpoint(ref.dist, count)
            assert check(mp, ba, ref, od, "centre", gate, dist=D) <= 1e-12
            assert cases.expected(ref, gate, None, D)[1][1] == k
        D, _ = cases.midpoint(ref.dist, len(ref.a) // 2)
        some = cases.midpoint(ref.stat, len(ref.a) // 3)[0]
        assert check(mp, ba, ref, od, "centre", some, labels=classes, dist=D) <= 1e-12   # all three tests together


# ---- 5. the yaw period -------------------------------------------------------------------------------------------------------------------------------------------
def test_a_copy_turned_by_half_a_turn_is_found_with_the_period_and_not_without():
    od, period = 7, float(np.pi)
    lab = cases.planted_labels(od)
    plain, wrapped = cases.reference("planted_yaw", od), cases.reference("planted_yaw", od, "all", period)
    t = cases.tested(wrapped, lab)
    gate, k = cases.midpoint(wrapped.stat[t], cases.N_COPIES)
    assert k == cases.N_COPIES
    turned = cases.planted_pairs(od)[2]
    ba = lender(od)
    with device_map("planted_yaw", od) as mp:
        assert check(mp, ba, wrapped, od, "all", gate, labels=lab, period=period) <= 1e-12
        a, b, s, w, counts = mp.match(ba, gate, lab, yaw_period=period)
        assert counts == (5, 5, 0) and [(int(x), int(y)) for x, y in zip(a, b)] == cases.planted_pairs(od)
        assert w[2] == np.pi and not w[[0, 1, 3, 4]].any()
        assert check(mp, ba, plain, od, "all", gate, labels=lab) <= 1e-12
        a, b, s, w, counts = mp.match(ba, gate, lab)
        assert counts == (4, 5, 0) and turned not in [(int(x), int(y)) for x, y in zip(a, b)] and not w.any()
        # the offset is reported whether or not row 3 is in the mask
        no_yaw = cases.reference("planted_yaw", od, "no_yaw", period)
        assert check(mp, ba, no_yaw, od, "no_yaw", cases.gates(no_yaw)[-1], labels=lab, period=period) <= 1e-12
        assert mp.match(ba, cases.gates(no_yaw)[-1], lab, cases.mask_of("no_yaw", od), yaw_period=period)[3][2] == np.pi
        assert check(mp, ba, wrapped, od, "all", cases.gates(wrapped)[2], period=period) <= 1e-12   # ... and with no labels, on every pair


# ---- 6. the contract ---------------------------------------------------------------------------------------------------------------------------------------------
def test_the_same_call_twice_and_on_either_kind_of_handle_gives_the_same_bits_and_writes_neither_map_nor_handle():
    od = 7
    mean, cov = the_map(od)
    ref = cases.reference("large", od)
    gate = cases.gates(ref)[2]
    rng = np.random.default_rng(9)
    user = objects_only(rng.normal(size=(N_MAP, od)), od)
    out = []
    with device_map("large", od) as mp:
        user.set_map_group_priors_from_map(mp, [[5, 1, 9], [2, 0]], [[60, 3, 33], [12, 44]], 1e6)
        r0, W0, _ = user.debug_linearize(T)
        err0 = last_error(user)
        for ba in (user, lender(od), lender(od, deterministic=True)):
            for _ in range(2):
                out.append(mp.match(ba, gate, max_centre_distance=cases.midpoint(ref.dist, 2000)[0]))
        after = mp.get()
        r, W, _ = user.debug_linearize(T)
        assert last_error(user) == err0 and user._fn("ba_num_factors")(user._h, C.c_int32(T)) == 2 and all(np.array_equal(x, y) for x, y in zip(W + r, W0 + r0))
    assert len(out[0][0]) > 0
    for o in out[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(o[:4], out[0][:4])) and o[4] == out[0][4]
    assert np.array_equal(after[0], mean) and np.array_equal(after[1], cov)         # the map is as it was
    assert status_of(lambda: user.solve(helpers.ba_params(max_it=3))) == 0          # the handle is usable
    user.close()


def test_refusals_leave_the_handle_and_the_outputs_as_they_were():
    od = 7
    mean, cov = the_map(od)
    ref = cases.reference("large", od)
    gate = cases.gates(ref)[2]
    rng = np.random.default_rng(9)
    ba = objects_only(rng.normal(size=(N_MAP, od)), od)
    mp = obvi_ba.Map.create(mean, cov, library=helpers.PRODUCT_LIB)
    ba.set_map_group_priors_from_map(mp, [[5, 1, 9], [2, 0]], [[60, 3, 33], [12, 44]], 1e6)
    r0, W0, _ = ba.debug_linearize(T)
    lib = ba._lib
    lib.obvi_map_match.restype = C.c_int
    lab = np.zeros(N_MAP, np.int32)

    def call(says, m=mp, mask=0, g=gate, dist=INF, period=0.0, cap=4, null=(), counts=True):
        out = [np.full(4, 77, np.uint32), np.full(4, 77, np.uint32), np.full(4, 77.0), np.full(4, 77.0)]
        cnt = np.full(3, 77, np.int64)
        ptrs = [None if i in null else x.ctypes.data_as(C.c_void_p) for i, x in enumerate(out)]
        rc = lib.obvi_map_match(ba._h, m._m if m is not None else None, lab.ctypes.data_as(C.c_void_p), C.c_uint32(mask), C.c_double(g), C.c_double(dist), C.c_double(period),
                                C.c_int64(cap), *ptrs, cnt.ctypes.data_as(C.c_void_p) if counts else None)
        assert says in last_error(ba), (says, last_error(ba))
        assert all((x == 77).all() for x in out) and (cnt == 77).all()                # nothing is written
        r, W, _ = ba.debug_linearize(T)
        assert ba._fn("ba_num_factors")(ba._h, C.c_int32(T)) == 2 and all(np.array_equal(x, y) for x, y in zip(W + r, W0 + r0))
        assert check(mp, ba, ref, od, "all", gate) <= 1e-12                          # a valid call goes through
        return rc

    # null pointers and counts
    assert call("bad arguments", m=None) == -1 and call("bad arguments", counts=False) == -1 and call("bad arguments", cap=-1) == -1
    assert all(call("bad arguments", null=(i,)) == -1 for i in range(4))
    # the map's side
    with obvi_ba.Map.create(np.zeros((3, 9)), np.eye(27), object_block_size=9, library=helpers.PRODUCT_LIB) as nine:
        assert call("block size", m=nine) == -1
    if torch.cuda.device_count() > 1:                                   # NOT exercised where the suite sees one GPU: the one refusal of the contract this test cannot reach there
        with obvi_ba.Map.create(mean, cov, device_id=1, library=helpers.PRODUCT_LIB) as far:
            assert call("another device", m=far) == -1
    # the mask, the gate, the distance, the period
    assert call("row_mask", mask=1 << 7) == -1 and call("row_mask", mask=0x80000001) == -1
    assert all(call("gate", g=g) == -1 for g in (0.0, -1.0, np.nan, np.inf))
    assert all(call("max_centre_distance", dist=d) == -1 for d in (0.0, -2.0, np.nan, -np.inf))
    assert all(call("yaw_period", period=p) == -1 for p in (-1.0, np.nan, np.inf))
    nine_ba = lender(9)
    with obvi_ba.Map.create(np.zeros((3, 9)), np.eye(27), object_block_size=9, library=helpers.PRODUCT_LIB) as nine:
        assert status_of(lambda: nine.match(nine_ba, 1.0, yaw_period=1.0)) == -1 and "7-parameter" in last_error(nine_ba)
        assert status_of(lambda: nine.match(nine_ba, 1.0, row_mask=1 << 9)) == -1 and status_of(lambda: nine.match(nine_ba, 1.0, row_mask=1 << 8)) == 0
    mp.close()
    assert status_of(lambda: ba.solve(helpers.ba_params(max_it=3))) == 0             # the handle is usable
    ba.close()


# ---- 7. from the match to the fused map ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,od", [("planted_yaw", 7), ("planted", 9)])
def test_match_resolve_and_merge_end_to_end(which, od):
    period = float(np.pi) if od == 7 else 0.0
    lab = cases.planted_labels(od)
    ref = cases.reference(which, od, "all", period)
    t = cases.tested(ref, lab)
    gate, _ = cases.midpoint(ref.stat[t], cases.N_COPIES)
    pairs = cases.planted_pairs(od)
    ba = lender(od)
    with device_map(which, od) as mp:
        a, b, s, w, counts = mp.match(ba, gate, lab, yaw_period=period)
        assert counts == (5, 5, 0) and [(int(x), int(y)) for x, y in zip(a, b)] == pairs                  # exactly the five planted pairs
        drop, keep, sel = obvi_ba.map_match_resolve(od, a, b, s, library=helpers.PRODUCT_LIB)
        offset = np.zeros((len(drop), od))
        offset[:, 3] = w[sel]
        fused, where = mp.merge(ba, drop, keep, offset)
        # the same lists written by hand: the copies into their sources, in the order of the reference's statistics; the turned copy's offset is pi
        order = np.argsort(ref.stat[t].astype(np.float64))
        hand_drop, hand_keep = [pairs[i][1] for i in order], [pairs[i][0] for i in order]
        hand_offset = np.zeros((5, od))
        if od == 7:
            hand_offset[list(order).index(2), 3] = np.pi
        assert list(drop) == hand_drop and list(keep) == hand_keep and np.array_equal(offset, hand_offset)
        by_hand, where2 = mp.merge(ba, hand_drop, hand_keep, hand_offset)
    with fused, by_hand:
        mu, Cn = fused.get()
        mu2, C2 = by_hand.get()
        assert fused.n_objects == N_SMALL and np.array_equal(mu, mu2) and np.array_equal(Cn, C2) and np.array_equal(where, where2)
        assert np.array_equal(where[N_SMALL:], cases.planted_sources(od))                                # every copy went into its source
        # a second match on the fused map finds none of them: the labels that are left are all distinct
        assert fused.match(ba, gate, lab[:N_SMALL], yaw_period=period)[4] == (0, 0, 0)
        a2, b2, _, _, counts2 = fused.match(ba, gate, yaw_period=period)
        assert counts2[1] == N_SMALL * (N_SMALL - 1) // 2 and counts2[2] == 0 and (b2 < N_SMALL).all()
