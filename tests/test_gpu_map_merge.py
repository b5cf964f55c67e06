"""GPU (-m gpu): duplicate objects of a device-resident map merged on the device (include/obvi_map_merge.h) through the C ABI, on a handle that lends only
its device, stream and workspaces.  The yardstick is the null-space form (exact merges) and the information form (with noise) in long double
(tests/map_merge_cases.py; held against the merge formula on the CPU by tests/test_map_merge_abi.py) -- never the product.  Bars: 1e-11 of the largest entry of
the yardstick for covariances and means -- the bar of tests/test_gpu_map_update.py for the same tile algebra on the same maps; numpy's fp64 evaluation of the
formula on these inputs is within 2.5e-13 -- and bit-equality where the contract promises it (symmetry, repeatability, new_index, the untouched old map and
handle, objects the pairs are not correlated with)."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (loaded before libobvi_ba.so: torch brings its own HIP runtime, and the one that is loaded first is the one that finds the device)

import helpers
import map_extend_cases
import map_merge_cases as cases
import obvi_ba
from map_update_cases import N_SMALL, posterior, rows_of, sym, update_formula
from test_gpu_map_pair_priors import inv_ld, spd
from test_gpu_map_resident import N_MAP, the_map
from map_support import errors, lender, objects_only, status_of

pytestmark = pytest.mark.gpu

T = obvi_ba.FACTOR_MAP_GROUP_PRIOR


def device_map(which, od):
    mean, cov = cases.map_of(which, od)
    return obvi_ba.Map.create(mean, cov, object_block_size=od, library=helpers.PRODUCT_LIB)


def merged(mp, ba, *args):
    """(mean, cov, new_index) of a merge whose map is read back and destroyed."""
    new, where = mp.merge(ba, *args)
    with new:
        mu, Cn = new.get()
        assert new.n_objects == len(mu)
    return mu, Cn, where


# ---- 1. every case against the yardstick ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,od,key,noisy", cases.CASES)
def test_the_merge_at_the_tile_edges(which, od, key, noisy):
    mean, cov = cases.map_of(which, od)
    n = len(mean)
    drop, keep, offset, noise = cases.merge_case(which, od, key, noisy)
    mu_ref, C_ref = cases.merge_reference(which, od, key, noisy)
    want_index, kept = cases.new_index(n, drop, keep)
    ba = lender(od)
    with device_map(which, od) as mp:
        mu, Cn, where = merged(mp, ba, drop, keep, offset, noise)
        old = mp.get()
    eC, em = errors(mu, Cn, mu_ref, C_ref)
    print("%s map, od %d, groups %s%s (%d pair rows, %d -> %d map rows): covariance %.2e  means %.2e" % (which, od, key, ", noise" if noisy else "", len(drop) * od, n * od, mu.size, eC, em))
    assert len(mu) == n - len(drop)
    assert eC <= 1e-11 and em <= 1e-11
    assert np.array_equal(Cn, Cn.T)
    assert np.array_equal(where, want_index)
    rows = rows_of(kept, od)
    assert np.linalg.eigvalsh(Cn).min() > 0
    assert np.linalg.eigvalsh(sym(np.asarray(cov))[np.ix_(rows, rows)] - Cn).min() >= -1e-12 * np.abs(C_ref).max()   # information was added, nowhere removed
    assert np.array_equal(old[0], mean) and np.array_equal(old[1], cov)              # the old map is as it was


# ---- 2. repeatability ----------------------------------------------------------------------------------------------------------------------------------
def test_the_same_call_twice_and_on_either_kind_of_handle_gives_the_same_bits():
    which, od, key = "large", 7, "3x10+2x10"
    args = cases.merge_case(which, od, key, True)
    out = []
    with device_map(which, od) as mp:
        for ba in (lender(od), lender(od, deterministic=True)):
            for _ in range(2):
                out.append(merged(mp, ba, *args))
    for mu, Cn, where in out[1:]:
        assert np.array_equal(mu, out[0][0]) and np.array_equal(Cn, out[0][1]) and np.array_equal(where, out[0][2])


# ---- 3. the choice of survivor is free -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("od", [7, 9])
def test_either_of_the_two_may_survive(od):
    a, b = 5, 17
    ba = lender(od)
    with device_map("small", od) as mp:
        mu1, C1, w1 = merged(mp, ba, [a], [b])                                       # a into b: the survivor is numbered as b was
        mu2, C2, w2 = merged(mp, ba, [b], [a])
    others = [o for o in range(N_SMALL) if o not in (a, b)]
    r1, r2 = rows_of(w1[others + [b]], od), rows_of(w2[others + [a]], od)            # the untouched objects, then the survivor
    eC, em = errors(mu2.ravel()[r2], C2[np.ix_(r2, r2)], mu1.ravel()[r1], C1[np.ix_(r1, r1)])
    print("od %d: a into b against b into a: covariance %.2e  means %.2e" % (od, eC, em))
    assert eC <= 1e-11 and em <= 1e-11


# ---- 4. two calls or one ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("od", [7, 9])
def test_two_pairs_in_two_calls_or_in_one(od):
    rng = np.random.default_rng(40 + od)
    drop, keep = np.array([3, 20], np.uint32), np.array([11, 8], np.uint32)
    offset = 0.1 * rng.normal(size=(2, od))
    A = rng.normal(size=(2, od, od))
    noise = 1e-3 * (A @ A.transpose(0, 2, 1) + od * np.eye(od))
    ba = lender(od)
    with device_map("small", od) as mp:
        one = merged(mp, ba, drop, keep, offset, noise)
        first, w = mp.merge(ba, drop[:1], keep[:1], offset[:1], noise[:1])
    with first:                                                                      # the old map went first
        two = merged(first, ba, w[drop[1:]], w[keep[1:]], offset[1:], noise[1:])
    eC, em = errors(two[0], two[1], one[0], one[1])
    print("od %d: two calls against one: covariance %.2e  means %.2e" % (od, eC, em))
    assert eC <= 1e-11 and em <= 1e-11
    assert np.array_equal(two[2][w], one[2])                                         # the two renumberings compose to the one


# ---- 5. objects the pairs are not correlated with ---------------------------------------------------------------------------------------------------------------
def test_objects_that_are_not_correlated_with_the_pairs_stay_to_the_last_bit():
    od, n = 7, N_SMALL
    rng = np.random.default_rng(55)
    touched = np.sort(rng.permutation(n)[:7])                                        # scattered; the groups 3 + 2 are among them, two more are only correlated with them
    rest = np.array([o for o in range(n) if o not in touched])
    cov = np.zeros((n * od, n * od))
    for sel in (touched, rest):
        rows = rows_of(sel, od)
        R = rng.normal(size=(len(rows), len(rows)))
        cov[np.ix_(rows, rows)] = spd(rng, len(rows), cond=1e3) + 1e-6 * (R - R.T)
    mean = rng.normal(size=(n, od))
    drop, keep = touched[[0, 4, 2]].astype(np.uint32), touched[[3, 3, 1]].astype(np.uint32)
    ba = lender(od)
    with obvi_ba.Map.create(mean, cov, object_block_size=od, library=helpers.PRODUCT_LIB) as mp:
        mu, Cn, where = merged(mp, ba, drop, keep, 0.1 * rng.normal(size=(3, od)))
    rows_old, rows_new = rows_of(rest, od), rows_of(where[rest], od)
    assert np.array_equal(Cn[np.ix_(rows_new, rows_new)], sym(cov)[np.ix_(rows_old, rows_old)]) and np.array_equal(mu[where[rest]], mean[rest])
    moved = [o for o in touched if o not in drop]
    assert all(not np.array_equal(mu[where[o]], mean[o]) for o in moved)             # ... while the pairs' own block did move, the two bystanders in it included
    cross = Cn[np.ix_(rows_new, rows_of(where[moved], od))]
    assert not cross.any()


# ---- 6. the merged map is a map like any other -------------------------------------------------------------------------------------------------------------------
def test_the_merged_map_serves_the_next_window():
    which, od, key = "large", 7, "3x10+2x10"
    drop, keep, offset, noise = cases.merge_case(which, od, key, True)
    mu_ref, C_ref = cases.merge_reference(which, od, key, True)
    n_new = len(mu_ref)                                                              # 40 objects
    ba = lender(od)
    with device_map(which, od) as mp:
        new, where = mp.merge(ba, drop, keep, offset, noise)
    with new:
        mu, Cn = new.get()
        # a group prior is cut from it: a survivor of a group of three, an untouched object, a survivor of a pair
        nxt = list(dict.fromkeys([int(where[keep[0]]), 0, int(where[keep[-1]])]))
        idx = rows_of(nxt, od)
        user = objects_only(np.zeros((4, od)), od)
        user.set_map_group_priors_from_map(new, [[2, 0, 3][:len(nxt)]], [nxt], 2.0)
        _, W, _ = user.debug_linearize(T)
        eW = helpers.rel_err(W[0].T @ W[0], inv_ld(C_ref[np.ix_(idx, idx)]).astype(np.float64))
        # it is conditioned on a window's posterior
        sel = np.array(list(dict.fromkeys([int(where[keep[3]]), n_new - 1, 2, int(where[keep[12]])])))
        widx = rows_of(sel, od)
        m, P = posterior(mu[sel], sym(Cn)[np.ix_(widx, widx)], seed=71)
        with new.condition(ba, sel, m.reshape(-1, od), P) as cond:
            c_mu, c_C = cond.get()
        want = update_formula(mu, Cn, sel, m, P, od)
        e_cond = errors(c_mu, c_C, want[0], want[1])
        # and it grows
        m2, P2 = map_extend_cases.window_posterior(mu[sel].ravel(), sym(Cn)[np.ix_(widx, widx)], 2 * od, seed=72)
        with new.extend(ba, sel, m2.reshape(-1, od), P2, 2) as grown:
            assert grown.n_objects == n_new + 2
            g_mu, g_C = grown.get()
        want = map_extend_cases.extension_formula(mu, Cn, sel, 2, m2.reshape(-1, od), P2, od)
        e_grow = errors(g_mu, g_C, np.asarray(want[0]).reshape(-1, od), want[1])
    print("W^T W of a cut from the merged map against the inverse of the yardstick's sub-block %.2e;  conditioned, against numpy on the merged map: covariance %.2e  "
          "means %.2e;  grown: covariance %.2e  means %.2e" % ((eW,) + e_cond + e_grow))
    assert eW <= 1e-11 and max(e_cond) <= 1e-11 and max(e_grow) <= 1e-11
    assert np.array_equal(c_C, c_C.T) and np.array_equal(g_C, g_C.T)
    user.close()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_and_nothing_behind():
    od = 7
    mean, cov = the_map(od)
    rng = np.random.default_rng(9)
    ba = objects_only(rng.normal(size=(N_MAP, od)), od)
    mp = obvi_ba.Map.create(mean, cov, library=helpers.PRODUCT_LIB)
    ba.set_map_group_priors_from_map(mp, [[5, 1, 9], [2, 0]], [[60, 3, 33], [12, 44]], 1e6)
    r0, W0, _ = ba.debug_linearize(T)
    lib = ba._lib
    lib.obvi_map_merge.restype = C.c_int
    lib.obvi_map_destroy.restype = None
    out = C.c_void_p()
    SENTINEL = 0xABCD1234

    def last_error():
        f = ba._fn("ba_last_error")
        f.restype = C.c_char_p
        return (f(ba._h) or b"").decode()

    def ptr(v, t):
        return None if v is None else np.ascontiguousarray(v, dtype=t).ctypes.data_as(C.c_void_p)

    def call(drop, keep, offset=None, noise=None, q=None, m=mp, o=out, says="map_merge", refused=True):
        out.value = 1
        where = np.full(m.n_objects if m is not None else 4, SENTINEL, np.uint32)
        keep_alive = [ptr(drop, np.uint32), ptr(keep, np.uint32), ptr(offset, np.float64), ptr(noise, np.float64)]
        rc = lib.obvi_map_merge(ba._h, m._m if m is not None else None, C.c_int64(len(drop) if q is None else q), keep_alive[0], keep_alive[1], keep_alive[2], keep_alive[3],
                                where.ctypes.data_as(C.c_void_p), C.byref(o) if o is not None else None)
        if not refused:
            return rc
        assert says in last_error(), (says, last_error())
        assert o is None or not out.value                                                                  # *out is NULL
        assert (where == SENTINEL).all()                                                                   # new_index is untouched
        r, W, _ = ba.debug_linearize(T)
        assert ba._fn("ba_num_factors")(ba._h, C.c_int32(T)) == 2 and all(np.array_equal(a, b) for a, b in zip(W + r, W0 + r0))
        good, where = mp.merge(ba, [4, 9], [2, 2])                                                         # a valid call goes through
        with good:
            assert good.n_objects == N_MAP - 2 and where[4] == where[2] == where[9] == 2 and where[N_MAP - 1] == N_MAP - 3
        return rc

    d1 = np.zeros((1, od))
    R1 = np.eye(od)[None]
    # null pointers and counts
    assert call([4], [2], o=None, says="bad arguments") == -1 and call(None, [2], q=1, says="bad arguments") == -1 and call([4], None, says="bad arguments") == -1
    assert call([4], [2], m=None, says="bad arguments") == -1 and call([4], [2], q=0, says="bad arguments") == -1 and call([4], [2], q=-1, says="bad arguments") == -1
    # the map's side
    with obvi_ba.Map.create(np.zeros((3, 9)), np.eye(27), object_block_size=9, library=helpers.PRODUCT_LIB) as nine:
        assert call([1], [0], m=nine, says="block size") == -1
    if torch.cuda.device_count() > 1:                                   # NOT exercised where the suite sees one GPU: the one refusal of the contract this test cannot reach there
        with obvi_ba.Map.create(mean, cov, device_id=1, library=helpers.PRODUCT_LIB) as far:
            assert call([4], [2], m=far, says="another device") == -1
    # the pairs
    assert call([4], [4], says="into itself") == -1                                                        # drop == keep
    assert call([4, 4], [2, 9], says="twice") == -1                                                        # an object dropped twice
    assert call([4, 2], [2, 9], says="chains") == -1 and call([2, 4], [9, 2], says="chains") == -1         # a chain, in either order
    assert call([N_MAP], [2], says="out of range") == -4 and call([4], [N_MAP], says="out of range") == -4 and call([4, 5], [2, 2 ** 32 - 1], says="out of range") == -4
    near_diagonal = np.eye(300 * od) + 1e-3 * np.diag(np.ones(300 * od - 1), 1)
    with obvi_ba.Map.create(np.zeros((300, od)), near_diagonal, library=helpers.PRODUCT_LIB) as wide:
        assert call(np.arange(293), np.full(293, 299), m=wide, says="OBVI_MAP_GROUP_MAX_ROWS") == -1      # 2051 pair rows: above the cap
        assert call(np.arange(293), np.full(293, 999), m=wide, says="OBVI_MAP_GROUP_MAX_ROWS") == -1      # ... whatever else is wrong with them
        assert call(np.arange(292), np.full(292, 299), m=wide, refused=False) == 0 and out.value          # 2044 rows: at it
        lib.obvi_map_destroy(out)
    # the offsets and the noise
    bad_d, bad_R = d1.copy(), R1.copy()
    bad_d[0, 3], bad_R[0, 2, 5] = np.inf, np.nan
    assert call([4], [2], bad_d, R1, says="offset") == -6 and call([4], [2], d1, bad_R, says="noise") == -6 and call([4], [2], None, bad_R, says="noise") == -6
    huge_R = R1.copy()
    huge_R[0, 1, 5] = huge_R[0, 5, 1] = 1.5e308                                                            # finite, but (R + R^T) / 2 is not: the device reports it
    assert call([4], [2], d1, huge_R, says="not SPD") == -6
    # what the device reports: a pair that is already merged.  Object 6 of this map IS object 2 (a map E Cr E^T, copied entry by entry): T = 0
    src = np.array([0, 1, 2, 3, 4, 5, 2])
    rows = rows_of(src, od)
    Cr = spd(rng, 6 * od)
    with obvi_ba.Map.create(rng.normal(size=(6, od))[src], Cr[np.ix_(rows, rows)], library=helpers.PRODUCT_LIB) as twin:
        assert call([6], [2], m=twin, says="not SPD") == -6
        assert call([6, 0], [2, 4], m=twin, says="not SPD") == -6                                          # ... also beside a pair that is not
        assert call([0], [4], m=twin, refused=False) == 0 and out.value                                    # which alone merges
        lib.obvi_map_destroy(out)
    mp.close()
    assert status_of(lambda: ba.solve(helpers.ba_params(max_it=3))) == 0                                   # the handle is usable
