"""GPU (-m gpu): group priors cut from a device-resident map and factored on the device (include/obvi_map_resident.h) through the C ABI.
The contract is one sentence -- the handle is left as obvi_map_set_group_priors(h, ..., mean[map_idx], cov[map_idx x map_idx], huber) would have left it -- so
every test holds the device path against (a) exact linear algebra in numpy, in the style of test_gpu_map_group_priors.py (whose reference is used: Lambda = C^-1
in long double, first held against its own fp64 form to 1e-12), and (b) the host entry on the same sub-block.  The map: 70 objects, spd(cond = 1e3) plus a small
antisymmetric part, so that the symmetrisation on the device is exercised; selections are scattered and out of order.
Bars (the project's own for factor type 10): linearisation 1e-12, reduced system 1e-11 of the largest entry, LM trajectory 1e-8.  Bit-equality where two runs of
the same arithmetic are compared: the device stages have no sum whose order depends on the schedule.  The cleared-groups test compares reduced systems bit for bit
on a deterministic handle: on a default handle the OTHER factors' fp64 atomics add in another order from run to run."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (loaded before libobvi_ba.so: torch brings its own HIP runtime, and the one that is loaded first is the one that finds the device)

import helpers
import obvi_ba
from helpers import rel_err
from test_gpu_map_pair_priors import base_problem, inv_ld, product, spd
from map_support import det_objects_only, objects_only, records, status_of

pytestmark = pytest.mark.gpu

T = obvi_ba.FACTOR_MAP_GROUP_PRIOR
LD = np.longdouble
N_MAP = 70
GROUPS = ([0, 3, 1], [4, 2])            # session objects of the base problem ...
MAP_GROUPS = ([41, 7, 66], [23, 58])    # ... and the map objects they are: scattered, 41 > 7
HUBER = 2.0


# ---- the map and the numpy reference -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def the_map(od, cond=1e3):
    """70 objects: spd + a small antisymmetric matrix; the means of MAP_GROUPS sit beside the base problem's objects (group 0 far: w < 1).  Computed once, never changed."""
    rng = np.random.default_rng(100 + od)
    n = N_MAP * od
    S = spd(rng, n, cond=cond)
    R = rng.normal(size=(n, n))
    cov = S + 1e-4 * 1e-2 * (R - R.T)
    mean = rng.normal(size=(N_MAP, od))
    prob = base_problem(od)
    mean[MAP_GROUPS[0]] = prob["objects"][GROUPS[0]] - rng.normal(scale=3.0, size=(3, od))
    mean[MAP_GROUPS[1]] = prob["objects"][GROUPS[1]] - rng.normal(scale=0.02, size=(2, od))
    assert np.abs(cov - cov.T).max() > 0
    mean.setflags(write=False); cov.setflags(write=False)
    return mean, cov


def rows_of(sel, od):
    return np.concatenate([np.arange(od * o, od * o + od) for o in sel])


def sub_block(cov, sel, od):
    """cov[map_idx x map_idx] as the caller of the host entry would cut it (not symmetrised), and its symmetrised form."""
    idx = rows_of(sel, od)
    raw = np.ascontiguousarray(cov[np.ix_(idx, idx)])
    return raw, 0.5 * (raw + raw.T)


def device_map(od, cond=1e3):
    mean, cov = the_map(od, cond)
    return obvi_ba.Map.create(mean, cov, object_block_size=od, library=helpers.PRODUCT_LIB)


def selection(rng, k):
    sel = rng.permutation(N_MAP)[:k]
    if (np.diff(sel) > 0).all():
        sel = sel[::-1].copy()
    assert (np.diff(sel) < 0).any() and sorted(sel) != list(range(k))       # out of order, not a prefix of the map
    return sel


def linearised(ba):
    r, W, J1 = ba.debug_linearize(T)
    assert J1 is None
    return r, W


# ---- 1. sizes at the tile edges ------------------------------------------------------------------------------------------------------------
SIZES = [(7, k) for k in (2, 9, 10, 19, 30, 64)] + [(9, k) for k in (2, 7, 8, 30, 64)]      # rows 14 63 70 133 210 448 | 18 63 72 270 576


@pytest.mark.parametrize("od,k", SIZES)
def test_one_group_at_the_tile_edges(od, k):
    mean, cov = the_map(od)
    rng = np.random.default_rng(1000 * od + k)
    sel, obj = selection(rng, k), rng.permutation(k)
    raw, sym = sub_block(cov, sel, od)
    x = np.zeros((k, od))
    x[obj] = mean[sel] + rng.normal(scale=0.05, size=(k, od))
    N = k * od
    with device_map(od) as mp:
        assert mp.n_objects == N_MAP
        ba = objects_only(x, od)
        ba.set_map_group_priors_from_map(mp, [list(obj)], [list(sel)], 1e6)
    assert ba.num_factors(T) == 1 and ba._fn("ba_num_factors")(ba._h, C.c_int32(T)) == 1 and ba._fn("ba_num_residuals")(ba._h) == N
    r, W = linearised(ba)
    assert W[0].shape == (N, N) and len(r[0]) == N
    assert not np.triu(W[0], 1).any() and (np.diag(W[0]) > 0).all()
    # the long-double reference, held against its own fp64 form first
    L = inv_ld(sym)
    L64 = np.linalg.inv(sym)
    d = (x[obj] - mean[sel]).ravel()
    Ld, s = L @ d.astype(LD), float(d.astype(LD) @ L @ d.astype(LD))
    assert np.abs(L64 - L).max() <= 1e-12 * np.abs(L).max() and np.abs(L64 @ d - Ld).max() <= 1e-12 * np.abs(Ld).max() and abs(d @ L64 @ d - s) <= 1e-12 * s
    errs = (rel_err(W[0].T @ W[0], L.astype(np.float64)), rel_err(W[0].T @ r[0], Ld.astype(np.float64)), abs(r[0] @ r[0] - s) / s)
    # the host entry on the same sub-block: the Cholesky factor is unique
    host = objects_only(x, od)
    host.set_map_group_priors([list(obj)], [mean[sel]], [raw], 1e6)
    rh, Wh = linearised(host)
    ew = np.abs(W[0] - Wh[0]).max() / np.abs(Wh[0]).max()
    print("od %d, %d rows: J^T J %.2e  J^T r %.2e  |r|^2 %.2e  W against the host's %.2e" % ((od, N) + errs + (ew,)))
    assert max(errs) < 1e-12, errs
    assert ew < 1e-12
    assert rel_err(r[0], rh[0]) < 1e-12


# ---- 2. several groups in one call -----------------------------------------------------------------------------------------------------------
def test_groups_of_one_call_do_not_meet():
    od, ks = 7, (2, 10, 30)                                                    # 14, 70 and 210 rows
    mean, cov = the_map(od)
    rng = np.random.default_rng(77)
    sel = selection(rng, sum(ks))
    obj = rng.permutation(sum(ks))
    cuts = np.cumsum((0,) + ks)
    groups = [list(obj[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    maps = [list(sel[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    x = rng.normal(size=(sum(ks), od))
    with device_map(od) as mp:
        ba = objects_only(x, od)
        ba.set_map_group_priors_from_map(mp, groups, maps, 1e6)
        r, W = linearised(ba)
        assert [w.shape[0] for w in W] == [od * k for k in ks]
        for g in range(3):
            ba.set_map_group_priors_from_map(mp, [groups[g]], [maps[g]], 1e6)
            r1, W1 = linearised(ba)
            assert np.array_equal(W1[0], W[g]) and rel_err(r1[0], r[g]) < 1e-14, g
            Lam = inv_ld(sub_block(cov, maps[g], od)[1]).astype(np.float64)
            assert rel_err(W[g].T @ W[g], Lam) < 1e-12, g


# ---- 3. the base problem -------------------------------------------------------------------------------------------------------------------------
def host_handle(prob, od, **opts):
    mean, cov = the_map(od)
    ba = product(prob, **opts)
    ba.set_map_group_priors([list(g) for g in GROUPS], [mean[list(m)] for m in MAP_GROUPS], [sub_block(cov, m, od)[0] for m in MAP_GROUPS], HUBER)
    return ba


def map_handle(prob, mp, **opts):
    ba = product(prob, **opts)
    ba.set_map_group_priors_from_map(mp, [list(g) for g in GROUPS], [list(m) for m in MAP_GROUPS], HUBER)
    return ba


def same_systems_and_trajectory(a, b, tag):
    Sa, ba_ = a.debug_reduced_system(1e300); Sb, bb = b.debug_reduced_system(1e300)
    eS, eb = np.abs(Sa - Sb).max() / np.abs(Sb).max(), np.abs(ba_ - bb).max() / np.abs(bb).max()
    print("%s: lhs %.2e  rhs %.2e" % (tag, eS, eb))
    assert eS < 1e-11 and eb < 1e-11
    for loss in (True, False):
        ca, ra, qa = a.evaluate(loss); cb, rb, qb = b.evaluate(loss)
        print("%s: loss %d: cost %.2e  residuals %.2e  norms %.2e" % (tag, loss, abs(ca - cb) / cb, rel_err(ra, rb), rel_err(qa, qb)))
        assert abs(ca - cb) <= 1e-12 * cb and len(ra) == len(rb) and rel_err(ra, rb) < 1e-12 and rel_err(qa, qb) < 1e-12
    prm = helpers.ba_params(max_it=10)
    sa, sb = a.solve(prm), b.solve(prm)
    ia, ib = records(a), records(b)
    assert sa.num_iterations == sb.num_iterations > 3 and sa.num_residuals_reduced == sb.num_residuals_reduced
    assert [x[:2] for x in ia] == [x[:2] for x in ib]
    worst = max(abs(x[2] - y[2]) / y[2] for x, y in zip(ia, ib))
    print("%s: %d iterations, costs %.2e" % (tag, sa.num_iterations, worst))
    assert worst <= 1e-8


@pytest.mark.parametrize("variant", ["default", "deterministic", "nine"])
def test_base_problem_equals_the_host_entry(variant):
    od = 9 if variant == "nine" else 7
    opts = dict(deterministic=True) if variant == "deterministic" else {}
    prob = base_problem(od)
    with device_map(od) as mp:
        a = map_handle(prob, mp, **opts)
    b = host_handle(prob, od, **opts)
    assert a.num_factors(T) == 2 and a._fn("ba_num_factors")(a._h, C.c_int32(T)) == 2
    same_systems_and_trajectory(a, b, variant)


# ---- 4. repeatability ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deterministic", [False, True])
def test_the_same_call_twice_and_a_smaller_call_after_it(deterministic):
    od = 7
    mean, cov = the_map(od)
    rng = np.random.default_rng(5)
    sel, obj = selection(rng, 30), rng.permutation(30)
    x = rng.normal(size=(30, od))

    with device_map(od) as mp:
        ba = objects_only(x, od) if not deterministic else det_objects_only(x, od)
        ba.set_map_group_priors_from_map(mp, [list(obj)], [list(sel)], 1e6)
        r1, W1 = linearised(ba)
        S1 = ba.debug_reduced_system(1e300)
        ba.set_map_group_priors_from_map(mp, [list(obj)], [list(sel)], 1e6)
        r2, W2 = linearised(ba)
        S2 = ba.debug_reduced_system(1e300)
        assert np.array_equal(W1[0], W2[0]) and np.array_equal(r1[0], r2[0])
        assert np.array_equal(S1[0], S2[0]) and np.array_equal(S1[1], S2[1])          # Lambda too: an objects-only problem's reduced system is the scatter alone
        # a smaller selection leaves nothing of the first
        small = [[list(obj[3:8]), list(obj[20:22])], [list(sel[3:8]), list(sel[20:22])]]
        ba.set_map_group_priors_from_map(mp, small[0], small[1], 1e6)
        fresh = objects_only(x, od) if not deterministic else det_objects_only(x, od)
        fresh.set_map_group_priors_from_map(mp, small[0], small[1], 1e6)
    assert ba.num_factors(T) == 2 and ba._fn("ba_num_residuals")(ba._h) == 7 * od
    ra, Wa = linearised(ba); rf, Wf = linearised(fresh)
    for g in range(2):
        assert np.array_equal(Wa[g], Wf[g]) and np.array_equal(ra[g], rf[g])
    Sa, Sf = ba.debug_reduced_system(1e300), fresh.debug_reduced_system(1e300)
    assert np.array_equal(Sa[0], Sf[0]) and np.array_equal(Sa[1], Sf[1])


def test_cleared_groups_leave_no_trace():
    prob = base_problem()
    plain = product(prob, deterministic=True)
    S0, b0 = plain.debug_reduced_system(1e300)
    with device_map(7) as mp:
        ba = map_handle(prob, mp, deterministic=True)
        ba.prepare()
        ba.set_map_group_priors_from_map(mp, [], [], 1.0)
    assert ba.num_factors(T) == 0 and ba._fn("ba_num_factors")(ba._h, C.c_int32(T)) == 0
    assert ba._fn("ba_num_residuals")(ba._h) == plain._fn("ba_num_residuals")(plain._h)
    S1, b1 = ba.debug_reduced_system(1e300)
    assert np.array_equal(S0, S1) and np.array_equal(b0, b1)
    ba.reset()                                                                   # reset clears the groups as well
    with device_map(7) as mp:
        ba2 = map_handle(prob, mp)
        ba2.reset()
        assert ba2._fn("ba_num_factors")(ba2._h, C.c_int32(T)) == 0 and ba2.num_factors(T) == 0
        assert mp.n_objects == N_MAP                                             # ... and does not touch the map


# ---- 5. one map, two handles; the map destroyed before the solve -------------------------------------------------------------------------------------------
def test_one_map_serves_two_handles_and_may_go_before_the_solve():
    prob = base_problem()
    mp = device_map(7)
    a1, a2 = map_handle(prob, mp), map_handle(prob, mp, deterministic=True)
    mp.close()
    assert mp.n_objects == -1
    same_systems_and_trajectory(a1, host_handle(prob, 7), "first handle")
    same_systems_and_trajectory(a2, host_handle(prob, 7, deterministic=True), "second handle")


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_groups_as_they_were():
    od = 7
    mean, cov = the_map(od)
    rng = np.random.default_rng(9)
    x = rng.normal(size=(N_MAP, od))
    ba = objects_only(x, od)
    mp = device_map(od)
    ba.set_map_group_priors_from_map(mp, [[5, 1, 9], [2, 0]], [[60, 3, 33], [12, 44]], 1e6)
    r0, W0 = linearised(ba)
    f = ba._lib.obvi_map_set_group_priors_from_map
    f.restype = C.c_int

    def unchanged():
        r, W = linearised(ba)
        return ba._fn("ba_num_factors")(ba._h, C.c_int32(T)) == 2 and all(np.array_equal(a, b) for a, b in zip(W + r, W0 + r0))

    def raw(ptr, idx, mid, m=mp, n=None, refused=True):
        a = [None if v is None else np.ascontiguousarray(v, dtype=t) for v, t in ((ptr, np.int64), (idx, np.uint32), (mid, np.uint32))]
        p = [None if v is None else v.ctypes.data_as(C.c_void_p) for v in a]
        rc = f(ba._h, m._m if m is not None else None, C.c_int64(len(ptr) - 1 if n is None else n), p[0], p[1], p[2], C.c_double(1.0))
        assert not refused or unchanged(), (ptr, idx, mid)
        return rc
    ok = ([0, 2], [0, 1], [4, 2])
    assert raw(None, ok[1], ok[2], n=1) == -1 and raw(ok[0], None, ok[2]) == -1 and raw(ok[0], ok[1], None) == -1      # every required pointer null in turn
    assert raw(*ok, n=-1) == -1
    assert raw(*ok, m=None) == -1                                                        # a null map
    assert raw([1, 2], [0, 1], [4, 2]) == -1                                             # group_ptr does not start at 0
    assert raw([0, 2, 1], [0, 1], [4, 2]) == -1                                          # ... decreases
    assert raw([0, 1, 1], [0], [4]) == -1                                                # an empty group
    assert raw([0, 293], np.arange(293), np.zeros(293)) == -1                            # 2051 rows: above the cap, before anything else is read
    assert raw([0, 2], [0, N_MAP], [4, 2]) == -4                                         # a session object >= O
    assert raw([0, 3], [0, 1, 0], [4, 2, 6]) == -1 and raw([0, 2, 4], [0, 1, 2, 1], [4, 2, 6, 8]) == -1               # an object twice: in one group, in two
    assert raw([0, 2], [0, 1], [4, N_MAP]) == -4                                         # a map object >= the map's count
    assert raw([0, 3], [0, 1, 2], [4, 2, 4]) == -1 and raw([0, 2, 4], [0, 1, 2, 3], [4, 2, 6, 2]) == -1               # a map object twice
    with obvi_ba.Map.create(np.zeros((3, 9)), np.eye(27), object_block_size=9, library=helpers.PRODUCT_LIB) as nine:
        assert raw(*ok, m=nine) == -1                                                    # the map's block size is not the handle's
    if torch.cuda.device_count() > 1:
        with obvi_ba.Map.create(mean, cov, device_id=1, library=helpers.PRODUCT_LIB) as far:
            assert raw(*ok, m=far) == -1                                                 # a map on another device
    # numerical refusals, decided from what the device reports.  Indefinite: one member's diagonal block less twice the map's largest eigenvalue (spd: scale x cond = 10)
    bad = np.array(cov)
    blk = slice(od * 33, od * 33 + od)
    bad[blk, blk] -= 2.0 * 10.0 * np.eye(od)
    everything = rng.permutation(N_MAP)
    with obvi_ba.Map.create(mean, bad, library=helpers.PRODUCT_LIB) as m_bad:
        assert raw([0, 3], [0, 1, 2], [60, 33, 3], m=m_bad) == -6
        assert raw([0, 2, 5], [0, 1, 2, 3, 4], [12, 44, 60, 33, 3], m=m_bad) == -6       # ... in the second group of two
        assert raw([0, 2], [0, 1], [12, 44], m=m_bad, refused=False) == 0                             # a sub-block that leaves the member out is as good as before
        ba.set_map_group_priors_from_map(mp, [[5, 1, 9], [2, 0]], [[60, 3, 33], [12, 44]], 1e6)
        assert unchanged()
    with device_map(od, cond=1e15) as m_ill:
        assert raw([0, N_MAP], np.arange(N_MAP), everything, m=m_ill) == -6              # the whole map as one group: condition number 1e15
    with device_map(od, cond=1e9) as m_fair:
        assert status_of(lambda: ba.set_map_group_priors_from_map(m_fair, [list(range(N_MAP))], [list(everything)], 1e6)) == 0
    assert ba._fn("ba_num_factors")(ba._h, C.c_int32(T)) == 1
    mp.close()
    s = ba.solve(helpers.ba_params(max_it=3))                                            # the handle is usable
    assert s.reduced_system_size == N_MAP * od
