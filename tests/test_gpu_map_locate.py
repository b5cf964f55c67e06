"""GPU (-m gpu): one device-resident map located in another from the constellations of their object centres (include/obvi_map_locate.h), through the C ABI on a
handle that lends only its device, stream and workspaces.  The reference is the header's definition in long double (tests/map_locate_cases.py; held against a
plain-Python restatement and a Newton yardstick on the CPU by tests/test_map_locate_abi.py) -- never the product.  Decisions are exact: counts, the reported
seeds and their order, inliers, partners -- the cases module asserts that no deciding quantity lies within 1e-9 of its threshold.  Figures -- cost, transform,
transform_cov -- are held to cases.GPU_BAR, three orders over numpy's own fp64 evaluation of the same definition (the rule of tests/test_gpu_map_match.py), and
to bit-equality where the contract promises it (repeatability, the planted ties' order, untouched arrays, maps and handle)."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (loaded before libobvi_ba.so: torch brings its own HIP runtime, and the one that is loaded first is the one that finds the device)

import helpers
import map_frame_cases as frame
import map_locate_cases as cases
import obvi_ba
from test_gpu_map_resident import N_MAP
from map_support import last_error, lender, objects_only, status_of

pytestmark = pytest.mark.gpu

TYPE = obvi_ba.FACTOR_MAP_GROUP_PRIOR
LD = np.longdouble


def device_map(mean, cov, od):
    return obvi_ba.Map.create(mean, cov, object_block_size=od, library=helpers.PRODUCT_LIB)


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Out:
    """The caller's arrays, `room` entries each, filled with marks the entry never writes."""
    def __init__(self, room, nb):
        self.seed, self.T, self.cov = np.full((room, 4), 0xDEAD, np.uint32), np.full((room, 4), -7.5), np.full((room, 4, 4), -7.5)
        self.inl, self.cost, self.partner, self.counts = np.full(room, -77, np.int32), np.full(room, -7.5), np.full((room, nb), -77, np.int32), np.full(3, -77, np.int64)

    def untouched_from(self, k):
        return ((self.seed[k:] == 0xDEAD).all() and (self.T[k:] == -7.5).all() and (self.cov[k:] == -7.5).all() and (self.inl[k:] == -77).all()
                and (self.cost[k:] == -7.5).all() and (self.partner[k:] == -77).all())


def locate(ba, ma, mb, c, p, iterations=3, capacity=None, room=None, **over):
    """(status, Out) of one call through the C ABI.  capacity None: a count-only call first, then one of the exact size."""
    f = ba._lib.obvi_map_locate
    f.restype = C.c_int
    nb = len(c.mean_b)
    params = obvi_ba.LocateParams(p.dmin, p.tol, p.gate, p.min_inliers, iterations)
    la = None if c.label_a is None else np.ascontiguousarray(c.label_a, np.int32)
    lb = None if c.label_b is None else np.ascontiguousarray(c.label_b, np.int32)
    if capacity is None:
        o = Out(0, nb)
        rc = f(ba._h, ma._m, mb._m, ptr(la), ptr(lb), C.byref(params), C.c_int64(0), None, None, None, None, None, None, ptr(o.counts))
        assert rc == 0, last_error(ba)
        capacity = int(o.counts[2])
    o = Out(capacity if room is None else room, nb)
    a = dict(h=ba._h, a=ma._m, b=mb._m, la=ptr(la), lb=ptr(lb), params=C.byref(params), cap=C.c_int64(capacity), seed=ptr(o.seed), T=ptr(o.T), cov=ptr(o.cov),
             inl=ptr(o.inl), cost=ptr(o.cost), partner=ptr(o.partner), counts=ptr(o.counts))
    a.update(over)
    rc = f(a["h"], a["a"], a["b"], a["la"], a["lb"], a["params"], a["cap"], a["seed"], a["T"], a["cov"], a["inl"], a["cost"], a["partner"], a["counts"])
    return rc, o


def held(o, c, p, iterations, capacity, what=""):
    """One call's outputs against the long-double reference: decisions exact, figures within the bar.  Returns the three errors."""
    r, k, T, cov = cases.report(c, p, iterations, capacity=capacity)
    assert tuple(int(v) for v in o.counts) == r.counts, (what, o.counts, r.counts)
    rank = r.order[:k]
    assert np.array_equal(o.seed[:k], r.seeds[rank]) and np.array_equal(o.inl[:k], r.inliers[rank]) and np.array_equal(o.partner[:k], r.partner[rank]), what
    assert o.untouched_from(k), what
    e = cases.errors(o.cost[:k], o.T[:k], o.cov[:k], r.cost[rank], T, cov, cost_scale=p.gate if c.name == "the square" else None)
    print("%s%s, %d iterations: counts %s, %d reported; cost %.2e  transform %.2e  covariance %.2e" % (c.name, what, iterations, r.counts, k, e[0], e[1], e[2]))
    assert max(e) <= cases.GPU_BAR, (what, e)
    assert k == 0 or np.array_equal(o.cov[:k], o.cov[:k].transpose(0, 2, 1))
    return e


# ---- 1. the exhaustive cases -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("od,n_a,labelling", cases.EXHAUSTIVE)
def test_every_hypothesis_of_the_small_maps_against_the_definition(od, n_a, labelling):
    c = cases.case(od, n_a, labelling)
    p = cases.thresholds(c)
    ba = lender(od)
    with device_map(c.mean_a, c.cov_a, od) as ma, device_map(c.mean_b, c.cov_b, od) as mb:
        for iterations in (3, 0):
            rc, o = locate(ba, ma, mb, c, p, iterations)
            assert rc == 0, last_error(ba)
            held(o, c, p, iterations, None)
    ba.close()


# ---- 2. every leading sub-map of B; one object on either side -----------------------------------------------------------------------------------------------
def test_every_leading_sub_map_of_b_and_maps_of_one_object():
    od = 7
    ba = lender(od)
    full = cases.case(od, 24, "classes")
    with device_map(full.mean_a, full.cov_a, od) as ma:
        for n_b in range(1, 11):
            c = cases.case(od, 24, "classes", n_b=n_b)
            p = cases.thresholds(c)
            with device_map(c.mean_b, c.cov_b, od) as mb:
                rc, o = locate(ba, ma, mb, c, p)
                assert rc == 0, last_error(ba)
                held(o, c, p, 3, None)
                assert n_b > 1 or tuple(o.counts) == (0, 0, 0)
        with device_map(*frame.leading(full.mean_a, full.cov_a, 1, od), od) as one, device_map(full.mean_b, full.cov_b, od) as mb:
            p = cases.thresholds(full)
            rc, o = locate(ba, one, mb, full._replace(label_a=full.label_a[:1]), p, capacity=3)
            assert rc == 0 and tuple(o.counts) == (0, 0, 0) and o.untouched_from(0)
    ba.close()


# ---- 3. capacities ---------------------------------------------------------------------------------------------------------------------------------------------
def test_capacities_around_the_number_found_leave_the_rest_of_the_callers_arrays_alone():
    od = 7
    c = cases.case(od, 24, "none")
    p = cases.thresholds(c)
    found = cases.evaluate(c, p).counts[2]
    assert found > 2
    ba = lender(od)
    with device_map(c.mean_a, c.cov_a, od) as ma, device_map(c.mean_b, c.cov_b, od) as mb:
        for capacity in (0, 1, found - 1, found, found + 5):
            rc, o = locate(ba, ma, mb, c, p, capacity=capacity, room=found + 8)
            assert rc == 0, last_error(ba)
            held(o, c, p, 3, capacity, " (capacity %d)" % capacity)
        rc, o = locate(ba, ma, mb, c, p, capacity=found, cov=None, partner=None)     # the two optional arrays left out
        assert rc == 0 and (o.cov == -7.5).all() and (o.partner == -77).all()
        r, k, T, _ = cases.report(c, p, 3)
        assert np.array_equal(o.seed, r.seeds[r.order]) and np.abs(o.T - T).max() <= cases.GPU_BAR * np.abs(T).max()
    ba.close()


# ---- 4. the planted ties -----------------------------------------------------------------------------------------------------------------------------------------
def test_the_tied_square_is_reported_in_seed_index_order():
    c, p = cases.square(), cases.square_thresholds()
    r = cases.evaluate(c, p)
    ties = cases.conditions(c, p, r)
    assert len(ties) == 2 and (r.inliers[r.order] == 4).all() and len(r.order) == 8
    ba = lender(c.od)
    with device_map(c.mean_a, c.cov_a, c.od) as ma, device_map(c.mean_b, c.cov_b, c.od) as mb:
        rc, o = locate(ba, ma, mb, c, p)
        assert rc == 0, last_error(ba)
        held(o, c, p, 3, None)
        place = {int(h): i for i, h in enumerate(r.order)}
        for i, j in ties:
            assert i < j and place[j] == place[i] + 1 and o.cost[place[i]] == o.cost[place[j]]       # equal bits, the lower seed index first
    ba.close()


# ---- 5. seed counts across one wavefront and one workgroup of the scoring launch ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n_compatible", [64, 65, 256, 257])
def test_seed_counts_across_a_wavefront_and_a_workgroup(n_compatible):
    od = 7
    c = cases.case(od, 24, "none")
    p = cases.thresholds(c, n_compatible=n_compatible)
    assert cases.evaluate(c, p).counts[1] == n_compatible
    cases.conditions(c, p)
    ba = lender(od)
    with device_map(c.mean_a, c.cov_a, od) as ma, device_map(c.mean_b, c.cov_b, od) as mb:
        rc, o = locate(ba, ma, mb, c, p)
        assert rc == 0, last_error(ba)
        held(o, c, p, 3, None, " (%d compatible seeds)" % n_compatible)
    ba.close()


# ---- 6. repeatability; the maps and the handle are left as they were ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("od", [7, 9])
def test_the_same_call_twice_and_on_three_handles_gives_the_same_bits_and_leaves_maps_and_handle_alone(od):
    c = cases.case(od, 24, "classes")
    p = cases.thresholds(c)
    user = objects_only(np.random.default_rng(9).normal(size=(N_MAP, od)), od)
    mean, cov = frame.case_map("large", od)
    outs = []
    with device_map(c.mean_a, c.cov_a, od) as ma, device_map(c.mean_b, c.cov_b, od) as mb, device_map(mean, cov, od) as prior:
        user.set_map_group_priors_from_map(prior, [[5, 1, 9], [2, 0]], [[60, 3, 33], [12, 44]], 1e6)
        r0, W0, _ = user.debug_linearize(TYPE)
        err0 = last_error(user)
        for ba in (user, lender(od), lender(od, deterministic=True)):
            for _ in range(2):
                rc, o = locate(ba, ma, mb, c, p)
                assert rc == 0, last_error(ba)
                outs.append(o)
        r, W, _ = user.debug_linearize(TYPE)
        assert last_error(user) == err0 and user._fn("ba_num_factors")(user._h, C.c_int32(TYPE)) == 2 and all(np.array_equal(x, y) for x, y in zip(W + r, W0 + r0))
        for m, (mu, cv) in ((ma, (c.mean_a, c.cov_a)), (mb, (c.mean_b, c.cov_b))):
            got = m.get()
            assert np.array_equal(got[0], mu) and np.array_equal(got[1], cv)
    assert outs[0].counts[2] > 0
    for o in outs[1:]:
        for name in ("seed", "T", "cov", "inl", "cost", "partner", "counts"):
            assert np.array_equal(getattr(o, name), getattr(outs[0], name)), name
    assert status_of(lambda: user.solve(helpers.ba_params(max_it=3))) == 0           # the handle is usable
    user.close()


# ---- 7. refusals beside a live handle --------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_the_handle_and_nothing_behind():
    od = 7
    c = cases.case(od, 24, "classes")
    p = cases.thresholds(c)
    ba = objects_only(np.random.default_rng(9).normal(size=(N_MAP, od)), od)
    mean, cov = frame.case_map("large", od)
    ma, mb, prior = device_map(c.mean_a, c.cov_a, od), device_map(c.mean_b, c.cov_b, od), device_map(mean, cov, od)
    ba.set_map_group_priors_from_map(prior, [[5, 1, 9], [2, 0]], [[60, 3, 33], [12, 44]], 1e6)
    r0, W0, _ = ba.debug_linearize(TYPE)
    found = cases.evaluate(c, p).counts[2]

    def refused(says, status=-1, counts_written=False, map_a=ma, map_b=mb, q=p, iterations=3, cc=c, **over):
        rc, o = locate(ba, map_a, map_b, cc, q, iterations, capacity=found, **over)
        assert rc == status and says in last_error(ba), (says, rc, last_error(ba))
        assert o.untouched_from(0) and (counts_written or (o.counts == -77).all())
        r, W, _ = ba.debug_linearize(TYPE)
        assert ba._fn("ba_num_factors")(ba._h, C.c_int32(TYPE)) == 2 and all(np.array_equal(x, y) for x, y in zip(W + r, W0 + r0))
        rc, good = locate(ba, ma, mb, c, p)                                           # a valid call goes through
        assert rc == 0 and int(good.counts[2]) == found
        return o

    for name in ("a", "b", "params", "counts", "seed", "T", "inl", "cost"):
        refused("bad arguments", **{name: None})
    refused("bad arguments", cap=C.c_int64(-1))
    with obvi_ba.Map.create(np.zeros((3, 9)), np.eye(27), object_block_size=9, library=helpers.PRODUCT_LIB) as nine:
        refused("block size", map_a=nine, cc=c._replace(label_a=None))
        refused("block size", map_b=nine, cc=c._replace(label_b=None))
    if torch.cuda.device_count() > 1:                                   # NOT exercised where the suite sees one GPU
        with obvi_ba.Map.create(c.mean_b, c.cov_b, device_id=1, library=helpers.PRODUCT_LIB) as far:
            refused("another device", map_b=far)
    for bad in (0.0, -1.0, np.nan, np.inf):
        refused("pair_min_distance", q=p._replace(dmin=bad))
    for bad in (-1e-3, np.nan, np.inf):
        refused("pair_tolerance", q=p._replace(tol=bad))
    for bad in (0.0, -2.0, np.nan, np.inf):
        refused("inlier gate", q=p._replace(gate=bad))
    refused("min_inliers", q=p._replace(min_inliers=1))
    refused("refine_iterations", iterations=-1)
    refused("refine_iterations", iterations=9)
    # the object limit, by refusal only: 808 + 12 = 820 objects are one too many, and are refused before anything is launched
    n_wide = obvi_ba_limit() + 1 - len(c.mean_b)
    with obvi_ba.Map.create(np.zeros((n_wide, od)), np.eye(n_wide * od), library=helpers.PRODUCT_LIB) as wide:
        refused("OBVI_MAP_LOCATE_MAX_OBJECTS", map_a=wide, cc=c._replace(label_a=None))
    # more compatible seeds than the seed workspace: 400 objects on a line at equal heights, every pair of pairs within a huge tolerance -- 79 800 x 132 > 2^20
    n_many = 400
    line = np.zeros((n_many, od))
    line[:, 0] = 3.0 * np.arange(n_many)
    with obvi_ba.Map.create(line, 1e-4 * np.eye(n_many * od), library=helpers.PRODUCT_LIB) as many:
        o = refused("OBVI_MAP_LOCATE_MAX_SEEDS", status=-4, counts_written=True, map_a=many, cc=c._replace(label_a=None, label_b=None), q=p._replace(tol=1e6))
        pairs_b = sum(1 for i in range(12) for j in range(12) if i != j and np.hypot(*(c.mean_b[j, :2] - c.mean_b[i, :2])) >= p.dmin)
        assert tuple(o.counts) == (n_many * (n_many - 1) // 2 * 132, n_many * (n_many - 1) // 2 * pairs_b, 0)
    for m in (ma, mb, prior):
        m.close()
    assert status_of(lambda: ba.solve(helpers.ba_params(max_it=3))) == 0             # the handle is usable
    ba.close()


def obvi_ba_limit():
    import re
    txt = open(helpers.ROOT + "/include/obvi_map_locate.h").read()
    return int(re.search(r"#define\s+OBVI_MAP_LOCATE_MAX_OBJECTS\s+(\d+)", txt).group(1))


# ---- 8. the chain: locate, move, join, match, resolve, merge -- no transform supplied by hand --------------------------------------------------------------------
def test_a_map_from_an_unknown_frame_is_located_moved_and_fused():
    c, p, ch, ref = cases.chain()
    od = c.od
    ba = lender(od)
    with device_map(c.mean_a, c.cov_a, od) as a, device_map(c.mean_b, c.cov_b, od) as b:
        loc = a.locate(ba, b, p.dmin, p.tol, p.gate, p.min_inliers, 3, labels=c.label_a, other_labels=c.label_b, capacity=1)
        assert loc.inliers[0] == cases.N_SHARED and list(loc.partner[0]) == list(c.shared) + [-1] * cases.N_EXTRA
        assert np.abs(loc.move[0] - ch.T_est).max() <= cases.GPU_BAR * np.abs(ch.T_est).max()
        with b.transform(ba, loc.move[0], cases.WIDE_SIGMA) as there:
            mu_m, _ = there.get()
            joined = a.join(ba, there)
    with joined:
        ia, ib, s, w, counts = joined.match(ba, ref.gate)
        assert [(int(x), int(y)) for x, y in zip(ia, ib)] == sorted(frame.planted(ch)) and counts[0] == cases.N_SHARED
        drop, keep, sel = obvi_ba.map_match_resolve(od, ia, ib, s, library=helpers.PRODUCT_LIB)
        assert np.array_equal(drop, ref.drop) and np.array_equal(keep, ref.keep)
        fused, where = joined.merge(ba, drop, keep)
    with fused:
        mu, Cn = fused.get()
    e_fused = frame.errors(mu, Cn, ref.fused_mean, ref.fused_cov)
    before, after = frame.extra_distances(ch, mu_m[cases.N_SHARED:]), frame.extra_distances(ch, mu[len(c.mean_a):])
    print("the fused map against the long-double chain: covariance %.2e  means %.2e;  B's own objects from the truth: %s -> %s" % (e_fused + (np.round(before, 4), np.round(after, 4))))
    assert max(e_fused) <= 1e-11
    assert len(mu) == len(c.mean_a) + cases.N_EXTRA and (after < before).all()
    ba.close()
