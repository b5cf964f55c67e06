"""GPU (-m gpu): a device-resident map read back and conditioned on a window's posterior (include/obvi_map_update.h) through the C ABI.
The yardstick is conditioning in information form in long double (tests/map_update_cases.py; held against the update formula on the CPU by
tests/test_map_update_abi.py) -- never the product.  Bars: 1e-11 of the largest entry of the yardstick for covariances and means (the project's bar for reduced
systems; numpy's fp64 evaluation of the update formula on these inputs is within 2e-13, so the bar is 50 x above fp64 round-off, and anything structural -- a
wrong tile, a padded row leaking in -- is 1e-2 and above); 1e-12 where the handle form is compared with the host-pointer form fed the same posterior; 1e-8 for an
LM trajectory; bit-equality where the contract promises it (symmetry, the window's own block and means, repeatability, the untouched old map and handle).

Measured on the MI355X: covariances within 1.3e-14 and means within 5.7e-16 of the yardstick at the tile edges, two windows in a row 4.8e-15,
the handle form 1.5e-15 from the host-pointer form on default handles and equal to the last bit on deterministic ones, the next window's W^T W 3.4e-15."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (loaded before libobvi_ba.so: torch brings its own HIP runtime, and the one that is loaded first is the one that finds the device)

import helpers
import map_update_cases as cases
import obvi_ba
import synth
from map_update_cases import rows_of, sym
from test_gpu_map_pair_priors import base_problem, inv_ld, product
from test_gpu_map_resident import N_MAP, the_map
from map_support import errors, lender, objects_only, records, status_of

pytestmark = pytest.mark.gpu

T = obvi_ba.FACTOR_MAP_GROUP_PRIOR
LD = np.longdouble
WINDOW_OBJ = [0, 3, 1, 4, 2]                # the base problem's five objects as one group ...
WINDOW_MAP = [41, 7, 66, 23, 58]            # ... and the map objects they are (the_map puts their means beside the objects)


def device_map(which, od):
    mean, cov = cases.map_of(which, od)
    return obvi_ba.Map.create(mean, cov, object_block_size=od, library=helpers.PRODUCT_LIB)


# ---- 1. round trip ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("od", [7, 9])
def test_get_returns_what_create_was_given(od):
    mean, cov = cases.small_map(od)
    with device_map("small", od) as mp:
        m, c = mp.get()
    assert np.array_equal(m, mean) and np.array_equal(c, cov)


# ---- 2. tile edges, host-pointer form ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,od,k", cases.EDGE_CASES)
def test_the_update_at_the_tile_edges(which, od, k):
    mean, cov = cases.map_of(which, od)
    sel, m, P = cases.edge_case(which, od, k)
    mu_ref, C_ref = cases.edge_reference(which, od, k)
    idx = rows_of(sel, od)
    ba = lender(od)
    with device_map(which, od) as mp:
        with mp.condition(ba, sel, m, P) as new:
            assert new.n_objects == len(mean)
            mu, Cn = new.get()
        old = mp.get()
    eC, em = errors(mu, Cn, mu_ref, C_ref)
    print("%s map, od %d, k %d (%d of %d rows): covariance %.2e  means %.2e" % (which, od, k, len(idx), od * len(mean), eC, em))
    assert eC <= 1e-11 and em <= 1e-11
    assert np.array_equal(Cn, Cn.T)
    assert np.array_equal(Cn[np.ix_(idx, idx)], 0.5 * (P + P.T)) and np.array_equal(mu[sel], m)
    Cs = sym(np.asarray(cov))
    scale = np.abs(C_ref).max()
    assert np.linalg.eigvalsh(Cn).min() > 0
    assert np.linalg.eigvalsh(Cs - Cn).min() >= -1e-11 * scale                       # information was added, nowhere removed
    assert np.array_equal(old[0], mean) and np.array_equal(old[1], cov)              # the old map is as it was


# ---- 3. no information -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("od,k", [(7, 10), (9, 24)])
def test_a_posterior_that_is_the_prior_changes_nothing(od, k):
    mean, cov = cases.small_map(od)
    Cs = sym(np.asarray(cov))
    sel = cases.selection(np.random.default_rng(31 + k), cases.N_SMALL, k)
    idx = rows_of(sel, od)
    with device_map("small", od) as mp, mp.condition(lender(od), sel, mean[sel], Cs[np.ix_(idx, idx)]) as new:
        mu, Cn = new.get()
    eC, em = errors(mu, Cn, mean, Cs)
    print("od %d, k %d: covariance %.2e  means %.2e" % (od, k, eC, em))
    assert eC <= 1e-11 and em <= 1e-11


# ---- 4. repeatability --------------------------------------------------------------------------------------------------------------------------
def test_the_same_call_twice_and_on_either_kind_of_handle_gives_the_same_bits():
    which, od, k = "large", 7, 30
    sel, m, P = cases.edge_case(which, od, k)
    out = []
    with device_map(which, od) as mp:
        for ba in (lender(od), lender(od, deterministic=True)):
            for _ in range(2):
                with mp.condition(ba, sel, m, P) as new:
                    out.append(new.get())
    for mu, Cn in out[1:]:
        assert np.array_equal(mu, out[0][0]) and np.array_equal(Cn, out[0][1])


# ---- 5. two windows in a row ---------------------------------------------------------------------------------------------------------------------
def test_two_windows_in_a_row():
    which, od = "small", 7
    mean, cov = cases.small_map(od)
    sel1 = np.array([17, 3, 9, 21, 0, 12, 5, 14, 8, 2, 19])                          # 77 rows
    sel2 = np.array([9, 23, 3, 1, 12, 20, 6, 17, 11, 4, 15, 7, 22])                  # 91 rows; 9 3 12 17 in both
    idx1, idx2 = rows_of(sel1, od), rows_of(sel2, od)
    Cs = sym(np.asarray(cov))
    m1, P1 = cases.posterior(mean[sel1], Cs[np.ix_(idx1, idx1)], seed=51)
    # the second window's prior is the marginal of the map after the first -- the yardstick's, not the product's
    mu1, C1 = cases.yardstick(which, od, [(sel1, m1, P1, None)])
    prior2 = (C1[np.ix_(idx2, idx2)], mu1[idx2])
    m2, P2 = cases.posterior(prior2[1], prior2[0], seed=52)
    mu_ref, C_ref = cases.yardstick(which, od, [(sel1, m1, P1, None), (sel2, m2, P2, prior2)])
    n1 = cases.update_formula(mean, cov, sel1, m1, P1, od)
    n2 = cases.update_formula(n1[0], n1[1], sel2, m2, P2, od)
    ba = lender(od)
    with device_map(which, od) as mp:
        first = mp.condition(ba, sel1, m1.reshape(-1, od), P1)
    with first, first.condition(ba, sel2, m2.reshape(-1, od), P2) as second:      # the old map went first
        mu, Cn = second.get()
    e_np = errors(mu, Cn, n2[0], n2[1])
    e_ld = errors(mu, Cn, mu_ref.reshape(-1, od), C_ref)
    print("against numpy's two updates: covariance %.2e  means %.2e;  against the information form with both windows added: covariance %.2e  means %.2e" % (e_np + e_ld))
    assert max(e_np) <= 1e-11 and max(e_ld) <= 1e-11


# ---- 6. the handle form ----------------------------------------------------------------------------------------------------------------------------
def window_handle(od, mp, deterministic):
    ba = product(base_problem(od), **(dict(deterministic=True) if deterministic else {}))
    ba.set_map_group_priors_from_map(mp, [WINDOW_OBJ], [WINDOW_MAP], 1e6)
    s = ba.solve(helpers.ba_params(max_it=50))
    assert s.num_iterations > 3
    return ba


def solve_and_condition(od, deterministic):
    """The window solved, the map conditioned on the handle.  Only the new map stays on the device (the fixture below closes it)."""
    with device_map("large", od) as mp:
        ba = window_handle(od, mp, deterministic)
        before = ba.get_state()
        new = mp.condition_on(ba, WINDOW_OBJ, WINDOW_MAP)
        after = ba.get_state()
        m = ba.get_objects()[WINDOW_OBJ]
        blocks = ba.object_covariances(np.repeat(WINDOW_OBJ, 5), np.tile(WINDOW_OBJ, 5))
        P = blocks.reshape(5, 5, od, od).transpose(0, 2, 1, 3).reshape(5 * od, 5 * od)
        with mp.condition(ba, WINDOW_MAP, m, P) as fed:
            fed_arrays = fed.get()
        ba.close()
    return dict(new=new, before=before, after=after, m=m, P=P, on=new.get(), fed=fed_arrays)


@pytest.fixture(scope="module")
def handle_form():
    """handle_form(od, deterministic): what tests 6 and 7 look at, computed once per variant; the new maps are destroyed when the module is done."""
    made = {}

    def get(od, deterministic):
        if (od, deterministic) not in made:
            made[od, deterministic] = solve_and_condition(od, deterministic)
        return made[od, deterministic]
    yield get
    for r in made.values():
        r["new"].close()


@pytest.mark.parametrize("od", [7, 9])
@pytest.mark.parametrize("deterministic", [False, True])
def test_the_handle_form(handle_form, od, deterministic):
    r = handle_form(od, deterministic)
    assert all(np.array_equal(a, b) for a, b in zip(r["before"], r["after"]))      # the estimate is where it was
    e_fed = errors(r["on"][0], r["on"][1], r["fed"][0], r["fed"][1])
    mu_ref, C_ref = cases.yardstick("large", od, [(np.array(WINDOW_MAP), r["m"], r["P"], None)])
    e_ld = errors(r["on"][0], r["on"][1], mu_ref.reshape(-1, od), C_ref)
    print("od %d, deterministic %d: against the host-pointer form fed from the handle: covariance %.2e  means %.2e;  against the yardstick: covariance %.2e  means %.2e"
          % ((od, deterministic) + e_fed + e_ld))
    assert max(e_fed) <= 1e-12 and max(e_ld) <= 1e-11
    idx = rows_of(WINDOW_MAP, od)
    assert np.array_equal(r["on"][1], r["on"][1].T) and np.array_equal(r["on"][0][WINDOW_MAP], r["m"])
    if deterministic:
        # a solve that follows runs as it does after obvi_ba_object_covariances: the call has that call's side effects and no others
        with device_map("large", od) as mp:
            twin = window_handle(od, mp, True)
            twin.object_covariances(WINDOW_OBJ)
            mine = window_handle(od, mp, True)
            mp.condition_on(mine, WINDOW_OBJ, WINDOW_MAP).close()
        prm = helpers.ba_params(max_it=5)
        twin.solve(prm); mine.solve(prm)
        assert records(twin) == records(mine) and len(records(mine)) >= 1
        twin.close(); mine.close()
    assert idx.size == 5 * od


# ---- 7. the loop closes ------------------------------------------------------------------------------------------------------------------------------
def test_the_next_window_cuts_its_prior_from_the_new_map(handle_form):
    od = 7
    r = handle_form(od, False)
    mean, cov = the_map(od)
    n_mu, n_C = cases.update_formula(mean, cov, WINDOW_MAP, r["m"], r["P"], od)      # numpy's update, fp64
    nxt_map = [41, 12, 66, 30, 58]                                                   # 41 66 58 were in the window; 12 and 30 never were
    idx = rows_of(nxt_map, od)
    sub = n_C[np.ix_(idx, idx)]
    prob = base_problem(od)
    a = product(prob)
    a.set_map_group_priors_from_map(r["new"], [WINDOW_OBJ], [nxt_map], 2.0)          # the cut succeeds
    _, W, _ = a.debug_linearize(T)
    eW = helpers.rel_err(W[0].T @ W[0], inv_ld(sub).astype(np.float64))
    b = product(prob)
    b.set_map_group_priors([WINDOW_OBJ], [n_mu[nxt_map]], [sub], 2.0)
    prm = helpers.ba_params(max_it=10)
    sa, sb = a.solve(prm), b.solve(prm)
    ia, ib = records(a), records(b)
    assert sa.num_iterations == sb.num_iterations > 3 and [x[:2] for x in ia] == [x[:2] for x in ib]
    worst = max(abs(x[2] - y[2]) / y[2] for x, y in zip(ia, ib))
    print("W^T W against the inverse of numpy's updated sub-block %.2e;  %d iterations, costs %.2e" % (eW, sa.num_iterations, worst))
    assert eW <= 1e-11 and worst <= 1e-8
    # a never-seen object that correlates with the window knows more than before
    Cs, Cn = sym(np.asarray(cov)), r["on"][1]
    for o in (12, 30):
        blk = slice(od * o, od * o + od)
        assert np.trace(Cn[blk, blk]) < np.trace(Cs[blk, blk])


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_and_nothing_behind():
    od = 7
    mean, cov = the_map(od)
    rng = np.random.default_rng(9)
    x = rng.normal(size=(N_MAP, od))
    ba = objects_only(x, od)
    mp = obvi_ba.Map.create(mean, cov, library=helpers.PRODUCT_LIB)
    ba.set_map_group_priors_from_map(mp, [[5, 1, 9], [2, 0]], [[60, 3, 33], [12, 44]], 1e6)
    r0, W0, _ = ba.debug_linearize(T)
    lib = ba._lib
    lib.obvi_map_condition.restype = lib.obvi_map_condition_on_handle.restype = C.c_int
    lib.obvi_map_destroy.restype = None
    out = C.c_void_p()
    ok_idx = np.array([4, 2], np.uint32)
    ok_m, ok_P = mean[[4, 2]], 0.5 * sym(np.asarray(cov))[np.ix_(rows_of([4, 2], od), rows_of([4, 2], od))]

    def last_error(h):
        f = h._fn("ba_last_error")
        f.restype = C.c_char_p
        return (f(h._h) or b"").decode()

    def ptr(v, t):
        return None if v is None else np.ascontiguousarray(v, dtype=t).ctypes.data_as(C.c_void_p)

    def after_a_refusal(null_out=True):
        assert not null_out or not out.value                                                               # *out is NULL
        r, W, _ = ba.debug_linearize(T)
        assert ba._fn("ba_num_factors")(ba._h, C.c_int32(T)) == 2 and all(np.array_equal(a, b) for a, b in zip(W + r, W0 + r0))
        with mp.condition(ba, ok_idx, ok_m, ok_P) as good:                                                  # a valid call goes through
            assert good.n_objects == N_MAP

    def host(idx, m_, P_, k=None, m=mp, o=out, refused=True):
        out.value = 1
        keep = [ptr(idx, np.uint32), ptr(m_, np.float64), ptr(P_, np.float64)]
        rc = lib.obvi_map_condition(ba._h, m._m if m is not None else None, C.c_int64(len(idx) if k is None else k), keep[0], keep[1], keep[2], C.byref(o) if o is not None else None)
        if refused:
            after_a_refusal(o is not None)
        return rc

    def on(obj, idx, k=None, m=mp, o=out, says=""):
        out.value = 1
        keep = [ptr(obj, np.uint32), ptr(idx, np.uint32)]
        rc = lib.obvi_map_condition_on_handle(ba._h, m._m if m is not None else None, C.c_int64(len(idx) if k is None else k), keep[0], keep[1], C.byref(o) if o is not None else None)
        assert says in last_error(ba)
        after_a_refusal(o is not None)
        return rc
    # null pointers, k < 1
    assert host(ok_idx, ok_m, ok_P, m=None) == -1 and host(ok_idx, ok_m, ok_P, o=None) == -1
    assert host(None, ok_m, ok_P, k=2) == -1 and host(ok_idx, None, ok_P) == -1 and host(ok_idx, ok_m, None) == -1
    assert host(ok_idx, ok_m, ok_P, k=0) == -1 and host(ok_idx, ok_m, ok_P, k=-1) == -1
    assert on([0, 1], ok_idx, m=None) == -1 and on([0, 1], ok_idx, o=None) == -1 and on(None, ok_idx) == -1 and on([0, 1], None, k=2) == -1 and on([0, 1], ok_idx, k=0) == -1
    # the map's side
    with obvi_ba.Map.create(np.zeros((3, 9)), np.eye(27), object_block_size=9, library=helpers.PRODUCT_LIB) as nine:
        assert host([1, 0], np.zeros((2, 9)), np.eye(18), m=nine) == -1 and on([0, 1], [1, 0], m=nine) == -1          # another block size than the handle's
    if torch.cuda.device_count() > 1:                                   # NOT exercised where the suite sees one GPU: the one refusal of the contract this test cannot reach there
        with obvi_ba.Map.create(mean, cov, device_id=1, library=helpers.PRODUCT_LIB) as far:
            assert host(ok_idx, ok_m, ok_P, m=far) == -1 and on([0, 1], ok_idx, m=far) == -1                          # another device
    assert host([4, 4], ok_m, ok_P) == -1 and on([0, 1], [4, 4]) == -1                                               # a map object twice
    assert host([4, N_MAP], ok_m, ok_P) == -4 and on([0, 1], [4, N_MAP]) == -4                                       # a map object >= n
    near_diagonal = np.eye(300 * od) + 1e-3 * np.diag(np.ones(300 * od - 1), 1)
    with obvi_ba.Map.create(np.zeros((300, od)), near_diagonal, library=helpers.PRODUCT_LIB) as wide:
        big = np.arange(293)                                                                                       # 2051 rows: above the cap
        assert host(big, np.zeros((293, od)), np.eye(293 * od), m=wide) == -1
        assert host(np.arange(292), np.zeros((292, od)), 0.5 * np.eye(292 * od), m=wide, refused=False) == 0 and out.value   # 2044 rows: at it
        lib.obvi_map_destroy(out)
    # the posterior's side
    bad_m, bad_P = ok_m.copy(), ok_P.copy()
    bad_m[1, 3], bad_P[2, 9] = np.inf, np.nan
    assert host(ok_idx, bad_m, ok_P) == -6 and host(ok_idx, ok_m, bad_P) == -6
    # the handle form's own
    assert on([0, 0], ok_idx) == -1                                                                                # a session object twice
    assert on([0, N_MAP], ok_idx) == -4                                                                            # a session object >= O
    flags = np.zeros(N_MAP, np.uint8); flags[7] = 1
    ba.set_const_flags(object_const=flags)
    assert on([0, 7], ok_idx) == -1                                                                                # a constant session object
    ba.set_const_flags(object_const=np.zeros(N_MAP, np.uint8))
    assert on([0, 3], ok_idx, says="no active factor") == -1                                                      # object 3 is in no group: no variable, no covariance
    # a handle that exchanges shared objects: refused from the flags and the hook, before it has planned and after, and no collective is entered
    calls = []
    ex = product(base_problem(od))
    ex.set_shared_objects(np.array([0, 0, 1, 0, 0], np.uint8), 0, 1)
    ex.set_allreduce(lambda buf, count, op, stream: calls.append(count) or 0)
    for planned in (False, True):
        if planned:
            ex.prepare()
        entered = len(calls)
        g0 = ex.debug_linearize(T)
        out.value = 1
        keep = [ptr([0, 1], np.uint32), ptr(ok_idx, np.uint32)]
        assert lib.obvi_map_condition_on_handle(ex._h, mp._m, C.c_int64(2), keep[0], keep[1], C.byref(out)) == -1 and not out.value
        assert "exchanges shared objects" in last_error(ex) and len(calls) == entered
        assert ex.debug_linearize(T) == g0 == ([], [], None)
        with mp.condition(ex, ok_idx, ok_m, ok_P) as good:                                                          # the host-pointer form only borrows the stream
            assert good.n_objects == N_MAP
        after_a_refusal(True)
    assert calls == []                                                                                             # the hook was never called
    ex.close()
    # reprojection and bounding-box factors but no cameras: OBVI_ERR_NOT_READY, as obvi_ba_object_covariances answers
    blind = product(base_problem(od))
    blind.set_cameras(np.zeros((0, 4)), np.zeros((0, 7)))                                                          # the factors stay, the cameras go
    out.value = 1
    keep = [ptr([0, 1], np.uint32), ptr(ok_idx, np.uint32)]
    assert lib.obvi_map_condition_on_handle(blind._h, mp._m, C.c_int64(2), keep[0], keep[1], C.byref(out)) == -5 and not out.value
    with mp.condition(blind, ok_idx, ok_m, ok_P) as good:
        assert good.n_objects == N_MAP
    blind.close()
    # what the device reports.  Indefinite: one eigenvalue of the window's own block flipped
    bad = np.array(sym(np.asarray(cov)))
    idx = rows_of([60, 33, 3], od)
    w, V = np.linalg.eigh(bad[np.ix_(idx, idx)])
    w[len(w) // 2] = -w[len(w) // 2]
    bad[np.ix_(idx, idx)] = (V * w) @ V.T
    P3 = 0.5 * sym(np.asarray(cov))[np.ix_(idx, idx)]
    with obvi_ba.Map.create(mean, bad, library=helpers.PRODUCT_LIB) as m_bad:
        assert host([60, 33, 3], mean[[60, 33, 3]], P3, m=m_bad) == -6
        assert on([5, 1, 9], [60, 33, 3], m=m_bad) == -6
        assert host(ok_idx, ok_m, ok_P, m=m_bad, refused=False) == 0 and out.value                                    # a window that leaves the block out is as good as before
        lib.obvi_map_destroy(out)
    # a free gauge: the handle form reports what obvi_ba_object_covariances reports, and the handle goes on working
    free = helpers.product_ba()
    synth.upload(free, synth.make_problem(P=12, L=30, O=2, seed=5, min_obj_obs=4, object_classes=("bench", "chair"), const_poses=0))
    out.value = 1
    keep = [ptr([0, 1], np.uint32), ptr([4, 2], np.uint32)]
    assert lib.obvi_map_condition_on_handle(free._h, mp._m, C.c_int64(2), keep[0], keep[1], C.byref(out)) == -6 and not out.value
    with mp.condition(free, ok_idx, ok_m, ok_P) as good:
        assert good.n_objects == N_MAP
    assert free.solve(helpers.ba_params(max_it=3)).num_iterations >= 1
    mp.close()
    assert status_of(lambda: ba.solve(helpers.ba_params(max_it=3))) == 0                                           # the handle is usable
