"""GPU (-m gpu): a device-resident map moved into another frame under an uncertain transform, and two maps joined (include/obvi_map_frame.h), through the C ABI
on a handle that lends only its device, stream and workspaces.  The yardstick is the information form in long double (tests/map_frame_cases.py; held against
the formula on the CPU by tests/test_map_frame_abi.py) -- never the product.  Bars: 1e-12 of the largest entry of the yardstick for covariances and means --
the rule of tests/test_gpu_map_match.py: three orders over numpy's own fp64 evaluation of the same short sums (6.1e-16 at worst on these inputs) -- 1e-11 for
the chain, the merge's own bar on these maps, and bit-equality where the contract promises it (symmetry, the two exactness clauses, repeatability, the join,
the untouched old map and handle)."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (loaded before libobvi_ba.so: torch brings its own HIP runtime, and the one that is loaded first is the one that finds the device)

import helpers
import map_frame_cases as cases
import obvi_ba
from map_update_cases import N_SMALL, rows_of, sym
from test_gpu_map_pair_priors import inv_ld
from test_gpu_map_resident import N_MAP
from map_support import last_error, lender, objects_only, status_of

pytestmark = pytest.mark.gpu

T = obvi_ba.FACTOR_MAP_GROUP_PRIOR


def device_map(mean, cov, od):
    return obvi_ba.Map.create(mean, cov, object_block_size=od, library=helpers.PRODUCT_LIB)


def moved(mp, ba, transform, cov=None):
    """(mean, cov) of a move whose map is read back and destroyed."""
    with mp.transform(ba, transform, cov) as new:
        assert new.n_objects == mp.n_objects
        return new.get()


def dimension_rows(n, od):
    return np.concatenate([np.arange(od * o + od - 3, od * o + od) for o in range(n)])


# ---- 1. every case against the yardstick ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,od,tname,with_sigma", cases.CASES)
def test_the_move_against_the_information_form(which, od, tname, with_sigma):
    mean, cov, Tr, Sigma = cases.case_inputs(which, od, tname, with_sigma)
    mu_ref, C_ref = cases.reference(which, od, tname, with_sigma)
    ba = lender(od)
    with device_map(mean, cov, od) as mp:
        mu, Cn = moved(mp, ba, Tr, Sigma)
        old = mp.get()
    eC, em = cases.errors(mu, Cn, mu_ref, C_ref)
    print("%s map, od %d, %s%s (%d rows): covariance %.2e  means %.2e" % (which, od, tname, ", Sigma" if with_sigma else "", len(Cn), eC, em))
    assert eC <= 1e-12 and em <= 1e-12
    assert np.array_equal(Cn, Cn.T)
    d = dimension_rows(len(mean), od)
    assert np.array_equal(Cn[np.ix_(d, d)], sym(np.asarray(cov))[np.ix_(d, d)])      # dimensions against dimensions: Cs itself, with or without Sigma
    assert np.array_equal(mu[:, od - 3:], mean[:, od - 3:])
    assert np.array_equal(old[0], mean) and np.array_equal(old[1], cov)              # the old map is as it was
    ba.close()


# ---- 2. the exactness clause of the 7-parameter block ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["small", "large"])
def test_a_pure_translation_of_the_yaw_block_moves_the_centres_and_nothing_else(which):
    od = 7
    mean, cov = cases.case_map(which, od)
    Tr = cases.transform_of("translation", od)
    ba = lender(od)
    with device_map(mean, cov, od) as mp:
        mu, Cn = moved(mp, ba, Tr)
    want = np.array(mean)
    want[:, :3] += Tr[:3]
    assert np.array_equal(Cn, sym(np.asarray(cov))) and np.array_equal(mu, want)
    ba.close()


# ---- 3. every leading sub-map -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("od", [7, 9])
def test_every_leading_sub_map_of_1_to_33_objects(od):
    """One block, block + 1 and 2 blocks + 1 of both block sizes (9 and 7 objects), and n = 1: the reference is the slice of the large map's."""
    mean, cov, Tr, Sigma = cases.case_inputs("large", od, "generic", True)
    mu_ref, C_ref = cases.reference("large", od, "generic", True)
    ba = lender(od)
    worst = (0.0, 0.0)
    for n in range(1, cases.N_SWEEP + 1):
        with device_map(*cases.leading(mean, cov, n, od), od) as mp:
            mu, Cn = moved(mp, ba, Tr, Sigma)
        e = cases.errors(mu, Cn, mu_ref[:n], C_ref[:n * od, :n * od])
        assert max(e) <= 1e-12 and np.array_equal(Cn, Cn.T), (n, e)
        worst = (max(worst[0], e[0]), max(worst[1], e[1]))
    print("od %d, sub-maps of 1 .. %d objects: covariance %.2e  means %.2e" % (od, cases.N_SWEEP, worst[0], worst[1]))
    ba.close()


# ---- 4. repeatability; the handle is left as it was --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("od", [7, 9])
def test_the_same_call_twice_and_on_either_kind_of_handle_gives_the_same_bits_and_leaves_the_handle_alone(od):
    mean, cov, Tr, Sigma = cases.case_inputs("large", od, "generic", True)
    rng = np.random.default_rng(9)
    user = objects_only(rng.normal(size=(N_MAP, od)), od)
    out = []
    with device_map(mean, cov, od) as mp:
        user.set_map_group_priors_from_map(mp, [[5, 1, 9], [2, 0]], [[60, 3, 33], [12, 44]], 1e6)
        r0, W0, _ = user.debug_linearize(T)
        err0 = last_error(user)
        for ba in (user, lender(od), lender(od, deterministic=True)):
            for _ in range(2):
                out.append(moved(mp, ba, Tr, Sigma))
        with mp.join(user, mp) as twice:
            assert twice.n_objects == 2 * N_MAP
        r, W, _ = user.debug_linearize(T)
        assert last_error(user) == err0 and user._fn("ba_num_factors")(user._h, C.c_int32(T)) == 2 and all(np.array_equal(x, y) for x, y in zip(W + r, W0 + r0))
    for mu, Cn in out[1:]:
        assert np.array_equal(mu, out[0][0]) and np.array_equal(Cn, out[0][1])
    assert status_of(lambda: user.solve(helpers.ba_params(max_it=3))) == 0           # the handle is usable
    user.close()


# ---- 5. refusals beside a live handle -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_and_nothing_behind():
    od = 7
    mean, cov, Tr, Sigma = cases.case_inputs("large", od, "generic", True)
    ba = objects_only(np.random.default_rng(9).normal(size=(N_MAP, od)), od)
    mp = device_map(mean, cov, od)
    ba.set_map_group_priors_from_map(mp, [[5, 1, 9], [2, 0]], [[60, 3, 33], [12, 44]], 1e6)
    r0, W0, _ = ba.debug_linearize(T)
    want = cases.formula(mean, cov, Tr, Sigma, od)
    lib = ba._lib
    lib.obvi_map_transform.restype = C.c_int
    lib.obvi_map_join.restype = C.c_int
    out = C.c_void_p()

    def ptr(v):
        return None if v is None else np.ascontiguousarray(v, dtype=np.float64).ctypes.data_as(C.c_void_p)

    def after(says, o):
        assert says in last_error(ba), (says, last_error(ba))
        assert o is None or not out.value                                                                  # *out is NULL
        r, W, _ = ba.debug_linearize(T)
        assert ba._fn("ba_num_factors")(ba._h, C.c_int32(T)) == 2 and all(np.array_equal(a, b) for a, b in zip(W + r, W0 + r0))
        assert max(cases.errors(*moved(mp, ba, Tr, Sigma), *want)) <= 1e-12                                # a valid call goes through

    def move(says, m=mp, t=Tr, s=Sigma, o=out):
        out.value = 1
        keep_alive = [ptr(t), ptr(s)]
        rc = lib.obvi_map_transform(ba._h, m._m if m is not None else None, keep_alive[0], keep_alive[1], C.byref(o) if o is not None else None)
        after(says, o)
        return rc

    def join(says, a=mp, b=mp, o=out):
        out.value = 1
        rc = lib.obvi_map_join(ba._h, a._m if a is not None else None, b._m if b is not None else None, C.byref(o) if o is not None else None)
        after(says, o)
        return rc

    assert move("bad arguments", m=None) == -1 and move("bad arguments", t=None) == -1 and move("bad arguments", o=None) == -1
    assert join("bad arguments", a=None) == -1 and join("bad arguments", b=None) == -1 and join("bad arguments", o=None) == -1
    with obvi_ba.Map.create(np.zeros((3, 9)), np.eye(27), object_block_size=9, library=helpers.PRODUCT_LIB) as nine:
        assert move("block size", m=nine) == -1
        assert join("block size", a=nine) == -1 and join("block size", b=nine) == -1                       # mixed block sizes, either way round
    if torch.cuda.device_count() > 1:                                   # NOT exercised where the suite sees one GPU: the one refusal of the contract this test cannot reach there
        with obvi_ba.Map.create(mean, cov, device_id=1, library=helpers.PRODUCT_LIB) as far:
            assert move("another device", m=far) == -1 and join("another device", b=far) == -1
    for bad in (np.nan, np.inf, -np.inf):
        t_bad, s_bad = np.array(Tr), np.array(Sigma)
        t_bad[2], s_bad[1, 3] = bad, bad
        assert move("transform that is not finite", t=t_bad) == -6 and move("covariance entry that is not finite", s=s_bad) == -6
        assert move("transform that is not finite", t=t_bad, s=None) == -6
    huge = np.array(Sigma)
    huge[1, 2] = huge[2, 1] = 1.5e308                                                                      # finite, but (Sigma + Sigma^T) / 2 is not: the device reports it
    assert move("non-finite entry in the new map", s=huge) == -6
    near_diagonal = np.eye(900 * od) + 1e-3 * np.diag(np.ones(900 * od - 1), 1)
    with obvi_ba.Map.create(np.zeros((900, od)), near_diagonal, library=helpers.PRODUCT_LIB) as wide:      # 2 x 900 x 7 = 12 600 rows: above the 11 585 of 1 GiB
        assert join("1 GiB", a=wide, b=wide) == -1
    mp.close()
    assert status_of(lambda: ba.solve(helpers.ba_params(max_it=3))) == 0                                   # the handle is usable
    ba.close()


# ---- 6. the join ------------------------------------------------------------------------------------------------------------------------------------------------
def blockdiag(a, b):
    na, nb = len(a), len(b)
    out = np.zeros((na + nb, na + nb))
    out[:na, :na], out[na:, na:] = a, b
    return out


@pytest.mark.parametrize("od", [7, 9])
def test_the_join_is_the_block_diagonal_bit_for_bit(od):
    small, large = cases.case_map("small", od), cases.case_map("large", od)
    one = cases.leading(*large, 1, od)
    ba = lender(od)
    with device_map(*small, od) as s, device_map(*large, od) as g, device_map(*one, od) as o:
        for a, b, ma, mb in ((s, s, small, small), (s, g, small, large), (g, s, large, small), (o, o, one, one), (o, g, one, large)):
            with a.join(ba, b) as j:
                mu, Cn = j.get()
            assert np.array_equal(mu, np.concatenate([ma[0], mb[0]])) and np.array_equal(Cn, blockdiag(ma[1], mb[1]))   # as the device holds them: not symmetrised
        joined = s.join(ba, g)
    with joined:                                                                     # both parents went first; the joined map serves a window
        nxt = [5, N_SMALL + 2, N_SMALL + 40]
        idx = rows_of(nxt, od)
        user = objects_only(np.zeros((4, od)), od)
        user.set_map_group_priors_from_map(joined, [[2, 0, 3]], [nxt], 2.0)
        _, W, _ = user.debug_linearize(T)
        full = sym(blockdiag(small[1], large[1]))
        eW = helpers.rel_err(W[0].T @ W[0], inv_ld(full[np.ix_(idx, idx)]).astype(np.float64))
        print("od %d: W^T W of a cut from the joined map against the inverse of its sub-block %.2e" % (od, eW))
        assert eW <= 1e-11
        user.close()
    ba.close()


# ---- 7. the chain: move, join, match, resolve, merge -------------------------------------------------------------------------------------------------------------
def test_a_map_from_another_frame_is_aligned_by_its_duplicates():
    ch = cases.chain()
    ref = cases.chain_reference()
    od = ch.od
    ba = lender(od)
    with device_map(ch.mean_a, ch.cov_a, od) as a, device_map(ch.mean_b, ch.cov_b, od) as b:
        with b.transform(ba, ch.T_est, ch.Sigma) as there:
            mu_m, C_m = there.get()
            joined = a.join(ba, there)
    with joined:
        ia, ib, s, w, counts = joined.match(ba, ref.gate)
        assert [(int(x), int(y)) for x, y in zip(ia, ib)] == sorted(cases.planted(ch)) and counts[0] == cases.N_SHARED and counts[2] == 0
        drop, keep, sel = obvi_ba.map_match_resolve(od, ia, ib, s, library=helpers.PRODUCT_LIB)
        assert np.array_equal(drop, ref.drop) and np.array_equal(keep, ref.keep)
        fused, where = joined.merge(ba, drop, keep)
    with fused:
        mu, Cn = fused.get()
    e_move = cases.errors(mu_m, C_m, ref.moved_mean, ref.moved_cov)
    e_fused = cases.errors(mu, Cn, ref.fused_mean, ref.fused_cov)
    before, after = cases.extra_distances(ch, mu_m[cases.N_SHARED:]), cases.extra_distances(ch, mu[len(ch.mean_a):])
    print("the move: covariance %.2e  means %.2e;  the fused map against the long-double chain: covariance %.2e  means %.2e;  B's own objects from the truth: %s -> %s"
          % (e_move + e_fused + (np.round(before, 4), np.round(after, 4))))
    assert max(e_move) <= 1e-12 and max(e_fused) <= 1e-11
    assert len(mu) == len(ch.mean_a) + cases.N_EXTRA and np.array_equal(Cn, Cn.T)
    assert (after < before).all()                                                    # the objects that have no duplicate were pulled into place too
    ba.close()
