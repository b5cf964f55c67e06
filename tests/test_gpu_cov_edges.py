"""The covariance kernels on the factor of the tile Cholesky (k_selinv_y, k_selinv_off, k_selinv_diag, k_cov_gather, k_cov_seed_rows, k_cov_forward,
k_cov_rhs_pairs) against the exact inverse of the system the pass itself inverts, at the tile, level and slab edges the cases of tests/cov_cases.py are aimed
at, through obvi_cov_debug_compute_pairs.  omega(block) = max |Sigma - Sigma*| / (|Sigma*| |L*||L*^T| |Sigma*|), Sigma* and L* in long double from the returned
system, must stay within max((3 m + 1) 2^-53, 8 omega(emulation)), the emulation being the numpy float64 restatement of the recursion (of the forward route)
on the same system in the device's own grid order.  A dropped product, an untransposed operand, a Y formed in place, a padding row taken for data, a skipped
forward term or a slab or a pair started one tile late exceed that bar by six to twelve orders (tests/test_cov_reference.py).

The blocks with a feature (k_cov_points, k_cov_point_cross) are held to the kernels' own formulas in long double on the same Sigma*, on the fixed incidence of
cov_cases.feature_case() (test_blocks_with_a_feature; the bar and what sets it: cov_cases.FEATURE_TABLE).

With 9-parameter objects the number of right-hand sides is a multiple of 3: deep9 stands at 63 and 66 where the other cases stand at exactly 64 and 65."""
import numpy as np
import pytest

import chol_cases as cc
import cov_cases as cv
import helpers
from test_gpu_chol_edges import SCHEDULES

pytestmark = pytest.mark.gpu

HANDLES = ("default", "deterministic")
RUNS = [(name, sched) for name in cv.CASES for sched in (sorted(SCHEDULES) if name in cv.MULTI_TILE else HANDLES)]
_systems = {}


def _product(name, sched, monkeypatch):
    c = cv.case(name)
    for k, v in {**c["knobs"], **SCHEDULES.get(sched, {})}.items():          # knobs are read once per handle: before it exists
        monkeypatch.setenv(k, v)
    g = helpers.product_ba(deterministic=sched == "deterministic", object_block_size=c["od"])
    cv.upload(g, c)
    return c, g, cv.Blocks(c)


def _system(S, row):
    """the reference of one returned system, computed once (a deterministic handle returns the same bits again)"""
    key = (S.tobytes(), row.tobytes())
    if key not in _systems:
        _systems[key] = cv.CovSystem(S, row)
    return _systems[key]


def _kinds(keys):
    return np.array([k[0] for k in keys], np.uint8), np.array([k[1] for k in keys], np.uint32)


def _check_on_pattern(g, B, s, what):
    """own blocks, every pair on the pattern both ways, the pattern test itself, exact symmetries, zero blocks, a refusal off the pattern"""
    bar, w_emu = s.bar(), s.omega_all(s.selinv())
    worst = 0.0
    poses = g.pose_covariances(np.arange(B.nP))
    objs = g.object_covariance_blocks(np.arange(B.nO))
    for p in B.const_pose:
        assert not poses[p].any(), "the block of a constant pose is not zero"
    for key in B.keys:
        X = poses[key[1]] if key[0] == cv.POSE else objs[key[1]]
        assert np.array_equal(X, X.T), (what, key, "own block not symmetric")
        w = s.omega(X, B.idx(key), B.idx(key))
        worst = max(worst, w)
        assert w <= bar, (what, key, w, bar)
    pairs = [(a, b) for x, a in enumerate(B.keys) for b in B.keys[x + 1:]]
    (ka, ia), (kb, ib) = _kinds([p[0] for p in pairs]), _kinds([p[1] for p in pairs])
    on = g.covariance_on_pattern(ka, ia, kb, ib)
    want = np.array([s.on_pattern(B.idx(a), B.idx(b)) for a, b in pairs])
    assert np.array_equal(on.astype(bool), want), (what, "obvi_cov_on_pattern differs from the fill closure of the returned system")
    assert np.array_equal(g.covariance_on_pattern(kb, ib, ka, ia), on)
    sel = np.flatnonzero(want)
    ab = g.cross_covariances(ka[sel], ia[sel], kb[sel], ib[sel])
    ba = g.cross_covariances(kb[sel], ib[sel], ka[sel], ia[sel])
    for x, q in enumerate(sel):
        a, b = pairs[q]
        assert np.array_equal(ba[x], ab[x].T), (what, a, b, "(b, a) is not the transpose of (a, b)")
        w = s.omega(ab[x], B.idx(a), B.idx(b))
        worst = max(worst, w)
        assert w <= bar, (what, a, b, w, bar)
    # pairs with a constant pose are zero blocks, on the pattern by definition
    for p in B.const_pose:
        z = g.cross_covariances([cv.POSE, cv.OBJECT], [p, 0], [cv.OBJECT, cv.POSE], [0, p])
        assert not z[0].any() and not z[1].any()
    off = np.flatnonzero(~want)
    if len(off):
        a, b = pairs[off[len(off) // 2]]
        with pytest.raises(helpers.obvi_ba.ObviError, match="status -1"):
            g.cross_covariances([a[0]], [a[1]], [b[0]], [b[1]])
        assert np.array_equal(g.pose_covariances(np.arange(B.nP)), poses)          # the handle goes on
    print("%s: m = %d, nt = %d, %d own blocks, %d pairs on the pattern, %d off it, omega(device) = %.3g, omega(emulation) = %.3g, bar = %.3g"
          % (what, s.m, s.nt, len(B.keys), len(sel), len(off), worst, w_emu, bar))
    return worst


def _check_stats(g, c, s):
    st = g.problem_stats()
    shown = {k: int(st[k]) for k in ("reduced_rows", "tiles_per_dim", "tiles_nonzero", "trsm_jobs", "update_jobs", "chol_levels")}
    print(c["name"], shown, "padding rows", int(st["tiles_per_dim"]) * cv.TILE - c["m"], "tiles of the Python fill closure", int(s.M.sum()))
    for k, v in c["expect"].items():
        if k.startswith("min_"):
            assert st[k[4:]] >= v, (k, st[k[4:]])
        else:
            assert st[k] == v, (k, st[k])
    assert int(s.M.sum()) == st["tiles_nonzero"]


@pytest.mark.parametrize("name,sched", RUNS)
def test_own_system_blocks_on_the_pattern(name, sched, monkeypatch):
    c, g, B = _product(name, sched, monkeypatch)
    S, row = g.covariance_debug_compute_pairs()
    assert S.shape == (c["m"], c["m"]) and np.array_equal(S, S.T) and len(np.unique(row)) == c["m"]
    s = _system(S, row)
    _check_stats(g, c, s)
    _check_on_pattern(g, B, s, "%s %s own" % (name, sched))
    # the same assembly as the undamped obvi_ba_debug_reduced_system (atomics: two assemblies differ in the last bits)
    S2, _ = g.debug_reduced_system(1e300)
    assert helpers.rel_err(S, S2) < 1e-11


def _base(name):
    """the oracle's undamped system of the case: what the given-values sets are made from"""
    c = cv.case(name)
    o = helpers.oracle_ba(object_block_size=c["od"])
    cv.upload(o, c)
    return o.debug_reduced_system(1e300)


_bases = {}


def _given(name, label, row):
    if name not in _bases:
        _bases[name] = _base(cv.SAME_PROBLEM.get(name, name))
    S, b = _bases[name]
    return cc.jacobi_scaled(S, b)[0] if label == "jacobi" else cc.random_on_pattern(S, row, 5)[0]


@pytest.mark.parametrize("sched", HANDLES)
@pytest.mark.parametrize("name", cv.GIVEN_ON)
def test_given_values_blocks_on_the_pattern(name, sched, monkeypatch):
    c, g, B = _product(name, sched, monkeypatch)
    S0, row = g.covariance_debug_compute_pairs()
    own = _system(S0, row)
    for label in ("jacobi", "random"):
        A = _given(name, label, row)
        assert cc.inside_mask(A, row, own.M)
        A2, row2 = g.covariance_debug_compute_pairs(lhs_in=A)
        assert np.array_equal(A2, A) and np.array_equal(row2, row)
        _check_on_pattern(g, B, _system(A, row), "%s %s given %s" % (name, sched, label))
    A = _given(name, "random", row)
    s = _system(A, row)

    def own_again(after):
        S1, _ = g.covariance_debug_compute_pairs()
        _check_on_pattern(g, B, _system(S1, row), "%s %s own after %s" % (name, sched, after))

    # an entry outside the structural mask is refused; the handle goes on
    perm, rows, nt = cc.grid(row)
    missing = [(i, j) for i in range(nt) for j in range(i) if not own.M[i, j] and (rows // cc.TILE == i).any() and (rows // cc.TILE == j).any()]
    assert missing or name == "wide"                             # (one dense node has every tile)
    if missing:
        a, b_ = missing[0]
        i, j = int(perm[np.flatnonzero(rows // cc.TILE == a)[0]]), int(perm[np.flatnonzero(rows // cc.TILE == b_)[0]])
        bad = A.copy(); bad[i, j] = bad[j, i] = 1e-3
        with pytest.raises(helpers.obvi_ba.ObviError, match="status -1"):
            g.covariance_debug_compute_pairs(lhs_in=bad)
        own_again("an entry outside the mask")
    bad = A.copy(); bad[3, 1] += 1.0                             # not symmetric
    with pytest.raises(helpers.obvi_ba.ObviError, match="status -1"):
        g.covariance_debug_compute_pairs(lhs_in=bad)
    # a pivot of -0.5 S_gg at a first-level row and at the root: OBVI_ERR_NUMERICAL, as the pass answers rank deficiency
    reject = cc.reject_rows(s.sys, own.M)
    for lab in ("first+1", "root+0"):
        bad, _ = cc.with_pivot(s.sys, reject[lab], -0.5)
        with pytest.raises(helpers.obvi_ba.ObviError, match="status -6"):
            g.covariance_debug_compute_pairs(lhs_in=bad)
        with pytest.raises(helpers.obvi_ba.ObviError):           # no result is served after a refused pass
            g.pose_covariances([1])
        own_again("a pivot of -0.5 S_gg at %s" % lab)
    nan = A.copy()
    i, j = int(perm[5]), int(perm[2])
    nan[i, j] = nan[j, i] = np.nan
    with pytest.raises(helpers.obvi_ba.ObviError, match="status -6"):
        g.covariance_debug_compute_pairs(lhs_in=nan)
    own_again("a NaN")


@pytest.mark.parametrize("sched", HANDLES)
@pytest.mark.parametrize("label", ["own", "random"])
@pytest.mark.parametrize("name", cv.OFF_PATTERN_ON)
def test_pairs_off_the_pattern_at_the_slab_edges(name, label, sched, monkeypatch):
    c, g, B = _product(name, sched, monkeypatch)
    S0, row = g.covariance_debug_compute_pairs()
    A = None if label == "own" else _given(name, "random", row)
    sets = cv.off_pattern_sets(_system(S0, row) if A is None else _system(A, row), B)
    counts = {k: cv.rhs_count(B, p) for k, p in sets.items()}
    print(name, label, sched, "right-hand sides:", counts)
    # each edge is reached
    assert all(sets.values())
    assert (counts["rhs64"], counts["rhs65"]) == (64, 65) if B.od == 7 else (counts["rhs63"], counts["rhs66"]) == (63, 66)
    tile = lambda k: int(row[B.start[k][0]]) // cv.TILE  # noqa: E731
    assert min(tile(k) for p in sets["past_tile0"] for k in p) >= 1
    assert abs(tile(sets["ends"][0][0]) - tile(sets["ends"][0][1])) >= (int(row.max()) // cv.TILE + 1) // 2
    assert {tuple(sorted((a[0], b[0]))) for a, b in sets["groups"]} == {(0, 0), (0, 2), (2, 2)}
    for key, pairs in sets.items():                               # (nothing is declared so far: the product's own word on the pattern)
        (ka, ia), (kb, ib) = _kinds([p[0] for p in pairs]), _kinds([p[1] for p in pairs])
        assert not g.covariance_on_pattern(ka, ia, kb, ib).any(), (key, "a pair of the request is on the pattern")
    for key, pairs in sets.items():
        (ka, ia), (kb, ib) = _kinds([p[0] for p in pairs]), _kinds([p[1] for p in pairs])
        S, row2 = g.covariance_debug_compute_pairs(ka, ia, kb, ib, lhs_in=A)
        assert np.array_equal(row2, row) and (A is None or np.array_equal(S, A))
        s = _system(S, row)
        if key == "over128":
            assert counts[key] > 2 * cv.TILE and cv.sixty_fourth_column_inside_a_block(s, B, pairs)
        assert g.covariance_on_pattern(ka, ia, kb, ib).all()
        blocks, ip = cv.request(s, B, pairs)
        bar, w_emu = s.bar_off(blocks, ip)
        ab, ba = g.cross_covariances(ka, ia, kb, ib), g.cross_covariances(kb, ib, ka, ia)
        worst = 0.0
        for x, (a, b) in enumerate(pairs):
            assert np.array_equal(ba[x], ab[x].T), (key, a, b, "(b, a) is not the transpose of (a, b)")
            w = s.omega(ab[x], B.idx(a), B.idx(b))
            worst = max(worst, w)
            assert w <= bar, (name, label, sched, key, a, b, w, bar)
        print("%s %s %s %s: %d pairs, %d right-hand sides, omega(device) = %.3g, omega(emulation) = %.3g, bar = %.3g" % (name, label, sched, key, len(pairs), counts[key], worst, w_emu, bar))
        if sched == "deterministic":                             # two passes are bit-identical
            g.covariance_debug_compute_pairs(ka, ia, kb, ib, lhs_in=A)
            again = g.cross_covariances(ka, ia, kb, ib)
            assert all(np.array_equal(x, y) for x, y in zip(ab, again)), key
    # the blocks on the pattern of the last pass are those of a plain pass, within the same bar
    poses = g.pose_covariances(B.var_pose)
    for x, p in enumerate(B.var_pose):
        assert s.omega(poses[x], B.idx((cv.POSE, int(p))), B.idx((cv.POSE, int(p)))) <= s.bar()


@pytest.mark.parametrize("after", ["debug_call", "rejected_call"])
@pytest.mark.parametrize("name", ["wide", "deep9"])
def test_a_handle_after_a_debug_call_is_a_fresh_handle(name, after, monkeypatch):
    """state hygiene on deterministic handles: two LM iterations after a debug call -- after a refused one -- give the records and the state of a handle that
    never made one, and a plain covariance pass gives the same bits"""
    prm = helpers.ba_params(max_it=2, ftol=0, ptol=0, gtol=0)
    out = []
    for debug in (False, True):
        c, g, B = _product(name, "deterministic", monkeypatch)
        if debug:
            S0, row = g.covariance_debug_compute_pairs()
            A = _given(name, "random", row)
            if after == "rejected_call":
                s = _system(A, row)
                bad, _ = cc.with_pivot(s.sys, int(s.sys.rows[1]), -0.5)
                with pytest.raises(helpers.obvi_ba.ObviError, match="status -6"):
                    g.covariance_debug_compute_pairs(lhs_in=bad)
            else:
                g.covariance_debug_compute_pairs(lhs_in=A)
        g.covariance_compute()
        blocks = [g.pose_covariances(np.arange(B.nP)), g.object_covariance_blocks(np.arange(B.nO))]
        g.solve(prm)
        its = g.iterations()
        for it in its:
            it.iteration_time_in_seconds = 0.0
        out.append(([bytes(it) for it in its], g.get_state(), blocks))
        g.close()
    assert len(out[0][0]) == 3
    assert out[0][0] == out[1][0] and all(np.array_equal(x, y) for x, y in zip(out[0][1], out[1][1]))
    assert all(np.array_equal(x, y) for x, y in zip(out[0][2], out[1][2])) and out[0][2][0][1].any()


# ---- blocks with a feature (k_cov_points, k_cov_point_cross) ---------------------------------------------------------------------------------------------

_feature_refs = {}


def _feature_ref():
    """the oracle's linearisation of the feature case (H_ll and W of every record) and Sigma* of the oracle's own system, computed once"""
    if not _feature_refs:
        case = cv.feature_case()
        o = helpers.oracle_ba()
        cv.feature_upload(o, case)
        S, b = o.debug_reduced_system(1e300)
        _feature_refs["ref"] = (case, cv.FeatureRef(case, *o.debug_linearize(0)), cv.CovSystem(S, np.arange(len(b))).Sigma)
    return _feature_refs["ref"]


@pytest.mark.parametrize("sched", HANDLES)
def test_blocks_with_a_feature(sched):
    """own blocks and declared (feature, pose), (feature, object), (feature, feature) pairs of the features with 2, 8, 9, 63, 64 and 65 records, the stereo, the
    masked and the constant-pose feature, against the kernels' formulas in long double on Sigma* of the returned system: within cov_cases.feature_bar"""
    case, ref, Sigma_oracle = _feature_ref()
    g = helpers.product_ba(deterministic=sched == "deterministic")
    cv.feature_upload(g, case)
    trip = cv.feature_pairs(case)
    (ka, ia), (kb, ib) = _kinds([a for _, a, _ in trip]), _kinds([b for _, _, b in trip])
    S, row = g.covariance_debug_compute_pairs(ka, ia, kb, ib)
    assert len(S) == case["m"]
    Sigma = _system(S, row).Sigma
    ab, ba = g.cross_covariances(ka, ia, kb, ib), g.cross_covariances(kb, ib, ka, ia)
    ids = [case["groups"][k][0] for k in cv.FEATURE_GROUPS]
    own = g.point_covariances(ids)
    d_worst = {k: [0.0, 0.0, 0.0] for k in cv.FEATURE_GROUPS}
    fails = []
    for x, (group, a, b) in enumerate(trip):
        assert np.array_equal(ba[x], ab[x].T), (a, b, "(b, a) is not the transpose of (a, b)")
        if a == b:                                               # the getter of own blocks and the declared self pair: one kernel, the same bits
            assert np.array_equal(own[ids.index(a[1])], ab[x]) and np.array_equal(ab[x], ab[x].T)
        err, bar = ref.error(ab[x], a, b, Sigma), cv.feature_bar(ref, group, a, b)
        d = ref.error(ref.block(a, b, Sigma_oracle), a, b, Sigma)
        k = cv.KINDS.index(cv.feature_kind(a, b))
        d_worst[group][k] = max(d_worst[group][k], d)
        print("%s %s %s %s: error(device) = %.3g, d = %.3g, n_terms = %d, bar = %.3g" % (sched, group, a, b, err, d, ref.n_terms(a, b), bar))
        if not err <= bar:
            fails.append((group, a, b, err, bar))
    for group in cv.FEATURE_GROUPS:
        print('    "%s": d=(%s)' % (group, ", ".join("%.2g" % v for v in d_worst[group])))
    assert not fails, fails
    # constant and unobserved features: exact zeros, own and declared
    dead = [case["groups"]["const_point"][0], case["groups"]["unobserved"][0]]
    assert not g.point_covariances(dead).any()
    g.covariance_compute_pairs([cv.POINT] * 4, dead + dead, [cv.POSE, cv.POSE, cv.POINT, cv.OBJECT], [5, 5, ids[0], 0])
    assert not any(x.any() for x in g.cross_covariances([cv.POINT] * 4, dead + dead, [cv.POSE, cv.POSE, cv.POINT, cv.OBJECT], [5, 5, ids[0], 0]))
    if sched == "deterministic":                                 # (the system a deterministic handle returns is the same bits every time: d is a fixed figure)
        for group in cv.FEATURE_GROUPS:
            for v, t in zip(d_worst[group], cv.FEATURE_TABLE[group]["d"]):
                assert t / 2 <= v <= 2 * t, (group, d_worst[group], cv.FEATURE_TABLE[group]["d"])
