"""CPU: the yardstick of tests/test_gpu_cov_edges.py judged on its own, on the oracle's undamped reduced system of every case of tests/cov_cases.py and on the
given-values sets (chol_cases.jacobi_scaled, chol_cases.random_on_pattern), in the grid order of cov_cases.cpu_grid_row.  The clean emulation lies within
the bar; every planted fault, wherever it can occur, lies at least 100 x above it -- a condition on the cases and the requests, not a measurement: on the
given sets of wide, deep, deeper and deep9 it holds for every fault.  On the handles' own systems the ratio is printed and asserted too, except where the
own system's far coupling is too weak for the fault to matter; those (case, request, fault) are covered by the given sets only:

    deep9, request rhs66, slab_first_late      0.018 x the bar: the second slab holds the last two rows (two extents) of one object, all but decoupled there

The blocks with a feature (k_cov_points, k_cov_point_cross): the fixed incidence of cov_cases.feature_case() holds what it is there for and is full rank
undamped (the long double factorisation of S and of every H_ll goes through), and e_emu of cov_cases.FEATURE_TABLE -- the float64 restatement of the kernels'
own order against the long double formulas -- is measured again and must not have drifted by more than a factor 2."""
import functools

import numpy as np
import pytest

import chol_cases as cc
import cov_cases as cv
import helpers

NAMES = [n for n in cv.CASES if n not in cv.SAME_PROBLEM]
SETS = [(n, lab) for n in cv.CASES for lab in (("own", "jacobi", "random") if n in cv.GIVEN_ON else ("own",))]
OFF_SETS = [(n, lab) for n in cv.OFF_PATTERN_ON for lab in ("own", "random")]
WEAK_OWN = {("deep9", "rhs66", "slab_first_late")}


@functools.lru_cache(maxsize=None)
def _own(name):
    """the oracle's undamped reduced system (the assembly the covariance pass factorises), computed once"""
    c = cv.case(cv.SAME_PROBLEM.get(name, name))
    o = helpers.oracle_ba(object_block_size=c["od"])
    cv.upload(o, c)
    S, b = o.debug_reduced_system(1e300)
    assert len(b) == c["m"] and np.array_equal(S, S.T)
    return S, b


@functools.lru_cache(maxsize=None)
def _system(name, label):
    S, b = _own(name)
    row = cv.cpu_grid_row(cv.case(name))
    A = S if label == "own" else cc.jacobi_scaled(S, b)[0] if label == "jacobi" else cc.random_on_pattern(S, row, 5)[0]
    return cv.CovSystem(A, row)


def _omega_of(s, blocks, ip, emu):
    return max(s.omega(X, np.arange(blocks[x][0], sum(blocks[x])), np.arange(blocks[y][0], sum(blocks[y]))) for X, (x, y) in zip(emu, ip))


@pytest.mark.parametrize("name,label", SETS)
def test_the_clean_recursion_is_within_the_bar(name, label):
    s = _system(name, label)
    w, bar = s.omega_all(s.selinv()), s.bar()
    w_ld = s.omega_all(s.Sigma.astype(np.float64))
    print("%s %s: m = %d, nt = %d, tiles = %d, levels = %d, floor = %.3g, omega(emulation) = %.3g, bar = %.3g, omega(numpy inv) = %.3g, omega(rounded reference) = %.3g"
          % (name, label, s.m, s.nt, int(s.M.sum()), int(cc.tile_levels(s.M).max()) + 1, s.floor, w, bar, s.omega_all(np.linalg.inv(s.S)), w_ld))
    assert bar >= s.floor and w <= bar
    assert w_ld <= cc.U, "the long double reference is not better than double rounding of its own result"
    # the emulation's diagonal tiles are symmetric, and the padding rows decoupled: Sigma there is the identity
    G = cv.emulate_selinv(s.S, s.grid_row)
    pad = np.setdiff1d(np.arange(s.nt * cv.TILE), s.grid_row)
    for k in range(s.nt):
        D = G[k * cv.TILE:(k + 1) * cv.TILE, k * cv.TILE:(k + 1) * cv.TILE]
        assert np.array_equal(D, D.T)
    assert all(G[p, p] == 1.0 for p in pad)


@pytest.mark.parametrize("fault", cv.RECURSION_FAULTS)
@pytest.mark.parametrize("name,label", SETS)
def test_the_measure_catches_a_fault_of_the_recursion(name, label, fault):
    s = _system(name, label)
    if not cv.fault_applies(s, fault):
        assert s.nt <= 2 or fault == "pad_as_data"       # two tiles: one product per target, no i < j; full tiles have no padding row
        return
    w, bar = s.omega_all(s.selinv(fault)), s.bar()
    print("%s %s %s: omega = %.3g = %.3g x bar" % (name, label, fault, w, w / bar))
    assert w >= 100.0 * bar


@pytest.mark.parametrize("name,label", OFF_SETS)
def test_the_clean_forward_route_is_within_the_bar_and_its_faults_are_caught(name, label):
    s, B = _system(name, label), cv.Blocks(cv.case(name))
    sets = cv.off_pattern_sets(s, B)
    caught = {f: 0 for f in cv.FAULTS[5:]}
    for key, pairs in sets.items():
        assert pairs, key
        assert not any(s.on_pattern(B.idx(a), B.idx(b)) for a, b in pairs)
        blocks, ip = cv.request(s, B, pairs)
        rows = [(int(s.grid_row[a]), d) for a, d in blocks]
        bar, w = s.bar_off(blocks, ip)
        line = "%s %s %s: %d pairs, %d right-hand sides, omega(emulation) = %.3g, bar = %.3g;" % (name, label, key, len(pairs), cv.rhs_count(B, pairs), w, bar)
        assert w <= bar
        for fault in caught:
            if not cv.fault_applies(s, fault, rows, ip):
                continue
            wf = _omega_of(s, blocks, ip, s.off_pattern(blocks, ip, fault))
            line += " %s %.3g x bar" % (fault, wf / bar)
            if label != "own" or (name, key, fault) not in WEAK_OWN:
                assert wf >= 100.0 * bar, (key, fault, wf / bar)
                caught[fault] += 1
        print(line)
    assert all(n >= 3 for n in caught.values()), caught
    # the requests reach the edges they are named after
    od = B.od
    counts = {k: cv.rhs_count(B, p) for k, p in sets.items()}
    assert (counts["rhs64"], counts["rhs65"]) == (64, 65) if od == 7 else (counts["rhs63"], counts["rhs66"]) == (63, 66)
    assert counts["over128"] > 128 and cv.sixty_fourth_column_inside_a_block(s, B, sets["over128"])
    assert min(int(s.grid_row[B.start[k][0]]) for p in sets["past_tile0"] for k in p) >= cv.TILE
    tile = lambda k: int(s.grid_row[B.start[k][0]]) // cv.TILE  # noqa: E731
    assert abs(tile(sets["ends"][0][0]) - tile(sets["ends"][0][1])) >= s.nt // 2
    assert {tuple(sorted((a[0], b[0]))) for a, b in sets["groups"]} == {(0, 0), (0, 2), (2, 2)}


@pytest.mark.parametrize("name", NAMES + ["deeper"])
def test_on_the_pattern_restated(name):
    """a pair is on the pattern iff every tile its two blocks' rows touch is in chol_cases.tile_mask: said once tile by tile (CovSystem.on_pattern), once entry by
    entry on the expanded mask; off the pattern exists exactly where the case has tiles that do not exist"""
    s, B = _system(name, "own"), cv.Blocks(cv.case(name))
    full = np.kron(s.M | s.M.T, np.ones((cv.TILE, cv.TILE), bool))
    n_off = 0
    for a in B.keys:
        for b in B.keys:
            ia, ib = B.idx(a), B.idx(b)
            on = s.on_pattern(ia, ib)
            assert on == bool(full[np.ix_(s.grid_row[ia], s.grid_row[ib])].all()) == s.on_pattern(ib, ia) == bool(s.on[np.ix_(ia, ib)].all())
            n_off += not on
    missing = int((~(s.M | s.M.T)).sum())
    print(name, "pairs off the pattern:", n_off, "tiles that do not exist:", missing)
    assert (n_off > 0) == (missing > 0) == (name in cv.OFF_PATTERN_ON)


# ---- blocks with a feature ----------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _features():
    """the feature case on the oracle: its undamped system (full rank: the long double factorisation goes through, for every H_ll too) and its linearisation"""
    case = cv.feature_case()
    o = helpers.oracle_ba()
    cv.feature_upload(o, case)
    S, b = o.debug_reduced_system(1e300)
    assert len(b) == case["m"]
    s = cv.CovSystem(S, np.arange(len(b)))
    ref = cv.FeatureRef(case, *o.debug_linearize(0))
    for l in np.flatnonzero((case["prob"]["point_const"] == 0) & (np.diff(ref.ptr) > 0)):
        cc.chol_ld(ref.H(int(l)))
    return case, s, ref


def test_the_feature_case_holds_what_it_is_there_for():
    case, s, ref = _features()
    g, prob = case["groups"], case["prob"]
    n = {k: len(ref.records(g[k][0])) for k in cv.FEATURE_GROUPS}
    live = {k: sum(r >= 0 for _, r in ref.records(g[k][0])) for k in cv.FEATURE_GROUPS}
    assert [n[k] for k in ("n2", "n8", "n9", "n63", "n64", "n65")] == [2, 8, 9, 63, 64, 65] and all(live[k] == n[k] for k in ("n2", "n8", "n9", "n63", "n64", "n65", "stereo"))
    assert n["n8"] ** 2 == 64 and n["n9"] ** 2 > 64                  # one full stride of k_cov_points; the second stride begun
    rec = ref.records(g["stereo"][0])
    assert len(rec) == 6 and len({r for _, r in rec}) == 3           # two records per frame
    assert live["masked"] == n["masked"] - 1 and live["const_pose"] == n["const_pose"] - 1
    assert prob["point_const"][g["const_point"][0]] == 1 and len(ref.records(g["unobserved"][0])) == 0
    assert ref.block((cv.POINT, g["const_point"][0]), (cv.POSE, 5), s.Sigma) is None


def test_the_feature_table_has_not_drifted():
    """e_emu per feature and kind of block, measured here on the oracle's system; the clean restatement lies within the bar by construction"""
    case, s, ref = _features()
    S64 = s.Sigma.astype(np.float64)
    worst = {k: [0.0, 0.0, 0.0] for k in cv.FEATURE_GROUPS}
    for group, a, b in cv.feature_pairs(case):
        e = ref.error(ref.emulate(a, b, S64), a, b, s.Sigma)
        k = cv.KINDS.index(cv.feature_kind(a, b))
        worst[group][k] = max(worst[group][k], e)
    for group in cv.FEATURE_GROUPS:
        print('    "%s": e_emu=(%s)' % (group, ", ".join("%.2g" % v for v in worst[group])))
    for group in cv.FEATURE_GROUPS:
        for v, t in zip(worst[group], cv.FEATURE_TABLE[group]["e_emu"]):
            assert t / 2 <= v <= 2 * t, (group, worst[group], cv.FEATURE_TABLE[group]["e_emu"])
    for group, a, b in cv.feature_pairs(case):
        assert ref.error(ref.emulate(a, b, S64), a, b, s.Sigma) <= cv.feature_bar(ref, group, a, b)
