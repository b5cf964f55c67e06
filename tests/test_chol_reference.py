"""CPU: the yardstick of tests/test_gpu_chol_edges.py judged on its own.  On every case's reduced system (the oracle's): the references -- the numpy emulation
of the tile algorithm, LAPACK, the oracle's long double mirror of obvi_ba_debug_reduced_solve -- stay within the bar of tests/chol_cases.py, and the metric
catches each fault planted in the emulation by at least 100 x the bar (a condition on the test's sensitivity: if a case fails it, the case changes).  The
oracle has no tile grid: its grid_row is the identity, so the tiles are cut in canonical order here; the GPU test cuts them in the device's order."""
import functools

import numpy as np
import pytest

import chol_cases as cc
import helpers

NAMES = [n for n in sorted(cc.CASES) if n not in cc.SAME_PROBLEM]
GIVEN_ON = ("wide", "deep")


@functools.lru_cache(maxsize=None)
def _oracle(name):
    c = cc.case(name)
    o = helpers.oracle_ba(object_block_size=c["od"])
    cc.upload(o, c)
    return o


@functools.lru_cache(maxsize=None)
def _system(name, radius):
    """computed once, shared, never modified"""
    S, b = _oracle(name).debug_reduced_system(radius)
    assert len(b) == cc.case(name)["m"]
    return cc.System(S, b, np.arange(len(b)))


@functools.lru_cache(maxsize=None)
def _random(name):
    s = _system(name, 100.0)
    A, r = cc.random_on_pattern(s.S, s.grid_row, 5)
    return cc.System(A, r, s.grid_row)


@pytest.mark.parametrize("radius", cc.RADII)
@pytest.mark.parametrize("name", NAMES)
def test_references_are_within_the_bar(name, radius):
    s = _system(name, radius)
    bar = s.bar()
    w_emu, w_lapack = s.omega(s.emulate()), s.omega(s.lapack())
    rc, S, b, y, row = _oracle(name).debug_reduced_solve(radius)
    w_oracle = s.omega(y)
    print("%s radius %g: m = %d, nt = %d, bar = %.3g, omega(emulation) = %.3g, omega(LAPACK) = %.3g, omega(oracle mirror) = %.3g" % (name, radius, s.m, s.nt, bar, w_emu, w_lapack, w_oracle))
    assert rc == 0 and np.array_equal(S, s.S) and np.array_equal(b, s.b) and np.array_equal(row, np.arange(s.m))
    assert bar >= (3 * s.m + 1) * cc.U and w_emu <= bar
    assert w_lapack <= bar and w_oracle <= bar
    assert w_oracle <= 4 * 2.0 ** -53, "the long double mirror is not better than double rounding of its own result"
    assert s.omega(cc.solve_ld(s.L, s.bg)[np.argsort(s.perm)].astype(np.float64)) <= 4 * 2.0 ** -53


@pytest.mark.parametrize("fault", cc.FAULTS)
@pytest.mark.parametrize("radius", cc.RADII)
@pytest.mark.parametrize("name", NAMES)
def test_the_metric_catches_a_planted_fault(name, radius, fault):
    s = _system(name, radius)
    if not cc.fault_applies(s, fault):
        assert s.nt == 1 or fault == "pad_zero"            # one tile has no product and no substitution term; full tiles have no padding row
        return
    w, bar = s.omega(s.emulate(fault)), s.bar()
    print("%s radius %g %s: omega = %.3g = %.3g x bar" % (name, radius, fault, w, w / bar))
    assert w >= 100.0 * bar


def test_every_fault_is_planted_somewhere():
    for fault in cc.FAULTS:
        assert sum(cc.fault_applies(_system(n, 100.0), fault) for n in NAMES) >= 3, fault


@pytest.mark.parametrize("name", GIVEN_ON)
def test_given_values_lie_inside_the_fill_closure_and_are_solved(name):
    s = _system(name, 100.0)
    M = cc.tile_mask(s.S, s.grid_row)
    o = _oracle(name)
    for label, (A, r) in (("jacobi", cc.jacobi_scaled(s.S, s.b)), ("random", cc.random_on_pattern(s.S, s.grid_row, 5))):
        assert np.array_equal(A, A.T) and cc.inside_mask(A, s.grid_row, M)
        g = cc.System(A, r, s.grid_row)
        rc, A2, r2, y, _ = o.debug_reduced_solve(100.0, A, r)
        assert rc == 0 and np.array_equal(A2, A) and np.array_equal(r2, r)
        print("%s given %s: bar = %.3g, omega(emulation) = %.3g, omega(LAPACK) = %.3g, omega(oracle mirror) = %.3g" % (name, label, g.bar(), g.omega(g.emulate()), g.omega(g.lapack()), g.omega(y)))
        assert g.omega(y) <= g.bar() and g.omega(g.lapack()) <= g.bar()
    # the closure is a closure, and it is no trivial one on the tree
    assert np.array_equal(cc.tile_mask(np.kron(M | M.T, np.ones((cc.TILE, cc.TILE)))[:s.m, :s.m], s.grid_row), M)
    with pytest.raises(helpers.obvi_ba.ObviError, match="status -1"):
        A = s.S.copy(); A[3, 1] += 1.0                      # not symmetric
        o.debug_reduced_solve(100.0, A, s.b)


@pytest.mark.parametrize("where", ["first", "mid", "root", "edge"])
@pytest.mark.parametrize("name", GIVEN_ON)
def test_oracle_mirror_rejects_and_accepts_the_pivot_sets(name, where):
    g = _random(name)
    o = _oracle(name)
    rows = cc.reject_rows(g)
    assert {lab.split("+")[0] for lab in rows} >= {"first", "mid", "root"} and len(rows) >= 16
    assert all("%s+%d" % (t, p) in rows for t in ("first", "mid", "root") for p in (0, 1, 2, 3, 4))
    for label, grow in rows.items():
        if label.split("+")[0] != (where if where != "edge" else "before_padding"):
            continue
        bad, c = cc.with_pivot(g, grow, -0.5)
        assert bad[c, c] < g.S[c, c] and o.debug_reduced_solve(100.0, bad, g.b)[0] == -6, label
        with pytest.raises(np.linalg.LinAlgError):
            cc.chol_ld(bad[np.ix_(g.perm, g.perm)])
        good, _ = cc.with_pivot(g, grow, 0.5)
        rc, _, _, y, _ = o.debug_reduced_solve(100.0, good, g.b)
        sg = cc.System(good, g.b, g.grid_row)
        at = int(np.flatnonzero(sg.rows == grow)[0])
        assert abs(float(sg.L[at, at] ** 2) / g.S[c, c] - 0.5) < 1e-12
        assert rc == 0 and sg.omega(y) <= sg.bar() and sg.omega(sg.emulate()) <= sg.bar(), label
    if where != "edge":
        return
    nan = g.S.copy()
    nan[5, 2] = nan[2, 5] = np.nan
    assert o.debug_reduced_solve(100.0, nan, g.b)[0] == -6
    rc, _, _, y, _ = o.debug_reduced_solve(100.0, g.S, g.b)
    assert rc == 0 and g.omega(y) <= g.bar()
