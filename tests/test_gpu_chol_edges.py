"""The tile Cholesky solve of an LM step (k_potrf, k_trsm, k_update, k_update_potrf / k_potrf_pre, k_backward, k_backward_det) by backward error, at the tile,
level and pivot edges the cases of tests/chol_cases.py are aimed at and on every schedule, through obvi_ba_debug_reduced_solve: the system the factorisation
saw, and the y the back-substitution pass reads.  omega(y) (chol_cases: componentwise backward error against |L*||L*^T|, L* in long double) must stay within
max((3 m + 1) 2^-53, 8 omega(y_emu)), y_emu the numpy float64 emulation of the tile algorithm on the same system in the device's own grid order.  A dropped
product, a skipped substitution term, a padding row taken for data or an inverse entry off in the ninth digit exceed that bar by two to twelve orders
(tests/test_chol_reference.py).  Then the pivot checks on given values: a pivot of -0.5 S_gg at each of the four roles of a 4 x 4 block, at the tile's far
end and in front of padding, in a first-level, a mid-level and the root tile, must be refused, its twin with +0.5 S_gg solved within the bar, a NaN refused,
and the handle must be clean afterwards."""
import functools

import numpy as np
import pytest

import chol_cases as cc
import helpers

pytestmark = pytest.mark.gpu

SCHEDULES = {"default": {}, "two_launch": {"OBVI_FUSED_POTRF": "0"}, "slice_none": {"OBVI_SLICE_MAX": "0"}, "slice_all": {"OBVI_SLICE_MAX": "1000000"},
             "xcd_off": {"OBVI_CHOL_XCD": "0"}, "deterministic": {}}
EXTRA = {"wide": {"chunk1": {"OBVI_UPD_CHUNK": "1"}, "chunk1_pre0": {"OBVI_UPD_CHUNK": "1", "OBVI_PRE_MAX": "0"}, "chunk2_pre0": {"OBVI_UPD_CHUNK": "2", "OBVI_PRE_MAX": "0"},
                  "chunk2_pre8": {"OBVI_UPD_CHUNK": "2", "OBVI_PRE_MAX": "8"}, "chunk1_pre8_two_launch": {"OBVI_UPD_CHUNK": "1", "OBVI_PRE_MAX": "8", "OBVI_FUSED_POTRF": "0"}},
         "deep": {"backward%s" % n: {"OBVI_BACKWARD_LEVELS": n} for n in ("1", "3", "4", "8")},
         "deeper": {"backward%s" % n: {"OBVI_BACKWARD_LEVELS": n} for n in ("1", "3", "4", "8")}}
RUNS = [(name, sched) for name in sorted(cc.CASES) for sched in (sorted(SCHEDULES) if name in cc.MULTI_TILE else ["default", "deterministic"]) + sorted(EXTRA.get(name, {}))]
GIVEN_ON = ("wide", "deep", "deeper")
TWO = ("default", "two_launch")            # the fused and the two-launch schedule


def _env(name, sched):
    return {**cc.case(name)["knobs"], **SCHEDULES.get(sched, {}), **EXTRA.get(name, {}).get(sched, {})}


def _product(name, sched, monkeypatch):
    c = cc.case(name)
    env = _env(name, sched)
    for k, v in env.items():                                     # knobs are read once per handle: before it exists
        monkeypatch.setenv(k, v)
    g = helpers.product_ba(deterministic=sched == "deterministic", object_block_size=c["od"])
    cc.upload(g, c)
    return c, g, env


def _within_bar(s, y, what):
    w, w_emu, bar = s.omega(y), s.omega(s.emulate()), s.bar()
    print("%s: m = %d, nt = %d, omega(device) = %.3g, omega(emulation) = %.3g, omega(LAPACK) = %.3g, bar = %.3g" % (what, s.m, s.nt, w, w_emu, s.omega(s.lapack()), bar))
    assert w <= bar, (what, w, bar)


@pytest.mark.parametrize("name,sched", RUNS)
def test_own_system_is_solved_within_the_bar(name, sched, monkeypatch):
    c, g, env = _product(name, sched, monkeypatch)
    for radius in cc.RADII:
        rc, S, b, y, row = g.debug_reduced_solve(radius)
        assert rc == 0 and len(b) == c["m"]
        st = g.problem_stats()
        nt = int(st["tiles_per_dim"])
        # grid_row: a permutation of real rows, blocks of 6 (od) consecutive rows, the rest of the grid padding
        assert len(np.unique(row)) == c["m"] and row.min() >= 0 and row.max() < nt * cc.TILE
        n_pose_rows = 6 * int(st["poses_var"])
        assert (np.diff(row[:n_pose_rows].reshape(-1, 6), axis=1) == 1).all() and (np.diff(row[n_pose_rows:].reshape(-1, c["od"]), axis=1) == 1).all()
        s = cc.System(S, b, row)
        assert s.nt == nt or nt * cc.TILE - c["m"] >= cc.TILE, "the last tiles of the grid hold padding only"
        _within_bar(s, y, "%s %s radius %g" % (name, sched, radius))
        # the same assembly as obvi_ba_debug_reduced_system, to that entry's tolerance against the oracle (atomics: two assemblies differ in the last bits)
        S2, b2 = g.debug_reduced_system(radius)
        assert helpers.rel_err(S, S2) < 1e-11 and helpers.rel_err(b, b2) < 1e-10 and np.array_equal(S, S.T)
    # the structure the case is there for
    M = cc.tile_mask(S, row)
    print(name, sched, {k: int(v) for k, v in st.items() if k in ("reduced_rows", "tiles_per_dim", "tiles_nonzero", "trsm_jobs", "update_jobs", "chol_levels", "fused_potrf", "potrf_wait_timeouts")},
          "padding rows", nt * cc.TILE - c["m"], "tiles of the Python fill closure", int(M.sum()), "levels", int(cc.tile_levels(M).max()) + 1)
    for k, v in c["expect"].items():
        if k.startswith("min_"):
            assert st[k[4:]] >= v, (k, st[k[4:]])
        else:
            assert st[k] == v, (k, st[k])
    if nt > 1:
        assert st["trsm_jobs"] >= 1 and int(M.sum()) == st["tiles_nonzero"] and int(cc.tile_levels(M).max()) + 1 <= st["chol_levels"]
    if st["potrf_wait_timeouts"] == 0:
        assert st["fused_potrf"] == (0 if env.get("OBVI_FUSED_POTRF") == "0" else 1)


@functools.lru_cache(maxsize=None)
def _base(name):
    """the oracle's system of the case at radius 100: what the given-values sets are made from (shared, never modified)"""
    c = cc.case(name)
    o = helpers.oracle_ba(object_block_size=c["od"])
    cc.upload(o, c)
    return o.debug_reduced_system(100.0)


def _given_sets(name, row):
    S, b = _base(name)
    return {"jacobi": cc.jacobi_scaled(S, b), "random": cc.random_on_pattern(S, row, 5)}


@pytest.mark.parametrize("sched", sorted(SCHEDULES))
@pytest.mark.parametrize("name", GIVEN_ON)
def test_given_values_are_solved_within_the_bar(name, sched, monkeypatch):
    c, g, _ = _product(name, sched, monkeypatch)
    rc, S0, b0, _, row = g.debug_reduced_solve(100.0)
    assert rc == 0
    M = cc.tile_mask(S0, row)
    for label, (A, r) in _given_sets(name, row).items():
        assert cc.inside_mask(A, row, M)
        rc, A2, r2, y, row2 = g.debug_reduced_solve(100.0, A, r)
        assert rc == 0 and np.array_equal(A2, A) and np.array_equal(r2, r) and np.array_equal(row2, row)
        _within_bar(cc.System(A, r, row), y, "%s %s given %s" % (name, sched, label))
    # an entry outside the structural mask is refused; the handle goes on
    perm, rows, nt = cc.grid(row)
    missing = [(i, j) for i in range(nt) for j in range(i) if not M[i, j] and (rows // cc.TILE == i).any() and (rows // cc.TILE == j).any()]
    assert missing or name == "wide"                             # (one dense node has every tile)
    if missing:
        a, b_ = missing[0]
        i, j = int(perm[np.flatnonzero(rows // cc.TILE == a)[0]]), int(perm[np.flatnonzero(rows // cc.TILE == b_)[0]])
        A, r = _given_sets(name, row)["random"]
        A = A.copy(); A[i, j] = A[j, i] = 1e-3
        with pytest.raises(helpers.obvi_ba.ObviError, match="status -1"):
            g.debug_reduced_solve(100.0, A, r)
    rc, S1, b1, y1, _ = g.debug_reduced_solve(100.0)
    assert rc == 0
    _within_bar(cc.System(S1, b1, row), y1, "%s %s own system after the given ones" % (name, sched))


@pytest.mark.parametrize("where", ["first", "mid", "root", "edge"])
@pytest.mark.parametrize("sched", TWO)
@pytest.mark.parametrize("name", GIVEN_ON)
def test_pivot_checks(name, sched, where, monkeypatch):
    """rejection set, acceptance twin, NaN; after every refusal the same handle solves the unmodified system within the bar"""
    c, g, _ = _product(name, sched, monkeypatch)
    rc, S0, b0, _, row = g.debug_reduced_solve(100.0)
    assert rc == 0
    A, r = _given_sets(name, row)["random"]
    s = cc.System(A, r, row)
    rows = cc.reject_rows(s, cc.tile_mask(S0, row))
    print(name, sched, "rows of the tile grid:", rows)
    roles = {lab.split("+")[0] for lab in rows}
    assert {"first", "root"} <= roles and ("mid" in roles or s.nt < 3)
    assert all("%s+%d" % (t, p) in rows for t in roles - {"before_padding"} for p in (0, 1, 2, 3, 4))
    if name == "wide":
        assert all("%s+%d" % (t, p) in rows for t in ("first", "mid", "root") for p in cc.REJECT_POS)
    else:
        assert "before_padding" in rows
    for label, grow in rows.items():
        if label.split("+")[0] != (where if where != "edge" else "before_padding"):
            continue
        bad, _ = cc.with_pivot(s, grow, -0.5)
        assert g.debug_reduced_solve(100.0, bad, r)[0] == -6, "a pivot of -0.5 S_gg at %s (grid row %d) was not refused" % (label, grow)
        rc, _, _, y, _ = g.debug_reduced_solve(100.0, A, r)           # failure counter and tiles were cleared
        assert rc == 0 and s.omega(y) <= s.bar(), (label, s.omega(y), s.bar())
        good, _ = cc.with_pivot(s, grow, 0.5)
        rc, _, _, y, _ = g.debug_reduced_solve(100.0, good, r)
        sg = cc.System(good, r, row)
        assert rc == 0 and sg.omega(y) <= sg.bar(), (label, rc, sg.omega(y), sg.bar())
    if where != "edge":
        return
    # a NaN in one entry (off the diagonal, in the first tile column)
    perm = s.perm
    nan = A.copy()
    i, j = int(perm[5]), int(perm[2])
    nan[i, j] = nan[j, i] = np.nan
    assert g.debug_reduced_solve(100.0, nan, r)[0] == -6
    rc, _, _, y, _ = g.debug_reduced_solve(100.0, A, r)
    assert rc == 0 and s.omega(y) <= s.bar()
    if sched == "two_launch":                                    # nothing waits inside a launch there
        assert g.problem_stats()["potrf_wait_timeouts"] == 0


@pytest.mark.parametrize("after", ["debug_call", "rejected_call"])
@pytest.mark.parametrize("name", GIVEN_ON)
def test_a_solve_after_a_debug_call_is_a_fresh_handles_solve(name, after, monkeypatch):
    """state hygiene on deterministic handles (two solves of one problem are bit-identical there): two LM iterations after a debug call -- after a refused one --
    give the records and the state of a handle that never made one"""
    prm = helpers.ba_params(max_it=2, ftol=0, ptol=0, gtol=0)
    out = []
    for debug in (False, True):
        c, g, _ = _product(name, "deterministic", monkeypatch)
        if debug:
            rc, S0, b0, _, row = g.debug_reduced_solve(100.0)
            assert rc == 0
            if after == "rejected_call":
                A, r = _given_sets(name, row)["random"]
                s = cc.System(A, r, row)
                bad, _ = cc.with_pivot(s, int(s.rows[1]), -0.5)
                assert g.debug_reduced_solve(100.0, bad, r)[0] == -6
        g.solve(prm)
        its = g.iterations()
        for it in its:
            it.iteration_time_in_seconds = 0.0
        out.append(([bytes(it) for it in its], g.get_state()))
        g.close()
    assert len(out[0][0]) == 3
    assert out[0][0] == out[1][0] and all(np.array_equal(x, y) for x, y in zip(out[0][1], out[1][1]))
