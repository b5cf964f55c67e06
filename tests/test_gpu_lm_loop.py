"""GPU (-m gpu): the trust-region loop of obvi_ba_solve (obvi-slam_amd/csrc/lm.cpp) driven through every exit and buffer rotation on purpose, on the designed
cases of tests/lm_cases.py (12 poses: milliseconds per solve).  The loop is a state machine over device buffers -- current, candidate, best and entry sets
rotated by swap, the pose cache and the staged pose-side sums riding along on an accepted step -- and each exit leaves another buffer as the answer.

Handles, created as tests/test_gpu_pose_lin_reuse.py creates them (the knob is read at obvi_ba_create):
  default                  side stream; at 12 poses the pose pass is sliced, so of the two caches only the pose cache rotates
  deterministic            one stream, the staged sums on: d_lin / d_lin_c rotate as well
  deterministic_no_reuse   OBVI_POSE_LIN_REUSE=0: a pose pass in every step

A  the records and the returned state follow the oracle, within lm_cases.bound (8 e(oracle), e(oracle) measured against the extended-precision arbiter by
   tests/test_lm_reference.py)
B  the state handed back is the minimum-cost iterate: a run capped at k hands back what the run capped at j(k) hands back, j(k) the first minimum of the accepted
   costs up to k -- byte for byte on the deterministic handles, where for the restore cases this compares a run that restored its parked best with a run that
   ended on it
C  the next call on the handle starts from that state and from no cache of the solve: the debug system, a second solve and a third behind a mask change, against
   a fresh handle given the returned state
D  the trust-region bookkeeping, read off the device's own records (lm_cases.check_bookkeeping; no reference)
E  invalid steps by self-consistency only: with a free gauge, which pivot fails is round-off -- the oracle takes AxrxrrrrA at a radius of 1e16 where the arbiter
   takes ArrrrrrrA, and at 1e20 the oracle fails (Axxxxx) where the arbiter goes on (Axxxxrrrr); tests/test_lm_reference.py holds that disagreement -- so no fp64
   implementation can be held to another's sequence there.  A failed pivot is the solver's flagged numerical path (SC_CHOL_FAIL), not a device fault.
"""
import functools

import numpy as np
import pytest

import helpers
import lm_cases as lc
import obvi_ba
import synth

pytestmark = pytest.mark.gpu

KNOB = "OBVI_POSE_LIN_REUSE"
KINDS = ("default", "deterministic", "deterministic_no_reuse")
BAR = 1e-10           # the trial cost against the evaluate / linearisation instantiation of the residuals
CHECKED = lc.COMPARED + (lc.COST_CHANGE,)


def handle(monkeypatch, kind, od=7):
    if kind == "deterministic_no_reuse":
        monkeypatch.setenv(KNOB, "0")
    else:
        monkeypatch.delenv(KNOB, raising=False)
    ba = helpers.product_ba(deterministic=kind != "default", object_block_size=od)       # (the knobs are read here, once per handle)
    monkeypatch.delenv(KNOB, raising=False)
    return ba


@functools.lru_cache(maxsize=None)
def problem_of(name):
    return lc.CASES[name]["build"]()


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    return lc.solve_case("oracle", name)


def fresh(monkeypatch, kind, name, state=None):
    ba = handle(monkeypatch, kind, lc.CASES[name]["od"])
    synth.upload(ba, problem_of(name))
    if state is not None:
        ba.update_state(poses=state[0], points=state[1], objects=state[2])
    return ba


def device_run(monkeypatch, kind, name, cap=None):
    """one solve of the case on a fresh handle: (summary, records, state, cost of evaluate at the returned state)"""
    ba = fresh(monkeypatch, kind, name)
    s, r, x = lc.run(ba, lc.solver_params(lc.CASES[name], cap))
    cost = ba.evaluate(True, False)[0]
    ba.close()
    return s, r, x, cost


def within(a, b, bar, what):
    """two record lists: decisions equal, every compared field within `bar` relative"""
    assert lc.decisions(a) == lc.decisions(b), (what, lc.sequence(a), lc.sequence(b))
    worst = lc.record_error(a, b, CHECKED)
    print("%s: %s, worst field %.3g (bar %.3g)" % (what, lc.sequence(a), worst, bar))
    assert worst <= bar, (what, [(x, y) for x, y in zip(a, b) if lc.record_error([x], [y], CHECKED) > bar][0])


def same_bits(a, b, what, closing_gradient=False):
    """two record lists bit for bit; closing_gradient: the two gradient norms of the last record within 1e-10 instead"""
    assert len(a) == len(b), (what, lc.sequence(a), lc.sequence(b))
    for k, (x, y) in enumerate(zip(a, b)):
        if closing_gradient and k == len(a) - 1:
            keep = [f for f in range(len(x)) if f not in (lc.GMAX, lc.GNORM)]
            assert [x[f] for f in keep] == [y[f] for f in keep], (what, k, x, y)
            assert lc.rel(x[lc.GMAX], y[lc.GMAX]) <= BAR and lc.rel(x[lc.GNORM], y[lc.GNORM]) <= BAR, (what, k, x, y)
            if (x[lc.GMAX], x[lc.GNORM]) != (y[lc.GMAX], y[lc.GNORM]):
                print("%s: the closing record's gradient norms differ in their last bits (%.2e, %.2e)" % (what, lc.rel(x[lc.GMAX], y[lc.GMAX]), lc.rel(x[lc.GNORM], y[lc.GNORM])))
        else:
            assert x == y, (what, k, x, y)


# ---- A ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_records_and_state_follow_the_oracle(name, kind, monkeypatch):
    so, ro, xo = oracle_run(name)
    s, r, x, cost = device_run(monkeypatch, kind, name)
    print("%s / %s: %s, %r" % (name, kind, lc.sequence(r), s["message"]))
    for k in lc.SAME_IN_SUMMARY:
        assert s[k] == so[k], (k, s[k], so[k])
    within(r, ro, lc.bound(name, "records"), "records against the oracle's")
    err = lc.state_error(x, xo)
    print("state against the oracle's: %.3g (bar %.3g)" % (err, lc.bound(name, "state")))
    assert err <= lc.bound(name, "state")
    assert s["final_cost"] == min(q[lc.COST] for q in r)
    assert lc.rel(s["initial_cost"], so["initial_cost"]) <= lc.bound(name, "records") and lc.rel(s["final_cost"], so["final_cost"]) <= lc.bound(name, "records")
    lc.reaches_its_aim(name, s, r)


# ---- D ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_trust_region_bookkeeping_of_the_device_s_own_records(name, kind, monkeypatch):
    s, r, _, _ = device_run(monkeypatch, kind, name)
    lc.check_bookkeeping(s, r, lc.CASES[name]["params"].get("max_radius", 1e4))
    if "rrrr" in lc.sequence(r):       # spelled out once: four rejections divide the radius by 2, 4, 8, 16, and the accepted step behind them starts from 2 again
        k = lc.sequence(r).index("rrrr")
        assert [r[k + i - 1][lc.RADIUS] / r[k + i][lc.RADIUS] for i in range(4)] == [2.0, 4.0, 8.0, 16.0]


# ---- B ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(lc.NO_TOLERANCE_EXIT))
def test_the_state_handed_back_is_the_minimum_cost_iterate(name, kind, monkeypatch):
    case = lc.CASES[name]
    runs = [device_run(monkeypatch, kind, name, cap=k) for k in range(case["cap"] + 1)]
    full = runs[-1][1]
    assert len(full) == case["cap"] + 1
    restored = 0
    for k, (s, r, x, cost) in enumerate(runs):
        what = "%s / %s, cap %d" % (name, kind, k)
        j = lc.first_minimum(full, k)
        restored += j < lc.last_successful(full, k)
        assert s["message"] == "Maximum number of iterations reached." and len(r) == k + 1
        if kind == "default":
            within(r, full[:k + 1], lc.bound(name, "records"), what + ": records against the first of the full run")
            assert lc.first_minimum(r) == j
            err = lc.state_error(x, runs[j][2])
            assert err <= lc.bound(name, "state"), (what, j, err)
        else:
            # the closing submission of a capped run is linearisation-only (no Schur complement, no solve): the gradient norms it completes the last accepted
            # record with are held to 1e-10 against the full run's, which took them from a full step; everything else is bit for bit
            same_bits(r, full[:k + 1], what, closing_gradient=k < case["cap"] and r[-1][lc.SUCCESSFUL] and k > 0)
            assert lc.same_bytes(x, runs[j][2]), "%s: the state is not the state of the run capped at %d (differs by %.3g)" % (what, j, lc.state_error(x, runs[j][2]))
        assert s["final_cost"] == r[j][lc.COST]
        assert lc.rel(cost, s["final_cost"]) <= BAR, (what, cost, s["final_cost"])
    print("%s / %s: %s, %d of the %d runs restored a parked best" % (name, kind, lc.sequence(full), restored, len(runs)))
    if case["aim"].get("restore"):
        assert restored >= 1        # (so the byte comparison above cannot pass without the restore path)


# ---- C ------------------------------------------------------------------------------------------------------------------------------------------------
def _compare(kind, name, got, want, what):
    (s, r, x), (sw, rw, xw) = got, want
    if kind == "default":
        within(r, rw, lc.bound(name, "records"), what)
        assert lc.state_error(x, xw) <= lc.bound(name, "state"), what
    else:
        same_bits(r, rw, what)
        assert lc.same_bytes(x, xw), what
    for k in lc.SAME_IN_SUMMARY:
        assert s[k] == sw[k], (what, k)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["restore_best_4", "cap_on_reject", "rejected_run"])
def test_the_next_call_starts_from_the_returned_state_not_from_a_cache(name, kind, monkeypatch):
    case = lc.CASES[name]
    prob = problem_of(name)
    radius = case["params"]["radius"]
    two = lc.solver_params(case, cap=2)
    mask = np.ones(len(prob["rp_pose"]), np.uint8)
    mask[::3] = 0
    ba = fresh(monkeypatch, kind, name)
    s1, _, x1 = lc.run(ba, lc.solver_params(case))
    # (i) the debug system at the returned state
    S, b = ba.debug_reduced_system(radius, m_cap=256)
    ref = fresh(monkeypatch, kind, name, x1)
    Sr, br = ref.debug_reduced_system(radius, m_cap=256)
    assert S.shape == Sr.shape and S.shape[0] > 0
    if kind == "default":
        assert helpers.rel_err(S, Sr) <= lc.bound(name, "records") and helpers.rel_err(b, br) <= lc.bound(name, "records")
    else:
        assert S.tobytes() == Sr.tobytes() and b.tobytes() == br.tobytes(), (helpers.rel_err(S, Sr), helpers.rel_err(b, br))
    # (ii) a second solve
    got = lc.run(ba, two)
    want = lc.run(ref, two)
    ref.close()
    _compare(kind, name, got, want, "%s / %s: second solve" % (name, kind))
    assert lc.rel(got[0]["initial_cost"], s1["final_cost"]) <= BAR, (got[0]["initial_cost"], s1["final_cost"])
    # (iii) a third behind a mask change
    x2 = got[2]
    ba.set_active_mask(obvi_ba.FACTOR_REPROJECTION, mask)
    got = lc.run(ba, two)
    ba.close()
    ref = fresh(monkeypatch, kind, name, x2)
    ref.prepare()       # the symbolic plan of the full problem, as on the first handle: a mask set behind it keeps the plan (the masked factors add zeros), a mask
    #                     set in front of it gets a plan of its own, whose sums run in another order -- the same numbers to the last bits but not in them
    ref.set_active_mask(obvi_ba.FACTOR_REPROJECTION, mask)
    want = lc.run(ref, two)
    ref.close()
    _compare(kind, name, got, want, "%s / %s: third solve, every third reprojection off" % (name, kind))
    assert got[0]["initial_cost"] < s1["final_cost"]        # (the mask took effect)


# ---- E ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["default", "deterministic"])
@pytest.mark.parametrize("radius", lc.FREE_GAUGE_RADII)
def test_invalid_steps_by_self_consistency(radius, kind, monkeypatch):
    """No comparison with the oracle's sequence: measured on the CPU, the fp64 oracle and the extended-precision arbiter disagree on it (1e16: AxrxrrrrA against
    ArrrrrrrA; 1e18: Axxxxrrrr against Axxrrrrrr; 1e20: Axxxxx, a FAILURE, against Axxxxrrrr).  On the default handle the order of the atomic sums can move a
    pivot across zero from run to run as well, so there the minimum-cost iterate is checked by its cost alone; on the deterministic handle also by the bytes of
    the run capped at it."""
    prob = lc.free_gauge_problem()
    entry = (prob["poses"], prob["points"], prob["objects"])
    prm = lc.free_gauge_params(radius)
    ba = handle(monkeypatch, kind)
    synth.upload(ba, prob)
    s, r, x = lc.run(ba, prm)
    print("free gauge, radius %g, %s: %s, %r" % (radius, kind, lc.sequence(r), s["message"]))
    lc.check_bookkeeping(s, r, 1e30)
    if s["message"] == lc.FAILURE_MESSAGE:
        assert s["termination_type"] == obvi_ba.FAILURE and s["is_solution_usable"] == 0
        assert lc.same_bytes(x, entry)
    else:
        assert s["message"] == "Maximum number of iterations reached."
        j = lc.first_minimum(r)
        assert s["final_cost"] == r[j][lc.COST] and lc.rel(ba.evaluate(True, False)[0], s["final_cost"]) <= BAR
        if kind == "deterministic":
            short = handle(monkeypatch, kind)
            synth.upload(short, prob)
            sj, rj, xj = lc.run(short, helpers.ba_params(max_it=j, ftol=0.0, gtol=0.0, ptol=0.0, radius=radius, max_radius=1e30))
            short.close()
            same_bits(rj, r[:j + 1], "the run capped at %d" % j, closing_gradient=j > 0)
            assert lc.same_bytes(x, xj)
    # the handle afterwards: the gauge fixed, the uploaded values again -- the records of a fresh handle on that problem
    name = "after_invalid"
    pc = prob["pose_const"].copy()
    pc[:2] = 1
    ba.set_const_flags(pose_const=pc)
    ba.update_state(poses=entry[0], points=entry[1], objects=entry[2])
    got = lc.run(ba, lc.solver_params(lc.CASES[name]))
    ba.close()
    ref = fresh(monkeypatch, kind, name)
    want = lc.run(ref, lc.solver_params(lc.CASES[name]))
    ref.close()
    _compare(kind, name, got, want, "the handle after the invalid steps")
