"""The designed LM-loop cases of tests/lm_cases.py on the CPU: the fp64 oracle and the extended-precision arbiter (oracle/libobvi_oracle_ld.so) must meet the
admission conditions stated there by themselves, each case must go where it is aimed, and e(oracle) -- the oracle against the arbiter, from which the bounds of
tests/test_gpu_lm_loop.py derive -- is measured and held against lm_cases.TABLE so that a stale table fails.  The record-keeping rules the GPU test reads off
the device's records (lm_cases.check_bookkeeping) are run on the oracle's records here, which is the check of the checker."""
import functools

import numpy as np
import pytest

import lm_cases as lc
import synth


@functools.lru_cache(maxsize=None)
def both(name):
    return lc.solve_case("oracle", name), lc.solve_case("arbiter", name)


@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_case_meets_the_admission_conditions(name):
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63
    (so, ro, _), (sa, ra, _) = both(name)
    print("%s: oracle %s, arbiter %s, %r" % (name, lc.sequence(ro), lc.sequence(ra), so["message"]))
    assert lc.decisions(ro) == lc.decisions(ra)
    for k in lc.SAME_IN_SUMMARY:
        assert so[k] == sa[k], k
    for s, r in ((so, ro), (sa, ra)):
        margin, gap = lc.decision_margin(r), lc.minimum_gap(r, s["fixed_cost"])
        print("   margin of the decisions %.3g, gap of the minimum comparisons %.3g" % (margin, gap))
        assert margin >= 0.05 and gap >= 1e-6
    if lc.CASES[name]["exit_on"]:
        for which in ("oracle", "arbiter"):
            runs = lc.tolerance_runs(which, name)
            print("   %s: as it is, tolerance doubled, halved: %r" % (which, runs))
            assert runs[0] == runs[1] == runs[2] == (lc.CASES[name]["aim"]["message"], lc.CASES[name]["aim"]["records"])
    moved = lc.input_sensitivity(name)
    print("   one ulp on the features moves the oracle's records by %.3g and its state by %.3g" % moved)
    assert moved[0] <= 0.5 * lc.bound(name, "records") and moved[1] <= 0.5 * lc.bound(name, "state")
    depth = lc.min_depth_visited(name)
    print("   smallest depth over every point the oracle evaluates: %.3g" % depth)
    assert depth > 0.0


@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_case_reaches_what_it_is_aimed_at(name):
    for s, r, _ in both(name):
        lc.reaches_its_aim(name, s, r)
        lc.check_bookkeeping(s, r, lc.CASES[name]["params"].get("max_radius", 1e4))


@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_e_oracle_is_what_the_table_says(name):
    (so, ro, xo), (sa, ra, xa) = both(name)
    e = dict(records=lc.record_error(ro, ra), state=lc.state_error(xo, xa))
    print("e(oracle) %s: records %.3g, state %.3g" % (name, e["records"], e["state"]))
    for what, v in e.items():
        t = lc.TABLE[name][what]
        assert v <= t <= 4.0 * max(v, 2.0 ** -60), "lm_cases.TABLE[%r][%r] = %.3g, measured %.3g: measure again and update the table" % (name, what, t, v)
    assert lc.rel(so["final_cost"], sa["final_cost"]) <= lc.bound(name, "records")


def test_every_cap_below_a_case_s_cap_is_a_prefix_of_it():
    """Part B of the GPU test solves every case with the cap at 0 .. cap and takes the run at cap j(k) for the iterate a run at cap k must hand back: on the
    oracle the records of a shorter run are the first records of the longer one bit for bit, and the state handed back at cap k is the state handed back at
    cap j(k), byte for byte -- the reference has the property the device is held to."""
    for name in ("restore_best_4", "cap_on_reject"):
        _, full, _ = both(name)[0]
        states = []
        for k in range(len(full)):
            _, r, x = lc.solve_case("oracle", name, cap=k)
            assert r == full[:k + 1]
            states.append(x)
        for k in range(len(full)):
            assert lc.same_bytes(states[k], states[lc.first_minimum(full, k)]), k


def test_invalid_steps_are_decided_by_round_off():
    """Why part E of the GPU test compares the device with nothing but itself: with a free gauge the oracle and the arbiter -- the same source in two
    precisions -- take different sequences, at a radius of 1e16 and at 1e20 (where one of them ends in FAILURE and the other does not).  Both keep their
    books by the rules (check_bookkeeping), and a FAILURE hands the entry state back."""
    prob = lc.free_gauge_problem()
    fixed = lc.CASES["after_invalid"]["build"]()      # the same problem with the first two poses constant: what the GPU test turns the handle into afterwards
    assert all(np.array_equal(prob[k], fixed[k]) for k in prob if k != "pose_const") and fixed["pose_const"].tolist() == [1, 1] + [0] * 10
    seqs = {}
    for radius in lc.FREE_GAUGE_RADII:
        for which in ("oracle", "arbiter"):
            ba = lc.reference_ba(which, dict(od=7))
            synth.upload(ba, prob)
            s, r, x = lc.run(ba, lc.free_gauge_params(radius))
            ba.close()
            seqs[radius, which] = lc.sequence(r)
            lc.check_bookkeeping(s, r, 1e30)
            if s["message"] == lc.FAILURE_MESSAGE:
                assert lc.same_bytes(x, (prob["poses"], prob["points"], prob["objects"]))
        print("radius %g: oracle %s, arbiter %s" % (radius, seqs[radius, "oracle"], seqs[radius, "arbiter"]))
    assert any("x" in s for s in seqs.values())
    assert seqs[1e16, "oracle"] != seqs[1e16, "arbiter"] and seqs[1e20, "oracle"] != seqs[1e20, "arbiter"]
