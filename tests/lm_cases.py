"""Designed cases for the trust-region loop of obvi_ba_solve (obvi-slam_amd/csrc/lm.cpp), shared by tests/test_lm_reference.py (CPU: the cases against their
admission conditions, on the fp64 oracle and the extended-precision arbiter) and tests/test_gpu_lm_loop.py (the device loop against them).

Every case is a 12-pose problem (synth.make_problem(P=12, L=120, O=2, ...)) that solves in milliseconds and is aimed at one path through the loop's state
machine: the restore of the parked best iterate, a best iterate that stays parked over several accepted steps and is then superseded, a run of rejected
steps, the iteration cap on an accepted and on a rejected step, each tolerance exit, the monotone setting, the 9-parameter object block.

Admission (test_lm_reference.py asserts it; the conditions are on the inputs, the reference alone must meet them):
  * oracle and arbiter take the same (iteration, valid, successful) sequence and end alike
  * every valid step of both has |relative_decrease - 1e-3| >= 0.05: no accept / reject decision hangs on round-off
  * every comparison "candidate cost < minimum cost so far" has a relative gap of 1e-6 or more in both
  * a tolerance exit is a factor 2 clear on both sides: the same solve with the tolerance doubled and with it halved ends on the same tolerance after the
    same number of records, in both (tolerance_runs)
  * every depth is positive at the start and at every candidate the oracle evaluates, accepted or rejected (min_depth_visited; the oracle keeps them on request,
    oracle_ba_debug_keep_visited, since a solve hands back its best iterate only)
  * the case does not amplify beyond its own bound: with every feature coordinate moved one ulp up, and one ulp down, the oracle takes the same decisions and its
    records and returned state move by no more than half of bound() (input_sensitivity).  e(oracle) is one sample of how the case amplifies round-off; where
    a last-bit change of the input moves the reference further than that, the sample was a lucky one and a handle that sums with atomics, whose last bits
    change from run to run, lands outside 8 e(oracle) by chance

What the search behind the table found (seeds 1 .. 100, feature noise 0.2 .. 2 m, radii 1e3 .. 1e8): the problems of the generator's defaults (5 % outliers, no
parallax bound) take non-monotonic steps readily, but by walking single features along their viewing rays -- depths go negative (to -47 m on seed 4 at noise
0.3, radius 1e4) and oracle and arbiter end 1e-2 ... 1e4 m apart with step norms that differ by a factor.  The cases here therefore use features with 3 degrees of
parallax and, but for two, no outliers; among those the seeds below are the ones where oracle and arbiter stay 1e-6 or closer.  A case whose FIRST accepted step
stays the best for the rest of the solve was not found with positive depths: a first step that is never beaten is a divergence.  `parked_best` is the nearest
admitted shape: the best is parked at step 6, four accepted steps above it use the superseded best buffers as candidate buffers, step 11 is a new best and
rotates the buffers again, step 12 ends above it.

The minimum-radius exit has no case.  A radius small enough to reach 1e-32 gives a zero step, and the function-tolerance test |cost change| <= ftol * cost
fires first even at ftol = 0 (measured at an initial radius of 1e-30: "Function tolerance reached." after one record).

Invalid steps have no case here either: with a free gauge the oracle and the arbiter disagree on which pivot fails (free_gauge_problem), so the device is only
held to its own records there (tests/test_gpu_lm_loop.py, part E).

TABLE holds e(oracle), the oracle against the arbiter, per case: `records` is the largest relative difference over every record's cost, two gradient norms,
step norm, relative decrease and radius; `state` the largest absolute difference over the returned poses, points and objects.  bound() is the rule of
schur_cases, object_cases and cov_cases: 8 e(oracle), with the floors 1e-10 relative for records (tests/test_gpu_pose_lin_reuse.py) and
1e-9 for the state (the bar tests/test_gpu_end_state.py holds poses to)."""
import ctypes as C
import os
import subprocess

import numpy as np

import helpers
import obvi_ba
import synth

ARBITER_LIB = os.path.join(helpers.ROOT, "oracle", "libobvi_oracle_ld.so")
MIN_REL_DECREASE = 1e-3
FLOOR = dict(records=1e-10, state=1e-9)

# record fields, in the order of record()
ITERATION, VALID, SUCCESSFUL, COST, COST_CHANGE, GMAX, GNORM, STEP_NORM, REL_DECREASE, RADIUS = range(10)
COMPARED = (COST, GMAX, GNORM, STEP_NORM, REL_DECREASE, RADIUS)      # the fields of TABLE's `records` figure


def problem(seed, point_noise, parallax=3.0, outliers=0.0, const_poses=2):
    return synth.make_problem(P=12, L=120, O=2, seed=seed, const_poses=const_poses, min_obj_obs=3, point_noise=point_noise, min_parallax_deg=parallax,
                              outlier_frac=outliers)


def problem_nine(seed, point_noise):
    return synth.nine_dof(problem(seed, point_noise), tilt=0.2, seed=seed)


def generator_defaults(const_poses=2):
    """seed 3 with the generator's own outliers and no parallax bound: the tolerance exits, and (free gauge) the invalid steps"""
    return problem(3, 0.1, parallax=0.0, outliers=0.05, const_poses=const_poses)


def free_gauge_problem():
    """Part E of tests/test_gpu_lm_loop.py: no constant pose, so a large radius leaves the reduced system singular to round-off.  With the cap at 8 and a
    maximum radius of 1e30 the oracle takes AxrxrrrrA at a radius of 1e16 and the arbiter ArrrrrrrA; at 1e20 the oracle Axxxxx (FAILURE) and the arbiter
    Axxxxrrrr (tests/test_lm_reference.py::test_invalid_steps_are_decided_by_round_off holds the disagreement)."""
    return generator_defaults(const_poses=0)


FREE_GAUGE_RADII = (1e16, 1e18, 1e20)


def free_gauge_params(radius):
    return helpers.ba_params(max_it=8, ftol=0.0, gtol=0.0, ptol=0.0, radius=radius, max_radius=1e30)


def _case(build, cap, aim, od=7, exit_on=None, **params):
    p = dict(ftol=0.0, gtol=0.0, ptol=0.0)
    p.update(params)
    return dict(build=build, cap=cap, params=p, od=od, aim=aim, exit_on=exit_on)


# aim: what the case is for; reaches_its_aim() holds the reference to it
CASES = {
    # costs 28205.8 1401.8 447.57 428.40 428.66: step 4 is accepted above step 3
    "restore_best_4": _case(lambda: problem(16, 0.3), 4, dict(restore=True, nonmonotonic=1), radius=1e3, max_radius=1e3),
    # steps 5, 7 and 8 are accepted above the running minimum, the best is step 6
    "restore_best_8": _case(lambda: problem(59, 0.5), 8, dict(restore=True, nonmonotonic=3), radius=1e4, max_radius=1e4),
    "parked_best": _case(lambda: problem(59, 0.5), 12, dict(restore=True, nonmonotonic=5, parked=4, rotations=3), radius=1e4, max_radius=1e4),
    # step 2 is accepted above the minimum (3940 against 3170); the five steps tried from there cost six times as much and are refused, the radius falling
    # by 2, 4, 8, 16, 32; steps 8 and 9 are accepted with the divisor back at 2 and end above the minimum, so the best (step 1) is restored as well
    "rejected_run": _case(lambda: problem(93, 0.2, outliers=0.05), 9, dict(sequence="AAArrrrrAA"), radius=1e8, max_radius=1e16),
    "cap_on_reject": _case(lambda: problem(93, 0.2, outliers=0.05), 6, dict(sequence="AAArrrr"), radius=1e8, max_radius=1e16),
    "monotone": _case(lambda: problem(93, 0.2, outliers=0.05), 9, dict(sequence="AArrrrrrrA"), radius=1e8, max_radius=1e16, nonmono=False),
    # exactly four rejections: the radius goes down by 2, 4, 8, 16 and the next accepted step puts the divisor back
    "monotone_run_of_4": _case(lambda: problem(59, 0.5), 10, dict(sequence="AAAAArrrrAA"), radius=1e5, max_radius=1e5, nonmono=False),
    # Seed 82 converges fast enough for a tolerance to sit a factor 2 clear of two consecutive steps: |cost change| / cost falls 0.955 0.478 0.0169 8.2e-4
    # 7.1e-5 9.9e-6, the step norm 5.10 0.987 0.256 0.097 (|x| is 136), the largest gradient entry 7202 5670 1070 140 54.7.  Each tolerance is the geometric
    # mean of the two steps it separates.  (At the tolerances 1e-3 / 1e-3 / 1e-1 on seed 3 of the generator's defaults the parameter and gradient exits sit
    # between steps that differ by a factor 1.4: doubling the tolerance ends those solves two records earlier.)
    "ftol": _case(lambda: problem(82, 0.2), 30, dict(message="Function tolerance reached.", records=5), exit_on="ftol", ftol=2.4e-4, radius=1e4, max_radius=1e4),
    "ptol": _case(lambda: problem(82, 0.2), 30, dict(message="Parameter tolerance reached.", records=2), exit_on="ptol", ptol=1.65e-2, radius=1e4, max_radius=1e4),
    "gtol": _case(lambda: problem(82, 0.2), 30, dict(message="Gradient tolerance reached.", records=4), exit_on="gtol", gtol=387.0, radius=1e4, max_radius=1e4),
    # (the same problem at cap 6 meets every condition but the last: one ulp on the features moves the oracle's records by 3.4e-7, twelve times its e(oracle))
    "nine_dof": _case(lambda: problem_nine(36, 0.3), 5, dict(restore=True, nonmonotonic=2), od=9, radius=1e3, max_radius=1e3),
    # the problem part E of the GPU test goes back to after its invalid steps (free_gauge_problem with the first two poses constant), restore_best_4's parameters
    "after_invalid": _case(generator_defaults, 4, dict(sequence="AAAAA"), radius=1e3, max_radius=1e3),
}
NO_TOLERANCE_EXIT = tuple(n for n, c in CASES.items() if c["exit_on"] is None)
TOLERANCE_EXIT = tuple(n for n, c in CASES.items() if c["exit_on"] is not None)

# name: e(oracle), tests/test_lm_reference.py prints them and fails when they drift (measured <= TABLE <= 4 measured)
TABLE = {
    "restore_best_4": dict(records=8e-11, state=2e-13),
    "restore_best_8": dict(records=4.3e-09, state=4.7e-11),
    "parked_best": dict(records=1.7e-06, state=1.2e-07),
    "rejected_run": dict(records=0.0036, state=3.7e-12),        # (the worst field is the relative decrease of the refused steps; their cost changes agree to 3e-4)
    "cap_on_reject": dict(records=0.0027, state=3.7e-12),
    "monotone": dict(records=1.1e-09, state=2e-07),
    "monotone_run_of_4": dict(records=5.6e-11, state=6e-11),
    "ftol": dict(records=7.5e-11, state=7.3e-14),
    "ptol": dict(records=2.1e-13, state=7.8e-13),
    "gtol": dict(records=8.5e-12, state=1.1e-13),
    "nine_dof": dict(records=4.4e-08, state=2.1e-07),
    "after_invalid": dict(records=4.2e-11, state=6e-13),
}


def bound(name, what):
    return max(8.0 * TABLE[name][what], FLOOR[what])


def solver_params(case, cap=None, **override):
    p = dict(case["params"])
    p.update(override)
    return helpers.ba_params(max_it=case["cap"] if cap is None else cap, **p)


def arbiter_ba(**options):
    if not os.path.exists(ARBITER_LIB):
        subprocess.check_call(["make", "-C", os.path.join(helpers.ROOT, "oracle"), "arbiter"])
    return obvi_ba.BundleAdjuster(library=ARBITER_LIB, prefix="oracle_", **options)


def reference_ba(which, case):
    return (helpers.oracle_ba if which == "oracle" else arbiter_ba)(object_block_size=case["od"])


def record(i):
    return (i.iteration, i.step_is_valid, i.step_is_successful, i.cost, i.cost_change, i.gradient_max_norm, i.gradient_norm, i.step_norm, i.relative_decrease,
            i.trust_region_radius)


def summary(s):
    return dict(termination_type=s.termination_type, message=s.message.decode(), num_iterations=s.num_iterations, num_successful_steps=s.num_successful_steps,
                num_unsuccessful_steps=s.num_unsuccessful_steps, is_solution_usable=s.is_solution_usable, initial_cost=s.initial_cost, final_cost=s.final_cost,
                fixed_cost=s.fixed_cost)


SAME_IN_SUMMARY = ("termination_type", "message", "num_iterations", "num_successful_steps", "num_unsuccessful_steps", "is_solution_usable")


def run(ba, prm):
    """one solve on an uploaded handle: (summary dict, records, (poses, points, objects))"""
    s = ba.solve(prm)
    return summary(s), [record(i) for i in ba.iterations()], ba.get_state()


def solve_case(which, name, cap=None, **override):
    case = CASES[name]
    ba = reference_ba(which, case)
    synth.upload(ba, case["build"]())
    out = run(ba, solver_params(case, cap, **override))
    ba.close()
    return out


def sequence(records):
    """A accepted, r rejected, x invalid"""
    return "".join("A" if r[SUCCESSFUL] else "r" if r[VALID] else "x" for r in records)


def decisions(records):
    return [r[:3] for r in records]


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def record_error(a, b, fields=COMPARED):
    """largest relative difference of two record lists over `fields`"""
    assert len(a) == len(b)
    return max(rel(x[f], y[f]) for x, y in zip(a, b) for f in fields)


def state_error(a, b):
    return max(float(np.abs(x - y).max()) for x, y in zip(a, b) if x.size)


def same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def first_minimum(records, upto=None):
    """j(k): index of the first minimum of the costs of the successful records 0 .. upto"""
    recs = records if upto is None else records[:upto + 1]
    ok = [k for k, r in enumerate(recs) if r[SUCCESSFUL]]
    return min(ok, key=lambda k: (recs[k][COST], k))


def last_successful(records, upto=None):
    recs = records if upto is None else records[:upto + 1]
    return max(k for k, r in enumerate(recs) if r[SUCCESSFUL])


def nonmonotonic_steps(records):
    """indices of the accepted steps whose cost is not below the smallest cost before them"""
    out, low = [], records[0][COST]
    for k, r in enumerate(records[1:], 1):
        if r[SUCCESSFUL]:
            if r[COST] >= low:
                out.append(k)
            low = min(low, r[COST])
    return out


def decision_margin(records):
    """min over the valid steps of |relative_decrease - 1e-3|"""
    m = [abs(r[REL_DECREASE] - MIN_REL_DECREASE) for r in records[1:] if r[VALID]]
    return min(m) if m else float("inf")


def minimum_gap(records, fixed_cost):
    """min over the accepted steps of the relative gap between the new cost and the smallest cost before it (both without the fixed cost, as the loop compares them)"""
    gaps, low = [], records[0][COST] - fixed_cost
    for r in records[1:]:
        if r[SUCCESSFUL]:
            c = r[COST] - fixed_cost
            gaps.append(abs(c - low) / low)
            low = min(low, c)
    return min(gaps) if gaps else float("inf")


def reaches_its_aim(name, summ, records):
    """asserts that a run of the case (the reference's) goes where the case is aimed"""
    aim = CASES[name]["aim"]
    seq = sequence(records)
    if "sequence" in aim:
        assert seq == aim["sequence"], seq
        assert summ["message"] == "Maximum number of iterations reached."
    if "message" in aim:
        assert summ["message"] == aim["message"] and len(records) == aim["records"], (summ["message"], len(records))
        assert "r" not in seq and "x" not in seq
    if aim.get("restore"):
        assert summ["message"] == "Maximum number of iterations reached."
        assert first_minimum(records) < last_successful(records) == len(records) - 1, "the last accepted step must end above the minimum"
        assert records[-1][COST] > summ["final_cost"]
        assert len(nonmonotonic_steps(records)) >= aim["nonmonotonic"], nonmonotonic_steps(records)
    if "parked" in aim:
        # a best that stays parked while `parked` accepted steps above it use the superseded best buffers as candidate buffers, and is superseded later; and
        # the number of accepted steps that are the minimum so far (each of them re-arms the rotation)
        best = [first_minimum(records, k) for k in range(len(records))]
        assert any(sum(1 for k in range(j + 1, len(records)) if best[k] == j and records[k][SUCCESSFUL]) >= aim["parked"] and best[-1] > j for j in set(best)), best
        assert sum(1 for k in range(1, len(records)) if best[k] == k) >= aim["rotations"], best


def tolerance_runs(which, name):
    """[(message, number of records)] of the case as it is, with its tolerance doubled, and with it halved.  All three alike: no step before the last is within
    a factor 2 of the tolerance (or the doubled one would stop there), and the step that ends the solve is a factor 2 inside it (or the halved one would go on).
    The step that ends a solve on the function or parameter tolerance leaves no record, so its quantity cannot be read off; this way it need not be."""
    tol = CASES[name]["exit_on"]
    value = CASES[name]["params"][tol]
    out = []
    for factor in (1.0, 2.0, 0.5):
        s, r, _ = solve_case(which, name, **{tol: value * factor})
        out.append((s["message"], len(r)))
    return out


def input_sensitivity(name):
    """(records, state): how far the oracle's run of the case moves when every feature coordinate is moved by one ulp, the larger of up and down"""
    case = CASES[name]
    _, r0, x0 = solve_case("oracle", name)
    worst = [0.0, 0.0]
    for toward in (np.inf, -np.inf):
        prob = dict(case["build"]())
        prob["points"] = np.nextafter(prob["points"], toward)
        ba = reference_ba("oracle", case)
        synth.upload(ba, prob)
        _, r, x = run(ba, solver_params(case))
        ba.close()
        assert decisions(r) == decisions(r0)
        worst = [max(worst[0], record_error(r, r0)), max(worst[1], state_error(x, x0))]
    return tuple(worst)


def min_depth(prob, poses, points):
    d = np.inf
    for c in range(len(prob["K"])):
        m = prob["rp_cam"] == c
        if m.any():
            d = min(d, float(synth.project_points(poses[prob["rp_pose"][m]], points[prob["rp_point"][m]], prob["K"][c], prob["ext"][c])[1].min()))
    return d


def min_depth_visited(name):
    """smallest depth over the start and every candidate the oracle evaluates in the case's solve, accepted or rejected (the oracle's test hook
    oracle_ba_debug_keep_visited; the solve itself hands back the best iterate only)"""
    case = CASES[name]
    prob = case["build"]()
    ba = reference_ba("oracle", case)
    synth.upload(ba, prob)
    ba._fn("ba_debug_keep_visited")(ba._h, C.c_int32(1))
    ba.solve(solver_params(case))
    get = ba._fn("ba_debug_get_visited")
    d = min_depth(prob, prob["poses"], prob["points"])
    poses, points = np.zeros((ba.P, 6)), np.zeros((ba.L, 3))
    n = get(ba._h, C.c_int32(-1), None, None)
    assert n >= sum(1 for i in ba.iterations()[1:] if i.step_is_valid)      # (a step that ends the solve on a tolerance is evaluated and leaves no record)
    for k in range(n):
        get(ba._h, C.c_int32(k), poses.ctypes.data_as(C.POINTER(C.c_double)), points.ctypes.data_as(C.POINTER(C.c_double)))
        d = min(d, min_depth(prob, poses, points))
    ba.close()
    return d


# ------------------------------------------------------------------------------------------
# the trust-region bookkeeping, read off one solve's own records (part D of the GPU test; the CPU test runs it on the oracle's)
# ------------------------------------------------------------------------------------------
FAILURE_MESSAGE = "Number of consecutive invalid steps more than Solver::Options::max_num_consecutive_invalid_steps"


def ulps(a, b):
    return abs(a - b) / np.spacing(max(abs(a), abs(b)))


def check_bookkeeping(summ, records, max_radius):
    """LevenbergMarquardtStrategy and TrustRegionMinimizer's record keeping [Ceres-doc], with no reference: every rule is stated on the records themselves."""
    failed = summ["message"] == FAILURE_MESSAGE
    closing = records[-1] if failed else None           # the fifth invalid step running: recorded, not counted, the radius not shrunk any more
    recs = records[:-1] if failed else records
    assert summ["num_iterations"] == len(records)
    assert summ["num_successful_steps"] + summ["num_unsuccessful_steps"] == len(recs)
    assert summ["num_successful_steps"] == sum(r[SUCCESSFUL] for r in recs)
    assert [r[ITERATION] for r in records] == list(range(len(records)))
    assert recs[0][VALID] and recs[0][SUCCESSFUL]
    divisor, current = 2.0, recs[0]
    for prev, r in zip(recs, recs[1:]):
        what = "record %d" % r[ITERATION]
        if r[SUCCESSFUL]:
            assert r[VALID], what
            rho = r[REL_DECREASE]
            assert rho > MIN_REL_DECREASE, what
            want = min(max_radius, prev[RADIUS] / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
            assert ulps(r[RADIUS], want) <= 4, (what, r[RADIUS], want)
            # the trial cost that took the decision against the cost the next linearisation finds at the same point: two instantiations of the residuals
            assert rel(current[COST] - r[COST_CHANGE], r[COST]) <= 1e-10, (what, current[COST] - r[COST_CHANGE], r[COST])
            divisor, current = 2.0, r
            continue
        assert r[RADIUS] == prev[RADIUS] / divisor, (what, r[RADIUS], prev[RADIUS], divisor)
        divisor *= 2.0
        assert r[GMAX] == prev[GMAX] and r[GNORM] == prev[GNORM], what                         # bit for bit: nothing was linearised
        if r[VALID]:
            assert r[REL_DECREASE] <= MIN_REL_DECREASE, what
            assert rel(r[COST], current[COST] - r[COST_CHANGE]) <= 1e-12, (what, r[COST], current[COST], r[COST_CHANGE])   # the candidate's cost
        else:
            assert r[COST] == current[COST], what
    if failed:
        assert closing[VALID] == 0 and closing[SUCCESSFUL] == 0 and sequence(recs).endswith("xxxx") and summ["is_solution_usable"] == 0
        assert closing[COST] == current[COST] and closing[GMAX] == recs[-1][GMAX] and closing[GNORM] == recs[-1][GNORM] and closing[RADIUS] == recs[-1][RADIUS]
    else:
        assert not sequence(records).endswith("xxxxx") and summ["is_solution_usable"] == 1
    assert summ["final_cost"] == min(r[COST] for r in recs if r[SUCCESSFUL])
