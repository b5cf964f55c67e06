"""GPU (-m gpu): the pose side of the reprojection linearisation staged by the trial cost (lm.cpp, cost_lin_block in ba_kernels.hip).

Where the pose pass runs one workgroup per pose -- more than 256 poses, or a deterministic handle -- the trial-cost launch of a step leaves the 27 sums per
pose of the candidate, an accepted step hands them to the next one, and a rejected or invalid step keeps the set it had: the pose pass itself runs in the
first step of a solve only.  OBVI_POSE_LIN_REUSE=0 (read at obvi_ba_create) restores the schedule with a pose pass in every step; that schedule is the
reference of every comparison here, on the two smallest shapes that reach the two kernel forms:
  * a default handle of 260 poses (just over the slicing bound: the plain loop, side stream), with constant poses and constant features
  * a deterministic handle of 12 poses (the two-round loop, one stream)
Bars: 1e-10 relative wherever both schedules start a step from the same values -- the staged sums are the pose pass's own
arithmetic in the same order, only the trial cost comes from another instantiation of the residual; from the second step on, on the default handle, the
spread tests/test_gpu_parity.py::test_config3_follows_the_oracle_for_two_steps allows between two fp64 realisations of a step (cost 1e-2, same decision).
"""
import numpy as np
import pytest

import helpers
import obvi_ba
import synth

pytestmark = pytest.mark.gpu

KNOB = "OBVI_POSE_LIN_REUSE"
BAR = 1e-10


def big_problem():
    """260 poses (the pose pass is unsliced above 256), 3000 features, 4 objects; the first three poses and every 17th feature constant."""
    prob = synth.make_well_posed(synth.make_problem(P=260, L=3000, O=4, seed=21, const_poses=3, min_obj_obs=5, object_classes=("bench",), bbox_noise=5.0))
    prob["point_const"] = prob["point_const"].copy()
    prob["point_const"][::17] = 1
    return prob


def small_problem(point_noise=0.1):
    return synth.make_problem(P=12, L=240, O=2, seed=3, const_poses=2, min_obj_obs=3, point_noise=point_noise)


@pytest.fixture(scope="module")
def big():
    return big_problem()


@pytest.fixture(scope="module")
def small():
    return small_problem()


def handle(monkeypatch, reuse, deterministic):
    if reuse:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, "0")
    ba = helpers.product_ba(deterministic=deterministic)       # (the knobs are read here, once per handle)
    monkeypatch.delenv(KNOB, raising=False)
    return ba


def records(ba):
    return [(i.iteration, i.step_is_valid, i.step_is_successful, i.cost, i.gradient_max_norm, i.gradient_norm, i.step_norm, i.relative_decrease, i.trust_region_radius)
            for i in ba.iterations()]


def solve(monkeypatch, prob, prm, reuse, deterministic):
    ba = handle(monkeypatch, reuse, deterministic)
    synth.upload(ba, prob)
    ba.solve(prm)
    out = records(ba), ba.get_poses()
    ba.close()
    return out


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def same_record(a, b, bar, what):
    """decisions equal; cost, both gradient norms and the radius within `bar`"""
    worst = max(rel(a[3], b[3]), rel(a[4], b[4]), rel(a[5], b[5]), rel(a[8], b[8]))
    print("%s: cost %.2e gmax %.2e |g| %.2e radius %.2e" % (what, rel(a[3], b[3]), rel(a[4], b[4]), rel(a[5], b[5]), rel(a[8], b[8])))
    assert a[:3] == b[:3], (what, a, b)
    assert worst <= bar, (what, a, b)


SHAPES = [("big", False), ("small", True)]


@pytest.mark.parametrize("name,deterministic", SHAPES)
def test_one_iteration(name, deterministic, big, small, monkeypatch):
    """One LM step and the linearisation-only submission behind it: the candidate's cost and the accept flag of the old schedule, and -- an accepted step --
    the gradient of the new point, which the new route takes from the staged sums."""
    prob = big if name == "big" else small
    prm = helpers.ba_params(max_it=1, ftol=0.0, gtol=0.0, ptol=0.0)
    new, _ = solve(monkeypatch, prob, prm, True, deterministic)
    old, _ = solve(monkeypatch, prob, prm, False, deterministic)
    assert len(new) == len(old) == 2 and old[1][2] == 1     # (the step of these starts is accepted: the staged set is used)
    same_record(new[0], old[0], BAR, name + " start")
    same_record(new[1], old[1], BAR, name + " step 1")


@pytest.mark.parametrize("name,deterministic", SHAPES)
def test_three_iterations(name, deterministic, big, small, monkeypatch):
    prob = big if name == "big" else small
    prm = helpers.ba_params(max_it=3, ftol=0.0, gtol=0.0, ptol=0.0)
    new, pn = solve(monkeypatch, prob, prm, True, deterministic)
    old, po = solve(monkeypatch, prob, prm, False, deterministic)
    assert len(new) == len(old) == 4
    same_record(new[0], old[0], BAR, name + " start")
    same_record(new[1], old[1], BAR, name + " step 1")
    for k in (2, 3):
        print("%s step %d: cost %.2e" % (name, k, rel(new[k][3], old[k][3])))
        assert new[k][:3] == old[k][:3] and rel(new[k][3], old[k][3]) <= 1e-2
    if deterministic:
        # one stream and fixed-order sums on both schedules: what separates them is the last digit of the trial costs, so every step holds the bar
        for k in (2, 3):
            same_record(new[k], old[k], BAR, name + " step %d" % k)
        assert np.abs(pn - po).max() <= 1e-9


def test_deterministic_handle_is_bit_identical_from_run_to_run(small, monkeypatch):
    prm = helpers.ba_params(max_it=6, ftol=0.0, gtol=0.0, ptol=0.0)
    a, pa = solve(monkeypatch, small, prm, True, True)
    b, pb = solve(monkeypatch, small, prm, True, True)
    assert a == b and np.array_equal(pa, pb)


def test_rejected_steps_keep_the_staged_set(monkeypatch):
    """12 poses, feature noise 0.5 m, initial radius 1e6 (close to Gauss-Newton): the CPU oracle rejects steps 1 and 2 and accepts from step 3 on.  The new
    route runs no pose pass in the steps behind a rejected one; its records are the old schedule's."""
    prob = small_problem(point_noise=0.5)
    prm = helpers.ba_params(max_it=6, ftol=0.0, gtol=0.0, ptol=0.0, radius=1e6, max_radius=1e16)
    o = helpers.oracle_ba()
    synth.upload(o, prob)
    o.solve(prm)
    decisions = [i.step_is_successful for i in o.iterations()]
    assert decisions == [1, 0, 0, 1, 1, 1, 1]
    new, pn = solve(monkeypatch, prob, prm, True, True)
    old, po = solve(monkeypatch, prob, prm, False, True)
    assert [r[2] for r in old] == decisions and len(new) == len(old)
    for k, (a, b) in enumerate(zip(new, old)):
        same_record(a, b, BAR, "step %d" % k)
    assert np.abs(pn - po).max() <= 1e-9


def _mask(ba, prob):
    m = np.ones(len(prob["rp_pose"]), np.uint8)
    m[::3] = 0
    ba.set_active_mask(obvi_ba.FACTOR_REPROJECTION, m)


def _points(ba, prob):
    ba.update_points(prob["points"] + 0.02 * np.sin(np.arange(3 * len(prob["points"]), dtype=np.float64)).reshape(-1, 3))


def _flags(ba, prob):
    pc = prob["pose_const"].copy()
    pc[5:9] = 1
    ba.set_const_flags(pose_const=pc)


@pytest.mark.parametrize("change", [_mask, _points, _flags], ids=["set_active_mask", "update_points", "set_const_flags"])
@pytest.mark.parametrize("name,deterministic", SHAPES)
def test_a_second_solve_does_not_use_sums_staged_by_the_first(name, deterministic, change, big, small, monkeypatch):
    """Two solves on one handle with the problem changed between them (and the values put back to the upload's, so that both schedules start alike): the second
    linearises at its own start -- the records of the old schedule's second solve, not sums of the first solve's last point, mask or flags."""
    prob = big if name == "big" else small
    prm = helpers.ba_params(max_it=2, ftol=0.0, gtol=0.0, ptol=0.0)
    out = []
    for reuse in (True, False):
        ba = handle(monkeypatch, reuse, deterministic)
        synth.upload(ba, prob)
        ba.solve(prm)
        ba.update_state(poses=prob["poses"], points=prob["points"], objects=prob["objects"])      # both schedules start the second solve from the same values
        change(ba, prob)
        ba.solve(prm)
        out.append(records(ba))
        ba.close()
    new, old = out
    assert len(new) == len(old) == 3
    same_record(new[0], old[0], BAR, name + " second solve, start")
    same_record(new[1], old[1], BAR, name + " second solve, step 1")
