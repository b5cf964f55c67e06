"""GPU (-m gpu): the side stream's packed schedule (OBVI_SIDE_PACKED, default on) against the schedule it replaces (OBVI_SIDE_PACKED=0).

Packed, the bounding-box factors of the STORE route (big problems and deterministic handles) are linearised by k_bbox_lin_dense -- 16 factors per 256-thread
workgroup, the lanes of a factor doing what they did in k_small_lin_lanes; the other families follow in a launch of their own.  On a deterministic handle nothing but the cost is added atomically on that route and the cost goes through the same partial-sum
slots, so the two schedules must agree bit for bit: the reduced system and the iteration records of a three-step solve, at the edges of a 16-factor workgroup.
On a default handle the sums are atomic: there the packed route is held to the oracle with the parity tests' tolerances (tests/test_gpu_parity.py), and the
far-pair blocks of k_schur_blocks (held to an 80-register allocation so that it fits beside the strip kernel's waves) to the long double reference of
tests/schur_cases.py, on the big-problem schedule where that kernel runs on the side stream."""
import functools

import numpy as np
import pytest

import helpers
import schur_cases as sc
import synth

pytestmark = pytest.mark.gpu

FACTOR_BBOX = 2
N_BB = (1, 15, 16, 17, 33)      # one factor; a workgroup one short, full, one over; two workgroups and a wavefront


@functools.lru_cache(maxsize=None)
def _base():
    prob = synth.make_problem(P=30, L=300, O=4, seed=23, object_classes=("bench",), bbox_noise=5.0, min_obj_obs=8)
    assert len(prob["bb_obj"]) >= max(N_BB) and len(prob["objects"]) >= 3
    return prob


@functools.lru_cache(maxsize=None)
def _case(n_bb, od):
    """n_bb bounding-box factors on two cameras with, from 15 factors on, every kind the kernel branches on; returns (problem, active mask, kinds per factor)"""
    prob = dict(_base())
    ext2 = synth.EXT_DEFAULT.copy(); ext2[5] = -0.12
    prob["K"], prob["ext"] = np.stack([synth.K_DEFAULT] * 2), np.stack([synth.EXT_DEFAULT, ext2])
    # factors of every object, round robin, so that a short list still has several objects; the last one is factor 0 again from the second camera
    by_obj = [list(np.flatnonzero(prob["bb_obj"] == o)) for o in range(len(prob["objects"]))]
    pick = [by_obj[o][k] for k in range(max(map(len, by_obj))) for o in range(len(by_obj)) if k < len(by_obj[o])][:max(1, n_bb - 1)]
    cam = np.zeros(len(pick), np.uint16)
    if n_bb > 1:
        pick.append(pick[0]); cam = np.append(cam, np.uint16(1))
    pick = np.array(pick)
    order = np.lexsort((cam, prob["bb_pose"][pick], prob["bb_obj"][pick]))
    pick, cam = pick[order], cam[order]
    for k in ("bb_obj", "bb_pose", "bb_corners", "bb_cov"):
        prob[k] = prob[k][pick].copy()
    prob["bb_cam"] = cam
    obj, pose = prob["bb_obj"].astype(int), prob["bb_pose"].astype(int)
    pose_const, object_const = prob["pose_const"].copy(), prob["object_const"].copy()
    objects = prob["objects"].copy()
    mask = np.ones(n_bb, np.uint8)
    if n_bb >= 15:
        # object 1 constant; the pose of its first factor constant as well (both constant); the pose of a factor of object 2 constant (constant pose only)
        object_const[1] = 1
        pose_const[pose[obj == 1][0]] = 1
        pose_const[pose[obj == 2][-1]] = 1
        mask[np.flatnonzero(obj == 2)[0]] = 0                                  # an inactive factor
        # the camera inside ellipsoid 0 as one of its frames sees it: the invalid-ellipse branch (xin <= 0) for that factor
        objects[0, 0:3] = prob["poses"][pose[obj == 0][0], 0:3]
        objects[0, 4:7] = 6.0
    prob.update(pose_const=pose_const, object_const=object_const, objects=objects)
    if od == 9:
        prob = synth.nine_dof(prob, tilt=0.3, seed=2)
    pc, oc = pose_const[pose] != 0, object_const[obj] != 0
    pairs = list(zip(obj, pose))
    kinds = dict(inactive=mask == 0, const_pose=pc & ~oc, const_object=oc & ~pc, both_const=pc & oc, twice=np.array([pairs.count(p) > 1 for p in pairs]))
    return prob, mask, kinds


def _handle(prob, mask, **options):
    g = helpers.product_ba(object_block_size=prob.get("object_block_size", 7), **options)
    synth.upload(g, prob)
    g.set_active_mask(FACTOR_BBOX, mask)
    return g


def _records(g):
    g.solve(helpers.ba_params(max_it=3, ftol=0.0, gtol=0.0, ptol=0.0))
    its = g.iterations()
    for it in its:
        it.iteration_time_in_seconds = 0.0          # wall time: the one field of a record that is no result
    return [bytes(it) for it in its]


@pytest.mark.parametrize("od", (7, 9))
@pytest.mark.parametrize("n_bb", N_BB)
def test_deterministic_handles_agree_bit_for_bit(n_bb, od, monkeypatch):
    prob, mask, kinds = _case(n_bb, od)
    out = {}
    for packed in ("1", "0"):
        monkeypatch.setenv("OBVI_SIDE_PACKED", packed)
        g = _handle(prob, mask, deterministic=True)
        if packed == "1" and n_bb >= 15:
            r = g.debug_linearize(FACTOR_BBOX)[0].reshape(n_bb, 4)
            kinds = dict(kinds, invalid=np.all(r == prob["bb_invalid"], axis=1))
            print(n_bb, od, {k: int(v.sum()) for k, v in kinds.items()})
            assert all(v.any() for v in kinds.values()), {k: int(v.sum()) for k, v in kinds.items()}
            assert not kinds["invalid"].all()
        S, b = g.debug_reduced_system(100.0)
        out[packed] = (S, b, _records(g), g.get_poses(), g.get_objects())
    (S1, b1, it1, p1, o1), (S0, b0, it0, p0, o0) = out["1"], out["0"]
    assert np.isfinite(S1).all() and np.abs(S1).max() > 0
    assert np.array_equal(S1, S0) and np.array_equal(b1, b0)
    assert len(it1) >= 2 and it1 == it0
    assert np.array_equal(p1, p0) and np.array_equal(o1, o0)


@pytest.fixture(scope="module")
def small():
    return synth.make_problem(P=30, L=400, O=3, seed=1, object_classes=("bench",), bbox_noise=5.0, min_obj_obs=5)


@pytest.fixture(scope="module")
def oracle_step(small):
    """the oracle's reduced system and its first LM step: computed once, shared, never modified"""
    o = helpers.oracle_ba(); synth.upload(o, small)
    So, bo = o.debug_reduced_system(100.0)
    so = o.solve(helpers.ba_params(max_it=1, ftol=0, ptol=0, gtol=0))
    return So, bo, so.final_cost, o.get_poses(), o.get_points(), o.get_objects(), o.iterations()[1]


@pytest.mark.parametrize("packed", ("1", "0"))
def test_default_handle_on_the_big_problem_schedule_follows_the_oracle(small, oracle_step, packed, monkeypatch):
    """the STORE route and the big-problem order of the side stream on a problem the oracle can follow: OBVI_SMALL_LANES_BELOW=1 sends the bounding boxes through
    the per-factor scratch, OBVI_FORK_EARLY_BELOW=0 forks the side stream behind the point pass.  Tolerances: tests/test_gpu_parity.py"""
    monkeypatch.setenv("OBVI_SIDE_PACKED", packed)
    monkeypatch.setenv("OBVI_SMALL_LANES_BELOW", "1")
    monkeypatch.setenv("OBVI_FORK_EARLY_BELOW", "0")
    So, bo, cost_o, poses_o, points_o, objects_o, io = oracle_step
    g = helpers.product_ba(); synth.upload(g, small)
    Sg, bg = g.debug_reduced_system(100.0)
    assert So.shape == Sg.shape
    assert helpers.rel_err(Sg, So) < 1e-11 and helpers.rel_err(bg, bo) < 1e-10
    sg = g.solve(helpers.ba_params(max_it=1, ftol=0, ptol=0, gtol=0))
    assert abs(sg.final_cost - cost_o) <= 1e-10 * cost_o
    for a, b in ((g.get_poses(), poses_o), (g.get_points(), points_o), (g.get_objects(), objects_o)):
        assert np.abs(a - b).max() < 1e-9
    ig = g.iterations()[1]
    assert abs(ig.step_norm - io.step_norm) <= 1e-9 * io.step_norm and abs(ig.relative_decrease - io.relative_decrease) < 1e-8


@functools.lru_cache(maxsize=None)
def _far_reference(radius):
    case = sc.strip_7()
    o = helpers.oracle_ba()
    synth.upload(o, case["prob"])
    return sc.reference(case["prob"], o, radius, case["mask0"], want_step=False)


@pytest.mark.parametrize("packed", ("1", "0"))
def test_far_pairs_on_the_side_stream(packed, monkeypatch):
    """strip_7 of tests/schur_cases.py (far blocks of 1, 16, 17, 64, 65 and 300 pairs; a diagonal block that only k_schur_blocks feeds) on the big-problem schedule,
    where k_schur_blocks runs on the side stream beside the strip kernel: entry by entry against the long
    double reference, within the case's bound"""
    monkeypatch.setenv("OBVI_SIDE_PACKED", packed)
    monkeypatch.setenv("OBVI_FORK_EARLY_BELOW", "0")
    case = sc.strip_7()
    g = helpers.product_ba()
    synth.upload(g, case["prob"])
    g.set_active_mask(0, case["mask0"])
    for radius in sc.RADII:
        ref = _far_reference(radius)
        S, b = g.debug_reduced_system(radius)
        eS, eb = sc.entry_error(S, ref["S"], ref["A_S"]), sc.entry_error(b, ref["b"], ref["A_b"])
        print("strip_7 packed=%s radius %g: e(S) = %.3g (bound %.3g), e(b) = %.3g (bound %.3g)" % (packed, radius, eS, sc.bound("strip_7", "S"), eb, sc.bound("strip_7", "b")))
        assert sc.exact_zeros(S, ref["S"]) and sc.exact_zeros(b, ref["b"])
        assert eS <= sc.bound("strip_7", "S") and eb <= sc.bound("strip_7", "b")
    assert g.problem_stats()["schur_pairs_blocks"] == case["predict"]["schur_pairs_blocks"] > 0
