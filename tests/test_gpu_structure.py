"""Ragged observation structures through the HIP path, checked against the oracle (reduced system + one LM step):
tracks longer than a wavefront, tracks with gaps, loop closures (pairs far outside the Schur strip), three observations of a
point from one pose, points and poses without observations."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers
import obvi_ba
import synth
from test_gpu_map_pair_priors import product, spd

pytestmark = pytest.mark.gpu


def _extra_observations(prob, point, poses, cam=0, rng=None):
    """append observations of `point` from `poses` (pixels from the ground truth + noise); pixels far outside the image are fine"""
    rng = rng or np.random.default_rng(0)
    poses = np.asarray(poses, dtype=np.int64)
    px, depth = synth.project_points(prob["gt_poses"][poses], np.repeat(prob["gt_points"][point][None, :], len(poses), axis=0))
    keep = depth > 0.1
    poses, px = poses[keep], px[keep] + rng.normal(size=(keep.sum(), 2))
    n = len(poses)
    prob["rp_pose"] = np.concatenate([prob["rp_pose"], poses.astype(prob["rp_pose"].dtype)])
    prob["rp_point"] = np.concatenate([prob["rp_point"], np.full(n, point, dtype=prob["rp_point"].dtype)])
    prob["rp_cam"] = np.concatenate([prob["rp_cam"], np.full(n, cam, dtype=prob["rp_cam"].dtype)])
    prob["rp_pixel"] = np.concatenate([prob["rp_pixel"], px])
    if np.ndim(prob["rp_sigma"]) > 0:
        prob["rp_sigma"] = np.concatenate([prob["rp_sigma"], np.full(n, prob["rp_sigma"][0])])
    if "rp_is_outlier" in prob:
        prob["rp_is_outlier"] = np.concatenate([prob["rp_is_outlier"], np.zeros(n, dtype=prob["rp_is_outlier"].dtype)])
    return n


def _ragged_problem():
    prob = synth.make_problem(P=120, L=500, O=2, seed=5, object_classes=("bench",), bbox_noise=5.0, min_obj_obs=5, outlier_frac=0.0)
    P = len(prob["poses"])
    seen = {(int(p), int(l)) for p, l in zip(prob["rp_pose"], prob["rp_point"])}

    def unseen(point, poses):
        return [p for p in poses if (p, point) not in seen]
    added = 0
    added += _extra_observations(prob, 3, unseen(3, range(1, 100)))                 # > 64 observations: per-point kernel, far pairs
    added += _extra_observations(prob, 7, unseen(7, [5, 6, 9, 30, 31, 90, 118]))   # gaps + loop closures
    added += _extra_observations(prob, 11, unseen(11, [2, 119]))                    # a single far pair
    p0 = int(prob["rp_pose"][prob["rp_point"] == 20][0])
    added += _extra_observations(prob, 20, [p0, p0])                                # three observations from one pose
    assert added > 80
    # a point and a pose nobody observes
    keep = (prob["rp_point"] != 33) & (prob["rp_pose"] != 60)
    for k in ("rp_pose", "rp_point", "rp_cam", "rp_pixel", "rp_sigma", "rp_is_outlier"):
        if k in prob and np.ndim(prob[k]) > 0:
            prob[k] = prob[k][keep]
    return prob


def test_ragged_structures_match_oracle():
    prob = _ragged_problem()
    o, g = helpers.oracle_ba(), helpers.product_ba()
    for ba in (o, g):
        synth.upload(ba, prob)
    assert abs(g.evaluate(True, False)[0] - o.evaluate(True, False)[0]) <= 1e-12 * o.evaluate(True, False)[0]
    for radius in (100.0, 1e4):
        So, bo = o.debug_reduced_system(radius)
        Sg, bg = g.debug_reduced_system(radius)
        assert So.shape == Sg.shape
        assert helpers.rel_err(Sg, So) < 1e-11 and helpers.rel_err(bg, bo) < 1e-10
    prm = helpers.ba_params(max_it=3, ftol=0, ptol=0, gtol=0)
    so, sg = o.solve(prm), g.solve(prm)
    assert sg.num_iterations == so.num_iterations
    for a, b in zip(o.iterations(), g.iterations()):
        assert a.step_is_successful == b.step_is_successful and abs(a.cost - b.cost) <= 1e-9 * a.cost
    assert np.abs(g.get_poses() - o.get_poses()).max() < 1e-7
    assert np.abs(g.get_points() - o.get_points()).max() < 1e-6


def test_ragged_structures_with_a_stereo_rig():
    """second camera on every frame of a few tracks + gaps: the two-layer (stereo) path of the Schur strip kernel"""
    prob = synth.make_problem(P=60, L=300, O=0, seed=9, stereo=True, outlier_frac=0.0)
    keep = ~((prob["rp_point"] % 7 == 0) & (prob["rp_pose"] % 5 == 2))               # punch holes into every 7th track
    for k in ("rp_pose", "rp_point", "rp_cam", "rp_pixel", "rp_sigma", "rp_is_outlier"):
        if k in prob and np.ndim(prob[k]) > 0:
            prob[k] = prob[k][keep]
    o, g = helpers.oracle_ba(), helpers.product_ba()
    for ba in (o, g):
        synth.upload(ba, prob)
    So, bo = o.debug_reduced_system(100.0)
    Sg, bg = g.debug_reduced_system(100.0)
    assert helpers.rel_err(Sg, So) < 1e-11 and helpers.rel_err(bg, bo) < 1e-10


@pytest.mark.parametrize("which", ["ragged", "stereo", "window"])
def test_slot_tables_filled_on_the_device_equal_the_hosts(which, monkeypatch):
    """Round 5: the slot tables of the Schur strip kernel (per visit four words, per 144-byte slot its source) are filled on the device, one lane per visit
    (plan_kernels.hip); the host only deals the visits to batches.  OBVI_PLAN_SLOTS_ON_HOST=1 is the host's own fill of rounds 1-4.  Same tables, hence --
    on deterministic handles -- bit-identical reduced systems and LM runs: gaps, loop closures, tracks over 64 sightings, three sightings from one frame,
    unobserved blocks (ragged), two records per frame (stereo: the second layer), and an ordinary window with objects."""
    if which == "ragged":
        prob = _ragged_problem()
    elif which == "stereo":
        prob = synth.make_problem(P=60, L=300, O=0, seed=9, stereo=True, outlier_frac=0.0)
        keep = ~((prob["rp_point"] % 7 == 0) & (prob["rp_pose"] % 5 == 2))
        for k in ("rp_pose", "rp_point", "rp_cam", "rp_pixel", "rp_sigma", "rp_is_outlier"):
            if k in prob and np.ndim(prob[k]) > 0:
                prob[k] = prob[k][keep]
    else:
        prob = synth.make_problem(P=130, L=9000, O=6, seed=21, const_poses=5, min_obj_obs=8)
    out = []
    for on_host in ("1", "0"):
        monkeypatch.setenv("OBVI_PLAN_SLOTS_ON_HOST", on_host)
        g = helpers.product_ba(deterministic=True)
        synth.upload(g, prob)
        S, b = g.debug_reduced_system(100.0)
        s = g.solve(helpers.ba_params(max_it=3, ftol=0, ptol=0, gtol=0))
        # a mask change keeps the plan (prepare_masks): the tables must serve the masked problem as well
        mask = np.ones(len(prob["rp_pose"]), np.uint8); mask[::9] = 0
        g.set_active_mask(0, mask)
        s2 = g.solve(helpers.ba_params(max_it=2, ftol=0, ptol=0, gtol=0))
        out.append((S, b, [(i.cost, i.step_norm, i.step_is_successful) for i in g.iterations()], s.final_cost, s2.final_cost, g.get_poses(), g.problem_stats()))
        g.close()
    (S0, b0, it0, f0, m0, p0, st0), (S1, b1, it1, f1, m1, p1, st1) = out
    assert st0 == st1 and np.array_equal(S0, S1) and np.array_equal(b0, b1)
    assert it0 == it1 and f0 == f1 and m0 == m1 and np.array_equal(p0, p1)


@pytest.mark.parametrize("knobs", [
    {"OBVI_PRE_MAX": "0"},                                   # every diagonal product is an update job: the signal / wait path of k_update_potrf
    {"OBVI_PRE_MAX": "8"},                                   # ... all of them applied by the potrf workgroups
    {"OBVI_SLICE_MAX": "0"},                                 # no level is row-sliced
    {"OBVI_SLICE_MAX": "1000000"},                           # every level is
    {"OBVI_ND_BALANCE": "0", "OBVI_ND_LEAF": "96"},          # the unbalanced dissection of the earlier builds
    {"OBVI_ND_LEAF": "16", "OBVI_ND_G": "1"},                # a deep tree of tiny leaves
    {"OBVI_SCHUR_WGS": "16", "OBVI_UPD_CHUNK": "1"},
    {"OBVI_SMALL_LANES_BELOW": "0"},                         # bounding boxes through the scratch + gather kernels of big problems (no atomics)
    {"OBVI_SMALL_LANES_BELOW": "1000000"},                   # ... through the one-launch atomic path of sliding windows
    {"OBVI_PAIR_BITMAP_MAX": "0"},                           # tile marks pair by pair (the path of more than 8192 variable poses)
    {"OBVI_SMALL_LANES_BELOW": "0"},                         # thread-per-factor small-factor kernels (the big-problem path) on a small problem
    {"OBVI_SMALL_LANES_BELOW": "1000000000", "OBVI_HOST_THREADS": "3"},   # ... 16 lanes per factor; symbolic phase on three host threads
    {"OBVI_BACKWARD_LEVELS": "1"},                           # backward substitution: one level per launch, nobody walks a chain
    {"OBVI_BACKWARD_LEVELS": "8", "OBVI_ND_LEAF": "16", "OBVI_ND_G": "1"},   # ... chains of seven ancestors in a deep tree (ragged: not every ancestor tile exists)
    {"OBVI_BACKWARD_LEVELS": "3", "OBVI_FUSED_POTRF": "0"},  # ... and the two-launch forward schedule
    {"OBVI_CHOL_XCD": "0", "OBVI_SLICE_MAX": "0"},           # no XCD placement of the wide levels' jobs (with every level wide)
    {"OBVI_CHOL_XCD": "1", "OBVI_SLICE_MAX": "0"},           # ... with it
    {"OBVI_BACKSUB_LANES": "1"},                             # back-substitution: a lane per feature
    {"OBVI_BACKSUB_LANES": "32"},                            # ... 32 lanes per feature (most of them beyond the feature's last sighting)
    {"OBVI_PLAN_SLOTS_ON_HOST": "1"},                        # the strip kernel's slot tables filled by the host (rounds 1-4) instead of by plan_kernels.hip
])
def test_schedule_knobs_change_round_off_only(knobs, monkeypatch):
    """The elimination order and the launch schedule are free choices (exact factorisation): whatever the tuning knobs say, a step
    is the oracle's step."""
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    prob = synth.make_problem(P=260, L=4000, O=8, seed=11, bbox_noise=5.0, object_classes=("bench",))
    o, g = helpers.oracle_ba(), helpers.product_ba()
    for ba in (o, g):
        synth.upload(ba, prob)
    prm = helpers.ba_params(max_it=2, ftol=0, ptol=0, gtol=0)
    so, sg = o.solve(prm), g.solve(prm)
    assert sg.num_iterations == so.num_iterations
    assert abs(sg.final_cost - so.final_cost) <= 1e-8 * so.final_cost
    assert np.abs(g.get_poses() - o.get_poses()).max() < 1e-7


@pytest.mark.parametrize("case", [
    dict(pose_noise=1.0, seed=5, max_it=12, unique_pairs=True, flags="AAAAAAArAAAAA", tol_after=1e-3, tol_final=1e-3, tol_poses=1e-2),    # ONE failed step (relative decrease -0.04) in the middle of the run
    dict(pose_noise=2.0, seed=6, max_it=5, unique_pairs=True, flags="AAAArr", tol_after=None, tol_final=1e-5, tol_poses=1e-6),           # the run ENDS in two failed steps (-0.16, -6.8): the state handed back is the last accepted one
    dict(pose_noise=1.0, seed=5, max_it=10, unique_pairs=False, flags="AAAAAAAAAAA", tol_after=None, tol_final=1e-4, tol_poses=1e-2)])   # two boxes on one (object, pose) pair (no failed step in this one)
def test_big_problem_schedule_on_a_small_problem_through_accepted_and_rejected_steps(case, monkeypatch):
    """The schedule of the big problems (side stream forked BEHIND the point pass, bounding-box factors through the per-factor scratch and
    the gather: OBVI_FORK_EARLY_BELOW=0, OBVI_SMALL_LANES_BELOW=0) on a problem the oracle can follow, started a metre or two off so that
    steps fail: the oracle's accept / reject sequence, its costs to 1e-4 up to the first failed step and to 1e-3 behind it.  (A step fails
    where the quadratic model is poor, and there the outcome amplifies round-off: the oracle and its own extended-precision build
    (oracle/libobvi_oracle_ld.so) agree to 1e-9 before such a step, to 4e-5 behind the one of the first case and differ by 0.3 in the
    relative decrease of the second case's last step.  The cases were picked on those two builds so that no decision is a close call.)"""
    monkeypatch.setenv("OBVI_FORK_EARLY_BELOW", "0")
    monkeypatch.setenv("OBVI_SMALL_LANES_BELOW", "0")
    prob = synth.make_problem(P=120, L=2500, O=6, seed=29, bbox_noise=5.0, object_classes=("bench", "chair"), min_obj_obs=6)
    prob["poses"] = prob["poses"] + case["pose_noise"] * np.random.default_rng(case["seed"]).normal(size=prob["poses"].shape) * np.array([1, 1, 1, 0.3, 0.3, 0.3])
    if not case["unique_pairs"]:      # their off-diagonal blocks meet on the same tile entries
        dup = np.arange(0, len(prob["bb_obj"]), 4)
        for k in ("bb_obj", "bb_pose", "bb_cam", "bb_cov"):
            prob[k] = np.concatenate([prob[k], prob[k][dup]])
        prob["bb_corners"] = np.concatenate([prob["bb_corners"], prob["bb_corners"][dup] + 2.0])
    o, g = helpers.oracle_ba(), helpers.product_ba()
    for ba in (o, g):
        synth.upload(ba, prob)
    prm = helpers.ba_params(max_it=case["max_it"], ftol=0, ptol=0, gtol=0, nonmono=False)
    so, sg = o.solve(prm), g.solve(prm)
    io, ig = o.iterations(), g.iterations()
    flags = "".join("A" if i.step_is_successful else "r" for i in io)
    assert flags == case["flags"] and "".join("A" if i.step_is_successful else "r" for i in ig) == flags
    assert all(abs(i.relative_decrease) > 0.03 for i in io[1:])                              # none of the decisions is a close call
    first = flags.index("r") if "r" in flags else len(flags)
    rel = [abs(a.cost - b.cost) / b.cost for a, b in zip(ig, io)]
    assert max(rel[:first]) < 1e-4 and max(abs(a.trust_region_radius - b.trust_region_radius) / b.trust_region_radius for a, b in zip(ig[:first], io[:first])) < 1e-4
    for k in range(first, len(flags)):
        if flags[k] == "r":                                                                   # a failed step shrinks the region
            assert ig[k].trust_region_radius < 0.6 * ig[k - 1].trust_region_radius
    if case["tol_after"] is not None:
        assert max(rel) < case["tol_after"]
    assert abs(sg.final_cost - so.final_cost) <= case["tol_final"] * so.final_cost and np.abs(g.get_poses() - o.get_poses()).max() < case["tol_poses"]


@pytest.mark.parametrize("below", ["0", "1000000"])
def test_an_object_seen_twice_from_one_frame(below, monkeypatch):
    """Two bounding-box factors on the same (object, pose) pair (two detections / two cameras): their off-diagonal blocks land on
    the same tile entries.  Both small-factor paths (scratch + gather with plain stores when every pair is unique, atomics
    otherwise; the one-launch atomic path) must give the oracle's reduced system and step."""
    monkeypatch.setenv("OBVI_SMALL_LANES_BELOW", below)
    prob = synth.make_problem(P=40, L=400, O=3, seed=21, object_classes=("bench",), bbox_noise=5.0, min_obj_obs=5)
    dup = np.arange(0, len(prob["bb_obj"]), 3)
    rng = np.random.default_rng(3)
    for k in ("bb_obj", "bb_pose", "bb_cam", "bb_cov"):
        prob[k] = np.concatenate([prob[k], prob[k][dup]])
    prob["bb_corners"] = np.concatenate([prob["bb_corners"], prob["bb_corners"][dup] + rng.normal(size=(len(dup), 4)) * 3.0])
    o, g = helpers.oracle_ba(), helpers.product_ba()
    for ba in (o, g):
        synth.upload(ba, prob)
    So, bo = o.debug_reduced_system(100.0)
    Sg, bg = g.debug_reduced_system(100.0)
    assert helpers.rel_err(Sg, So) < 1e-11 and helpers.rel_err(bg, bo) < 1e-10
    prm = helpers.ba_params(max_it=3, ftol=0, ptol=0, gtol=0)
    so, sg = o.solve(prm), g.solve(prm)
    assert abs(sg.final_cost - so.final_cost) <= 1e-9 * so.final_cost and np.abs(g.get_objects() - o.get_objects()).max() < 1e-8


def test_symbolic_plan_survives_a_mask_change():
    """Phase II of a window re-solves the phase-I problem minus the excluded factors (offline_problem_runner.h:803-892).  The library
    keeps the symbolic plan when the new masks select a subset of what it was built for: masked observations contribute zero
    records, features that lose all their sightings drop out, the rows of an object that loses all its boxes become padding.  Same
    result as a handle whose plan was built for the masked problem, and as the oracle; re-enabling everything rebuilds the plan."""
    prob = synth.make_problem(P=130, L=3000, O=6, seed=17, object_classes=("bench",), bbox_noise=5.0, min_obj_obs=6)
    rng = np.random.default_rng(4)
    m_rp = (rng.uniform(size=len(prob["rp_pose"])) > 0.12).astype(np.uint8)
    gone = rng.choice(len(prob["points"]), 40, replace=False)
    m_rp[np.isin(prob["rp_point"], gone)] = 0                       # these features lose every sighting
    left = np.bincount(prob["rp_point"], weights=m_rp, minlength=len(prob["points"]))
    m_rp[left[prob["rp_point"]] < 3] = 0                            # ... and so do features left with fewer than 3 (as the min-observation filter would)
    gone = np.flatnonzero(np.bincount(prob["rp_point"], weights=m_rp, minlength=len(prob["points"])) == 0)
    m_bb = (rng.uniform(size=len(prob["bb_obj"])) > 0.1).astype(np.uint8)
    m_bb[prob["bb_obj"] == 2] = 0                                   # object 2 loses every box ...
    m_sp = np.ones(len(prob["sp_obj"]), np.uint8); m_sp[prob["sp_obj"] == 2] = 0   # ... and its shape prior: it drops out of the problem
    prm = helpers.ba_params(max_it=6, ftol=0, gtol=0, ptol=0)

    def masked(ba, build_plan_first):
        synth.upload(ba, prob)
        if build_plan_first:
            ba.snapshot(); ba.solve(helpers.ba_params(max_it=2)); ba.restore()       # a full plan and a solve on it, as phase I does
        ba.set_active_mask(0, m_rp); ba.set_active_mask(2, m_bb); ba.set_active_mask(3, m_sp)
        s = ba.solve(prm)
        return s, ba.get_poses(), ba.get_objects(), ba.get_points()
    g1, g2, o = helpers.product_ba(), helpers.product_ba(), helpers.oracle_ba()
    (s1, p1, o1, x1), (s2, p2, o2, x2), (so, po, oo, xo) = masked(g1, True), masked(g2, False), masked(o, False)
    assert s1.num_parameters_reduced == s2.num_parameters_reduced == so.num_parameters_reduced
    assert s1.num_residuals_reduced == s2.num_residuals_reduced == so.num_residuals_reduced and s1.reduced_system_size == s2.reduced_system_size
    assert g1.problem_stats()["chol_levels"] >= g2.problem_stats()["chol_levels"]       # g1 still runs the plan of the full problem
    for s, p, ob, x in ((s1, p1, o1, x1), (s2, p2, o2, x2)):
        assert s.num_iterations == so.num_iterations and abs(s.initial_cost - so.initial_cost) <= 1e-11 * so.initial_cost
        assert abs(s.final_cost - so.final_cost) <= 1e-8 * so.final_cost
        assert np.abs(p - po).max() < 1e-7 and np.abs(ob - oo).max() < 1e-7 and np.abs(x - xo).max() < 1e-6
    assert np.array_equal(o1[2], prob["objects"][2]) and np.array_equal(x1[gone], prob["points"][gone])     # dropped blocks do not move
    # covariance blocks on the kept plan: the dropped object's block is zero, the others equal the rebuilt plan's
    c1, c2 = g1.object_covariances(np.arange(6)), g2.object_covariances(np.arange(6))
    assert np.all(c1[2] == 0.0) and np.abs(c1 - c2).max() <= 1e-7 * np.abs(c2).max()
    # back to all factors: not a subset of the masked state's plan for g2 -> rebuilt; g1's plan still fits
    for ba in (g1, g2, o):
        ba.set_poses(prob["poses"], prob["pose_const"]); ba.set_points(prob["points"], prob["point_const"]); ba.set_objects(prob["objects"], prob["object_const"])
        for t in (0, 2, 3):
            ba.set_active_mask(t, None)
    sa, sb, sc = g1.solve(prm), g2.solve(prm), o.solve(prm)
    assert abs(sa.final_cost - sc.final_cost) <= 1e-8 * sc.final_cost and abs(sb.final_cost - sc.final_cost) <= 1e-8 * sc.final_cost


def test_blocks_or_cameras_re_uploaded_after_the_factors():
    """The ABI states no call order, so the library must cope with one: a later set_poses / set_points / set_objects with FEWER
    blocks than the factors refer to is an error at the next evaluate / solve (OBVI_ERR_OUT_OF_RANGE = -4, nothing read out of
    bounds), and a later set_cameras re-derives what the bounding-box factors baked from the intrinsics."""
    prob = synth.make_problem(P=30, L=200, O=2, seed=5, object_classes=("bench",), bbox_noise=5.0, min_obj_obs=5)
    g = helpers.product_ba(); synth.upload(g, prob)
    c0 = g.evaluate(True, False)[0]
    for setter, arr, flags in ((g.set_poses, prob["poses"][:10], prob["pose_const"][:10]), (g.set_points, prob["points"][:50], prob["point_const"][:50]),
                               (g.set_objects, prob["objects"][:1], prob["object_const"][:1])):
        setter(np.ascontiguousarray(arr), flags)
        with pytest.raises(obvi_ba.ObviError, match="status -4"):
            g.evaluate(True, False)
        with pytest.raises(obvi_ba.ObviError, match="status -4"):
            g.solve(helpers.ba_params(max_it=2))
        g.set_poses(prob["poses"], prob["pose_const"]); g.set_points(prob["points"], prob["point_const"]); g.set_objects(prob["objects"], prob["object_const"])
        assert abs(g.evaluate(True, False)[0] - c0) <= 1e-13 * c0     # the handle is intact once the blocks are back (sums are atomic: order-dependent round-off)
    # shared-object flags given for another object count
    g.set_shared_objects(np.ones(2, np.uint8), 0, 1)
    g.set_objects(np.concatenate([prob["objects"], prob["objects"][:1]]), np.zeros(3, np.uint8))
    with pytest.raises(obvi_ba.ObviError, match="status -4"):
        g.evaluate(True, False)
    g.set_objects(prob["objects"], prob["object_const"]); g.set_shared_objects(None, 0, 1)
    # cameras after the bounding boxes: same as a fresh upload with those cameras
    K2 = prob["K"].copy(); K2[:, 0] *= 1.1; K2[:, 1] *= 0.9; K2[:, 2] += 7.0
    g.set_cameras(K2, prob["ext"])
    fresh = helpers.product_ba(); p2 = dict(prob); p2["K"] = K2; synth.upload(fresh, p2)
    cg, rg, _ = g.evaluate(True); cf, rf, _ = fresh.evaluate(True)
    assert abs(cg - cf) <= 1e-13 * cf and np.array_equal(rg, rf) and abs(cg - c0) > 1e-3 * c0
    o = helpers.oracle_ba(); synth.upload(o, p2)
    assert abs(o.evaluate(True, False)[0] - cg) <= 1e-12 * cg


def test_uploads_outlive_their_source_buffers_and_the_staging_arena_wraps():
    """Uploads are copied through a pinned arena of the handle and enqueued from there without waiting (host_util.h: StagingArena), so
    (1) the caller may overwrite its buffer the moment a set_* call returns, and (2) a long run of uploads with no solve in between
    fills the 16 MB arena: the copy that no longer fits goes the plain way, the call synchronises, the arena starts over.  Each
    upload here carries its own serial number; whatever is read back must be the last one."""
    g = helpers.product_ba()
    n = 40000                                           # 0.96 MB per upload: the arena is full after 17 of them
    buf = np.empty((n, 3))
    for k in range(60):
        buf[:] = k                                      # same buffer, new contents: the previous upload must not see them
        g.set_points(buf, None)
    assert np.array_equal(g.get_points(), np.full((n, 3), 59.0))
    for k in range(60, 100):                            # update_points: the other raw copy of the ABI
        buf[:] = k
        g.update_points(buf)
    assert np.array_equal(g.get_points(), np.full((n, 3), 99.0))
    big = np.arange(3 * 400000, dtype=np.float64).reshape(-1, 3)   # 9.6 MB: above the per-copy limit of the arena, straight from the caller
    g.set_points(big, None)
    big_copy = big.copy(); big[:] = -1.0
    assert np.array_equal(g.get_points(), big_copy)


def test_reprojection_upload_forms_scalar_sigma_default_camera_empty_and_reused_buffers():
    """obvi_ba_set_reproj takes sigma as an array or as one number, camera indices as an array or not at all (camera 0), and n = 0; the
    arrays only the device reads go up in the caller's order and a kernel permutes them (k_reproj_gather), so the caller's buffers are
    free the moment the call returns.  All forms of the same problem evaluate to the same residuals, bit for bit; the oracle agrees."""
    prob = synth.make_problem(P=30, L=900, O=3, seed=23, bbox_noise=2.0)
    prob["rp_cam"] = np.zeros_like(prob["rp_cam"]); prob["rp_sigma"] = np.full(len(prob["rp_pose"]), 1.75)
    g = helpers.product_ba(); synth.upload(g, prob)
    c0, r0, q0 = g.evaluate(True)
    o = helpers.oracle_ba(); synth.upload(o, prob)
    assert abs(o.evaluate(True, False)[0] - c0) <= 1e-12 * c0
    # one sigma for all, no camera indices
    g.set_reproj(prob["rp_pose"], prob["rp_point"], None, prob["rp_pixel"], 1.75, prob["rp_huber"])
    c1, r1, q1 = g.evaluate(True)
    assert abs(c1 - c0) <= 1e-13 * c0 and np.array_equal(r1, r0) and np.array_equal(q1, q0)   # (the cost is a sum of atomics: last bits)
    # the caller scribbles over its buffers right behind the call
    pose, point, cam = prob["rp_pose"].copy(), prob["rp_point"].copy(), prob["rp_cam"].copy()
    pix, sig = prob["rp_pixel"].copy(), prob["rp_sigma"].copy()
    g.set_reproj(pose, point, cam, pix, sig, prob["rp_huber"])
    pix[:] = -1e9; sig[:] = 1e-9; cam[:] = 0
    c2, r2, _ = g.evaluate(True)
    assert abs(c2 - c0) <= 1e-13 * c0 and np.array_equal(r2, r0)
    # a shuffled factor order is the same problem: residuals come back in the caller's order
    perm = np.random.default_rng(5).permutation(len(pose))
    g.set_reproj(prob["rp_pose"][perm], prob["rp_point"][perm], prob["rp_cam"][perm], prob["rp_pixel"][perm], prob["rp_sigma"][perm], prob["rp_huber"])
    c3, r3, _ = g.evaluate(True)
    n2 = 2 * len(pose)
    assert abs(c3 - c0) <= 1e-13 * c0 and np.array_equal(r3[:n2].reshape(-1, 2), r0[:n2].reshape(-1, 2)[perm])
    # no reprojection factors at all
    g.set_reproj(pose[:0], point[:0], None, pix[:0], 1.0, prob["rp_huber"])
    c4, r4, _ = g.evaluate(True)
    assert len(r4) == len(r0) - n2 and 0.0 < c4 < c0
    s = g.solve(helpers.ba_params(max_it=3))
    assert s.final_cost <= s.initial_cost


def test_two_launch_schedule_of_the_tile_cholesky(monkeypatch):
    """OBVI_FUSED_POTRF=0: update jobs of a level and the potrf of the next level as two launches (nothing waits inside a launch);
    same steps as the fused schedule and as the oracle.  The knob is read once per process, so this runs in a child process."""
    import subprocess, sys, textwrap
    code = textwrap.dedent("""
        import sys, numpy as np
        sys.path[:0] = [%r, %r]
        import helpers, synth
        prob = synth.make_problem(P=260, L=4000, O=8, seed=11, bbox_noise=5.0, object_classes=("bench",))
        o, g = helpers.oracle_ba(), helpers.product_ba()
        for ba in (o, g):
            synth.upload(ba, prob)
        prm = helpers.ba_params(max_it=3, ftol=0, ptol=0, gtol=0)
        so, sg = o.solve(prm), g.solve(prm)
        assert sg.num_iterations == so.num_iterations and abs(sg.final_cost - so.final_cost) <= 1e-8 * so.final_cost, (sg.final_cost, so.final_cost)
        assert np.abs(g.get_poses() - o.get_poses()).max() < 1e-7
        assert g.problem_stats()["chol_levels"] > 3
        print("two-launch ok")
    """) % (os.path.join(helpers.ROOT, "obvi-slam_amd", "python"), os.path.join(helpers.ROOT, "tests"))
    env = dict(os.environ, OBVI_FUSED_POTRF="0")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "two-launch ok" in out.stdout, out.stdout + out.stderr


def test_non_finite_input_is_a_failed_solve_and_the_handle_survives():
    """A NaN observation poisons cost, gradient and the reduced system: every step is invalid (non-finite step / failed factorisation),
    the solve stops after max_num_consecutive_invalid_steps like the oracle's, the parameters are left untouched, and the same
    handle then solves the clean problem to the oracle's result (nothing non-finite survives in the device buffers)."""
    prob = synth.make_problem(P=40, L=200, O=2, seed=3, outlier_frac=0.0, object_classes=("bench",))
    bad = dict(prob); bad["rp_pixel"] = prob["rp_pixel"].copy(); bad["rp_pixel"][5, 0] = np.nan
    o, g = helpers.oracle_ba(), helpers.product_ba()
    for ba in (o, g):
        synth.upload(ba, bad)
    prm = helpers.ba_params(max_it=8)
    so, sg = o.solve(prm), g.solve(prm)
    assert sg.termination_type == so.termination_type and sg.message == so.message and sg.num_iterations == so.num_iterations
    assert b"invalid steps" in sg.message
    assert [it.step_is_valid for it in g.iterations()] == [it.step_is_valid for it in o.iterations()]
    assert np.array_equal(g.get_poses(), prob["poses"]) and np.array_equal(g.get_points(), prob["points"])
    assert sg.is_solution_usable == 0 and sg.num_successful_steps == so.num_successful_steps == 1 and sg.num_unsuccessful_steps == so.num_unsuccessful_steps
    for ba in (o, g):
        synth.upload(ba, prob)
    so, sg = o.solve(prm), g.solve(prm)
    assert sg.num_iterations == so.num_iterations and np.isfinite(sg.final_cost)
    assert abs(sg.final_cost - so.final_cost) <= 1e-9 * so.final_cost
    assert np.abs(g.get_poses() - o.get_poses()).max() < 1e-8


def test_get_state_reads_what_the_three_getters_read():
    """obvi_ba_get_state (one wait, copies through the handle's pinned arena) against obvi_ba_get_poses / _points / _objects, after an
    upload and after a solve; on a problem whose points do not fit the arena any more (16 MB) the copies go straight out."""
    for P, L in ((40, 600), (60, 800000)):
        prob = synth.make_problem(P=P, L=L, O=4 if L < 10000 else 0, seed=3, bbox_noise=5.0, object_classes=("bench",), min_obj_obs=5)
        g = helpers.product_ba()
        synth.upload(g, prob)
        for solved in (False, True):
            if solved:
                if L > 10000:
                    break
                g.solve(helpers.ba_params(max_it=3))
            po, pt, ob = g.get_state()
            assert np.array_equal(po, g.get_poses()) and np.array_equal(pt, g.get_points()) and np.array_equal(ob, g.get_objects())
            if not solved:
                assert np.array_equal(po, prob["poses"]) and np.array_equal(pt, prob["points"])


def test_a_window_planned_ahead_and_given_its_values_later():
    """obvi_ba_prepare + obvi_ba_update_state: a window is uploaded with PLACEHOLDER values and planned while another handle solves on another host thread (what
    the host mirror's runner does beside a window's last solve); the start values arrive afterwards.  The symbolic phase reads no value, so the solve is the one of
    a handle that was given the values at upload -- bit for bit in deterministic mode -- and the oracle's; the first solve does not run the symbolic phase again."""
    import threading
    prob = synth.make_problem(P=50, L=3000, O=5, seed=23, object_classes=("bench",), bbox_noise=5.0, min_obj_obs=6)
    other = synth.make_problem(P=60, L=4000, O=3, seed=24, object_classes=("bench",), bbox_noise=5.0, min_obj_obs=6)
    prm = helpers.ba_params(max_it=8, ftol=0, gtol=0, ptol=0)
    rng = np.random.default_rng(1)
    placeholder = dict(prob)
    placeholder["poses"] = prob["poses"] + rng.normal(scale=0.3, size=prob["poses"].shape)
    placeholder["points"] = prob["points"] + rng.normal(scale=1.0, size=prob["points"].shape)
    placeholder["objects"] = prob["objects"] + rng.normal(scale=0.2, size=prob["objects"].shape) * (np.arange(7) != 3)
    for det in (True, False):
        plain, ahead, busy = helpers.product_ba(deterministic=det), helpers.product_ba(deterministic=det), helpers.product_ba(deterministic=det)
        synth.upload(plain, prob)
        s_plain = plain.solve(prm)
        synth.upload(busy, other)
        errors = []

        def plan():
            try:
                synth.upload(ahead, placeholder)
                ahead.prepare()
            except Exception as e:   # noqa: BLE001 -- reported by the main thread
                errors.append(e)
        t = threading.Thread(target=plan)
        t.start()
        s_busy = busy.solve(helpers.ba_params(max_it=30, ftol=0, gtol=0, ptol=0))
        t.join()
        assert not errors, errors
        assert s_busy.num_iterations >= 30 or s_busy.termination_type >= 0
        levels = ahead.problem_stats()["chol_levels"]
        assert levels == plain.problem_stats()["chol_levels"] and levels > 0          # the plan exists before any solve
        ahead.update_state(prob["poses"], prob["points"], prob["objects"])
        assert np.array_equal(ahead.get_poses(), prob["poses"]) and np.array_equal(ahead.get_points(), prob["points"]) and np.array_equal(ahead.get_objects(), prob["objects"])
        s_ahead = ahead.solve(prm)
        assert s_ahead.num_iterations == s_plain.num_iterations
        if det:
            assert s_ahead.final_cost == s_plain.final_cost and np.array_equal(ahead.get_poses(), plain.get_poses()) and np.array_equal(ahead.get_points(), plain.get_points())
        else:
            assert abs(s_ahead.final_cost - s_plain.final_cost) <= 1e-9 * s_plain.final_cost and np.abs(ahead.get_poses() - plain.get_poses()).max() < 1e-7
        # one kind of block only; the others stay
        points_before = ahead.get_points()
        ahead.update_state(poses=placeholder["poses"])
        assert np.array_equal(ahead.get_poses(), placeholder["poses"]) and np.array_equal(ahead.get_points(), points_before)
    o = helpers.oracle_ba()
    synth.upload(o, placeholder); o.prepare(); o.update_state(prob["poses"], prob["points"], prob["objects"])
    so = o.solve(prm)
    assert so.num_iterations == s_plain.num_iterations and abs(so.final_cost - s_plain.final_cost) <= 1e-8 * so.final_cost


def test_update_state_and_prepare_refuse_what_they_cannot_do():
    g = helpers.product_ba()
    g.prepare()                                                                      # the empty problem is a problem (as for obvi_ba_solve)
    prob = synth.make_problem(P=20, L=300, O=0, seed=2)
    synth.upload(g, prob)
    with pytest.raises(ValueError):
        g.update_state(points=prob["points"][:-1])                                   # (the binding checks the count: the ABI takes the counts as uploaded)
    g.snapshot()
    g.update_state(points=prob["points"] + 1.0)
    with pytest.raises(obvi_ba.ObviError):
        g.restore()                                                                  # the snapshot was dropped with the values it belonged to
    assert np.array_equal(g.get_points(), prob["points"] + 1.0) and np.array_equal(g.get_poses(), prob["poses"])


# factor type -> factors of the problem below, in the order obvi_ba_evaluate lays the families out
SEVEN_FAMILIES = {obvi_ba.FACTOR_REPROJECTION: 37, obvi_ba.FACTOR_BBOX: 5, obvi_ba.FACTOR_SHAPE_PRIOR: 3, obvi_ba.FACTOR_LTM_PRIOR: 2, obvi_ba.FACTOR_REL_POSE: 5,
                  obvi_ba.FACTOR_MAP_PAIR_PRIOR: 2, obvi_ba.FACTOR_MAP_GROUP_PRIOR: 2}
SEVEN_GROUPS = ([0, 2, 4], [5])


def _seven_families(od):
    """6 poses, 40 features, 6 objects and every factor family at once, none of the counts a multiple of 4 or 64: 37 observations, 5 boxes, 3 shape priors,
    2 LTM priors, 5 relative poses, 2 map pair priors, map group priors of 3 and 1 members (no pair inside a group); a different Huber width per family."""
    prob = synth.make_problem(P=6, L=40, O=6, seed=7, object_classes=("bench",), bbox_noise=5.0, min_obj_obs=3, outlier_frac=0.0)
    rng = np.random.default_rng(31)
    keep = np.sort(rng.choice(len(prob["rp_pose"]), 37, replace=False))
    for k in ("rp_pose", "rp_point", "rp_cam", "rp_pixel", "rp_is_outlier"):
        prob[k] = prob[k][keep]
    keep = np.sort(rng.choice(len(prob["bb_obj"]), 5, replace=False))
    for k in ("bb_obj", "bb_pose", "bb_cam", "bb_corners", "bb_cov"):
        prob[k] = prob[k][keep]
    for k in ("sp_obj", "sp_mean", "sp_cov"):
        prob[k] = prob[k][[1, 3, 4]]
    prob.update(lt_obj=np.array([5, 2], np.uint32), lt_mean=prob["objects"][[5, 2]] + rng.normal(scale=0.05, size=(2, 7)),
                lt_cov=np.stack([spd(rng, 7), spd(rng, 7)]).reshape(2, 49))
    prob.update(rp_huber=1.25, bb_huber=0.5, sp_huber=10.0, lt_huber=3.0, rl_huber=0.75)
    if od == 9:
        prob = synth.nine_dof(prob, tilt=0.3, seed=2)
    obj = prob["objects"]
    a, b = np.array([0, 2], np.uint32), np.array([1, 3], np.uint32)
    pairs = dict(a=a, b=b, mean_a=obj[a] - rng.normal(scale=0.1, size=(2, od)), mean_b=obj[b] - rng.normal(scale=0.1, size=(2, od)),
                 cov=np.stack([spd(rng, 2 * od), spd(rng, 2 * od)]), huber=2.0)
    groups = dict(groups=[list(g) for g in SEVEN_GROUPS], means=[obj[list(g)] - rng.normal(scale=0.1, size=(len(g), od)) for g in SEVEN_GROUPS],
                  covs=[spd(rng, od * len(g)) for g in SEVEN_GROUPS], huber=1.5)
    ba = product(prob)
    ba.set_map_pair_priors(pairs["a"], pairs["b"], pairs["mean_a"], pairs["mean_b"], pairs["cov"], None, pairs["huber"])
    ba.set_map_group_priors(groups["groups"], groups["means"], groups["covs"], groups["huber"])
    return ba


@pytest.mark.parametrize("od", [7, 9])
def test_seven_factor_families_in_one_evaluate_layout(od):
    """Every factor family on one handle: counts, the evaluate layout (norms and residual rows family after family: reprojection, boxes, shape priors, LTM
    priors, relative poses, map pair priors, map group priors), outlier selection per family on its own segment of the norms, and masks that take out one
    factor and nothing else.  The un-robustified residuals of a family are also what obvi_ba_debug_linearize computes for it in another kernel: the same
    fp64 formula, and a block norm sums at most 27 squares here, so both comparisons hold to 1e-12."""
    ba = _seven_families(od)
    types = list(SEVEN_FAMILIES)
    n = np.array([SEVEN_FAMILIES[t] for t in types])
    members = [len(g) for g in SEVEN_GROUPS]
    rows_of = {0: [2] * 37, 2: [4] * 5, 3: [3] * 3, 4: [od] * 2, 5: [6] * 5, 9: [2 * od] * 2, 10: [od * k for k in members]}   # residual rows of every factor
    for t in types:
        assert ba._fn("ba_num_factors")(ba._h, C.c_int32(t)) == ba.num_factors(t) == SEVEN_FAMILIES[t] == len(rows_of[t])
    assert ba._fn("ba_num_factors")(ba._h, C.c_int32(7)) == -1
    assert ba._fn("ba_num_residuals")(ba._h) == ba.num_residuals() == sum(sum(rows_of[t]) for t in types)
    slot0 = np.concatenate([[0], np.cumsum(n)])
    row0 = np.concatenate([[0], np.cumsum([sum(rows_of[t]) for t in types])])
    cost, res, sq = ba.evaluate(False)
    assert len(res) == row0[-1] and len(sq) == slot0[-1] and np.all(sq > 0.0)
    for f, t in enumerate(types):
        seg, q = res[row0[f]:row0[f + 1]], sq[slot0[f]:slot0[f + 1]]
        ends = np.concatenate([[0], np.cumsum(rows_of[t])])
        sums = np.array([(seg[ends[i]:ends[i + 1]] ** 2).sum() for i in range(n[f])])
        r = ba.debug_linearize(t)[0]
        r = np.concatenate([np.ravel(x) for x in r]) if t == obvi_ba.FACTOR_MAP_GROUP_PRIOR else r.ravel()
        print("od %d type %2d: norms %.2e  debug_linearize %.2e" % (od, t, np.abs(q / sums - 1.0).max(), helpers.rel_err(seg, r)))
        assert np.all(np.abs(q - sums) <= 1e-12 * sums) and r.shape == seg.shape and helpers.rel_err(seg, r) <= 1e-12
    assert abs(cost - 0.5 * sq.sum()) <= 1e-12 * cost
    # selection: the family's own segment of the norms and its own mask, exactly its length written
    for f, t in enumerate(types):
        want, want_n = helpers.map_rule(sq[slot0[f]:slot0[f + 1]], np.ones(n[f]), 0.5)
        mask, n_out = ba.select_outliers(t, 0.5)
        assert len(mask) == n[f] and n_out == want_n == n[f] // 2 and np.array_equal(mask, want), (t, mask, want)
        buf, nex = np.full(n[f] + 8, 7, np.uint8), C.c_int64(-1)
        ba._check(ba._fn("ba_select_outliers")(ba._h, C.c_int32(t), C.c_double(0.5), buf.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(nex)), "select_outliers")
        assert np.array_equal(buf[:n[f]], want) and np.all(buf[n[f]:] == 7) and nex.value == want_n
    with pytest.raises(obvi_ba.ObviError, match="status -1 select_outliers: unknown factor type"):
        ba._check(ba._fn("ba_select_outliers")(ba._h, C.c_int32(7), C.c_double(0.5), buf.ctypes.data_as(C.POINTER(C.c_uint8)), None), "select_outliers")
    # masks: one factor of one family out, family after family
    for f, t in enumerate(types):
        k = n[f] // 2
        mask = np.ones(n[f], np.uint8); mask[k] = 0
        ba.set_active_mask(t, mask)
        _, res1, sq1 = ba.evaluate(False)
        ends = row0[f] + np.concatenate([[0], np.cumsum(rows_of[t])])
        gone_rows = np.zeros(len(res), bool); gone_rows[ends[k]:ends[k + 1]] = True
        gone = np.zeros(len(sq), bool); gone[slot0[f] + k] = True
        assert np.all(res1[gone_rows] == 0.0) and np.all(sq1[gone] == 0.0), t
        assert np.array_equal(res1[~gone_rows], res[~gone_rows]) and np.array_equal(sq1[~gone], sq[~gone]), t
        ba.set_active_mask(t, None)
    _, res2, sq2 = ba.evaluate(False)
    assert np.array_equal(res2, res) and np.array_equal(sq2, sq)
    with pytest.raises(obvi_ba.ObviError, match="status -1 set_active_mask: unknown factor type"):
        ba.set_active_mask(7, None)
