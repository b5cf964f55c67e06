"""The point pass with its loads requested in front of the `live` branch against the order it replaces (k_point_pass in ba_kernels.hip).

OBVI_POINT_FLAT (default 1): k_point_pass requests pixel, camera index, sigma and flag of an observation with its two indices, the 21 pose-cache gathers beside
the point's flags and position, and the point's Jacobi scale in front of the segmented scan; 0: inside the `live` branch and behind the scan, as before.  The
knob only moves loads: lanes, arithmetic, order of every sum and every reduction are the knob-off route's, which is the reference of every comparison here.
  * deterministic handle, three LM iterations: iteration records, features, poses and objects EXACTLY equal
  * default handle, one LM step from identical values: records and the state behind the step within 1e-10 relative (the bar of
    tests/test_gpu_pose_lin_reuse.py), after two runs of the knob-off route have been shown to agree within the same bar (else the case decides nothing)
Shapes: the two problems of tests/test_gpu_pose_lin_reuse.py; 5 features (less than one wavefront's) and 241 (a partial last wavefront and workgroup); 72 poses
with five features of 70 sightings (k_point_pass_long, which keeps its order, beside pieces of the flat kernel); tracks cut so that feature k keeps
1 + k % 13 sightings (pieces of many short runs, one-sighting features); a mask that switches off all sightings of some features and single sightings of
others (lanes whose hoisted loads are not used).  Every case runs under OBVI_BACKSUB_LANES = 1, 2, 4, 8 and 16: the back-substitution reads what the point
pass wrote, with every lane count it can be given.

(The staged back-substitution these cases were also written for -- a wavefront fetching the Z records of a round together through LDS -- was measured and
not kept: profiles/EXPERIMENTS.md, round 10.)

Without a GPU: registers and private segment of k_point_pass, read from the code object as tests/test_side_register_budget.py does.
"""
import numpy as np
import pytest

import helpers
import obvi_ba
import synth
from test_gpu_pose_lin_reuse import big_problem, records, same_record, small_problem
from test_side_register_budget import CU_LDS_BYTES, _one, kernel_metadata

BAR = 1e-10
LANES = (1, 2, 4, 8, 16)
FLAT, LANES_KNOB = "OBVI_POINT_FLAT", "OBVI_BACKSUB_LANES"
LONG_SIGHTINGS, LONG_FEATURES = 70, (7, 60, 133, 210, 299)


def cut_tracks(prob, keep_whole=()):
    """feature k keeps its first 1 + k % 13 sightings (the sightings are sorted by feature, then pose)"""
    prob = dict(prob)
    pt = prob["rp_point"].astype(np.int64)
    n = len(pt)
    rank = np.arange(n) - np.searchsorted(pt, pt)          # position of a sighting inside its feature's run
    keep = (rank < 1 + pt % 13) | np.isin(pt, keep_whole)
    for k, v in list(prob.items()):
        if k.startswith("rp_") and isinstance(v, np.ndarray) and v.shape[:1] == (n,):
            prob[k] = v[keep]
    return prob


def long_problem():
    """72 poses, 300 features; five of them are seen from 70 poses each: more sightings than a wavefront has lanes (k_point_pass_long), and 70 = 8 x 8 + 6 =
    17 x 4 + 2 sightings per lane group of the back-substitution.  Their points lie 18-24 m ahead of the middle of the arc, in front of every camera of the trajectory."""
    prob = synth.make_problem(P=72, L=300, O=2, seed=5, const_poses=2, min_obj_obs=3)
    P = 72
    rng = np.random.Generator(np.random.MT19937(77))
    radius = max(P * 0.2 / (2 * np.pi), 10.0)
    mid = 0.5 * (P - 1) * 0.2 / radius
    drop = np.isin(prob["rp_point"], LONG_FEATURES)
    out = {k: [v[~drop]] for k, v in prob.items() if k.startswith("rp_") and isinstance(v, np.ndarray) and v.shape[:1] == (len(drop),)}
    prob["points"], prob["gt_points"] = prob["points"].copy(), prob["gt_points"].copy()
    for i, l in enumerate(LONG_FEATURES):
        rho = 18.0 + 1.5 * i
        ang = mid + 0.05 * (i - 2)
        X = np.array([-rho * np.sin(ang), rho * np.cos(ang), 0.3 * i - 0.5])
        frames = np.arange(1, 1 + LONG_SIGHTINGS)
        pix, z = synth.project_points(prob["gt_poses"][frames], np.repeat(X[None, :], len(frames), axis=0))
        assert z.min() > 0.5, (l, z.min())
        prob["gt_points"][l] = X
        prob["points"][l] = X + 0.1 * rng.normal(size=3)
        out["rp_pose"].append(frames.astype(np.uint32)); out["rp_point"].append(np.full(len(frames), l, np.uint32))
        out["rp_cam"].append(np.zeros(len(frames), np.uint16)); out["rp_pixel"].append(pix + rng.normal(size=pix.shape))
        out["rp_is_outlier"].append(np.zeros(len(frames), bool))
    cat = {k: np.concatenate(v) for k, v in out.items()}
    order = np.lexsort((cat["rp_cam"], cat["rp_pose"], cat["rp_point"]))
    for k, v in cat.items():
        prob[k] = v[order]
    return prob


def sighting_mask(prob):
    """all sightings of every 11th feature off (a feature without factors), and the second sighting (the first of a one-sighting feature) of every 7th"""
    pt = prob["rp_point"].astype(np.int64)
    rank = np.arange(len(pt)) - np.searchsorted(pt, pt)
    count = np.bincount(pt, minlength=len(prob["points"]))[pt]
    m = np.ones(len(pt), np.uint8)
    m[pt % 11 == 3] = 0
    m[(pt % 7 == 2) & (rank == np.minimum(1, count - 1))] = 0
    return m


def _build(name):
    if name == "small":
        return cut_tracks(small_problem()), False
    if name == "small_masked":
        return cut_tracks(small_problem()), True
    if name == "big":
        return cut_tracks(big_problem()), False
    if name == "five":
        return cut_tracks(synth.make_problem(P=12, L=5, O=2, seed=3, const_poses=2, min_obj_obs=3)), False
    if name == "l241":
        return cut_tracks(synth.make_problem(P=12, L=241, O=2, seed=4, const_poses=2, min_obj_obs=3)), False
    if name == "long":
        return cut_tracks(long_problem(), keep_whole=LONG_FEATURES), False
    if name == "long_masked":
        return cut_tracks(long_problem(), keep_whole=LONG_FEATURES), True
    raise KeyError(name)


PROBLEMS = ("small", "small_masked", "big", "five", "l241", "long", "long_masked")
_cache = {}


def problem(name):
    if name not in _cache:
        _cache[name] = _build(name)
    return _cache[name]


def test_the_problems_have_the_shapes_the_routes_branch_on():
    for name in PROBLEMS:
        prob, _ = problem(name)
        count = np.bincount(prob["rp_point"].astype(np.int64), minlength=len(prob["points"]))
        print(name, len(prob["poses"]), len(prob["points"]), len(prob["rp_point"]), np.bincount(count)[:15])
        assert count.min() >= 1
        if name in ("small", "big", "l241"):
            for c in (1, 2, 3, 4, 5, 7, 8, 9):          # both sides of every multiple of 2, 4 and 8 a cut track can reach
                assert (count == c).any(), (name, c)
    assert len(problem("five")[0]["points"]) == 5 and len(problem("l241")[0]["points"]) == 241
    prob, _ = problem("long")
    count = np.bincount(prob["rp_point"].astype(np.int64), minlength=300)
    assert (count[list(LONG_FEATURES)] == LONG_SIGHTINGS).all() and (np.delete(count, LONG_FEATURES) <= 13).all()
    m = sighting_mask(prob)
    off = np.bincount(prob["rp_point"].astype(np.int64), weights=1.0 - m, minlength=300)
    assert ((off == count) & (count > 0)).any() and (off == 1).any()


def run(monkeypatch, name, lanes, flat, deterministic, max_it):
    prob, masked = problem(name)
    monkeypatch.setenv(LANES_KNOB, str(lanes))
    monkeypatch.setenv(FLAT, "1" if flat else "0")
    ba = helpers.product_ba(deterministic=deterministic)       # (the knobs are read here, once per handle)
    for k in (LANES_KNOB, FLAT):
        monkeypatch.delenv(k, raising=False)
    synth.upload(ba, prob)
    if masked:
        ba.set_active_mask(obvi_ba.FACTOR_REPROJECTION, sighting_mask(prob))
    ba.solve(helpers.ba_params(max_it=max_it, ftol=0.0, gtol=0.0, ptol=0.0))
    out = records(ba), ba.get_points(), ba.get_poses(), ba.get_objects()
    ba.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("name", PROBLEMS)
def test_deterministic_handle_is_bit_identical_to_the_knob_off_route(name, lanes, monkeypatch):
    ref = run(monkeypatch, name, lanes, False, True, 3)
    assert len(ref[0]) == 4
    got = run(monkeypatch, name, lanes, True, True, 3)
    assert got[0] == ref[0], (name, lanes, got[0], ref[0])
    for a, b in zip(got[1:], ref[1:]):
        assert np.array_equal(a, b), (name, lanes, float(np.abs(a - b).max()))


def close(a, b, what):
    """records (decisions equal, cost / gradient norms / radius within BAR) and the state behind the step within BAR relative"""
    assert len(a[0]) == len(b[0]) == 2, what
    for k in range(2):
        same_record(a[0][k], b[0][k], BAR, "%s record %d" % (what, k))
    for x, y, label in zip(a[1:], b[1:], ("features", "poses", "objects")):
        err = helpers.rel_err(x, y)
        print("%s %s: %.2e" % (what, label, err))
        assert err <= BAR, (what, label, err)


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("name", PROBLEMS)
def test_default_handle_agrees_with_the_knob_off_route_over_one_step(name, lanes, monkeypatch):
    ref = run(monkeypatch, name, lanes, False, False, 1)
    again = run(monkeypatch, name, lanes, False, False, 1)
    close(again, ref, "%s lanes %d knob-off twice" % (name, lanes))      # the case decides at this bar
    got = run(monkeypatch, name, lanes, True, False, 1)
    close(got, ref, "%s lanes %d flat" % (name, lanes))


def test_register_budget_of_the_point_pass():
    """k_point_pass: at most 128 registers and no private segment (four wavefronts per SIMD beside its 40 KB LDS image, four workgroups' images on a CU), in
    both orders of its loads."""
    kernels = kernel_metadata()
    passes = {n: k for n, k in _one(kernels, "k_point_pass").items() if "k_point_pass_long" not in n}
    assert len(passes) == 2, sorted(passes)          # <false>: the order before, <true>: the flat one
    for name, k in passes.items():
        print(name, k[".vgpr_count"], k[".group_segment_fixed_size"], k[".private_segment_fixed_size"])
        assert k[".vgpr_count"] <= 128 and k[".private_segment_fixed_size"] == 0, (name, k[".vgpr_count"], k[".private_segment_fixed_size"])
        assert 4 * k[".group_segment_fixed_size"] <= CU_LDS_BYTES, (name, k[".group_segment_fixed_size"])
