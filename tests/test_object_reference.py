"""The extended-precision reference of tests/object_cases.py against the fp64 oracle, on the CPU: the reduced system over (variable poses, variable objects)
entry by entry on the scale A, one LM step, its scalars -- e(oracle) of object_cases.TABLE -- and the same reference fed with the product's own factor
arithmetic compiled for the host (tests/libhostmath.so) against the oracle-fed one -- e(second).  The bounds of tests/test_gpu_object_edges.py derive from
both.  Also here: the conditions under which the reference alone stays inside such a bound (positive depths and pivots, both Huber branches in every family,
the oracle accepts the first step, valid ellipses well away from the invalid branch and exactly the designed factors invalid), and what every case is aimed
at (list lengths, tails, kinds, straddling blocks), from the case's own arrays and the restated row layout."""
import numpy as np
import pytest

import helpers
import object_cases as oc
import schur_cases as sc
import synth

RE_AIM = " -- the case drifted off its target: re-aim the cases of tests/object_cases.py"
STEP_KEYS = ("step_pose", "step_point", "step_object")
SCALARS = ("cost", "gradient_max_norm", "gradient_norm", "step_norm")


def measure(name):
    """e(oracle) and e(second) of a case, as a dict with the keys of object_cases.TABLE"""
    case = oc.CASES[name]()
    prob, m0 = case["prob"], case["masks0"]
    o = helpers.oracle_ba(object_block_size=case["od"])
    oc.upload(o, case)
    lin = oc.oracle_lin(o)
    lin2, valid2 = oc.second_lin(prob, lin)
    # exactly the designed factors are invalid, by either arithmetic, with zero Jacobians
    designed = case["inside"][prob["bb_obj"]]
    for r, Jo, Jp in (lin[2], lin2[2]):
        invalid = np.all(r == prob["bb_invalid"], axis=1)
        assert np.array_equal(invalid, designed) and not Jo[invalid].any() and not Jp[invalid].any()
    assert np.array_equal(~valid2, designed)
    out = dict(S=0.0, b=0.0, second_S=0.0, second_b=0.0, n_terms=0)
    for radius in oc.RADII:
        ref = oc.reference(case, lin, radius, m0, want_step=False)
        ref2 = oc.reference(case, lin2, radius, m0, want_step=False)
        assert ref["pivots_ok"], "a 3x3 pivot of the reference is not positive"
        assert ref["both_huber_branches"] and all(ref["side_branches"][t] == (True, True) for t in oc.FAMILIES), ref["side_branches"]
        S, b = o.debug_reduced_system(radius)
        assert S.shape == ref["S"].shape == ref2["S"].shape
        assert sc.exact_zeros(S, ref["S"]) and sc.exact_zeros(b, ref["b"])
        assert np.array_equal(ref["S"] == 0, ref2["S"] == 0)
        out["S"] = max(out["S"], sc.entry_error(S, ref["S"], ref["A_S"]))
        out["b"] = max(out["b"], sc.entry_error(b, ref["b"], ref["A_b"]))
        nz, nzb = ref["A_S"] > 0, ref["A_b"] > 0
        out["second_S"] = max(out["second_S"], float((np.abs(ref2["S"][nz] - ref["S"][nz]) / ref["A_S"][nz]).max()))
        out["second_b"] = max(out["second_b"], float((np.abs(ref2["b"][nzb] - ref["b"][nzb]) / ref["A_b"][nzb]).max()))
        out["n_terms"] = max(out["n_terms"], ref["n_terms"])
    ref = oc.reference(case, lin, oc.RADII[0], m0)
    ref2 = oc.reference(case, lin2, oc.RADII[0], m0)
    o.solve(helpers.ba_params(max_it=1, ftol=0.0, gtol=0.0, ptol=0.0, radius=oc.RADII[0]))
    it = o.iterations()
    assert len(it) == 2 and it[1].step_is_successful, "the oracle must accept the first step"
    out["step_pose"], out["step_point"], out["step_object"] = oc.step_errors(prob, o.get_poses(), o.get_points(), o.get_objects(), ref)
    out.update(sc.scalar_errors(it[0], it[1], ref))
    for k in STEP_KEYS:
        out["second_" + k] = float(np.abs(ref2[k] - ref[k]).max() / np.abs(ref[k]).max())
    for k in SCALARS:
        out["second_" + k] = float(abs(ref2[k] - ref[k]) / ref[k])
    # what the step must not touch
    still_l, still_p, still_o = ~ref["point_var"], ~ref["pose_var"], ~ref["object_var"]
    assert still_p.sum() >= 3 and still_o.sum() >= 1
    assert np.array_equal(o.get_points()[still_l], prob["points"][still_l]) and np.array_equal(o.get_poses()[still_p], prob["poses"][still_p])
    assert np.array_equal(o.get_objects()[still_o], prob["objects"][still_o])
    return out


@pytest.mark.parametrize("name", sorted(oc.CASES))
def test_oracle_and_host_arithmetic_against_the_extended_reference(name):
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63
    case = oc.CASES[name]()
    prob = case["prob"]
    for c in range(len(prob["K"])):                                   # every depth is positive; every valid ellipse is well away from the invalid branch
        m = prob["rp_cam"] == c
        assert (synth.project_points(prob["poses"][prob["rp_pose"][m]], prob["points"][prob["rp_point"][m]], prob["K"][c], prob["ext"][c])[1] > 0).all()
        m = (prob["bb_cam"] == c) & ~case["inside"][prob["bb_obj"]]
        px, valid, depth = synth.project_ellipsoids(prob["objects"][prob["bb_obj"][m]], prob["poses"][prob["bb_pose"][m]], prob["K"][c], prob["ext"][c])
        assert valid.all() and (depth > 5.0).all()
        # xin / q13^2 = ((u_max - u_min) / (u_max + u_min))^2 in normalised image coordinates, and the same for y
        u = (px - prob["K"][c][[2, 2, 3, 3]]) / prob["K"][c][[0, 0, 1, 1]]
        margin = np.minimum(((u[:, 0] - u[:, 1]) / (u[:, 0] + u[:, 1])) ** 2, ((u[:, 2] - u[:, 3]) / (u[:, 2] + u[:, 3])) ** 2)
        assert margin.min() > 1e-4, margin.min()
    e = measure(name)
    print("%s: dict(%s)," % (name, ", ".join("%s=%.2g" % kv if kv[0] != "n_terms" else "%s=%d" % kv for kv in e.items())))
    t = oc.TABLE[name]
    assert e["n_terms"] == t["n_terms"]
    for k, v in e.items():
        if k == "n_terms":
            continue
        # fp64 against long double: a small multiple of 2^-53 times the conditioning of the case, far below a dropped term (order 1 on these scales)
        assert v < 1e-9, (k, v)
        assert v <= 2.0 * t[k] and t[k] <= 2.0 * max(v, 2.0 ** -60), "object_cases.TABLE[%r][%r] = %.3g, measured %.3g: measure again and update the table" % (name, k, t[k], v)


@pytest.mark.parametrize("od", (7, 9))
@pytest.mark.parametrize("variant", ("d", "u"))
def test_what_the_lanes_case_is_aimed_at(od, variant):
    case = oc.lanes(od, variant)
    prob, a = case["prob"], oc.aim(case)
    print(case["name"], a)
    # the last wavefront of four and the last workgroup of sixteen factors are partly filled; the tails differ across od and variant
    assert a["n_bb"] % 4 == {(7, "d"): 3, (9, "d"): 2, (7, "u"): 1, (9, "u"): 3}[(od, variant)] and a["n_bb"] % 16 != 0, "bounding-box tail" + RE_AIM
    want = {1, 6, 7, 8, 14, 15} if od == 7 else {1, 3, 4, 5, 9}
    assert want <= set(a["object_lists"]) and 0 in a["object_lists"], "object lists" + RE_AIM
    if variant == "d":
        assert max(a["object_lists"]) >= 29 and a["bbox"]["twice"], "the long list" + RE_AIM
    else:
        assert not a["bbox"]["twice"], "an (object, pose) pair twice in the variant of the plain-store route" + RE_AIM
    assert {0, 1, 2} <= set(a["pose_lists"]) and max(a["pose_lists"]) >= 5, "pose lists" + RE_AIM
    assert all(v for k, v in a["bbox"].items() if k != "twice"), str(a["bbox"]) + RE_AIM
    # priors: the switch of family inside a wavefront, the last workgroup partly filled
    assert a["n_sp"] % 64 != 0 and a["n_sp"] < 64 < a["n_sp"] + a["n_lt"] and (a["n_sp"] + a["n_lt"]) % 64 != 0, "prior counts" + RE_AIM
    assert all(a["priors"].values()), str(a["priors"]) + RE_AIM
    assert a["n_rl"] % 4 != 0 and all(a["relpose"].values()), str(a["relpose"]) + RE_AIM
    # rows: a pose block and an object block straddle a multiple of 64; so does, in both directions, an object x pose block with an active bounding-box factor
    pose_row, obj_row, m = oc.leaf_rows(prob, case["masks0"], od)
    assert m == 6 * len(pose_row) + od * len(obj_row) and m > 2 * oc.TILE
    assert any(oc.straddles(r, 6) for r in pose_row.values()) and any(oc.straddles(r, od) for r in obj_row.values()), "straddling blocks" + RE_AIM
    act = case["masks0"][2] != 0
    both = [(int(o), int(p)) for o, p in zip(prob["bb_obj"][act], prob["bb_pose"][act])
            if int(o) in obj_row and int(p) in pose_row and oc.straddles(obj_row[int(o)], od) and oc.straddles(pose_row[int(p)], 6)]
    assert both, "an object x pose block that straddles in both directions" + RE_AIM
    # the masks of the second kind leave one pose and one object without an active factor
    vp0, vo0 = oc.variable_blocks(prob, case["masks0"])
    vp1, vo1 = oc.variable_blocks(prob, case["masks1"])
    assert vp0.sum() - vp1.sum() == 1 and not vp1[case["drop_pose"]] and vo0.sum() - vo1.sum() == 1 and not vo1[case["drop_obj"]]


@pytest.mark.parametrize("od", (7, 9))
def test_what_the_tree_case_is_aimed_at(od):
    case = oc.tree(od)
    prob, a = case["prob"], oc.aim(case)
    print(case["name"], a)
    vp0, vo0 = oc.variable_blocks(prob, case["masks0"])
    vp1, vo1 = oc.variable_blocks(prob, case["masks1"])
    assert vp0.sum() == 40 and vp0.sum() - vp1.sum() == 1 and vo0.sum() - vo1.sum() == 1
    frame = np.cumsum(vp0) - 1
    span = {}
    for o, p in zip(prob["bb_obj"][case["masks0"][2] != 0], prob["bb_pose"][case["masks0"][2] != 0]):
        if vp0[p]:
            lo, hi = span.get(int(o), (99, -1))
            span[int(o)] = (min(lo, int(frame[p])), max(hi, int(frame[p])))
    n = case["names"]
    assert all(span[n[k]][1] - span[n[k]][0] <= 5 for k in ("leaf_a", "leaf_b", "leaf_c", "leaf_d")), "objects inside a leaf" + RE_AIM
    assert all(7 <= span[n[k]][1] - span[n[k]][0] <= 9 for k in ("across_low", "across_mid", "across_high")), "objects across a separator" + RE_AIM
    assert span[n["root"]] == (0, 39), "an object seen from the first and the last frame" + RE_AIM
    assert a["relpose"]["reverse"] and a["relpose"]["consecutive"] and a["relpose"]["far"] and a["relpose"]["inactive"] and a["bbox"]["twice"]


def test_the_row_layout_of_a_leaf_on_a_hand_made_problem():
    """leaf_rows on a problem small enough to do by hand: poses 0 (constant), 1, 2; objects 0 (first seen from pose 2), 1 (from pose 1), 2 (a prior only)"""
    prob = dict(poses=np.zeros((3, 6)), objects=np.zeros((3, 7)), pose_const=np.array([1, 0, 0], np.uint8), object_const=np.zeros(3, np.uint8),
                point_const=np.zeros(1, np.uint8), rp_pose=np.array([1, 2], np.uint32), rp_point=np.array([0, 0], np.uint32),
                bb_obj=np.array([0, 1, 1], np.uint32), bb_pose=np.array([2, 1, 0], np.uint32), bb_huber=0.5, sp_obj=np.array([2], np.uint32), sp_huber=10.0)
    masks = {0: np.ones(2, np.uint8), 2: np.ones(3, np.uint8), 3: np.ones(1, np.uint8)}
    assert oc.leaf_rows(prob, masks, 7) == ({1: 0, 2: 6}, {1: 12, 0: 19, 2: 26}, 33)
    masks[2] = np.array([1, 0, 1], np.uint8)                       # object 1 is left with a box from the constant pose: variable, no observing frame
    assert oc.leaf_rows(prob, masks, 9) == ({1: 0, 2: 6}, {0: 12, 1: 21, 2: 30}, 39)
    assert oc.straddles(60, 6) and oc.straddles(123, 7) and oc.straddles(120, 9) and not oc.straddles(64, 9) and not oc.straddles(58, 6)
