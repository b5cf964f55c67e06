"""The extended-precision reference of tests/schur_cases.py against the fp64 oracle, on the CPU: the reduced system entry by entry on the scale A, one LM
step, the step's scalars -- and the conditions the cases must meet so that the reference alone stays inside them (the oracle accepts the first step, every
depth is positive, no 3x3 pivot of the reference is non-positive, both Huber branches occur).  The errors measured here are e(oracle) of the case table
(schur_cases.TABLE): the bounds of tests/test_gpu_schur_edges.py derive from them."""
import numpy as np
import pytest

import helpers
import schur_cases as sc
import synth


def measure(name):
    """e(oracle) of a case, as a dict with the keys of schur_cases.TABLE"""
    case = sc.CASES[name]()
    prob = case["prob"]
    o = helpers.oracle_ba()
    synth.upload(o, prob)
    o.set_active_mask(0, case["mask0"])
    out = dict(S=0.0, b=0.0, n_terms=0)
    for radius in sc.RADII:
        ref = sc.reference(prob, o, radius, case["mask0"], want_step=False)
        assert ref["pivots_ok"], "a 3x3 pivot of the reference is not positive"
        assert ref["both_huber_branches"]
        S, b = o.debug_reduced_system(radius)
        assert S.shape == ref["S"].shape
        assert sc.exact_zeros(S, ref["S"]) and sc.exact_zeros(b, ref["b"])
        out["S"] = max(out["S"], sc.entry_error(S, ref["S"], ref["A_S"]))
        out["b"] = max(out["b"], sc.entry_error(b, ref["b"], ref["A_b"]))
        out["n_terms"] = max(out["n_terms"], ref["n_terms"])
    ref = sc.reference(prob, o, sc.RADII[0], case["mask0"])
    o.solve(helpers.ba_params(max_it=1, ftol=0.0, gtol=0.0, ptol=0.0, radius=sc.RADII[0]))
    it = o.iterations()
    assert len(it) == 2 and it[1].step_is_successful, "the oracle must accept the first step"
    out["step_pose"], out["step_point"] = sc.step_errors(prob, o.get_poses(), o.get_points(), ref)
    out.update(sc.scalar_errors(it[0], it[1], ref))
    # what the step must not touch
    still = ~ref["point_var"]
    assert np.array_equal(o.get_points()[still], prob["points"][still]) and np.array_equal(o.get_poses()[~ref["pose_var"]], prob["poses"][~ref["pose_var"]])
    return out


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_oracle_against_the_extended_reference(name):
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63
    case = sc.CASES[name]()
    prob = case["prob"]
    for c in range(len(prob["K"])):                                   # every depth is positive
        m = prob["rp_cam"] == c
        assert (synth.project_points(prob["poses"][prob["rp_pose"][m]], prob["points"][prob["rp_point"][m]], prob["K"][c], prob["ext"][c])[1] > 0).all()
    e = measure(name)
    print("e(oracle) %s: %s" % (name, ", ".join("%s=%.3g" % kv for kv in e.items())))
    t = sc.TABLE[name]
    assert e["n_terms"] == t["n_terms"]
    for k, v in e.items():
        if k == "n_terms":
            continue
        # the oracle is fp64: its error is a small multiple of 2^-53 times the conditioning of the case, far below a dropped term (order 1 on these scales)
        assert v < 1e-9, (k, v)
        assert v <= 2.0 * t[k] and t[k] <= 2.0 * max(v, 2.0 ** -60), "schur_cases.TABLE[%r][%r] = %.3g, measured %.3g: measure again and update the table" % (name, k, t[k], v)


def test_the_cutting_rules_on_hand_made_lists():
    """cut_pieces on lists short enough to do by hand"""
    assert sc.cut_pieces([3, 0, 2]) == ([(0, 5)], [])
    assert sc.cut_pieces([64, 1]) == ([(0, 64), (64, 1)], [])
    assert sc.cut_pieces([2, 65, 2]) == ([(0, 2), (67, 2)], [1])
    assert sc.cut_pieces([1] + [0] * 62 + [1]) == ([(0, 2)], [])            # ids 0 and 63: 63 apart
    assert sc.cut_pieces([1] + [0] * 63 + [1]) == ([(0, 1), (1, 1)], [])    # ids 0 and 64
    assert sc.cut_pieces([2] * 32) == ([(0, 62), (62, 2)], [])              # 18 * 64 + 4 * 32 = 1280 > 1264
    assert sc.cut_pieces([1] * 58) == ([(0, 57), (57, 1)], [])              # 22 * 58 = 1276 > 1264
