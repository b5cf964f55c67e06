"""The object side of the reduced system -- bounding boxes, shape and LTM priors, relative poses (bbox_lin_lanes / k_bbox_lin_dense / k_bbox_gather,
object_priors_lin, relpose_lin_lanes, k_small_gather) and the rows and columns of the objects -- at the lane, slice and tile edges the designed cases of
tests/object_cases.py are aimed at, on four handles: default, the STORE route (OBVI_SMALL_LANES_BELOW=1) with the packed and with the unpacked side
stream, and deterministic.  Checked: the reduced system entry by entry, one LM step with its scalars and its trial cost, the reduced system again after a
mask change on the kept plan -- all against the long double reference, within max(8 max(e(oracle), e(second)), n_terms 2^-53) (object_cases.TABLE;
tests/test_object_reference.py measures both errors) -- bit-identity of deterministic handles across the two schedules, and the linearisation of types 2 to 5
against the oracle.  A dropped, doubled or misplaced contribution is an error of order 1 on these scales."""
import functools
import math

import numpy as np
import pytest

import helpers
import object_cases as oc
import schur_cases as sc

pytestmark = pytest.mark.gpu

HANDLES = {"default": {}, "store": {"OBVI_SMALL_LANES_BELOW": "1"}, "store_unpacked": {"OBVI_SMALL_LANES_BELOW": "1", "OBVI_SIDE_PACKED": "0"}, "deterministic": {}}
RE_AIM = " -- the row layout of a leaf changed, or its Python restatement is off: re-aim the cases of tests/object_cases.py"
PARAMS = dict(max_it=1, ftol=0.0, gtol=0.0, ptol=0.0, radius=oc.RADII[0])


def _oracle(case, prob=None):
    o = helpers.oracle_ba(object_block_size=case["od"])
    oc.upload(o, case, prob)
    return o


@functools.lru_cache(maxsize=None)
def _reference(name, radius):
    """computed once per case and radius, shared by the tests, never modified; the step only at the solve's own radius"""
    case = oc.CASES[name]()
    return oc.reference(case, oc.oracle_lin(_oracle(case)), radius, case["masks0"], want_step=radius == oc.RADII[0])


@functools.lru_cache(maxsize=None)
def _reference_after(name, state):
    """the reference with the masks of the second kind at a state the device reached (its bytes are the key: handles that agree bit for bit share it)"""
    case = oc.CASES[name]()
    P, L, od = len(case["prob"]["poses"]), len(case["prob"]["points"]), case["od"]
    x = np.frombuffer(state, np.float64)
    moved = dict(case["prob"], poses=x[:6 * P].reshape(P, 6), points=x[6 * P:6 * P + 3 * L].reshape(L, 3), objects=x[6 * P + 3 * L:].reshape(-1, od))
    lin = oc.oracle_lin(_oracle(case, moved))
    return [oc.reference(case, lin, radius, case["masks1"], want_step=False, prob=moved) for radius in oc.RADII]


def _product(name, handle, monkeypatch, **env):
    case = oc.CASES[name]()
    for k, v in {**oc.KNOBS.get(name, {}), **HANDLES[handle], **env}.items():
        monkeypatch.setenv(k, v)
    g = helpers.product_ba(deterministic=handle == "deterministic", object_block_size=case["od"])
    oc.upload(g, case)                                  # the masks of the first kind before the first plan
    return case, g


def _check_system(name, g, radius, ref, what=""):
    S, b = g.debug_reduced_system(radius)
    assert S.shape == ref["S"].shape
    eS, eb = sc.entry_error(S, ref["S"], ref["A_S"]), sc.entry_error(b, ref["b"], ref["A_b"])
    print("%s%s radius %g: e(S) = %.3g (bound %.3g), e(b) = %.3g (bound %.3g)" % (name, what, radius, eS, oc.bound(name, "S"), eb, oc.bound(name, "b")))
    assert sc.exact_zeros(S, ref["S"]) and sc.exact_zeros(b, ref["b"]), "an entry outside the structure is not exactly zero"
    if eS > oc.bound(name, "S"):
        i, j = np.unravel_index(np.argmax(np.where(ref["A_S"] > 0, np.abs(S - ref["S"]) / np.where(ref["A_S"] > 0, ref["A_S"], 1), 0)), S.shape)
        print("the worst entry: row %d, column %d of the canonical order (%d pose rows, then the objects)" % (i, j, ref["n_pose_rows"]))
    assert eS <= oc.bound(name, "S") and eb <= oc.bound(name, "b")
    return S, b


def _check_step(name, case, g, ref):
    prob = case["prob"]
    g.solve(helpers.ba_params(**PARAMS))
    it = g.iterations()
    assert len(it) == 2 and it[1].step_is_successful
    poses, points, objects = g.get_state()
    e = sc.scalar_errors(it[0], it[1], ref)
    e["step_pose"], e["step_point"], e["step_object"] = oc.step_errors(prob, poses, points, objects, ref)
    # the trial cost of the accepted step: sum of rho / 2 in long double from the oracle's block norms at the state the device reached (a fresh handle)
    o = _oracle(case, dict(prob, poses=poses, points=points, objects=objects))
    trial = oc.robust_cost(o.evaluate(False)[2], prob, [o.num_factors(t) for t in (0,) + oc.FAMILIES])
    e["trial_cost"] = float(abs(np.longdouble(it[1].cost) - trial) / trial)
    print("%s step: %s" % (name, ", ".join("e(%s) = %.3g (bound %.3g)" % (k, v, oc.bound(name, "cost" if k == "trial_cost" else k)) for k, v in e.items())))
    # constant or untouched blocks come back bit for bit
    assert (~ref["pose_var"]).sum() >= 3 and (~ref["object_var"]).sum() >= 1
    assert np.array_equal(points[~ref["point_var"]], prob["points"][~ref["point_var"]]) and np.array_equal(poses[~ref["pose_var"]], prob["poses"][~ref["pose_var"]])
    assert np.array_equal(objects[~ref["object_var"]], prob["objects"][~ref["object_var"]])
    for k, v in e.items():
        assert v <= oc.bound(name, "cost" if k == "trial_cost" else k), (k, v)
    return poses, points, objects


@pytest.mark.parametrize("handle", sorted(HANDLES))
@pytest.mark.parametrize("name", sorted(oc.CASES))
def test_reduced_system(name, handle, monkeypatch):
    case, g = _product(name, handle, monkeypatch)
    for radius in oc.RADII:
        _check_system(name, g, radius, _reference(name, radius), " " + handle)
    st = g.problem_stats()
    print(name, handle, {k: int(st[k]) for k in ("poses_var", "objects_var", "reduced_rows", "tiles_per_dim", "chol_levels", "bbox_active")})
    if name.startswith("lanes"):
        pose_row, obj_row, m = oc.leaf_rows(case["prob"], case["masks0"], case["od"])
        assert st["poses_var"] == len(pose_row) and st["objects_var"] == len(obj_row)
        assert st["reduced_rows"] == m == 6 * len(pose_row) + case["od"] * len(obj_row), "rows" + RE_AIM
        assert st["tiles_per_dim"] == math.ceil(m / oc.TILE) >= 2, "tiles" + RE_AIM
    else:
        assert st["poses_var"] == 40 and st["chol_levels"] >= 3, "the elimination tree is not three levels deep: re-aim the tree case of tests/object_cases.py"


@pytest.mark.parametrize("handle", sorted(HANDLES))
@pytest.mark.parametrize("name", sorted(oc.CASES))
def test_step_and_the_reduced_system_after_a_mask_change(name, handle, monkeypatch):
    case, g = _product(name, handle, monkeypatch)
    ref = _reference(name, oc.RADII[0])
    poses, points, objects = _check_step(name, case, g, ref)
    # the masks of the second kind, on the kept plan: a pose and an object lose every factor, their rows become padding and the system shrinks
    for t, m in case["masks1"].items():
        g.set_active_mask(t, m)
    after = _reference_after(name, np.concatenate([poses.ravel(), points.ravel(), objects.ravel()]).tobytes())
    assert after[0]["S"].shape[0] == ref["S"].shape[0] - 6 - case["od"]
    for radius, r in zip(oc.RADII, after):
        _check_system(name, g, radius, r, " %s after the mask change" % handle)


@pytest.mark.parametrize("name", sorted(oc.CASES))
def test_deterministic_handles_agree_bit_for_bit(name, monkeypatch):
    """OBVI_SIDE_PACKED 1 and 0, and a second run of the first: the reduced system, the records of the step and the state it leaves"""
    out = []
    for packed in ("1", "0", "1"):
        case, g = _product(name, "deterministic", monkeypatch, OBVI_SIDE_PACKED=packed)
        S, b = g.debug_reduced_system(oc.RADII[0])
        g.solve(helpers.ba_params(**PARAMS))
        its = g.iterations()
        for it in its:
            it.iteration_time_in_seconds = 0.0          # wall time: the one field of a record that is no result
        out.append((S, b, [bytes(it) for it in its], g.get_state()))
        g.close()
    assert len(out[0][2]) == 2 and np.abs(out[0][0]).max() > 0
    for S, b, its, state in out[1:]:
        assert np.array_equal(S, out[0][0]) and np.array_equal(b, out[0][1]) and its == out[0][2]
        assert all(np.array_equal(x, y) for x, y in zip(state, out[0][3]))


@pytest.mark.parametrize("name", sorted(oc.CASES))
def test_linearization_matches_oracle(name, monkeypatch):
    """types 2 to 5 at the tolerances of tests/test_gpu_parity.py; the invalid set is equal, with zero Jacobians"""
    case, g = _product(name, "default", monkeypatch)
    o = _oracle(case)
    for t in oc.FAMILIES:
        ro, J0o, J1o = o.debug_linearize(t)
        rg, J0g, J1g = g.debug_linearize(t)
        assert len(ro) > 0
        assert np.abs(rg - ro).max() <= 1e-12 * max(1.0, np.abs(ro).max()), t
        assert helpers.rel_err(J0g, J0o) < 1e-12, t
        if J1o is not None:
            assert helpers.rel_err(J1g, J1o) < 1e-12, t
        if t == 2:
            inv = np.all(ro == case["prob"]["bb_invalid"], axis=1)
            assert np.array_equal(inv, case["inside"][case["prob"]["bb_obj"]]) and np.array_equal(inv, np.all(rg == case["prob"]["bb_invalid"], axis=1))
            assert not J0g[inv].any() and not J1g[inv].any()
