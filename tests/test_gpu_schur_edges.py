"""The point pass (k_point_pass / k_point_pass_long) and the Schur assembly (k_schur_window / k_schur_blocks) at the edges of the host's packing and windowing,
on the designed incidence structures of tests/schur_cases.py: how the host routed the work (obvi_ba_get_problem_stats against the Python restatement of the
two cutting rules), the reduced system entry by entry, one LM step with its scalars, and the reduced system again after a mask change on the kept plan --
all against the long double reference, within max(8 e(oracle), n_terms 2^-53) (schur_cases.TABLE; tests/test_schur_reference.py measures e(oracle)).
A dropped or doubled contribution is an error of order 1 on these scales."""
import functools

import numpy as np
import pytest

import helpers
import schur_cases as sc
import synth

pytestmark = pytest.mark.gpu

HANDLES = ("default", "deterministic")
RE_AIM = " -- the strip geometry or the LDS image changed, or the Python restatement is off: re-aim the cases of tests/schur_cases.py"


@functools.lru_cache(maxsize=None)
def _reference(name, radius):
    """computed once per case and radius, shared by the tests, never modified; the step only at the solve's own radius"""
    case = sc.CASES[name]()
    o = helpers.oracle_ba()
    synth.upload(o, case["prob"])
    return sc.reference(case["prob"], o, radius, case["mask0"], want_step=radius == sc.RADII[0])


def _product(name, handle):
    case = sc.CASES[name]()
    g = helpers.product_ba(deterministic=handle == "deterministic")
    synth.upload(g, case["prob"])
    g.set_active_mask(0, case["mask0"])                 # before the first plan
    return case, g


def _check_system(name, g, radius, ref, what=""):
    S, b = g.debug_reduced_system(radius)
    assert S.shape == ref["S"].shape
    eS, eb = sc.entry_error(S, ref["S"], ref["A_S"]), sc.entry_error(b, ref["b"], ref["A_b"])
    print("%s%s radius %g: e(S) = %.3g (bound %.3g), e(b) = %.3g (bound %.3g)" % (name, what, radius, eS, sc.bound(name, "S"), eb, sc.bound(name, "b")))
    assert sc.exact_zeros(S, ref["S"]) and sc.exact_zeros(b, ref["b"]), "an entry outside the structure is not exactly zero"
    assert eS <= sc.bound(name, "S") and eb <= sc.bound(name, "b")
    return S, b


def _check_step(name, case, g, ref):
    prob = case["prob"]
    g.solve(helpers.ba_params(max_it=1, ftol=0.0, gtol=0.0, ptol=0.0, radius=sc.RADII[0]))
    it = g.iterations()
    assert len(it) == 2 and it[1].step_is_successful
    poses, points = g.get_poses(), g.get_points()
    e = sc.scalar_errors(it[0], it[1], ref)
    e["step_pose"], e["step_point"] = sc.step_errors(prob, poses, points, ref)
    print("%s step: %s" % (name, ", ".join("e(%s) = %.3g (bound %.3g)" % (k, v, sc.bound(name, k)) for k, v in e.items())))
    # what the step must not touch comes back bit for bit: constant poses; constant, unobserved and fully masked points
    groups = case["groups"]
    still = ~ref["point_var"]
    for k in ("const_point", "all_masked", "unobserved"):
        assert all(still[l] for l in groups.get(k, []))
    assert np.array_equal(points[still], prob["points"][still]) and np.array_equal(poses[~ref["pose_var"]], prob["poses"][~ref["pose_var"]])
    for k, v in e.items():
        assert v <= sc.bound(name, k), (k, v, sc.bound(name, k))
    return poses, points


@pytest.mark.parametrize("handle", HANDLES)
@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_routing(name, handle):
    case, g = _product(name, handle)
    g.evaluate(True, False)
    g.debug_reduced_system(sc.RADII[0])                 # (the plan exists after it)
    st, pr = g.problem_stats(), case["predict"]
    print(name, handle, {k: int(st[k]) for k in ("poses_var", "points_var", "point_pieces", "long_points", "schur_pairs", "schur_pairs_blocks", "schur_blocks", "schur_batches")},
          "predicted batches on a deterministic handle:", pr["schur_batches_det"])
    assert st["poses_var"] == pr["n_frames"]
    assert st["point_pieces"] == pr["point_pieces"] and st["long_points"] == len(pr["long_points"]), "k_point_pass pieces" + RE_AIM
    assert st["schur_pairs_blocks"] == pr["schur_pairs_blocks"], "pairs of k_schur_blocks" + RE_AIM
    assert st["schur_pairs"] == pr["schur_pairs_blocks"] + pr["schur_pairs_strip"], "pairs in all" + RE_AIM
    assert st["schur_blocks"] == (pr["schur_blocks_det"] if handle == "deterministic" else pr["schur_items_default"]), "blocks / work items of k_schur_blocks" + RE_AIM
    if handle == "deterministic":                          # one workgroup per work list: the batches are those of the lists
        assert st["schur_batches"] == pr["schur_batches_det"], "batches of k_schur_window" + RE_AIM
    if name == "strip_7":
        assert st["schur_batches"] >= 4 and max(pr["list_batches"].values()) >= 4
        if handle == "default":
            assert st["schur_blocks"] == pr["schur_blocks_det"] + 1                    # the 300-pair block: two work items


@pytest.mark.parametrize("handle", HANDLES)
@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_reduced_system(name, handle):
    case, g = _product(name, handle)
    for radius in sc.RADII:
        _check_system(name, g, radius, _reference(name, radius))


@pytest.mark.parametrize("handle", HANDLES)
@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_step_and_the_reduced_system_after_a_mask_change(name, handle):
    case, g = _product(name, handle)
    poses, points = _check_step(name, case, g, _reference(name, sc.RADII[0]))
    # the masks of the second kind, on the kept plan; the reference at the state the device is in (a fresh oracle handle, linearised there)
    g.set_active_mask(0, case["mask1"])
    moved = dict(case["prob"], poses=poses, points=points)
    o = helpers.oracle_ba()
    synth.upload(o, moved)
    for radius in sc.RADII:
        _check_system(name, g, radius, sc.reference(moved, o, radius, case["mask1"], want_step=False), " after the mask change")


@pytest.mark.parametrize("lanes", [2, 4, 8, 16])
@pytest.mark.parametrize("name", sc.PACKING_CASES)
def test_back_substitution_lanes(name, lanes, monkeypatch):
    """tracks of 1, 2, 63 and 65 sightings under every width of the back-substitution (1 and 32 are covered by tests/test_gpu_parity.py)"""
    monkeypatch.setenv("OBVI_BACKSUB_LANES", str(lanes))
    case, g = _product(name, "default")
    counts = set(case["predict"]["counts"])
    assert {1, 2, 63, 65} <= counts
    _check_step(name, case, g, _reference(name, sc.RADII[0]))


def test_renumbered_points(monkeypatch):
    """the features renumbered by first sighting (as for large problems): other pieces, same numbers"""
    monkeypatch.setenv("OBVI_POINT_RENUMBER_MIN", "1")
    case, g = _product("pack_a", "default")
    for radius in sc.RADII:
        _check_system("pack_a", g, radius, _reference("pack_a", radius))
    _check_step("pack_a", case, g, _reference("pack_a", sc.RADII[0]))


def test_slot_tables_of_the_host(monkeypatch):
    """the host's own fill of the slot tables (split and merged layouts, twins): within the bound, and on deterministic handles bit-identical to the device's fill"""
    out = []
    for on_host in ("1", "0"):
        monkeypatch.setenv("OBVI_PLAN_SLOTS_ON_HOST", on_host)
        case, g = _product("strip_7", "deterministic")
        assert case["predict"]["layouts"]["twin split"] > 0 and case["predict"]["layouts"]["split"] > 0
        out.append([_check_system("strip_7", g, radius, _reference("strip_7", radius), " slots on host " + on_host) for radius in sc.RADII])
        g.close()
    for (S1, b1), (S0, b0) in zip(*out):
        assert np.array_equal(S1, S0) and np.array_equal(b1, b0)
