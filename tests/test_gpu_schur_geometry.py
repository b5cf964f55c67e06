"""GPU (-m gpu), and the code object's metadata without one: the two strip geometries of k_schur_window (ba_device.h: SchurWide,
SchurNarrow).

A default handle takes the narrow geometry (three tile columns per column group, 24 KB batches, three wavefronts per SIMD) from OBVI_SCHUR_WIDE_BELOW
reprojection observations on and the wide one (five, 32 KB, two) below; a deterministic handle is always wide.  The knob is read at obvi_ba_create; the cases of
tests/schur_geometry_cases.py are far below its default, so the tests set it: 0 = narrow, 1 << 62 = wide.

  * the assembled reduced system of either geometry against the extended-precision reference, with the checker and the bound of tests/test_gpu_schur_edges.py
  * the iteration records of a three-step solve, narrow against wide, at the bars of tests/test_gpu_pose_lin_reuse.py for two schedules of the same arithmetic
  * a deterministic handle: bit-identical results whatever the knob says
  * registers, LDS and private segment of the four instantiations, from the metadata note of the built code object (no instruction text)
"""
import functools

import numpy as np
import pytest

import helpers
import schur_cases as sc
import schur_geometry_cases as gc
import synth
from test_gpu_pose_lin_reuse import BAR, records, rel, same_record
from test_side_register_budget import CU_LDS_BYTES, SIMD_VGPRS, _alloc, _one, kernel_metadata

KNOB = "OBVI_SCHUR_WIDE_BELOW"
GEOMETRIES = {"narrow": ("0", 3), "wide": (str(1 << 62), 5)}
# k_schur_window<TWIN, SchurWide> as the parent of the narrow geometry built it (TWIN true and false alike): .vgpr_count, LDS bytes, private segment
WIDE_VGPRS, WIDE_LDS, WIDE_PRIVATE = 214, 69808, 0


def handle(monkeypatch, knob, deterministic=False):
    if knob is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, knob)
    ba = helpers.product_ba(deterministic=deterministic)       # (the knobs are read here, once per handle)
    monkeypatch.delenv(KNOB, raising=False)
    return ba


@functools.lru_cache(maxsize=None)
def _reference(name, radius):
    """computed once per case and radius, shared by the tests, never modified"""
    case = gc.CASES[name]()
    o = helpers.oracle_ba()
    synth.upload(o, case["prob"])
    return sc.reference(case["prob"], o, radius, case["mask0"], want_step=False)


@pytest.mark.gpu
@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
@pytest.mark.parametrize("name", sorted(gc.CASES))
def test_reduced_system(name, geometry, monkeypatch):
    knob, cols = GEOMETRIES[geometry]
    case = gc.CASES[name]()
    g = handle(monkeypatch, knob)
    synth.upload(g, case["prob"])
    for radius in sc.RADII:
        ref = _reference(name, radius)
        S, b = g.debug_reduced_system(radius)
        assert S.shape == ref["S"].shape
        eS, eb = sc.entry_error(S, ref["S"], ref["A_S"]), sc.entry_error(b, ref["b"], ref["A_b"])
        print("%s %s radius %g: e(S) = %.3g (bound %.3g), e(b) = %.3g (bound %.3g)" % (name, geometry, radius, eS, sc.bound(name, "S", gc.TABLE), eb, sc.bound(name, "b", gc.TABLE)))
        assert sc.exact_zeros(S, ref["S"]) and sc.exact_zeros(b, ref["b"]), "an entry outside the structure is not exactly zero"
        assert eS <= sc.bound(name, "S", gc.TABLE) and eb <= sc.bound(name, "b", gc.TABLE)
    st = g.problem_stats()
    assert st["schur_group_cols"] == cols, "the handle did not take the %s geometry" % geometry
    assert st["schur_pairs_blocks"] == case["predict"]["schur_pairs_blocks"]      # the far-pair route does not depend on the geometry
    if geometry == "narrow":
        # the handle cut its work lists into exactly the batches the restated rule gives: with it, the one workgroup of the long list streamed the
        # five (ten) 24 KB batches predicted for it, and both LDS buffers turned over
        batches = case["predict"]["narrow_batches"]
        print(name, "batches", int(st["schur_batches"]), "predicted", sum(sum(v) for v in batches.values()), "long list", batches[(gc.BIG_CHUNK, gc.BIG_GROUP)])
        assert st["schur_batches"] == sum(sum(v) for v in batches.values()), "batches of k_schur_window, narrow geometry"
        assert len(batches[(gc.BIG_CHUNK, gc.BIG_GROUP)]) == 1 and batches[(gc.BIG_CHUNK, gc.BIG_GROUP)][0] >= 3
    g.close()


def _solve(monkeypatch, prob, knob, deterministic, steps=3):
    ba = handle(monkeypatch, knob, deterministic)
    synth.upload(ba, prob)
    ba.solve(helpers.ba_params(max_it=steps, ftol=0.0, gtol=0.0, ptol=0.0))
    out = records(ba), ba.get_poses(), ba.get_points(), ba.get_objects(), int(ba.problem_stats()["schur_group_cols"])
    ba.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(gc.CASES))
def test_three_iterations_narrow_against_wide(name, monkeypatch):
    prob = gc.CASES[name]()["prob"]
    new, pn, _, _, cn = _solve(monkeypatch, prob, GEOMETRIES["narrow"][0], False)
    old, po, _, _, co = _solve(monkeypatch, prob, GEOMETRIES["wide"][0], False)
    assert (cn, co) == (3, 5) and len(new) == len(old) == 4
    same_record(new[0], old[0], BAR, name + " start")
    same_record(new[1], old[1], BAR, name + " step 1")
    for k in (2, 3):     # from the second step on: the spread between two fp64 realisations of a step on a default handle (tests/test_gpu_pose_lin_reuse.py)
        print("%s step %d: cost %.2e" % (name, k, rel(new[k][3], old[k][3])))
        assert new[k][:3] == old[k][:3] and rel(new[k][3], old[k][3]) <= 1e-2


@pytest.mark.gpu
def test_a_deterministic_handle_ignores_the_knob(monkeypatch):
    """poses, features, objects and iteration costs, bit for bit, with the knob unset, at narrow and at wide; the plan is the wide geometry's every time"""
    prob = synth.make_problem(P=40, L=1500, O=3, seed=17, const_poses=2, min_obj_obs=4, object_classes=("bench",), bbox_noise=5.0)
    runs = [_solve(monkeypatch, prob, knob, True) for knob in (None, GEOMETRIES["narrow"][0], GEOMETRIES["wide"][0])]
    for rec, poses, points, objects, cols in runs:
        assert cols == 5
        assert np.array_equal(np.array([r[3] for r in rec]), np.array([r[3] for r in runs[0][0]]))
        assert rec == runs[0][0]
        assert np.array_equal(poses, runs[0][1]) and np.array_equal(points, runs[0][2]) and np.array_equal(objects, runs[0][3])


def test_resources_of_the_strip_kernels():
    strips = _one(kernel_metadata(), "k_schur_window")
    narrow = {n: k for n, k in strips.items() if "SchurNarrow" in n}
    wide = {n: k for n, k in strips.items() if "SchurWide" in n}
    assert len(narrow) == 2 and len(wide) == 2 and len(strips) == 4, sorted(strips)      # TWIN true and false of either geometry
    for n, k in strips.items():
        print(n, k[".vgpr_count"], k[".group_segment_fixed_size"], k[".private_segment_fixed_size"])
    for n, k in narrow.items():      # three workgroups per CU: three wavefronts on every SIMD
        assert 3 * _alloc(k) <= SIMD_VGPRS, (n, k[".vgpr_count"])
        assert 3 * k[".group_segment_fixed_size"] <= CU_LDS_BYTES, (n, k[".group_segment_fixed_size"])
        assert k[".private_segment_fixed_size"] == 0, (n, k[".private_segment_fixed_size"])
    for n, k in wide.items():        # the kernel every deterministic handle runs: what it was before the geometry became a parameter
        assert (k[".vgpr_count"], k[".group_segment_fixed_size"], k[".private_segment_fixed_size"]) == (WIDE_VGPRS, WIDE_LDS, WIDE_PRIVATE), n
