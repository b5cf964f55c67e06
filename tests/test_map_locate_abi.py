"""CPU: the entry that locates one device-resident map in another (include/obvi_map_locate.h) is declared under the obvi_map_ prefix in a header of its own --
one function and one parameter struct, nothing in the obvi_ba_ namespace the oracle mirrors -- exported by libobvi_ba.so, bound by obvi_ba.Map.locate, and
refuses what it can refuse without a device with its outputs untouched (the refusals that need a handle to read a device and a block size from are in
tests/test_gpu_map_locate.py).  The header includes obvi_map_resident.h alone, no other header names it, and it names none of the neighbouring entries the
other headers' tests reserve for their owners.
And the reference of tests/test_gpu_map_locate.py is itself held: the vectorised long-double evaluation of tests/map_locate_cases.py against a plain-Python
restatement of the header, seed by seed and pair by pair, on the 12-object case; the planted case's best hypothesis has exactly the 8 planted partners, and its
Gauss-Newton result against the Newton yardstick on the full objective, with the derived bars of the cases module; the conditions on the inputs (no deciding
quantity within 1e-9 of its threshold) on every case; numpy's fp64 evaluation of the same definition against the long-double one on every case -- decisions
equal, figures within cases.FP64_WORST, the number DESIGN.md 4c.9 records and the GPU bar is three orders over.

Measured: see DESIGN.md 4c.9."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import helpers
import map_locate_cases as cases
from map_support import header as _header

sys.path.insert(0, helpers.ROOT)
import __graft_entry__ as entry  # noqa: E402

LD = np.longdouble
SYMBOLS = ["obvi_map_locate"]
RESERVED = ["map_merge", "map_match", "map_update", "map_extend", "map_frame", "obvi_map_condition", "obvi_map_get", "obvi_map_extend", "obvi_map_select", "obvi_map_join"]


def test_the_header_declares_the_entry_and_its_struct_and_the_library_exports_it():
    assert entry.abi_symbols("obvi_map_locate.h", "obvi_map_") == SYMBOLS
    assert entry.abi_symbols("obvi_map_locate.h", "obvi_ba_") == []                 # nothing there for the oracle to mirror
    txt = _header("obvi_map_locate.h")
    body = re.search(r"typedef\s+struct\s*\{(.*?)\}\s*obvi_map_locate_params\s*;", txt, flags=re.S).group(1)
    fields = re.findall(r"\b(double|int32_t)\s+(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [("double", "pair_min_distance"), ("double", "pair_tolerance"), ("double", "inlier_gate"), ("int32_t", "min_inliers"), ("int32_t", "refine_iterations")]
    lib = C.CDLL(helpers.PRODUCT_LIB)
    for s in SYMBOLS:
        assert hasattr(lib, s), s


def test_the_header_includes_the_resident_map_alone_and_no_other_header_mentions_it():
    txt = _header("obvi_map_locate.h")
    assert re.findall(r'#include\s+"([^"]+)"', txt) == ["obvi_map_resident.h"]
    for word in RESERVED:
        assert word not in txt, word
    for other in sorted(os.listdir(os.path.join(helpers.ROOT, "include"))):
        if other != "obvi_map_locate.h":
            assert "map_locate" not in _header(other) and "MAP_LOCATE" not in _header(other), other


def test_what_needs_no_device_is_refused_with_the_outputs_untouched():
    import obvi_ba
    lib = C.CDLL(helpers.PRODUCT_LIB)
    lib.obvi_map_locate.restype = C.c_int
    null, fake = C.c_void_p(), C.c_void_p(8)                                        # fake: never dereferenced, the null handle is refused first
    params = obvi_ba.LocateParams(2.0, 0.25, 16.0, 3, 3)
    assert C.sizeof(params) == 32
    counts = np.full(3, 7, np.int64)
    seed, t, inl, cost = np.full((2, 4), 9, np.uint32), np.full((2, 4), 9.0), np.full(2, 9, np.int32), np.full(2, 9.0)
    P = C.c_void_p

    def call(h=null, a=fake, b=fake, p=C.byref(params), cap=2, cnt=counts, s=seed):
        return lib.obvi_map_locate(h, a, b, None, None, p, C.c_int64(cap), None if s is None else s.ctypes.data_as(P), t.ctypes.data_as(P), None, inl.ctypes.data_as(P),
                                   cost.ctypes.data_as(P), None, None if cnt is None else cnt.ctypes.data_as(P))

    for kw in ({}, {"a": null}, {"b": null}, {"p": None}, {"cnt": None}, {"cap": -1}, {"s": None}):
        assert call(**kw) == -1, kw
        assert (counts == 7).all() and (seed == 9).all() and (t == 9.0).all() and (inl == 9).all() and (cost == 9.0).all()


def test_the_python_binding_has_the_method_and_the_result():
    import obvi_ba
    assert callable(getattr(obvi_ba.Map, "locate", None))
    assert obvi_ba.Located._fields == ("seed", "transform", "transform_cov", "inliers", "cost", "partner", "counts", "move")
    assert [f[0] for f in obvi_ba.LocateParams._fields_] == ["pair_min_distance", "pair_tolerance", "inlier_gate", "min_inliers", "refine_iterations"]


# ---- the reference of the GPU tests is itself held --------------------------------------------------------------------------------------------------------
def plain(c, p):
    """The header restated with scalars: (counts, [(seed, T, inliers, cost, partner)] of the hypotheses that qualify, ranked)."""
    od, na, nb = c.od, len(c.mean_a), len(c.mean_b)

    def rec(mean, cov, o):
        blk = [[(LD(cov[od * o + r, od * o + q]) + LD(cov[od * o + q, od * o + r])) * LD(0.5) for q in range(3)] for r in range(3)]
        return [LD(v) for v in mean[o, :3]], blk
    A, B = [rec(c.mean_a, c.cov_a, o) for o in range(na)], [rec(c.mean_b, c.cov_b, o) for o in range(nb)]
    la = [0] * na if c.label_a is None else [int(v) for v in c.label_a]
    lb = [0] * nb if c.label_b is None else [int(v) for v in c.label_b]
    tested = compatible = 0
    found = []
    index = -1
    for a1 in range(na):
        for a2 in range(a1 + 1, na):
            for b1 in range(nb):
                for b2 in range(nb):
                    if b1 == b2:
                        continue
                    index += 1
                    if not (la[a1] == lb[b1] >= 0 and la[a2] == lb[b2] >= 0):
                        continue
                    tested += 1
                    (pa1, _), (pa2, _), (pb1, _), (pb2, _) = A[a1], A[a2], B[b1], B[b2]
                    ux, uy, vx, vy = pa2[0] - pa1[0], pa2[1] - pa1[1], pb2[0] - pb1[0], pb2[1] - pb1[1]
                    nu, nv = np.sqrt(ux * ux + uy * uy), np.sqrt(vx * vx + vy * vy)
                    if not (nu >= p.dmin and nv >= p.dmin and abs(nu - nv) <= p.tol and abs((pa2[2] - pa1[2]) - (pb2[2] - pb1[2])) <= p.tol):
                        continue
                    compatible += 1
                    psi = np.arctan2(vx * uy - vy * ux, vx * ux + vy * uy)
                    cs, sn = np.cos(psi), np.sin(psi)
                    mA, mB = [(pa1[i] + pa2[i]) / 2 for i in range(3)], [(pb1[i] + pb2[i]) / 2 for i in range(3)]
                    T = [mA[0] - (cs * mB[0] - sn * mB[1]), mA[1] - (sn * mB[0] + cs * mB[1]), mA[2] - mB[2], psi]
                    R = [[cs, -sn, 0], [sn, cs, 0], [0, 0, 1]]
                    inl, cost, partner = 0, LD(0), []
                    for b in range(nb):
                        pb, Bb = B[b]
                        q = [sum(R[i][j] * pb[j] for j in range(3)) + T[i] for i in range(3)]
                        RB = [[sum(R[i][k] * Bb[k][m] * R[j][m] for k in range(3) for m in range(3)) for j in range(3)] for i in range(3)]
                        best, who = LD(np.inf), -1
                        for a in range(na):
                            if lb[b] < 0 or la[a] != lb[b]:
                                continue
                            pa, Aa = A[a]
                            S = np.array([[Aa[i][j] + RB[i][j] for j in range(3)] for i in range(3)], dtype=LD)
                            L = cases.chol3(S)
                            e = np.array([pa[i] - q[i] for i in range(3)], dtype=LD)
                            y = cases.forward(L, e[:, None])[:, 0]
                            s = y @ y
                            if s < best:
                                best, who = s, a
                        if best <= p.gate:
                            inl, cost = inl + 1, cost + best
                        partner.append(who if best <= p.gate else -1)
                    if inl >= p.min_inliers:
                        found.append(((a1, a2, b1, b2), T, inl, cost, partner, index))
    found.sort(key=lambda f: (-f[2], f[3], f[5]))
    return (tested, compatible, len(found)), found


def test_the_long_double_reference_is_the_header_restated_in_plain_python():
    c = cases.case(7, 12, "classes")
    p = cases.thresholds(c)
    r = cases.evaluate(c, p)
    counts, found = plain(c, p)
    assert counts == r.counts and counts[2] > 0
    worst = 0.0
    for (seed, T, inl, cost, partner, _), h in zip(found, r.order):
        assert tuple(r.seeds[h]) == seed and r.inliers[h] == inl and list(r.partner[h]) == partner
        worst = max(worst, float(abs(r.cost[h] - cost) / cost), float(np.abs(r.T0[h] - np.array(T, dtype=LD)).max()))
    print("the vectorised long-double reference against the restatement, %d hypotheses: %.2e" % (len(found), worst))
    assert worst <= 1e-15                                                            # two long-double evaluations of sums of a few terms: 1e-19 a term, times the statistic's condition


def test_the_planted_case_finds_its_eight_pairs_and_gauss_newton_ends_at_the_minimiser():
    c = cases.case(7, 70, "classes")
    p = cases.thresholds(c)
    iterations = 8
    r, k, T, cov = cases.report(c, p, iterations, capacity=1)
    best = r.order[0]
    assert r.inliers[best] == cases.N_SHARED and list(r.partner[best]) == list(c.shared) + [-1] * cases.N_EXTRA
    T_star, cov_star, grad = cases.newton(c, r.partner[best])
    gap, hgap = cases.gauss_newton_gap(c, T_star, cov_star, r.partner[best]), cases.hessian_gap(c, T_star, r.partner[best])
    dT = np.abs(T[0] - T_star)
    dC = float(np.abs(cov[0] - cov_star).max() / np.abs(cov_star).max())
    print("the planted case: Gauss-Newton after %d steps against the Newton minimiser (gradient left %.1e): |dT| %s, first-order gap %s; covariance %.2e (bar %.2e); "
          "from the truth: %s" % (iterations, grad, np.asarray(dT, float), np.asarray(gap, float), dC, hgap, np.asarray(np.abs(T_star - cases.T_TRUE), float)))
    assert (dT <= 2 * gap + 1e-9).all()
    assert dC <= hgap
    sig = np.sqrt(np.diag(cov_star).astype(np.float64))
    assert (np.abs(T_star - cases.T_TRUE).astype(np.float64) <= 5 * sig).all()       # and the minimiser is where the maps were made from


ALL_CASES = [cases.case(*e) for e in cases.EXHAUSTIVE] + [cases.case(7, 24, "classes", n_b=k) for k in range(1, 11)] + [cases.case(7, 70, "classes")]


def test_the_conditions_on_the_inputs_hold_and_numpys_fp64_evaluation_stays_within_the_recorded_figure():
    worst = [0.0, 0.0, 0.0]
    for c, p in [(c, cases.thresholds(c)) for c in ALL_CASES] + [(cases.square(), cases.square_thresholds())]:
        r, k, T, cov = cases.report(c, p, 3)
        ties = cases.conditions(c, p, r)
        assert (c.name == "the square") == bool(ties)
        r64, k64, T64, cov64 = cases.report(c, p, 3, dtype=np.float64)
        assert r64.counts == r.counts and np.array_equal(r64.order, r.order) and np.array_equal(r64.inliers, r.inliers) and np.array_equal(r64.partner, r.partner), c.name
        e = cases.errors(r64.cost[r64.order], T64, cov64, r.cost[r.order], T, cov, cost_scale=p.gate if c.name == "the square" else None)
        worst = [max(a, b) for a, b in zip(worst, e)]
    print("numpy's fp64 evaluation against the long-double reference, worst over %d cases: cost %.2e  transform %.2e  covariance %.2e" % ((len(ALL_CASES) + 1,) + tuple(worst)))
    assert max(worst) <= cases.FP64_WORST


def test_the_chain_finds_the_planted_pairs_and_pulls_the_unmatched_objects_into_place():
    """locate -> transform -> join -> match -> resolve -> merge in long double, before any device runs it: nobody supplies the transform."""
    import map_frame_cases as frame
    c, p, ch, ref = cases.chain()
    assert sorted(ref.pairs) == sorted(frame.planted(ch)) and len(ref.pairs) == cases.N_SHARED
    assert sorted(zip(ref.keep.tolist(), ref.drop.tolist())) == sorted(frame.planted(ch))
    d = np.asarray(ch.T_est - ch.T_true, dtype=LD)
    assert d @ np.linalg.inv(cases.WIDE_SIGMA) @ d < 1.0                             # the wide Sigma covers what the located transform is off by
    moved = frame.extra_distances(ch, ref.moved_mean[cases.N_SHARED:])
    fused = frame.extra_distances(ch, ref.fused_mean[len(c.mean_a):])
    print("B's own objects, centre distance from the truth: after the move %s, after the merge %s" % (np.round(moved, 4), np.round(fused, 4)))
    assert len(fused) == cases.N_EXTRA and (fused < moved).all()
