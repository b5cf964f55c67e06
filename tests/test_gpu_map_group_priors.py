"""GPU (-m gpu): joint map priors on groups of objects (include/obvi_map_group_prior.h, factor type 10) through the C ABI.  The CPU oracle does not
know the factor, so the reference is exact linear algebra in numpy, in the style of test_gpu_map_pair_priors.py (whose helpers are used): Lambda = C^-1
comes out of long-double arithmetic (fp64 inverse + Newton-Schulz steps) and is first held against the plain fp64 evaluation of the same formula to 1e-12,
so that the bars below measure the device.  Base problem: that file's own, 9 variable poses + 5 objects (od = 7: 89 rows, object blocks on both sides of the
64-row tile edge and across it), groups {0, 3, 1} (far from its mean: w < 1) and {4, 2}.  Large group: an objects-only problem of 30 objects in ONE group
(od 7: 210 rows = three full 64-row slabs + a ragged one of 18; od 9: 270 rows, five tile rows).
Bars: linearisation 1e-12, reduced system 1e-11 of the largest entry, LM trajectory 1e-8, covariances 1e-9."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (loaded before libobvi_ba.so: torch brings its own HIP runtime, and the one that is loaded first is the one that finds the device)

import helpers
import obvi_ba
from helpers import rel_err
from test_gpu_map_pair_priors import base_problem, inv_ld, object_rows, objects_only, product, spd

pytestmark = pytest.mark.gpu

T = obvi_ba.FACTOR_MAP_GROUP_PRIOR
LD = np.longdouble
GROUPS = ([0, 3, 1], [4, 2])


# ---- the numpy reference ---------------------------------------------------------------------------------------------------------------
def reference(gp, objects):
    """Per group: Lambda, d, Lambda d, s = d^T Lambda d, the Huber weight w and rho -- long double, checked against fp64, handed out as fp64."""
    out = []
    for members, mean, cov in zip(gp["groups"], gp["means"], gp["covs"]):
        L = inv_ld(cov)
        L64 = np.linalg.inv(cov)
        d = (objects[members] - mean).ravel()
        Ld, s = L @ d.astype(LD), d.astype(LD) @ L @ d.astype(LD)
        assert np.abs(L64 - L).max() <= 1e-12 * np.abs(L).max() and np.abs(L64 @ d - Ld).max() <= 1e-12 * np.abs(Ld).max() and abs(d @ L64 @ d - s) <= 1e-12 * s
        s = float(s); h = gp["huber"]
        w = 1.0 if s <= h * h else h / np.sqrt(s)
        rho = s if s <= h * h else 2.0 * h * np.sqrt(s) - h * h
        out.append(dict(L=L.astype(np.float64), d=d, Ld=Ld.astype(np.float64), s=s, w=w, rho=rho))
    return out


def make_groups(prob, od, seed=7, huber=2.0):
    rng = np.random.default_rng(seed)
    obj = prob["objects"]
    means = [obj[GROUPS[0]] - rng.normal(scale=3.0, size=(3, od)), obj[GROUPS[1]] - rng.normal(scale=0.02, size=(2, od))]
    return dict(groups=[list(g) for g in GROUPS], means=means, covs=[spd(rng, 3 * od), spd(rng, 2 * od)], huber=huber)


def set_groups(ba, gp):
    ba.set_map_group_priors(gp["groups"], gp["means"], gp["covs"], gp["huber"])


def scatter(ref, groups, rows, m, od):
    E, e = np.zeros((m, m)), np.zeros(m)
    for f, members in zip(ref, groups):
        for x, a in enumerate(members):
            if rows[a] < 0:
                continue
            e[rows[a]:rows[a] + od] += f["w"] * f["Ld"][od * x:od * x + od]
            for y, b in enumerate(members):
                if rows[b] >= 0:
                    E[rows[a]:rows[a] + od, rows[b]:rows[b] + od] += f["w"] * f["L"][od * x:od * x + od, od * y:od * y + od]
    return E, e


def signs(ba, prob, rows, od, S0, b0):
    """The signs of the two sides of debug_reduced_system, read off a type-4 prior on object 0."""
    rng = np.random.default_rng(5)
    C4, m4 = spd(rng, od), prob["objects"][0] + 0.03
    ba.set_ltm_priors([0], m4[None], C4.reshape(1, -1), 1e6)
    S4, b4 = ba.debug_reduced_system(1e300)
    ba.set_ltm_priors(np.zeros(0, np.uint32), np.zeros((0, od)), np.zeros((0, od * od)), 1.0)
    L4 = np.linalg.inv(C4)
    o0 = slice(rows[0], rows[0] + od)
    sH, sg = np.sign(np.trace((S4 - S0)[o0, o0])), np.sign((b4 - b0)[o0] @ (L4 @ (prob["objects"][0] - m4)))
    assert rel_err((S4 - S0)[o0, o0], sH * L4) < 1e-9 and sH != 0 and sg != 0
    return sH, sg


def records(ba):
    return [(i.iteration, i.step_is_successful, i.cost, i.cost_change, i.gradient_max_norm, i.gradient_norm, i.step_norm, i.relative_decrease, i.trust_region_radius)
            for i in ba.iterations()]


# ---- 1. linearisation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("od", [7, 9])
def test_linearisation_is_the_information_matrix(od):
    prob = base_problem(od)
    gp = make_groups(prob, od)
    ba = product(prob)
    set_groups(ba, gp)
    r, W, J1 = ba.debug_linearize(T)
    assert J1 is None and [len(x) for x in r] == [3 * od, 2 * od] and [w.shape for w in W] == [(3 * od, 3 * od), (2 * od, 2 * od)]
    for g, f in enumerate(reference(gp, prob["objects"])):
        errs = (rel_err(W[g].T @ W[g], f["L"]), rel_err(W[g].T @ r[g], f["Ld"]), abs(r[g] @ r[g] - f["s"]) / f["s"])
        print("od %d group %d: J^T J %.2e  J^T r %.2e  |r|^2 %.2e" % ((od, g) + errs))
        assert max(errs) < 1e-12, (g, errs)
        assert not np.triu(W[g], 1).any() and (np.diag(W[g]) > 0).all()                # the inverse Cholesky factor: lower triangular


# ---- 2. reduced system and cost ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["default", "object_constant", "nine", "deterministic"])
def test_reduced_system_gains_w_lambda(variant):
    od = 9 if variant == "nine" else 7
    prob = base_problem(od)
    if variant == "object_constant":
        prob = dict(prob, object_const=np.array([0, 0, 0, 1, 0], np.uint8))        # object 3: the middle member of {0, 3, 1}
    gp = make_groups(prob, od)
    ref = reference(gp, prob["objects"])
    assert ref[0]["w"] < 1.0 and ref[1]["w"] == 1.0
    rows, m = object_rows(prob, od)
    ba = product(prob, deterministic=(variant == "deterministic"))
    S0, b0 = ba.debug_reduced_system(1e300)
    c0 = [ba.evaluate(loss) for loss in (True, False)]
    assert S0.shape == (m, m) and (variant != "default" or m == 89)
    sH, sg = signs(ba, prob, rows, od, S0, b0)
    set_groups(ba, gp)
    assert ba._fn("ba_num_factors")(ba._h, C.c_int32(T)) == 2
    S1, b1 = ba.debug_reduced_system(1e300)
    E, e = scatter(ref, gp["groups"], rows, m, od)
    eS, eb = np.abs(S1 - S0 - sH * E).max() / np.abs(S1).max(), np.abs(b1 - b0 - sg * e).max() / np.abs(b1).max()
    print("%s: lhs %.2e  rhs %.2e  (m = %d, w = %s)" % (variant, eS, eb, m, [f["w"] for f in ref]))
    assert eS < 1e-11 and eb < 1e-11
    # evaluate: the base value plus sum rho / 2 (with loss) or sum s / 2 (without); residuals (k od per group) and one norm per group behind what was there
    nrow = 5 * od
    for (cb, rb, qb), loss in zip(c0, (True, False)):
        c1, r1, q1 = ba.evaluate(loss)
        add = 0.5 * sum(f["rho"] if loss else f["s"] for f in ref)
        print("%s: cost, loss %d: %.2e" % (variant, loss, abs(c1 - cb - add) / c1))
        assert abs(c1 - cb - add) <= 1e-12 * c1
        assert len(r1) == len(rb) + nrow == ba._fn("ba_num_residuals")(ba._h) and len(q1) == len(qb) + 2
        assert np.array_equal(r1[:len(rb)], rb) and np.array_equal(q1[:len(qb)], qb)
        assert rel_err(q1[len(qb):], [f["s"] for f in ref]) < 1e-12
        tail = r1[len(rb):]
        got = [(tail[:3 * od] ** 2).sum(), (tail[3 * od:] ** 2).sum()]
        assert rel_err(got, [f["s"] * (f["w"] if loss else 1.0) for f in ref]) < 1e-12
    # the reduced program counts the factor's residuals: a group with a variable member has k od of them
    s0 = product(prob).solve(helpers.ba_params(max_it=1))
    s1 = ba.solve(helpers.ba_params(max_it=1))
    assert s1.num_residuals_reduced == s0.num_residuals_reduced + nrow and s1.reduced_system_size == m
    assert abs(s1.initial_cost - s0.initial_cost - 0.5 * sum(f["rho"] for f in ref)) <= 1e-12 * s1.initial_cost
    # masking a group takes exactly its part out again
    ba2 = product(prob, deterministic=(variant == "deterministic"))
    set_groups(ba2, gp)
    ba2.set_active_mask(T, [0, 1])
    S2, b2 = ba2.debug_reduced_system(1e300)
    E2, e2 = scatter(ref[1:], gp["groups"][1:], rows, m, od)
    assert np.abs(S2 - S0 - sH * E2).max() < 1e-11 * np.abs(S2).max() and np.abs(b2 - b0 - sg * e2).max() < 1e-11 * np.abs(b2).max()


def test_all_members_constant_is_fixed_cost_and_a_lone_member_is_a_variable():
    prob = dict(base_problem(), object_const=np.array([0, 0, 1, 0, 1], np.uint8))      # {4, 2}: both constant
    gp = make_groups(prob, 7)
    ref = reference(gp, prob["objects"])
    ba0, ba1 = product(prob), product(prob)
    set_groups(ba1, gp)
    prm = helpers.ba_params(max_it=2)
    s0, s1 = ba0.solve(prm), ba1.solve(prm)
    assert abs(s1.fixed_cost - s0.fixed_cost - 0.5 * ref[1]["rho"]) <= 1e-12 * s1.fixed_cost
    assert s1.num_residuals_reduced == s0.num_residuals_reduced + 21
    assert abs(s1.initial_cost - s0.initial_cost - 0.5 * sum(f["rho"] for f in ref)) <= 1e-12 * s1.initial_cost
    # objects that nothing but a group prior touches are variables of the solve, and the solve puts them on the mean
    rng = np.random.default_rng(3)
    mu = rng.normal(size=(3, 7))
    lone = objects_only(mu + 0.1)
    lone.set_map_group_priors([[2, 0, 1]], [mu[[2, 0, 1]]], [spd(rng, 21)], 1e6)
    s = lone.solve(helpers.ba_params(max_it=50, ftol=0.0, gtol=0.0, ptol=0.0))
    assert s.reduced_system_size == 21 and np.abs(lone.get_objects() - mu).max() < 1e-9


# ---- 3. a group of two is a joint pair prior ------------------------------------------------------------------------------------------------
def test_a_group_of_two_is_a_joint_pair_prior():
    prob = base_problem()
    rng = np.random.default_rng(13)
    a, b = 1, 3
    Cj = spd(rng, 14)
    mean = prob["objects"][[a, b]] - rng.normal(scale=1.0, size=(2, 7))                # outside the Huber region: w < 1 at the start
    grp, pair = product(prob), product(prob)
    grp.set_map_group_priors([[a, b]], [mean], [Cj], 2.0)
    pair.set_map_pair_priors([a], [b], mean[:1], mean[1:], Cj[None], None, 2.0)
    for radius in (100.0, 0.5):
        Sg, bg = grp.debug_reduced_system(radius); Sp, bp = pair.debug_reduced_system(radius)
        print("radius %g: lhs %.2e rhs %.2e" % (radius, rel_err(Sg, Sp), rel_err(bg, bp)))
        assert rel_err(Sg, Sp) < 1e-11 and rel_err(bg, bp) < 1e-11
    prm = helpers.ba_params(max_it=40)
    sg, sp = grp.solve(prm), pair.solve(prm)
    assert sg.termination_type == sp.termination_type and sg.num_iterations == sp.num_iterations and sg.num_iterations > 4
    assert sg.num_residuals_reduced == sp.num_residuals_reduced
    for x, y in zip(grp.iterations(), pair.iterations()):
        assert x.step_is_successful == y.step_is_successful and abs(x.cost - y.cost) <= 1e-8 * y.cost
    for x, y in zip(grp.get_state(), pair.get_state()):
        assert np.abs(x - y).max() < 1e-8


# ---- 4. a block-diagonal group is type-4 priors ---------------------------------------------------------------------------------------------
def test_a_block_diagonal_group_is_ltm_priors():
    prob = base_problem()
    rng = np.random.default_rng(11)
    members = [1, 4, 3]
    blocks = [spd(rng, 7) for _ in members]
    Cg = np.zeros((21, 21))
    for k, B in enumerate(blocks):
        Cg[7 * k:7 * k + 7, 7 * k:7 * k + 7] = B
    mean = prob["gt_objects"][members] + np.array([0.05, -0.05, 0.02])[:, None]
    grp, ltm = product(prob), product(prob)
    grp.set_map_group_priors([members], [mean], [Cg], 1e6)                            # all inside the Huber region
    ltm.set_ltm_priors(members, mean, np.stack([B.ravel() for B in blocks]), 1e6)
    for radius in (100.0, 0.5):
        Sg, bg = grp.debug_reduced_system(radius); St, bt = ltm.debug_reduced_system(radius)
        print("radius %g: lhs %.2e rhs %.2e" % (radius, rel_err(Sg, St), rel_err(bg, bt)))
        assert rel_err(Sg, St) < 1e-11 and rel_err(bg, bt) < 1e-11
    prm = helpers.ba_params(max_it=40)
    sg, st = grp.solve(prm), ltm.solve(prm)
    assert sg.termination_type == st.termination_type and sg.num_iterations == st.num_iterations and sg.num_iterations > 4
    assert sg.num_residuals_reduced == st.num_residuals_reduced
    for x, y in zip(grp.iterations(), ltm.iterations()):
        assert x.step_is_successful == y.step_is_successful and abs(x.cost - y.cost) <= 1e-8 * y.cost
    for x, y in zip(grp.get_state(), ltm.get_state()):
        assert np.abs(x - y).max() < 1e-8


# ---- 5. one group of 30 objects -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("od", [7, 9])
def test_one_group_of_thirty_objects(od):
    """210 rows (od 7: slabs of 64, 64, 64 and 18 rows, four tile rows of S) or 270 (od 9: five tile rows).  The members go in an order of their own, and
    objects 3 and 17 also carry a type-4 prior: every member pair is on the tile pattern, and the covariance of all pairs is the inverse of Lambda plus the
    other factors."""
    O = 30
    rng = np.random.default_rng(41 + od)
    n = O * od
    Cg = spd(rng, n)
    order = rng.permutation(O)
    mu = rng.normal(size=(O, od))
    ba = objects_only(mu + rng.normal(scale=0.05, size=(O, od)), od)
    ba.set_map_group_priors([list(order)], [mu[order]], [Cg], 1e6)
    C4 = np.stack([spd(rng, od, cond=10.0, scale=1e-2) for _ in range(2)])
    ba.set_ltm_priors([3, 17], mu[[3, 17]], C4.reshape(2, -1), 1e6)
    # the information in object-index order: Lambda permuted, plus the two diagonal blocks
    perm = np.concatenate([np.arange(od * o, od * o + od) for o in order])             # row of the group -> row in index order
    info = np.zeros((n, n), dtype=LD)
    info[np.ix_(perm, perm)] = inv_ld(Cg)
    for o, c in zip((3, 17), C4):
        info[od * o:od * o + od, od * o:od * o + od] += inv_ld(c)
    Sigma = inv_ld(info).astype(np.float64)
    assert np.abs(np.linalg.inv(info.astype(np.float64)) - Sigma).max() <= 1e-12 * np.abs(Sigma).max()
    ia, ib = np.repeat(np.arange(O), O), np.tile(np.arange(O), O)
    cov = ba.object_covariances(ia, ib)
    worst = max(rel_err(c, Sigma[od * i:od * i + od, od * j:od * j + od]) for i, j, c in zip(ia, ib, cov))
    print("od %d: %d rows, worst block of Sigma %.2e" % (od, n, worst))
    assert worst < 1e-9
    ba.covariance_compute()
    assert ba.covariance_on_pattern(np.full(O * O, 2), ia, np.full(O * O, 2), ib).all()
    s = ba.solve(helpers.ba_params(max_it=50, ftol=0.0, gtol=0.0, ptol=0.0))
    assert s.reduced_system_size == n and np.abs(ba.get_objects() - mu).max() < 1e-9
    # the linearisation at this size: ragged last slab, rows of W longer than a wavefront
    ba.set_objects(mu + rng.normal(scale=0.05, size=(O, od)), np.zeros(O, np.uint8))
    x = ba.get_objects()
    r, W, _ = ba.debug_linearize(T)
    L = inv_ld(Cg)
    d = (x[order] - mu[order]).ravel()
    errs = (rel_err(W[0].T @ W[0], L.astype(np.float64)), rel_err(W[0].T @ r[0], (L @ d.astype(LD)).astype(np.float64)), abs(r[0] @ r[0] - float(d.astype(LD) @ L @ d.astype(LD))) / (r[0] @ r[0]))
    print("od %d: J^T J %.2e  J^T r %.2e  |r|^2 %.2e" % ((od,) + errs))
    assert max(errs) < 1e-12


# ---- 6. round trip ----------------------------------------------------------------------------------------------------------------------------
def test_round_trip_of_the_whole_map_through_the_covariance_call():
    prob = base_problem()
    src = product(prob)
    src.solve(helpers.ba_params(max_it=15))
    O, od = 5, 7
    ia, ib = np.repeat(np.arange(O), O), np.tile(np.arange(O), O)
    blk = src.object_covariances(ia, ib)
    Sigma = np.block([[blk[O * i + j] for j in range(O)] for i in range(O)])
    Sigma = 0.5 * (Sigma + Sigma.T)
    ev = np.linalg.eigvalsh(Sigma)
    mean = src.get_objects()
    dst = objects_only(mean + 0.01)
    dst.set_map_group_priors([list(range(O))], [mean], [Sigma], 1e6)
    back = dst.object_covariances(ia, ib)
    got = np.block([[back[O * i + j] for j in range(O)] for i in range(O)])
    print("round trip: %.2e (condition number of Sigma_oo %.2e)" % (rel_err(got, Sigma), ev[-1] / ev[0]))
    assert rel_err(got, Sigma) < 1e-9


# ---- 7. evaluate, selection and masks ---------------------------------------------------------------------------------------------------------
def test_evaluate_order_selection_and_masks_on_a_planned_handle():
    """The residuals and norms of type 10 come after those of type 9; obvi_ba_select_outliers on type 10 follows the rule it follows on type 4 (helpers.map_rule
    on the un-robustified block norms); a mask change on a planned handle takes a group out (subset: the plan stays) and puts it back (superset: a new plan)."""
    prob = base_problem()
    rng = np.random.default_rng(19)
    gp = dict(groups=[[0, 3], [1], [4, 2]], huber=2.0, covs=[spd(rng, 14), spd(rng, 7), spd(rng, 14)],
              means=[prob["objects"][[0, 3]] - rng.normal(scale=3.0, size=(2, 7)), prob["objects"][[1]] - 0.01, prob["objects"][[4, 2]] - 0.02])
    ref = reference(gp, prob["objects"])
    base = product(prob).evaluate(True)[0]
    ba = product(prob)
    Cp = spd(rng, 14)
    ba.set_map_pair_priors([3], [1], prob["objects"][[3]] - 0.01, prob["objects"][[1]] + 0.01, Cp[None], None, 2.0)   # (3 and 1 are in different groups)
    cp, rp, qp = ba.evaluate(True)
    set_groups(ba, gp)
    assert ba.num_factors(T) == 3 and ba._fn("ba_num_factors")(ba._h, C.c_int32(T)) == 3
    c1, r1, q1 = ba.evaluate(True)
    assert len(r1) == len(rp) + 35 and len(q1) == len(qp) + 3
    assert np.array_equal(r1[:len(rp)], rp) and np.array_equal(q1[:len(qp)], qp)      # type 9 and everything before it stay where they were
    assert rel_err(q1[-3:], [f["s"] for f in ref]) < 1e-12
    bounds = [0, 14, 21, 35]
    for g, f in enumerate(ref):
        assert abs((r1[len(rp) + bounds[g]:len(rp) + bounds[g + 1]] ** 2).sum() - f["w"] * f["s"]) <= 1e-12 * f["s"]
    assert abs(c1 - cp - 0.5 * sum(f["rho"] for f in ref)) <= 1e-12 * c1
    ba.set_map_pair_priors(np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros((0, 7)), np.zeros((0, 7)), np.zeros((0, 196)))

    def summary():                                                                  # one LM iteration for the reduced program's counts, the state put back
        ba.snapshot()
        s = ba.solve(helpers.ba_params(max_it=1))
        ba.restore()
        return s
    s_all = summary()                                                               # (this also plans the handle)
    sq = ba.evaluate(False)[2][-3:]
    for fraction in (0.34, 0.7):
        mask, n_out = ba.select_outliers(T, fraction)
        want, want_n = helpers.map_rule(sq, np.ones(3), fraction)
        assert n_out == want_n and list(mask) == list(want) and n_out == int(3 * fraction)
    mask, _ = ba.select_outliers(T, 0.34)
    assert list(mask) == [0, 1, 1]                                                  # the far group goes
    ba.set_active_mask(T, mask)
    c2 = ba.evaluate(True)[0]
    assert abs(c2 - base - 0.5 * (ref[1]["rho"] + ref[2]["rho"])) <= 1e-12 * c2
    s_sub = summary()
    assert s_sub.num_residuals_reduced == s_all.num_residuals_reduced - 14 and abs(s_sub.initial_cost - c2) <= 1e-12 * c2
    m2, n2 = ba.select_outliers(T, 0.5)                                             # the masked group is not a candidate: one of the two that are left goes
    assert n2 == 1 and list(m2) == list(helpers.map_rule(sq, mask, 0.5)[0]) and m2[0] == 0 and sorted(m2[1:]) == [0, 1]
    ba.set_active_mask(T, [1, 1, 1])
    c3 = ba.evaluate(True)[0]
    s_back = summary()
    assert abs(c3 - base - 0.5 * sum(f["rho"] for f in ref)) <= 1e-12 * c3 and s_back.num_residuals_reduced == s_all.num_residuals_reduced
    rows, m = object_rows(prob, 7)
    plain = product(prob)
    S0, b0 = plain.debug_reduced_system(1e300)
    sH, sg = signs(plain, prob, rows, 7, S0, b0)
    S1, b1 = ba.debug_reduced_system(1e300)
    E, e = scatter(ref, gp["groups"], rows, m, 7)
    assert np.abs(S1 - S0 - sH * E).max() < 1e-11 * np.abs(S1).max() and np.abs(b1 - b0 - sg * e).max() < 1e-11 * np.abs(b1).max()


def test_shrinking_the_mask_keeps_the_plan_and_growing_it_replans():
    """A group alone puts its member pairs on the tile pattern.  Planned with the group masked, the pattern lacks the pair; unmasking replans (the pair appears),
    masking again keeps that plan (the pair stays on the pattern although no active factor marks it)."""
    od, O = 7, 30
    rng = np.random.default_rng(31)
    mu = rng.normal(size=(O, od))
    ba = objects_only(mu + 0.05)
    ba.set_ltm_priors(np.arange(O), mu, np.stack([spd(rng, od, cond=10.0).ravel() for _ in range(O)]), 1e6)
    ba.set_map_group_priors([[0, 29]], [mu[[0, 29]]], [spd(rng, 14, cond=10.0)], 1e6)

    def on_pattern():
        ba.covariance_compute()
        return int(ba.covariance_on_pattern([2], [0], [2], [29])[0])
    ba.set_active_mask(T, [0])
    assert on_pattern() == 0                                                        # 30 objects in index order: tile (3, 0) holds nothing
    ba.set_active_mask(T, [1])
    assert on_pattern() == 1                                                        # grown: a new plan, the members last and the pair marked
    ba.set_active_mask(T, [0])
    assert on_pattern() == 1                                                        # shrunk: the plan is kept
    s = ba.solve(helpers.ba_params(max_it=50, ftol=0.0, gtol=0.0, ptol=0.0))
    assert s.num_residuals_reduced == O * od and np.abs(ba.get_objects() - mu).max() < 1e-9


# ---- 8. deterministic ---------------------------------------------------------------------------------------------------------------------------
def test_deterministic_handle_repeats_bit_for_bit():
    prob = base_problem()
    gp = make_groups(prob, 7)

    def run():
        ba = product(prob, deterministic=True)
        set_groups(ba, gp)
        s = ba.solve(helpers.ba_params(max_it=12))
        ia, ib = np.repeat(np.arange(5), 5), np.tile(np.arange(5), 5)
        return (s.num_iterations, s.termination_type, s.initial_cost, s.final_cost, s.fixed_cost), records(ba), ba.get_state(), ba.object_covariances(ia, ib)
    (s1, i1, x1, c1), (s2, i2, x2, c2) = run(), run()
    assert s1 == s2 and i1 == i2 and s1[0] > 3
    for u, v in zip(x1, x2):
        assert np.array_equal(u, v)
    assert np.array_equal(c1, c2)


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    prob = base_problem()
    ba = product(prob)
    rng = np.random.default_rng(1)
    m = prob["objects"]

    def status(groups, covs=None):
        try:
            ba.set_map_group_priors(groups, [m[np.minimum(g, 4)] for g in groups], [spd(rng, 7 * len(g)) for g in groups] if covs is None else covs, 1.0)
        except obvi_ba.ObviError as e:
            return int(str(e).split("status ")[1].split()[0])
        return 0
    assert status([[0, 1, 2]]) == 0
    f = ba._lib.obvi_map_set_group_priors
    f.restype = C.c_int
    ok = [np.array([0, 2], np.int64), np.array([0, 1], np.uint32), np.ascontiguousarray(m[:2]), np.ascontiguousarray(spd(rng, 14))]
    ptrs = [x.ctypes.data_as(C.c_void_p) for x in ok]
    for k in range(4):                                                                  # every required pointer null in turn
        assert f(ba._h, C.c_int64(1), *[None if j == k else p for j, p in enumerate(ptrs)], C.c_double(1.0)) == -1, k
    assert f(ba._h, C.c_int64(-1), *ptrs, C.c_double(1.0)) == -1

    def raw(ptr, idx, rows):
        p, i = np.array(ptr, np.int64), np.array(idx, np.uint32)
        mu, cv = np.zeros((max(len(i), 1), 7)), np.concatenate([spd(rng, r).ravel() for r in rows])
        return f(ba._h, C.c_int64(len(p) - 1), p.ctypes.data_as(C.c_void_p), i.ctypes.data_as(C.c_void_p), mu.ctypes.data_as(C.c_void_p), cv.ctypes.data_as(C.c_void_p), C.c_double(1.0))
    assert raw([0, 2, 1], [0, 1], [14, 7]) == -1                                        # group_ptr decreases
    assert raw([1, 2], [0, 1], [7]) == -1                                               # ... does not start at 0
    assert raw([0, 1, 1], [0], [7, 7]) == -1                                            # an empty group
    assert status([[0, 1, 0]]) == -1                                                    # an object twice in one group
    assert status([[0, 1], [2, 1]]) == -1                                               # ... in two groups
    assert status([[0, 5]]) == -4 and status([[7]]) == -4                               # an index >= O
    bad = spd(rng, 14); bad[3, 3] = -1.0
    assert status([[0, 1]], [bad]) == -6                                                # not SPD
    semi = np.zeros((14, 14)); semi[:7, :7] = np.eye(7)
    assert status([[0, 1]], [semi]) == -6
    Q, _ = np.linalg.qr(rng.normal(size=(14, 14)))
    ill = (Q * np.logspace(0, -15, 14)) @ Q.T
    assert status([[0, 1]], [0.5 * (ill + ill.T)]) == -6                                # condition number 1e15
    nan = spd(rng, 14); nan[2, 5] = nan[5, 2] = np.nan
    assert status([[0, 1]], [nan]) == -6
    assert ba._fn("ba_num_factors")(ba._h, C.c_int32(T)) == 1                           # a refused call leaves the group that was there
    ba.solve(helpers.ba_params(max_it=2))                                               # ... and the handle usable
    # a group above the cap: 293 objects x 7 = 2051 rows (refused before the covariance is read)
    big = objects_only(np.zeros((293, 7)))
    p, i = np.array([0, 293], np.int64), np.arange(293, dtype=np.uint32)
    one = np.zeros(1)
    assert f(big._h, C.c_int64(1), p.ctypes.data_as(C.c_void_p), i.ctypes.data_as(C.c_void_p), np.zeros((293, 7)).ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p), C.c_double(1.0)) == -1
    ba.reset()
    assert ba._fn("ba_num_factors")(ba._h, C.c_int32(T)) == 0 and ba.num_factors(T) == 0
    # a pair prior inside a group: refused when the problem is validated, whichever was set first; the handle works again once either is gone
    for first in ("pair", "group"):
        ba = product(prob)
        setters = dict(pair=lambda: ba.set_map_pair_priors([3], [0], m[[3]], m[[0]], spd(rng, 14)[None]), group=lambda: ba.set_map_group_priors([[0, 3, 1], [4, 2]], [m[[0, 3, 1]], m[[4, 2]]], [spd(rng, 21), spd(rng, 14)]))
        setters[first](); setters["group" if first == "pair" else "pair"]()
        for call in (ba.prepare, lambda: ba.solve(helpers.ba_params(max_it=2)), lambda: ba.evaluate()):
            with pytest.raises(obvi_ba.ObviError, match="status -1"):
                call()
        ba.set_map_pair_priors([3], [4], m[[3]], m[[4]], spd(rng, 14)[None])            # across two groups: legal
        ba.solve(helpers.ba_params(max_it=2))
    # a handle that exchanges shared objects refuses the problem before any collective
    calls = []
    ex = product(prob)
    ex.set_map_group_priors([[0, 1]], [m[:2]], [spd(rng, 14)])
    ex.set_shared_objects(np.array([0, 0, 1, 0, 0], np.uint8), 0, 1)
    ex.set_allreduce(lambda buf, count, op, stream: calls.append(count) or 0)
    for call in (ex.prepare, lambda: ex.solve(helpers.ba_params(max_it=2)), lambda: ex.evaluate(), ex.covariance_compute):
        with pytest.raises(obvi_ba.ObviError, match="status -1"):
            call()
    assert calls == []
    ex.set_map_group_priors([], [], [])
    ex.prepare()                                                                        # without group priors the handle is as before


# ---- 10. n_groups = 0 after a set ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deterministic", [False, True])
def test_cleared_groups_leave_no_trace(deterministic):
    prob = base_problem()
    gp = make_groups(prob, 7)
    plain, ba = product(prob, deterministic=deterministic), product(prob, deterministic=deterministic)
    set_groups(ba, gp)
    ba.prepare()
    ba.set_map_group_priors([], [], [])
    assert ba._fn("ba_num_factors")(ba._h, C.c_int32(T)) == 0 and ba._fn("ba_num_residuals")(ba._h) == plain._fn("ba_num_residuals")(plain._h) == len(ba.evaluate()[1])
    prm = helpers.ba_params(max_it=12)
    s0, s1 = plain.solve(prm), ba.solve(prm)
    r0, r1 = records(plain), records(ba)
    assert s0.num_iterations == s1.num_iterations > 3 and s0.num_residuals_reduced == s1.num_residuals_reduced
    if deterministic:
        assert r0 == r1 and s0.final_cost == s1.final_cost
        for u, v in zip(plain.get_state(), ba.get_state()):
            assert np.array_equal(u, v)
    else:                                                                               # (fp64 atomics add in another order from run to run: the LM bar)
        for x, y in zip(r0, r1):
            assert x[:2] == y[:2] and abs(x[2] - y[2]) <= 1e-8 * y[2]
