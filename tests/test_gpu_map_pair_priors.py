"""GPU (-m gpu): joint map priors on object pairs (include/obvi_map_prior.h, factor type 9) through the C ABI.  The CPU oracle does not know the
factor, so the reference is exact linear algebra in numpy: the information matrix Lambda of either form comes out of long-double arithmetic
(fp64 inverse + Newton-Schulz steps) and is first held against the plain fp64 evaluation of the same formula to 1e-12, so that the bars below
measure the device.  Base problem: 9 variable poses + 5 objects (od = 7: 54 + 35 = 89 rows -- object blocks on both sides of the 64-row tile
edge, one across it).  Bars: linearisation 1e-12, reduced system 1e-11 of the largest entry, LM trajectory 1e-8, covariances 1e-9."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (loaded before libobvi_ba.so: torch brings its own HIP runtime, and the one that is loaded first is the one that finds the device)

import helpers
import obvi_ba
import synth
from helpers import rel_err
from map_support import objects_only

pytestmark = pytest.mark.gpu

T = obvi_ba.FACTOR_MAP_PAIR_PRIOR
JOINT, COND = obvi_ba.MAP_PAIR_JOINT, obvi_ba.MAP_PAIR_CONDITIONAL
LD = np.longdouble


# ---- the numpy reference ---------------------------------------------------------------------------------------------------------------
def spd(rng, n, cond=1e3, scale=1e-2):
    """Random SPD matrix with eigenvalues in [scale, scale * cond], both ends taken."""
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    ev = scale * np.exp(rng.uniform(0.0, np.log(cond), n))
    ev[0], ev[-1] = scale, scale * cond
    M = (Q * ev) @ Q.T
    return 0.5 * (M + M.T)


def inv_ld(M):
    """Inverse in long double: the fp64 inverse refined by two Newton-Schulz steps (quadratic: the second step leaves only long-double rounding)."""
    M = np.asarray(M, dtype=LD)
    X = np.linalg.inv(M.astype(np.float64)).astype(LD)
    eye = np.eye(len(M), dtype=LD)
    for _ in range(2):
        X = X @ (2 * eye - M @ X)
    return 0.5 * (X + X.T)


def information(Cj, form, od, inv=inv_ld, dtype=LD):
    Cj = np.asarray(Cj, dtype=dtype)
    if form == JOINT:
        return inv(Cj)
    A, B, D = Cj[:od, :od], Cj[:od, od:], Cj[od:, od:]
    K = B.T @ inv(A)
    G = np.concatenate([-K, np.eye(od, dtype=dtype)], axis=1)
    return G.T @ inv(D - K @ B) @ G


def reference(pairs, objects, od):
    """Per factor: Lambda, d, Lambda d, s = d^T Lambda d, the Huber weight w and rho -- long double, checked against fp64, handed out as fp64."""
    out = []
    for i in range(len(pairs["a"])):
        L = information(pairs["cov"][i], pairs["form"][i], od)
        L64 = information(pairs["cov"][i], pairs["form"][i], od, inv=np.linalg.inv, dtype=np.float64)
        d = np.concatenate([objects[pairs["a"][i]] - pairs["mean_a"][i], objects[pairs["b"][i]] - pairs["mean_b"][i]])
        Ld, s = L @ d.astype(LD), d.astype(LD) @ L @ d.astype(LD)
        assert np.abs(L64 - L).max() <= 1e-12 * np.abs(L).max() and np.abs(L64 @ d - Ld).max() <= 1e-12 * np.abs(Ld).max() and abs(d @ L64 @ d - s) <= 1e-12 * s
        s = float(s); h = pairs["huber"]
        w = 1.0 if s <= h * h else h / np.sqrt(s)
        rho = s if s <= h * h else 2.0 * h * np.sqrt(s) - h * h
        out.append(dict(L=L.astype(np.float64), d=d, Ld=Ld.astype(np.float64), s=s, w=w, rho=rho))
    return out


# ---- problems --------------------------------------------------------------------------------------------------------------------------
def base_problem(od=7):
    prob = synth.make_problem(P=10, L=300, O=5, seed=3, object_classes=("bench",), bbox_noise=5.0, min_obj_obs=5)
    return synth.nine_dof(prob, tilt=0.3, seed=2) if od == 9 else prob


def make_pairs(prob, od, seed=7, huber=2.0):
    """(0,1) joint and far from its mean (w < 1), (3,2) conditional, (1,4) joint: five objects, every one in a pair, object 1 in two."""
    rng = np.random.default_rng(seed)
    a, b, form = np.array([0, 3, 1], np.uint32), np.array([1, 2, 4], np.uint32), np.array([JOINT, COND, JOINT], np.uint8)
    obj = prob["objects"]
    off = rng.normal(scale=0.02, size=(3, 2, od))
    off[0] = rng.normal(scale=3.0, size=(2, od))
    return dict(a=a, b=b, form=form, mean_a=obj[a] - off[:, 0], mean_b=obj[b] - off[:, 1], cov=np.stack([spd(rng, 2 * od) for _ in range(3)]), huber=huber)


def product(prob, **opts):
    ba = helpers.product_ba(object_block_size=prob.get("object_block_size", 7), **opts)
    synth.upload(ba, prob)
    return ba


def set_pairs(ba, p):
    ba.set_map_pair_priors(p["a"], p["b"], p["mean_a"], p["mean_b"], p["cov"], p["form"], p["huber"])


def object_rows(prob, od):
    """First row of every variable object in the canonical reduced system (variable poses by index, then objects by index); -1: constant."""
    nPv = int((np.asarray(prob["pose_const"]) == 0).sum())
    rows, nxt = [], 6 * nPv
    for c in prob["object_const"]:
        rows.append(-1 if c else nxt)
        nxt += 0 if c else od
    return rows, nxt


def scatter(ref, pairs, rows, m, od):
    E, e = np.zeros((m, m)), np.zeros(m)
    for f, a, b in zip(ref, pairs["a"], pairs["b"]):
        blk = [(rows[a], 0), (rows[b], od)]
        for rx, ox in blk:
            if rx < 0:
                continue
            e[rx:rx + od] += f["w"] * f["Ld"][ox:ox + od]
            for ry, oy in blk:
                if ry >= 0:
                    E[rx:rx + od, ry:ry + od] += f["w"] * f["L"][ox:ox + od, oy:oy + od]
    return E, e


# ---- 1. linearisation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("od", [7, 9])
def test_linearisation_is_the_information_matrix(od):
    prob = base_problem(od)
    pairs = make_pairs(prob, od)
    ba = product(prob)
    set_pairs(ba, pairs)
    r, J0, J1 = ba.debug_linearize(T)
    assert r.shape == (3, 2 * od) and J0.shape == (3, 2 * od, od) and J1.shape == (3, 2 * od, od)
    ref = reference(pairs, prob["objects"], od)
    for i, f in enumerate(ref):
        J = np.concatenate([J0[i], J1[i]], axis=1)
        errs = (rel_err(J.T @ J, f["L"]), rel_err(J.T @ r[i], f["Ld"]), abs(r[i] @ r[i] - f["s"]) / f["s"])
        print("od %d factor %d form %d: J^T J %.2e  J^T r %.2e  |r|^2 %.2e" % ((od, i, pairs["form"][i]) + errs))
        assert max(errs) < 1e-12, (i, errs)
        if pairs["form"][i] == COND:
            assert not r[i, :od].any() and not J[:od].any()                   # p(b | a): the first od residuals are zero


# ---- 2. reduced system and cost ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["default", "object_constant", "nine", "deterministic"])
def test_reduced_system_gains_w_lambda(variant):
    od = 9 if variant == "nine" else 7
    prob = base_problem(od)
    if variant == "object_constant":
        prob = dict(prob, object_const=np.array([0, 1, 0, 0, 0], np.uint8))        # object 1: b of (0,1), a of (1,4)
    pairs = make_pairs(prob, od)
    ref = reference(pairs, prob["objects"], od)
    assert ref[0]["w"] < 1.0 and ref[1]["w"] == 1.0 and ref[2]["w"] == 1.0
    rows, m = object_rows(prob, od)
    ba = product(prob, deterministic=(variant == "deterministic"))
    S0, b0 = ba.debug_reduced_system(1e300)
    c0 = [ba.evaluate(loss) for loss in (True, False)]
    assert S0.shape == (m, m) and (variant != "default" or m == 89)
    # the signs of the two sides, read off a type-4 prior on object 0
    rng = np.random.default_rng(5)
    C4, m4 = spd(rng, od), prob["objects"][0] + 0.03
    ba.set_ltm_priors([0], m4[None], C4.reshape(1, -1), 1e6)
    S4, b4 = ba.debug_reduced_system(1e300)
    ba.set_ltm_priors(np.zeros(0, np.uint32), np.zeros((0, od)), np.zeros((0, od * od)), 1.0)
    L4 = np.linalg.inv(C4)
    o0 = slice(rows[0], rows[0] + od)
    sH = np.sign(np.trace((S4 - S0)[o0, o0]))
    sg = np.sign((b4 - b0)[o0] @ (L4 @ (prob["objects"][0] - m4)))
    assert rel_err((S4 - S0)[o0, o0], sH * L4) < 1e-9 and sH != 0 and sg != 0
    # the pair priors
    set_pairs(ba, pairs)
    assert ba._fn("ba_num_factors")(ba._h, C.c_int32(T)) == 3
    S1, b1 = ba.debug_reduced_system(1e300)
    E, e = scatter(ref, pairs, rows, m, od)
    eS, eb = np.abs(S1 - S0 - sH * E).max() / np.abs(S1).max(), np.abs(b1 - b0 - sg * e).max() / np.abs(b1).max()
    print("%s: lhs %.2e  rhs %.2e  (m = %d, w = %s)" % (variant, eS, eb, m, [f["w"] for f in ref]))
    assert eS < 1e-11 and eb < 1e-11
    # evaluate: the base value plus sum rho / 2 (with loss) or sum s / 2 (without), the new residuals and norms behind what was there before
    for (cb, rb, qb), loss in zip(c0, (True, False)):
        c1, r1, q1 = ba.evaluate(loss)
        add = 0.5 * sum(f["rho"] if loss else f["s"] for f in ref)
        print("%s: cost, loss %d: %.2e" % (variant, loss, abs(c1 - cb - add) / c1))
        assert abs(c1 - cb - add) <= 1e-12 * c1
        assert len(r1) == len(rb) + 3 * 2 * od and len(q1) == len(qb) + 3
        assert np.array_equal(r1[:len(rb)], rb) and np.array_equal(q1[:len(qb)], qb)
        assert rel_err(q1[len(qb):], [f["s"] for f in ref]) < 1e-12
        scale = [np.sqrt(f["w"]) if loss else 1.0 for f in ref]
        assert rel_err((r1[len(rb):].reshape(3, 2 * od) ** 2).sum(axis=1), [f["s"] * k * k for f, k in zip(ref, scale)]) < 1e-12
    # the reduced program counts the factor's residuals: a pair with a variable object has 2 od of them
    s0 = product(prob).solve(helpers.ba_params(max_it=1))
    s1 = ba.solve(helpers.ba_params(max_it=1))
    assert s1.num_residuals_reduced == s0.num_residuals_reduced + 3 * 2 * od and s1.reduced_system_size == m
    # masking a factor takes exactly its part out again
    ba2 = product(prob, deterministic=(variant == "deterministic"))
    set_pairs(ba2, pairs)
    ba2.set_active_mask(T, [0, 1, 1])
    S2, b2 = ba2.debug_reduced_system(1e300)
    E2, e2 = scatter(ref[1:], dict(a=pairs["a"][1:], b=pairs["b"][1:]), rows, m, od)
    assert np.abs(S2 - S0 - sH * E2).max() < 1e-11 * np.abs(S2).max() and np.abs(b2 - b0 - sg * e2).max() < 1e-11 * np.abs(b2).max()


def test_both_objects_constant_is_fixed_cost():
    prob = dict(base_problem(), object_const=np.array([1, 1, 0, 0, 0], np.uint8))
    pairs = make_pairs(prob, 7)
    ref = reference(pairs, prob["objects"], 7)
    ba0, ba1 = product(prob), product(prob)
    set_pairs(ba1, pairs)
    prm = helpers.ba_params(max_it=2)
    s0, s1 = ba0.solve(prm), ba1.solve(prm)
    assert abs(s1.fixed_cost - s0.fixed_cost - 0.5 * ref[0]["rho"]) <= 1e-12 * s1.fixed_cost       # (0,1): both constant
    assert s1.num_residuals_reduced == s0.num_residuals_reduced + 2 * 14
    assert abs(s1.initial_cost - s0.initial_cost - 0.5 * sum(f["rho"] for f in ref)) <= 1e-12 * s1.initial_cost


# ---- 3. equivalence with two type-4 priors -----------------------------------------------------------------------------------------------
def test_block_diagonal_pair_is_two_ltm_priors():
    prob = base_problem()
    rng = np.random.default_rng(11)
    a, b = 1, 3
    CA, CB = spd(rng, 7), spd(rng, 7)
    Cj = np.zeros((14, 14)); Cj[:7, :7] = CA; Cj[7:, 7:] = CB
    ma, mb = prob["gt_objects"][a] + 0.05, prob["gt_objects"][b] - 0.05
    pair, two = product(prob), product(prob)
    pair.set_map_pair_priors([a], [b], ma[None], mb[None], Cj[None], None, 1e6)
    two.set_ltm_priors([a, b], np.stack([ma, mb]), np.stack([CA.ravel(), CB.ravel()]), 1e6)
    for radius in (100.0, 0.5):
        Sp, bp = pair.debug_reduced_system(radius); St, bt = two.debug_reduced_system(radius)
        print("radius %g: lhs %.2e rhs %.2e" % (radius, rel_err(Sp, St), rel_err(bp, bt)))
        assert rel_err(Sp, St) < 1e-11 and rel_err(bp, bt) < 1e-11
    assert rel_err(pair.column_sqnorms()[2], two.column_sqnorms()[2]) < 1e-11
    prm = helpers.ba_params(max_it=40)
    sp, st = pair.solve(prm), two.solve(prm)
    assert sp.termination_type == st.termination_type and sp.num_iterations == st.num_iterations and sp.num_iterations > 4
    assert sp.num_residuals_reduced == st.num_residuals_reduced
    for x, y in zip(pair.iterations(), two.iterations()):
        assert x.step_is_successful == y.step_is_successful and abs(x.cost - y.cost) <= 1e-8 * y.cost
    for x, y in zip(pair.get_state(), two.get_state()):
        assert np.abs(x - y).max() < 1e-8


# ---- 4. / 5. objects-only problems --------------------------------------------------------------------------------------------------------


def test_a_tree_of_conditionals_is_the_exact_joint():
    od = 7
    rng = np.random.default_rng(21)
    # block-tridiagonal SPD information: a Markov chain 0 - 1 - 2 (diagonally dominant by blocks: eigenvalues within [0.2, 1.8] x 100)
    info = np.zeros((3 * od, 3 * od))
    for k in range(3):
        info[od * k:od * k + od, od * k:od * k + od] = spd(rng, od, cond=2.0, scale=0.7)
    for k in range(2):
        X = rng.normal(size=(od, od)); X *= 0.2 / np.linalg.norm(X, 2)
        info[od * k + od:od * k + 2 * od, od * k:od * k + od] = X; info[od * k:od * k + od, od * k + od:od * k + 2 * od] = X.T
    info *= 100.0
    Sigma = inv_ld(info).astype(np.float64)
    assert np.abs(np.linalg.inv(info) - Sigma).max() <= 1e-12 * np.abs(Sigma).max()
    mu = rng.normal(size=(3, od))
    sub = lambda i, j: Sigma[np.ix_(np.r_[od * i:od * i + od, od * j:od * j + od], np.r_[od * i:od * i + od, od * j:od * j + od])]   # noqa: E731
    ba = objects_only(mu + rng.normal(scale=0.3, size=(3, od)))
    ba.set_ltm_priors([0], mu[:1], Sigma[:od, :od].reshape(1, -1), 1e6)
    ba.set_map_pair_priors([0, 1], [1, 2], mu[[0, 1]], mu[[1, 2]], np.stack([sub(0, 1), sub(1, 2)]), [COND, COND], 1e6)
    s = ba.solve(helpers.ba_params(max_it=50, ftol=0.0, gtol=0.0, ptol=0.0))
    err = np.abs(ba.get_objects() - mu).max()
    print("tree: %d iterations, |x - mu| %.2e, final cost %.2e" % (s.num_iterations, err, s.final_cost))
    assert err < 1e-9
    ia, ib = np.repeat(np.arange(3), 3), np.tile(np.arange(3), 3)
    cov = ba.object_covariances(ia, ib)
    for i, j, c in zip(ia, ib, cov):
        want = Sigma[od * i:od * i + od, od * j:od * j + od]
        print("tree: Sigma(%d,%d) %.2e" % (i, j, rel_err(c, want)))
        assert rel_err(c, want) < 1e-9, (i, j)                                     # relative to the block's own largest entry, the small (0,2) block included


def test_a_pair_prior_puts_its_block_on_the_tile_pattern():
    """30 objects with a type-4 prior each and nothing else: 210 rows in index order, four tile rows, and only the diagonal tiles marked.  The pair (0, 29)
    is rows 0.. against rows 203..: tile (3, 0), which nothing but the pair prior's mark in the plan puts on the pattern; without it the kernel's adds would
    land in a tile that is neither cleared nor factorised.  (1, 20) is tile (2, 0): no factor, no fill (column 0 has one off-diagonal tile), off the pattern."""
    od, O = 7, 30
    rng = np.random.default_rng(31)
    mu = rng.normal(size=(O, od))
    C4 = np.stack([spd(rng, od, cond=10.0, scale=1e-2) for _ in range(O)])
    Cp = spd(rng, 2 * od, cond=10.0, scale=1e-2)
    ba = objects_only(mu + rng.normal(scale=0.05, size=(O, od)))
    ba.set_ltm_priors(np.arange(O), mu, C4.reshape(O, -1), 1e6)
    ba.set_map_pair_priors([0], [29], mu[:1], mu[29:], Cp[None], [JOINT], 1e6)
    info = np.zeros((O * od, O * od), dtype=LD)
    for o in range(O):
        info[od * o:od * o + od, od * o:od * o + od] = inv_ld(C4[o])
    rows = np.r_[0:od, od * 29:od * 30]
    info[np.ix_(rows, rows)] += inv_ld(Cp)
    Sigma = inv_ld(info).astype(np.float64)
    assert np.abs(np.linalg.inv(info.astype(np.float64)) - Sigma).max() <= 1e-12 * np.abs(Sigma).max()
    ia, ib = np.array([0, 0, 29, 29, 5, 0]), np.array([0, 29, 0, 29, 5, 5])
    cov = ba.object_covariances(ia, ib)
    for i, j, c in zip(ia[:5], ib[:5], cov):
        want = Sigma[od * i:od * i + od, od * j:od * j + od]
        print("pattern: Sigma(%d,%d) %.2e" % (i, j, rel_err(c, want)))
        assert rel_err(c, want) < 1e-9, (i, j)
    assert np.abs(cov[5]).max() <= 1e-9 * np.abs(Sigma).max()                      # (0, 5): independent
    ba.covariance_compute()
    assert list(ba.covariance_on_pattern([2, 2], [0, 1], [2, 2], [29, 20])) == [1, 0]
    s = ba.solve(helpers.ba_params(max_it=50, ftol=0.0, gtol=0.0, ptol=0.0))
    assert s.reduced_system_size == O * od and np.abs(ba.get_objects() - mu).max() < 1e-9


def test_selection_and_masks_on_a_planned_handle():
    """obvi_ba_select_outliers on type 9 follows the rule it follows on type 4 (helpers.map_rule on the un-robustified block norms), and a mask change on a
    handle that already holds a plan takes the factor out (subset: the plan stays) and puts it back (superset: a new plan)."""
    prob = base_problem()
    pairs = make_pairs(prob, 7)
    ref = reference(pairs, prob["objects"], 7)
    base = product(prob).evaluate(True)[0]
    ba = product(prob)
    set_pairs(ba, pairs)
    assert ba.num_factors(T) == 3

    def summary():                                                                  # one LM iteration for the reduced program's counts, the state put back
        ba.snapshot()
        s = ba.solve(helpers.ba_params(max_it=1))
        ba.restore()
        return s
    s_all = summary()                                                               # (this also plans the handle)
    assert np.array_equal(ba.get_objects(), prob["objects"])
    sq = ba.evaluate(False)[2][-3:]
    assert rel_err(sq, [f["s"] for f in ref]) < 1e-12
    for fraction in (0.34, 0.7):
        mask, n_out = ba.select_outliers(T, fraction)
        want, want_n = helpers.map_rule(sq, np.ones(3), fraction)
        assert n_out == want_n and list(mask) == list(want) and n_out == int(3 * fraction)
    mask, _ = ba.select_outliers(T, 0.34)
    assert list(mask) == [0, 1, 1]                                                  # the far pair goes
    ba.set_active_mask(T, mask)
    c1 = ba.evaluate(True)[0]
    assert abs(c1 - base - 0.5 * (ref[1]["rho"] + ref[2]["rho"])) <= 1e-12 * c1
    s_sub = summary()
    assert s_sub.num_residuals_reduced == s_all.num_residuals_reduced - 14 and abs(s_sub.initial_cost - c1) <= 1e-12 * c1
    m2, n2 = ba.select_outliers(T, 0.5)                                             # the masked factor is not a candidate: one of the two that are left goes
    assert n2 == 1 and list(m2) == list(helpers.map_rule(sq, mask, 0.5)[0]) and m2[0] == 0 and sorted(m2[1:]) == [0, 1]
    ba.set_active_mask(T, [1, 1, 1])
    c2 = ba.evaluate(True)[0]
    s_back = summary()
    assert abs(c2 - base - 0.5 * sum(f["rho"] for f in ref)) <= 1e-12 * c2 and s_back.num_residuals_reduced == s_all.num_residuals_reduced
    rows, m = object_rows(prob, 7)
    plain = product(prob)
    S0, b0 = plain.debug_reduced_system(1e300)
    S1, b1 = ba.debug_reduced_system(1e300)
    E, e = scatter(ref, pairs, rows, m, 7)
    assert np.abs(np.abs(S1 - S0) - np.abs(E)).max() < 1e-11 * np.abs(S1).max() and np.abs(np.abs(b1 - b0) - np.abs(e)).max() < 1e-11 * np.abs(b1).max()


def test_round_trip_through_the_covariance_call():
    prob = base_problem()
    src = product(prob)
    src.solve(helpers.ba_params(max_it=15))
    a, b = 1, 3
    blk = src.object_covariances([a, a, b], [a, b, b])
    Cj = np.block([[blk[0], blk[1]], [blk[1].T, blk[2]]])
    Cj = 0.5 * (Cj + Cj.T)
    ev = np.linalg.eigvalsh(Cj)
    mean = src.get_objects()[[a, b]]
    dst = objects_only(mean + 0.01)
    dst.set_map_pair_priors([0], [1], mean[:1], mean[1:], Cj[None], None, 1e6)
    back = dst.object_covariances([0, 0, 1], [0, 1, 1])
    got = np.block([[back[0], back[1]], [back[1].T, back[2]]])
    print("round trip: %.2e (condition number of the pair's covariance %.2e)" % (rel_err(got, Cj), ev[-1] / ev[0]))
    assert rel_err(got, Cj) < 1e-9


# ---- 6. deterministic ----------------------------------------------------------------------------------------------------------------------
def test_deterministic_handle_repeats_bit_for_bit():
    prob = base_problem()
    pairs = make_pairs(prob, 7)

    def run():
        ba = product(prob, deterministic=True)
        set_pairs(ba, pairs)
        s = ba.solve(helpers.ba_params(max_it=12))
        its = [(i.iteration, i.step_is_successful, i.cost, i.cost_change, i.gradient_max_norm, i.gradient_norm, i.step_norm, i.relative_decrease, i.trust_region_radius) for i in ba.iterations()]
        return (s.num_iterations, s.termination_type, s.initial_cost, s.final_cost, s.fixed_cost), its, ba.get_state()
    (s1, i1, x1), (s2, i2, x2) = run(), run()
    assert s1 == s2 and i1 == i2 and s1[0] > 3
    for u, v in zip(x1, x2):
        assert np.array_equal(u, v)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    prob = base_problem()
    ba = product(prob)
    rng = np.random.default_rng(1)
    Cj, m = spd(rng, 14), prob["objects"]

    def status(a, b, cov=None, form=None):
        n = len(a)
        try:
            ba.set_map_pair_priors(a, b, m[np.minimum(a, 4)], m[np.minimum(b, 4)], np.stack([Cj] * n) if cov is None else cov, form, 1.0)
        except obvi_ba.ObviError as e:
            return int(str(e).split("status ")[1].split()[0])
        return 0
    assert status([0], [1]) == 0
    f = ba._lib.obvi_map_set_pair_priors
    f.restype = C.c_int
    ok = [np.zeros(1, np.uint32), np.ones(1, np.uint32), np.ascontiguousarray(m[:1]), np.ascontiguousarray(m[1:2]), np.ascontiguousarray(Cj)]
    for k in range(5):                                                                  # every required pointer null in turn
        args = [None if j == k else x.ctypes.data_as(C.c_void_p) for j, x in enumerate(ok)]
        assert f(ba._h, C.c_int64(1), *args, None, C.c_double(1.0)) == -1, k
    assert f(ba._h, C.c_int64(-1), *[x.ctypes.data_as(C.c_void_p) for x in ok], None, C.c_double(1.0)) == -1
    assert status([2], [2]) == -1                                                       # a == b
    assert status([0, 0], [1, 1]) == -1 and status([0, 1], [1, 0]) == -1                # the same unordered pair twice
    assert status([0], [1], form=[2]) == -1                                             # an unknown form
    assert status([0], [5]) == -4 and status([7], [1]) == -4                            # an index >= O
    bad = Cj.copy(); bad[3, 3] = -1.0
    assert status([0], [1], cov=bad[None]) == -6                                        # not SPD
    semi = np.zeros((14, 14)); semi[:7, :7] = np.eye(7)
    assert status([0], [1], cov=semi[None], form=[COND]) == -6
    assert ba._fn("ba_num_factors")(ba._h, C.c_int32(T)) == 1                           # a refused call leaves the factors that were there
    ba.reset()
    assert ba._fn("ba_num_factors")(ba._h, C.c_int32(T)) == 0 and ba.num_factors(T) == 0
    # n = 0 clears
    ba = product(prob)
    assert status([0], [1]) == 0 and ba._fn("ba_num_factors")(ba._h, C.c_int32(T)) == 1
    ba.set_map_pair_priors(np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros((0, 7)), np.zeros((0, 7)), np.zeros((0, 196)))
    assert ba._fn("ba_num_factors")(ba._h, C.c_int32(T)) == 0 and ba._fn("ba_num_residuals")(ba._h) == len(ba.evaluate()[1])
    # a handle that exchanges shared objects refuses the problem before any collective
    calls = []
    ex = product(prob)
    ex.set_map_pair_priors([0], [1], m[:1], m[1:2], Cj[None])
    ex.set_shared_objects(np.array([0, 0, 1, 0, 0], np.uint8), 0, 1)
    ex.set_allreduce(lambda buf, count, op, stream: calls.append(count) or 0)
    for call in (ex.prepare, lambda: ex.solve(helpers.ba_params(max_it=2)), lambda: ex.evaluate(), ex.covariance_compute):
        with pytest.raises(obvi_ba.ObviError, match="status -1"):
            call()
    assert calls == []
    ex.set_map_pair_priors(np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros((0, 7)), np.zeros((0, 7)), np.zeros((0, 196)))
    ex.prepare()                                                                        # without pair priors the handle is as before
