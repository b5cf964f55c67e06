"""GPU: covariance blocks of poses, features and objects by selected inversion (include/obvi_cov.h) against numpy on the ORACLE's
linearisation, against the merged route (obvi_ba_object_covariances) and against identities of the inverse."""
import numpy as np
import pytest

import helpers
import obvi_ba
import synth
import test_gpu_structure as structure
import test_oracle_solver as ref

pytestmark = pytest.mark.gpu

POSE, OBJ = 0, 2


def block_err(got, want):
    """largest deviation relative to the wanted block's largest entry"""
    return float(np.abs(got - want).max() / np.abs(want).max())


def parameters(oracle):
    """(pose, feature, object) masks of the blocks that are parameters of the problem, from the oracle's column norms"""
    p, l, o = oracle.column_sqnorms()
    return p[:, 0] >= 0, l[:, 0] >= 0, o[:, 0] >= 0


def canonical(pvar, ovar, od):
    """first row in the canonical reduced order (variable poses by index, then variable objects) per pose / object, -1: none"""
    prow = np.where(pvar, 6 * (np.cumsum(pvar) - 1), -1)
    orow = np.where(ovar, 6 * int(pvar.sum()) + od * (np.cumsum(ovar) - 1), -1)
    return prow, orow


def reduced_blocks(prow, orow, od):
    """(kind, index, first row, size) of every reduced block"""
    return [(POSE, i, int(r), 6) for i, r in enumerate(prow) if r >= 0] + [(OBJ, i, int(r), od) for i, r in enumerate(orow) if r >= 0]


def joined_pairs(prob, pvar, ovar):
    """pairs of reduced blocks joined by a factor or a common feature: the contract says their cross blocks are served"""
    pairs = set()
    by_point = {}
    for p, l in zip(prob["rp_pose"], prob["rp_point"]):
        if pvar[p]:
            by_point.setdefault(int(l), set()).add(int(p))
    for ps in by_point.values():
        ps = sorted(ps)
        pairs.update(((POSE, a), (POSE, b)) for a in ps for b in ps if a < b)
    for o, p in zip(prob.get("bb_obj", []), prob.get("bb_pose", [])):
        if ovar[o] and pvar[p]:
            pairs.add(((POSE, int(p)), (OBJ, int(o))))
    for a, b in zip(prob.get("rl_a", []), prob.get("rl_b", [])):
        if pvar[a] and pvar[b] and a != b:
            pairs.add(((POSE, int(min(a, b))), (POSE, int(max(a, b)))))
    return sorted(pairs)


def served_pairs(g, blocks):
    """all pairs of reduced blocks the product says it can serve (the pattern decides what is compared, never a value)"""
    ka, ia, kb, ib = [], [], [], []
    for x, a in enumerate(blocks):
        for b in blocks[x + 1:]:
            ka.append(a[0]); ia.append(a[1]); kb.append(b[0]); ib.append(b[1])
    on = g.covariance_on_pattern(ka, ia, kb, ib).astype(bool)
    return [((ka[i], ia[i]), (kb[i], ib[i])) for i in np.flatnonzero(on)]


def check_cross(g, pairs, rows, dims, C, bar, label):
    """cross blocks (a, b) and (b, a) of the pairs against the dense inverse C"""
    if not pairs:
        return 0.0
    ka, ia, kb, ib = zip(*[(a[0], a[1], b[0], b[1]) for a, b in pairs])
    ab, ba = g.cross_covariances(ka, ia, kb, ib), g.cross_covariances(kb, ib, ka, ia)
    worst = 0.0
    for (a, b), x, y in zip(pairs, ab, ba):
        want = C[rows[a]:rows[a] + dims[a], rows[b]:rows[b] + dims[b]]
        scale = max(np.abs(want).max(), 1e-300)
        worst = max(worst, float(np.abs(x - want).max() / scale), float(np.abs(y - want.T).max() / scale))
        assert np.array_equal(x, y.T), (a, b)
    print("%s: %d cross blocks, worst relative deviation %.3e (bar %.1e)" % (label, len(pairs), worst, bar))
    assert worst < bar
    return worst


@pytest.mark.parametrize("od,renumber", [(7, False), (9, False), (7, True)])
def test_every_block_of_a_small_problem_against_the_dense_inverse_of_the_oracles_jacobian(od, renumber, monkeypatch):
    """12 poses (2 constant), 30 features, 2 objects: C = inv(J^T J), J the oracle's dense robustified Jacobian.  Every pose, feature and object
    block, every cross block on the pattern and its transposed pair.  Bar 1e-8 of the block's largest entry (the project's bar for blocks of
    this inverse on a window of this size); the reference's own resolution d is measured per kind by forming C a second way, from the QR
    factor of J, and the bar of a kind is max(1e-8, 10 d)."""
    if renumber:
        monkeypatch.setenv("OBVI_POINT_RENUMBER_MIN", "1")
    prob = ref.small_problem() if od == 7 else ref.nine_problem()     # (the nine-parameter problem carries LTM priors: their rows join the dense Jacobian)
    monkeypatch.setitem(ref.FACTOR_BLOCKS, 4, (("object", "lt_obj"),)); monkeypatch.setitem(ref.HUBER, 4, "lt_huber")
    o, g = helpers.oracle_ba(object_block_size=od), helpers.product_ba(object_block_size=od)
    for ba in (o, g):
        synth.upload(ba, prob)
    J, _, m, pv = ref.dense_normal_equations(o, prob)
    C = np.linalg.inv(J.T @ J)
    R = np.linalg.qr(J, mode="r")
    Ri = np.linalg.solve(R, np.eye(len(R)))
    C2 = Ri @ Ri.T
    P, L, O = len(prob["poses"]), len(prob["points"]), len(prob["objects"])
    nPv = int((pv >= 0).sum())
    rows, dims = {}, {}
    for p in range(P):
        if pv[p] >= 0:
            rows[(POSE, p)], dims[(POSE, p)] = 6 * pv[p], 6
    for ob in range(O):
        rows[(OBJ, ob)], dims[(OBJ, ob)] = 6 * nPv + od * ob, od
    d = {}
    for kind, keys, dim in (("pose", [k for k in rows if k[0] == POSE], 6), ("object", [k for k in rows if k[0] == OBJ], od)):
        d[kind] = max(block_err(C2[rows[k]:rows[k] + dim, rows[k]:rows[k] + dim], C[rows[k]:rows[k] + dim, rows[k]:rows[k] + dim]) for k in keys)
    d["point"] = max(block_err(C2[m + 3 * l:m + 3 * l + 3, m + 3 * l:m + 3 * l + 3], C[m + 3 * l:m + 3 * l + 3, m + 3 * l:m + 3 * l + 3]) for l in range(L))
    keys = sorted(rows)
    d["cross"] = max(float(np.abs(C2[rows[a]:rows[a] + dims[a], rows[b]:rows[b] + dims[b]] - C[rows[a]:rows[a] + dims[a], rows[b]:rows[b] + dims[b]]).max() /
                           np.abs(C[rows[a]:rows[a] + dims[a], rows[b]:rows[b] + dims[b]]).max()) for a in keys for b in keys if a < b)
    bar = {k: max(1e-8, 10 * v) for k, v in d.items()}
    print("disagreement of the two numpy routes per kind:", {k: "%.2e" % v for k, v in d.items()}, "cond(J^T J) %.2e" % np.linalg.cond(J.T @ J))

    g.covariance_compute()
    cp, cl, co = g.pose_covariances(np.arange(P)), g.point_covariances(np.arange(L)), g.object_covariance_blocks(np.arange(O))
    worst = {"pose": 0.0, "point": 0.0, "object": 0.0}
    for p in range(P):
        if pv[p] < 0:
            assert np.all(cp[p] == 0.0)            # a constant pose: a zero block
        else:
            worst["pose"] = max(worst["pose"], block_err(cp[p], C[6 * pv[p]:6 * pv[p] + 6, 6 * pv[p]:6 * pv[p] + 6]))
    for l in range(L):
        worst["point"] = max(worst["point"], block_err(cl[l], C[m + 3 * l:m + 3 * l + 3, m + 3 * l:m + 3 * l + 3]))
    for ob in range(O):
        r0 = rows[(OBJ, ob)]
        worst["object"] = max(worst["object"], block_err(co[ob], C[r0:r0 + od, r0:r0 + od]))
    print("worst relative deviation per kind:", {k: "%.2e" % v for k, v in worst.items()}, "bars", {k: "%.1e" % v for k, v in bar.items()})
    for k, v in worst.items():
        assert v < bar[k], (k, v, bar[k])
    blocks = [(k[0], k[1], rows[k], dims[k]) for k in keys]
    served = served_pairs(g, blocks)
    pvar, ovar = pv >= 0, np.ones(O, bool)
    assert set(joined_pairs(prob, pvar, ovar)) <= set(served)
    check_cross(g, served, rows, dims, C, bar["cross"], "small problem")
    assert len(g.pose_covariances([])) == 0 and len(g.point_covariances([])) == 0 and g.cross_covariances([], [], [], []) == []


def dissected_problem():
    prob = synth.make_problem(P=260, L=5000, O=24, seed=11, min_obj_obs=5, const_poses=3)
    prob["object_const"][5] = 1
    return prob


def check_against_the_merged_route(g, O, own_bar, cross_bar):
    ids = np.arange(O)
    merged = g.object_covariances(ids)
    g.covariance_compute()
    own = g.object_covariance_blocks(ids)
    live = [i for i in ids if np.any(merged[i] != 0.0)]
    assert all(np.all(own[i] == 0.0) for i in ids if i not in live)
    worst = max(block_err(own[i], merged[i]) for i in live)
    a, b = np.array([(x, y) for x in live for y in live if x < y]).T
    on = g.covariance_on_pattern(np.full(len(a), OBJ), a, np.full(len(a), OBJ), b).astype(bool)
    cross = g.cross_covariances(np.full(on.sum(), OBJ), a[on], np.full(on.sum(), OBJ), b[on]) if on.any() else []
    want = g.object_covariances(a[on], b[on]) if on.any() else []
    scale = float(np.abs(merged).max())
    worst_x = max([float(np.abs(x - w).max()) / scale for x, w in zip(cross, want)] + [0.0])
    print("merged route: own blocks %.3e (bar %.0e), %d of %d object pairs on the pattern, cross %.3e (bar %.0e)" % (worst, own_bar, on.sum(), len(on), worst_x, cross_bar))
    assert worst < own_bar and worst_x < cross_bar
    return a, b, on


def test_the_merged_route_agrees():
    """obvi_cov_object_blocks(o) == obvi_ba_object_covariances(o, o) and the on-pattern object cross blocks equal the (a, b) answer, at that route's own bars
    against the oracle (1e-8 on the small problem, 1e-7 over the dissected factor; cross blocks relative to the largest own entry, as there)."""
    small = ref.small_problem()
    g = helpers.product_ba(); synth.upload(g, small)
    check_against_the_merged_route(g, len(small["objects"]), 1e-8, 1e-8)
    prob = dissected_problem()
    g = helpers.product_ba(); synth.upload(g, prob)
    a, b, on = check_against_the_merged_route(g, len(prob["objects"]), 1e-7, 1e-7)
    assert not on.all()                                   # objects far apart in the tree: off the pattern, refused with a pointer to the merged route
    off = int(np.flatnonzero(~on)[0])
    g.covariance_compute()                                # (the merged route's own linearisation ended the pass above)
    with pytest.raises(obvi_ba.ObviError, match="status -1 .*not on the tile pattern.*obvi_ba_object_covariances"):
        g.cross_covariances([OBJ], [a[off]], [OBJ], [b[off]])


def point_blocks_from_the_oracle(o, prob, Sigma, prow, lvar, sample):
    """Hll^-1 + Hll^-1 W^T Sigma W Hll^-1 per sampled feature, from the oracle's reprojection Jacobians (robustified as dense_normal_equations does)"""
    r, J0, J1 = o.debug_linearize(0)
    a = prob["rp_huber"]
    s = (r ** 2).sum(axis=1)
    w2 = np.where(s > a * a, a / np.sqrt(np.maximum(s, 1e-300)), 1.0)
    out = {}
    for l in sample:
        if not lvar[l]:                                   # constant or unobserved: not a parameter, a zero block is expected
            out[l] = np.zeros((3, 3))
            continue
        obs = np.flatnonzero(prob["rp_point"] == l)
        H = np.zeros((3, 3)); W = np.zeros((Sigma.shape[0], 3))
        for f in obs:
            H += w2[f] * J1[f].T @ J1[f]
            pr = prow[prob["rp_pose"][f]]
            if pr >= 0:
                W[pr:pr + 6] += w2[f] * J0[f].T @ J1[f]
        Hi = np.linalg.inv(H)
        out[l] = Hi + Hi @ W.T @ Sigma @ W @ Hi
    return out


def check_against_the_oracles_reduced_system(prob, n_sample, bar, label):
    o, g = helpers.oracle_ba(), helpers.product_ba()
    for ba in (o, g):
        synth.upload(ba, prob)
    pvar, lvar, ovar = parameters(o)
    prow, orow = canonical(pvar, ovar, 7)
    S, _ = o.debug_reduced_system(1e300)
    assert S.shape[0] == 6 * pvar.sum() + 7 * ovar.sum()
    Sigma = np.linalg.inv(S)
    g.covariance_compute()
    P = len(prob["poses"])
    cp = g.pose_covariances(np.arange(P))
    worst = 0.0
    for p in range(P):
        if prow[p] < 0:
            assert np.all(cp[p] == 0.0)
        else:
            worst = max(worst, block_err(cp[p], Sigma[prow[p]:prow[p] + 6, prow[p]:prow[p] + 6]))
    print("%s: pose blocks against inv(S_oracle): %.3e (bar %.0e), cond(S) %.2e" % (label, worst, bar, np.linalg.cond(S)))
    assert worst < bar
    blocks = reduced_blocks(prow, orow, 7)
    rows = {(k, i): r for k, i, r, _ in blocks}; dims = {(k, i): d for k, i, _, d in blocks}
    joined = joined_pairs(prob, pvar, ovar)
    ka, ia, kb, ib = zip(*[(a[0], a[1], b[0], b[1]) for a, b in joined])
    assert g.covariance_on_pattern(ka, ia, kb, ib).all()          # every pair joined by a factor or a common feature is served
    check_cross(g, joined, rows, dims, Sigma, bar, label)
    rng = np.random.default_rng(20250101)
    sample = rng.choice(len(prob["points"]), size=min(n_sample, len(prob["points"])), replace=False)
    want = point_blocks_from_the_oracle(o, prob, Sigma, prow, lvar, sample)
    got = g.point_covariances(sample)
    worst = 0.0
    for x, l in zip(got, sample):
        if lvar[l]:
            worst = max(worst, block_err(x, want[l]))
        else:
            assert np.all(x == 0.0)
    print("%s: %d sampled feature blocks against the formula on the oracle's linearisation: %.3e (bar %.0e)" % (label, len(sample), worst, bar))
    assert worst < bar
    return g


def test_several_dissection_levels_against_the_oracles_reduced_system():
    """260 frames, several dissection levels: Sigma = inv(S), S the ORACLE's reduced system at radius 1e300.  All pose blocks, the cross blocks of every pair joined
    by a factor or a common feature, and 200 seeded features against Hll^-1 + Hll^-1 W^T Sigma W Hll^-1 assembled from the oracle's Jacobians.  Bar: the
    project's 1e-7 for this size."""
    g = check_against_the_oracles_reduced_system(dissected_problem(), 200, 1e-7, "260 frames")
    assert g.problem_stats()["chol_levels"] >= 3


@pytest.mark.parametrize("which", ["ragged", "stereo"])
def test_ragged_structures_against_the_oracles_reduced_system(which):
    """tracks longer than a wavefront, loop closures, three sightings from one frame, an unobserved feature and an unobserved pose; a stereo rig with holes
    (two records of one frame per feature)."""
    if which == "ragged":
        prob = structure._ragged_problem()
    else:
        prob = synth.make_problem(P=60, L=300, O=0, seed=9, stereo=True, outlier_frac=0.0)
        keep = ~((prob["rp_point"] % 7 == 0) & (prob["rp_pose"] % 5 == 2))
        for k in ("rp_pose", "rp_point", "rp_cam", "rp_pixel", "rp_sigma", "rp_is_outlier"):
            if k in prob and np.ndim(prob[k]) > 0:
                prob[k] = prob[k][keep]
    tracks = np.bincount(prob["rp_point"])
    assert which != "ragged" or tracks.max() > 64
    check_against_the_oracles_reduced_system(prob, 200, 1e-7, which)


def test_identities_of_the_inverse_at_local_ba_size():
    """500 keyframes / 50 000 features / 50 objects, no oracle.  Own object blocks equal the merged route to its 1e-8.  With S the product's own undamped reduced
    system: sum_q Sigma_pq S_qp = I_6 for every pose p, the sum over the q whose block S_qp is non-zero (exact: S_qp vanishes off the pattern); the bar is the
    same identity evaluated with numpy's inv(S) restricted to those blocks, times 10.  Diagonal blocks are symmetric to 1e-12 and positive definite.  Masking a
    seeded tenth of the reprojection factors (no feature left with fewer than two sightings, so the rank stays) makes no pose more certain: no diagonal entry of a pose block decreases by more than 2e-8 of its block's largest entry
    (twice the 1e-8 to which a block of this inverse is held at this size)."""
    prob = synth.make_problem(P=500, L=50000, O=50, seed=3, const_poses=1, min_obj_obs=10)
    g = helpers.product_ba(); synth.upload(g, prob)
    P, O = len(prob["poses"]), len(prob["objects"])
    merged = g.object_covariances(np.arange(O))
    S, _ = g.debug_reduced_system(1e300)
    pvar = ~prob["pose_const"].astype(bool)
    ovar = np.array([np.any(merged[i] != 0.0) for i in range(O)])
    prow, orow = canonical(pvar, ovar, 7)
    assert S.shape[0] == 6 * pvar.sum() + 7 * ovar.sum()
    g.covariance_compute()
    own = g.object_covariance_blocks(np.arange(O))
    worst = max(block_err(own[i], merged[i]) for i in range(O) if ovar[i])
    print("own object blocks against the merged route: %.3e" % worst)
    assert worst < 1e-8
    blocks = reduced_blocks(prow, orow, 7)
    Sn = np.linalg.inv(S)
    ka, ia, kb, ib, owner = [], [], [], [], []
    ref_err = 0.0
    partners = {}
    for p in range(P):
        if prow[p] < 0:
            continue
        col = S[:, prow[p]:prow[p] + 6]
        acc = np.zeros((6, 6))
        partners[p] = []
        for k, i, r, d in blocks:
            if np.any(col[r:r + d] != 0.0):
                partners[p].append((k, i, r, d))
                ka.append(POSE); ia.append(p); kb.append(k); ib.append(i); owner.append(p)
                acc += Sn[prow[p]:prow[p] + 6, r:r + d] @ col[r:r + d]
        ref_err = max(ref_err, float(np.abs(acc - np.eye(6)).max()))
    bar = 10 * ref_err
    got = g.cross_covariances(ka, ia, kb, ib)
    err, at = 0.0, 0
    for p in partners:
        acc = np.zeros((6, 6))
        for k, i, r, d in partners[p]:
            acc += got[at] @ S[r:r + d, prow[p]:prow[p] + 6]; at += 1
        err = max(err, float(np.abs(acc - np.eye(6)).max()))
    print("sum_q Sigma_pq S_qp - I over %d poses, %d blocks: %.3e; numpy's inverse on the same blocks: %.3e (bar %.3e); cond(S) %.2e" % (len(partners), len(got), err, ref_err, bar, np.linalg.cond(S)))
    assert err < bar
    cp = g.pose_covariances(np.arange(P))
    for blk in list(cp[pvar]) + list(own[ovar]):
        assert np.abs(blk - blk.T).max() <= 1e-12 * np.abs(blk).max() and np.all(np.linalg.eigvalsh(blk) > 0)
    rng = np.random.default_rng(7)
    mask = rng.random(len(prob["rp_pose"])) >= 0.1
    left = np.bincount(prob["rp_point"][mask], minlength=len(prob["points"]))
    mask |= left[prob["rp_point"]] < 2                    # (two of the 50 000 features would keep one sighting: a rank-deficient problem, rightly refused with -6)
    assert 0.09 < 1.0 - mask.mean() < 0.11
    mask = mask.astype(np.uint8)
    g.set_active_mask(0, mask)
    with pytest.raises(obvi_ba.ObviError, match="status -5"):
        g.pose_covariances([1])
    g.covariance_compute()
    cm = g.pose_covariances(np.arange(P))
    drop = max(float((np.diag(a) - np.diag(b)).max() / np.abs(a).max()) for a, b in zip(cp[pvar], cm[pvar]))
    print("masking a tenth of the reprojection factors: largest decrease of a diagonal entry %.3e of its block's largest entry" % drop)
    assert drop <= 2e-8


def test_two_passes_on_a_deterministic_handle_are_bit_identical():
    prob = dissected_problem()
    g = helpers.product_ba(deterministic=True); synth.upload(g, prob)
    P, L, O = len(prob["poses"]), len(prob["points"]), len(prob["objects"])
    out = []
    for _ in range(2):
        g.covariance_compute()
        out.append((g.pose_covariances(np.arange(P)), g.point_covariances(np.arange(L)), g.object_covariance_blocks(np.arange(O)),
                    np.concatenate([x.ravel() for x in g.cross_covariances(np.zeros(P - 4, int), np.arange(3, P - 1), np.zeros(P - 4, int), np.arange(4, P))])))
    for a, b in zip(*out):
        assert np.array_equal(a, b) and np.any(a != 0.0)


def test_state_rules():
    prob = ref.small_problem()
    g = helpers.product_ba(deterministic=True); synth.upload(g, prob)
    not_ready = dict(match="status -5")
    with pytest.raises(obvi_ba.ObviError, **not_ready):
        g.pose_covariances([2])
    g.covariance_compute()
    assert np.all(g.pose_covariances([0, 1]) == 0.0) and np.any(g.pose_covariances([2]) != 0.0)        # constant poses: zero blocks
    with pytest.raises(obvi_ba.ObviError, match="status -4"):
        g.pose_covariances([len(prob["poses"])])
    with pytest.raises(obvi_ba.ObviError, match="status -1 .*features"):
        g.cross_covariances([1], [0], [POSE], [2])
    po, pt, ob = g.get_state()
    g.update_state(po, pt, ob)
    for call in (lambda: g.pose_covariances([2]), lambda: g.point_covariances([0]), lambda: g.object_covariance_blocks([0]), lambda: g.cross_covariances([POSE], [2], [POSE], [3])):
        with pytest.raises(obvi_ba.ObviError, **not_ready):
            call()
    g.covariance_compute(); g.pose_covariances([2])
    g.set_active_mask(0, np.ones(len(prob["rp_pose"]), np.uint8))
    with pytest.raises(obvi_ba.ObviError, **not_ready):
        g.pose_covariances([2])
    g.covariance_compute(); g.pose_covariances([2])
    # a solve after a covariance pass: the same LM records as without it, bit for bit on a deterministic handle
    prm = helpers.ba_params(max_it=6)
    s1 = g.solve(prm)
    with pytest.raises(obvi_ba.ObviError, **not_ready):
        g.pose_covariances([2])
    g2 = helpers.product_ba(deterministic=True); synth.upload(g2, prob)
    s2 = g2.solve(prm)
    assert s1.num_iterations == s2.num_iterations and s1.final_cost == s2.final_cost
    for a, b in zip(g.iterations(), g2.iterations()):
        assert (a.cost, a.gradient_max_norm, a.step_norm, a.relative_decrease, a.trust_region_radius) == (b.cost, b.gradient_max_norm, b.step_norm, b.relative_decrease, b.trust_region_radius)
    assert np.array_equal(g.get_poses(), g2.get_poses()) and np.array_equal(g.get_points(), g2.get_points())
    # an oracle-backed adjuster has no such entry
    with pytest.raises(obvi_ba.ObviError):
        helpers.oracle_ba().covariance_compute()


def test_a_free_gauge_is_a_status_not_a_fault():
    """no constant pose, one camera: the normal equations are rank deficient -> OBVI_ERR_NUMERICAL, and the handle goes on working"""
    prob = synth.make_problem(P=12, L=30, O=2, seed=5, min_obj_obs=4, object_classes=("bench", "chair"), const_poses=0)
    g = helpers.product_ba(); synth.upload(g, prob)
    with pytest.raises(obvi_ba.ObviError, match="status -6"):
        g.covariance_compute()
    with pytest.raises(obvi_ba.ObviError, match="status -5"):
        g.pose_covariances([0])
    assert g.solve(helpers.ba_params(max_it=3)).num_iterations >= 1
