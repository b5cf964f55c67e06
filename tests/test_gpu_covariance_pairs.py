"""GPU: covariance blocks of declared pairs (obvi_cov_compute_pairs, include/obvi_cov_pairs.h) -- pose and object pairs off the tile pattern of the factor
and every cross block with a feature -- against numpy on the ORACLE's linearisation."""
import functools

import numpy as np
import pytest

import helpers
import obvi_ba
import synth
import test_gpu_covariance_blocks as blocks
import test_gpu_structure as structure
import test_oracle_solver as ref

pytestmark = pytest.mark.gpu

POSE, POINT, OBJ = 0, 1, 2
KIND = {POSE: "pose", POINT: "point", OBJ: "object"}


def declare(g, pairs):
    ka, ia, kb, ib = zip(*[(a[0], a[1], b[0], b[1]) for a, b in pairs])
    g.covariance_compute_pairs(ka, ia, kb, ib)


def served(g, pairs):
    """the blocks (a, b) and (b, a) of the pairs; the second is the exact transpose of the first"""
    ka, ia, kb, ib = zip(*[(a[0], a[1], b[0], b[1]) for a, b in pairs])
    assert g.covariance_on_pattern(ka, ia, kb, ib).all() and g.covariance_on_pattern(kb, ib, ka, ia).all()
    ab, ba = g.cross_covariances(ka, ia, kb, ib), g.cross_covariances(kb, ib, ka, ia)
    for p, x, y in zip(pairs, ab, ba):
        assert np.array_equal(x, y.T), p
    return ab


@pytest.mark.parametrize("od,renumber", [(7, False), (9, False), (7, True)])
def test_every_pair_of_a_small_problem_against_the_dense_inverse_of_the_oracles_jacobian(od, renumber, monkeypatch):
    """12 poses (2 constant), 30 features, 2 objects: all pairs among all 44 blocks, self pairs and constant poses included, declared and compared with
    C = inv(J^T J), J the oracle's dense robustified Jacobian, relative to the wanted block's largest entry.  Bar per kind of pair max(1e-8, 10 d), d the
    disagreement on the same blocks of the two numpy routes to C (the inverse, and the QR factor of J).  Blocks with a constant pose are exactly zero.  The
    plain getters return the same bits after compute_pairs as after compute (deterministic handle)."""
    if renumber:
        monkeypatch.setenv("OBVI_POINT_RENUMBER_MIN", "1")
    prob = ref.small_problem() if od == 7 else ref.nine_problem()
    monkeypatch.setitem(ref.FACTOR_BLOCKS, 4, (("object", "lt_obj"),)); monkeypatch.setitem(ref.HUBER, 4, "lt_huber")
    o, g = helpers.oracle_ba(object_block_size=od), helpers.product_ba(object_block_size=od, deterministic=True)
    for ba in (o, g):
        synth.upload(ba, prob)
    J, _, m, pv = ref.dense_normal_equations(o, prob)
    C = np.linalg.inv(J.T @ J)
    R = np.linalg.qr(J, mode="r")
    Ri = np.linalg.solve(R, np.eye(len(R)))
    C2 = Ri @ Ri.T
    P, L, O = len(prob["poses"]), len(prob["points"]), len(prob["objects"])
    nPv = int((pv >= 0).sum())
    span = {}
    for p in range(P):
        span[(POSE, p)] = None if pv[p] < 0 else (6 * pv[p], 6)
    for l in range(L):
        span[(POINT, l)] = (m + 3 * l, 3)
    for ob in range(O):
        span[(OBJ, ob)] = (6 * nPv + od * ob, od)
    keys = sorted(span)
    assert len(keys) == 44
    pairs = [(a, b) for x, a in enumerate(keys) for b in keys[x:]]

    g.covariance_compute()
    reduced = [(k[0], k[1], span[k][0], span[k][1]) for k in keys if k[0] != POINT and span[k] is not None]
    on_pairs = blocks.served_pairs(g, reduced)
    ka, ia, kb, ib = zip(*[(a[0], a[1], b[0], b[1]) for a, b in on_pairs])

    def plain():
        return [g.pose_covariances(np.arange(P)), g.point_covariances(np.arange(L)), g.object_covariance_blocks(np.arange(O)),
                np.concatenate([x.ravel() for x in g.cross_covariances(ka, ia, kb, ib)])]
    before = plain()
    declare(g, pairs)
    for x, y in zip(before, plain()):
        assert np.array_equal(x, y) and np.any(x != 0.0)

    got = served(g, pairs)
    d, worst = {}, {}
    for (a, b), x in zip(pairs, got):
        da, db = 6 if a[0] == POSE else 3 if a[0] == POINT else od, 6 if b[0] == POSE else 3 if b[0] == POINT else od
        assert x.shape == (da, db)
        if span[a] is None or span[b] is None:
            assert np.all(x == 0.0), (a, b)                # a constant pose: exactly zero
            continue
        (ra, _), (rb, _) = span[a], span[b]
        want, want2 = C[ra:ra + da, rb:rb + db], C2[ra:ra + da, rb:rb + db]
        kind = KIND[a[0]] + "-" + KIND[b[0]]
        scale = np.abs(want).max()
        d[kind] = max(d.get(kind, 0.0), float(np.abs(want2 - want).max() / scale))
        worst[kind] = max(worst.get(kind, 0.0), float(np.abs(x - want).max() / scale))
    print("disagreement of the two numpy routes per kind of pair:", {k: "%.2e" % v for k, v in d.items()})
    print("worst relative deviation per kind of pair:          ", {k: "%.2e" % v for k, v in worst.items()})
    assert len(worst) == 6
    for k, v in worst.items():
        assert v < max(1e-8, 10 * d[k]), (k, v, d[k])


# ---- the oracle's reduced system and Jacobians as the yardstick ------------------------------------------------------------------------------------------

class Yardstick:
    """Sigma = inv(S_oracle) (and a second route to it, by Cholesky), and per feature H_ll and W_l = sum_a J_pose^T J_point, robustified, from the oracle's
    Jacobians.  Blocks with a feature:  Sigma_{l,x} = -H_l^-1 W_l^T Sigma[:, x],  Sigma_{l,m} = H_l^-1 W_l^T Sigma W_m H_m^-1  -- the two formulas of
    DESIGN.md 4b with C C^T = H_l and Z_a = W_a C^-T."""

    def __init__(self, prob, mask=None):
        self.prob = prob
        o = helpers.oracle_ba(); synth.upload(o, prob)
        if mask is not None:
            o.set_active_mask(0, mask)
        self.pvar, self.lvar, self.ovar = blocks.parameters(o)
        self.prow, self.orow = blocks.canonical(self.pvar, self.ovar, 7)
        S, _ = o.debug_reduced_system(1e300)
        assert S.shape[0] == 6 * self.pvar.sum() + 7 * self.ovar.sum()
        self.Sigma = np.linalg.inv(S)
        Li = np.linalg.solve(np.linalg.cholesky(S), np.eye(len(S)))
        self.Sigma2 = Li.T @ Li
        r, self.J0, self.J1 = o.debug_linearize(0)
        a = prob["rp_huber"]
        s = (r ** 2).sum(axis=1)
        self.w2 = np.where(s > a * a, a / np.sqrt(np.maximum(s, 1e-300)), 1.0)
        if mask is not None:
            self.w2 = self.w2 * (np.asarray(mask) != 0)
        order = np.argsort(prob["rp_point"], kind="stable")
        self.obs_ptr = np.searchsorted(prob["rp_point"][order], np.arange(len(prob["points"]) + 1))
        self.obs_of = order
        self._hw = {}

    def obs(self, l):
        return self.obs_of[self.obs_ptr[l]:self.obs_ptr[l + 1]]

    def hw(self, l):
        if l not in self._hw:
            H = np.zeros((3, 3)); W = np.zeros((self.Sigma.shape[0], 3))
            for f in self.obs(l):
                H += self.w2[f] * self.J1[f].T @ self.J1[f]
                pr = self.prow[self.prob["rp_pose"][f]]
                if pr >= 0:
                    W[pr:pr + 6] += self.w2[f] * self.J0[f].T @ self.J1[f]
            self._hw[l] = (np.linalg.inv(H), W)
        return self._hw[l]

    def rows(self, key):
        r = self.prow[key[1]] if key[0] == POSE else self.orow[key[1]]
        return None if r < 0 else slice(int(r), int(r) + (6 if key[0] == POSE else 7))

    def block(self, a, b, Sigma):
        """the wanted block (a, b); None: a zero block (a constant or unused block takes part)"""
        if a[0] == POINT and b[0] == POINT:
            if not (self.lvar[a[1]] and self.lvar[b[1]]):
                return None
            (Ha, Wa), (Hb, Wb) = self.hw(a[1]), self.hw(b[1])
            return Ha @ Wa.T @ Sigma @ Wb @ Hb + (Ha if a[1] == b[1] else 0.0)
        if b[0] == POINT:
            x = self.block(b, a, Sigma)
            return None if x is None else x.T
        if a[0] == POINT:
            rb = self.rows(b)
            if rb is None or not self.lvar[a[1]]:
                return None
            Ha, Wa = self.hw(a[1])
            return -Ha @ Wa.T @ Sigma[:, rb]
        ra, rb = self.rows(a), self.rows(b)
        return None if ra is None or rb is None else Sigma[ra, rb]

    def check(self, g, pairs, floor, label):
        """served blocks against the yardstick, bar max(floor, 10 d) of the wanted block's largest entry; d: the two routes to Sigma on the same blocks"""
        got = served(g, pairs)
        d = worst = 0.0
        for (a, b), x in zip(pairs, got):
            want = self.block(a, b, self.Sigma)
            if want is None:
                assert np.all(x == 0.0), (a, b)
                continue
            scale = np.abs(want).max()
            d = max(d, float(np.abs(self.block(a, b, self.Sigma2) - want).max() / scale))
            worst = max(worst, float(np.abs(x - want).max() / scale))
        bar = max(floor, 10 * d)
        print("%s: %d declared pairs, worst relative deviation %.3e; the two numpy routes disagree by d = %.3e; bar %.3e" % (label, len(pairs), worst, d, bar))
        assert worst < bar
        return got


@functools.lru_cache(maxsize=None)
def dissected():
    prob = blocks.dissected_problem()
    return prob, Yardstick(prob)


def dissected_pairs(g, prob, y):
    """after a plain compute on g: pose-pose, pose-object and object-object pairs the product reports off the pattern (at least 8 of each, the first and the
    last variable pose among the poses), and 30 + 30 + 30 + 30 pairs with a feature"""
    rng = np.random.default_rng(20260301)
    pv = np.flatnonzero(y.pvar)
    poses = [int(pv[i]) for i in np.unique(np.linspace(0, len(pv) - 1, 24).round().astype(int))]
    assert poses[0] == pv[0] and poses[-1] == pv[-1]
    objs = [int(i) for i in np.flatnonzero(y.ovar)]
    cand = {"pose-pose": [((POSE, poses[0]), (POSE, poses[-1]))] + [((POSE, a), (POSE, b)) for x, a in enumerate(poses) for b in poses[x + 1:] if (a, b) != (poses[0], poses[-1])],
            "pose-object": [((POSE, a), (OBJ, b)) for a in poses for b in objs],
            "object-object": [((OBJ, a), (OBJ, b)) for x, a in enumerate(objs) for b in objs[x + 1:]]}
    off = {}
    for kind, c in cand.items():
        ka, ia, kb, ib = zip(*[(a[0], a[1], b[0], b[1]) for a, b in c])
        on = g.covariance_on_pattern(ka, ia, kb, ib).astype(bool)
        off[kind] = [p for p, x in zip(c, on) if not x][:40]
        assert len(off[kind]) >= 8, (kind, len(off[kind]))
    rp_pose, rp_point = prob["rp_pose"], prob["rp_point"]
    seen = {(int(p), int(l)) for p, l in zip(rp_pose, rp_point)}
    live = [f for f in rng.permutation(len(rp_pose)) if y.pvar[rp_pose[f]] and y.lvar[rp_point[f]]]
    feat = {"pose observes feature": [((POSE, int(rp_pose[f])), (POINT, int(rp_point[f]))) for f in live[:30]], "pose does not": [], "feature-object": [], "feature-feature": []}
    while len(feat["pose does not"]) < 30:
        p, l = int(rng.choice(pv)), int(rng.integers(len(prob["points"])))
        if (p, l) not in seen and y.lvar[l]:
            feat["pose does not"].append(((POSE, p), (POINT, l)))
    feat["feature-object"] = [((POINT, int(rp_point[f])), (OBJ, int(rng.choice(objs)))) for f in live[30:60]]
    poses_of = lambda l: {int(rp_pose[f]) for f in y.obs(l)}
    for f in live[60:]:                                   # a common observing pose: two features of one frame
        if len(feat["feature-feature"]) == 15:
            break
        others = [int(rp_point[q]) for q in np.flatnonzero(rp_pose == rp_pose[f]) if rp_point[q] != rp_point[f] and y.lvar[rp_point[q]]]
        if others:
            feat["feature-feature"].append(((POINT, int(rp_point[f])), (POINT, others[0])))
    while len(feat["feature-feature"]) < 30:              # none in common
        l, mm = (int(x) for x in rng.integers(len(prob["points"]), size=2))
        if l != mm and y.lvar[l] and y.lvar[mm] and not (poses_of(l) & poses_of(mm)):
            feat["feature-feature"].append(((POINT, l), (POINT, mm)))
    assert [len(v) for v in feat.values()] == [30, 30, 30, 30]
    return off, feat


def test_pairs_off_the_pattern_and_pairs_with_a_feature_over_several_dissection_levels():
    """260 frames, 5 000 features, 24 objects, several dissection levels.  Pose-pose, pose-object and object-object pairs the product itself reports off
    the pattern (poses spread over the chain, the first and the last variable pose among them) against inv(S_oracle); pose-feature pairs (the pose observes
    the feature / does not), feature-object and feature-feature pairs (with and without a common observing pose) against the two formulas on the oracle's
    Jacobians and inv(S_oracle).  Bar max(1e-7, 10 d): 1e-7 is the project's bar at this size, d the disagreement of inv(S_oracle) with a Cholesky solve.
    Object pairs also agree with obvi_ba_object_covariances at that route's bar (1e-7 of the largest own entry)."""
    prob, y = dissected()
    g = helpers.product_ba(); synth.upload(g, prob)
    g.covariance_compute()
    assert g.problem_stats()["chol_levels"] >= 3          # (the plan exists once a pass has run)
    off, feat = dissected_pairs(g, prob, y)
    pairs = sum(off.values(), []) + sum(feat.values(), [])
    declare(g, pairs)
    for kind, c in list(off.items()) + list(feat.items()):
        y.check(g, c, 1e-7, "260 frames, " + kind)
    oo = served(g, off["object-object"])
    a, b = np.array([(p[0][1], p[1][1]) for p in off["object-object"]]).T
    merged = g.object_covariances(a, b)
    scale = float(np.abs(g.object_covariances(np.flatnonzero(y.ovar))).max())
    worst = max(float(np.abs(x - w).max()) / scale for x, w in zip(oo, merged))
    print("off-pattern object pairs against obvi_ba_object_covariances: %.3e (bar 1e-07)" % worst)
    assert worst < 1e-7


@pytest.mark.parametrize("which", ["ragged", "stereo"])
def test_ragged_and_stereo_structures(which):
    """pose-feature and feature-feature pairs on tracks longer than 40 frames (longer than a wavefront in the ragged problem), on features with two records of
    one frame (stereo) or three sightings from one pose, and on features with masked sightings; yardstick and bar of the 260-frame test."""
    if which == "ragged":
        prob = structure._ragged_problem()
    else:
        prob = synth.make_problem(P=60, L=300, O=0, seed=9, stereo=True, outlier_frac=0.0)
        keep = ~((prob["rp_point"] % 7 == 0) & (prob["rp_pose"] % 5 == 2))
        for k in ("rp_pose", "rp_point", "rp_cam", "rp_pixel", "rp_sigma", "rp_is_outlier"):
            if k in prob and np.ndim(prob[k]) > 0:
                prob[k] = prob[k][keep]
    rp_pose, rp_point = prob["rp_pose"], prob["rp_point"]
    tracks = np.bincount(rp_point, minlength=len(prob["points"]))
    frames = np.array([len(set(rp_pose[rp_point == l])) for l in range(len(prob["points"]))])
    by_length = [int(l) for l in np.argsort(-frames, kind="stable")]
    long_tracks = by_length[:6]
    if which == "ragged":
        assert frames[long_tracks[0]] > 64
    doubled = [int(l) for l in np.flatnonzero(tracks > frames)][:6]             # more than one record of a frame
    assert doubled and (which == "ragged" or len(doubled) == 6)
    # every third sighting of six features of middling length is masked (at least two stay)
    dimmed = [l for l in by_length[40:] if tracks[l] >= 6][:6]
    mask = np.ones(len(rp_pose), np.uint8)
    for l in dimmed:
        mask[np.flatnonzero(rp_point == l)[::3]] = 0
    y = Yardstick(prob, mask)
    g = helpers.product_ba(); synth.upload(g, prob); g.set_active_mask(0, mask)
    feats = [l for l in dict.fromkeys(long_tracks + doubled + dimmed) if y.lvar[l]]
    assert len(feats) >= 12
    pv = np.flatnonzero(y.pvar)
    pairs = [((POINT, a), (POINT, b)) for x, a in enumerate(feats) for b in feats[x:]]
    for l in feats:
        seen = sorted({int(rp_pose[f]) for f in y.obs(l)} & set(pv.tolist()))
        unseen = [int(p) for p in pv if p not in seen]
        pairs += [((POSE, p), (POINT, l)) for p in (seen[0], seen[-1], unseen[0], unseen[-1])]
    if len(prob["objects"]):
        pairs += [((POINT, l), (OBJ, 0)) for l in feats]
    declare(g, pairs)
    y.check(g, pairs, 1e-7, which)


def test_joint_covariance_of_a_pose_and_a_feature_it_observes_is_positive_definite():
    """50 observations of the 260-frame problem: [[pose, cross], [cross^T, feature]] from the own blocks and the declared cross block is symmetric positive definite"""
    prob, y = dissected()
    g = helpers.product_ba(); synth.upload(g, prob)
    rng = np.random.default_rng(5)
    live = [f for f in rng.permutation(len(prob["rp_pose"])) if y.pvar[prob["rp_pose"][f]] and y.lvar[prob["rp_point"][f]]][:50]
    p, l = prob["rp_pose"][live], prob["rp_point"][live]
    g.covariance_compute_pairs(POSE, p, POINT, l)
    pp, ll, pl, lp = g.pose_covariances(p), g.point_covariances(l), g.cross_covariances(POSE, p, POINT, l), g.cross_covariances(POINT, l, POSE, p)
    for i in range(50):
        joint = np.block([[pp[i], pl[i]], [lp[i], ll[i]]])
        assert np.abs(joint - joint.T).max() <= 1e-12 * np.abs(joint).max()
        assert np.all(np.linalg.eigvalsh(joint) > 0), (p[i], l[i])


def test_two_passes_on_a_deterministic_handle_are_bit_identical():
    prob, y = dissected()
    g = helpers.product_ba(deterministic=True); synth.upload(g, prob)
    g.covariance_compute()
    off, feat = dissected_pairs(g, prob, y)
    pairs = sum(off.values(), []) + sum(feat.values(), [])
    out = []
    for _ in range(2):
        declare(g, pairs)
        out.append(np.concatenate([x.ravel() for x in served(g, pairs)]))
    assert np.array_equal(out[0], out[1]) and np.any(out[0] != 0.0)


def test_contract():
    prob, y = dissected()
    g = helpers.product_ba(); synth.upload(g, prob)
    g.covariance_compute()
    off, feat = dissected_pairs(g, prob, y)
    (a, b), (c, d) = off["pose-pose"][0], off["pose-pose"][1]
    (fp, fl), (fp2, fl2) = feat["pose observes feature"][0], feat["pose observes feature"][1]
    refused_off = dict(match="status -1 .*not on the tile pattern")
    refused_feature = dict(match="status -1 .*features")
    not_ready = dict(match="status -5")

    def undeclared_are_refused():
        with pytest.raises(obvi_ba.ObviError, **refused_off):
            g.cross_covariances([POSE], [c[1]], [POSE], [d[1]])
        with pytest.raises(obvi_ba.ObviError, **refused_feature):
            g.cross_covariances([POSE], [fp2[1]], [POINT], [fl2[1]])
        assert g.covariance_on_pattern([POSE], [c[1]], [POSE], [d[1]])[0] == 0

    def declared_are_served():
        assert g.covariance_on_pattern([POSE, POSE, POINT], [a[1], fp[1], fl[1]], [POSE, POINT, POSE], [b[1], fl[1], fp[1]]).tolist() == [1, 1, 1]
        x, z = g.cross_covariances([POSE, POSE], [a[1], fp[1]], [POSE, POINT], [b[1], fl[1]])
        assert x.shape == (6, 6) and z.shape == (6, 3) and np.any(x != 0.0) and np.any(z != 0.0)

    undeclared_are_refused()
    g.covariance_compute_pairs([POSE, POSE], [a[1], fp[1]], [POSE, POINT], [b[1], fl[1]])
    declared_are_served()
    undeclared_are_refused()                              # ... with today's statuses and messages
    # the declared set dies with the result
    po, pt, ob = g.get_state()
    g.update_state(po, pt, ob)
    for call in (lambda: g.cross_covariances([POSE], [a[1]], [POSE], [b[1]]), lambda: g.covariance_on_pattern([POSE], [fp[1]], [POINT], [fl[1]])):
        with pytest.raises(obvi_ba.ObviError, **not_ready):
            call()
    g.covariance_compute_pairs([POSE, POSE], [a[1], fp[1]], [POSE, POINT], [b[1], fl[1]])
    declared_are_served()
    g.solve(helpers.ba_params(max_it=1))
    with pytest.raises(obvi_ba.ObviError, **not_ready):
        g.cross_covariances([POSE], [a[1]], [POSE], [b[1]])
    g.covariance_compute_pairs([POSE, POSE], [a[1], fp[1]], [POSE, POINT], [b[1], fl[1]])
    declared_are_served()
    g.covariance_compute()                                # a plain pass clears the set: refused again
    with pytest.raises(obvi_ba.ObviError, **refused_off):
        g.cross_covariances([POSE], [a[1]], [POSE], [b[1]])
    with pytest.raises(obvi_ba.ObviError, **refused_feature):
        g.cross_covariances([POSE], [fp[1]], [POINT], [fl[1]])
    assert g.covariance_on_pattern([POSE], [a[1]], [POSE], [b[1]])[0] == 0
    # n = 0 is a plain pass
    g.covariance_compute_pairs([], [], [], [])
    assert np.any(g.pose_covariances([a[1]]) != 0.0)
    # a bad kind or index is refused before any device work: the result of the pass before stays valid
    P, L, O = len(prob["poses"]), len(prob["points"]), len(prob["objects"])
    with pytest.raises(obvi_ba.ObviError, match="status -1 .*unknown block kind"):
        g.covariance_compute_pairs([3], [0], [POSE], [a[1]])
    for kind, count in ((POSE, P), (POINT, L), (OBJ, O)):
        with pytest.raises(obvi_ba.ObviError, match="status -4"):
            g.covariance_compute_pairs([POSE], [a[1]], [kind], [count])
    assert np.any(g.pose_covariances([a[1]]) != 0.0)


def test_a_handle_that_exchanges_refuses_declared_pairs():
    prob = ref.small_problem()
    g = helpers.product_ba(); synth.upload(g, prob)
    calls = []
    g.set_shared_objects(np.ones(len(prob["objects"]), np.uint8), 0, 1)
    g.set_allreduce(lambda ptr, n, op, stream: calls.append(n) or 0)
    with pytest.raises(obvi_ba.ObviError, match="status -1 .*exchanges"):
        g.covariance_compute_pairs([POSE], [2], [POINT], [0])
    assert calls == []                                    # ... before any collective
    g.covariance_compute_pairs([], [], [], [])            # n = 0: the collective plain pass
    assert calls and np.any(g.pose_covariances([2]) != 0.0)


def test_a_free_gauge_is_a_status_not_a_fault():
    """no constant pose, one camera: rank deficient -> OBVI_ERR_NUMERICAL from the declared-pairs pass too, and the handle goes on working"""
    prob = synth.make_problem(P=12, L=30, O=2, seed=5, min_obj_obs=4, object_classes=("bench", "chair"), const_poses=0)
    g = helpers.product_ba(); synth.upload(g, prob)
    with pytest.raises(obvi_ba.ObviError, match="status -6"):
        g.covariance_compute_pairs([POSE, POSE, POINT], [0, 0, 1], [POSE, POINT, OBJ], [11, 3, 1])
    with pytest.raises(obvi_ba.ObviError, match="status -5"):
        g.cross_covariances([POSE], [0], [POINT], [3])
    assert g.solve(helpers.ba_params(max_it=3)).num_iterations >= 1
