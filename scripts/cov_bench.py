#!/usr/bin/env python3
"""Times obvi_ba_object_covariances on BASELINE config #3 (200 objects, own blocks) and, with --oracle, the CPU restatement
on a smaller problem of the same shape; with --selinv, the selected-inversion entries of include/obvi_cov.h (compute split into linearise + factorise and
inversion, reading all pose / feature blocks) beside the merged route and a one-iteration solve, at config #3's sizes and at 500 frames / 50 objects.
With --shared K: K sessions of 500 frames / 50 000 features over one shared map of 50 objects behind one group -- the wall time of the COLLECTIVE
obvi_cov_compute (every member in a thread of its own), split as obvi_cov_get_stats splits it, beside K unshared handles doing the pass on their sessions alone
and one fused handle holding the joint problem.
With --pairs: obvi_cov_compute_pairs (include/obvi_cov_pairs.h) at 500 frames and at config #3 -- off-pattern pose pairs, observed pose-feature pairs and the
object pairs (o, o + 1) -- beside a plain obvi_cov_compute and obvi_ba_object_covariances on the same object pairs: median and range of the repeated runs.
usage: python scripts/cov_bench.py [--oracle] [--selinv] [--shared K] [--pairs]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "obvi-slam_amd", "python"), os.path.join(ROOT, "tests")]
import numpy as np
import obvi_ba, synth



def selinv_leg(g, prob, label, n=5):
    P, L, O = len(prob["poses"]), len(prob["points"]), len(prob["objects"])
    ids = np.arange(O)
    def timed(fn):
        fn(); t = time.time()
        for _ in range(n):
            out = fn()
        return (time.time() - t) / n * 1e3, out
    lin = inv = 0.0
    g.covariance_compute(); t = time.time()
    for _ in range(n):
        g.covariance_compute(); a, b, scratch = g.covariance_stats(); lin += a / n; inv += b / n
    total = (time.time() - t) / n * 1e3
    t_pose, cp = timed(lambda: g.pose_covariances(np.arange(P)))
    t_point, cl = timed(lambda: g.point_covariances(np.arange(L)))
    t_obj, co = timed(lambda: g.object_covariance_blocks(ids))
    t_merged, cm = timed(lambda: g.object_covariances(ids))
    one = obvi_ba.SolverParams(max_num_iterations=1, allow_non_monotonic_steps=True, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0,
                               initial_trust_region_radius=1e4, max_trust_region_radius=1e16)
    po, pt, ob = g.get_state()
    def one_iteration():
        g.update_state(po, pt, ob); return g.solve(one)
    t_solve, _ = timed(one_iteration)
    st = g.problem_stats()
    live = np.abs(cm).max(axis=(1, 2)) > 0
    print("%s: %d tile columns, %d non-zero tiles, %d levels; scratch %.1f MB (dense tile grid %.1f MB)" %
          (label, st["tiles_per_dim"], st["tiles_nonzero"], st["chol_levels"], scratch / 2 ** 20, st["tiles_per_dim"] ** 2 * 32768 / 2 ** 20))
    print("  obvi_cov_compute %.2f ms = linearise + factorise %.2f + selected inversion %.2f" % (total, lin, inv))
    print("  read all %d pose blocks %.2f ms, all %d feature blocks %.2f ms, %d object blocks %.2f ms" % (P, t_pose, L, t_point, O, t_obj))
    print("  obvi_ba_object_covariances (own blocks) %.2f ms; solve of one iteration (two LM steps) %.2f ms" % (t_merged, t_solve))
    print("  own object blocks, both routes: max relative difference %.2e; median pose sigma xyz %.3g m" %
          ((np.abs(co - cm).max(axis=(1, 2))[live] / np.abs(cm).max(axis=(1, 2))[live]).max(), np.median(np.sqrt(np.einsum("pii->pi", cp)[:, :3][np.einsum("pii->pi", cp)[:, 0] > 0]))))


def shared_leg(K, n=5, O=50):
    import dist_util
    warm = obvi_ba.SolverParams(max_num_iterations=6, allow_non_monotonic_steps=True, function_tolerance=1e-6, gradient_tolerance=1e-10,
                                parameter_tolerance=1e-8, initial_trust_region_radius=1e4, max_trust_region_radius=1e16)
    sessions = synth.make_sessions(K, P=500, L=50000, O=O, seed0=1000, object_seed=77, const_poses=1, min_obj_obs=10, object_classes=("bench",))

    def members(call, handles):
        out = dist_util.run_members([lambda h=h: call(h) for h in handles])
        for o in out:
            if isinstance(o, Exception):
                raise o
        return out

    def timed_pass(handles):
        members(lambda h: h.covariance_compute(), handles)
        wall, lin, inv = 0.0, 0.0, 0.0
        for _ in range(n):
            t = time.time(); members(lambda h: h.covariance_compute(), handles); wall += (time.time() - t) / n * 1e3
            st = [h.covariance_stats() for h in handles]
            lin += max(a for a, _, _ in st) / n; inv += max(b for _, b, _ in st) / n
        return wall, lin, inv

    def handles_of(problems, group=None):
        hs = []
        for m, q in enumerate(problems):
            ba = obvi_ba.BundleAdjuster(device_id=0); synth.upload(ba, q)
            if group is not None:
                group.attach(m, ba, np.ones(O, np.uint8))
            hs.append(ba)
        return hs
    print("%d sessions of 500 frames / 50 000 features over one map of %d objects; wall time per obvi_cov_compute of all members (threads), ms; the split is the slowest member's" % (K, O))
    group = dist_util.RcclGroup(K); group.set_timeout(120.0)
    hs = handles_of(sessions, group)
    members(lambda h: h.solve(warm), hs)
    c0 = group.stats()[0]
    wall, lin, inv = timed_pass(hs)
    per_pass = (group.stats()[0] - c0) / (n + 1)
    st = hs[0].problem_stats()
    print("  collective pass behind one group:   %.2f ms = linearise + factorise + %g collectives %.2f + selected inversion %.2f   (%d tile columns, %d levels per member)" %
          (wall, per_pass, lin, inv, st["tiles_per_dim"], st["chol_levels"]))
    states = [h.get_state() for h in hs]
    shared_blocks = hs[0].object_covariance_blocks(np.arange(O))
    for h in hs:
        h.close()
    group.close()
    alone = []
    for q, (po, pt, ob) in zip(sessions, states):
        a = dict(q); a.update(poses=po, points=pt, objects=ob); alone.append(a)
    hs = handles_of(alone)
    wall, lin, inv = timed_pass(hs)
    print("  %d unshared handles, sessions alone:  %.2f ms = linearise + factorise %.2f + selected inversion %.2f" % (K, wall, lin, inv))
    t = time.time()
    for _ in range(n):
        hs[0].covariance_compute()
    print("  one unshared handle by itself:       %.2f ms" % ((time.time() - t) / n * 1e3))
    for h in hs:
        h.close()
    joint = synth.join_problems(sessions)
    joint.update(poses=np.concatenate([s[0] for s in states]), points=np.concatenate([s[1] for s in states]), objects=states[0][2])
    hs = handles_of([joint])
    wall, lin, inv = timed_pass(hs)
    st = hs[0].problem_stats()
    fused_blocks = hs[0].object_covariance_blocks(np.arange(O))
    print("  one fused handle, the joint problem: %.2f ms = linearise + factorise %.2f + selected inversion %.2f   (%d tile columns, %d levels)" % (wall, lin, inv, st["tiles_per_dim"], st["chol_levels"]))
    print("  shared object blocks, collective against fused: max relative difference %.2e" % (np.abs(shared_blocks - fused_blocks).max(axis=(1, 2)) / np.abs(fused_blocks).max(axis=(1, 2))).max())
    hs[0].close()


def pairs_leg(g, prob, label, n=7):
    """median [min, max] ms over n runs after a warm-up run"""
    rng = np.random.default_rng(17)
    P, O = len(prob["poses"]), len(prob["objects"])
    def timed(fn):
        fn(); ts = []
        for _ in range(n):
            t = time.perf_counter(); fn(); ts.append((time.perf_counter() - t) * 1e3)
        return "%8.2f [%7.2f, %7.2f]" % (np.median(ts), min(ts), max(ts))
    g.covariance_compute()
    pv = np.flatnonzero(np.abs(g.pose_covariances(np.arange(P))).max(axis=(1, 2)) > 0)
    a, b = rng.choice(pv, 4000), rng.choice(pv, 4000)
    off = np.flatnonzero((g.covariance_on_pattern(0, a, 0, b) == 0) & (a != b))[:100]
    pa, pb = np.concatenate([[pv[0]], a[off]]), np.concatenate([[pv[-1]], b[off]])
    n_off = int((g.covariance_on_pattern(0, pa, 0, pb) == 0).sum())
    obs = rng.choice(len(prob["rp_pose"]), 10000, replace=False)
    oa = np.arange(O - 1)
    st = g.problem_stats()
    print("%s: %d tile columns, %d levels; median [min, max] ms over %d runs after a warm-up" % (label, st["tiles_per_dim"], st["chol_levels"], n))
    print("  obvi_cov_compute                                                  %s" % timed(g.covariance_compute))
    print("  obvi_cov_compute_pairs, %3d pose pairs (%d off the pattern)        %s" % (len(pa), n_off, timed(lambda: g.covariance_compute_pairs(0, pa, 0, pb))))
    print("  obvi_cov_compute_pairs, 10 000 observed pose-feature pairs        %s" % timed(lambda: g.covariance_compute_pairs(0, prob["rp_pose"][obs], 1, prob["rp_point"][obs])))
    print("  obvi_cov_compute_pairs, the %3d object pairs (o, o + 1)            %s" % (len(oa), timed(lambda: g.covariance_compute_pairs(2, oa, 2, oa + 1))))
    print("  obvi_ba_object_covariances, the same pairs                        %s" % timed(lambda: g.object_covariances(oa, oa + 1)))
    g.covariance_compute_pairs(2, oa, 2, oa + 1)
    new = np.array(g.cross_covariances(2, oa, 2, oa + 1)); old = g.object_covariances(oa, oa + 1)
    print("  the two routes on those pairs: max difference %.2e of the largest entry" % (np.abs(new - old).max() / np.abs(old).max()))
    g.covariance_compute()
    print("  (%d of them are off the pattern of the factor)" % int((g.covariance_on_pattern(2, oa, 2, oa + 1) == 0).sum()))


if "--shared" in sys.argv:
    shared_leg(int(sys.argv[sys.argv.index("--shared") + 1]))
    sys.exit(0)

if "--pairs" in sys.argv:
    only = sys.argv[sys.argv.index("--pairs") + 1] if len(sys.argv) > sys.argv.index("--pairs") + 1 else ""
    for label, kw in (("500 frames / 50 000 features / 50 objects", dict(P=500, L=50000, O=50, seed=3)), ("config #3: 2000 frames / 300 000 features / 200 objects", dict(P=2000, L=300000, O=200, seed=20241008))):
        if only and not label.startswith(only):
            continue
        pr = synth.make_problem(const_poses=1, min_obj_obs=10, **kw)
        gg = obvi_ba.BundleAdjuster(device_id=0); synth.upload(gg, pr)
        gg.solve(obvi_ba.SolverParams(max_num_iterations=10, allow_non_monotonic_steps=True, function_tolerance=1e-6, gradient_tolerance=1e-10,
                                      parameter_tolerance=1e-8, initial_trust_region_radius=1e4, max_trust_region_radius=1e16))
        pairs_leg(gg, pr, label)
        gg.close()
    sys.exit(0)

if "--selinv" in sys.argv:
    for label, kw in (("500 frames / 50 000 features / 50 objects", dict(P=500, L=50000, O=50, seed=3)), ("config #3: 2000 frames / 300 000 features / 200 objects", dict(P=2000, L=300000, O=200, seed=20241008))):
        pr = synth.make_problem(const_poses=1, min_obj_obs=10, **kw)
        gg = obvi_ba.BundleAdjuster(device_id=0); synth.upload(gg, pr)
        gg.solve(obvi_ba.SolverParams(max_num_iterations=10, allow_non_monotonic_steps=True, function_tolerance=1e-6, gradient_tolerance=1e-10,
                                      parameter_tolerance=1e-8, initial_trust_region_radius=1e4, max_trust_region_radius=1e16))
        selinv_leg(gg, pr, label)
        gg.close()
    sys.exit(0)

prob = synth.make_problem(P=2000, L=300000, O=200, seed=20241008, const_poses=1, min_obj_obs=10)
g = obvi_ba.BundleAdjuster(device_id=0)
synth.upload(g, prob)
g.solve(obvi_ba.SolverParams(max_num_iterations=10, allow_non_monotonic_steps=True, function_tolerance=1e-6, gradient_tolerance=1e-10,
                             parameter_tolerance=1e-8, initial_trust_region_radius=1e4, max_trust_region_radius=1e16))
ids = np.arange(len(prob["objects"]))
g.object_covariances(ids)
t = time.time(); n = 5
for _ in range(n):
    c = g.object_covariances(ids)
dt = (time.time() - t) / n
sd = np.sqrt(np.einsum("oii->oi", c))
print("covariances of %d objects: %.2f ms per call; median sigma xyz %.3g m, yaw %.3g rad, dims %.3g m" %
      (len(ids), dt * 1e3, np.median(sd[:, :3]), np.median(sd[:, 3]), np.median(sd[:, 4:])))
pairs = np.array([(a, b) for a in range(20) for b in range(a + 1, 20)])
t = time.time(); g.object_covariances(pairs[:, 0], pairs[:, 1]); print("190 cross blocks: %.2f ms" % ((time.time() - t) * 1e3))
if "--oracle" in sys.argv:
    import helpers
    small = synth.make_problem(P=500, L=50000, O=50, seed=3, const_poses=1, min_obj_obs=10)
    o = helpers.oracle_ba(); synth.upload(o, small)
    g2 = obvi_ba.BundleAdjuster(device_id=0); synth.upload(g2, small)
    ids2 = np.arange(len(small["objects"]))
    t = time.time(); co = o.object_covariances(ids2); to = time.time() - t
    g2.object_covariances(ids2); t = time.time(); cg = g2.object_covariances(ids2); tg = time.time() - t
    print("P=500 / 50 objects: oracle %.2f s, device %.2f ms, max relative difference %.2e" % (to, tg * 1e3, (np.abs(cg - co).max(axis=(1, 2)) / np.abs(co).max(axis=(1, 2))).max()))
