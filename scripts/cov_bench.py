#!/usr/bin/env python3
"""Times obvi_ba_object_covariances on BASELINE config #3 (200 objects, own blocks) and, with --oracle, the CPU restatement
on a smaller problem of the same shape; with --selinv, the selected-inversion entries of include/obvi_cov.h (compute split into linearise + factorise and
inversion, reading all pose / feature blocks) beside the merged route and a one-iteration solve, at config #3's sizes and at 500 frames / 50 objects.
usage: python scripts/cov_bench.py [--oracle] [--selinv]"""
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
