#!/usr/bin/env python3
"""BASELINE config #5 on one GPU: sessions over the same place chained through the long-term map
(ltm_trajectory_sequence_executor.py:45-92 runs the reference's sessions one after the other in the same way): session s
= local-BA-sized problem (500 keyframes / 50 000 features) over one shared object set; it starts from the map of session
s-1 (ellipsoid estimates + marginal covariances as IndependentObjectMapFactor priors), runs the two-phase BA and ends by
extracting the new map on the device.  Prints per-session times and the map's error against the synthetic truth.
usage: python scripts/multi_session.py [sessions=16] [objects=200]
       python scripts/multi_session.py --concurrent [sessions=4] [objects=50]
       python scripts/multi_session.py --concurrent --resident-map [sessions=4] [objects=50]
--concurrent: the sessions run at the same time instead, one handle each behind one group, as ONE joint solve over the shared map, and the job ends
with the map of the joint solve (the collective obvi_cov_compute through dist_util.joint_long_term_map): estimates and joint covariances of the shared objects.
--resident-map (with --concurrent): TWO concurrent jobs chained through a map that never leaves the device: the first job's joint posterior is
born as an obvi_ba.Map, member 0 of the second job cuts its group prior over all objects from that map, and the second job's joint posterior is folded back
into it -- dist_util.resident_map_prior / joint_resident_map.  Only the report at the end reads a map back."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "obvi-slam_amd", "python")]
import numpy as np
import obvi_ba, synth

concurrent = "--concurrent" in sys.argv
resident = "--resident-map" in sys.argv
args = [a for a in sys.argv[1:] if a not in ("--concurrent", "--resident-map")]
n_sessions = int(args[0]) if len(args) > 0 else (4 if concurrent else 16)
n_objects = int(args[1]) if len(args) > 1 else (50 if concurrent else 200)
prm = obvi_ba.SolverParams(max_num_iterations=50, allow_non_monotonic_steps=True, function_tolerance=1e-4, gradient_tolerance=1e-10,
                           parameter_tolerance=1e-8, initial_trust_region_radius=100.0, max_trust_region_radius=1e4)

def concurrent_sessions():
    import dist_util
    t0 = time.time()
    sessions = synth.make_sessions(n_sessions, P=500, L=50000, O=n_objects, seed0=1000, object_seed=77, const_poses=1, min_obj_obs=10, object_classes=("bench",))
    t1 = time.time()
    group = dist_util.RcclGroup(n_sessions)
    group.set_timeout(120.0)
    handles = []
    for m, q in enumerate(sessions):
        ba = obvi_ba.BundleAdjuster(device_id=0)
        synth.upload(ba, q)
        group.attach(m, ba, np.ones(n_objects, np.uint8))
        handles.append(ba)
    t2 = time.time()
    out = dist_util.run_members([lambda h=h: h.solve(prm) for h in handles])
    for o in out:
        if isinstance(o, Exception):
            raise o
    t3 = time.time()
    ltm = dist_util.joint_long_term_map(handles, np.arange(n_objects))
    t4 = time.time()
    gt = sessions[0]["gt_objects"]
    err = np.linalg.norm(ltm["mean"][:, :3] - gt[:, :3], axis=1)
    sd = np.sqrt(np.einsum("oii->oi", ltm["cov"])[:, :3]).mean(axis=1)
    print("%d concurrent sessions over %d objects: joint solve %.1f ms (%d iterations, final cost %.6e) | joint map %.2f ms (%d collectives in all) | generation %.0f ms, upload %.0f ms | centre error median %.3f m, sigma median %.3f m"
          % (n_sessions, n_objects, (t3 - t2) * 1e3, out[0].num_iterations, out[0].final_cost, (t4 - t3) * 1e3, group.stats()[0], (t1 - t0) * 1e3, (t2 - t1) * 1e3, np.median(err), np.median(sd)), flush=True)
    for ba in handles:
        ba.close()
    group.close()


def resident_map_chain():
    import dist_util
    ids = np.arange(n_objects, dtype=np.uint32)
    mp = None
    for job in range(2):
        sessions = synth.make_sessions(n_sessions, P=500, L=50000, O=n_objects, seed0=1000 + 100 * job, object_seed=77, const_poses=1, min_obj_obs=10, object_classes=("bench",))
        group = dist_util.RcclGroup(n_sessions)
        group.set_timeout(120.0)
        handles = []
        for m, q in enumerate(sessions):
            ba = obvi_ba.BundleAdjuster(device_id=0)
            synth.upload(ba, q)
            group.attach(m, ba, np.ones(n_objects, np.uint8))
            handles.append(ba)
        t0 = time.time()
        dist_util.resident_map_prior(handles, mp, ids, ids, huber=1e6, uploader=0 if mp is not None else None)   # job 0: the switch alone, there is no map yet
        t1 = time.time()
        out = dist_util.run_members([lambda h=h: h.solve(prm) for h in handles])
        for o in out:
            if isinstance(o, Exception):
                raise o
        t2 = time.time()
        new = dist_util.joint_resident_map(handles, mp, ids, ids, new_obj=ids if mp is None else ())[0]
        t3 = time.time()
        if mp is not None:
            mp.close()
        mp = new
        mean, cov = mp.get()                                      # (the report alone: the chain itself never reads the map back)
        err = np.linalg.norm(mean[:, :3] - sessions[0]["gt_objects"][:, :3], axis=1)
        sd = np.sqrt(np.diag(cov).reshape(-1, 7)[:, :3]).mean(axis=1)
        print("job %d: %d concurrent sessions over %d objects%s: prior cut %.2f ms | joint solve %.1f ms (%d iterations, final cost %.6e) | posterior folded into the map %.2f ms (%d collectives in all) | centre error median %.3f m, sigma median %.3f m"
              % (job, n_sessions, n_objects, "" if job == 0 else ", prior from the resident map", (t1 - t0) * 1e3, (t2 - t1) * 1e3, out[0].num_iterations, out[0].final_cost, (t3 - t2) * 1e3, group.stats()[0],
                 np.median(err), np.median(sd)), flush=True)
        for ba in handles:
            ba.close()
        group.close()
    mp.close()


if concurrent:
    resident_map_chain() if resident else concurrent_sessions()
    sys.exit(0)
ltm = None   # (object ids, means, covariances)
g = obvi_ba.BundleAdjuster(device_id=0)
for s in range(n_sessions):
    t0 = time.time()
    prob = synth.make_problem(P=500, L=50000, O=n_objects, seed=1000 + s, object_seed=77, const_poses=1, min_obj_obs=10, object_classes=("bench",))
    if ltm is not None:
        prob["objects"][ltm[0]] = ltm[1]                          # a mapped object starts from the map
        prob.update(lt_obj=ltm[0].astype(np.uint32), lt_mean=ltm[1], lt_cov=ltm[2].reshape(-1, 49), lt_huber=1.0)
    t1 = time.time()
    synth.upload(g, prob)
    s1 = g.solve(prm)                                             # phase I
    mask, nex = g.select_outliers(0, 0.1)                         # phase II without the worst 10 % of the visual factors
    g.set_active_mask(0, mask)
    s2 = g.solve(prm)
    ids = np.arange(len(prob["objects"]), dtype=np.uint32)
    t2 = time.time()
    g.set_active_mask(0, np.ones_like(mask))                      # the extraction problem holds every factor again (a feature left with one sighting is rank deficient)
    cov = g.object_covariances(ids)
    t3 = time.time()
    est = g.get_objects()
    seen = np.abs(cov).max(axis=(1, 2)) > 0
    err = np.linalg.norm(est[seen, :3] - prob["gt_objects"][seen, :3], axis=1)
    sd = np.sqrt(np.einsum("oii->oi", cov[seen])[:, :3]).mean(axis=1)
    print("session %2d: %3d objects mapped | BA %5.1f ms (%2d + %2d iterations) | map extraction %5.2f ms | problem generation %4.0f ms | centre error median %.3f m, sigma median %.3f m"
          % (s, int(seen.sum()), (t2 - t1) * 1e3, s1.num_iterations, s2.num_iterations, (t3 - t2) * 1e3, (t1 - t0) * 1e3, np.median(err), np.median(sd)), flush=True)
    ltm = (ids[seen], est[seen], cov[seen])
