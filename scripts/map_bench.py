#!/usr/bin/env python
"""Group priors of one window, prepared on the host and on the device.  For od = 7 at 70, 210 and 1 400 rows, one group per call over an
objects-only problem: median and range of five calls of obvi_map_set_group_priors (host pointers: blocked Cholesky, triangular inverse, W^T W and the power steps
on the host's workers, then the upload) and of obvi_map_set_group_priors_from_map (the map already resident: gather, the same algebra and the condition estimate
on the device, one read-back).  Each entry is called once before it is timed (its first call allocates).  obvi_map_create's time is printed beside them.
--update: the way back instead -- obvi_map_condition_on_handle and obvi_map_condition at 70, 210 and 1 400 window rows on the same 200-object
map, against the round trip through the host that gives the same map without them.
--extend: a map that grows -- obvi_map_extend_on_handle and obvi_map_extend at 70 and 210 window rows of which 14 and 42 belong to objects
the map lacks, against the round trip that grows the map without them: obvi_map_get, object_covariances of all pairs, numpy, obvi_map_create.
--shared K: K concurrent sessions of 500 frames / 50 000 features over 50 shared objects behind one group: ms per joint LM step without and
with the whole-map group prior on member 0, and the wall time of the collective obvi_map_condition_on_handle (every member folds all 50 objects back) against
the same call on ONE handle that holds the joint problem.
--merge: a map that shrinks -- obvi_map_merge of 1, 10 and 30 pairs of the 200-object map (noise on every pair), wait included, against the
round trip that merges without it: obvi_map_get, the same formula in numpy, obvi_map_create.
--match: which objects are duplicates -- obvi_map_match over all 19 900 pairs of the 200-object map (whole block, no labels), both waits
included, against the only route without it: obvi_map_get and the same statistic vectorised in numpy; nothing is uploaded again on either side.
--move: another frame -- obvi_map_transform of the 200-object map without and with a transform covariance, wait included, against the round
trip that moves it without the entry: obvi_map_get, the same formula in numpy, obvi_map_create; obvi_map_join of two 200-object maps; and the move of a
800-object map (5 600 rows, 251 MB), where the covariance kernel is most of the call, beside the copy bandwidth obvi_ba_measure_peaks reports.
--locate: where another map lies -- obvi_map_locate of a 60-object moved and noisy part of the 200-object map in that map (no labels: 70 million
seeds), both waits and the refinement of the best 16 hypotheses included, against the only route without it: obvi_map_get of both maps and the same
hypothesise-and-score search vectorised in numpy.
usage (GPU box, repo root): python scripts/map_bench.py [--update | --extend | --merge | --match | --move | --locate | --shared K]"""
import os
import sys
import time

import numpy as np
import torch  # noqa: F401  (loaded before libobvi_ba.so, as in the tests)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "obvi-slam_amd", "python"))
import obvi_ba  # noqa: E402
import synth  # noqa: E402

OD, N_MAP, CALLS = 7, 200, 5


def spd(rng, n, cond=1e3, scale=1e-2):
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    ev = scale * np.exp(rng.uniform(0.0, np.log(cond), n))
    ev[0], ev[-1] = scale, scale * cond
    M = (Q * ev) @ Q.T
    return 0.5 * (M + M.T)


def timed(fn):
    fn()
    ms = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return "median %8.3f ms  (%.3f .. %.3f)" % (float(np.median(ms)), min(ms), max(ms)), float(np.median(ms))


def main():
    rng = np.random.default_rng(1)
    mean, cov = rng.normal(size=(N_MAP, OD)), spd(rng, N_MAP * OD)
    t0 = time.perf_counter()
    mp = obvi_ba.Map.create(mean, cov, object_block_size=OD)
    print("obvi_map_create, %d objects (%d rows, %.1f MB): %.3f ms" % (N_MAP, N_MAP * OD, cov.nbytes / 1e6, 1e3 * (time.perf_counter() - t0)))
    for k in (10, 30, 200):
        sel = rng.permutation(N_MAP)[:k]
        idx = np.concatenate([np.arange(OD * o, OD * o + OD) for o in sel])
        sub, mu = np.ascontiguousarray(cov[np.ix_(idx, idx)]), np.ascontiguousarray(mean[sel])
        ba = obvi_ba.BundleAdjuster(object_block_size=OD)
        ba.set_cameras(synth.K_DEFAULT[None], synth.EXT_DEFAULT[None])
        ba.set_poses(np.zeros((1, 6)), np.ones(1, np.uint8))
        ba.set_points(np.zeros((0, 3)), np.zeros(0, np.uint8))
        ba.set_objects(mu + 0.05, np.zeros(k, np.uint8))
        groups, maps = [list(range(k))], [list(sel)]
        host, h = timed(lambda: ba.set_map_group_priors(groups, [mu], [sub], 1e6))
        _, Wh, _ = ba.debug_linearize(obvi_ba.FACTOR_MAP_GROUP_PRIOR)
        dev, d = timed(lambda: ba.set_map_group_priors_from_map(mp, groups, maps, 1e6))
        _, Wd, _ = ba.debug_linearize(obvi_ba.FACTOR_MAP_GROUP_PRIOR)
        print("%5d rows: host entry %s   from the map %s   host / device %.2f   |W - W_host| / |W_host| %.1e"
              % (k * OD, host, dev, h / d, np.abs(Wd[0] - Wh[0]).max() / np.abs(Wh[0]).max()))
        ba.close()
    mp.close()


def numpy_update(mean, cov, sel, m, P):
    """The formulas of include/obvi_map_update.h on the host: what a session computes without the device entry."""
    idx = np.concatenate([np.arange(OD * o, OD * o + OD) for o in sel])
    Cs, Ps = 0.5 * (cov + cov.T), 0.5 * (P + P.T)
    Caa = Cs[np.ix_(idx, idx)]
    K = np.linalg.solve(Caa, Cs[idx]).T
    mu = mean.ravel() + K @ (m.ravel() - mean.ravel()[idx])
    Cn = Cs - K @ (Caa - Ps) @ K.T
    Cn = 0.5 * (Cn + Cn.T)
    Cn[np.ix_(idx, idx)] = Ps
    mu[idx] = m.ravel()
    return mu.reshape(-1, OD), Cn


def update():
    """a window's posterior folded back into the map.  Both device entries against the round trip a session needs without them: object_covariances
    of the k^2 pairs, numpy_update on the host, obvi_map_create."""
    rng = np.random.default_rng(1)
    mean, cov = rng.normal(size=(N_MAP, OD)), spd(rng, N_MAP * OD)
    mp = obvi_ba.Map.create(mean, cov, object_block_size=OD)
    for k in (10, 30, 200):
        sel = rng.permutation(N_MAP)[:k]
        ba = obvi_ba.BundleAdjuster(object_block_size=OD)
        ba.set_cameras(synth.K_DEFAULT[None], synth.EXT_DEFAULT[None])
        ba.set_poses(np.zeros((1, 6)), np.ones(1, np.uint8))
        ba.set_points(np.zeros((0, 3)), np.zeros(0, np.uint8))
        ba.set_objects(mean[sel] + 0.05, np.zeros(k, np.uint8))
        obj = np.arange(k)
        ba.set_map_group_priors_from_map(mp, [list(obj)], [list(sel)], 1e6)
        ba.set_ltm_priors(obj, mean[sel] + 0.02, np.tile((0.05 * np.eye(OD)).ravel(), (k, 1)), 1e6)      # what the window measured
        ba.solve(obvi_ba.SolverParams(max_num_iterations=10, allow_non_monotonic_steps=True, function_tolerance=1e-6, initial_trust_region_radius=100.0,
                                      max_trust_region_radius=1e4))
        pa, pb = np.repeat(obj, k), np.tile(obj, k)

        def posterior():
            P = ba.object_covariances(pa, pb).reshape(k, k, OD, OD).transpose(0, 2, 1, 3).reshape(k * OD, k * OD)
            return ba.get_objects(), P
        m, P = posterior()
        last = {}

        def round_trip():
            mm, PP = posterior()
            mu, Cn = numpy_update(mean, cov, sel, mm, PP)
            with obvi_ba.Map.create(mu, Cn, object_block_size=OD) as new:
                last["host"] = (mu, Cn, new.n_objects)

        def on_handle():
            with mp.condition_on(ba, obj, sel) as new:
                last["n"] = new.n_objects

        def host_pointers():
            with mp.condition(ba, sel, m, P) as new:
                last["n"] = new.n_objects
        base, b = timed(round_trip)
        dev_on, d1 = timed(on_handle)
        dev_hp, d2 = timed(host_pointers)
        with mp.condition_on(ba, obj, sel) as new:
            mu, Cn = new.get()
        print("%5d window rows: round trip %s   condition_on_handle %s  (x %.1f)   condition %s  (x %.1f)   |C' - numpy's| / |C'| %.1e"
              % (k * OD, base, dev_on, b / d1, dev_hp, b / d2, np.abs(Cn - last["host"][1]).max() / np.abs(Cn).max()))
        ba.close()
    mp.close()


def numpy_extend(mean, cov, sel, m, P, k_new):
    """The formulas of include/obvi_map_extend.h on the host."""
    n, k_old = len(mean), len(sel)
    N, NA = n * OD, k_old * OD
    Ps = 0.5 * (P + P.T)
    mu, Cn = np.zeros((n + k_new, OD)), np.zeros((N + k_new * OD, N + k_new * OD))
    mu[:n], Cn[:N, :N] = numpy_update(mean, cov, sel, m[:k_old], P[:NA, :NA])
    idx = np.concatenate([np.arange(OD * o, OD * o + OD) for o in sel])
    Cs = 0.5 * (cov + cov.T)
    K = np.linalg.solve(Cs[np.ix_(idx, idx)], Cs[idx]).T
    Cn[:N, N:] = K @ Ps[:NA, NA:]
    Cn[N:, :N] = Cn[:N, N:].T
    rows = np.concatenate([idx, np.arange(N, N + k_new * OD)])
    Cn[np.ix_(rows, rows)] = Ps
    mu[n:] = m[k_old:]
    return mu, Cn


def extend():
    """a window's new objects appended to the map.  Both device entries against the round trip a session needs without them."""
    rng = np.random.default_rng(1)
    mean, cov = rng.normal(size=(N_MAP, OD)), spd(rng, N_MAP * OD)
    mp = obvi_ba.Map.create(mean, cov, object_block_size=OD)
    for k, k_new in ((10, 2), (30, 6)):
        k_old = k - k_new
        sel = rng.permutation(N_MAP)[:k_old]
        start = np.concatenate([mean[sel] + 0.05, rng.normal(size=(k_new, OD))])
        ba = obvi_ba.BundleAdjuster(object_block_size=OD)
        ba.set_cameras(synth.K_DEFAULT[None], synth.EXT_DEFAULT[None])
        ba.set_poses(np.zeros((1, 6)), np.ones(1, np.uint8))
        ba.set_points(np.zeros((0, 3)), np.zeros(0, np.uint8))
        ba.set_objects(start, np.zeros(k, np.uint8))
        obj = np.arange(k)
        old, new_obj = obj[:k_old], obj[k_old:]
        ba.set_map_group_priors_from_map(mp, [list(old)], [list(sel)], 1e6)
        ba.set_ltm_priors(obj, start - 0.03, np.tile((0.05 * np.eye(OD)).ravel(), (k, 1)), 1e6)      # what the window measured: the new objects have nothing else
        ba.solve(obvi_ba.SolverParams(max_num_iterations=10, allow_non_monotonic_steps=True, function_tolerance=1e-6, initial_trust_region_radius=100.0,
                                      max_trust_region_radius=1e4))
        pa, pb = np.repeat(obj, k), np.tile(obj, k)

        def posterior():
            P = ba.object_covariances(pa, pb).reshape(k, k, OD, OD).transpose(0, 2, 1, 3).reshape(k * OD, k * OD)
            return ba.get_objects(), P
        m, P = posterior()
        last = {}

        def round_trip():
            old_mean, old_cov = mp.get()
            mm, PP = posterior()
            mu, Cn = numpy_extend(old_mean, old_cov, sel, mm, PP, k_new)
            with obvi_ba.Map.create(mu, Cn, object_block_size=OD) as new:
                last["host"] = (mu, Cn, new.n_objects)

        def on_handle():
            with mp.extend_on(ba, old, sel, new_obj) as new:
                last["n"] = new.n_objects

        def host_pointers():
            with mp.extend(ba, sel, m, P, k_new) as new:
                last["n"] = new.n_objects
        base, b = timed(round_trip)
        dev_on, d1 = timed(on_handle)
        dev_hp, d2 = timed(host_pointers)
        with mp.extend_on(ba, old, sel, new_obj) as new:
            mu, Cn = new.get()
        print("%5d window rows, %3d of them new: round trip %s   extend_on_handle %s  (x %.1f)   extend %s  (x %.1f)   |C' - numpy's| / |C'| %.1e"
              % (k * OD, k_new * OD, base, dev_on, b / d1, dev_hp, b / d2, np.abs(Cn - last["host"][1]).max() / np.abs(Cn).max()))
        ba.close()
    mp.close()


def numpy_merge(mean, cov, drop, keep, offset, noise):
    """The formulas of include/obvi_map_merge.h on the host."""
    n, q = len(mean), len(drop)
    Cs = 0.5 * (cov + cov.T)
    rows = lambda o: np.concatenate([np.arange(OD * x, OD * x + OD) for x in o])   # noqa: E731
    rb, rk = rows(drop), rows(keep)
    G = Cs[:, rb] - Cs[:, rk]                                                       # Cs H^T
    Tm = G[rb] - G[rk]
    for r in range(q):
        Tm[OD * r:OD * r + OD, OD * r:OD * r + OD] += 0.5 * (noise[r] + noise[r].T)
    resid = mean.ravel()[rb] - mean.ravel()[rk] - offset.ravel()
    K = np.linalg.solve(0.5 * (Tm + Tm.T), G.T).T
    kept = rows(np.setdiff1d(np.arange(n), drop))
    mu = (mean.ravel() - K @ resid)[kept]
    Cn = (Cs - K @ G.T)[np.ix_(kept, kept)]
    return mu.reshape(-1, OD), 0.5 * (Cn + Cn.T)


def merge():
    """duplicate objects of the map merged.  The device entry against the round trip a session needs without it."""
    rng = np.random.default_rng(1)
    mean, cov = rng.normal(size=(N_MAP, OD)), spd(rng, N_MAP * OD)
    mp = obvi_ba.Map.create(mean, cov, object_block_size=OD)
    ba = obvi_ba.BundleAdjuster(object_block_size=OD)
    ba.set_cameras(synth.K_DEFAULT[None], synth.EXT_DEFAULT[None])
    ba.set_poses(np.zeros((1, 6)), np.ones(1, np.uint8))
    ba.set_points(np.zeros((0, 3)), np.zeros(0, np.uint8))
    ba.set_objects(np.zeros((1, OD)), np.zeros(1, np.uint8))
    for q in (1, 10, 30):
        perm = rng.permutation(N_MAP)
        drop, keep = perm[:q], perm[q:2 * q]
        offset = 0.1 * rng.normal(size=(q, OD))
        A = rng.normal(size=(q, OD, OD))
        noise = 1e-3 * (A @ A.transpose(0, 2, 1) + OD * np.eye(OD))
        last = {}

        def round_trip():
            old_mean, old_cov = mp.get()
            mu, Cn = numpy_merge(old_mean, old_cov, drop, keep, offset, noise)
            with obvi_ba.Map.create(mu, Cn, object_block_size=OD) as new:
                last["host"] = (mu, Cn, new.n_objects)

        def device():
            new, _ = mp.merge(ba, drop, keep, offset, noise)
            with new:
                last["n"] = new.n_objects
        base, b = timed(round_trip)
        dev, d = timed(device)
        new, _ = mp.merge(ba, drop, keep, offset, noise)
        with new:
            mu, Cn = new.get()
        print("%3d pairs (%4d rows), %d -> %d map rows: round trip %s   obvi_map_merge %s  (x %.1f)   |C' - numpy's| / |C'| %.1e"
              % (q, q * OD, N_MAP * OD, (N_MAP - q) * OD, base, dev, b / d, np.abs(Cn - last["host"][1]).max() / np.abs(Cn).max()))
    ba.close()
    mp.close()


def numpy_match(mean, cov, gate):
    """The statistic of include/obvi_map_match.h for every pair on the host, vectorised: whole block, no labels, no distance."""
    n = len(mean)
    a, b = np.triu_indices(n, 1)
    blocks = (0.5 * (cov + cov.T)).reshape(n, OD, n, OD).transpose(0, 2, 1, 3)
    Tm = blocks[b, b] - blocks[b, a] - blocks[a, b] + blocks[a, a]
    d = mean[b] - mean[a]
    s = np.einsum("pi,pi->p", d, np.linalg.solve(Tm, d[:, :, None])[:, :, 0])
    hit = s <= gate
    return a[hit], b[hit], s[hit]


def match():
    """duplicate objects of the map proposed.  The device entry (a count-only call, then one of the exact size) against the only route without
    it: obvi_map_get and the same statistic in numpy; nothing is uploaded again on either side."""
    rng = np.random.default_rng(1)
    mean, cov = rng.normal(size=(N_MAP, OD)), spd(rng, N_MAP * OD)
    mp = obvi_ba.Map.create(mean, cov, object_block_size=OD)
    ba = obvi_ba.BundleAdjuster(object_block_size=OD)
    ba.set_cameras(synth.K_DEFAULT[None], synth.EXT_DEFAULT[None])
    ba.set_poses(np.zeros((1, 6)), np.ones(1, np.uint8))
    ba.set_points(np.zeros((0, 3)), np.zeros(0, np.uint8))
    ba.set_objects(np.zeros((1, OD)), np.zeros(1, np.uint8))
    pairs = N_MAP * (N_MAP - 1) // 2
    s_all = numpy_match(mean, cov, np.inf)[2]
    for want in (20, pairs):
        v = np.sort(s_all)
        gate = 0.5 * (v[want - 1] + v[want]) if want < pairs else 2.0 * v[-1]
        last = {}

        def round_trip():
            old_mean, old_cov = mp.get()
            last["host"] = numpy_match(old_mean, old_cov, gate)

        def device():
            last["dev"] = mp.match(ba, gate)

        def device_sized():
            last["dev"] = mp.match(ba, gate, capacity=pairs)
        base, b = timed(round_trip)
        two, d2 = timed(device)
        one, d1 = timed(device_sized)
        ha, hb, hs = last["host"]
        da, db, ds, _, counts = last["dev"]
        same = np.array_equal(ha, da) and np.array_equal(hb, db)
        print("%d objects (%d rows, %d pairs), %5d found: obvi_map_get + numpy %s   obvi_map_match, count then exact size %s  (x %.1f)   one call, capacity = all pairs %s  (x %.1f)   "
              "same pairs: %s   |s - numpy's| / s %.1e" % (N_MAP, N_MAP * OD, pairs, counts[0], base, two, b / d2, one, b / d1, same, float((np.abs(ds - hs) / hs).max()) if same else np.nan))
    ba.close()
    mp.close()


def numpy_move(mean, cov, T, Sigma):
    """The formulas of include/obvi_map_frame.h on the host (od 7)."""
    n = len(mean)
    c, s = np.cos(T[3]), np.sin(T[3])
    J = np.eye(OD)
    J[:2, :2] = [[c, -s], [s, c]]
    mu = mean @ J.T
    mu[:, :3] += T[:3]
    mu[:, 3] += T[3]
    Cn = np.einsum("ik,akbl,jl->aibj", J, (0.5 * (cov + cov.T)).reshape(n, OD, n, OD), J).reshape(n * OD, n * OD)
    if Sigma is not None:
        G = np.zeros((n, OD, 4))
        G[:, :3, :3], G[:, 3, 3] = np.eye(3), 1.0
        G[:, 0, 3], G[:, 1, 3] = -s * mean[:, 0] - c * mean[:, 1], c * mean[:, 0] - s * mean[:, 1]
        G = G.reshape(n * OD, 4)
        Cn += G @ (0.5 * (Sigma + Sigma.T)) @ G.T
    return mu, 0.5 * (Cn + Cn.T)


def move():
    """the map moved into another frame, and two maps joined.  The device entries against the round trip a session needs without them."""
    rng = np.random.default_rng(1)
    mean, cov = rng.normal(size=(N_MAP, OD)), spd(rng, N_MAP * OD)
    mp = obvi_ba.Map.create(mean, cov, object_block_size=OD)
    ba = obvi_ba.BundleAdjuster(object_block_size=OD)
    ba.set_cameras(synth.K_DEFAULT[None], synth.EXT_DEFAULT[None])
    ba.set_poses(np.zeros((1, 6)), np.ones(1, np.uint8))
    ba.set_points(np.zeros((0, 3)), np.zeros(0, np.uint8))
    ba.set_objects(np.zeros((1, OD)), np.zeros(1, np.uint8))
    T = np.array([3.0, -2.0, 0.5, 0.7])
    A = rng.normal(size=(4, 4))
    for Sigma in (None, 1e-2 * (A @ A.T + 4 * np.eye(4))):
        last = {}

        def round_trip():
            old_mean, old_cov = mp.get()
            mu, Cn = numpy_move(old_mean, old_cov, T, Sigma)
            with obvi_ba.Map.create(mu, Cn, object_block_size=OD) as new:
                last["host"] = (mu, Cn, new.n_objects)

        def device():
            with mp.transform(ba, T, Sigma) as new:
                last["n"] = new.n_objects
        base, b = timed(round_trip)
        dev, d = timed(device)
        with mp.transform(ba, T, Sigma) as new:
            mu, Cn = new.get()
        print("%d objects (%d rows), %s: round trip %s   obvi_map_transform %s  (x %.1f)   |C' - numpy's| / |C'| %.1e"
              % (N_MAP, N_MAP * OD, "exact transform" if Sigma is None else "with Sigma", base, dev, b / d, np.abs(Cn - last["host"][1]).max() / np.abs(Cn).max()))

    def join():
        with mp.join(ba, mp) as new:
            assert new.n_objects == 2 * N_MAP
    print("obvi_map_join of two %d-object maps (%d rows, %.1f MB written): %s" % (N_MAP, 2 * N_MAP * OD, 8e-6 * (2 * N_MAP * OD) ** 2, timed(join)[0]))
    mp.close()
    n_big = 800
    N = n_big * OD
    big = 1e-3 * rng.normal(size=(N, N))
    big += big.T
    np.fill_diagonal(big, 1.0)
    peaks = ba.measure_peaks()
    with obvi_ba.Map.create(rng.normal(size=(n_big, OD)), big, object_block_size=OD) as wide:
        def device_big():
            wide.transform(ba, T, Sigma).close()
        txt, ms = timed(device_big)
        print("%d objects (%d rows, %.0f MB read and as much written): obvi_map_transform %s -- the whole call, allocation, two launches and the wait: %.0f GB/s   "
              "(copy bandwidth of obvi_ba_measure_peaks: %.0f GB/s)" % (n_big, N, 8e-6 * N * N, txt, 2 * 8e-6 * N * N / ms, peaks["hbm_copy_gbs"]))
    ba.close()


def numpy_locate(mean_a, cov_a, mean_b, cov_b, dmin, tol, gate, min_inliers):
    """The search of include/obvi_map_locate.h on the host, fp64, up to the ranking: (counts, best seed, its inliers, its cost)."""
    def records(mean, cov):
        n = len(mean)
        Cs = 0.5 * (cov + cov.T)
        return mean[:, :3], np.array([Cs[OD * o:OD * o + 3, OD * o:OD * o + 3] for o in range(n)])
    pa, A = records(mean_a, cov_a)
    pb, B = records(mean_b, cov_b)
    na, nb = len(pa), len(pb)
    a1, a2 = np.triu_indices(na, 1)
    b1, b2 = np.divmod(np.arange(nb * nb), nb)
    b1, b2 = b1[b1 != b2], b2[b1 != b2]
    u, v = pa[a2] - pa[a1], pb[b2] - pb[b1]
    nu, nv = np.hypot(u[:, 0], u[:, 1]), np.hypot(v[:, 0], v[:, 1])
    rows, cols = np.flatnonzero(nu >= dmin), np.flatnonzero(nv >= dmin)
    seeds = []
    for r0 in range(0, len(rows), 512):                                # 512 rows of A pairs against every B pair at a time
        r = rows[r0:r0 + 512]
        ok = (np.abs(nu[r, None] - nv[None, cols]) <= tol) & (np.abs(u[r, 2][:, None] - v[cols, 2][None, :]) <= tol)
        i, j = np.nonzero(ok)
        seeds.append(np.column_stack([a1[r[i]], a2[r[i]], b1[cols[j]], b2[cols[j]]]))
    seeds = np.concatenate(seeds)
    sa1, sa2, sb1, sb2 = seeds.T
    su, sv = pa[sa2] - pa[sa1], pb[sb2] - pb[sb1]
    psi = np.arctan2(sv[:, 0] * su[:, 1] - sv[:, 1] * su[:, 0], sv[:, 0] * su[:, 0] + sv[:, 1] * su[:, 1])
    cs, sn = np.cos(psi), np.sin(psi)
    ma, mb = 0.5 * (pa[sa1] + pa[sa2]), 0.5 * (pb[sb1] + pb[sb2])
    t = np.column_stack([ma[:, 0] - (cs * mb[:, 0] - sn * mb[:, 1]), ma[:, 1] - (sn * mb[:, 0] + cs * mb[:, 1]), ma[:, 2] - mb[:, 2]])
    inl, cost = np.zeros(len(seeds), np.int64), np.zeros(len(seeds))
    for h0 in range(0, len(seeds), 64):
        h = slice(h0, h0 + 64)
        R = np.zeros((len(cs[h]), 3, 3))
        R[:, 0, 0], R[:, 0, 1], R[:, 1, 0], R[:, 1, 1], R[:, 2, 2] = cs[h], -sn[h], sn[h], cs[h], 1.0
        e = pa[None, None] - (np.einsum("hij,bj->hbi", R, pb) + t[h, None])[:, :, None]
        S = A[None, None] + np.einsum("hij,bjk,hlk->hbil", R, B, R)[:, :, None]
        s = np.einsum("hbai,hbai->hba", e, np.linalg.solve(S, e[..., None])[..., 0])
        best = s.min(axis=2)
        inl[h], cost[h] = (best <= gate).sum(axis=1), np.where(best <= gate, best, 0.0).sum(axis=1)
    q = np.flatnonzero(inl >= min_inliers)
    first = q[np.lexsort((q, cost[q], -inl[q]))[0]]
    return (na * (na - 1) // 2 * nb * (nb - 1), len(seeds), len(q)), seeds[first], int(inl[first]), float(cost[first])


def locate():
    """one map located in another.  The device entry against the only route without it."""
    rng = np.random.default_rng(1)
    n_b = 60
    mean = rng.normal(size=(N_MAP, OD))
    mean[:, :2], mean[:, 2] = rng.uniform(-50.0, 50.0, size=(N_MAP, 2)), rng.uniform(0.0, 3.0, size=N_MAP)
    cov = spd(rng, N_MAP * OD)
    cov *= 0.03 ** 2 / np.diag(cov).mean()
    T = np.array([-4.0, 2.5, 0.3, -1.1])
    c, s = np.cos(T[3]), np.sin(T[3])
    part = rng.permutation(N_MAP)[:n_b]
    mean_b = mean[part].copy()
    mean_b[:, :3] = (mean[part, :3] - T[:3]) @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    cov_b = spd(rng, n_b * OD)
    cov_b *= 0.03 ** 2 / np.diag(cov_b).mean()
    mean_b += (np.linalg.cholesky(cov_b) @ rng.normal(size=n_b * OD)).reshape(n_b, OD)
    ma, mb = obvi_ba.Map.create(mean, cov, object_block_size=OD), obvi_ba.Map.create(mean_b, cov_b, object_block_size=OD)
    ba = obvi_ba.BundleAdjuster(object_block_size=OD)
    ba.set_cameras(synth.K_DEFAULT[None], synth.EXT_DEFAULT[None])
    ba.set_poses(np.zeros((1, 6)), np.ones(1, np.uint8))
    ba.set_points(np.zeros((0, 3)), np.zeros(0, np.uint8))
    ba.set_objects(np.zeros((1, OD)), np.zeros(1, np.uint8))
    dmin, tol, gate, min_inliers = 5.0, 0.05, 16.0, 10
    last = {}

    def round_trip():
        a_mean, a_cov = ma.get()
        b_mean, b_cov = mb.get()
        last["host"] = numpy_locate(a_mean, a_cov, b_mean, b_cov, dmin, tol, gate, min_inliers)

    def device():
        last["dev"] = ma.locate(ba, mb, dmin, tol, gate, min_inliers, 3, capacity=16)
    dev, d = timed(device)
    loc = last["dev"]
    if "--device-only" in sys.argv[1:]:                                 # a profiler's run: the device entry alone
        print("%d objects against %d of them moved, counts %s: obvi_map_locate, 16 reported and refined %s" % (N_MAP, n_b, loc.counts, dev))
        return
    base, b = timed(round_trip)
    counts, seed, inl, cost = last["host"]
    print("%d objects against %d of them moved, %d seeds, %d compatible, %d hypotheses with >= %d inliers: obvi_map_get x 2 + numpy %s   obvi_map_locate, 16 reported and refined %s  (x %.0f)"
          % ((N_MAP, n_b) + loc.counts + (min_inliers, base, dev, b / d)))
    print("same counts: %s   same best seed: %s   inliers %d / %d   |cost - numpy's| / cost %.1e   located T %s (made with %s)   its sigmas %s"
          % (counts == loc.counts, np.array_equal(seed, loc.seed[0]), loc.inliers[0], inl, abs(loc.cost[0] - cost) / cost, np.round(loc.transform[0], 4), T,
             np.round(np.sqrt(np.diag(loc.transform_cov[0])), 5)))
    peaks = ba.measure_peaks()
    print("obvi_ba_measure_peaks: %d compute units at %.0f MHz -- %.1f TFLOP/s of fp64 vector FMAs at 128 FLOP a clock and compute unit; fp64 MFMA issue rate %.1f TFLOP/s"
          % (peaks["compute_units"], peaks["clock_mhz"], 128e-6 * peaks["compute_units"] * peaks["clock_mhz"], peaks["mfma_f64_issue_tflops"]))
    ba.close()
    ma.close()
    mb.close()


def shared(n_sessions):
    """the map entries on handles that exchange shared objects."""
    import dist_util
    n_obj, steps = 50, 10
    ids = np.arange(n_obj, dtype=np.uint32)
    sessions = synth.make_sessions(n_sessions, P=500, L=50000, O=n_obj, seed0=1000, object_seed=77, const_poses=1, min_obj_obs=10, object_classes=("bench",))
    rng = np.random.default_rng(1)
    mean, cov = sessions[0]["objects"] - rng.normal(scale=0.02, size=(n_obj, OD)), spd(rng, n_obj * OD)
    prm = obvi_ba.SolverParams(max_num_iterations=steps, allow_non_monotonic_steps=True, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0,
                               initial_trust_region_radius=100.0, max_trust_region_radius=1e4)
    mp = obvi_ba.Map.create(mean, cov, object_block_size=OD)

    def job(prior):
        group = dist_util.RcclGroup(n_sessions)
        group.set_timeout(120.0)
        handles = []
        for m, q in enumerate(sessions):
            ba = obvi_ba.BundleAdjuster(object_block_size=OD)
            synth.upload(ba, q)
            group.attach(m, ba, np.ones(n_obj, np.uint8))
            handles.append(ba)
        dist_util.resident_map_prior(handles, mp, ids, ids, huber=1e6, uploader=0 if prior else None)
        ms = []
        for _ in range(1 + 3):                                     # (the first solve plans and allocates: not timed)
            for h, q in zip(handles, sessions):
                h.update_state(poses=q["poses"], points=q["points"], objects=q["objects"])
            t0 = time.perf_counter()
            out = dist_util.run_members([lambda h=h: h.solve(prm) for h in handles])
            dt = time.perf_counter() - t0
            for o in out:
                if isinstance(o, Exception):
                    raise o
            ms.append(1e3 * dt / max(1, out[0].num_iterations - 1))
        return group, handles, ms[1:], out[0]
    for prior in (False, True):
        group, handles, ms, s = job(prior)
        print("%d sessions x 500 frames over %d shared objects, %s: %.3f ms per joint LM step (median of 3 solves of %d steps: %s), final cost %.6e"
              % (n_sessions, n_obj, "whole-map group prior on member 0" if prior else "no map prior", float(np.median(ms)), s.num_iterations - 1, " ".join("%.3f" % x for x in ms), s.final_cost))
        if prior:
            def fold_all():
                for m in dist_util.joint_resident_map(handles, mp, ids, ids, folding=tuple(range(n_sessions))).values():
                    m.close()
            coll, _ = timed(fold_all)
            print("collective condition_on_handle, every one of %d members folds %d rows back: %s" % (n_sessions, n_obj * OD, coll))
        for h in handles:
            h.close()
        group.close()
    one = obvi_ba.BundleAdjuster(object_block_size=OD)
    synth.upload(one, synth.join_problems(sessions))
    one.set_map_group_priors_from_map(mp, [list(ids)], [list(ids)], 1e6)
    one.solve(prm)

    def fold_one():
        mp.condition_on(one, ids, ids).close()
    alone, _ = timed(fold_one)
    print("condition_on_handle on ONE handle that holds the joint problem: %s" % alone)
    one.close()
    mp.close()


if __name__ == "__main__":
    if "--shared" in sys.argv[1:]:
        shared(int(sys.argv[sys.argv.index("--shared") + 1]))
        sys.exit(0)
    locate() if "--locate" in sys.argv[1:] else move() if "--move" in sys.argv[1:] else match() if "--match" in sys.argv[1:] else merge() if "--merge" in sys.argv[1:] else extend() if "--extend" in sys.argv[1:] else update() if "--update" in sys.argv[1:] else main()
