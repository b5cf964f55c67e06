#!/usr/bin/env python
"""Group priors of one window, prepared on the host and on the device.  For od = 7 at 70, 210 and 1 400 rows, one group per call over an
objects-only problem: median and range of five calls of obvi_map_set_group_priors (host pointers: blocked Cholesky, triangular inverse, W^T W and the power steps
on the host's workers, then the upload) and of obvi_map_set_group_priors_from_map (the map already resident: gather, the same algebra and the condition estimate
on the device, one read-back).  Each entry is called once before it is timed (its first call allocates).  obvi_map_create's time is printed beside them.
usage (GPU box, repo root): python scripts/map_bench.py"""
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


if __name__ == "__main__":
    main()
