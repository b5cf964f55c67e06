#!/usr/bin/env python
"""Bit identity of the entries that write a new map, across two builds of the library: obvi_map_condition on the EDGE_CASES of tests/map_update_cases.py,
obvi_map_extend on the EXTEND_CASES of tests/map_extend_cases.py and obvi_map_merge on the CASES of tests/map_merge_cases.py, each on a default handle and on a
deterministic one.  One line per case and handle: a SHA-256 digest (first 16 hex digits) of the returned mean's and covariance's bytes, and of new_index for
the merge.  Run it once per build (OBVI_BA_LIBRARY names a build other than csrc/libobvi_ba.so) and compare the listings: a refactor leaves every line as it was.
usage (GPU box, repo root): python scripts/map_digests.py > listing.txt"""
import hashlib
import os
import sys

import numpy as np
import torch  # noqa: F401  (loaded before libobvi_ba.so, as in the tests)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "obvi-slam_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import obvi_ba  # noqa: E402
import synth  # noqa: E402
import map_extend_cases  # noqa: E402
import map_merge_cases  # noqa: E402
import map_update_cases  # noqa: E402


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def lender(od, deterministic):
    """A handle that only lends its stream and workspaces (the tests' objects_only / det_objects_only)."""
    ba = obvi_ba.BundleAdjuster(object_block_size=od, **(dict(deterministic=True) if deterministic else {}))
    ba.set_cameras(synth.K_DEFAULT[None], synth.EXT_DEFAULT[None])
    ba.set_poses(np.zeros((1, 6)), np.ones(1, np.uint8))
    ba.set_points(np.zeros((0, 3)), np.zeros(0, np.uint8))
    ba.set_objects(np.zeros((1, od)), np.zeros(1, np.uint8))
    return ba


def main():
    handles = {(od, det): lender(od, det) for od in (7, 9) for det in (False, True)}
    maps = {}

    def device_map(which, od):
        if (which, od) not in maps:
            mean, cov = map_update_cases.map_of(which, od)
            maps[which, od] = obvi_ba.Map.create(mean, cov, object_block_size=od)
        return maps[which, od]

    for det in (False, True):
        kind = "deterministic" if det else "default"
        for which, od, k in map_update_cases.EDGE_CASES:
            sel, m, P = map_update_cases.edge_case(which, od, k)
            with device_map(which, od).condition(handles[od, det], sel, m, P) as new:
                mu, Cn = new.get()
            print("condition %-5s od %d k %-3d %-13s mean %s cov %s" % (which, od, k, kind, digest(mu), digest(Cn)))
        for which, od, k_old, k_new in map_extend_cases.EXTEND_CASES:
            sel, m, P = map_extend_cases.extend_case(which, od, k_old, k_new)
            with device_map(which, od).extend(handles[od, det], sel, m, P, k_new) as new:
                mu, Cn = new.get()
            print("extend    %-5s od %d k %-3d + %-3d %-13s mean %s cov %s" % (which, od, k_old, k_new, kind, digest(mu), digest(Cn)))
        for which, od, key, noisy in map_merge_cases.CASES:
            drop, keep, offset, noise = map_merge_cases.merge_case(which, od, key, noisy)
            new, where = device_map(which, od).merge(handles[od, det], drop, keep, offset, noise)
            with new:
                mu, Cn = new.get()
            print("merge     %-5s od %d %-16s noise %d %-13s mean %s cov %s new_index %s" % (which, od, key, noisy, kind, digest(mu), digest(Cn), digest(where)))
    for mp in maps.values():
        mp.close()
    for ba in handles.values():
        ba.close()


if __name__ == "__main__":
    main()
