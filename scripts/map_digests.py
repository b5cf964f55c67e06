#!/usr/bin/env python
"""Bit identity of the entries on a device-resident map, across two builds of the library: obvi_map_condition on the EDGE_CASES of tests/map_update_cases.py,
obvi_map_extend on the EXTEND_CASES of tests/map_extend_cases.py, obvi_map_merge on the CASES of tests/map_merge_cases.py, obvi_map_match on the four maps, both
block sizes and the MASKS of tests/map_match_cases.py at the gates that report about twenty and all pairs (the gates from numpy's fp64 evaluation of the formula:
the same for both builds), obvi_map_transform on the CASES of tests/map_frame_cases.py, obvi_map_join, and obvi_map_locate on the EXHAUSTIVE cases of
tests/map_locate_cases.py and on those of 64, 65, 256 and 257 compatible seeds, each on a default handle and on a deterministic one.  One line per case and
handle: a SHA-256 digest (first 16 hex digits) of the bytes of every array the entry returns (a new map: mean and covariance, and new_index for the merge),
and the counts of the two report entries.  Run it once per build (OBVI_BA_LIBRARY names a build other than csrc/libobvi_ba.so) and compare the listings: a refactor leaves every line as it was.
usage (GPU box, repo root): python scripts/map_digests.py > listing.txt"""
import functools
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
import map_frame_cases  # noqa: E402
import map_locate_cases  # noqa: E402
import map_match_cases  # noqa: E402
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


@functools.lru_cache(maxsize=None)
def match_gates(which, od, mask):
    """The gates that report about twenty and all of a map's pairs."""
    mean, cov = map_match_cases.case_map(which, od)
    return map_match_cases.gates(map_match_cases.formula(mean, cov, od, map_match_cases.mask_of(mask, od), dtype=np.float64))[-2:]


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
        for od in (7, 9):
            for which in ("small", "large", "planted", "copies"):
                mean, cov = map_match_cases.case_map(which, od)
                with obvi_ba.Map.create(mean, cov, object_block_size=od) as mp:
                    for mask in map_match_cases.MASKS:
                        row_mask = map_match_cases.mask_of(mask, od)
                        for gate in match_gates(which, od, mask):
                            a, b, st, yaw, counts = mp.match(handles[od, det], gate, row_mask=row_mask)
                            print("match     %-7s od %d mask %-6s gate %-22r %-13s a %s b %s stat %s yaw_offset %s counts %s"
                                  % (which, od, mask, gate, kind, digest(a), digest(b), digest(st), digest(yaw), counts))
        for which, od, tname, with_sigma in map_frame_cases.CASES:
            mean, cov, T, Sigma = map_frame_cases.case_inputs(which, od, tname, with_sigma)
            with obvi_ba.Map.create(mean, cov, object_block_size=od) as mp, mp.transform(handles[od, det], T, Sigma) as new:
                mu, Cn = new.get()
            print("transform %-5s od %d %-11s sigma %d %-13s mean %s cov %s" % (which, od, tname, with_sigma, kind, digest(mu), digest(Cn)))
        for od in (7, 9):
            with device_map("small", od).join(handles[od, det], device_map("large", od)) as new:
                mu, Cn = new.get()
            print("join      small + large od %d %-13s mean %s cov %s" % (od, kind, digest(mu), digest(Cn)))
        locate_cases = [(od, n_a, lab, None) for od, n_a, lab in map_locate_cases.EXHAUSTIVE] + [(7, 24, "none", n) for n in (64, 65, 256, 257)]
        for od, n_a, lab, n_compatible in locate_cases:
            c = map_locate_cases.case(od, n_a, lab)
            p = map_locate_cases.thresholds(c, n_compatible=n_compatible)
            with obvi_ba.Map.create(c.mean_a, c.cov_a, object_block_size=od) as ma, obvi_ba.Map.create(c.mean_b, c.cov_b, object_block_size=od) as mb:
                for iterations in (3, 0):
                    loc = ma.locate(handles[od, det], mb, p.dmin, p.tol, p.gate, p.min_inliers, iterations, c.label_a, c.label_b)
                    print("locate    od %d n_a %-2d labels %-7s seeds %-4s it %d %-13s seed %s transform %s transform_cov %s inliers %s cost %s partner %s counts %s"
                          % (od, n_a, lab, n_compatible or "-", iterations, kind, digest(loc.seed), digest(loc.transform), digest(loc.transform_cov), digest(loc.inliers),
                             digest(loc.cost), digest(loc.partner), loc.counts))
    for mp in maps.values():
        mp.close()
    for ba in handles.values():
        ba.close()


if __name__ == "__main__":
    main()
