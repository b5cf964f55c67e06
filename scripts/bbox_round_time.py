"""Time of one bounding-box association round (include/obvi_bbox_frontend.h) at a stated size, on the device and on the host.

  python scripts/bbox_round_time.py [--feat 1500 --box 12 --cand 150 --views 80 --view-feat 40 --calls 200] [--store]

Device: the wall time of obvi_bbox_frontend_associate -- the host's sort of the frame's ids, the uploads, the three kernels, the read-back; the call ends in a
stream synchronise -- over --calls calls after a warm-up, every output requested.  Host: the same round through std::unordered_set look-ups as the reference does
it (scripts/bbox_host_round.cpp, which this script builds with g++ -O2 into a temporary directory), on the same seeded round written to a file.  The outputs of the two are compared before any time
is reported.  --store: the same round over views kept in an appearance store (include/obvi_bbox_store.h) instead of the host round: the views are put into the store
once, outside the timing; a timed call is obvi_bbox_store_associate plus the obvi_bbox_store_commit that gives twelve owners the view of the round.  Those twelve
owners are made before and released after the timed part of every call, so the store does not grow with the calls.  The stateless figure comes from the same run,
and the outputs of the two entries are compared for equality before a time is printed.  DESIGN.md "Bounding-box data association" records the figures."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "obvi-slam_amd", "python"))
import obvi_ba  # noqa: E402


def make_round(a):
    """Every candidate's views draw half of their ids from a window of the frame's id list (an object keeps seeing the same features) and half from ids of the past."""
    rng = np.random.default_rng(5)
    feat_id = rng.choice(1 << 40, size=a.feat, replace=False).astype(np.uint64)
    pixel = rng.uniform([0, 0], [1280, 720], (a.feat, 2))
    order = np.argsort(pixel[:, 0], kind="stable")                                   # neighbours in x: a window of this order is a vertical strip of the image
    x0, y0 = rng.uniform(0, 1000, a.box), rng.uniform(0, 500, a.box)
    corners = np.stack([x0, x0 + rng.uniform(80, 280, a.box), y0, y0 + rng.uniform(80, 220, a.box)], axis=1)
    views = np.zeros((a.cand * a.views, a.view_feat), np.uint64)
    for c in range(a.cand):
        start = int(rng.integers(0, a.feat - 4 * a.view_feat))
        window = feat_id[order[start:start + 4 * a.view_feat]]
        for v in range(a.views):
            seen = rng.choice(window, size=a.view_feat // 2, replace=False)
            past = (rng.choice(1 << 40, size=a.view_feat - len(seen), replace=False) | (1 << 41)).astype(np.uint64)
            views[c * a.views + v] = np.concatenate([seen, past])
    n_views = a.cand * a.views
    return dict(feat_id=feat_id, feat_pixel=pixel, box_corners=corners, box_label=rng.integers(0, 3, a.box).astype(np.int32), cand_label=rng.integers(0, 3, a.cand).astype(np.int32),
                view_ptr=(np.arange(a.cand + 1) * a.views).astype(np.uint64), feat_ptr=(np.arange(n_views + 1) * a.view_feat).astype(np.uint64), view_feat=views.ravel())


def store_mode(a, r, ba, prm, stateless_out, stateless_times):
    store = obvi_ba.BboxStore(ba)
    owners = store.new_owners(a.cand)
    n_views = a.cand * a.views
    store.put_views(np.repeat(owners, a.views), np.tile(np.arange(a.views), a.cand), np.zeros(n_views, np.uint64), list(r["view_feat"].reshape(n_views, a.view_feat)))
    args = [r[k] for k in ("feat_id", "feat_pixel", "box_corners", "box_label")] + [owners, r["cand_label"]]
    results = {}
    for name, want_in_box in (("every output", True), ("in_box left out, as the host mirror calls it", False)):
        times, out = [], None
        for i in range(20 + a.calls):
            scratch_owners = store.new_owners(a.box)
            t = time.perf_counter()
            out = store.associate(*args, params=prm, want_in_box=want_in_box, n_views=n_views)
            store.commit(1000 + i, 0, scratch_owners)
            times.append(time.perf_counter() - t)
            store.release(scratch_owners)
        for got, want in list(zip(out, stateless_out))[0 if want_in_box else 1:]:
            assert got.tobytes() == want.tobytes()                                   # integers and scores, byte for byte
        results[name] = np.sort(times[20:]) * 1e3
    st = store.stats()
    store.close()
    print("stateless call, the same run: median %.3f ms, min %.3f, 90%% %.3f over %d calls" %
          (float(np.median(stateless_times)), float(stateless_times[0]), float(stateless_times[int(0.9 * len(stateless_times))]), a.calls))
    for name, times in results.items():
        print("store associate + commit of %d views (%s): median %.3f ms, min %.3f, 90%% %.3f over %d calls; stateless / store %.2f" %
              (a.box, name, float(np.median(times)), float(times[0]), float(times[int(0.9 * len(times))]), a.calls, float(np.median(stateless_times)) / float(np.median(times))))
    print("store: %d bytes uploaded per round beside %d of the stateless call; %d live ids, %d dead, pool of %d" %
          (st.last_round_upload_bytes, sum(np.ascontiguousarray(r[k]).nbytes for k in r), st.live_ids, st.dead_ids, st.pool_capacity_ids))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--feat", type=int, default=1500); ap.add_argument("--box", type=int, default=12); ap.add_argument("--cand", type=int, default=150)
    ap.add_argument("--views", type=int, default=80); ap.add_argument("--view-feat", type=int, default=40); ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--store", action="store_true")
    a = ap.parse_args()
    r = make_round(a)
    scratch = tempfile.TemporaryDirectory()
    path = os.path.join(scratch.name, "bbox_round.bin")
    with open(path, "wb") as f:
        np.array([a.feat, a.box, a.cand, a.cand * a.views, len(r["view_feat"])], np.int64).tofile(f)
        for k in ("feat_id", "feat_pixel", "box_corners", "box_label", "cand_label", "view_ptr", "feat_ptr", "view_feat"):
            np.ascontiguousarray(r[k]).tofile(f)
    prm = obvi_ba.BboxFrontendParams(2.5, 2.0)
    ba = obvi_ba.BundleAdjuster(device_id=0)
    args = [r[k] for k in ("feat_id", "feat_pixel", "box_corners", "box_label", "cand_label", "view_ptr", "feat_ptr", "view_feat")]
    for _ in range(20):
        out = ba.bbox_associate(*args, params=prm)
    times = []
    for _ in range(a.calls):
        t = time.perf_counter()
        ba.bbox_associate(*args, params=prm)
        times.append(time.perf_counter() - t)
    times = np.sort(times) * 1e3
    in_box, count, overlap, match, score = out
    if a.store:
        store_mode(a, r, ba, prm, out, times)
        return
    program = os.path.join(scratch.name, "bbox_host_round")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", program, os.path.join(ROOT, "scripts", "bbox_host_round.cpp")])
    host = subprocess.run([program, path, "2.5", "2.0", str(max(5, a.calls // 10))], capture_output=True, text=True, check=True).stdout.split()
    host_ms, host_count, host_overlap, host_match, host_score = float(host[0]), int(host[1]), int(host[2]), int(host[3]), float(host[4])
    mine = (int(count.sum()), int(overlap.sum()), int(match.sum()), float(np.nansum(score)))
    assert mine[:3] == (host_count, host_overlap, host_match) and abs(mine[3] - host_score) <= 1e-9 * max(1.0, host_score), (mine, host)
    print("%d features, %d boxes, %d candidates x %d views x %d ids: %d features in boxes, overlap total %d, %d matches" %
          (a.feat, a.box, a.cand, a.views, a.view_feat, mine[0], mine[1], mine[2]))
    print("device call (sort, uploads, three kernels, read-back): median %.3f ms, min %.3f, 90%% %.3f over %d calls (python binding included)" %
          (float(np.median(times)), float(times[0]), float(times[int(0.9 * len(times))]), a.calls))
    print("host unordered_set round, -O2, one thread: %.3f ms (sets of the views built outside the timed part, as the reference keeps them)" % host_ms)


if __name__ == "__main__":
    main()
