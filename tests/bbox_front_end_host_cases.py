"""Support of tests/test_gpu_bbox_front_end_host.py: a detection stream, and the Python restatement of the reference's whole addBoundingBoxObservations sequence
(bounding_box_front_end.h:78-323 with the pieces of feature_based_bounding_box_front_end.h and bounding_box_front_end_helpers.h the host mirror
obvi-slam_amd/host/obvi_bounding_box_front_end.h names), one statement at a time, on dicts, sets and lists.  The association round inside it is the restatement of
tests/bbox_frontend_cases.py.  The hooks are the stubs of tests/bbox_front_end_replay.cpp: a constant covariance (variance 9), the distance scorer over x, y, z,
a refinement that returns the rough estimates unchanged.  Where the reference walks a hash container and the order shows, the order is the one the mirror's header
defines: pending candidates in list order, then objects by id; views by (frame, camera); merges and additions by ascending pending index.

The stream: 30 frames, one camera (fx = fy = 500, cx = 320, cy = 240, at the robot's origin, the robot standing still), 2 classes, 5 physical objects with 14
features each at fixed pixels, 30 clutter features per frame with ids of their own."""
import numpy as np

import bbox_frontend_cases as cases

FX = FY = 500.0
CX, CY = 320.0, 240.0
PARAMS = dict(min_obs_local=3, min_obs=5, discard_after=4, validity_window=6, min_conf=0.3, min_overlap=2.0, inflation=1.0, max_merge_distance=0.6)
DIMS = {"chair": (0.5, 0.5, 1.0), "table": (1.0, 1.0, 0.8)}
# name: class, box (x0, y0, x1, y1), frames it is detected in
PHYSICAL = {"A": ("chair", (60.0, 150.0, 140.0, 250.0), set(range(0, 7)) | set(range(18, 25))),
            "B": ("chair", (260.0, 150.0, 340.0, 250.0), set(range(0, 30))),
            "C": ("table", (450.0, 100.0, 570.0, 220.0), set(range(3, 30))),
            "D": ("chair", (100.0, 330.0, 180.0, 430.0), {8, 9}),
            "E": ("table", (300.0, 320.0, 420.0, 440.0), set(range(12, 30)))}
N_FRAMES = 30


def make_stream(seed=7):
    """[(frame, [(feature id, (x, y))], [(class, x0, y0, x1, y1, confidence)])]"""
    rng = np.random.default_rng(seed)
    own = {}
    for k, (name, (_, (x0, y0, x1, y1), _)) in enumerate(sorted(PHYSICAL.items())):
        px = np.round(rng.uniform([x0 + 6, y0 + 6], [x1 - 6, y1 - 6], (14, 2)) * 4) / 4
        own[name] = [(1000 * (k + 1) + i, (float(p[0]), float(p[1]))) for i, p in enumerate(px)]
    ring = [(9001, (246.0, 200.0)), (9002, (352.0, 160.0)), (9003, (300.0, 262.0))]                   # around B: inside the wide second box of frame 10 only
    stream = []
    for frame in range(N_FRAMES):
        feats, boxes = [], []
        for name in sorted(PHYSICAL):
            cls, (x0, y0, x1, y1), frames = PHYSICAL[name]
            if frame not in frames:
                continue
            seen = sorted(rng.choice(14, size=10, replace=False))
            feats += [own[name][i] for i in seen]
            j = np.round(rng.uniform(-2, 2, 4) * 4) / 4
            boxes.append((cls, x0 + float(j[0]), y0 + float(j[1]), x1 + float(j[2]), y1 + float(j[3]), 0.9))
        if frame == 10:
            feats += ring
            boxes.append(("chair", 240.0, 130.0, 360.0, 270.0, 0.8))                                     # a second box on B
        if frame == 5:
            boxes.append(("table", 20.0, 20.0, 120.0, 120.0, 0.2))                                       # below the confidence filter
        clutter = np.round(rng.uniform([0, 0], [640, 480], (30, 2)) * 4) / 4
        feats += [(100000 + 100 * frame + i, (float(p[0]), float(p[1]))) for i, p in enumerate(clutter)]
        order = rng.permutation(len(feats))
        stream.append((frame, [feats[i] for i in order], boxes))
    return stream


def write_stream(path, stream):
    p = PARAMS
    with open(path, "w") as f:
        f.write("params %d %d %d %d %r %r %r %r\n" % (p["min_obs_local"], p["min_obs"], p["discard_after"], p["validity_window"], p["min_conf"], p["min_overlap"], p["inflation"],
                                                     p["max_merge_distance"]))
        f.write("classes %d\n" % len(DIMS))
        for name, d in sorted(DIMS.items()):
            f.write("%s %r %r %r\n" % ((name,) + d))
        f.write("frames %d\n" % len(stream))
        for frame, feats, boxes in stream:
            f.write("frame %d %d %d\n" % (frame, len(feats), len(boxes)))
            for fid, (x, y) in feats:
                f.write("%d %r %r\n" % (fid, x, y))
            for b in boxes:
                f.write("%s %r %r %r %r %r\n" % b)


NOT_INITIALIZED, ENOUGH_VIEWS_FOR_MERGE, SUFFICIENT_VIEWS_FOR_NEW = range(3)


def single_view_estimate(cls, corners):
    """helpers.h:204-264 with the camera at the world's origin: corners (min_x, max_x, min_y, max_y)"""
    if cls not in DIMS:
        return None
    dim = DIMS[cls]
    depth = dim[2] * FY / (corners[3] - corners[2])
    u, v = (corners[0] + corners[1]) / 2, (corners[2] + corners[3]) / 2
    return (depth * ((u - CX) / FX), depth * ((v - CY) / FY), depth, 0.0) + dim


def similarity(a, b):
    dist = float(np.sqrt((a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2 + (a[2] - b[2]) ** 2))
    return None if dist > PARAMS["max_merge_distance"] else -1 * dist


class Restated:
    def __init__(self):
        self.pending = []            # uninitialized_object_info_
        self.appearance = {}         # object_appearance_info_: object id -> {(frame, camera): set of feature ids}
        self.objects = {}            # the pose graph's ellipsoids: id -> (class, estimate)
        self.factors = []            # the pose graph's object observation factors: (object, frame, camera, corners, confidence)
        self.next_object_id = 0
        self.log = []                # (frame, event ...)
        self.rounds = []             # (frame, decisions)
        self.ties = []               # frames whose competing scores are NOT apart

    # ---- one round -------------------------------------------------------------------------------------------------------------------------------------------
    def add_bounding_box_observations(self, frame, feats, raw_boxes, camera=0):
        p = PARAMS
        boxes = [b for b in raw_boxes if b[5] > p["min_conf"]]                                         # filterBoundingBoxes
        observed = dict(feats)
        in_bb = [cases.features_in_box(((b[1], b[2]), (b[3], b[4])), p["inflation"], observed) for b in boxes]
        assignments = self.get_bounding_box_assignments(frame, boxes, in_bb)
        self.rounds.append((frame, assignments))
        for i, (initialized, oid) in enumerate(assignments):                                           # :137-202
            cls, x0, y0, x1, y1, conf = boxes[i]
            corners = (x0, x1, y0, y1)
            if initialized:
                self.factors.append((oid, frame, camera, corners, conf))
                self.appearance[oid][(frame, camera)] = in_bb[i]
            elif oid >= len(self.pending):
                self.pending.append(dict(cls=cls, factors=[(frame, camera, corners, conf)], feats={(frame, camera): in_bb[i]}, max_conf=conf, min_frame=frame, max_frame=frame,
                                         est=single_view_estimate(cls, corners), ready=False))
            else:
                q = self.pending[oid]
                q["factors"].append((frame, camera, corners, conf))
                q["max_frame"], q["min_frame"] = max(frame, q["max_frame"]), min(frame, q["min_frame"])
                q["max_conf"] = max(q["max_conf"], conf)
                q["feats"][(frame, camera)] = in_bb[i]
                if q["est"] is None:
                    q["est"] = single_view_estimate(cls, corners)
        self.setup_initial_estimate_generation(assignments)
        added, existing_associated, mergable = [], set(), {}
        for initialized, oid in assignments:                                                            # :220-251
            if initialized:
                existing_associated.add(oid)
                continue
            status, est = self.try_initialize(self.pending[oid])
            if status in (ENOUGH_VIEWS_FOR_MERGE, SUFFICIENT_VIEWS_FOR_NEW):
                mergable[oid] = (status, est)
        to_merge, to_add = self.search_for_object_merges(mergable, existing_associated)
        added += self.merge_pending(frame, to_merge)
        for pid, est in to_add:                                                                          # :269-295
            info = self.pending[pid]
            new_id = self.next_object_id
            self.next_object_id += 1
            self.objects[new_id] = (info["cls"], est)
            self.log.append((frame, "new_object", pid, new_id))
            self.appearance[new_id] = dict(info["feats"])
            for (f, c, corners, conf) in info["factors"]:
                self.factors.append((new_id, f, c, corners, conf))
            added.append(pid)
        for pid in sorted(added, reverse=True):
            del self.pending[pid]
        for pid in sorted(self.merge_existing_pending(frame), reverse=True):
            del self.pending[pid]
        self.cleanup(frame)

    def get_bounding_box_assignments(self, frame, boxes, in_bb):
        """bounding_box_front_end.h:941-985 with the feature-based pieces, through the restatement of tests/bbox_frontend_cases.py"""
        candidates = [(False, i, q["cls"], q["feats"]) for i, q in enumerate(self.pending)]
        candidates += [(True, oid, self.objects[oid][0], self.appearance[oid]) for oid in sorted(self.objects) if oid in self.appearance]
        n_pending = len(self.pending)
        r = cases.Round()
        r.is_match, r.score = np.zeros((len(boxes), len(candidates)), np.uint8), np.full((len(boxes), len(candidates)), np.nan)
        r.n_views_of = np.array([len(c[3]) for c in candidates], int)
        with_scores = []
        for b, box in enumerate(boxes):
            mine = []
            for c, (_, _, cls, feats) in enumerate(candidates):
                views = {k: feats[k] for k in sorted(feats)}
                per_obs = {}
                if cases.is_candidate_match(box[0], cls, in_bb[b], views, PARAMS["min_overlap"], per_obs):
                    score = cases.score_candidate_match(in_bb[b], views, per_obs)
                    mine.append((c, score))
                    r.is_match[b, c], r.score[b, c] = 1, score
            with_scores.append(mine)
        if not cases.competing_scores_are_apart(r, 100.0):
            self.ties.append(frame)
        if (r.is_match.sum(axis=0) >= 2).any():
            self.log.append((frame, "compete"))
        out = []
        for is_new, c in cases.greedily_assign(with_scores, n_pending):
            if is_new:
                self.log.append((frame, "open", c))
                out.append((False, c))
            else:
                out.append((candidates[c][0], candidates[c][1]))
        return out

    def setup_initial_estimate_generation(self, assignments):                                          # :594-672; the refinement stub returns its input
        rough = {}
        for initialized, oid in assignments:
            if not initialized and self.pending[oid]["est"] is not None:
                rough[oid] = self.pending[oid]["est"]
        for pid, q in enumerate(self.pending):
            if pid not in rough and q["ready"] and q["est"] is not None:
                rough[pid] = q["est"]
        for pid, est in rough.items():
            q = self.pending[pid]
            q["est"] = est
            q["ready"] = len(q["factors"]) >= PARAMS["min_obs_local"] and q["max_conf"] >= 0 and q["est"] is not None

    @staticmethod
    def try_initialize(q):                                                                               # :674-692
        if not q["ready"]:
            return NOT_INITIALIZED, None
        return (ENOUGH_VIEWS_FOR_MERGE if len(q["factors"]) < PARAMS["min_obs"] else SUFFICIENT_VIEWS_FOR_NEW), q["est"]

    def search_for_object_merges(self, mergable, existing_associated):                                  # :742-843, helpers.h:29-123
        merge_candidates = {}
        for pid in sorted(mergable):
            q = self.pending[pid]
            for oid in sorted(self.objects):
                if self.objects[oid][0] != q["cls"] or oid in existing_associated:
                    continue
                sources = {(f, c) for (o, f, c, _, _) in self.factors if o == oid}
                if not any((f, c) in sources for (f, c, _, _) in q["factors"]):
                    merge_candidates.setdefault(pid, []).append(oid)
        flattened = []
        for pid in sorted(mergable):
            for oid in merge_candidates.get(pid, []):
                score = similarity(mergable[pid][1], self.objects[oid][1])
                if score is not None:
                    flattened.append(((pid, oid), score))
        flattened.sort(key=lambda e: (-e[1], e[0]))
        unmerged, to_merge = set(mergable), []
        for (pid, oid), _ in flattened:
            if pid not in unmerged:
                continue
            unmerged.discard(pid)
            to_merge.append((pid, oid))
            if not unmerged:
                break
        to_add = [(pid, mergable[pid][1]) for pid in sorted(unmerged) if mergable[pid][0] == SUFFICIENT_VIEWS_FOR_NEW]
        return to_merge, to_add

    def merge_pending(self, frame, to_merge):                                                            # bounding_box_front_end.h:438-468
        merged = []
        for pid, oid in to_merge:
            info = self.pending[pid]
            for (f, c, corners, conf) in info["factors"]:
                self.factors.append((oid, f, c, corners, conf))
            for k, v in info["feats"].items():
                self.appearance[oid][k] = v
            self.log.append((frame, "merge", pid, oid))
            merged.append(pid)
        return merged

    def merge_existing_pending(self, frame):                                                             # :694-740
        mergable = {pid: (ENOUGH_VIEWS_FOR_MERGE, q["est"]) for pid, q in enumerate(self.pending) if q["ready"]}
        to_merge, _ = self.search_for_object_merges(mergable, set())
        return self.merge_pending(frame, to_merge)

    def cleanup(self, frame):                                                                            # :506-592
        keep = [q for q in self.pending if frame <= q["max_frame"] + PARAMS["discard_after"]]
        if len(keep) != len(self.pending):
            self.log.append((frame, "discard", len(self.pending) - len(keep)))
        dropped = 0
        for views in [q["feats"] for q in keep] + [self.appearance[o] for o in sorted(self.appearance)]:
            for k in [k for k in views if k[0] + PARAMS["validity_window"] < frame]:
                del views[k]
                dropped += 1
        self.pending = keep
        if dropped:
            self.log.append((frame, "views_dropped", dropped))

    # ---- the print-out of tests/bbox_front_end_replay.cpp -------------------------------------------------------------------------------------------------------
    def lines(self):
        out = []
        events = {}
        for e in self.log:
            if e[1] != "compete":
                events.setdefault(e[0], []).append(e)
        for frame, decisions in self.rounds:
            out.append(" ".join(["round", str(frame)] + [("O" if init else "P") + str(oid) for init, oid in decisions]))
            for e in events.get(frame, []):                                                              # in the order the round meets them
                out.append(" ".join(["event", str(frame)] + [str(x) for x in e[1:]]))
        for q in self.pending:
            est = list(q["est"]) if q["est"] is not None else []
            out.append(" ".join(str(x) for x in ["pending", q["cls"], len(q["factors"]), int(q["ready"]), q["min_frame"], q["max_frame"], q["max_conf"]] + est + ["views"] +
                                ["%d:%d" % (k[0], len(q["feats"][k])) for k in sorted(q["feats"])]))
        for oid in sorted(self.objects):
            cls, est = self.objects[oid]
            views = self.appearance.get(oid, {})
            out.append(" ".join(str(x) for x in ["object", oid, cls] + list(est) + ["views"] + ["%d:%d" % (k[0], len(views[k])) for k in sorted(views)]))
        out.append("factors %d" % len(self.factors))
        for (oid, f, c, corners, conf) in sorted(self.factors, key=lambda e: (e[0], e[1])):
            out.append(" ".join(str(x) for x in ["factor", oid, f, c] + list(corners) + [9, conf]))
        return out


def replay(stream):
    r = Restated()
    for frame, feats, boxes in stream:
        r.add_bounding_box_observations(frame, feats, boxes)
    return r


def same_print_out(got, want, rel=1e-9):
    """None when the two print-outs agree -- words equal, numbers within rel --, else the first difference."""
    if len(got) != len(want):
        return "%d lines against %d" % (len(got), len(want))
    for a, b in zip(got, want):
        ta, tb = a.split(), b.split()
        if len(ta) != len(tb):
            return "%r against %r" % (a, b)
        for x, y in zip(ta, tb):
            if x == y:
                continue
            try:
                fx, fy = float(x), float(y)
            except ValueError:
                return "%r against %r" % (a, b)
            if abs(fx - fy) > rel * max(1.0, abs(fy)):
                return "%r against %r" % (a, b)
    return None
