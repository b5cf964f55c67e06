"""Designed incidence structures for the point pass and the Schur strip, with an extended-precision reference of one LM step.

The synthetic generator (synth.make_problem) makes one kind of track, 5 to 40 consecutive frames, so the places where the host cuts the kernels' work --
wavefront pieces of whole points that must fit an LDS image (upload.cpp), 8-frame row chunks with a 40-frame strip in three column groups, visits as 144-byte
slots in 32 KB batches, far pairs handed to k_schur_blocks (plan.cpp) -- are reached by accident or not at all.  The cases here FIX the incidence (which point is
seen from which frame by which camera) so that every cut has a point on both of its sides, and check what comes out against arithmetic that shares nothing with
either implementation: reference() takes the raw residuals and Jacobians of the oracle's debug_linearize(0) and forms the reduced system, the scalars and the
LM step in numpy long double.

Scene: a camera looking sideways (+y) moves 0.1 m per frame along +x past a slab of points 8 to 20 m away, so every point has positive depth in every frame and
any (point, frame, camera) incidence can be chosen; pixels are the ground truth plus 1 px noise (some land outside the image, which is fine), every 37th
sighting is pushed 40 px off (far past the Huber threshold); the start is a few centimetres / milliradians off the ground truth, which already puts a good part
of the residuals past the threshold.

Two Python restatements of the host's cutting rules travel with every case (`predict`): cut_pieces() (the wavefront pieces and the long points of k_point_pass)
and strip_routing() (which pairs the strip takes, which go to k_schur_blocks and in how many blocks, the visits per (chunk, column group) and their batches).
tests/test_gpu_schur_edges.py holds obvi_ba_get_problem_stats to them: a change of the strip geometry or of the image size fails there, and the cases have
to be re-aimed.

Tolerances.  TABLE holds, per case, the error of the fp64 ORACLE against the reference as measured by tests/test_schur_reference.py (entry-wise on the scale
A = sum of the absolute values of all terms of an entry for the reduced system; relative to the largest entry of the step for the step; relative for the
scalars), and n_terms, the largest number of summed terms of any entry of the case.  The bound for the device is bound() = max(8 e(oracle), n_terms 2^-53):
the factor 8 is the margin for another summation order (atomics, four wavefront streams, the K-padding of the MFMA) -- another order changes round-off by a
small factor, not by orders -- and the floor is the classical summation bound, for the case that the oracle happens to land on the reference.
"""
import functools
from collections import Counter, defaultdict

import numpy as np
from scipy.spatial.transform import Rotation as Rot

import synth

LD = np.longdouble
RADII = (100.0, 1e4)

# name: e(oracle) per quantity (tests/test_schur_reference.py prints them; it fails if they drift by more than a factor 2) and n_terms
TABLE = {
    "pack_a": dict(S=7.2e-14, b=5.4e-16, n_terms=228, step_pose=1.4e-13, step_point=6.2e-14, cost=5.1e-16, gradient_max_norm=1.6e-16, gradient_norm=4.1e-16, step_norm=6.8e-15),
    "pack_b": dict(S=1.1e-13, b=8.9e-15, n_terms=113, step_pose=9.4e-14, step_point=1.2e-14, cost=3.8e-16, gradient_max_norm=9e-17, gradient_norm=1.1e-15, step_norm=1.6e-15),
    "strip_7": dict(S=3.1e-14, b=4.4e-16, n_terms=3056, step_pose=8e-14, step_point=2.4e-14, cost=1.4e-16, gradient_max_norm=3.5e-16, gradient_norm=1e-15, step_norm=3.3e-15),
    "strip_1": dict(S=7.3e-14, b=7.7e-16, n_terms=220, step_pose=2.1e-13, step_point=1e-14, cost=9.8e-16, gradient_max_norm=3.5e-17, gradient_norm=3.9e-16, step_norm=1e-14),
}

# geometry of the cuts (ba_device.h); the cases are aimed at these numbers
ROWS, STRIP, BACK, GROUP_TILES, TILE = 8, 40, 32, 5, 16
BATCH_SLOTS, BATCH_VISITS, PAIRS_PER_ITEM = 32768 // 144, 128, 256
IMAGE_DOUBLES = 1264


def bound(case, what, table=None):
    """(table: another module's case table; an entry "second_<what>" there is a second measured error of the reference's inputs, tests/object_cases.py)"""
    t = (TABLE if table is None else table)[case]
    return max(8.0 * max(t[what], t.get("second_" + what, 0.0)), t["n_terms"] * 2.0 ** -53)


# ------------------------------------------------------------------------------------------
# the host's two cutting rules, restated
# ------------------------------------------------------------------------------------------
def cut_pieces(counts):
    """Point pass: whole points per piece, at most 64 sightings, the ids of a piece less than 64 apart, 18 n + 4 span <= 1264 doubles of LDS image (span: the
    point ids from the first to the last of the piece, unobserved ones included); a track over 64 sightings is a long point and closes the piece before it.
    counts: sightings per point id (all uploaded ones: masks and constness play no part).  Returns ([(first sighting, count)], [long point ids])."""
    first_obs = np.concatenate([[0], np.cumsum(counts)])
    pieces, longs, cur = [], [], None          # cur = [first id, first sighting, count]
    for l, k in enumerate(counts):
        if k == 0:
            continue
        fits = cur is not None and k <= 64 and cur[2] + k <= 64 and l - cur[0] < 64 and 18 * (cur[2] + k) + 4 * (l - cur[0] + 1) <= IMAGE_DOUBLES
        if cur is not None and not fits:
            pieces.append((cur[1], cur[2])); cur = None
        if k > 64:
            longs.append(l)
        elif cur is None:
            cur = [l, int(first_obs[l]), int(k)]
        else:
            cur[2] += int(k)
    if cur is not None:
        pieces.append((cur[1], cur[2]))
    return pieces, longs


def _frames_of_tile(t):
    return range((TILE * t) // 6, (TILE * t + TILE - 1) // 6 + 1)


def _visit_groups(offs):
    """offs: strip frame offsets (0..39) of a point in one chunk -> {group: (column tiles in use, row tiles in use)}; a visit has a tile (tc, tr) where the point
    has a frame in column tile tc and in row tile 12 + tr, lower triangle only (tc <= 12 + tr)."""
    ntiles = STRIP * 6 // TILE
    row0 = BACK * 6 // TILE
    touched = [any(f in offs for f in _frames_of_tile(t)) for t in range(ntiles)]
    out = {}
    for g in range(ntiles // GROUP_TILES):
        cols, rows = set(), set()
        for tc in range(GROUP_TILES * g, GROUP_TILES * (g + 1)):
            for tr in range(3):
                if touched[tc] and touched[row0 + tr] and tc <= row0 + tr:
                    cols.add(tc); rows.add(tr)
        if cols:
            out[g] = (cols, rows)
    return out


def _visit_slots(cols, rows, twin):
    """144-byte slots of a visit: the frames of its row tiles, the tail, the frames of its column tiles (one range if the two touch or overlap); twice for a twin."""
    row0 = BACK * 6 // TILE
    b0, b1 = min(_frames_of_tile(min(cols))), min(max(_frames_of_tile(max(cols))), STRIP - 1)
    a0, a1 = min(_frames_of_tile(row0 + min(rows))), min(max(_frames_of_tile(row0 + max(rows))), STRIP - 1)
    if b0 <= a1 + 1 and a0 <= b1 + 1:
        span = max(a1, b1) - min(a0, b0) + 1
        return span + 1 + (span if twin else 0), True
    one = (a1 - a0 + 1) + 1 + (b1 - b0 + 1)
    return (2 * one if twin else one), False


def strip_routing(prob, mask=None):
    """Schur strip: frames are the variable poses in trajectory order; a pair of sightings (fp >= fq) of a point is in the strip iff no frame of the point holds
    more than two sightings and fq >= 8 (fp // 8) - 32; every other pair goes to k_schur_blocks, in the 6x6 block of its two poses (a pair of two different
    sightings from ONE pose twice, in both orders).  A point that the strip takes is visited once per chunk it has a frame in, in every column group where it
    has a tile."""
    n = len(prob["rp_pose"])
    act = np.ones(n, bool) if mask is None else np.asarray(mask, bool)
    pose, point = prob["rp_pose"].astype(np.int64), prob["rp_point"].astype(np.int64)
    live = act & ~((prob["pose_const"][pose] != 0) & (prob["point_const"][point] != 0))
    var_pose = (prob["pose_const"] == 0) & (np.bincount(pose[live], minlength=len(prob["poses"])) > 0)
    frame = np.where(var_pose, np.cumsum(var_pose) - 1, -1)
    n_frames = int(var_pose.sum())
    blocks, lists, layouts = Counter(), defaultdict(list), Counter()
    n_strip = 0
    for l in range(len(prob["points"])):
        if prob["point_const"][l]:
            continue
        F = sorted(int(frame[p]) for p in pose[(point == l) & act] if frame[p] >= 0)
        if not F:
            continue
        mult = Counter(F)
        windowed = max(mult.values()) <= 2
        twin = max(mult.values()) == 2
        for i, fp in enumerate(F):
            for j in range(i + 1):
                fq = F[j]
                if windowed and fq >= ROWS * (fp // ROWS) - BACK:
                    n_strip += 1
                    continue
                blocks[(fp, fq)] += 2 if (i != j and fp == fq) else 1
        if windowed:
            for c in sorted({f // ROWS for f in F}):
                base = ROWS * c - BACK
                offs = {f - base for f in F if base <= f < ROWS * (c + 1)}
                for g, (cols, rows) in _visit_groups(offs).items():
                    slots, merged = _visit_slots(cols, rows, twin)
                    lists[(c, g)].append((l, slots))
                    layouts[("twin " if twin else "") + ("merged" if merged else "split")] += 1
    batches = {}
    for key, visits in lists.items():          # (visits of a list in point order: one workgroup on a deterministic handle)
        nb, used, cnt = 1, 0, 0
        for _, slots in visits:
            if cnt == BATCH_VISITS or used + slots > BATCH_SLOTS:
                nb, used, cnt = nb + 1, 0, 0
            used += slots; cnt += 1
        batches[key] = nb
    return dict(n_frames=n_frames, frame_of_pose=frame, block_pairs=dict(blocks), schur_pairs_blocks=sum(blocks.values()), schur_pairs_strip=n_strip,
                schur_blocks_det=len(blocks), schur_items_default=sum(-(-v // PAIRS_PER_ITEM) for v in blocks.values()),
                list_visits={k: len(v) for k, v in lists.items()}, list_batches=batches, schur_batches_det=sum(batches.values()), layouts=dict(layouts))


# ------------------------------------------------------------------------------------------
# the case builder
# ------------------------------------------------------------------------------------------
class _Builder:
    def __init__(self, name, P, stereo, seed, const_poses=None):
        self.name, self.P, self.stereo = name, P, stereo
        self.rng = np.random.Generator(np.random.MT19937(seed))
        self.pose_const = np.zeros(P, np.uint8)
        self.pose_const[[0, 37, 38, 39, P - 1] if const_poses is None else list(const_poses)] = 1
        self.pose_of_frame = np.flatnonzero(self.pose_const == 0)       # every variable pose gets a sighting (checked in finish)
        self.n_frames = len(self.pose_of_frame)
        self.sightings = []          # (point, pose, cam, masked from the start, masked after the solve)
        self.n_points = 0
        self.point_const = []
        self.groups = defaultdict(list)

    def point(self, group, sightings, const=False):
        """sightings: (pose index, cam[, "m0" | "m1"]): m0 = masked before the first plan (and after), m1 = masked after the solve"""
        l = self.n_points
        for s in sightings:
            tag = s[2] if len(s) > 2 else ""
            assert 0 <= s[0] < self.P and s[1] in ((0, 1) if self.stereo else (0,))
            self.sightings.append((l, int(s[0]), int(s[1]), tag == "m0", tag in ("m0", "m1")))
        self.n_points += 1
        self.point_const.append(1 if const else 0)
        self.groups[group].append(l)
        return l

    def gap(self, n):
        """n point ids that nobody observes"""
        for _ in range(n):
            self.point("unobserved", [])

    def frames(self, group, frames, cams=(0,), const=False):
        """a point seen from the given FRAMES (ranks among the variable poses) by each of `cams`"""
        return self.point(group, [(self.pose_of_frame[f], c) for f in frames for c in cams], const)

    def track(self, group, pose0, n, cams=(0,)):
        """n consecutive POSES from pose0 on (constant ones included)"""
        return self.point(group, [(p, c) for p in range(pose0, pose0 + n) for c in cams])

    def fillers(self, n, skip_frames=()):
        """ordinary short tracks (4 to 8 consecutive frames) so that every pose is held by several points"""
        ok = [f for f in range(self.n_frames) if f not in skip_frames]
        for j in range(n):
            i0 = (j * 5) % max(1, len(ok) - 8)
            self.frames("filler", ok[i0:i0 + 4 + j % 5])
        seen = {s[1] for s in self.sightings}
        for i, f in enumerate(ok):                                  # whatever frame is still unseen: the last of a 4-track
            if self.pose_of_frame[f] not in seen:
                self.frames("filler", ok[max(0, i - 3):i + 1])
                seen.add(self.pose_of_frame[f])

    def finish(self):
        P, L = self.P, self.n_points
        rng = self.rng
        i = np.arange(P)
        pos = np.stack([0.1 * i, 0.02 * np.sin(0.7 * i), 0.01 * np.cos(0.9 * i)], axis=1)
        R = Rot.from_euler("ZYX", np.stack([np.pi / 2 + 0.03 * np.sin(0.5 * i), 0.02 * np.sin(0.3 * i + 0.3), 0.015 * np.cos(0.4 * i)], axis=1))
        gt_poses = np.concatenate([pos, R.as_rotvec()], axis=1)
        gt_points = np.stack([rng.uniform(-3.0, 0.1 * P + 3.0, L), rng.uniform(8.0, 20.0, L), rng.uniform(-2.0, 2.0, L)], axis=1)
        s = sorted(self.sightings, key=lambda x: (x[0], x[1], x[2]))          # by (point, pose, camera), as synth does
        rp_point = np.array([x[0] for x in s], np.uint32); rp_pose = np.array([x[1] for x in s], np.uint32); rp_cam = np.array([x[2] for x in s], np.uint16)
        mask0 = np.array([0 if x[3] else 1 for x in s], np.uint8); mask1 = np.array([0 if x[4] else 1 for x in s], np.uint8)
        ext2 = synth.EXT_DEFAULT.copy(); ext2[5] = -0.12                       # synth's stereo camera: 0.12 m to the right
        K = np.stack([synth.K_DEFAULT] * (2 if self.stereo else 1)); ext = np.stack([synth.EXT_DEFAULT, ext2][:2 if self.stereo else 1])
        pix = np.zeros((len(s), 2))
        for c in range(len(K)):
            m = rp_cam == c
            px, z = synth.project_points(gt_poses[rp_pose[m]], gt_points[rp_point[m]], K[c], ext[c])
            assert (z > 5.0).all()
            pix[m] = px
        pix += rng.normal(size=pix.shape)
        is_out = np.arange(len(s)) % 37 == 5
        pix[is_out] += np.array([40.0, -40.0])
        poses = gt_poses + rng.normal(size=gt_poses.shape) * np.array([0.02, 0.02, 0.02, 0.004, 0.004, 0.004])
        points = gt_points + rng.normal(size=gt_points.shape) * 0.05
        prob = dict(K=K, ext=ext, poses=poses, gt_poses=gt_poses, pose_const=self.pose_const.copy(), points=points, gt_points=gt_points,
                    point_const=np.array(self.point_const, np.uint8), rp_pose=rp_pose, rp_point=rp_point, rp_cam=rp_cam, rp_pixel=pix,
                    rp_sigma=synth.RESIDUAL_PARAMS["reproj_sigma"], rp_huber=synth.RESIDUAL_PARAMS["reproj_huber"], rp_is_outlier=is_out,
                    objects=np.zeros((0, 7)), gt_objects=np.zeros((0, 7)), object_const=np.zeros(0, np.uint8),
                    bb_obj=np.zeros(0, np.uint32), bb_pose=np.zeros(0, np.uint32), bb_cam=np.zeros(0, np.uint16), bb_corners=np.zeros((0, 4)), bb_cov=np.zeros((0, 16)),
                    bb_huber=0.5, bb_invalid=1000.0, sp_obj=np.zeros(0, np.uint32), sp_mean=np.zeros((0, 3)), sp_cov=np.zeros((0, 9)), sp_huber=10.0, obj_class=[])
        # every depth is positive at the START too, for every camera (tests/test_schur_reference.py checks it again from the residuals' side)
        for c in range(len(K)):
            m = rp_cam == c
            assert (synth.project_points(poses[rp_pose[m]], points[rp_point[m]], K[c], ext[c])[1] > 5.0).all()
        assert P <= 100 and L <= 700
        counts = np.bincount(rp_point, minlength=L)
        pieces, longs = cut_pieces(counts)
        predict = dict(pieces=pieces, long_points=longs, point_pieces=len(pieces), counts=counts)
        predict.update(strip_routing(prob, mask0))
        predict["after_mask"] = strip_routing(prob, mask1)
        assert predict["n_frames"] == self.n_frames == predict["after_mask"]["n_frames"], "a variable pose without a sighting"
        return dict(name=self.name, prob=prob, mask0=mask0, mask1=mask1, groups=dict(self.groups), predict=predict, pose_of_frame=self.pose_of_frame)


def _piece_of(case, l):
    """index of the piece that holds point l (None: a long point or an unobserved one)"""
    ptr = np.concatenate([[0], np.cumsum(case["predict"]["counts"])])
    for i, (a, n) in enumerate(case["predict"]["pieces"]):
        if a <= ptr[l] < a + n and ptr[l + 1] > ptr[l]:
            return i
    return None


def _points_of_piece(case, i):
    a, n = case["predict"]["pieces"][i]
    return sorted(set(int(x) for x in case["prob"]["rp_point"][a:a + n]))


def _mask_group(b):
    """pattern 7, inside one piece: a constant point, a variable point whose poses are all constant, a point with every sighting masked (from the start / after
    the solve), a point with some sightings masked (from the start / after the solve), an ordinary point"""
    P = b.P
    b.point("const_point", [(10, 0), (11, 0), (12, 0)], const=True)
    b.point("const_poses_only", [(0, 0), (37, 0), (38, 0), (39, 0), (P - 1, 0)])
    b.point("all_masked", [(20, 0, "m0"), (21, 0, "m0"), (22, 0, "m0"), (23, 0, "m0")])
    b.point("some_masked", [(20, 0), (21, 0, "m0"), (22, 0), (23, 0, "m0"), (24, 0), (60, 0)])
    b.point("all_masked_later", [(30, 0, "m1"), (31, 0, "m1"), (32, 0, "m1")])
    b.point("some_masked_later", [(30, 0), (31, 0, "m1"), (32, 0), (33, 0), (34, 0, "m1"), (70, 0, "m1")])
    b.point("mask_neighbour", [(20, 0), (21, 0), (22, 0)])


def _check_mask_group(case):
    g = case["groups"]
    ids = [g[k][0] for k in ("const_point", "const_poses_only", "all_masked", "some_masked", "all_masked_later", "some_masked_later", "mask_neighbour")]
    assert len({_piece_of(case, l) for l in ids}) == 1 and _piece_of(case, ids[0]) is not None, "pattern 7 must lie inside one piece"


@functools.lru_cache(maxsize=None)
def pack_a():
    """Point-pass packing, stereo: tracks of 63 / 64 / 65 / 128 sightings side by side, a long track between two short ones, a 65-track as the first and as the
    last id, forty 2-tracks (the image rule cuts after 31 points), seventy 1-tracks (after 57), the mask group."""
    b = _Builder("pack_a", 100, True, 7101)
    b.track("first_65", 1, 65)
    b.track("short", 10, 3)
    b.track("t63", 20, 63); b.track("t64", 20, 64); b.track("t65", 20, 65); b.track("t128", 30, 64, cams=(0, 1))
    b.track("short", 50, 2); b.track("between_65", 2, 65); b.track("short", 52, 2)
    b.track("sep64", 3, 64)                                     # a wavefront by itself: the pieces around it start and end flush
    for j in range(40):
        b.frames("twos", [2 * j, 2 * j + 1])
    b.track("sep64", 30, 64)
    for j in range(70):
        b.frames("ones", [(j * 4) % b.n_frames])
    b.track("sep64", 33, 64)
    _mask_group(b)
    b.fillers(60)
    b.track("last_65", 30, 65)
    case = b.finish()
    pr, g = case["predict"], case["groups"]
    longs = g["first_65"] + g["t65"] + g["t128"] + g["between_65"] + g["last_65"]
    assert pr["long_points"] == sorted(longs) and longs[0] == 0 and longs[-1] == len(case["prob"]["points"]) - 1
    for name in ("t63", "t64"):                                # each a piece by itself
        assert _points_of_piece(case, _piece_of(case, g[name][0])) == g[name]
    assert _points_of_piece(case, _piece_of(case, g["twos"][0])) == g["twos"][:31], "the image rule cuts the 2-tracks after 31 points"
    assert _points_of_piece(case, _piece_of(case, g["ones"][0])) == g["ones"][:57], "the image rule cuts the 1-tracks after 57 points"
    assert _points_of_piece(case, _piece_of(case, g["short"][1])) == [g["short"][1]] and _points_of_piece(case, _piece_of(case, g["short"][2])) == [g["short"][2]]
    _check_mask_group(case)
    return case


@functools.lru_cache(maxsize=None)
def pack_b():
    """Point-pass packing, one camera (the strip kernel without twins): the span rule from both sides, the mask group, a final piece of a single observation."""
    b = _Builder("pack_b", 94, False, 7102)
    b.track("first_65", 1, 65)
    b.fillers(50)
    b.gap(70)
    # the span rule: ids of a piece are less than 64 apart.  62 unobserved ids between two points: one piece; 63 and 64: the rule cuts
    b.frames("span62_a", [5, 6, 7, 50]); b.gap(62); b.frames("span62_b", [8, 9, 10, 60])
    b.gap(70)
    b.frames("span63_a", [15, 16, 17, 66]); b.gap(63); b.frames("span63_b", [18, 19, 20, 70])
    b.gap(70)
    b.frames("span64_a", [25, 26, 27, 74]); b.gap(64); b.frames("span64_b", [28, 29, 30, 80])
    b.gap(70)
    _mask_group(b)
    b.track("t63", 25, 63)
    for j in range(12):
        b.frames("ones", [7 * j + 3])
    for j in range(12):
        b.frames("twos", [7 * j + 1, 7 * j + 2])
    b.track("t64", 5, 64)
    b.frames("last_single", [44])
    case = b.finish()
    pr, g = case["predict"], case["groups"]
    assert pr["long_points"] == g["first_65"] == [0]
    assert _piece_of(case, g["span62_a"][0]) == _piece_of(case, g["span62_b"][0])
    assert _piece_of(case, g["span63_a"][0]) + 1 == _piece_of(case, g["span63_b"][0])
    assert _piece_of(case, g["span64_a"][0]) + 1 == _piece_of(case, g["span64_b"][0])
    assert pr["pieces"][-1][1] == 1 and _points_of_piece(case, len(pr["pieces"]) - 1) == g["last_single"], "a final piece of a single observation"
    _check_mask_group(case)
    return case


def _exact_lists(b, targets, sizes, avoid):
    """pattern 16: add two-sighting points until, for every n in `targets`, some (chunk, column group 0 or 1) work list holds exactly n visits.  A point on
    (fq, fp) with fq inside a group's frames of the strip of fp's chunk adds one visit to that list and otherwise only to lists of group 2."""
    free = sorted(((sizes.get((c, g), 0), c, g) for c in range(4, (b.n_frames - 1) // ROWS + 1) for g in (0, 1)), key=lambda x: (x[0], x[1], x[2]))
    chosen = {}
    for n in sorted(targets):
        k = next(i for i, (have, c, g) in enumerate(free) if have <= n)
        have, c, g = free.pop(k)
        chosen[n] = (c, g)
        rows = [f for f in range(ROWS * c, min(ROWS * (c + 1), b.n_frames)) if f != avoid]
        cols = [f for f in range(ROWS * c - BACK + (1 if g == 0 else 14), ROWS * c - BACK + (12 if g == 0 else 25)) if f != avoid]   # strictly inside the group: offsets 1..11 / 14..24
        for j in range(n - have):
            b.frames("list_fill", [cols[(3 * j) % len(cols)], rows[j % len(rows)]])
    return chosen


def _strip_case(name, P, seed, variant):
    b = _Builder(name, P, True, seed)
    nF = b.n_frames
    last = (nF - 1) // ROWS                                        # the last, incomplete chunk
    reserved = 70                                                   # pattern 19: a frame that only points outside the strip see
    # 8. the strip boundary fq = 8 (fp // 8) - 32 from both sides, at fp % 8 = 0 and 7
    for fp in ((40, 47) if variant == 0 else (48, 55)):
        fq = ROWS * (fp // ROWS) - BACK
        b.frames("edge_in", [fq, fp]); b.frames("edge_out", [fq - 1, fp])
    # 9. partly strip, partly blocks
    b.frames("partly", [0, 20, 45])
    b.frames("run41", range(10, 51) if variant == 0 else range(12, 53))
    b.frames("run48", range(20, 68) if variant == 0 else range(14, 62))
    # 10. only in chunk 0 (negative strip frames)
    b.frames("chunk0", [0, 3, 7]); b.frames("chunk0", [1, 2]); b.frames("chunk0", [5])
    # 11. ending in the last chunk
    b.frames("last_chunk", range(ROWS * last - 8, nF)); b.frames("last_chunk", [ROWS * last - 3, nF - 1]); b.frames("last_chunk", [nF - 1, nF - 1 - BACK - (nF - 1) % ROWS])
    # 12. across every constant pose
    b.track("across_const", 0, 4); b.track("across_const", 35, 8); b.track("across_const", P - 4, 4); b.point("across_const", [(36, 0), (38, 0), (40, 0), (P - 1, 0)])
    # 13. column frames in one group only, row frames in the chunk: the split layout; frames that straddle 16-column tiles
    c = 6
    base = ROWS * c - BACK
    b.frames("split_g0", [base + 2, base + 4, ROWS * c + 2, ROWS * c + 5])
    b.frames("split_g1", [base + 17, base + 22, ROWS * c + 2, ROWS * c + 5])
    b.frames("straddle", [2, 5, 8]); b.frames("straddle", [base + 2, base + 5, base + 8, ROWS * c + 4])
    # 14. twins, with a point that is no twin in the same work lists
    c = 7
    base = ROWS * c - BACK
    b.frames("twin_corners", [base, ROWS * c + 7], cams=(0, 1))
    b.point("twin_same_camera", [(b.pose_of_frame[ROWS * c + 4], 0), (b.pose_of_frame[ROWS * c + 4], 0), (b.pose_of_frame[ROWS * c + 6], 0)])
    b.point("twin_split", [(b.pose_of_frame[base + 2], 0), (b.pose_of_frame[base + 2], 1), (b.pose_of_frame[ROWS * c + 2], 0)])
    b.frames("twin_neighbour", [base + 2, ROWS * c + 2]); b.frames("twin_neighbour", [base, ROWS * c + 7])
    # 15. three sightings from one frame: the whole point goes to k_schur_blocks, its same-pose pairs in both orders
    q = b.pose_of_frame
    b.point("triple", [(q[44], 0), (q[44], 1), (q[44], 0), (q[45], 0), (q[47], 1)])
    # 19. a frame whose diagonal block only k_schur_blocks feeds: nothing but points with a triple sighting see it
    b.point("blocks_only_diag", [(q[20], 0), (q[20], 1), (q[20], 0), (q[reserved], 0)])
    b.point("blocks_only_diag", [(q[21], 0), (q[21], 1), (q[21], 0), (q[reserved], 1), (q[75], 0)])
    b.point("blocks_only_diag", [(q[reserved], 0), (q[reserved], 1), (q[reserved], 0), (q[22], 0)])
    if variant == 0:
        # 17. wide visits (a twin in the split layout over all of group 0 and all row tiles: 46 slots) -- 16 of them make one work list four batches long
        c = 9
        base = ROWS * c - BACK
        for _ in range(16):
            b.frames("wide", [base, base + 13, ROWS * c, ROWS * c + 7], cams=(0, 1))
        # 18. loop closures between two far frames: blocks with exactly 1, 16, 17, 64, 65 and 300 pairs (a stereo point on both frames gives four)
        for k, (n, fa) in enumerate(((1, 1), (16, 2), (17, 3), (64, 4), (65, 5), (300, 6))):
            fb = nF - 1 - k
            for _ in range(n // 4):
                b.frames("far%d" % n, [fa, fb], cams=(0, 1))
            for _ in range(n % 4):
                b.frames("far%d" % n, [fa, fb])
    b.fillers(70, skip_frames=(reserved,))

    chosen = _exact_lists(b, range(1, 10), _probe_finish(b)["predict"]["list_visits"], avoid=reserved) if variant == 1 else {}
    case = b.finish()
    pr, g, fr = case["predict"], case["groups"], case["predict"]["frame_of_pose"]
    prob = case["prob"]
    seen_by = defaultdict(set)
    for l, p in zip(prob["rp_point"], prob["rp_pose"]):
        seen_by[int(fr[p])].add(int(l))
    assert seen_by[reserved] == set(g["blocks_only_diag"]) and pr["block_pairs"][(reserved, reserved)] == 1 + 1 + 3 + 6
    for n, (c, gg) in chosen.items():
        assert pr["list_visits"][(c, gg)] == n, "a work list with exactly %d visits" % n
    if variant == 1:
        assert set(range(1, 10)) <= set(pr["list_visits"].values())
    lay = pr["layouts"]
    assert all(lay.get(k, 0) > 0 for k in ("merged", "split", "twin merged", "twin split")), lay
    tq = int(fr[q[44]])
    assert pr["block_pairs"][(tq, tq)] == 3 + 6                     # three same-sighting pairs, three pairs of different sightings in both orders
    if variant == 0:
        c = 9
        assert pr["list_batches"][(c, 0)] >= 4, "a work list of at least four batches"
        for k, n in enumerate((1, 16, 17, 64, 65, 300)):
            assert pr["block_pairs"][(nF - 1 - k, 1 + k)] == n
        assert pr["schur_items_default"] == pr["schur_blocks_det"] + 1    # the 300-pair block is two work items
    ein = [tuple(sorted(int(fr[p]) for p in prob["rp_pose"][prob["rp_point"] == l])) for l in g["edge_in"]]
    eout = [tuple(sorted(int(fr[p]) for p in prob["rp_pose"][prob["rp_point"] == l])) for l in g["edge_out"]]
    assert all((fp, fq) not in pr["block_pairs"] for fq, fp in ein) and all(pr["block_pairs"][(fp, fq)] >= 1 for fq, fp in eout)
    return case


def _probe_finish(b):
    """the case as it stands, without consuming the builder's random stream (only the incidence matters to the routing)"""
    state = b.rng.bit_generator.state
    c = b.finish()
    b.rng.bit_generator.state = state
    return c


@functools.lru_cache(maxsize=None)
def strip_7():
    """Schur strip, 95 variable poses (8 k + 7): boundary pairs, twins, the batch list, the far blocks of 1 .. 300 pairs."""
    return _strip_case("strip_7", 100, 7103, 0)


@functools.lru_cache(maxsize=None)
def strip_1():
    """Schur strip, 89 variable poses (8 k + 1): boundary pairs, twins, work lists of exactly 1 .. 9 visits."""
    return _strip_case("strip_1", 94, 7104, 1)


CASES = {"pack_a": pack_a, "pack_b": pack_b, "strip_7": strip_7, "strip_1": strip_1}
PACKING_CASES = ("pack_a", "pack_b")


# ------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------
def _inv3(H):
    """closed-form inverse of symmetric 3x3 matrices [n,3,3] (adjugate over determinant), and the pivots of their elimination"""
    a, b, c, d, e, f = H[:, 0, 0], H[:, 1, 0], H[:, 1, 1], H[:, 2, 0], H[:, 2, 1], H[:, 2, 2]
    A = np.empty_like(H)
    A[:, 0, 0] = c * f - e * e; A[:, 1, 0] = A[:, 0, 1] = d * e - b * f; A[:, 2, 0] = A[:, 0, 2] = b * e - c * d
    A[:, 1, 1] = a * f - d * d; A[:, 2, 1] = A[:, 1, 2] = b * d - a * e; A[:, 2, 2] = a * c - b * b
    det = a * A[:, 0, 0] + b * A[:, 1, 0] + d * A[:, 2, 0]
    p1 = a; p2 = c - b * b / a; p3 = det / A[:, 2, 2]
    return A / det[:, None, None], np.stack([p1, p2, p3], axis=1)


def _lm_lambda(colsq, radius):
    """the documented LM rule (ba_kernels.hip, lm_lambda): Jacobi scale s = 1 / (1 + sqrt(colsq)), damping clamp(colsq s^2, 1e-6, 1e32) / radius / s^2"""
    s = 1 / (1 + np.sqrt(colsq))
    return np.clip(colsq * s * s, LD(1e-6), LD(1e32)) / LD(radius) / (s * s)


def reference(prob, oracle_handle, radius, mask=None, want_step=True, side=None, lin0=None):
    """One LM step at the handle's current estimate, in numpy long double, from the oracle's raw r, Jp, Jl of every sighting, the Huber weight and the LM rule
    alone.  Returns a dict: S, b (variable poses in upload order), their scales A_S, A_b, n_terms, cost, gradient_max_norm, gradient_norm, step_pose [P,6],
    step_point [L,3], step_norm, point_var, pivots_ok.  want_step=False: the reduced system and the scalars of the linearisation only (at a large radius the reduced
    system is too ill-conditioned for a step that is better than fp64: the refinement stalls at cond(S) 2^-64, and the step is checked at the solve's own radius).
    side (tests/object_cases.py, SideTerms): the factors of the other families -- the reduced system then runs over (variable poses, variable objects), both in
    upload order, the damping of a row comes from the whole diagonal of J^T J, and object_var, step_object are returned too.  lin0: (r, Jp, Jl) of the sightings
    from somewhere else than the oracle handle."""
    assert np.finfo(LD).eps <= 2.0 ** -63, "numpy long double is no wider than double here: the reference needs the x87 format or better"
    r64, Jp64, Jl64 = oracle_handle.debug_linearize(0) if lin0 is None else lin0
    r, Jp, Jl = r64.astype(LD), Jp64.astype(LD), Jl64.astype(LD)
    n = len(r)
    P, L = len(prob["poses"]), len(prob["points"])
    pose, point = prob["rp_pose"].astype(np.int64), prob["rp_point"].astype(np.int64)
    act = np.ones(n, bool) if mask is None else np.asarray(mask, bool)
    cp, cl = prob["pose_const"][pose] != 0, prob["point_const"][point] != 0
    s = (r * r).sum(axis=1)
    h = LD(prob["rp_huber"])
    over = s > h * h
    rho = np.where(over, 2 * h * np.sqrt(s) - h * h, s)
    w = np.where(over, h / np.sqrt(np.where(over, s, 1)), LD(1))
    cost = (rho[act]).sum() / 2
    both = bool(over[act].any()) and bool((~over[act]).any())
    live = act & ~(cp & cl)
    var_pose = (prob["pose_const"] == 0) & (np.bincount(pose[live], minlength=P) > 0)
    if side is not None:
        var_pose |= (prob["pose_const"] == 0) & side.pose_used
    var_point = (prob["point_const"] == 0) & (np.bincount(point[live], minlength=L) > 0)
    frame = np.where(var_pose, np.cumsum(var_pose) - 1, -1)
    nF = int(var_pose.sum())
    ex = side.assemble(var_pose, frame) if side is not None else None
    # pose side: every active sighting of a variable pose (a constant point's too)
    Hpp, App, gp, Agp = np.zeros((nF, 6, 6), LD), np.zeros((nF, 6, 6), LD), np.zeros((nF, 6), LD), np.zeros((nF, 6), LD)
    mp = act & var_pose[pose]
    np.add.at(Hpp, frame[pose[mp]], np.einsum("n,nka,nkb->nab", w[mp], Jp[mp], Jp[mp]))
    np.add.at(App, frame[pose[mp]], np.einsum("n,nka,nkb->nab", w[mp], np.abs(Jp[mp]), np.abs(Jp[mp])))
    np.add.at(gp, frame[pose[mp]], np.einsum("n,nka,nk->na", w[mp], Jp[mp], r[mp]))
    np.add.at(Agp, frame[pose[mp]], np.einsum("n,nka,nk->na", w[mp], np.abs(Jp[mp]), np.abs(r[mp])))
    nobs_pose = np.bincount(frame[pose[mp]], minlength=nF)
    # point side: every active sighting of a variable point (a constant pose's too)
    Hll, gl, Agl = np.zeros((L, 3, 3), LD), np.zeros((L, 3), LD), np.zeros((L, 3), LD)
    ml = act & var_point[point]
    np.add.at(Hll, point[ml], np.einsum("n,nka,nkb->nab", w[ml], Jl[ml], Jl[ml]))
    np.add.at(gl, point[ml], np.einsum("n,nka,nk->na", w[ml], Jl[ml], r[ml]))
    np.add.at(Agl, point[ml], np.einsum("n,nka,nk->na", w[ml], np.abs(Jl[ml]), np.abs(r[ml])))
    ix = np.arange(3)
    lam_l = np.zeros((L, 3), LD)
    lam_l[var_point] = _lm_lambda(Hll[var_point][:, ix, ix], radius)
    Hd = Hll.copy()
    Hd[:, ix, ix] += lam_l
    Hd[~var_point] = np.eye(3, dtype=LD)
    Hinv, piv = _inv3(Hd)
    pivots_ok = bool((piv[var_point] > 0).all())
    i6 = np.arange(6)
    lam_p = _lm_lambda(Hpp[:, i6, i6] if ex is None else Hpp[:, i6, i6] + np.diagonal(ex["H"])[:6 * nF].reshape(nF, 6), radius)
    S4 = np.zeros((nF, nF, 6, 6), LD); A4 = np.zeros((nF, nF, 6, 6), LD); T4 = np.zeros((nF, nF), np.int64)
    fi = np.arange(nF)
    S4[fi, fi] = Hpp; S4[fi[:, None], fi[:, None], i6[None, :], i6[None, :]] += lam_p
    A4[fi, fi] = App; A4[fi[:, None], fi[:, None], i6[None, :], i6[None, :]] += lam_p
    T4[fi, fi] = 2 * nobs_pose + 1
    b = gp.copy(); Ab = Agp.copy(); Tb = 2 * nobs_pose
    mz = act & var_pose[pose] & var_point[point]
    Hpl = np.einsum("n,nka,nkb->nab", w, Jp, Jl)                   # [n,6,3]; used where mz
    order = np.flatnonzero(mz)
    starts = np.searchsorted(point[order], np.arange(L + 1))
    for l in range(L):
        idx = order[starts[l]:starts[l + 1]]
        if not len(idx):
            continue
        f = frame[pose[idx]]
        W = Hpl[idx]
        Y = W @ Hinv[l]                                            # [k,6,3]
        np.subtract.at(S4, (f[:, None], f[None, :]), np.einsum("iab,jcb->ijac", Y, W))
        np.add.at(A4, (f[:, None], f[None, :]), np.einsum("iab,jcb->ijac", np.abs(W) @ np.abs(Hinv[l]), np.abs(W)))
        np.add.at(T4, (f[:, None], f[None, :]), 9)
        np.subtract.at(b, f, Y @ gl[l])
        np.add.at(Ab, f, (np.abs(W) @ np.abs(Hinv[l])) @ Agl[l])
        np.add.at(Tb, f, 9)
    m = 6 * nF
    S = S4.transpose(0, 2, 1, 3).reshape(m, m); A_S = A4.transpose(0, 2, 1, 3).reshape(m, m)
    bv, A_b = b.reshape(m), Ab.reshape(m)
    g_all = np.concatenate([gp.ravel(), gl[var_point].ravel()])
    n_terms = int(max(T4.max(), Tb.max()))
    if ex is not None:
        # the other families: their J^T J and J^T r over (variable poses, variable objects), the objects' damping from their own diagonal
        mp, m = m, ex["H"].shape[0]
        io = np.arange(mp, m)
        lam_o = _lm_lambda(np.diagonal(ex["H"])[mp:], radius)
        Sf, Af = ex["H"].copy(), ex["A"].copy()
        Sf[:mp, :mp] += S; Af[:mp, :mp] += A_S
        Sf[io, io] += lam_o; Af[io, io] += lam_o
        bf, Abf = ex["g"].copy(), ex["Ag"].copy()
        bf[:mp] += bv; Abf[:mp] += A_b
        Tf, Tbf = ex["T"].copy(), ex["Tg"].copy()
        Tf[:mp, :mp] += np.kron(T4, np.ones((6, 6), np.int64)); Tf[io, io] += 1
        Tbf[:mp] += np.repeat(Tb, 6)
        g_all = np.concatenate([gp.ravel() + ex["g"][:mp], ex["g"][mp:], gl[var_point].ravel()])
        S, A_S, bv, A_b, n_terms, cost = Sf, Af, bf, Abf, int(max(Tf.max(), Tbf.max())), cost + ex["cost"]
    out = dict(S=S, b=bv, A_S=A_S, A_b=A_b, n_terms=n_terms, cost=cost, gradient_max_norm=np.abs(g_all).max(), gradient_norm=np.sqrt((g_all * g_all).sum()),
               point_var=var_point, pose_var=var_pose, pivots_ok=pivots_ok, both_huber_branches=both)
    if ex is not None:
        out.update(object_var=ex["object_var"], side_branches=ex["branches"], n_pose_rows=6 * nF)
    if not want_step:
        return out
    # the step: S y = b in fp64 with iterative refinement on long double residuals; poses move by -y, points by -Hinv (g_l - sum Hpl^T y)
    import scipy.linalg
    cf = scipy.linalg.cho_factor(S.astype(np.float64))
    y = np.zeros(m, LD)
    for _ in range(40):
        d = scipy.linalg.cho_solve(cf, (bv - S @ y).astype(np.float64)).astype(LD)
        y += d
        if np.abs(d).max() <= LD(1e-17) * np.abs(y).max():
            break
    else:
        raise AssertionError("the refinement of the reference step did not converge")
    yf = y[:6 * nF].reshape(nF, 6)
    t = gl.copy()
    np.subtract.at(t, point[order], np.einsum("nab,na->nb", Hpl[order], yf[frame[pose[order]]]))
    step_point = -np.einsum("lab,lb->la", Hinv, t)
    step_point[~var_point] = 0
    step_pose = np.zeros((P, 6), LD)
    step_pose[var_pose] = -yf
    out.update(step_pose=step_pose, step_point=step_point, step_norm=np.sqrt((step_pose ** 2).sum() + (step_point ** 2).sum()))
    if ex is not None:                                                # objects move by minus their part of y
        step_object = np.zeros((len(ex["object_var"]), ex["od"]), LD)
        step_object[ex["object_var"]] = -y[6 * nF:].reshape(-1, ex["od"])
        out.update(step_object=step_object, step_norm=np.sqrt((step_pose ** 2).sum() + (step_point ** 2).sum() + (step_object ** 2).sum()))
    return out


# ------------------------------------------------------------------------------------------
# errors against the reference, on the scales the bounds are stated on
# ------------------------------------------------------------------------------------------
def entry_error(X, ref, A):
    """largest |X - ref| / A over the entries with A > 0 (A: the sum of the absolute values of all terms of the entry)"""
    nz = A > 0
    return float((np.abs(X.astype(LD)[nz] - ref[nz]) / A[nz]).max())


def exact_zeros(X, ref):
    """every entry that the reference has exactly zero is exactly zero"""
    return bool((X[ref == 0] == 0).all())


def step_errors(prob, poses, points, ref):
    """error of the new poses / points against start + reference step, relative to the largest entry of that part of the step (the addition is rounded to fp64 once
    by either implementation: that rounding is part of e(oracle) as it is of the device's error)"""
    ep = np.abs(poses.astype(LD) - (prob["poses"].astype(LD) + ref["step_pose"])).max() / np.abs(ref["step_pose"]).max()
    el = np.abs(points.astype(LD) - (prob["points"].astype(LD) + ref["step_point"])).max() / np.abs(ref["step_point"]).max()
    return float(ep), float(el)


def scalar_errors(it0, it1, ref):
    return {k: float(abs(LD(v) - ref[k]) / ref[k]) for k, v in (("cost", it0.cost), ("gradient_max_norm", it0.gradient_max_norm), ("gradient_norm", it0.gradient_norm),
                                                                 ("step_norm", it1.step_norm))}
